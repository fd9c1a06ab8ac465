// TEST INFRASTRUCTURE ONLY: gc_minimax.h's first half with the quiescence nest below the leaves
// (mm_qs / mm_qedge under minimax_row, what k_minimax<NODES, true> computes wave-wide) compiled for
// the HOST with g++, with and without pruning.  quiesce 0 takes the plain levels object, as
// gc_env_minimax_q does.  tests/test_quiesce.py pins it to a plain QS / V over the C oracle, and
// tests/test_quiesce_gpu.py pins the kernel to it bit for bit.
#include <climits>
#include <cstdint>
#include <cstring>

#include "../../gym-chess_amd/csrc/gc_core.h"
#include "../../gym-chess_amd/csrc/gc_env.h"
#include "../../gym-chess_amd/csrc/gc_perft.h"
#include "../../gym-chess_amd/csrc/gc_minimax.h"

using namespace gc;

struct PlainScratch {
    static constexpr bool kPark = true;
    u64 v[SCRATCH_SLOTS];
    void put(int j, u64 x) { v[j] = x; }
    u64 get(int j) const { return v[j]; }
};
struct PlainLevels {  // one scratch object per interior level below the root
    PlainScratch l[MM_MAX_DEPTH - 1];
    template <int D>
    PlainScratch& at() {
        static_assert(D >= 1 && D < MM_MAX_DEPTH, "an interior level below the root");
        return l[D - 1];
    }
};

// a board as gc_env_set_states ingests it (k_env_import, checks = 0): the flags as given
static Pos import_board(const int8_t* b, const uint8_t* m, int done) {
    const u32 meta = (m[0] ? M_WHITE : 0u) | (m[1] ? M_WKC : 0u) | (m[2] ? M_WQC : 0u) | (m[3] ? M_BKC : 0u) |
                     (m[4] ? M_BQC : 0u) | (m[5] ? M_WCHK : 0u) | (m[6] ? M_BCHK : 0u) | ((u32)m[7] << M_MC_SHIFT) |
                     (done ? (u32)M_DONE : 0u);
    return from_mailbox(b, meta);
}

template <bool PRUNE>
static MinimaxRow row_of(const Pos& s, int depth, int quiesce, int tiebreak, uint64_t seed, uint32_t board_index,
                         uint32_t draw, int cap, uint16_t* actions, int32_t* scores) {
    PlainLevels lv;
    PlainScratch rs;
    memset(&lv, 0, sizeof(lv));
    memset(&rs, 0, sizeof(rs));
    if (!quiesce) return minimax_row<PRUNE>(s, depth, tiebreak, seed, board_index, draw, cap, actions, scores, lv, rs);
    MmQuiesce<PlainLevels> lq{lv, quiesce};
    return minimax_row<PRUNE>(s, depth, tiebreak, seed, board_index, draw, cap, actions, scores, lq, rs);
}

// One row of gc_env_minimax_q for (board, meta8, done) as board index `board_index`, quiesce in
// 0..MM_MAX_QUIESCE.  prune 0 runs the recursion full-width (every window open, no cut, no
// stand-pat return).  out i32[4] = count, pick, score, nodes; value f32[1]; actions u16[cap] /
// scores i32[cap] or NULL.  Returns 1 for a done board (zeros), -1 for a quiesce out of range.
extern "C" int qh_row(const int8_t* board, const uint8_t* meta8, int done, int depth, int quiesce, int tiebreak,
                      uint64_t seed, uint32_t board_index, uint32_t draw, int prune, int cap, uint16_t* actions,
                      int32_t* scores, int32_t* out, float* value) {
    if (quiesce < 0 || quiesce > MM_MAX_QUIESCE || depth < 1 || depth > MM_MAX_DEPTH) return -1;
    const Pos s = import_board(board, meta8, done);
    if (s.meta & M_DONE) {
        for (int k = 0; k < cap; k++) {
            if (actions) actions[k] = 0xFFFF;
            if (scores) scores[k] = INT32_MIN;
        }
        out[0] = 0; out[1] = A_NONE; out[2] = 0; out[3] = 0;
        *value = 0.0f;
        return 1;
    }
    const MinimaxRow r = prune ? row_of<true>(s, depth, quiesce, tiebreak, seed, board_index, draw, cap, actions, scores)
                               : row_of<false>(s, depth, quiesce, tiebreak, seed, board_index, draw, cap, actions, scores);
    out[0] = r.count; out[1] = r.pick; out[2] = r.score; out[3] = (int32_t)r.nodes;
    *value = r.value;
    return 0;
}

extern "C" uint32_t qh_policy_index(uint64_t seed, uint32_t board, uint32_t draw, uint32_t n) {
    return policy_index(seed, board, draw, n);
}
extern "C" int qh_max_quiesce() { return MM_MAX_QUIESCE; }
