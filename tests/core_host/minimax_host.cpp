// TEST INFRASTRUCTURE ONLY: the first half of gc_minimax.h (the recursion, the material term, the
// value mapping, the tie rule and the whole row, minimax_row -- what k_minimax computes wave-wide)
// compiled for the HOST with g++, with and without pruning.  tests/test_minimax.py pins it to a
// plain negamax over the C oracle, and tests/test_minimax_gpu.py pins the kernel to it bit for bit.
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

// One row of gc_env_minimax for (board, meta8, done) as board index `board_index`.  prune 0 runs the
// recursion full-width (every window open, no cut).  out i32[4] = count, pick, score, nodes;
// value f32[1]; actions u16[cap] / scores i32[cap] or NULL.  Returns 1 for a done board (zeros).
extern "C" int mh_row(const int8_t* board, const uint8_t* meta8, int done, int depth, int tiebreak, uint64_t seed,
                      uint32_t board_index, uint32_t draw, int prune, int cap, uint16_t* actions, int32_t* scores,
                      int32_t* out, float* value) {
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
    PlainLevels lv;
    PlainScratch rs;
    memset(&lv, 0, sizeof(lv));
    memset(&rs, 0, sizeof(rs));
    const MinimaxRow r = prune ? minimax_row<true>(s, depth, tiebreak, seed, board_index, draw, cap, actions, scores, lv, rs)
                               : minimax_row<false>(s, depth, tiebreak, seed, board_index, draw, cap, actions, scores, lv, rs);
    out[0] = r.count; out[1] = r.pick; out[2] = r.score; out[3] = (int32_t)r.nodes;
    *value = r.value;
    return 0;
}

extern "C" int mh_material(const int8_t* board, int white_to_move) {
    uint8_t m[8] = {(uint8_t)(white_to_move != 0), 0, 0, 0, 0, 0, 0, 0};
    return minimax_material(import_board(board, m, 0));
}
extern "C" float mh_value(int score) { return minimax_value(score); }
extern "C" uint32_t mh_policy_index(uint64_t seed, uint32_t board, uint32_t draw, uint32_t n) {
    return policy_index(seed, board, draw, n);
}
extern "C" int mh_big(const int8_t* board, const uint8_t* meta8) {  // more own pieces than scratch slots (ms.big)
    Gen g;
    gen_init(import_board(board, meta8, 0), g);
    return popc(g.own) > SCRATCH_SLOTS;
}
