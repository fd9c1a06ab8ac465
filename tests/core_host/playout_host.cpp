// TEST INFRASTRUCTURE ONLY: the playout body of gc_playout.h (playout_lane, playout_material,
// playout_value -- what k_playout runs per lane and per row) compiled for the HOST with g++, the
// private 3-fold window as a plain array.  tests/test_playout.py pins it to the C oracle, and
// tests/test_playout_gpu.py pins the kernel to it bit for bit.
#include <cstdint>
#include <cstring>

#include "../../gym-chess_amd/csrc/gc_core.h"
#include "../../gym-chess_amd/csrc/gc_env.h"
#include "../../gym-chess_amd/csrc/gc_playout.h"

using namespace gc;

struct PlainHist {  // PlayHist's contract on a plain array: no spill table, immediate stores
    RepEntry tab[1 << PLAY_BITS];
    u32 g = 0;
    PlainHist() { memset(tab, 0, sizeof(tab)); }
    int bits() const { return PLAY_BITS; }
    u32 gen() const { return g; }
    void bump_gen() { g++; }
    RepEntry load(int p) const { return tab[p]; }
    void store_hdr(int p, u64 h) { tab[p].hdr = h; }
    void store(int p, const RepEntry& e) { tab[p] = e; }
    void commit() {}
    u32 spill_mask() const { return 0; }
    u32 owner() const { return 0; }
    u64 sp_hdr(u32) const { return 0; }
    bool sp_cas(u32, u64&, u64) { return false; }
    void sp_set_hdr(u32, u64) {}
    void sp_put(u32, const Pos&) {}
    bool sp_same(u32, const Pos&) const { return false; }
    u32 sp_owner_gen(u32) const { return g; }
    void sp_claimed() {}
    void sp_fail() {}
};

struct PlainScratch {
    static constexpr bool kPark = true;
    u64 v[SCRATCH_SLOTS];
    void put(int j, u64 x) { v[j] = x; }
    u64 get(int j) const { return v[j]; }
};

// a board as gc_env_set_states ingests it (k_env_import, checks = 0): the flags as given,
// meta8[7] = move_count; `done` = the env's done flag
static Pos import_board(const int8_t* b, const uint8_t* m, int done) {
    const u32 meta = (m[0] ? M_WHITE : 0u) | (m[1] ? M_WKC : 0u) | (m[2] ? M_WQC : 0u) | (m[3] ? M_BKC : 0u) |
                     (m[4] ? M_BQC : 0u) | (m[5] ? M_WCHK : 0u) | (m[6] ? M_BCHK : 0u) | ((u32)m[7] << M_MC_SHIFT) |
                     (done ? (u32)M_DONE : 0u);
    return from_mailbox(b, meta);
}

struct Trace {
    int32_t* act;
    uint8_t* why;
    void operator()(int ply, int a, int reason) const {
        if (act) act[ply] = a;
        if (why) why[ply] = (uint8_t)reason;
    }
};

// One row of gc_playout_run: P playouts of n_plies plies from (board, meta8, done) on the lanes
// lane0 .. lane0 + P - 1 of the stream (seed, lane, draw + ply).
// actions i32 [P][n_plies] (-1 past the end), reasons u8 [P][n_plies], ends i32 [P][3] = kind,
// plies, m (any of the three may be NULL); tally i32 [6], value f32 [1] as the kernel writes them.
// Returns 1 for a skipped row (a done board: zeros), else 0.
extern "C" int ph_row(const int8_t* board, const uint8_t* meta8, int done, uint64_t seed, uint32_t lane0, int P,
                      uint32_t draw, int n_plies, float cut_weight, int32_t* actions, uint8_t* reasons, int32_t* ends,
                      int32_t* tally, float* value) {
    Pos s0 = import_board(board, meta8, done);
    int t[PLAYOUT_TALLY] = {0, 0, 0, 0, 0, 0};
    const bool skip = (s0.meta & M_DONE) != 0;
    for (int p = 0; p < P; p++) {
        int32_t* act = actions ? actions + (size_t)p * n_plies : nullptr;
        uint8_t* why = reasons ? reasons + (size_t)p * n_plies : nullptr;
        for (int k = 0; k < n_plies; k++) {
            if (act) act[k] = -1;
            if (why) why[k] = 0;
        }
        PlayoutEnd r = {PO_OTHER, 0, 0};
        if (!skip) {
            PlainHist h;
            PlainScratch scr;
            h.bump_gen();  // zeroed entries are of generation 0: dead
            Pos s = s0;
            s.meta = with_hl(s.meta, 0);
            PolicyCtx pc = {seed, lane0 + (u32)p, draw};
            r = playout_lane(s, h, scr, pc, n_plies, true, PlayoutOneLane{}, Trace{act, why});
            t[r.kind]++;
            t[4] += r.m;
            t[5] += r.plies;
        }
        if (ends) { ends[3 * p] = r.kind; ends[3 * p + 1] = r.plies; ends[3 * p + 2] = r.m; }
    }
    for (int k = 0; k < PLAYOUT_TALLY; k++) tally[k] = t[k];
    *value = playout_value(t[0], t[1], t[4], cut_weight, P);
    return skip ? 1 : 0;
}

extern "C" int ph_material(const int8_t* board, int own_white) {
    uint8_t m[8] = {0};
    return playout_material(import_board(board, m, 0), own_white != 0);
}
extern "C" float ph_value(int wins, int losses, int msum, float cut_weight, int P) {
    return playout_value(wins, losses, msum, cut_weight, P);
}
extern "C" int ph_table_bits() { return PLAY_BITS; }
