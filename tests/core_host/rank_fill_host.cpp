// TEST INFRASTRUCTURE ONLY: the carry-propagation rank fills of gc_core.h against the
// Kogge-Stone templates they replace along a rank, compiled for the host (tests/test_rank_fill.py).
#include <cstdint>

#include "../../gym-chess_amd/csrc/gc_core.h"
#include "../../gym-chess_amd/csrc/gc_env.h"

using namespace gc;

// all forms of one case: bit k of the result is set where form k differs from its reference
//   0 att east   1 att west   2 to east   3 to west   4/5 pair east (ge / go)   6/7 pair west
//   8/9 att with shared operands (RankOcc) east / west, 10/11 to with shared operands
static unsigned diff_one(u64 occ, u64 ge, u64 go, u64 tm) {
    const u64 empty = ~occ;
    const u64 ke = ray_fill_att<1, true>(ge, empty, ~FILE_A), kw = ray_fill_att<1, false>(ge, empty, ~FILE_H);
    const u64 koe = ray_fill_att<1, true>(go, empty, ~FILE_A), kow = ray_fill_att<1, false>(go, empty, ~FILE_H);
    const RankOcc R = rank_occ(occ);
    unsigned d = 0;
    d |= (rank_fill_att<true>(ge, occ) != ke) << 0;
    d |= (rank_fill_att<false>(ge, occ) != kw) << 1;
    d |= (rank_fill_to<true>(ge, occ, tm) != ray_fill_to<1, true>(ge, empty, ~FILE_A, tm)) << 2;
    d |= (rank_fill_to<false>(ge, occ, tm) != ray_fill_to<1, false>(ge, empty, ~FILE_H, tm)) << 3;
    u64 ae, ao, re, ro;
    rank_fill_pair<true>(ge, go, R, ae, ao);
    ray_fill_pair<1, true>(ge, go, empty, ~FILE_A, re, ro);
    d |= (ae != re || ae != ke) << 4;
    d |= (ao != ro || ao != koe) << 5;
    rank_fill_pair<false>(ge, go, R, ae, ao);
    ray_fill_pair<1, false>(ge, go, empty, ~FILE_H, re, ro);
    d |= (ae != re || ae != kw) << 6;
    d |= (ao != ro || ao != kow) << 7;
    d |= (rank_fill_att<true>(go, R) != koe) << 8;
    d |= (rank_fill_att<false>(go, R) != kow) << 9;
    d |= (rank_fill_to<true>(go, R, tm) != (koe & tm)) << 10;
    d |= (rank_fill_to<false>(go, R, tm) != (kow & tm)) << 11;
    return d;
}

// n cases (go[i] and ge[i] within occ[i]); returns the number that differ, the first one's
// index and form bits in first[0..1]
extern "C" int rf_compare(const uint64_t* occ, const uint64_t* ge, const uint64_t* go, const uint64_t* tm, int n,
                          int64_t* first) {
    int bad = 0;
    for (int i = 0; i < n; i++) {
        const unsigned d = diff_one(occ[i], ge[i], go[i], tm[i]);
        if (d && !bad++) { first[0] = i; first[1] = d; }
    }
    return bad;
}

// out: {new east, new west, Kogge-Stone east, Kogge-Stone west} attack fills of one case
extern "C" void rf_eval(uint64_t occ, uint64_t gen, uint64_t* out) {
    out[0] = rank_fill_att<true>(gen, occ);
    out[1] = rank_fill_att<false>(gen, occ);
    out[2] = ray_fill_att<1, true>(gen, ~occ, ~FILE_A);
    out[3] = ray_fill_att<1, false>(gen, ~occ, ~FILE_H);
}

// ---- whole positions: the converted callers against the same expressions with the
// Kogge-Stone templates in all eight directions (what they were before the rank fills)
static u64 ks_attacks_orth(const Pos& s, bool white) {
    const u64 occ = occ_of(s), empty = ~occ;
    const u64 rq = (s.r | s.q) & (white ? s.w : (occ & ~s.w));
    return ray_fill_att<8, false>(rq, empty, ~0ull) | ray_fill_att<8, true>(rq, empty, ~0ull) |
           ray_fill_att<1, true>(rq, empty, ~FILE_A) | ray_fill_att<1, false>(rq, empty, ~FILE_H);
}
static void ks_sw_orth(const Pos& s, const Gen& g, u64* t) {
    const SliderGens G = slider_gens(s, g);
    const u64 empty = ~g.occ, tm = ~g.own & g.checkmask;
    t[0] = ray_fill_to<8, false>(G.f, empty, ~0ull, tm);
    t[1] = ray_fill_to<8, true>(G.f, empty, ~0ull, tm);
    t[2] = ray_fill_to<1, true>(G.r, empty, ~FILE_A, tm);
    t[3] = ray_fill_to<1, false>(G.r, empty, ~FILE_H, tm);
}
static int ks_count_sliders(const Pos& s, const Gen& g) {
    const SliderGens G = slider_gens(s, g);
    const u64 empty = ~g.occ, tm = ~g.own & g.checkmask;
    return ray_count<8, false>(G.f, empty, ~0ull, tm) + ray_count<8, true>(G.f, empty, ~0ull, tm) +
           ray_count<1, true>(G.r, empty, ~FILE_A, tm) + ray_count<1, false>(G.r, empty, ~FILE_H, tm) +
           ray_count<7, false>(G.a, empty, ~FILE_A, tm) + ray_count<9, false>(G.d, empty, ~FILE_H, tm) +
           ray_count<9, true>(G.d, empty, ~FILE_A, tm) + ray_count<7, true>(G.a, empty, ~FILE_H, tm);
}
// 0 if the position's orthogonal attack maps (both sides), orthogonal move sets, carried-operand
// forms and move counts agree with the Kogge-Stone forms; else a bit per failing check.
// *count: count_moves' total (the test compares it with the oracle's list length)
extern "C" int rf_position(const int8_t* b, const uint8_t* m, int white, int* count) {
    u32 meta = (white ? M_WHITE : 0u) | (m[1] ? M_WKC : 0u) | (m[2] ? M_WQC : 0u) | (m[3] ? M_BKC : 0u) |
               (m[4] ? M_BQC : 0u) | (m[5] ? M_WCHK : 0u) | (m[6] ? M_BCHK : 0u) | ((u32)m[7] << M_MC_SHIFT);
    Pos s = from_mailbox(b, meta);
    s.meta = (s.meta & ~(u32)M_RIGHTS) | eff_rights(s);
    Gen g;
    gen_init(s, g);
    int bad = 0;
    const OrthCarry oc = orth_carry(g.occ);
    const DiagCarry dc = diag_carry(g.occ);
    for (int w = 0; w < 2; w++) {
        bad |= (side_attacks_orth(s, w != 0) != ks_attacks_orth(s, w != 0)) << 0;
        bad |= (side_attacks_orth(s, w != 0, oc) != ks_attacks_orth(s, w != 0)) << 1;
        bad |= (side_attacks_diag(s, w != 0, dc) != side_attacks_diag(s, w != 0)) << 2;
    }
    u64 t[SW_SETS] = {0}, tc[SW_SETS] = {0}, k[4];
    sw_orth(s, g, t);
    sw_orth(s, g, oc, tc);
    ks_sw_orth(s, g, k);
    for (int j = 0; j < 4; j++) bad |= (t[SW_ORTH + j] != k[j] || tc[SW_ORTH + j] != k[j]) << 3;
    sw_diag(s, g, t);
    sw_diag(s, g, dc, tc);
    for (int j = 0; j < 4; j++) bad |= (t[SW_DIAG + j] != tc[SW_DIAG + j]) << 4;
    const int c = count_moves(s, g);
    bad |= (c != count_nonsliders(s, g) + ks_count_sliders(s, g)) << 5;
    bad |= (c != count_position(s) || c != count_legal(s, g)) << 6;
    *count = c;
    return bad;
}
