// TEST INFRASTRUCTURE ONLY: the fused ply's count words and pick of gc_core.h compiled for the host
// (tests/test_count_prefix.py): the makers' running-prefix words (sw_prefix_make) against
// byte_prefix of sw_pack's words, sw_locate_pre against its earlier multiply form and a scan, and
// the pick from fetched sets (sw_pick_sets: sw_locate_pre / sw_finish, the scan for 256 moves and
// more) against sw_select.
#include <cstddef>
#include <cstdint>

#include "../../gym-chess_amd/csrc/gc_core.h"
#include "../../gym-chess_amd/csrc/gc_env.h"

using namespace gc;

// the three makers' words of the 28 sets t, summed word by word; returns the sum of their totals
static u32 makers_words(const u64* t, u64* pw) {
    u64 a[4], b[4], c[4];
    u32 pa, pb, pc;
    sw_prefix_make<SW_OWN_Q0>(t, a, pa);
    sw_prefix_make<SW_OWN_Q2>(t, b, pb);
    sw_prefix_make<SW_OWN_Q3>(t, c, pc);
    for (int w = 0; w < 4; w++) pw[w] = a[w] + b[w] + c[w];
    return pa + pb + pc;
}

// sw_locate_pre as it stood before the 32-bit form: K by a 64-bit multiply, signed rank
static int locate_pre_mul(const u64* pw, int& k) {
    const u64 p0 = pw[0], p1 = pw[1], p2 = pw[2], p3 = pw[3];
    const int c1 = (int)(p0 >> 56), c2 = c1 + (int)(p1 >> 56), c3 = c2 + (int)(p2 >> 56);
    const int w = (k >= c1) + (k >= c2) + (k >= c3);
    const u64 p = w == 0 ? p0 : w == 1 ? p1 : w == 2 ? p2 : p3;
    k -= w == 0 ? 0 : w == 1 ? c1 : w == 2 ? c2 : c3;
    const u64 H = 0x8000800080008000ull, K = (u64)(k + 1) * 0x0001000100010001ull, M = 0x00FF00FF00FF00FFull;
    const int above = popc((((p & M) | H) - K) & H) + popc(((((p >> 8) & M) | H) - K) & H);
    const int b = 8 - above;
    k -= b ? (int)((p >> (8 * b - 8)) & 0xFF) : 0;
    return 8 * w + b;
}

// n cases of 28 sets, each case's total below 256.  The makers' words, summed, against
// byte_prefix of sw_pack's words bit for bit (and each maker's own words against byte_prefix of
// its own packed counts: 0 before its first set, the word's total after its last); the totals'
// sum against the sets' popcount.  Returns the number of cases that differ (first[0]: the first).
extern "C" int cp_words(const uint64_t* sets, int n, int64_t* first) {
    int bad = 0;
    for (int c = 0; c < n; c++) {
        const u64* t = reinterpret_cast<const u64*>(sets) + (size_t)c * SW_SETS;
        u64 cw[4] = {0, 0, 0, 0}, pw[4];
        sw_pack(t, 0, SW_SETS, cw);
        const u32 total = makers_words(t, pw);
        bool ok = (int)total == sw_popc(t, 0, SW_SETS);
        for (int w = 0; w < 4; w++) ok = ok && pw[w] == byte_prefix(cw[w]);
        // one maker at a time
        u64 own[4] = {0, 0, 0, 0}, mw[4];
        u32 part;
        sw_pack(t, 0, SW_ORTH, own);
        sw_prefix_make<SW_OWN_Q0>(t, mw, part);
        for (int w = 0; w < 4; w++) ok = ok && mw[w] == byte_prefix(own[w]);
        ok = ok && (int)part == sw_popc(t, 0, SW_ORTH);
        own[0] = own[1] = own[2] = own[3] = 0;
        sw_pack(t, SW_ORTH, SW_DIAG, own);
        sw_pack(t, SW_K, SW_SETS, own);
        sw_prefix_make<SW_OWN_Q2>(t, mw, part);
        for (int w = 0; w < 4; w++) ok = ok && mw[w] == byte_prefix(own[w]);
        ok = ok && (int)part == sw_popc(t, SW_ORTH, SW_DIAG) + sw_popc(t, SW_K, SW_SETS);
        own[0] = own[1] = own[2] = own[3] = 0;
        sw_pack(t, SW_DIAG, SW_K, own);
        sw_prefix_make<SW_OWN_Q3>(t, mw, part);
        for (int w = 0; w < 4; w++) ok = ok && mw[w] == byte_prefix(own[w]);
        ok = ok && (int)part == sw_popc(t, SW_DIAG, SW_K);
        if (!ok && !bad++) first[0] = c;
    }
    return bad;
}

// The same cases: for every rank below the total, sw_locate_pre on the makers' words against its
// multiply form on byte_prefix of sw_pack's words and against a scan over the sets' counts.
// Returns the number of ranks that differ (first[0..1]: case, rank); ranks[0] += the ranks compared.
extern "C" int cp_locate(const uint64_t* sets, int n, int64_t* ranks, int64_t* first) {
    int bad = 0;
    for (int c = 0; c < n; c++) {
        const u64* t = reinterpret_cast<const u64*>(sets) + (size_t)c * SW_SETS;
        u64 cw[4] = {0, 0, 0, 0}, pw[4], qw[4];
        sw_pack(t, 0, SW_SETS, cw);
        for (int w = 0; w < 4; w++) qw[w] = byte_prefix(cw[w]);
        const int total = (int)makers_words(t, pw);
        for (int k = 0; k < total; k++) {
            int k0 = k, k1 = k, k2 = k, j2 = 0;
            const int j0 = sw_locate_pre(pw, k0), j1 = locate_pre_mul(qw, k1);
            while (k2 >= popc(t[j2])) k2 -= popc(t[j2++]);
            if ((j0 != j1 || k0 != k1 || j0 != j2 || k0 != k2) && !bad++) { first[0] = c; first[1] = k; }
            ranks[0]++;
        }
    }
    return bad;
}

// One case of 28 sets with the Gen terms the pick reads (occupancy, side, castles): for every rank
// below the total (castles counted), sw_pick_sets from the makers' prefix words (PRE), from
// sw_pack's words, and with the wave's any_big flag set, against sw_select.  Totals of 256 and
// more take the scan, whatever the words hold.  acts (optional): sw_select's action per rank.
// Returns the number of ranks that differ (first[0]: the first); ranks[0] += the ranks compared.
static int pick_case(const u64* t, const Gen& g, uint16_t* acts, int64_t* ranks, int64_t* first) {
    u64 cw[4] = {0, 0, 0, 0}, pw[4];
    sw_pack(t, 0, SW_SETS, cw);
    makers_words(t, pw);
    const int tot = sw_popc(t, 0, SW_SETS) + popc(g.castles);
    const auto get = [&](int j) { return t[j]; };
    int bad = 0;
    for (int k = 0; k < tot; k++) {
        const int want = sw_select(g, t, k);
        const bool big = tot >= 256;
        const int a0 = sw_pick_sets<true>(get, g, pw, tot, k, big), a1 = sw_pick_sets<false>(get, g, cw, tot, k, big);
        const int a2 = sw_pick_sets<true>(get, g, pw, tot, k, true);
        int r = k;
        // below 256 moves: sw_finish on the located set, stated on its own
        const int a3 = big || k >= tot - popc(g.castles) ? want : [&] { const int j = sw_locate_pre(pw, r); return sw_finish(g, j, t[j], r); }();
        if ((a0 != want || a1 != want || a2 != want || a3 != want) && !bad++) first[0] = k;
        if (acts) acts[k] = (uint16_t)want;
        ranks[0]++;
    }
    return bad;
}

// the move sets of the side to move in (b, m), as the fused ply's makers generate them
extern "C" int cp_pick_board(const int8_t* b, const uint8_t* m, uint16_t* acts, int64_t* ranks, int64_t* first) {
    const u32 meta = (m[0] ? M_WHITE : 0u) | (m[1] ? M_WKC : 0u) | (m[2] ? M_WQC : 0u) | (m[3] ? M_BKC : 0u) |
                     (m[4] ? M_BQC : 0u) | (m[5] ? M_WCHK : 0u) | (m[6] ? M_BCHK : 0u) | ((u32)m[7] << M_MC_SHIFT);
    Pos s = from_mailbox(b, meta);
    s.meta = (s.meta & ~(u32)M_RIGHTS) | eff_rights(s);
    Gen g;
    gen_init(s, g);
    u64 t[SW_SETS];
    const int n = sw_gen(s, g, t);
    if (n > 255) return -1;
    first[1] = pick_case(t, g, acts, ranks, first);  // (the ranks that differ; the return is the move count)
    return n;
}

// synthetic sets (any total: 256 and more take the scan)
extern "C" int cp_pick_sets(const uint64_t* sets, uint64_t occ, int white, int castles, int64_t* ranks, int64_t* first) {
    Gen g{};
    g.occ = occ;
    g.white = white != 0;
    g.castles = (u32)castles;
    return pick_case(reinterpret_cast<const u64*>(sets), g, nullptr, ranks, first);
}
