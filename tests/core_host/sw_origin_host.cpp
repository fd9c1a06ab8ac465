// TEST INFRASTRUCTURE ONLY: the pick's tail of gc_core.h compiled for the host
// (tests/test_sw_origin.py): sw_origin over arrays of cases, the prefix form of sw_locate against
// the form that takes the count words, and the apply's forms without the castle terms against
// apply_legal.
#include <cstddef>
#include <cstdint>

#include "../../gym-chess_amd/csrc/gc_core.h"
#include "../../gym-chess_amd/csrc/gc_env.h"

using namespace gc;

// out[i] = sw_origin of set j[i] and target to[i] on the occupancy occ[i] for the side white[i]
extern "C" void so_origin(const uint64_t* occ, const uint8_t* white, const int32_t* j, const int32_t* to, int n,
                          int32_t* out) {
    for (int i = 0; i < n; i++) {
        Gen g{};
        g.occ = occ[i];
        g.white = white[i] != 0;
        out[i] = sw_origin(g, j[i], to[i]);
    }
}

// The makers of the fused ply's count words (gc_quad.h quad_ply): Q0 the pawn and knight sets,
// Q2 the rook / queen and king sets, Q3 the bishop / queen sets.
static int maker_of(int set) { return set < SW_ORTH ? 0 : set < SW_DIAG ? 1 : set < SW_K ? 2 : 1; }

// n cases of 28 counts (one byte per set, each case's total below 256).  Every maker packs its own
// sets' counts, takes the byte prefixes of its words, and the prefixes are summed word by word;
// sw_locate_pre on the sums against sw_locate on the OR of the packed words, and both against a
// scan over the counts, for every rank below the total.  Returns the number of ranks that differ
// (first[0..1]: the first one's case and rank); ranks[0] += the ranks compared.
extern "C" int so_locate(const uint8_t* counts, int n, int64_t* ranks, int64_t* first) {
    int bad = 0;
    for (int c = 0; c < n; c++) {
        const uint8_t* cnt = counts + (size_t)c * SW_SETS;
        u64 mw[3][4] = {}, cw[4] = {}, pw[4] = {};
        int total = 0;
        for (int s = 0; s < SW_SETS; s++) {
            mw[maker_of(s)][s >> 3] |= (u64)cnt[s] << (8 * (s & 7));
            total += cnt[s];
        }
        for (int w = 0; w < 4; w++)
            for (int m = 0; m < 3; m++) {
                cw[w] |= mw[m][w];
                pw[w] += byte_prefix(mw[m][w]);
            }
        for (int k = 0; k < total; k++) {
            int k0 = k, k1 = k, k2 = k, j2 = 0;
            const int j0 = sw_locate(cw, k0), j1 = sw_locate_pre(pw, k1);
            while (k2 >= cnt[j2]) k2 -= cnt[j2++];
            if ((j0 != j1 || k0 != k1 || j1 != j2 || k1 != k2) && !bad++) { first[0] = c; first[1] = k; }
            ranks[0]++;
        }
    }
    return bad;
}

// n actions of the side to move in (b, m), none of them a castle: apply_legal against the forms
// without the castle terms (apply_legal_with<false>, and the halves apply_legal_krw<false> /
// apply_legal_qbnp<false> each on its own copy).  Returns the number of actions whose results
// differ (first[0]: the first one's index).
extern "C" int so_apply_plain(const int8_t* b, const uint8_t* m, const uint16_t* acts, int n, int64_t* first) {
    const bool white = m[0] != 0;
    u32 meta = (white ? M_WHITE : 0u) | (m[1] ? M_WKC : 0u) | (m[2] ? M_WQC : 0u) | (m[3] ? M_BKC : 0u) |
               (m[4] ? M_BQC : 0u) | (m[5] ? M_WCHK : 0u) | (m[6] ? M_BCHK : 0u) | ((u32)m[7] << M_MC_SHIFT);
    Pos s = from_mailbox(b, meta);
    s.meta = (s.meta & ~(u32)M_RIGHTS) | eff_rights(s);
    int bad = 0;
    for (int j = 0; j < n; j++) {
        const int a = acts[j];
        if (a >= 4096) return -1;
        Pos ref = s, one = s, h0 = s, h1 = s;
        int rw = -1, rw1 = -1, rw2 = -1;
        bool ir = false, ir1 = false, ir2 = false;
        apply_legal(ref, white, a, &rw, &ir);
        apply_legal_with<false>(one, white, a, &rw1, &ir1, occ_of(s), s.k & s.w, s.r & s.w);
        apply_legal_krw<false>(h0, a, s.k & s.w, s.r & s.w);
        apply_legal_qbnp<false>(h1, a, &rw2, &ir2, occ_of(s));
        const bool same = one.k == ref.k && one.q == ref.q && one.r == ref.r && one.b == ref.b && one.n == ref.n &&
                          one.p == ref.p && one.w == ref.w && one.meta == ref.meta && rw1 == rw && ir1 == ir &&
                          h0.k == ref.k && h0.r == ref.r && h0.w == ref.w && h0.meta == ref.meta && h1.q == ref.q &&
                          h1.b == ref.b && h1.n == ref.n && h1.p == ref.p && rw2 == rw && ir2 == ir;
        if (!same && !bad++) first[0] = j;
    }
    return bad;
}
