// TEST INFRASTRUCTURE ONLY: the two halves of the branch-free apply (gc_core.h apply_legal_krw,
// apply_legal_qbnp: the fused ply runs them on two waves) against apply_legal, compiled for the
// host (tests/test_apply_split.py).
#include <cstdint>

#include "../../gym-chess_amd/csrc/gc_core.h"
#include "../../gym-chess_amd/csrc/gc_env.h"

using namespace gc;

enum {
    C_KSW, C_QSW, C_KSB, C_QSB,                 // castles
    C_CAP_Q, C_CAP_R, C_CAP_B, C_CAP_N, C_CAP_P,  // captures by the captured piece's type
    C_WKING,                                    // a white king moves (both white rights revoked)
    C_WROOK_A, C_WROOK_H,                       // a white rook leaves column 0 / 7, the right still set
    C_PAWN,                                     // pawn moves
    C_MOVES,
    C_N
};

// n legal actions of the side to move in (b, m): every one applied by apply_legal and by the two
// halves, each half on its own copy of the position as its wave holds it.  Returns the number of
// actions whose results differ (the first one's index and differing parts in first[0..1]: bit 0-6
// the bitboards k q r b n p w, 7 the meta word, 8 the reward, 9 irrev, 10 a half wrote a member
// that is not its own); counts[C_N] += the cases met.
extern "C" int as_compare(const int8_t* b, const uint8_t* m, const uint16_t* acts, int n, int64_t* counts,
                          int64_t* first) {
    const bool white = m[0] != 0;
    u32 meta = (white ? M_WHITE : 0u) | (m[1] ? M_WKC : 0u) | (m[2] ? M_WQC : 0u) | (m[3] ? M_BKC : 0u) |
               (m[4] ? M_BQC : 0u) | (m[5] ? M_WCHK : 0u) | (m[6] ? M_BCHK : 0u) | ((u32)m[7] << M_MC_SHIFT);
    Pos s = from_mailbox(b, meta);
    s.meta = (s.meta & ~(u32)M_RIGHTS) | eff_rights(s);
    int bad = 0;
    for (int j = 0; j < n; j++) {
        const int a = acts[j];
        Pos ref = s, h0 = s, h1 = s;
        int rw = -1, rw1 = -1;
        bool ir = false, ir1 = false;
        apply_legal(ref, white, a, &rw, &ir);
        apply_legal_krw(h0, a, s.k & s.w, s.r & s.w);
        apply_legal_qbnp(h1, a, &rw1, &ir1, occ_of(s));
        unsigned d = 0;
        d |= (h0.k != ref.k) << 0;
        d |= (h1.q != ref.q) << 1;
        d |= (h0.r != ref.r) << 2;
        d |= (h1.b != ref.b) << 3;
        d |= (h1.n != ref.n) << 4;
        d |= (h1.p != ref.p) << 5;
        d |= (h0.w != ref.w) << 6;
        d |= (h0.meta != ref.meta) << 7;
        d |= (rw1 != rw) << 8;
        d |= (ir1 != ir) << 9;
        d |= (h0.q != s.q || h0.b != s.b || h0.n != s.n || h0.p != s.p || h1.k != s.k || h1.r != s.r || h1.w != s.w ||
              h1.meta != s.meta) << 10;
        if (d && !bad++) { first[0] = j; first[1] = d; }
        counts[C_MOVES]++;
        if (a >= 4096) {
            counts[a == A_KSW ? C_KSW : a == A_QSW ? C_QSW : a == A_KSB ? C_KSB : C_QSB]++;
            continue;
        }
        const int f = a >> 6, t = a & 63;
        const int ct = type_at(s, t);
        if (ct == QUEEN) counts[C_CAP_Q]++;
        if (ct == ROOK) counts[C_CAP_R]++;
        if (ct == BISHOP) counts[C_CAP_B]++;
        if (ct == KNIGHT) counts[C_CAP_N]++;
        if (ct == PAWN) counts[C_CAP_P]++;
        const int id = id_at(s, f);
        if (id == KING) counts[C_WKING]++;
        if (id == ROOK && (f & 7) == 0 && (s.meta & M_WQC)) counts[C_WROOK_A]++;
        if (id == ROOK && (f & 7) == 7 && (s.meta & M_WKC)) counts[C_WROOK_H]++;
        if (id == PAWN || id == -PAWN) counts[C_PAWN]++;
    }
    return bad;
}
