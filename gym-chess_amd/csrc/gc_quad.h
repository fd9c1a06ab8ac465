// gc_quad.h -- the fused quad ply, four waves per 64 boards: quad_ply, the headline rollout
// k_env_rollout4 and the one-wave k_env_rollout.  Included by gymchess.hip after the paired
// step (PairCtx, PairIO) and before the single-board env ops.
#pragma once

// ----------------------------------------------------------------------------- quad step
// k_env_rollout4: the headline rollout (opponent "none", reference rules, move-set order) with
// FOUR waves per 64 boards.  With two (k_env_rollout2) a SIMD holds 2 waves -- all 65 536
// boards give -- and a wave's ply is one long dependency chain: a lone wave runs its ply in
// 3.75 us, two share the SIMD at 6.0 us each (tools/pstamp_probe.py), VALU issue ~35 % busy.
// The ply's parallel parts -- the enemy map's three parts, the own slider sets' two halves --
// go to their own waves, so each wave's chain is shorter and a SIMD holds four of them:
//
//   phase 0   Q0: applies the action (the last ply's pick) to kings, rooks, colours, the meta word
//             Q1: applies it to the other four boards; the capture's value, the irreversible flag
//             Q3: checks the Philox word made ahead against the settled draw counter
//   phase 1   Q0: checkers, check mask, pins                   Q1: the mover's own check flag
//             Q2: enemy leaper + orthogonal slider attacks     Q3: enemy diagonal slider attacks
//   phase 2   Q0: castles, pawn and knight sets                Q1: the 3-fold commit
//             Q2: the own rook/queen direction sets, king sets Q3: the bishop/queen ones
//   phase 3   Q0: the outcome                                  Q1: the outcome, the stores, the
//             Q2: the pick of the next action                      next ply's window probe
//             Q3: the next ply's Philox word and reset table read, on the draw counter's usual step
//
// Phase 0 is the interval a quad runs on one wave's chain, so it is cut three ways: Q0 and Q1 both
// resolve the action and each applies it to the boards of its half (gc_core.h apply_legal_krw,
// apply_legal_qbnp; the halves cross in LDS after the barrier), and the Philox chain runs on Q3
// while it waits for the ply's last barrier.  The draw counter steps on every ply but the one
// after which the next side has no move (the stalemate: the driver's no-move reset follows);
// Q0 publishes the settled counter before that barrier and Q3 makes the wave's words again where
// a lane's differs -- exact, tests/test_philox_ahead_gpu.py.  With two quads per workgroup (the
// short launches) phase 0 stays as it was: all of the apply on Q0, the word on Q1 (S0 below).
//
// Q0 and Q1 carry the board's state between plies; Q2 and Q3 are stateless (the post-move
// board and the pins come through LDS) and compute their sets unconditionally -- ignored,
// like the totals, when no generation is due.  Same decisions in the same order as
// pair_ply (and so as k_env_step<true, false> and the oracle): tests/test_gpu_parity.py and
// tests/test_full_size.py run the fused rollouts against the oracle and the launched kernel.
//
// Geometry (k_env_rollout4<OCC, QW>, QW quads per workgroup).  The four barriers of a ply wait
// for a workgroup's waves, and two quads share no data, so a quad is a workgroup of its own
// (QW = ROLL_QUADS_WG = 1: 256 threads, 34 KB of LDS, four workgroups per CU) and waits only
// for its own slowest role: 9 900 vs 10 330 cycles per ply by stamps.  Every SIMD then hosts
// all four roles, one of each workgroup of its CU (the dispatcher's placement: see the role
// map in the kernel), and the four take weighted turns (ROLL_TURNS).  Twice the workgroups
// cost a short launch more than the ply gains, so launches below ROLL_SPLIT_MIN_PLIES
// (gc_host_env.h) keep QW = QUADS_WG = 2, where every SIMD hosts a state-carrying and a
// stateless role of each workgroup.  tests/test_rollout_geometry_gpu.py runs both at 1-6
// workgroups.
#define QUAD_BOARDS 64
#ifndef QUADS_WG
#define QUADS_WG 2  // the API steps: two quads per workgroup; the second's roles rotated by 2 so that
                    // every SIMD hosts a state-carrying and a stateless role of each workgroup
#endif
#ifndef GC_QXOR
#define GC_QXOR 2  // the roles of an API step workgroup's second quad: SIMD s holds roles s and s ^ GC_QXOR
#endif
#define ROLL_QUADS_WG 1  // the rollout (k_env_rollout4<OCC, ROLL_QUADS_WG>): one quad per workgroup, four
                         // workgroups per CU; launches too short to pay for twice the workgroups keep
                         // the paired form <OCC, QUADS_WG> (gc_host_env.h roll_quads_wg)
// The 3-fold window's occupancy in LDS (k_env_rollout4<true>; Q1's, a bit per table slot: 64 B per board).
// The table is open-addressed with linear probing and entries leave it only all at once (a
// generation bump), so a board whose home slot is free is not in the window -- its probe would
// stop at once and insert there.  While a board's bitmap mirrors its window (OccQ::valid: since the
// window was last emptied inside this launch -- a reset or an irreversible move), Q1 tests the
// next board's home slot in LDS and loads nothing when it is free (~80 % of plies: the window is
// short and a repetition is rare); a taken home slot (the board again, or another on its slot)
// is probed in the table as before, and so is every board of a window that predates the launch.
// Exact: the fast path makes the same decision rep_commit makes on a free first probe.  It
// removes the probe's line from most plies (the window's bytes).  Where the
// work goes (tools/pstamp_probe.py: the ply's chain is Q2's, phases 1-3): the bitmap is cleared
// and the next board looked up in phase 1 (Q1 computes only the mover's check flag there), this
// ply's entry is added in phase 2 beside the commit; in phase 3 every lane issues ONE load as
// before -- a slow lane its home entry, a fast lane the env's init block, one line that every
// lane of the chip reads (it stays in L2) -- so the registers merge no loaded data and the wait
// stays at phase 2's commit; the fast lane's header is replaced after it.  (v1, all of it in
// phase 3: Q1's phase 3 2 589 vs 1 447 cycles, -5 % at K = 1 000; v2, a load issued only by the
// slow lanes: the merge of the loaded registers waited for it at the end of phase 3.)

struct QuadLds {
    u64 sets[SW_SETS][QUAD_BOARDS];  // the next side's move sets (Q0: pawns / knights, Q2, Q3)
    u64 ns[NBB][QUAD_BOARDS];        // Q0 (k, r, w), Q1 (q, b, n, p) -> all: the post-move board (phase 0)
    u32 nmeta[QUAD_BOARDS];          //           (two quads per workgroup: all of it Q0's)
    int32_t mr[QUAD_BOARDS];         // Q0 -> Q1, two quads per workgroup: its capture reward
    u32 irrev[QUAD_BOARDS];          //           irreversible move
    u64 pin3[3][QUAD_BOARDS];        // Q0 -> Q2, Q3: check mask, pinned, pin rays
    u32 f0[QUAD_BOARDS];             // Q0 -> Q1: the side to move is in check
    u64 enemy[3][QUAD_BOARDS];       // Q2 / Q3 -> Q0, Q2: the enemy map's leaper + orthogonal ([1]), diagonal ([2]) parts
    u32 f1[QUAD_BOARDS];             // Q1 -> Q0: the mover is in check after its move
    // the sets' byte counts (gc_core.h sw_pack: set i in byte i % 8 of word i / 8) reach Q2 as
    // byte prefixes of the words a maker owns, made as running sums (sw_prefix_make); prefixes of
    // disjoint bytes add
    u64 cw3[QUAD_BOARDS];            // Q3 -> Q2: word 2 (the bishop / queen sets)
    u64 cw0[2][QUAD_BOARDS];         // Q0 -> Q2: words 0, 1 (pawns, knights)
    u32 part[4][QUAD_BOARDS];        // partial move totals (Q0's holds the castles)
    u32 rep[QUAD_BOARDS];            // Q1 -> Q0: 3-fold count | window length << 8
    u32 x0[QUAD_BOARDS];             // Q3 (two quads per workgroup: Q1) -> Q2: the Philox word of the next draw
    u32 ra[QUAD_BOARDS];             // Q3 -> Q0, Q1 (Q1 -> Q0): the start-position table pick
    u32 act[QUAD_BOARDS];            // Q0 -> Q1, two quads per workgroup: this ply's action (phase 0)
    u32 pick[QUAD_BOARDS];           // Q2 -> Q0: the policy's pick from this ply's move sets (phase 3)
    u32 d[QUAD_BOARDS];              // Q0 -> Q3: the settled draw counter (phase 3)
    u32 castles[QUAD_BOARDS];        // Q0 -> Q2: the castles (phase 2)
    u64 occ[HTAB / 64][QUAD_BOARDS];  // (OCC) Q1: the window's taken table slots, a bit per slot
    u32 nkey[QUAD_BOARDS];            // (OCC) Q1, phase 1 -> 3: the next board's key if the move stands
    u32 rkey0;                        // (OCC) the reset position's key
    Pos rp;                          // the reset position (read at a reset: no registers held for it)
};
// one set of the next side's moves into LDS, its count into the packed byte counts and the total
template <class LT>
struct QuadSetsT {
    LT& L;
    int l;
    u64 cw[4];
    int part;
    __device__ void put(int j, u64 t) {
        L.sets[j][l] = t;
        const int c = popc(t);
        cw[j >> 3] |= (u64)c << (8 * (j & 7));
        part += c;
    }
    template <int LO, int HI>
    __device__ void put_all(const u64* t) {
#pragma unroll
        for (int j = LO; j < HI; j++) put(j, t[j - LO]);
    }
};
// (the API step's makers, ApiQuadVsLds; the rollout's hand over byte prefixes: quad_put below)
// sets LO .. HI - 1 of t into LDS
template <int LO, int HI>
__device__ __forceinline__ void quad_put(QuadLds& L, int l, const u64* t) {
#pragma unroll
    for (int j = LO; j < HI; j++) L.sets[j][l] = t[j];
}

// Q0's choice of the next action, left for the start of the next ply: Q2 makes the pick from
// the move sets in phase 3 while Q0 and Q1 settle the outcome (the pick was phase 3's longest
// chain); a board that resets takes the start position's table pick instead.
struct QuadPend {
    bool have;     // the move stood: Q2's pick
    uint16_t ra;   // else: the table pick (the launch's first ply: the env's action)
    __device__ int resolve(const QuadLds& L, int l) const {
        // read whether taken or not: one ds_read and a select (pinned: left to itself the compiler
        // sinks the read into an exec region of the lanes that take it)
        u32 pk = L.pick[l];
        pin(pk);
        return have ? (int)pk : (int)ra;
    }
};
// Q0: what the apply needs of the settled state alone, made at the end of phase 3 and held
// across barrier D: the meta word with the rights State::new sees, the occupancy
// (irreversible move), the white kings and rooks (rights revoked)
struct QuadQ0Pre {
    u32 meta0;
    u64 occ, kw, rw;
};
// (S0, quad_ply's short phase 0: the occupancy is then Q1's to hold, for its half of the apply)
template <bool S0>
__device__ __forceinline__ QuadQ0Pre quad_q0pre(const Pos& s) {
    QuadQ0Pre q{(s.meta & ~(u32)M_RIGHTS) | eff_rights(s), S0 ? 0ull : occ_of(s), s.k & s.w, s.r & s.w};
    pin(q.meta0); pin(q.kw); pin(q.rw);
    if (!S0) pin(q.occ);
    return q;
}
// Q1's half of the apply needs the occupancy alone
__device__ __forceinline__ QuadQ0Pre quad_q1pre(const Pos& s) {
    QuadQ0Pre q{0u, occ_of(s), 0ull, 0ull};
    pin(q.occ);
    return q;
}
// Q3: the draw's Philox word and the reset table's pick, made a ply ahead
struct QuadAhead {
    u32 x0, ra;
};
__device__ __forceinline__ void quad_ahead(const PairCtx& C, int i, u32 d, QuadAhead& ah) {
    ah.x0 = philox_x0(C.seed, (u32)i, d);
    ah.ra = C.rtable ? (u32)C.racts[scale_rank(ah.x0, C.rtotal)] : (u32)(uint16_t)A_NONE;
}

// One ply of board i for role R of its quad (RoleC<0..3>).  Q0 / Q1: in/out as pair_ply (s, a,
// d, h, nst); both return the same s and a.  Q2 / Q3: s, a, d, h, nst unused.  oq (Q1, OCC):
// the occupancy bitmap mirrors the window (valid), and is to be cleared before use (clr: a reset)
struct OccQ {
    bool valid;  // the bitmap mirrors the window
    bool clr;    // it is to be cleared first (the window was emptied: a reset, an irreversible move)
    bool probe;  // the next board, if the move stands, is probed in the table
    bool fast;   // the probe in flight is the init block's line: its header reads as a free slot
};
// (Two quads per workgroup; one: ROLL_TURNS below.)  The two workgroups of a CU (blocks b and
// b + half: tools/pstamp_probe.py reads each wave's HW_ID) start together on the same SIMDs, and at equal priority the SQ issues the older wave
// first -- so block b ran its plies at 4.21 us and block b + half at 5.01 (every CU; same roles on
// every SIMD), and the launch ended with the later ones.  They take turns instead: for turns of
// GC_TURN_SHIFT (below) plies one workgroup's roles run one level above the other's (s_setprio 3 /
// 1 over 2 / 0).  One-ply turns: 0.14 us apart, the launch 4 858 vs 5 636 us by stamps; same box
// 16.01 vs 15.43e9 at K = 1 000, 13.25 vs 13.19e9 at K = 20 (run_r06p).  (Round 3's feedback form,
// progress words per CU, levelled them too but cost more than it gave.)
#ifndef GC_WG_FAIR
#define GC_WG_FAIR 1  // 0: A/B
#endif
#ifndef GC_OCC_RUN
#define GC_OCC_RUN 1  // the commit's probes beyond the home slot consult the bitmap (0: A/B, every one loaded)
#endif
// s_setprio(x), one level up on the plies where this workgroup has its turn (GC_WG_FAIR)
#define QSETPRIO(x, up)                                       \
    do {                                                      \
        if (GC_WG_FAIR && (up)) __builtin_amdgcn_s_setprio((x) + 1); \
        else __builtin_amdgcn_s_setprio(x);                   \
    } while (0)
template <int R, bool OCC, bool S0>
__device__ __forceinline__ StepOut quad_ply(QuadLds& L, const PairCtx& C, int l, int i, bool live, Pos& s, int& a,
                                            u32& d, DevHist& h, u32& nst, RepProbe& pr, QuadPend& pend, OccQ& oq,
                                            QuadQ0Pre& q0, QuadAhead& ah, bool up = false) {
    constexpr bool CARRY = R < 2;  // Q0 / Q1 hold the state
#ifdef GC_PSTAMPS
    bool pst_loaded = false;  // Q1: the commit loaded a slot beyond the home slot
#endif
    // Q2's pick (phase 3's longest) is raised over Q0's outcome there: 14.43-14.63 -> 14.90-15.12e9
    if (R == 0) QSETPRIO(2, up);
    if (R == 2) QSETPRIO(0, up);
    if (GC_WG_FAIR && R == 1) QSETPRIO(2, up);
    if (GC_WG_FAIR && R == 3) QSETPRIO(0, up);
    if (R == 0 || (S0 && R == 1)) a = pend.resolve(L, l);  // the last ply's action: Q2's pick, or the reset table's
    u32 x0 = 0;
    uint16_t ra = (uint16_t)A_NONE;
    if (R == 1 && !S0) {  // phase 0 work first: it does not depend on the action, which Q1 learns after it
        x0 = philox_x0(C.seed, (u32)i, d);  // the next draw (independent of the position)
        if (C.rtable) ra = C.racts[scale_rank(x0, C.rtotal)];
        L.x0[l] = x0;
    }
    if (R == 3 && S0) {
        // the word made ahead (d: the counter it was made from) against the settled counter: it
        // stands unless the last ply was a stalemate (the counter stayed); then the whole wave
        // makes its words again from the settled counters -- the same word where they agree
        const u32 dt = L.d[l];
        if (__any(dt != d)) {
            d = dt;
            quad_ahead(C, i, d, ah);
        }
        L.x0[l] = ah.x0;
        L.ra[l] = ah.ra;
    }
    if (R == 0 && !S0) L.act[l] = (u32)a;
    PST(7);  // (GC_PSTAMPS: the segments as in the paired kernel, phase 0 .. wait D)
    if (R == 1 && !S0) {
        pair_barrier();  // (Q1's phase 0 is above; it meets the others' barrier A here)
        a = (int)L.act[l];
    }
    const bool none = a == A_NONE;                           // empty list: driver reset
    const bool done0 = (s.meta & M_DONE) != 0;               // chess_v2.py:245-251
    const bool cap = mc_of(s.meta) > MOVES_MAX;              // 252-258
    const bool mv = live && !none && !done0 && !cap;         // env_ply runs
    const bool white = (s.meta & M_WHITE) != 0;
    int mr = 0;
    bool irrev = false;
    Pos ns;
    // ---- phase 0
    // A castle is played on one wave-ply in fifty (0.03 % of board-plies), so its terms of the
    // apply -- the cleared squares, the king's and rook's targets, the selects on them -- are made
    // only where a lane of the wave plays one
    const bool cas = R < 2 && __any(mv && a >= 4096);
    if (R == 0 && S0) {  // the apply's king / rook / colour half
        ns = s;
        ns.meta = q0.meta0;  // State::new's rights
        if (!mv) {
        } else if (cas) {
            apply_legal_krw(ns, a, q0.kw, q0.rw);
        } else {
            apply_legal_krw<false>(ns, a, q0.kw, q0.rw);
        }
        L.ns[0][l] = ns.k; L.ns[2][l] = ns.r; L.ns[6][l] = ns.w;
        L.nmeta[l] = ns.meta;
    } else if (R == 1 && S0) {  // the other four boards, the capture's value, the irreversible flag
        ns = s;
        if (!mv) {
        } else if (cas) {
            apply_legal_qbnp(ns, a, &mr, &irrev, q0.occ);
        } else {
            apply_legal_qbnp<false>(ns, a, &mr, &irrev, q0.occ);
        }
        L.ns[1][l] = ns.q; L.ns[3][l] = ns.b; L.ns[4][l] = ns.n; L.ns[5][l] = ns.p;
    } else if (R == 0) {
        ns = s;
        ns.meta = q0.meta0;  // State::new's rights
        if (!mv) {
        } else if (cas) {
            apply_legal_with(ns, white, a, &mr, &irrev, q0.occ, q0.kw, q0.rw);
        } else {
            apply_legal_with<false>(ns, white, a, &mr, &irrev, q0.occ, q0.kw, q0.rw);
        }
        L.ns[0][l] = ns.k; L.ns[1][l] = ns.q; L.ns[2][l] = ns.r; L.ns[3][l] = ns.b;
        L.ns[4][l] = ns.n; L.ns[5][l] = ns.p; L.ns[6][l] = ns.w;
        L.nmeta[l] = ns.meta;
        L.mr[l] = mr;
        L.irrev[l] = irrev ? 1u : 0u;
    }
    PST(0);
    if (S0) PST_ARRIVE(0);  // (GC_PSTAMPS, one quad per workgroup: who arrives last, per barrier)
    if (R != 1 || S0) pair_barrier();
    if (S0) PST_LAST(0);
    PST(1);
    // ---- phase 1
    Gen g;
    bool my_chk = false;
    // Q2 / Q3 fill twice over the post-move board's occupancy, the enemy's sliders here and the own
    // ones in phase 2: the rank operands and the propagator masks are built once and held across
    // the barrier (10 and 12 u64; these two roles carry no state)
    OrthCarry oc{};
    DiagCarry dc{};
    if (R == 0 && S0) {
        ns.q = L.ns[1][l]; ns.b = L.ns[3][l]; ns.n = L.ns[4][l]; ns.p = L.ns[5][l];
    } else if (R == 1 && S0) {
        ns.k = L.ns[0][l]; ns.r = L.ns[2][l]; ns.w = L.ns[6][l];
        ns.meta = L.nmeta[l];
    } else if (R != 0) {
        ns.k = L.ns[0][l]; ns.q = L.ns[1][l]; ns.r = L.ns[2][l]; ns.b = L.ns[3][l];
        ns.n = L.ns[4][l]; ns.p = L.ns[5][l]; ns.w = L.ns[6][l];
        ns.meta = L.nmeta[l];
    }
    if (R == 1 && !S0) {
        mr = L.mr[l];
        irrev = L.irrev[l] != 0;
    }
    gen_base(ns, g);
    if (R == 0) {
        gen_pins(ns, g);
        L.pin3[0][l] = g.checkmask;
        L.pin3[1][l] = g.pinned;
        L.pin3[2][l] = g.pinrays;
        L.f0[l] = g.in_check ? 1u : 0u;
    } else if (R == 1) {
        my_chk = mv && mover_checked(s, ns, white, a);
        L.f1[l] = my_chk ? 1u : 0u;
        if constexpr (OCC) {
        if (oq.clr) {  // the window was emptied
#pragma unroll
            for (int w = 0; w < HTAB / 64; w++) L.occ[w][l] = 0ull;
            oq.clr = false;
        }
        // the next ply's pre-move board if this move stands (ns): its key, and whether its home
        // slot is taken in the window before this ply's entry (phase 2 adds that one)
        const u32 nk = board_key(ns);
        L.nkey[l] = nk;
        oq.probe = !oq.valid || ((L.occ[(nk & (HTAB - 1)) >> 6][l] >> (nk & 63)) & 1) != 0;
        }
    } else if (R == 2) {
        oc = orth_carry(g.occ);
        L.enemy[1][l] = g.ks >= 0 ? side_attacks_leapers(ns, !g.white) | side_attacks_orth(ns, !g.white, oc) : 0ull;
    } else {
        dc = diag_carry(g.occ);
        L.enemy[2][l] = g.ks >= 0 ? side_attacks_diag(ns, !g.white, dc) : 0ull;
    }
    PST(2);
    if (S0) PST_ARRIVE(1);
    pair_barrier();
    if (S0) PST_LAST(1);
    PST(3);
    // ---- phase 2
#define QUAD_ENEMY(l) (L.enemy[1][l] | L.enemy[2][l])
    if (R == 0) {
        g.enemy_att = QUAD_ENEMY(l);
        gen_castles(ns, g);  // lib.rs:578-610 with the whole enemy map
        my_chk = L.f1[l] != 0;
    } else if (R == 1) {
        g.in_check = L.f0[l] != 0;
    } else {
        g.checkmask = L.pin3[0][l];
        g.pinned = L.pin3[1][l];
        g.pinrays = L.pin3[2][l];
        if (R == 2) g.enemy_att = QUAD_ENEMY(l);  // for the king sets
    }
    const bool opp_chk = g.in_check;
    const bool both = opp_chk && my_chk;  // lib.rs:1442-1446
    const bool gen = mv && !both;
    // this maker's sets go to LDS as they are made; their counts leave as the byte prefixes of the
    // count words (gc_core.h sw_prefix_make: running sums through the popcounts), with the total
    u64 pw[4] = {0, 0, 0, 0};
    u32 part = 0;
    int c = 0;
    u32 hl = hl_of(s.meta);
    if (R == 0) {  // pawn sets; castles counted here (phase 2 was Q0's longest: knights to Q3, kings to Q2)
        if (gen) {
            u64 T[SW_SETS];
            sw_pawns(ns, g, T);
            quad_put<SW_P1, SW_N>(L, l, T);
            // the knight sets here, not on Q3: Q0's SIMDs (Q0 + Q2) are the lighter pair in phase 2
            // (same-box A/B: 14.81 vs 14.59e9 at K = 1 000, 4.62 vs 4.70 us per ply at K = 20)
            sw_knights(ns, g, T);
            quad_put<SW_N, SW_ORTH>(L, l, T);
            sw_prefix_make<SW_OWN_Q0>(T, pw, part);
            part += (u32)popc(g.castles);
        }
        L.cw0[0][l] = pw[0];
        L.cw0[1][l] = pw[1];
        L.castles[l] = g.castles;
    } else if (R == 1) {
        if (mv && !both) {
            pin(pr.e0.hdr); pin(pr.e0.k); pin(pr.e0.q); pin(pr.e0.r);
            pin(pr.e0.b); pin(pr.e0.n); pin(pr.e0.p); pin(pr.e0.w);
            if (OCC && oq.fast) pr.e0.hdr = (u64)(h.gen() ^ 1u);  // (after the wait: no loaded register merged)
            // table write deferred to h.commit()
            if constexpr (OCC && GC_OCC_RUN) {
                // Beyond a taken home slot the bitmap answers for the table as well: a slot whose
                // bit is clear holds no entry of this window, so the probe ends there unloaded --
                // in nine of ten such plies that is slot home + 1, and the load was a memory round
                // trip on this phase's chain.  Read here, not carried from phase 1: the bitmap
                // holds every entry up to the last ply's (this ply's is added below).
                c = rep_commit(h, s, pr, hl, irrev, [&](u32 pos) {
                    const bool free = oq.valid && ((L.occ[pos >> 6][l] >> (pos & 63)) & 1) == 0;
                    PST_LOADED(!free);
                    return free;
                });
            } else {  // every slot loaded (the stamp build counts the plies that do)
                c = rep_commit(h, s, pr, hl, irrev, [&](u32) {
                    PST_LOADED(true);
                    return false;
                });
            }
            if (!OCC) {
            } else if (irrev) {  // the window is cleared: from the next ply on the bitmap mirrors it again
                oq.valid = true;
                oq.clr = true;
                oq.probe = false;
            } else if (h.wkind == 2) {  // this ply's new entry: its slot, and the next board's home?
                L.occ[h.wpos >> 6][l] |= 1ull << (h.wpos & 63);
                oq.probe = oq.probe || (u32)h.wpos == (L.nkey[l] & (HTAB - 1));
            }
        }
        L.rep[l] = (u32)c | (hl << 8);
        if (!S0) L.ra[l] = ra;
    } else if (R == 2) {  // unconditional: ignored unless generation is due
        u64 T[SW_SETS];
        sw_orth(ns, g, oc, T);
        quad_put<SW_ORTH, SW_DIAG>(L, l, T);
        sw_kings(ns, g, T);
        quad_put<SW_K, SW_SETS>(L, l, T);
        sw_prefix_make<SW_OWN_Q2>(T, pw, part);
        L.part[2][l] = part;
        // (word 0 holds none of Q2's sets; its own words' prefixes stay in registers across barrier
        // C, pinned: they are complete before it, not made again behind it on the pick's chain)
        pin(pw[1]); pin(pw[2]); pin(pw[3]);
    } else {
        u64 T[SW_SETS];
        sw_diag(ns, g, dc, T);
        quad_put<SW_DIAG, SW_K>(L, l, T);
        sw_prefix_make<SW_OWN_Q3>(T, pw, part);
        L.part[3][l] = part;
        L.cw3[l] = pw[2];  // its four sets are bytes of word 2
    }
    if (R == 0) L.part[0][l] = part;
#ifdef GC_PSTAMPS
    if (R == 1) gc_pst_mark_run(4, pst_loaded);
    else
#endif
    PST(4);
    if (S0) PST_ARRIVE(2);
    pair_barrier();
    if (S0) PST_LAST(2);
    PST(5);
    // ---- phase 3: the outcome (Q0 and Q1, identical arithmetic); Q2 picks the next action
    // from the move sets (Q0 takes it, or the reset table's, at the start of the next ply)
    StepOut o = {0, 0, R_NONE, 0};
    if (R == 0) QSETPRIO(0, up);
    if (R == 2) QSETPRIO(2, up);
    if (R == 2) {  // (on Q3, whose SIMDs Q1 shares: 12.77-12.98 vs 13.30-13.42e9)
        const int total = (int)L.part[0][l] + (int)part + (int)L.part[3][l];
        // the words' byte prefixes, summed where two makers meet (word 1: Q0's knights and the
        // rook / queen sets here; word 2: Q3's sets and the king's)
        const u64 cw[4] = {L.cw0[0][l], pw[1] + L.cw0[1][l], pw[2] + L.cw3[l], pw[3]};
        g.castles = L.castles[l];
        // (a board whose generation is not due reads stale sets here: its pick is not taken)
        L.pick[l] = total > 0 ? (u32)sw_pick_lds<true>(L, l, g, cw, total, (int)scale_rank(L.x0[l], (u32)total)) : (u32)A_NONE;
    }
    if constexpr (CARRY) {
        const int total = gen ? (R == 0 ? (int)part : (int)L.part[0][l]) + (int)L.part[2][l] + (int)L.part[3][l] : 0;
        if (R == 0) {
            const u32 rpk = L.rep[l];
            c = (int)(rpk & 0xFFu);
            hl = rpk >> 8;
            ra = (uint16_t)L.ra[l];
        } else {
            if (S0) ra = (uint16_t)L.ra[l];
            h.commit();  // the window write, issued before the outcome
        }
        // The outcome as flags and selects, no nested regions (in self-play nearly every lane
        // takes the ladder's last arm, so no branch of it was ever skipped).  Chess_v2.py:245-258
        // and lib.rs:1442-1446 end the ply before the move stands; where it stands (play) the
        // 3-fold count, the full window and the mate (270-272) end it after
        const bool play = !none && !done0 && !cap && !both;
        const bool rep3 = c >= 3, full = c == 0, mate = total == 0 && opp_chk;  // 404-407
        const bool end1 = rep3 || full || mate;
        const u32 chk = white ? ((my_chk ? M_WCHK : 0u) | (opp_chk ? M_BCHK : 0u))
                              : ((opp_chk ? M_WCHK : 0u) | (my_chk ? M_BCHK : 0u));
        u32 meta1 = with_hl((ns.meta & ~(u32)(M_WCHK | M_BCHK | M_DONE)) | chk | ((rep3 || full) ? M_DONE : 0u), hl);
        meta1 |= mate ? (u32)M_DONE : 0u;
        meta1 += !end1 && !white ? (1u << M_MC_SHIFT) : 0u;  // 291-292
        const int reason1 = mate ? R_MATE : full ? R_WINDOW_FULL : rep3 ? R_REPETITION : R_NONE;
        const bool have = play && !end1;
        nst += none ? 0u : 1u;
        o.reward = play ? -10 + mr + (mate ? 100 : 0) : 0;
        o.done = none ? 0 : play ? (end1 ? 1 : 0) : 1;
        o.reason = none ? R_NO_MOVES : done0 ? R_DONE_ALREADY : cap ? R_MOVE_CAP : both ? R_BOTH_CHECKED : reason1;
        o.moved = play ? 1 : 0;
        s = ns;  // (the state is the post-move board or the reset position: nothing else survives a ply)
        s.meta = meta1;
        if (!have) {  // reset (chess_v2.py:183-206), also the no-move driver reset
            s = L.rp;
            h.bump_gen();
        }
        // Q1: the next ply's probe, its pre-move board settled, while Q0 still picks (Q1 waits at
        // the next barrier anyway); after this ply's window write, so it sees it
        if (R == 1 && OCC) {  // (the verdict is phases 1-2's; a reset's window is empty, its bitmap cleared next ply)
            pr.key = have ? L.nkey[l] : L.rkey0;
            if (!have) {
                oq.valid = true;
                oq.clr = true;
            }
            oq.fast = !(live && have && oq.probe);
            // one load per lane: the home entry, or the init block's line (a free slot, see above)
            const ulonglong2* src = oq.fast ? reinterpret_cast<const ulonglong2*>(C.icd)
                                            : reinterpret_cast<const ulonglong2*>(h.htab + h.entry((int)(pr.key & (HTAB - 1))) * 8);
            const ulonglong2 e0 = src[0], e1 = src[1], e2 = src[2], e3 = src[3];
            pr.e0 = RepEntry{e0.x, e0.y, e1.x, e1.y, e2.x, e2.y, e3.x, e3.y};
        } else if (R == 1 && live) {
            rep_prefetch(h, s, pr);
        }
        // the draw counter (both: the quads run only with the start position's pick table, so a
        // reset's pick count is its total) and Q0's pending choice of the next action
        const int tot = have ? total : (int)C.rtotal;
        d += tot > 0 ? 1u : 0u;
        if (R == 0) {
            if (S0) L.d[l] = d;
            pend = QuadPend{have, ra};
            q0 = quad_q0pre<S0>(s);  // the next ply's, in the wait for barrier D
        } else if (S0) {
            pend = QuadPend{have, ra};
            q0 = quad_q1pre(s);
        }
    }
    if (R == 3 && S0) {  // the next ply's word, on the counter's usual step, in the wait for barrier D
        d += 1u;
        pin(d);  // (after barrier C: the chain is not to be scheduled into phase 2)
        quad_ahead(C, i, d, ah);
    }
    PST(6);
    if (S0) PST_ARRIVE(3);
    pair_barrier();  // Q2's pick to Q0; LDS free for the next ply
    if (S0) PST_LAST(3);
    return o;
}

// The quads' LDS (static, shared by the role functions below: a direct reference keeps every
// access a ds_ instruction)
__shared__ QuadLds g_quad_lds[ROLL_QUADS_WG];
__shared__ QuadLds g_quad_lds2[QUADS_WG];  // (the paired form's: a kernel is charged only the array it names)
template <int QW>
__device__ __forceinline__ QuadLds& roll_lds(int qw) {
    if constexpr (QW == ROLL_QUADS_WG) return g_quad_lds[qw];
    else return g_quad_lds2[qw];
}

// Turns among the workgroups that share a CU.  A full chip takes a launch's workgroups round
// by round, so with QW quads per workgroup block b meets b + wgs / (4 / QW) ... on its CU and
// the block's part of the launch (half, quarter) is its age there (tools/pstamp_probe.py:
// every CU, profiles/r08_geometry).  At equal priority the SQ issues the older wave first, so
// the plies ran 4.18 / 4.28 / 4.40 / 4.54 us by quarter with two groups of two alternating
// and the launch ended with the youngest.  One quad per workgroup: two of the four are one
// level up in every turn, by a schedule that favours the young -- with ranks 1-4 by (level,
// age), the pairs {0,3} 4, {1,2} 4, {1,3} 3, {2,3} 5 of 16 turns give every workgroup the
// mean rank 2.5 (the oldest is up a quarter of the time, the youngest three quarters):
// 4.32 / 4.37 / 4.40 / 4.40 us.  A nibble per turn, a bit per place.
#define ROLL_TURNS 0xCA69C6A9C69AC69Cull
template <int QW>
__device__ __forceinline__ int roll_place(int block, int wgs) {
    const int part = wgs / (4 / QW);  // the workgroups of one round over the chip
    return (part ? block / part : block) & (4 / QW - 1);
}
template <int QW>
__device__ __forceinline__ bool roll_turn(int place, int turn) {
    if (QW == 2) return ((place ^ turn) & 1) != 0;  // two workgroups per CU: alternating
    return ((ROLL_TURNS >> (4 * (turn & 15) + place)) & 1) != 0;
}

// One role's whole launch (its K plies and its stores), inlined into the kernel's switch on the
// role: a non-inlined function takes generic pointers -- flat memory instructions, which count
// in lgkmcnt too, so every barrier's lgkmcnt(0) waited for the window probe in flight.
template <int RR, bool ST, bool OCC, int QW>
__device__ __forceinline__ void quad_run(uint8_t* __restrict__ slab, int nn, uint64_t seed, u64* __restrict__ htab,
                                      const uint16_t* __restrict__ racts, const EnvDev::InitCache* __restrict__ icd,
                                      u32 rinfo, int plies, uint64_t* __restrict__ stats, u64* __restrict__ trace,
                                      int qw, int l, int i, int place) {
    // the short phase 0 (quad_ply) with one quad per workgroup; the paired form, the short launches',
    // keeps all of the apply on Q0 and the Philox word on Q1: there the short one costs 4-5 %
    constexpr bool S0 = QW == ROLL_QUADS_WG;
    QuadLds& L = roll_lds<QW>(qw);
    const bool live = i < nn;
    const int ii = live ? i : nn - 1;  // dead lanes read a valid board, store nothing
    const PairIO in_io(slab, nn);
    const PairCtx C = {seed, htab, in_io.hgen, racts, icd, (rinfo >> 16) != 0, rinfo & 0xFFFFu};
    Pos s{};
    u32 ua = 0, g0 = 0, nst = 0, d = 0;
    if (RR == 3 && S0) {
        d = in_io.draw[ii];
        pin(d);
    }
    if (RR < 2) {
        s = in_io.load(ii);
        ua = in_io.act[ii];
        g0 = in_io.hgen[ii];
        nst = in_io.nsteps[ii];
        d = in_io.draw[ii];
        pin(s); pin(ua); pin(g0); pin(nst); pin(d);
    }
    // the reset position (and its key) into LDS by Q3, which has no work in phase 0 (on Q0 the
    // wait for its load sat in front of ply 0's apply); read after ply 0's first barrier
    if (RR == 3 && l == 0) {
        const Pos rp = icd->pos;
        L.rp = rp;
        if (OCC) L.rkey0 = board_key(rp);
    }
    int a = (int)ua;
    DevHist h = DevHist{htab, in_io.hgen, g0, ii, HTAB_BITS};
    RepProbe pr;  // Q1: the window probe of the coming ply's pre-move board
    if (RR == 1 && live) rep_prefetch(h, s, pr);
    // Q1: the occupancy bitmap starts empty, so it mirrors a board's window only once that is
    // empty (from the launch's start, or at a reset / an irreversible move); until then the board
    // is probed in the table
    OccQ oq{RR == 1 && hl_of(s.meta) == 0, RR == 1, true, false};
    QuadPend pend{false, (uint16_t)ua};  // Q0 (and Q1): the first ply's action is the env's
    QuadQ0Pre q0{};
    if (RR == 0) q0 = quad_q0pre<S0>(s);
    if (RR == 1 && S0) q0 = quad_q1pre(s);
    QuadAhead ah{};
    if (RR == 3 && S0) {  // the first ply's word, from the entry's counter (read back at the ply's top)
        quad_ahead(C, i, d, ah);
        L.d[l] = d;
    }
#ifdef GC_PSTAMPS
    const unsigned long long g_pst_entry = pst_entry_where();
    unsigned long long rt1 = 0;
    if (l == 0) {
        for (int k = 0; k < 8; k++) gc_pst[threadIdx.x >> 6][k] = 0;
        gc_pst_run[threadIdx.x >> 6][0] = gc_pst_run[threadIdx.x >> 6][1] = 0;
        if (S0)
            for (int b = 0; b < 4; b++)
                for (int k = 0; k <= PST_BINS; k++) gc_pst_last[threadIdx.x >> 6][b][k] = 0;
        gc_pst[threadIdx.x >> 6][8] = __builtin_amdgcn_s_memtime();
    }
    const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();
#endif
    // per-launch stats (ST), packed: a launch runs <= ROLLOUT_MAX_PLIES plies, so every count fits
    // 16 bits and the reward sum 32 -- four registers instead of nine
    u32 sa = 0, sb = 0, sc = 0;  // steps | errors << 16, mates | 3-folds << 16, move caps | no-moves << 16
    int32_t rsum = 0;
    StepOut o = {0, 0, R_NONE, 0};
#ifndef GC_TURN_SHIFT
#define GC_TURN_SHIFT 2  // turns of 4 plies: same box at K = 20, 8 repeats, 13.32 vs 13.01e9 (events
                         // 4.53 vs 4.66 us per ply; 8-ply turns 13.22); at K = 1 000 level (run_r06v, w).
                         // One quad per workgroup, K = 1 000: 17.06 vs 16.87 (2 plies), 16.82e9 (1)
#endif
    // (GC_WG_FAIR, above: this workgroup's turn one level up; the turn's bit is made once per turn)
    constexpr int TURN = 1 << GC_TURN_SHIFT;
    for (int p0 = 0; p0 < plies; p0 += TURN) {
      const bool up = GC_WG_FAIR && roll_turn<QW>(place, p0 >> GC_TURN_SHIFT);
      const int pe = p0 + TURN < plies ? p0 + TURN : plies;
      for (int p = p0; p < pe; p++) {
        o = quad_ply<RR, OCC, S0>(L, C, l, i, live, s, a, d, h, nst, pr, pend, oq, q0, ah, up);
        const int played = a;  // (Q0: resolved at the ply's start; Q1: read after its barrier A)
#ifdef GC_PSTAMPS
        if (p == 0) rt1 = __builtin_amdgcn_s_memrealtime();
#endif
        if (RR == 1) {  // the ply's outputs (trace, stats) and the window write
            if (trace && live) trace[(size_t)p * nn + i] = trace_word(played == A_NONE ? -1 : played, o);
            if (!ST) {
            } else if (played == A_NONE) {
                sc += 1u << 16;
            } else {
                sa += 1u;
                rsum += o.reward;
                if (o.done) {
                    sb += (o.reason == R_MATE || o.reason == R_MATED ? 1u : 0u) | (o.reason == R_REPETITION ? 1u << 16 : 0u);
                    sc += (o.reason == R_MOVE_CAP ? 1u : 0u) | (o.reason == R_OPP_NO_MOVE ? 1u << 16 : 0u);
                    sa += o.reason == R_BOTH_CHECKED || o.reason == R_WINDOW_FULL ? 1u << 16 : 0u;
                }
            }
            h.commit();  // this ply's window write lands before the next ply's probe
        }
      }
    }
#ifdef GC_PSTAMPS
    if (g_pst_out != nullptr && l == 0) {
        const size_t w = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        for (int k = 0; k < 8; k++) g_pst_out[w * 12 + k] = gc_pst[threadIdx.x >> 6][k];
        g_pst_out[w * 12 + 8] = g_pst_entry;
        g_pst_out[w * 12 + 9] = rt0;
        g_pst_out[w * 12 + 10] = rt1;
        g_pst_out[w * 12 + 11] = __builtin_amdgcn_s_memrealtime();
        if (g_pst_run_out != nullptr) {
            g_pst_run_out[w * 2] = gc_pst_run[threadIdx.x >> 6][0];
            g_pst_run_out[w * 2 + 1] = gc_pst_run[threadIdx.x >> 6][1];
        }
        if (S0 && g_pst_last_out != nullptr)
            for (int b = 0; b < 4; b++)
                for (int k = 0; k <= PST_BINS; k++)
                    g_pst_last_out[(w * 4 + b) * (PST_BINS + 1) + k] = gc_pst_last[threadIdx.x >> 6][b][k];
    }
#endif
    if (!live || RR >= 2) return;
    const PairIO io = store_io(slab, nn);
    if (RR == 0) {
        a = pend.resolve(L, l);  // the next action (Q2's last pick arrived before the last barrier)
        io.act[i] = (uint16_t)a;
        io.draw[i] = d;
    } else {
        io.store(i, s);
        // (h.flush through io's freshly derived pointer: h's own, kept from the entry load across
        // the whole loop, was the kernel's one spill -- and a private segment slows every wave's launch)
        if (h.gen() != g0) io.hgen[i] = h.gen();
        io.nsteps[i] = nst;
        io.reward[i] = o.reward;
        io.done[i] = (uint8_t)o.done;
        io.reason[i] = (uint8_t)o.reason;
        if (ST) {
            uint64_t* so = stats + 8 * (size_t)i;
            so[0] += sa & 0xFFFFu; so[1] += (uint64_t)(int64_t)rsum;
            so[2 + R_MATE] += sb & 0xFFFFu; so[2 + R_REPETITION] += sb >> 16; so[2 + R_MOVE_CAP] += sc & 0xFFFFu;
            so[2 + R_NO_MOVES] += sc >> 16; so[2 + R_BOTH_CHECKED] += sa >> 16;
        }
    }
}

// The fused K-ply rollout on quads (k_env_rollout2's contract: same arguments, state, trace
// and stats).  Q0 writes the next action and draw counter, Q1 the rest, as W0 / W1 there.
template <bool OCC, int QW>
__global__ void __launch_bounds__(4 * QUAD_BOARDS * QW) __attribute__((amdgpu_waves_per_eu(4)))
    k_env_rollout4(uint8_t* __restrict__ slab, int nn, uint64_t seed, u64* __restrict__ htab,
                   const uint16_t* __restrict__ racts, const EnvDev::InitCache* __restrict__ icd, u32 rinfo,
                   uint64_t* __restrict__ stats, u64* __restrict__ trace) {
    const int plies = (int)(rinfo >> 18);
    rinfo &= 0x1FFFFu;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int qw = wv >> 2;  // the quad of this wave within the workgroup
    const int wgs = (nn + QUAD_BOARDS * QW - 1) / (QUAD_BOARDS * QW);  // (not gridDim: no implicit kernargs)
    const int place = roll_place<QW>((int)blockIdx.x, wgs);
    // role = (wave & 3) ^ rot: a permutation of the quad's roles whatever rot is.  One quad per
    // workgroup: rot = 0 -- the dispatcher starts each workgroup of a CU one SIMD further on
    // (waves 0-3 on SIMDs 2130, 1302, 3021, 0213: every CU, tools/pstamp_probe.py), so every
    // SIMD hosts the four roles, one of each workgroup, as it is; rotating by the place as
    // well undid that (6 of the 16 role-SIMD pairs per CU, 13.7 vs 16.0e9).  Two: the second
    // quad's waves land on the first's SIMDs, so its roles are rotated by GC_QXOR.
    const int role = (wv & 3) ^ ((qw & 1) ? GC_QXOR : 0);
    const int l = threadIdx.x & (QUAD_BOARDS - 1);
    const int i = (blockIdx.x * QW + qw) * QUAD_BOARDS + l;
    // Issue priority: a SIMD hosts Q0 + Q2 or Q1 + Q3 (of both quads of a workgroup and of the
    // CU's other workgroup; one quad per workgroup: all four roles); the state-carrying roles
    // hold the longer chains, so their waves issue first (same-box A/B: 13.39-13.46 ->
    // 14.21-14.25e9; Q1 alone 13.99-14.17).  Packed 2-bit priority per role, GC_QPRIO for
    // diagnostic builds.  Re-measured with one quad per workgroup (K = 1 000, two groups of two
    // alternating: 16.37e9): no role priorities 15.02, Q2 high throughout 16.09, Q1 low 15.45,
    // no swap for phase 3 16.06 -- the scheme stays.
#ifndef GC_QPRIO
#define GC_QPRIO 0x0A  // Q0 2, Q1 2, Q2 0, Q3 0
#endif
    switch ((GC_QPRIO >> (2 * role)) & 3) {  // (s_setprio takes an immediate)
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        case 3: __builtin_amdgcn_s_setprio(3); break;
        default: break;
    }
    switch (role) {
        case 0: quad_run<0, false, OCC, QW>(slab, nn, seed, htab, racts, icd, rinfo, plies, stats, trace, qw, l, i, place); break;
        case 1:
            if (stats) quad_run<1, true, OCC, QW>(slab, nn, seed, htab, racts, icd, rinfo, plies, stats, trace, qw, l, i, place);
            else quad_run<1, false, OCC, QW>(slab, nn, seed, htab, racts, icd, rinfo, plies, stats, trace, qw, l, i, place);
            break;
        case 2: quad_run<2, false, OCC, QW>(slab, nn, seed, htab, racts, icd, rinfo, plies, stats, trace, qw, l, i, place); break;
        default: quad_run<3, false, OCC, QW>(slab, nn, seed, htab, racts, icd, rinfo, plies, stats, trace, qw, l, i, place); break;
    }
    // The completion word: every workgroup, its stores performed (the barrier waits for them),
    // counts itself; the last one bumps the launch count and writes it to host-mapped memory,
    // where gc_env_wait_rollout sees it ~5 us before the stream's completion signal would tell
    // (the end-of-kernel write-back and the command processor's signal: tools/region_anatomy.hip).
    // A timing signal only -- the results are read through the stream, after the kernel's own
    // release -- so no fences: an agent-scope release per workgroup writes its XCD's L2 back
    // (+40 us per launch, measured).
    const EnvDev::InitCache::DoneWord dw = icd->done;
    if (dw.ctr) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const u32 prev = __hip_atomic_fetch_add(dw.ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (prev == (u32)wgs - 1) {
                __hip_atomic_store(dw.ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const u32 v = __hip_atomic_fetch_add(dw.seq, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
                __hip_atomic_store(dw.host, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// Fused K-ply random self-play: state in registers for the whole launch.  Per-ply outputs
// go to the optional trace [ply][N] (trace_word); the last ply's outputs and per-board stats
// [steps, reward_sum(two's complement), ends[0..5]] are written.
template <bool OPP>
__global__ void __launch_bounds__(BLOCK) k_env_rollout(EnvDev e, int plies, u64* trace, uint64_t* stats) {
    LDS_SCRATCH_DECL;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e.n) return;
    Pos s = e.st.load(i);
    u32 g0 = e.hgen[i], d = e.draw[i], ua = e.act[i];
    pin(s); pin(g0); pin(d); pin(ua);
    DevHist h = e.hist(i, g0);
    PolicyCtx pc = {e.seed, (u32)i, d};
    int a = (int)ua;
    uint64_t steps = 0, rsum = 0;
    u32 e_mate = 0, e_rep = 0, e_cap = 0, e_nomove = 0, e_err = 0;
    StepOut o = {0, 0, R_NONE, 0};
    for (int p = 0; p < plies; p++) {
        o = {0, 0, R_NONE, 0};
        Gen g;
        MoveSet ms;
        bool have = false;
        int played = a;
        if (a == A_NONE) {
            reset_board(e, s, h);
            o.reason = R_NO_MOVES;
            e_nomove++;
            played = -1;
        } else {
            o = OPP ? env_step_vs<false>(s, h, a, nullptr, g, ms, scr, pc) : env_step<false>(s, h, a, nullptr, g, ms, scr);
            have = o.moved;
            steps++;
            rsum += (uint64_t)(int64_t)o.reward;
            if (o.done) {
                e_mate += o.reason == R_MATE || o.reason == R_MATED;
                e_rep += o.reason == R_REPETITION;
                e_cap += o.reason == R_MOVE_CAP;
                e_err += o.reason == R_BOTH_CHECKED || o.reason == R_WINDOW_FULL;
                e_nomove += o.reason == R_OPP_NO_MOVE;
                reset_board(e, s, h);
                have = false;
            }
        }
        if (OPP && !have) after_reset<OPP>(e, s, h, g, ms, scr, pc);
        if (trace) trace[(size_t)p * e.n + i] = trace_word(played, o);
        a = selfplay_pick(s, pc);
        h.commit();
    }
    e.reward[i] = o.reward;  // the last ply's env.step() outputs (per-ply: trace buffers)
    e.done[i] = (uint8_t)o.done;
    e.reason[i] = (uint8_t)o.reason;
    e.st.store(i, s);
    h.flush(g0);
    e.draw[i] = pc.draw;
    e.act[i] = (uint16_t)a;
    e.nsteps[i] += (u32)steps;
    if (stats) {
        uint64_t* so = stats + 8 * (size_t)i;
        so[0] += steps; so[1] += rsum;
        so[2 + R_MATE] += e_mate; so[2 + R_REPETITION] += e_rep; so[2 + R_MOVE_CAP] += e_cap;
        so[2 + R_NO_MOVES] += e_nomove; so[2 + R_BOTH_CHECKED] += e_err;
    }
}
