// gc_minimax.h -- fixed-depth minimax search (gc_env_minimax, include/gymchess.h): for a device list
// of boards, the exact depth-limited negamax score of every root move on reference rules, the best
// move under a stated tie rule and a leaf value in tree.backup's units.  Position-only: it reads the
// env and writes nothing of it; 3-fold repetition, the move cap and the window play no part.
//
// The first half compiles for the host too (tests/core_host/minimax_host.cpp): the recursion over
// the remaining depth (mm_edge / mm_node, a template on it: nested loops, one scratch object per
// interior level, no per-thread stack), the material term, the value mapping, the tie rule and the
// whole row as one sequential function (minimax_row) -- the statement of what k_minimax computes
// wave-wide.  It is built on gen_init / gen_moves / MoveWalk / select_action / apply_legal /
// eff_rights / mover_checked / count_moves and on nothing else.  The second half is the kernel.
//
// The definition (include/gymchess.h states it in full).  V(pos, d, ply), for the side to move:
// no legal move: -(MATE - ply) in check, else 0; d == 0: material(pos) (the leaf still counts its
// moves first, so depth 1 sees a mate in one); else the maximum over the legal moves a, ascending
// action id, of E(pos, a, d, ply) = 0 on an edge that leaves both kings in check (env_ply's
// R_BOTH_CHECKED) and -V(child(pos, a), d - 1, ply + 1) on any other.  A root move's score is
// s_a = E(root, a, depth, 0).
//
// Pruning.  Below a root move the search is a fail-soft alpha-beta, which returns the exact value
// whenever it lies inside the window.  A root move is searched with the full window -- its score is
// exact -- except that a lane's later root moves take (its own best so far) - 1 as the lower bound:
// a score that fails low there is strictly below that best, so it is neither the maximum nor a tie.
// When the score list is asked for, every root move gets the full window.
//
// Mapping: one 64-lane workgroup per row.  Every lane generates the root (wave-uniform work, its
// parked targets in one 128-byte plane the wave shares) and takes the root moves lane, lane + 64, ...
// by rank in ascending action id (select_action); the wave then reduces with shuffles and ballots:
// the maximum, the ties in rank order, the reservoir rule.  LDS: one SCRATCH_SLOTS x 64 x 8 B plane
// per interior level below the root, three (24 KB) at depth 4.  The wave lasts as long as its
// slowest lane, and 64 rows are 64 waves; splitting one root move's subtree over lanes is not done.
//
// Quiescence (gc_env_minimax_q, quiesce = q in 1..MM_MAX_QUIESCE).  The leaf's material becomes
// QS(pos, q, ply): no move: rule 1; q == 0: material; in check: the maximum over ALL moves, no
// stand-pat; else max(material, the maximum over the captures) -- each edge EQ = 0 when both kings
// are checked, else -QS(child, q - 1, ply + 1).  The levels object carries q (MmQuiesce<L>): with
// it mm_node<0> enters mm_qs, a fixed nest of MM_MAX_QUIESCE levels with the remaining q a runtime
// value; without it (quiesce == 0) nothing of this is instantiated.  A quiescence level parks no move
// set: it walks the own pieces by ctz and takes legal_targets per piece (select_action's ms.big
// walk), masked with g.opp unless in check, then the castles when in check -- no LDS of its own.
// Order: ascending action id, as everywhere else here; fail-soft alpha-beta, the stand-pat value
// raises alpha and returns at once when it reaches beta.
#pragma once

namespace gc {

static constexpr int MM_MATE = 30000;      // a mate at ply p scores MM_MATE - p for the winner
static constexpr int MM_MATE_BAND = 128;   // scores within it of MM_MATE are mates (value +-1)
static constexpr int MM_INF = 32767;       // outside every score
static constexpr int MM_MAX_DEPTH = 4;
static constexpr int MM_MAX_QUIESCE = 4;   // quiescence plies below a leaf (0: the leaf is its material)
static constexpr int MM_LANES = 64;        // root moves are dealt to this many lanes, rank % MM_LANES

// material from the view of the side to move: sum of value * (own - enemy) in apply_move's capture
// values (Q 10, R 5, B 3, N 3, P 1; kings 0), unclamped
GC_HD int minimax_material(const Pos& s) {
    const u64 occ = s.k | s.q | s.r | s.b | s.n | s.p;
    const u64 own = (s.meta & M_WHITE) ? s.w : occ & ~s.w, opp = occ & ~own;
    return 10 * (popc(s.q & own) - popc(s.q & opp)) + 5 * (popc(s.r & own) - popc(s.r & opp)) +
           3 * (popc((s.b | s.n) & own) - popc((s.b | s.n) & opp)) + (popc(s.p & own) - popc(s.p & opp));
}

// a score as a leaf value for the side to move: +-1 in the mate bands, else the material clamped
// to +-16 in sixteenths (playout_value's material scale); every case is exact in fp32
GC_HD float minimax_value(int score) {
    if (score >= MM_MATE - MM_MATE_BAND) return 1.0f;
    if (score <= -(MM_MATE - MM_MATE_BAND)) return -1.0f;
    const int c = score < -16 ? -16 : (score > 16 ? 16 : score);
    return (float)c * 0.0625f;
}

// the random tie rule (reservoir sampling over the ties T in ascending action id, keyed by the
// BOARD index): the pick is T[i] of the largest i for which this holds; it holds for i = 0
GC_HD bool minimax_tie_keeps(u64 seed, u32 board, u32 draw, u32 i) {
    return policy_index(seed, board, draw + i, i + 1) == 0;
}

// MoveWalk's castles come queen side first (the reference's order); in action ids the king side
// (4096 / 4098) sorts before the queen side (4097 / 4099), so with both the two swap
GC_HD int mm_ascending(int action, u32 castles) { return (action >= 4096 && castles == 3u) ? action ^ 1 : action; }

// the levels object of a search with quiescence: L's planes and the plies q below a leaf
template <class L>
struct MmQuiesce {
    L& lv;
    int q;
    template <int D>
    GC_HDM decltype(auto) at() { return lv.template at<D>(); }
};
template <class L> struct mm_quiesces { static constexpr bool value = false; };
template <class L> struct mm_quiesces<MmQuiesce<L>> { static constexpr bool value = true; };

template <int N, bool PRUNE>
GC_HD int mm_qs(const Pos& s, const Gen& g, int q, int ply, int alpha, int beta, u32& nodes);

// EQ(s, a, q, ply) within (alpha, beta), q >= 1 the quiescence plies left at s, N >= q the levels
// left in the nest: mm_edge with QS below it
template <int N, bool PRUNE>
GC_HD int mm_qedge(const Pos& s, bool white, int action, int q, int ply, int alpha, int beta, u32& nodes) {
    Pos c = s;
    c.meta = (c.meta & ~(u32)M_RIGHTS) | eff_rights(s);
    int rw;
    bool irrev;
    apply_legal(c, white, action, &rw, &irrev);
    Gen g;
    gen_init(c, g);
    if (g.in_check && mover_checked(s, c, white, action)) return 0;
    nodes++;
    return -mm_qs<N - 1, PRUNE>(c, g, q - 1, ply + 1, -beta, -alpha, nodes);
}

// QS(s, q, ply) within (alpha, beta); g = gen_init(s), q <= N.  The caller has counted the node.
// One call site of mm_qedge per level (the castles ride in the same loop as the piece moves): the
// nest is inlined, so a second one would double the code at every level.
template <int N, bool PRUNE>
GC_HD int mm_qs(const Pos& s, const Gen& g, int q, int ply, int alpha, int beta, u32& nodes) {
    if (count_moves(s, g) == 0) return g.in_check ? -(MM_MATE - ply) : 0;
    const int stand = minimax_material(s);
    if constexpr (N == 0) {
        return stand;
    } else {
        if (q <= 0) return stand;
        int best = -MM_INF;
        if (!g.in_check) {  // the stand-pat: the side to move may decline every capture
            best = stand;
            if (PRUNE) {
                alpha = best > alpha ? best : alpha;
                if (alpha >= beta) return best;
            }
        }
        const u64 keep = g.in_check ? ~0ull : g.opp;  // in check every evasion, else the captures
        u32 cs = g.in_check ? g.castles : 0u;
        u64 pcs = g.own, tg = 0;
        int sq = 0;
        for (;;) {  // ascending action id: squares by ctz, targets by ctz, then KS, QS
            while (!tg && pcs) {
                sq = ctz(pcs);
                pcs &= pcs - 1;
                tg = legal_targets(s, g, sq, type_at(s, sq)) & keep;
            }
            int a;
            if (tg) {
                a = sq * 64 + ctz(tg);
                tg &= tg - 1;
            } else if (cs & 2u) {
                a = g.white ? A_KSW : A_KSB;
                cs &= ~2u;
            } else if (cs & 1u) {
                a = g.white ? A_QSW : A_QSB;
                cs = 0u;
            } else {
                break;
            }
            const int e = mm_qedge<N, PRUNE>(s, g.white, a, q, ply, alpha, beta, nodes);
            best = e > best ? e : best;
            if (PRUNE) {
                alpha = best > alpha ? best : alpha;
                if (alpha >= beta) break;
            }
        }
        return best;
    }
}

template <int D, bool PRUNE, class L>
GC_HD int mm_node(const Pos& s, const Gen& g, int ply, int alpha, int beta, L& lv, u32& nodes);

// E(s, a, D, ply) within (alpha, beta), D >= 1 the remaining depth at s: exact inside the window, a
// bound on its side outside (fail-soft); !PRUNE: always exact
template <int D, bool PRUNE, class L>
GC_HD int mm_edge(const Pos& s, bool white, int action, int ply, int alpha, int beta, L& lv, u32& nodes) {
    Pos c = s;
    c.meta = (c.meta & ~(u32)M_RIGHTS) | eff_rights(s);  // State::new, as env_ply
    int rw;
    bool irrev;
    apply_legal(c, white, action, &rw, &irrev);
    Gen g;
    gen_init(c, g);
    if (g.in_check && mover_checked(s, c, white, action)) return 0;  // both kings in check: the episode ends, nobody is rewarded
    return -mm_node<D - 1, PRUNE>(c, g, ply + 1, -beta, -alpha, lv, nodes);
}

// V(s, D, ply) within (alpha, beta); g = gen_init(s).  Level D parks its targets in lv.at<D>().
template <int D, bool PRUNE, class L>
GC_HD int mm_node(const Pos& s, const Gen& g, int ply, int alpha, int beta, L& lv, u32& nodes) {
    nodes++;
    if constexpr (D == 0 && mm_quiesces<L>::value) {
        return mm_qs<MM_MAX_QUIESCE, PRUNE>(s, g, lv.q, ply, alpha, beta, nodes);
    } else if constexpr (D == 0) {
        if (count_moves(s, g) == 0) return g.in_check ? -(MM_MATE - ply) : 0;
        return minimax_material(s);
    } else {
        auto&& scr = lv.template at<D>();
        MoveSet ms;
        gen_moves(s, g, ms, scr);
        if (ms.total == 0) return g.in_check ? -(MM_MATE - ply) : 0;
        int best = -MM_INF;
        MoveWalk w(g);
        for (int k = 0; k < ms.total; k++) {
            const int a = mm_ascending(next_child(w, s, g, ms, scr, k), g.castles);  // (any order gives the same maximum)
            const int e = mm_edge<D, PRUNE>(s, g.white, a, ply, alpha, beta, lv, nodes);
            best = e > best ? e : best;
            if (PRUNE) {
                alpha = best > alpha ? best : alpha;
                if (alpha >= beta) break;
            }
        }
        return best;
    }
}

// a root move's score s_a = E(root, a, depth, 0) for depth in 1..MM_MAX_DEPTH, exact if it is above
// `lower` (PRUNE: otherwise some value <= lower); nodes += the positions visited below the root
template <bool PRUNE, class L>
GC_HD int minimax_root_edge(const Pos& root, bool white, int action, int depth, int lower, L& lv, u32& nodes) {
    switch (depth) {
        case 1: return mm_edge<1, PRUNE>(root, white, action, 0, lower, MM_INF, lv, nodes);
        case 2: return mm_edge<2, PRUNE>(root, white, action, 0, lower, MM_INF, lv, nodes);
        case 3: return mm_edge<3, PRUNE>(root, white, action, 0, lower, MM_INF, lv, nodes);
        default: return mm_edge<4, PRUNE>(root, white, action, 0, lower, MM_INF, lv, nodes);
    }
}

// what one lane keeps over its root moves: its best score and in which of its rounds (round q =
// the ranks 64 q ... 64 q + 63) it reached it.  A side has at most 63 * 27 + 2 < 32 * 64 moves.
struct MinimaxLane {
    int best;
    u32 rounds;
    GC_HDM void take(int round, int e) {
        rounds = e > best ? 0u : rounds;
        best = e > best ? e : best;
        rounds |= e == best ? 1u << round : 0u;
    }
    // the lower bound for this lane's next root move (exact: every score must be exact)
    GC_HDM int lower(bool exact) const { return (exact || best == -MM_INF) ? -MM_INF : best - 1; }
};

struct MinimaxRow {
    int count;     // root moves; 0 for a done board
    int pick;      // A_NONE without a move
    int score;
    float value;
    u32 nodes;     // positions visited, the root included
};

// One row, sequentially: the root `s` (not done) searched to `depth`, root moves dealt to MM_LANES
// lanes exactly as the kernel deals them (so `nodes` is the kernel's too).  tiebreak 0 = first,
// 1 = random on (seed, board, draw + i).  actions / scores: the first min(count, cap) root moves in
// ascending action id with their exact scores, padded with 0xFFFF / INT32_MIN to cap (or null).
// lv: the levels' scratch objects, rs: the root's.
template <bool PRUNE, class L, class RS>
GC_HD MinimaxRow minimax_row(const Pos& s, int depth, int tiebreak, u64 seed, u32 board, u32 draw, int cap,
                             uint16_t* actions, int32_t* scores, L& lv, RS& rs) {
    MinimaxRow r = {0, A_NONE, 0, 0.0f, 1};
    Gen g;
    MoveSet ms;
    gen_init(s, g);
    gen_moves(s, g, ms, rs);
    r.count = ms.total;
    for (int k = 0; k < cap; k++) {
        if (actions) actions[k] = 0xFFFF;
        if (scores) scores[k] = INT32_MIN;
    }
    if (ms.total == 0) {
        r.score = g.in_check ? -MM_MATE : 0;
        r.value = minimax_value(r.score);
        return r;
    }
    const bool exact = !PRUNE || actions || scores;
    MinimaxLane ln[MM_LANES];
    int best = -MM_INF;
    for (int lane = 0; lane < MM_LANES; lane++) {
        ln[lane] = MinimaxLane{-MM_INF, 0u};
        for (int k = lane; k < ms.total; k += MM_LANES) {
            const int a = select_action(s, g, ms, rs, k);
            const int e = minimax_root_edge<PRUNE>(s, g.white, a, depth, ln[lane].lower(exact), lv, r.nodes);
            ln[lane].take(k / MM_LANES, e);
            if (k < cap) {
                if (actions) actions[k] = (uint16_t)a;
                if (scores) scores[k] = e;
            }
        }
        best = ln[lane].best > best ? ln[lane].best : best;
    }
    int rank = -1;
    u32 i = 0;  // the ties so far
    for (int k = 0; k < ms.total; k++) {
        const MinimaxLane& l = ln[k % MM_LANES];
        if (l.best != best || !((l.rounds >> (k / MM_LANES)) & 1)) continue;
        if (tiebreak ? minimax_tie_keeps(seed, board, draw, i) : i == 0) rank = k;
        i++;
    }
    r.pick = select_action(s, g, ms, rs, rank);
    r.score = best;
    r.value = minimax_value(best);
    return r;
}

}  // namespace gc

#if defined(__HIPCC__)
// ----------------------------------------------------------------------------- device side
#define MINIMAX_BLOCK 64  // one wave per workgroup, one workgroup per row

// per-lane move-target scratch of one level: slot j of lane t at plane[j * 64 + t] (LdsScratch's
// layout at this kernel's block size)
struct MmLaneScratch {
    static constexpr bool kPark = true;
    u64* base;
    __device__ void put(int j, u64 v) { base[j * MINIMAX_BLOCK] = v; }
    __device__ u64 get(int j) const { return base[j * MINIMAX_BLOCK]; }
};
// the root's: every lane of the wave generates the same root, so all park the same value in the
// same slot and read it back as a broadcast
struct MmRootScratch {
    static constexpr bool kPark = true;
    u64* base;
    __device__ void put(int j, u64 v) { base[j] = v; }
    __device__ u64 get(int j) const { return base[j]; }
};
struct MmLevels {  // level D (remaining depth at the node, 1 .. MM_MAX_DEPTH - 1) -> its plane
    u64* base;
    template <int D>
    __device__ MmLaneScratch at() const {
        static_assert(D >= 1 && D < gc::MM_MAX_DEPTH, "an interior level below the root");
        return MmLaneScratch{base + (D - 1) * SCRATCH_SLOTS * MINIMAX_BLOCK};
    }
};

struct MinimaxArgs {
    const int32_t* idx;  // [rows] or null (board j)
    int depth, tiebreak;
    uint64_t seed;
    u32 draw;
    uint16_t* pick;      // [rows] or null
    int32_t* score;      // [rows] or null
    float* value;        // [rows] or null
    int32_t* count;      // [rows] or null
    int cap;
    uint16_t* actions;   // [rows][cap] or null
    int32_t* scores;     // [rows][cap] or null
    int quiesce;         // 0 .. MM_MAX_QUIESCE; read by the QUIESCE instantiations only
};

template <bool QUIESCE>
__device__ __forceinline__ auto& mm_levels_of(MmLevels& plain, gc::MmQuiesce<MmLevels>& q) {
    if constexpr (QUIESCE) return q;
    else return plain;
}

// NODES: count the positions visited (nodes_out is not null); QUIESCE: a quiescence search below
// the leaves (a.quiesce >= 1; the levels object is MmQuiesce<MmLevels>)
template <bool NODES, bool QUIESCE = false>
__global__ void __launch_bounds__(MINIMAX_BLOCK) k_minimax(SoA st, MinimaxArgs a, u32* __restrict__ nodes_out) {
    __shared__ u64 lds_levels[(gc::MM_MAX_DEPTH - 1) * SCRATCH_SLOTS * MINIMAX_BLOCK];
    __shared__ u64 lds_root[SCRATCH_SLOTS];
    const int lane = threadIdx.x, j = blockIdx.x;
    const int b = a.idx ? a.idx[j] : j;
    const bool inside = (u32)b < (u32)st.n;
    uint16_t* const acts = a.actions ? a.actions + (size_t)j * a.cap : nullptr;
    int32_t* const scs = a.scores ? a.scores + (size_t)j * a.cap : nullptr;
    const Pos s = st.load(inside ? b : 0);
    const bool live = inside && !(s.meta & M_DONE);  // wave-uniform, as everything about the root
    Gen g;
    MoveSet ms;
    MmRootScratch rs{lds_root};
    int count = inside ? 0 : -1;
    if (live) {
        gen_init(s, g);
        gen_moves(s, g, ms, rs);
        count = ms.total;
    }
    const int listed = count < 0 ? 0 : (count < a.cap ? count : a.cap);
    for (int k = listed + lane; k < a.cap; k += MINIMAX_BLOCK) {  // the padding
        if (acts) acts[k] = 0xFFFF;
        if (scs) scs[k] = INT32_MIN;
    }
    int pick = A_NONE, score = 0;
    u32 nodes = 0;
    if (live && count == 0) score = g.in_check ? -gc::MM_MATE : 0;
    if (live && count > 0) {
        MmLevels planes{lds_levels + lane};
        gc::MmQuiesce<MmLevels> deeper{planes, a.quiesce};
        auto& lv = mm_levels_of<QUIESCE>(planes, deeper);
        const bool exact = acts || scs;
        gc::MinimaxLane ln = {-gc::MM_INF, 0u};
        for (int k = lane; k < count; k += MINIMAX_BLOCK) {
            const int act = select_action(s, g, ms, rs, k);
            const int e = gc::minimax_root_edge<true>(s, g.white, act, a.depth, ln.lower(exact), lv, nodes);
            ln.take(k / MINIMAX_BLOCK, e);
            if (k < a.cap) {
                if (acts) acts[k] = (uint16_t)act;
                if (scs) scs[k] = e;
            }
        }
        // the maximum over the wave
        int best = ln.best;
        for (int off = MINIMAX_BLOCK / 2; off; off >>= 1) {
            const int o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
        // the ties in rank order, round by round: the first, or the last the reservoir rule keeps
        const u32 mine = ln.best == best ? ln.rounds : 0u;
        const int rounds = (count + MINIMAX_BLOCK - 1) / MINIMAX_BLOCK;
        int rank = -1;
        u32 seen = 0;
        for (int q = 0; q < rounds; q++) {
            const bool tie = (mine >> q) & 1;
            const u64 ties = __ballot(tie);
            if (!ties) continue;
            if (a.tiebreak) {
                const u32 i = seen + (u32)gc::popc(ties & gc::below(lane));
                const u64 kept = __ballot(tie && gc::minimax_tie_keeps(a.seed, (u32)b, a.draw, i));
                if (kept) rank = q * MINIMAX_BLOCK + gc::msb(kept);
            } else if (rank < 0) {
                rank = q * MINIMAX_BLOCK + gc::ctz(ties);
            }
            seen += (u32)gc::popc(ties);
        }
        pick = select_action(s, g, ms, rs, rank);
        score = best;
        if (NODES)
            for (int off = MINIMAX_BLOCK / 2; off; off >>= 1) nodes += (u32)__shfl_xor((int)nodes, off);
    }
    if (lane) return;
    if (a.pick) a.pick[j] = (uint16_t)pick;
    if (a.score) a.score[j] = score;
    if (a.value) a.value[j] = live ? gc::minimax_value(score) : 0.0f;
    if (a.count) a.count[j] = count;
    if (NODES) nodes_out[j] = live ? nodes + 1 : 0u;
}
#endif
