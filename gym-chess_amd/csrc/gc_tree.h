// gc_tree.h -- the batched search tree on the device: per-game node arrays in HBM, a PUCT descent
// to one leaf per game (k_tree_select), the leaf's expansion and the negamax backup
// (k_tree_backup), the same for several leaves per game per call with a virtual loss
// (k_tree_select_batch / k_tree_backup_batch), the root's visit distribution with a move
// (k_tree_root_policy), and the played move's subtree kept across moves (k_tree_advance_mark /
// k_tree_advance_compact, at the end) (gc_tree_*, include/gymchess.h).  The solver
// (gc_tree_solver_enable: forced wins, draws and losses proven during the search) is the <true>
// instantiation of k_tree_reset / select / backup / root_policy / advance_compact, plus
// tree_propagate and k_tree_root_proof; the <false> instantiations never name its arrays.  Gumbel
// root search (gc_tree_gumbel_enable: Gumbel-top-k, sequential halving, the improved policy) is
// k_tree_gumbel_begin, the <false, true> instantiation of k_tree_select -- only its level 0 differs
// -- and k_tree_gumbel_policy; no other instantiation names its arrays.
//
// Geometry: G games, `nodes` nodes per game, `cap` child slots per node (1..256).  Node k of game
// g is board g * nodes + k of the tree env; node 0 is the root.  Edge statistics live with the
// PARENT ([G][nodes][cap]: action, prior, child, edge_visits, edge_value), so one level of the
// descent is a handful of contiguous loads of one node's row -- no gather through child pointers.
// edge_value[j] is the sum of the backed-up values seen from the side to move at the parent.
//
// Mapping: one wave per game, lanes over the child slots (chunks of 64 when cap > 64), TREE_WAVES
// games per workgroup; no LDS (but advance's keep bitmap), no barrier, no atomics (a game is
// touched by its own wave only, so every result is deterministic).  For cap <= 64 a level of the
// descent is ONE round trip: the node's n_children and its visits / values / priors / children /
// actions rows are loaded together (the rows are cap long for every node, so lane < cap is in
// bounds before n_children is known) and the chosen child comes out of a lane, not out of memory.
//
// A node's rows are written when the node is created (k_tree_reset: the root; k_tree_backup: the
// new leaf), padding included; nodes at or past n_nodes hold whatever an earlier search left.
#pragma once
#include "gc_policy.h"

namespace gc {

#define TREE_WAVES 4  // games per workgroup
#define TREE_MAX_CAP 256
#define TREE_NO_ACTION 0xFFFFu

struct TreeDev {
    // [G][nodes][cap]
    uint16_t* action;
    float* prior;
    int32_t* child;
    int32_t* edge_visits;
    float* edge_value;
    // [G][nodes]
    int32_t* n_children;
    int32_t* parent;
    int32_t* parent_slot;
    float* leaf_value;
    uint8_t* terminal;
    // [G]
    int32_t* n_nodes;
    int32_t* overflow;
    int32_t* depth;     // entries of the pending path
    int32_t* leaf;      // the node the pending path ends at
    int32_t* leaf_new;  // 1: that node was allotted by the selection and is created by the backup
    int32_t* path;      // [G][nodes][2]: (node, slot) per level
    int games, nodes, cap;
};

// a block of child lists: policy_priors' output, row stride pri_cap
struct TreePriors {
    const uint16_t* actions;
    const float* priors;
    const int32_t* count;
    int pri_cap;
};

// The solver's arrays (gc_tree_solver_enable; the header has the rules): proofs of forced wins,
// draws and losses.  Status codes are seen from the side to move at the node / the side choosing
// among the node's edges.  Every kernel that reads them is the <true> instantiation of a template
// whose <false> one never names them, so a tree without the solver runs the code it always ran.
#define TREE_UNKNOWN 0
#define TREE_WIN 1
#define TREE_DRAW 2
#define TREE_LOSS 3
struct TreeSolverDev {
    uint8_t* edge_proven;  // [G][nodes][cap]
    uint16_t* edge_plies;  // [G][nodes][cap]
    uint8_t* node_proven;  // [G][nodes]
    uint16_t* node_plies;  // [G][nodes]
    uint8_t* complete;     // [G][nodes]
};

using TreeReduceI = hipcub::WarpReduce<int, 64>;
using TreeReduceD = hipcub::WarpReduce<double, 64>;
using TreeReduceU64 = hipcub::WarpReduce<unsigned long long, 64>;
__device__ __forceinline__ int tree_wave_sum(int v) {
    TreeReduceI::TempStorage ts;
    return __builtin_amdgcn_readfirstlane(TreeReduceI(ts).Sum(v));
}
__device__ __forceinline__ double tree_wave_sum(double v) {
    TreeReduceD::TempStorage ts;
    return __shfl(TreeReduceD(ts).Sum(v), 0, 64);
}
__device__ __forceinline__ unsigned long long tree_wave_max(unsigned long long v) {
    TreeReduceU64::TempStorage ts;
    return __shfl(TreeReduceU64(ts).Reduce(v, hipcub::Max()), 0, 64);
}

// Gumbel root search's arrays and parameters (gc_tree_gumbel_enable; the header has the rules).
// Only k_tree_gumbel_begin, k_tree_select<false, true> and k_tree_gumbel_policy name them, so a
// tree that is not armed runs the code it always ran.
struct TreeGumbelDev {
    float* gumbel;          // [G][cap]
    float* logit;           // [G][cap]
    int32_t* base_visits;   // [G][cap]
    const uint16_t* table;  // [considered + 1][sims]: the considered visit count per simulation
    int considered, sims;
    float c_visit, c_scale;
};
// one lane's slot of the root's rows: chunk 0 arrives in the caller's registers, with the node's
// other loads; a slot at or past nc holds ev 0, lg -inf
struct TreeGumbelSlot {
    int ev;
    float val, pr, gu, lg;
    int bv;
};
__device__ __forceinline__ TreeGumbelSlot tree_gumbel_load(const TreeDev& T, const TreeGumbelDev& U, int g, int nc,
                                                           int c, int lane, const TreeGumbelSlot& r0) {
    if (c == 0) return r0;
    TreeGumbelSlot r{0, 0.f, 0.f, 0.f, -__builtin_inff(), 0};
    const int s = c * 64 + lane;
    if (s < nc) {
        const size_t o = (size_t)g * T.nodes * T.cap + s, w = (size_t)g * T.cap + s;
        r.ev = T.edge_visits[o];
        r.val = T.edge_value[o];
        r.pr = T.prior[o];
        r.gu = U.gumbel[w];
        r.lg = U.logit[w];
        r.bv = U.base_visits[w];
    }
    return r;
}
// sigma(qhat) of a slot: the completed Q (the edge's mean, v_mix without a visit) times the scale
__device__ __forceinline__ float tree_gumbel_sigma(const TreeGumbelSlot& r, float vmix, float scale) {
    return scale * (r.ev > 0 ? r.val / (float)r.ev : vmix);
}

// The root's slot under the Gumbel rule (the header's "gc_tree_select on an armed tree"), for the
// wave of game g; S = the sum of the root's edge_visits, lv = leaf_value[root].  FINAL: the
// candidates are the slots with the most search visits (gc_tree_gumbel_policy's pick), otherwise
// those with the table's count.  v_mix's two sums are fp64 (exact for <= 256 fp32 terms but for
// denormal-sized ones), so v_mix is the rounding of the documented quotient.  -1 with NaN scores or
// no child.  *vmix and *scale are written for every nc.
template <bool FINAL>
__device__ __forceinline__ int tree_gumbel_slot(const TreeDev& T, const TreeGumbelDev& U, int g, int nc, int lane,
                                                const TreeGumbelSlot& r0, int S, float lv, float* vmix,
                                                float* scale) {
    const float ninf = -__builtin_inff();
    const int chunks = (nc + 63) >> 6;
    int t = 0, nmax = 0, vmax = 0;
    double num = 0.0, den = 0.0;
    for (int c = 0; c < chunks; c++) {
        const TreeGumbelSlot r = tree_gumbel_load(T, U, g, nc, c, lane, r0);
        if (c * 64 + lane >= nc) continue;
        const int v = r.ev - r.bv;
        t += v;
        nmax = r.ev > nmax ? r.ev : nmax;
        vmax = v > vmax ? v : vmax;
        if (r.ev > 0) {
            den += (double)r.pr;
            num += (double)r.pr * ((double)r.val / (double)r.ev);
        }
    }
    TreeReduceI::TempStorage ts;
    nmax = __builtin_amdgcn_readfirstlane(TreeReduceI(ts).Reduce(nmax, hipcub::Max()));
    den = tree_wave_sum(den);
    num = tree_wave_sum(num);
    const float vm = S > 0 && den != 0.0 ? (float)(((double)lv + (double)S * (num / den)) / (1.0 + (double)S)) : lv;
    const float sc = (U.c_visit + (float)nmax) * U.c_scale;
    *vmix = vm;
    *scale = sc;
    int want;  // the search visits of a candidate
    if (FINAL) {
        want = __builtin_amdgcn_readfirstlane(TreeReduceI(ts).Reduce(vmax, hipcub::Max()));
    } else {
        t = tree_wave_sum(t);
        t = t < 0 ? 0 : t < U.sims ? t : U.sims - 1;
        const int k = U.considered < nc ? U.considered : nc;
        want = __builtin_amdgcn_readfirstlane((int)U.table[(size_t)k * U.sims + t]);
    }
    bool any = false;
    for (int c = 0; c < chunks; c++) {
        const TreeGumbelSlot r = tree_gumbel_load(T, U, g, nc, c, lane, r0);
        any |= __ballot(c * 64 + lane < nc && r.ev - r.bv == want) != 0;
    }
    float best = ninf;
    int j = -1;
    for (int c = 0; c < chunks; c++) {
        const TreeGumbelSlot r = tree_gumbel_load(T, U, g, nc, c, lane, r0);
        const bool on = c * 64 + lane < nc && (!any || r.ev - r.bv == want);
        const float x = on ? (r.gu + r.lg) + tree_gumbel_sigma(r, vm, sc) : ninf;
        const float mx = pol_wave_max(x);
        const unsigned long long hit = __ballot(on && x == mx);
        if (hit && (j < 0 || mx > best)) {  // an earlier chunk keeps a tie
            best = mx;
            j = c * 64 + (int)__builtin_ctzll(hit);
        }
    }
    return j;
}

// node `node` of game g (all rows written): its child list = the first min(count, pri_cap, cap)
// entries of row g of P (none, and the row unread, when !listed: a terminal node), edges zeroed,
// children -1
__device__ __forceinline__ void tree_init_node(const TreeDev& T, int g, int node, const TreePriors& P, bool listed,
                                               int lane) {
    int m = 0;
    if (listed) {
        m = P.count[g];
        m = m < P.pri_cap ? m : P.pri_cap;
        m = m < T.cap ? m : T.cap;
        m = m > 0 ? m : 0;
    }
    const size_t nb = (size_t)g * T.nodes + node, o = nb * T.cap, src = (size_t)g * P.pri_cap;
    for (int s = lane; s < T.cap; s += 64) {
        const bool on = s < m;
        T.action[o + s] = on ? P.actions[src + s] : (uint16_t)TREE_NO_ACTION;
        T.prior[o + s] = on ? P.priors[src + s] : 0.f;
        T.child[o + s] = -1;
        T.edge_visits[o + s] = 0;
        T.edge_value[o + s] = 0.f;
    }
    if (lane == 0) T.n_children[nb] = m;
}

// complete iff the list holds every legal move: the row's count fits both the block and the
// tree's cap; a terminal node (!listed, the row unread) counts as complete.  (Called before
// tree_init_node's stores, so that the count's load is one with its own.)
__device__ __forceinline__ bool tree_row_complete(const TreeDev& T, int g, const TreePriors& P, bool listed) {
    if (!listed) return true;
    const int c = P.count[g];
    return c >= 0 && c <= P.pri_cap && c <= T.cap;
}

// the solver's part of a new node: no edge proven; `status`: TREE_UNKNOWN, or a terminal node's
// verdict, plies 0
__device__ __forceinline__ void tree_solver_init_node(const TreeDev& T, const TreeSolverDev& V, int g, int node,
                                                      bool complete, int status, int lane) {
    const size_t nb = (size_t)g * T.nodes + node, o = nb * T.cap;
    for (int s = lane; s < T.cap; s += 64) {
        V.edge_proven[o + s] = TREE_UNKNOWN;
        V.edge_plies[o + s] = 0;
    }
    if (lane == 0) {
        V.complete[nb] = complete ? 1 : 0;
        V.node_proven[nb] = (uint8_t)status;
        V.node_plies[nb] = 0;
    }
}

// game g a single root with the child list of row g of P
template <bool SOLVER>
__device__ __forceinline__ void tree_reset_game(const TreeDev& T, const TreeSolverDev& V, int g, const TreePriors& P,
                                                const float* value, int lane) {
    bool complete = false;
    if constexpr (SOLVER) complete = tree_row_complete(T, g, P, true);
    tree_init_node(T, g, 0, P, true, lane);
    if constexpr (SOLVER) tree_solver_init_node(T, V, g, 0, complete, TREE_UNKNOWN, lane);
    if (lane == 0) {
        const size_t nb = (size_t)g * T.nodes;
        T.parent[nb] = -1;
        T.parent_slot[nb] = -1;
        T.leaf_value[nb] = value ? value[g] : 0.f;
        T.terminal[nb] = 0;
        T.n_nodes[g] = 1;
        T.overflow[g] = 0;
        T.depth[g] = 0;
        T.leaf[g] = 0;
        T.leaf_new[g] = 0;
    }
}

// every game a single root with the child list of row g of P
template <bool SOLVER>
__global__ __launch_bounds__(64 * TREE_WAVES) void k_tree_reset(const TreeDev T, const TreePriors P,
                                                                 const float* __restrict__ value,
                                                                 const TreeSolverDev V) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (g >= T.games) return;
    tree_reset_game<SOLVER>(T, V, g, P, value, lane);
}

// the proof's slot among the first nc edges of the row at o: the edge of status `want` with the
// fewest plies (TREE_WIN) or the most (TREE_LOSS), ties to the lowest slot; -1 without such an edge
__device__ __forceinline__ int tree_proof_slot(const TreeSolverDev& V, size_t o, int nc, int want, int lane) {
    unsigned long long key = 0;  // plies (a WIN's: 0xFFFF - plies) << 32 | ~slot; 0 = no such edge
    for (int s = lane; s < nc; s += 64) {
        if ((int)V.edge_proven[o + s] != want) continue;
        const u32 pl = V.edge_plies[o + s];
        const unsigned long long mine =
            ((unsigned long long)(want == TREE_WIN ? 0xFFFFu - pl : pl) << 32) | (0xFFFFFFFFu - (u32)s);
        key = mine > key ? mine : key;
    }
    key = tree_wave_max(key);
    return __builtin_amdgcn_readfirstlane(key ? (int)(0xFFFFFFFFu - (u32)key) : -1);
}

// the node rule over the first nc edges of the row at o, with edge j taken as (sj, pj) from the
// caller's registers (the row's stored entry j is not read): status | plies << 8, wave-uniform
__device__ __forceinline__ u32 tree_node_rule(const TreeSolverDev& V, size_t o, int nc, bool complete, int j, int sj,
                                              int pj, int lane) {
    int wmin = 0x10000, amax = 0;
    bool unknown = false, draw = false;
    for (int s = lane; s < nc; s += 64) {
        const int st = s == j ? sj : (int)V.edge_proven[o + s];
        const int pl = s == j ? pj : (int)V.edge_plies[o + s];
        if (st == TREE_WIN) wmin = pl < wmin ? pl : wmin;
        unknown |= st == TREE_UNKNOWN;
        draw |= st == TREE_DRAW;
        amax = pl > amax ? pl : amax;
    }
    TreeReduceI::TempStorage ts;
    wmin = __builtin_amdgcn_readfirstlane(TreeReduceI(ts).Reduce(wmin, hipcub::Min()));
    if (wmin < 0x10000) return TREE_WIN | (u32)wmin << 8;
    if (!complete || __ballot(unknown)) return TREE_UNKNOWN;
    if (__ballot(draw)) return TREE_DRAW;
    amax = __builtin_amdgcn_readfirstlane(TreeReduceI(ts).Reduce(amax, hipcub::Max()));
    return TREE_LOSS | (u32)amax << 8;
}

// PUCT descent of every game to one leaf (the header's contract has the rule and the three ways
// it ends).  score_j = Q_j + c_puct * prior_j * sqrt(n_k) / (1 + visits_j) in fp32, in exactly
// this order of operations; the largest score wins, ties to the lowest slot.
// SOLVER: the node's edge_proven row joins the loads of the level's one round trip.  A proven
// edge scores with Q = +1 / 0 / -1, LOSS edges leave the argmax unless all are LOSS, a node with
// a WIN edge (only ever the root) takes the proof's slot, and a descent that chooses a proven edge
// ends at its child (the header's "Select on a solver tree").
// GUMBEL (an armed tree, never with SOLVER): level 0 takes the slot of tree_gumbel_slot; its three
// [cap] rows and the root's leaf_value join the loads of the level's round trip (the table entry
// is one dependent load more, of a few hundred bytes every wave shares).  Every deeper level, the
// path and the three endings are the code below, unchanged.
template <bool SOLVER, bool GUMBEL = false>
__global__ __launch_bounds__(64 * TREE_WAVES) void k_tree_select(const TreeDev T, float c_puct, float fpu,
                                                                  int32_t* __restrict__ out_parent,
                                                                  int32_t* __restrict__ out_child,
                                                                  uint16_t* __restrict__ out_action,
                                                                  const TreeSolverDev V, const TreeGumbelDev U) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (g >= T.games) return;
    const float ninf = -__builtin_inff();
    const size_t gb = (size_t)g * T.nodes;
    const int nn = __builtin_amdgcn_readfirstlane(T.n_nodes[g]);
    int32_t* path = T.path + gb * 2;
    int k = 0, D = 0, leaf = 0, is_new = 0;
    int o_parent = -1, o_child = -1;
    u32 o_action = TREE_NO_ACTION;
    // (D < nodes always holds in a tree -- a path visits distinct nodes --; the test bounds the
    // loop and the path's stores whatever the arrays hold)
    while (D < T.nodes) {
        const size_t o = (gb + k) * T.cap;
        // chunk 0 of the node's rows together with its child count: one round trip
        const bool in0 = lane < T.cap;
        // (SOLVER: issued first and without a branch -- slot 0 exists in every row -- so that it
        // is in flight with the others; a lane at or past nc holds a value nothing below reads)
        int ep0 = TREE_UNKNOWN;
        if constexpr (SOLVER) ep0 = (int)V.edge_proven[o + (in0 ? lane : 0)];
        int nc = __builtin_amdgcn_readfirstlane(T.n_children[gb + k]);
        nc = nc < T.cap ? nc : T.cap;
        int ev0 = in0 ? T.edge_visits[o + lane] : 0;
        const float val0 = in0 ? T.edge_value[o + lane] : 0.f;
        const float pr0 = in0 ? T.prior[o + lane] : 0.f;
        const int ch0 = in0 ? T.child[o + lane] : -1;
        const u32 ac0 = in0 ? T.action[o + lane] : TREE_NO_ACTION;
        TreeGumbelSlot g0{};
        float lv0 = 0.f;
        if constexpr (GUMBEL) {
            if (D == 0) {  // (without a branch on the lane, like ep0)
                const size_t w = (size_t)g * T.cap + (in0 ? lane : 0);
                g0.gu = U.gumbel[w];
                g0.lg = U.logit[w];
                g0.bv = U.base_visits[w];
                lv0 = T.leaf_value[gb];
            }
        }
        if (nc <= 0) break;  // (b) a terminal or childless node: the path ends here
        if (lane >= nc) ev0 = 0;
        const int chunks = (nc + 63) >> 6;
        int total = ev0;
        for (int c = 1; c < chunks; c++) {
            const int s = c * 64 + lane;
            total += s < nc ? T.edge_visits[o + s] : 0;
        }
        total = tree_wave_sum(total);
        const float sq = sqrtf((float)(1 + total));
        auto score = [&](int ev, float val, float pr, int ep) {
            float q = ev ? val / (float)ev : fpu;
            if constexpr (SOLVER) q = ep == TREE_UNKNOWN ? q : ep == TREE_WIN ? 1.0f : ep == TREE_DRAW ? 0.0f : -1.0f;
            return q + c_puct * pr * sq / (float)(1 + ev);
        };
        // SOLVER: the edges left out of the argmax (LOSS, unless every edge is), and a WIN edge
        bool drop_loss = false, won = false;
        if constexpr (SOLVER) {
            int n_loss = __popcll(__ballot(lane < nc && ep0 == TREE_LOSS));
            won = __ballot(lane < nc && ep0 == TREE_WIN) != 0;
            for (int c = 1; c < chunks; c++) {
                const int s = c * 64 + lane;
                const int ep = s < nc ? (int)V.edge_proven[o + s] : TREE_UNKNOWN;
                n_loss += __popcll(__ballot(ep == TREE_LOSS));
                won |= __ballot(ep == TREE_WIN) != 0;
            }
            drop_loss = n_loss < nc;
        }
        float best = ninf;
        int j = -1;
        if (GUMBEL && D == 0) {  // the root of an armed tree
            if constexpr (GUMBEL) {
                g0.ev = ev0;
                g0.val = val0;
                g0.pr = pr0;
                if (lane >= nc) g0.lg = ninf;
                float vmix, scale;
                j = tree_gumbel_slot<false>(T, U, g, nc, lane, g0, total, lv0, &vmix, &scale);
            }
        } else if (SOLVER && won) {
            j = tree_proof_slot(V, o, nc, TREE_WIN, lane);
        } else {
            {
                const bool on = lane < nc && !(SOLVER && drop_loss && ep0 == TREE_LOSS);
                const float sc = on ? score(ev0, val0, pr0, ep0) : ninf;
                const float mx = pol_wave_max(sc);
                const unsigned long long hit = __ballot(on && sc == mx);
                if (hit) {
                    best = mx;
                    j = (int)__builtin_ctzll(hit);
                }
            }
            for (int c = 1; c < chunks; c++) {
                const int s = c * 64 + lane;
                int ep = TREE_UNKNOWN;
                if constexpr (SOLVER) ep = s < nc ? (int)V.edge_proven[o + s] : TREE_UNKNOWN;
                const bool on = s < nc && !(SOLVER && drop_loss && ep == TREE_LOSS);
                const float sc = on ? score(T.edge_visits[o + s], T.edge_value[o + s], T.prior[o + s], ep) : ninf;
                const float mx = pol_wave_max(sc);
                const unsigned long long hit = __ballot(on && sc == mx);
                if (hit && (j < 0 || mx > best)) {  // an earlier chunk keeps a tie
                    best = mx;
                    j = c * 64 + (int)__builtin_ctzll(hit);
                }
            }
        }
        if (j < 0) j = 0;  // (only with NaN scores: some slot, in bounds)
        int ch, epj = TREE_UNKNOWN;
        u32 ac;
        if (j < 64) {
            ch = __builtin_amdgcn_readfirstlane(__shfl(ch0, j, 64));
            ac = __builtin_amdgcn_readfirstlane(__shfl(ac0, j, 64));
            if constexpr (SOLVER) epj = __builtin_amdgcn_readfirstlane(__shfl(ep0, j, 64));
        } else {
            ch = __builtin_amdgcn_readfirstlane(T.child[o + j]);
            ac = __builtin_amdgcn_readfirstlane((u32)T.action[o + j]);
            if constexpr (SOLVER) epj = __builtin_amdgcn_readfirstlane((int)V.edge_proven[o + j]);
        }
        if (lane == 0) {
            path[2 * D] = k;
            path[2 * D + 1] = j;
        }
        D++;
        if (SOLVER && epj != TREE_UNKNOWN && ch >= 0 && ch < T.nodes) {  // a proven edge: the path ends at its child
            leaf = ch;
            k = -1;
            break;
        }
        if (ch >= 0 && ch < T.nodes) {  // descend
            k = ch;
            continue;
        }
        if (nn < T.nodes) {  // (a) a new leaf
            leaf = nn;
            is_new = 1;
            o_parent = (int)(gb + k);
            o_child = (int)(gb + nn);
            o_action = ac;
        } else {  // (c) the game's tree is full: the path ends at k
            D--;
            leaf = k;
            if (lane == 0) T.overflow[g] += 1;
        }
        k = -1;
        break;
    }
    if (k >= 0) leaf = k;  // (b)
    if (lane == 0) {
        if (is_new) T.n_nodes[g] = nn + 1;
        T.depth[g] = D;
        T.leaf[g] = leaf;
        T.leaf_new[g] = is_new;
        out_parent[g] = o_parent;
        out_child[g] = o_child;
        out_action[g] = (uint16_t)o_action;
    }
}

// A new terminal leaf's verdict carried up the pending path (the header's "Propagation"), by the
// game's own wave.  Ordering: nothing a lane stores here is loaded by another lane of this launch.
//  * the status of the node below (first the leaf's, from done / reason; then node k's, just
//    recomputed) travels from level to level in wave-uniform registers, never through node_proven;
//  * edge (k, j) is stored by the lane that owns slot j and enters the node rule from registers
//    (tree_node_rule takes it as an argument and skips the stored entry);
//  * every other entry of k's rows, n_children[k], complete[k] and the stored verdict of k that
//    step 5 compares with were written by EARLIER launches: a path holds distinct nodes, none of
//    them the leaf, so this launch has stored nothing of k before level d is reached;
//  * the path itself was written by the select launch.
// So the stream's kernel boundary is the only ordering needed: no fence, no atomics.
__device__ __forceinline__ void tree_propagate(const TreeDev& T, const TreeSolverDev& V, size_t gb,
                                               const int32_t* path, int D, int status, int lane) {
    int cs = status, cp = 0;  // the node below: its status and plies
    for (int d = D - 1; d >= 0 && cs != TREE_UNKNOWN; d--) {
        const int k = __builtin_amdgcn_readfirstlane(path[2 * d]), j = __builtin_amdgcn_readfirstlane(path[2 * d + 1]);
        if ((unsigned)k >= (unsigned)T.nodes || (unsigned)j >= (unsigned)T.cap) break;
        const size_t o = (gb + k) * T.cap;
        int nc = __builtin_amdgcn_readfirstlane(T.n_children[gb + k]);
        nc = nc < T.cap ? nc : T.cap;
        const bool complete = __builtin_amdgcn_readfirstlane((int)V.complete[gb + k]) != 0;
        const int os = __builtin_amdgcn_readfirstlane((int)V.node_proven[gb + k]);
        const int op = __builtin_amdgcn_readfirstlane((int)V.node_plies[gb + k]);
        const int es = cs == TREE_WIN ? TREE_LOSS : cs == TREE_LOSS ? TREE_WIN : cs;
        const int ep = cp + 1 < 65535 ? cp + 1 : 65535;
        if (lane == (j & 63)) {
            V.edge_proven[o + j] = (uint8_t)es;
            V.edge_plies[o + j] = (uint16_t)ep;
        }
        const u32 r = tree_node_rule(V, o, nc, complete, j, es, ep, lane);
        const int ns = (int)(r & 0xFFu), np = (int)(r >> 8);
        if (ns == os && np == op) break;
        if (lane == 0) {
            V.node_proven[gb + k] = (uint8_t)ns;
            V.node_plies[gb + k] = (uint16_t)np;
        }
        cs = ns;
        cp = np;
    }
}

// the pending leaf created (a new one) and its value added along the pending path
// SOLVER: a new node gets its solver rows, a new terminal one is propagated, and a proven leaf is
// worth its verdict
template <bool SOLVER>
__global__ __launch_bounds__(64 * TREE_WAVES) void k_tree_backup(const TreeDev T, const float* __restrict__ value,
                                                                  const uint8_t* __restrict__ done,
                                                                  const uint8_t* __restrict__ reason,
                                                                  const TreePriors P, const TreeSolverDev V) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (g >= T.games) return;
    const size_t gb = (size_t)g * T.nodes;
    const int D = T.depth[g], L = T.leaf[g];
    const int32_t* path = T.path + gb * 2;
    if (D < 0 || D > T.nodes || L < 0 || L >= T.nodes) return;  // (never with a selection pending)
    float v;
    if (T.leaf_new[g]) {
        const bool fin = done[g] != 0;
        v = fin ? (reason[g] == 1 ? -1.0f : 0.0f) : value[g];  // reason 1: the side to move at L is mated
        bool complete = false;
        if constexpr (SOLVER) complete = tree_row_complete(T, g, P, !fin);
        tree_init_node(T, g, L, P, !fin, lane);
        if (lane == 0 && D > 0) {
            const int pk = path[2 * (D - 1)], pj = path[2 * (D - 1) + 1];
            T.parent[gb + L] = pk;
            T.parent_slot[gb + L] = pj;
            T.leaf_value[gb + L] = v;
            T.terminal[gb + L] = fin ? 1 : 0;
            if ((unsigned)pk < (unsigned)T.nodes && (unsigned)pj < (unsigned)T.cap) T.child[(gb + pk) * T.cap + pj] = L;
        }
        if constexpr (SOLVER) {
            const int status = fin ? (reason[g] == 1 ? TREE_LOSS : TREE_DRAW) : TREE_UNKNOWN;
            tree_solver_init_node(T, V, g, L, complete, status, lane);
            if (fin) tree_propagate(T, V, gb, path, D, status, lane);
        }
    } else {
        v = T.leaf_value[gb + L];
        if constexpr (SOLVER) {
            const int st = V.node_proven[gb + L];
            v = st == TREE_UNKNOWN ? v : st == TREE_WIN ? 1.0f : st == TREE_DRAW ? 0.0f : -1.0f;
        }
    }
    // one lane per path entry: the entries name distinct nodes, so the stores are independent
    for (int d = lane; d < D; d += 64) {
        const int k = path[2 * d], j = path[2 * d + 1];
        if ((unsigned)k >= (unsigned)T.nodes || (unsigned)j >= (unsigned)T.cap) continue;
        const size_t e = (gb + k) * T.cap + j;
        T.edge_visits[e] += 1;
        T.edge_value[e] += ((D - d) & 1) ? -v : v;
    }
}

// ---------------------------------------------------------------------------------------------
// Several leaves per game per call, with virtual loss (gc_tree_select_batch / gc_tree_backup_batch;
// the header's contract has the rule and the four ways a descent ends).  The scratch of
// gc_tree_batch_reserve, K = the reserved leaves per game:
struct TreeBatchDev {
    uint8_t* inflight;    // [G][nodes][cap]: descents of the pending batch that hold this edge
    int32_t* path;        // [G][K][nodes][2]
    int32_t* depth;       // [G][K]
    int32_t* leaf;        // [G][K]
    int32_t* kind;        // [G][K]: 0 an existing node, 1 a new node, 2 a collision
    int32_t* collisions;  // [G]
    int K;
};

// The descents l = 0 .. leaves - 1 of a game run one after another inside the game's wave.  The
// only value a descent leaves for a later one of the same launch is inflight[k][j], and it never
// crosses lanes through memory: the lane that owns slot j (j & 63) stores the incremented byte and
// the same lane is the one that loads it in a later descent, so that lane's own program order is
// the ordering -- no fence.  Whether the chosen edge was in flight comes out of its owner's
// register by a shuffle, like the child and the action.  n_nodes, overflow and collisions live in
// registers for the whole batch and are stored once at the end; a node allotted in this batch is
// never entered by a later descent, because its parent's child[j] stays -1 until the backup.
// For cap <= 64 a level is still one round trip: inflight's row joins the loads issued together.
// With every inflight byte 0 the score is k_tree_select's bit for bit (val - vloss * 0 == val,
// contracted or not).
__global__ __launch_bounds__(64 * TREE_WAVES) void k_tree_select_batch(const TreeDev T, const TreeBatchDev B,
                                                                        int leaves, float c_puct, float fpu,
                                                                        float vloss, int32_t* __restrict__ out_parent,
                                                                        int32_t* __restrict__ out_child,
                                                                        uint16_t* __restrict__ out_action) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (g >= T.games) return;
    const float ninf = -__builtin_inff();
    const size_t gb = (size_t)g * T.nodes;
    int nn = __builtin_amdgcn_readfirstlane(T.n_nodes[g]);
    int over = 0, coll = 0;
    for (int l = 0; l < leaves; l++) {
        int32_t* path = B.path + ((size_t)g * B.K + l) * T.nodes * 2;
        int k = 0, D = 0, leaf = 0, kind = 0;
        int o_parent = -1, o_child = -1;
        u32 o_action = TREE_NO_ACTION;
        while (D < T.nodes) {
            const size_t o = (gb + k) * T.cap;
            // chunk 0 of the node's rows, its in-flight row and its child count: one round trip
            const bool in0 = lane < T.cap;
            int nc = __builtin_amdgcn_readfirstlane(T.n_children[gb + k]);
            nc = nc < T.cap ? nc : T.cap;
            int ev0 = in0 ? T.edge_visits[o + lane] : 0;
            int if0 = in0 ? (int)B.inflight[o + lane] : 0;
            const float val0 = in0 ? T.edge_value[o + lane] : 0.f;
            const float pr0 = in0 ? T.prior[o + lane] : 0.f;
            const int ch0 = in0 ? T.child[o + lane] : -1;
            const u32 ac0 = in0 ? T.action[o + lane] : TREE_NO_ACTION;
            if (nc <= 0) break;  // (b) a terminal or childless node: the path ends here
            if (lane >= nc) ev0 = if0 = 0;
            const int chunks = (nc + 63) >> 6;
            int total = ev0 + if0;
            for (int c = 1; c < chunks; c++) {
                const int s = c * 64 + lane;
                total += s < nc ? T.edge_visits[o + s] + (int)B.inflight[o + s] : 0;
            }
            total = tree_wave_sum(total);
            const float sq = sqrtf((float)(1 + total));
            auto score = [&](int ev, int f, float val, float pr) {
                const int n = ev + f;
                const float q = n ? (val - vloss * (float)f) / (float)n : fpu;
                return q + c_puct * pr * sq / (float)(1 + n);
            };
            float best = ninf;
            int j = -1;
            {
                const bool on = lane < nc;
                const float sc = on ? score(ev0, if0, val0, pr0) : ninf;
                const float mx = pol_wave_max(sc);
                const unsigned long long hit = __ballot(on && sc == mx);
                if (hit) {
                    best = mx;
                    j = (int)__builtin_ctzll(hit);
                }
            }
            for (int c = 1; c < chunks; c++) {
                const int s = c * 64 + lane;
                const bool on = s < nc;
                const float sc =
                    on ? score(T.edge_visits[o + s], (int)B.inflight[o + s], T.edge_value[o + s], T.prior[o + s]) : ninf;
                const float mx = pol_wave_max(sc);
                const unsigned long long hit = __ballot(on && sc == mx);
                if (hit && (j < 0 || mx > best)) {  // an earlier chunk keeps a tie
                    best = mx;
                    j = c * 64 + (int)__builtin_ctzll(hit);
                }
            }
            if (j < 0) j = 0;  // (only with NaN scores: some slot, in bounds)
            // the chosen slot's child, action and in-flight count from the lane that owns the slot
            const bool mine = lane == (j & 63);
            int ch, fj;
            u32 ac;
            if (j < 64) {
                ch = ch0, ac = ac0, fj = if0;
            } else {
                ch = mine ? T.child[o + j] : -1;
                ac = mine ? (u32)T.action[o + j] : TREE_NO_ACTION;
                fj = mine ? (int)B.inflight[o + j] : 0;
            }
            ch = __builtin_amdgcn_readfirstlane(__shfl(ch, j & 63, 64));
            ac = __builtin_amdgcn_readfirstlane(__shfl(ac, j & 63, 64));
            fj = __builtin_amdgcn_readfirstlane(__shfl(fj, j & 63, 64));
            if (lane == 0) {
                path[2 * D] = k;
                path[2 * D + 1] = j;
            }
            const bool down = ch >= 0 && ch < T.nodes;
            if (!down && fj == 0 && nn >= T.nodes) {  // (c) the game's tree is full: the path ends at k, no mark
                leaf = k;
                over++;
                k = -1;
                break;
            }
            if (mine) B.inflight[o + j] = (uint8_t)(fj + 1);
            D++;
            if (down) {  // descend
                k = ch;
                continue;
            }
            if (fj > 0) {  // (d) an earlier descent of this batch holds the edge
                leaf = k;
                kind = 2;
                coll++;
            } else {  // (a) a new leaf
                leaf = nn;
                kind = 1;
                o_parent = (int)(gb + k);
                o_child = (int)(gb + nn);
                o_action = ac;
                nn++;
            }
            k = -1;
            break;
        }
        if (k >= 0) leaf = k;  // (b)
        if (lane == 0) {
            const size_t r = (size_t)g * B.K + l, w = (size_t)g * leaves + l;
            B.depth[r] = D;
            B.leaf[r] = leaf;
            B.kind[r] = kind;
            out_parent[w] = o_parent;
            out_child[w] = o_child;
            out_action[w] = (uint16_t)o_action;
        }
    }
    if (lane == 0) {
        T.n_nodes[g] = nn;
        if (over) T.overflow[g] += over;
        if (coll) B.collisions[g] += coll;
    }
}

// The batch's new nodes created and every descent's value added along its path, l ascending: one
// fp32 add per edge per descent, no atomics, in a fixed order.  An edge sits at the same depth d in
// every path that contains it (the tree path from the root to its node is unique), so lane d & 63
// owns it in every descent: with l on the outside and the lanes over d on the inside, the
// read-modify-writes of one edge -- edge_visits, edge_value and the in-flight byte -- are all one
// lane's, in that lane's program order; no fence.  A descent's value stays in a register (a new
// node's leaf_value is stored, never read back here), and a new node's rows are no path entry of
// this batch, so creating node l inside the loop over l orders nothing.
__global__ __launch_bounds__(64 * TREE_WAVES) void k_tree_backup_batch(const TreeDev T, const TreeBatchDev B,
                                                                        int leaves, const float* __restrict__ value,
                                                                        const uint8_t* __restrict__ done,
                                                                        const uint8_t* __restrict__ reason,
                                                                        const TreePriors P) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (g >= T.games) return;
    const size_t gb = (size_t)g * T.nodes;
    for (int l = 0; l < leaves; l++) {
        const size_t r = (size_t)g * B.K + l, w = (size_t)g * leaves + l;
        const int D = B.depth[r], L = B.leaf[r], kind = B.kind[r];
        const int32_t* path = B.path + r * T.nodes * 2;
        if (D < 0 || D > T.nodes || L < 0 || L >= T.nodes) continue;  // (never with a batch pending)
        float v = 0.f;
        if (kind == 1) {
            const bool fin = done[w] != 0;
            v = fin ? (reason[w] == 1 ? -1.0f : 0.0f) : value[w];  // reason 1: the side to move at L is mated
            // row w of the block, seen as row g by tree_init_node
            const size_t sh = w - (size_t)g;
            const TreePriors Pw{P.actions + sh * P.pri_cap, P.priors + sh * P.pri_cap, P.count + sh, P.pri_cap};
            tree_init_node(T, g, L, Pw, !fin, lane);
            if (lane == 0 && D > 0) {
                const int pk = path[2 * (D - 1)], pj = path[2 * (D - 1) + 1];
                T.parent[gb + L] = pk;
                T.parent_slot[gb + L] = pj;
                T.leaf_value[gb + L] = v;
                T.terminal[gb + L] = fin ? 1 : 0;
                if ((unsigned)pk < (unsigned)T.nodes && (unsigned)pj < (unsigned)T.cap) T.child[(gb + pk) * T.cap + pj] = L;
            }
        } else if (kind != 2) {
            v = T.leaf_value[gb + L];  // (a node of an earlier launch)
        }
        for (int d = lane; d < D; d += 64) {
            const int k = path[2 * d], j = path[2 * d + 1];
            if ((unsigned)k >= (unsigned)T.nodes || (unsigned)j >= (unsigned)T.cap) continue;
            const size_t e = (gb + k) * T.cap + j;
            B.inflight[e] -= 1;
            if (kind == 2) continue;
            T.edge_visits[e] += 1;
            T.edge_value[e] += ((D - d) & 1) ? -v : v;
        }
    }
}

struct TreeRootArgs {
    uint64_t seed;
    u32 draw;
    int greedy;
    uint16_t* actions;  // [G][cap], may be NULL
    int32_t* visits;    // [G][cap], may be NULL
    float* pi;          // [G][cap], may be NULL
    uint16_t* pick;     // [G], may be NULL
    float* value;       // [G], may be NULL
    int proof;          // flag bit 1 (a solver tree only): the pick respects the root's proofs
};

// the root's visit counts, their distribution, the root value and a move per game
// SOLVER with A.proof: only the pick changes (the header's "Root policy, flag bit 1").  `fixed`
// is the slot a proof decides alone (a WIN edge; all edges LOSS; candidates without visits);
// otherwise the greedy / sampled rule below runs over the candidates' visits (a LOSS edge counts
// as 0 visits and is never chosen), which for a tree without proofs are all the visits.
template <bool SOLVER>
__global__ __launch_bounds__(64 * TREE_WAVES) void k_tree_root_policy(const TreeDev T, const TreeRootArgs A,
                                                                       const TreeSolverDev V) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (g >= T.games) return;
    const size_t o = (size_t)g * T.nodes * T.cap, w = (size_t)g * T.cap;
    int nc = T.n_children[(size_t)g * T.nodes];
    nc = nc < T.cap ? nc : T.cap;
    const int chunks = (T.cap + 63) >> 6;
    int total = 0;
    double vsum = 0.0;  // (in fp64 the sum of <= 256 fp32 values is exact but for denormal-sized terms)
    for (int c = 0; c < chunks; c++) {
        const int s = c * 64 + lane;
        if (s < nc) {
            total += T.edge_visits[o + s];
            vsum += (double)T.edge_value[o + s];
        }
    }
    total = tree_wave_sum(total);
    vsum = tree_wave_sum(vsum);
    if (lane == 0 && A.value) A.value[g] = total > 0 ? (float)(vsum / (double)total) : 0.f;
    const bool proof = SOLVER && A.proof;
    int ptotal = total;  // the visits the pick is drawn from
    bool fixed = false;
    u32 pick = TREE_NO_ACTION;
    if constexpr (SOLVER) {
        if (proof) {
            int cv = 0, first = TREE_MAX_CAP;  // the candidates' visits, the lowest candidate slot
            bool won = false;
            for (int c = 0; c < chunks; c++) {
                const int s = c * 64 + lane;
                const int ep = s < nc ? (int)V.edge_proven[o + s] : TREE_LOSS;
                const unsigned long long cand = __ballot(s < nc && ep != TREE_LOSS);
                won |= __ballot(s < nc && ep == TREE_WIN) != 0;
                if (cand && first == TREE_MAX_CAP) first = c * 64 + (int)__builtin_ctzll(cand);
                cv += s < nc && ep != TREE_LOSS ? T.edge_visits[o + s] : 0;
            }
            ptotal = tree_wave_sum(cv);
            int slot = -1;
            if (won) {
                slot = tree_proof_slot(V, o, nc, TREE_WIN, lane);
            } else if (first == TREE_MAX_CAP) {
                slot = tree_proof_slot(V, o, nc, TREE_LOSS, lane);
            } else if (ptotal == 0) {
                slot = total > 0 ? first : -1;
            }
            fixed = won || first == TREE_MAX_CAP || ptotal == 0;
            if (slot >= 0 && slot < nc) pick = T.action[o + slot];
        }
    }
    // greedy: the most visited slot, ties to the lowest; sampled: the first slot whose inclusive
    // visit prefix exceeds r = ((x0 >> 8) * total) >> 24, the sampler's Philox word (gc_policy.h)
    const u64 r = ptotal > 0 ? (((u64)(philox_x0(A.seed, (u32)g, A.draw) >> 8) * (u64)ptotal) >> 24) : 0;
    unsigned long long key = 0;  // visits << 32 | ~slot
    u32 carry = 0;
    for (int c = 0; c < chunks; c++) {
        const int s = c * 64 + lane;
        const bool in = s < T.cap, on = s < nc;
        const int ev = on ? T.edge_visits[o + s] : 0;
        const u32 ac = on ? T.action[o + s] : TREE_NO_ACTION;
        if (in) {
            if (A.actions) A.actions[w + s] = (uint16_t)ac;
            if (A.visits) A.visits[w + s] = ev;
            if (A.pi) A.pi[w + s] = total > 0 ? (float)ev / (float)total : 0.f;
        }
        bool can = on;  // a candidate of the pick
        if constexpr (SOLVER) can = on && !(proof && V.edge_proven[o + s] == TREE_LOSS);
        const int pv = can ? ev : 0;
        if (A.greedy) {
            const unsigned long long mine = can ? ((unsigned long long)(u32)pv << 32) | (0xFFFFFFFFu - (u32)s) : 0ull;
            key = mine > key ? mine : key;
        } else {
            const u32 incl = carry + pol_wave_scan((u32)pv);
            const unsigned long long hit = __ballot(can && (u64)incl > r && (u64)(incl - (u32)pv) <= r);
            if (hit && pick == TREE_NO_ACTION && ptotal > 0 && !fixed) pick = __shfl(ac, (int)__builtin_ctzll(hit), 64);
            carry = __shfl(incl, 63, 64);
        }
    }
    if (A.greedy && ptotal > 0 && !fixed) {
        key = tree_wave_max(key);
        const int s = (int)(0xFFFFFFFFu - (u32)key);
        if (s >= 0 && s < nc) pick = T.action[o + s];
    }
    if (lane == 0 && A.pick) A.pick[g] = (uint16_t)pick;
}

// the root's status, its plies and the proof's move per game (the header's gc_tree_root_proof)
__global__ __launch_bounds__(64 * TREE_WAVES) void k_tree_root_proof(const TreeDev T, const TreeSolverDev V,
                                                                      uint8_t* __restrict__ out_status,
                                                                      uint16_t* __restrict__ out_plies,
                                                                      uint16_t* __restrict__ out_move) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (g >= T.games) return;
    const size_t nb = (size_t)g * T.nodes, o = nb * T.cap;
    int nc = __builtin_amdgcn_readfirstlane(T.n_children[nb]);
    nc = nc < T.cap ? nc : T.cap;
    const int st = __builtin_amdgcn_readfirstlane((int)V.node_proven[nb]);
    int slot = -1;
    if (st == TREE_WIN || st == TREE_LOSS) slot = tree_proof_slot(V, o, nc, st, lane);
    if (lane == 0) {
        if (out_status) out_status[g] = (uint8_t)st;
        if (out_plies) out_plies[g] = V.node_plies[nb];
        if (out_move) out_move[g] = slot >= 0 ? T.action[o + slot] : (uint16_t)TREE_NO_ACTION;
    }
}

// ---------------------------------------------------------------------------------------------
// Gumbel root search (gc_tree_gumbel_*; the header has the contract).
// k_tree_gumbel_begin: per root slot j < nc the logit logf(prior), the Gumbel variate of the Philox
// word (seed, g * 256 + j, draw) and the visits the root already has; the padding 0 / -inf / 0.
// u = (n + 0.5) * 2^-24 with n the word's top 24 bits lies in (0, 1); n + 0.5 is exact in fp32 only
// below 2^23, so the upper half goes through 1 - u = (2^24 - n - 0.5) * 2^-24, which is exact there,
// and log1pf: no u rounds to 1 (a variate of +inf) and -log u keeps its relative accuracy near 1.
__global__ __launch_bounds__(64 * TREE_WAVES) void k_tree_gumbel_begin(const TreeDev T, const TreeGumbelDev U,
                                                                        u64 seed, u32 draw) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (g >= T.games) return;
    const size_t o = (size_t)g * T.nodes * T.cap, w = (size_t)g * T.cap;
    int nc = __builtin_amdgcn_readfirstlane(T.n_children[(size_t)g * T.nodes]);
    nc = nc < T.cap ? nc : T.cap;
    for (int s = lane; s < T.cap; s += 64) {
        const bool on = s < nc;
        const float pr = on ? T.prior[o + s] : 0.f;
        const int ev = on ? T.edge_visits[o + s] : 0;
        const u32 n = philox_x0(seed, (u32)g * 256u + (u32)s, draw) >> 8;
        const float nl = n < (1u << 23) ? -logf(((float)n + 0.5f) * 0x1p-24f)
                                        : -log1pf(-(((float)((1u << 24) - n) - 0.5f) * 0x1p-24f));
        U.gumbel[w + s] = on ? -logf(nl) : 0.f;
        U.logit[w + s] = logf(pr);  // (the padding's prior 0: -inf)
        U.base_visits[w + s] = ev;
    }
}

struct TreeGumbelOut {  // every array may be NULL
    uint16_t* actions;  // [G][cap]
    int32_t* visits;    // [G][cap]
    float* pi;          // [G][cap]
    int32_t* target;    // [G][cap]
    uint16_t* pick;     // [G]
    float* value;       // [G]
};

// the improved policy softmax(logit + sigma(completed Q)) over the root's children, its fixed-point
// form for the sample store, v_mix and the move: the best score among the most searched slots
__global__ __launch_bounds__(64 * TREE_WAVES) void k_tree_gumbel_policy(const TreeDev T, const TreeGumbelDev U,
                                                                         const TreeGumbelOut A) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (g >= T.games) return;
    const float ninf = -__builtin_inff();
    const size_t nb = (size_t)g * T.nodes, o = nb * T.cap, w = (size_t)g * T.cap;
    int nc = __builtin_amdgcn_readfirstlane(T.n_children[nb]);
    nc = nc < T.cap ? nc : T.cap;
    const float lv = T.leaf_value[nb];
    TreeGumbelSlot r0{0, 0.f, 0.f, 0.f, ninf, 0};
    if (lane < nc) {
        r0.ev = T.edge_visits[o + lane];
        r0.val = T.edge_value[o + lane];
        r0.pr = T.prior[o + lane];
        r0.gu = U.gumbel[w + lane];
        r0.lg = U.logit[w + lane];
        r0.bv = U.base_visits[w + lane];
    }
    constexpr int CH = TREE_MAX_CAP / 64;
    int ev[CH];
    int S = 0;
#pragma unroll
    for (int c = 0; c < CH; c++) {
        ev[c] = c * 64 < nc ? tree_gumbel_load(T, U, g, nc, c, lane, r0).ev : 0;
        S += ev[c];
    }
    S = tree_wave_sum(S);
    float vmix, scale;
    int j = tree_gumbel_slot<true>(T, U, g, nc, lane, r0, S, lv, &vmix, &scale);
    if (j < 0 && nc > 0) j = 0;  // (only with NaN scores: some slot, in bounds)
    // x = logit + sigma, its maximum, exp(x - max) and their sum (fp64: the order of the lanes'
    // partial sums does not show in the result)
    float x[CH], m = ninf;
#pragma unroll
    for (int c = 0; c < CH; c++) {
        x[c] = ninf;
        if (c * 64 >= nc) continue;
        const TreeGumbelSlot r = tree_gumbel_load(T, U, g, nc, c, lane, r0);
        if (c * 64 + lane < nc) x[c] = r.lg + tree_gumbel_sigma(r, vmix, scale);
        m = fmaxf(m, x[c]);
    }
    m = pol_wave_max(m);
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < CH; c++) {
        x[c] = c * 64 + lane < nc && m > ninf ? expf(x[c] - m) : 0.f;
        sum += (double)x[c];
    }
    sum = tree_wave_sum(sum);
    const float total = (float)sum;
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const int s = c * 64 + lane;
        if (s >= T.cap) continue;
        const float p = total > 0.f ? x[c] / total : 0.f;
        if (A.actions) A.actions[w + s] = s < nc ? T.action[o + s] : (uint16_t)TREE_NO_ACTION;
        if (A.visits) A.visits[w + s] = ev[c];
        if (A.pi) A.pi[w + s] = p;
        if (A.target) A.target[w + s] = (int32_t)(p * 1048576.0f + 0.5f);
    }
    if (lane == 0) {
        if (A.pick) A.pick[g] = j >= 0 ? T.action[o + j] : (uint16_t)TREE_NO_ACTION;
        if (A.value) A.value[g] = vmix;
    }
}

// ---------------------------------------------------------------------------------------------
// gc_tree_advance: the played move's subtree kept across moves.  Three launches, each one wave per
// game: k_tree_advance_mark (which child, the kept set, its ranks -> kept[], remap[][]),
// k_tree_advance_compact (the tree's rows moved in place, or the game reset) and k_move_boards
// (gc_clone.h: the boards).  The choices:
//  * cross-lane traffic: remap[] is written by the lane that owns node k and read by whichever
//    lane holds a child or parent link to k.  It crosses a KERNEL BOUNDARY: the mark launch only
//    writes it, the two later launches only read it.  Inside the mark launch the only value one
//    lane produces and another reads later is the keep bitmap of the earlier chunks; that goes
//    through LDS (one 64-bit ballot word per chunk, written by lane 0) behind a workgroup-scope
//    fence, never through global memory.
//  * LDS bound: TREE_WAVES * ceil(nodes / 64) * 8 bytes of dynamic LDS, so nodes <=
//    TREE_ADV_MAX_NODES (32 KiB per workgroup); gc_tree_advance refuses a larger tree with a message.
//  * in-place compaction: ascending old index; row new[k] (new[k] <= k) is written after it was read.
//    Lane s owns slots s, s + 64, ... of EVERY row in both roles and lane 0 owns the per-node
//    scalars, so a lane's own program order is the read-before-write ordering.  TREE_ADV_AHEAD
//    rows are read before the first of them is written (their targets lie at or below the lowest
//    of them), which shortens the chain of round trips.
#define TREE_ADV_MAX_NODES 65536
#define TREE_ADV_AHEAD 4

// which child the move names, the kept set (that child and its descendants) and its stable
// ranks: kept[g] (0: a fresh game) and remap[g][k] for every k < nodes (-1: not kept)
__global__ __launch_bounds__(64 * TREE_WAVES) void k_tree_advance_mark(const TreeDev T,
                                                                        const uint16_t* __restrict__ move,
                                                                        int32_t* __restrict__ kept,
                                                                        int32_t* __restrict__ remap) {
    extern __shared__ unsigned long long tree_adv_bits[];  // [TREE_WAVES][ceil(nodes / 64)]
    const int lane = threadIdx.x & 63, g = blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (g >= T.games) return;
    const int words = (T.nodes + 63) >> 6;
    unsigned long long* bits = tree_adv_bits + (size_t)(threadIdx.x >> 6) * words;
    const size_t gb = (size_t)g * T.nodes;
    int nn = __builtin_amdgcn_readfirstlane(T.n_nodes[g]);
    nn = nn < T.nodes ? nn : T.nodes;
    // the lowest root slot with the move's action and an expanded child
    const u32 mv = move[g];
    int nc = __builtin_amdgcn_readfirstlane(T.n_children[gb]);
    nc = nc < T.cap ? nc : T.cap;
    int r = -1;
    if (mv != TREE_NO_ACTION) {
        for (int c = 0; c * 64 < nc && r < 0; c++) {
            const int s = c * 64 + lane;
            const bool on = s < nc;
            const u32 ac = on ? T.action[gb * T.cap + s] : TREE_NO_ACTION;
            const int ch = on ? T.child[gb * T.cap + s] : -1;
            const unsigned long long hit = __ballot(on && ac == mv && ch >= 0 && ch < nn);
            if (hit) r = __builtin_amdgcn_readfirstlane(__shfl(ch, (int)__builtin_ctzll(hit), 64));
        }
    }
    // keep[k] = k == r || keep[parent[k]], a chain through ascending indices (a parent outside
    // [0, k) counts as not kept): chunk by chunk, parents of earlier chunks from their ballot
    // words, parents inside the chunk by iterating the ballot to its fixed point
    int run = 0;
    for (int c = 0; c < words; c++) {
        const int k = c * 64 + lane;
        const bool live = r >= 0 && k >= r && k < nn;
        const int p = live ? T.parent[gb + k] : -1;
        const bool okp = live && p >= r && p < k;
        const bool inside = okp && (p >> 6) == c;
        bool kp = live && k == r;
        if (okp && !inside) kp = (bits[p >> 6] >> (p & 63)) & 1;
        unsigned long long bal = __ballot(kp);
        if (__ballot(inside)) {
            for (;;) {
                if (inside && ((bal >> (p & 63)) & 1)) kp = true;
                const unsigned long long nb = __ballot(kp);
                if (nb == bal) break;
                bal = nb;
            }
        }
        if (lane == 0) bits[c] = bal;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the word is in LDS before a later chunk reads it
        if (k < T.nodes) remap[gb + k] = kp ? run + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
        run += __popcll(bal);
    }
    if (lane == 0) kept[g] = run;
}

// a kept game's rows moved to their new indices with the links renumbered; a fresh game reset
// SOLVER: the solver's rows and scalars move with their nodes, the same lanes owning them
template <bool SOLVER>
__global__ __launch_bounds__(64 * TREE_WAVES) void k_tree_advance_compact(const TreeDev T, const TreePriors P,
                                                                           const float* __restrict__ value,
                                                                           const int32_t* __restrict__ kept,
                                                                           const int32_t* __restrict__ remap,
                                                                           const TreeSolverDev V) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * TREE_WAVES + (threadIdx.x >> 6);
    if (g >= T.games) return;
    const int m = __builtin_amdgcn_readfirstlane(kept[g]);
    if (m <= 0) {
        tree_reset_game<SOLVER>(T, V, g, P, value, lane);
        return;
    }
    const size_t gb = (size_t)g * T.nodes;
    const int32_t* rm = remap + gb;
    int nn = __builtin_amdgcn_readfirstlane(T.n_nodes[g]);
    nn = nn < T.nodes ? nn : T.nodes;
    auto renumber = [&](int k) { return (unsigned)k < (unsigned)nn ? rm[k] : -1; };
    for (int c0 = 0; c0 < nn; c0 += 64) {
        const int k = c0 + lane;
        const int nw = k < nn ? rm[k] : -1;
        unsigned long long todo = __ballot(nw >= 0 && nw <= k);
        while (todo) {
            int from[TREE_ADV_AHEAD], to[TREE_ADV_AHEAD];
#pragma unroll
            for (int u = 0; u < TREE_ADV_AHEAD; u++) {
                from[u] = to[u] = -1;
                if (todo) {
                    const int l = (int)__builtin_ctzll(todo);
                    todo &= todo - 1;
                    from[u] = c0 + l;
                    to[u] = __builtin_amdgcn_readfirstlane(__shfl(nw, l, 64));
                }
            }
            for (int s = lane; s < T.cap; s += 64) {
                uint16_t ac[TREE_ADV_AHEAD];
                float pr[TREE_ADV_AHEAD], va[TREE_ADV_AHEAD];
                int ch[TREE_ADV_AHEAD], ev[TREE_ADV_AHEAD];
                uint8_t ep[TREE_ADV_AHEAD];
                uint16_t pl[TREE_ADV_AHEAD];
#pragma unroll
                for (int u = 0; u < TREE_ADV_AHEAD; u++) {
                    if (from[u] < 0) continue;
                    const size_t o = (gb + from[u]) * T.cap + s;
                    ac[u] = T.action[o];
                    pr[u] = T.prior[o];
                    ch[u] = T.child[o];
                    ev[u] = T.edge_visits[o];
                    va[u] = T.edge_value[o];
                    if constexpr (SOLVER) {
                        ep[u] = V.edge_proven[o];
                        pl[u] = V.edge_plies[o];
                    }
                }
#pragma unroll
                for (int u = 0; u < TREE_ADV_AHEAD; u++)
                    if (from[u] >= 0) ch[u] = renumber(ch[u]);
#pragma unroll
                for (int u = 0; u < TREE_ADV_AHEAD; u++) {
                    if (from[u] < 0) continue;
                    const size_t o = (gb + to[u]) * T.cap + s;
                    T.action[o] = ac[u];
                    T.prior[o] = pr[u];
                    T.child[o] = ch[u];
                    T.edge_visits[o] = ev[u];
                    T.edge_value[o] = va[u];
                    if constexpr (SOLVER) {
                        V.edge_proven[o] = ep[u];
                        V.edge_plies[o] = pl[u];
                    }
                }
            }
            if (lane == 0) {
                int nch[TREE_ADV_AHEAD], pa[TREE_ADV_AHEAD], ps[TREE_ADV_AHEAD];
                float lv[TREE_ADV_AHEAD];
                uint8_t te[TREE_ADV_AHEAD], np[TREE_ADV_AHEAD], co[TREE_ADV_AHEAD];
                uint16_t npl[TREE_ADV_AHEAD];
#pragma unroll
                for (int u = 0; u < TREE_ADV_AHEAD; u++) {
                    if (from[u] < 0) continue;
                    const size_t o = gb + from[u];
                    nch[u] = T.n_children[o];
                    pa[u] = T.parent[o];
                    ps[u] = T.parent_slot[o];
                    lv[u] = T.leaf_value[o];
                    te[u] = T.terminal[o];
                    if constexpr (SOLVER) {
                        np[u] = V.node_proven[o];
                        npl[u] = V.node_plies[o];
                        co[u] = V.complete[o];
                    }
                }
#pragma unroll
                for (int u = 0; u < TREE_ADV_AHEAD; u++) {
                    if (from[u] < 0) continue;
                    const bool root = to[u] == 0;
                    pa[u] = root ? -1 : renumber(pa[u]);
                    ps[u] = root ? -1 : ps[u];
                }
#pragma unroll
                for (int u = 0; u < TREE_ADV_AHEAD; u++) {
                    if (from[u] < 0) continue;
                    const size_t o = gb + to[u];
                    T.n_children[o] = nch[u];
                    T.parent[o] = pa[u];
                    T.parent_slot[o] = ps[u];
                    T.leaf_value[o] = lv[u];
                    T.terminal[o] = te[u];
                    if constexpr (SOLVER) {
                        V.node_proven[o] = np[u];
                        V.node_plies[o] = npl[u];
                        V.complete[o] = co[u];
                    }
                }
            }
        }
    }
    if (lane == 0) {
        T.n_nodes[g] = m;
        T.overflow[g] = 0;
        T.depth[g] = 0;
        T.leaf[g] = 0;
        T.leaf_new[g] = 0;
    }
}

}  // namespace gc
