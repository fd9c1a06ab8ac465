"""CPU: the reference of the search tree's solver (gc_tree_solver_enable, gym-chess_amd/csrc/gc_tree.h:
forced wins, draws and losses proven during the search) on top of test_tree_search's RefTree and
test_tree_advance's AdvTree, checked against cases written out by hand, against a bottom-up
recomputation of every node, against plain minimax, and against brute-force restatements of the
root's proof and pick.  test_tree_solver_gpu.py runs the device against this reference.

RefSolverTree keeps the five solver arrays beside RefTree's ([G][nodes][cap] edge_proven u8 /
edge_plies u16, [G][nodes] node_proven u8 / node_plies u16 / complete u8) and applies the header's
rules incrementally, exactly as the device does: node creation in _init_node (reset, backup, a
fresh game of advance), the propagation in backup, exact Q / exclusion / the proven root / the end
at a proven edge in select.  Proofs are integers, so they must match the device bit for bit.

The acceptance rule is test_tree_search's, over the candidates (the edges that are not LOSS, or
all when every edge is): a proven edge's Q is exact, which takes one rounded division out of the
score, so the same tolerance holds.  Among candidates whose (prior, visits, value, status) are
bitwise the chosen one's the chosen slot must be the lowest.
"""
import os
import re

import numpy as np
import pytest

import test_policy_sample as P
import test_tree_advance as A
import test_tree_search as R

NONE = R.NONE
UNKNOWN, WIN, DRAW, LOSS = 0, 1, 2, 3
FLIP = {UNKNOWN: UNKNOWN, WIN: LOSS, DRAW: DRAW, LOSS: WIN}
EXACT = {WIN: 1.0, DRAW: 0.0, LOSS: -1.0}
SOLVER_EDGE_KEYS = ("edge_proven", "edge_plies")
SOLVER_NODE_KEYS = ("node_proven", "node_plies", "complete")
SOLVER_SYMBOLS = ("gc_tree_solver_enable", "gc_tree_solver_pointers", "gc_tree_root_proof")


class RefSolverTree(A.AdvTree):
    def __init__(self, games, nodes, cap, solver=True):
        super().__init__(games, nodes, cap)
        G, N, C = games, nodes, cap
        self.solver = solver
        self.edge_proven = np.zeros((G, N, C), dtype=np.uint8)
        self.edge_plies = np.zeros((G, N, C), dtype=np.uint16)
        self.node_proven = np.zeros((G, N), dtype=np.uint8)
        self.node_plies = np.zeros((G, N), dtype=np.uint16)
        self.complete = np.zeros((G, N), dtype=np.uint8)
        self.climbs = []  # per propagation: the nodes whose verdict it changed
        self.ended_proven = 0  # descents that ended at a proven edge

    # ------------------------------------------------------------------ node creation
    def _init_node(self, g, k, actions, priors, count, pri_cap, listed=True):
        super()._init_node(g, k, actions, priors, count, pri_cap, listed=listed)
        if self.solver:
            self.edge_proven[g, k] = 0
            self.edge_plies[g, k] = 0
            self.complete[g, k] = 1 if not listed else int(0 <= int(count[g]) <= min(pri_cap, self.cap))
            self.node_proven[g, k] = UNKNOWN
            self.node_plies[g, k] = 0

    # ------------------------------------------------------------------ the rules
    def node_rule(self, g, k):
        m = int(self.n_children[g, k])
        st, pl = self.edge_proven[g, k, :m], self.edge_plies[g, k, :m]
        if (st == WIN).any():
            return WIN, int(pl[st == WIN].min())
        if self.complete[g, k] and not (st == UNKNOWN).any():
            return (DRAW, 0) if (st == DRAW).any() else (LOSS, int(pl.max()))
        return UNKNOWN, 0

    def proof_slot(self, g, k, want):
        """the `want` edge of node k with the fewest (WIN) / the most (LOSS) plies, ties to the
        lowest slot; -1 without one"""
        m = int(self.n_children[g, k])
        st, pl = self.edge_proven[g, k, :m], self.edge_plies[g, k, :m].astype(np.int64)
        at = np.flatnonzero(st == want)
        if not at.size:
            return -1
        return int(at[np.argmin(pl[at])] if want == WIN else at[np.argmax(pl[at])])

    def _propagate(self, g, D):
        c, changed = int(self.leaf[g]), 0
        for d in range(D - 1, -1, -1):
            k, j = (int(x) for x in self.path[g, d])
            if self.node_proven[g, c] == UNKNOWN:
                break
            self.edge_proven[g, k, j] = FLIP[int(self.node_proven[g, c])]
            self.edge_plies[g, k, j] = min(65535, int(self.node_plies[g, c]) + 1)
            st, pl = self.node_rule(g, k)
            if (st, pl) == (int(self.node_proven[g, k]), int(self.node_plies[g, k])):
                break
            self.node_proven[g, k], self.node_plies[g, k] = st, pl
            changed += 1
            c = k
        self.climbs.append(changed)

    # ------------------------------------------------------------------ selection
    def scores(self, g, k, c_puct, fpu):
        if not self.solver:
            return super().scores(g, k, c_puct, fpu)
        nc = int(self.n_children[g, k])
        ev = self.edge_visits[g, k, :nc].astype(np.float64)
        val = self.edge_value[g, k, :nc].astype(np.float64)
        pr = self.prior[g, k, :nc].astype(np.float64)
        st = self.edge_proven[g, k, :nc]
        q = np.where(ev > 0, val / np.maximum(ev, 1.0), float(np.float32(fpu)))
        for code, exact in EXACT.items():
            q = np.where(st == code, exact, q)
        return q + float(np.float32(c_puct)) * pr * np.sqrt(1.0 + ev.sum()) / (1.0 + ev)

    def candidates(self, g, k):
        """the edges the argmax runs over: not LOSS, or all of them when every edge is LOSS"""
        st = self.edge_proven[g, k, : int(self.n_children[g, k])]
        cand = st != LOSS
        return cand if cand.any() else np.ones_like(cand)

    def _decide(self, g, k, c_puct, fpu, dev_slot):
        if not self.solver:
            return super()._decide(g, k, c_puct, fpu, dev_slot)
        nc = int(self.n_children[g, k])
        self.decisions += 1
        if (self.edge_proven[g, k, :nc] == WIN).any():  # the proven root: no scores
            j = self.proof_slot(g, k, WIN)
            assert dev_slot is None or int(dev_slot) == j, (g, k, dev_slot, j)
            return j
        if nc == 1:
            assert dev_slot is None or int(dev_slot) == 0, (g, k, dev_slot)
            return 0
        cand = self.candidates(g, k)
        ref = self.scores(g, k, c_puct, fpu)
        best = float(ref[cand].max())
        tol = R.TOL * max(1.0, float(np.abs(ref[cand]).max()))
        tri = np.concatenate([self._triples(g, k), self.edge_proven[g, k, :nc, None].astype(np.int64)], axis=1)
        j = int(np.flatnonzero(cand & (ref == best))[0]) if dev_slot is None else int(dev_slot)
        assert 0 <= j < nc, (g, k, j, nc)
        assert cand[j], f"game {g} node {k}: slot {j} is proven LOSS and another edge is not"
        assert ref[j] >= best - tol, f"game {g} node {k}: slot {j} scores {ref[j]!r}, the best {best!r}"
        same = np.flatnonzero((tri == tri[j]).all(axis=1))
        assert j == same[0], f"game {g} node {k}: slot {j} chosen, slot {same[0]} has the same inputs"
        if any((tri[i] != tri[j]).any() for i in np.flatnonzero(cand & (ref >= best - tol))):
            self.near_ties += 1
        return j

    def select(self, c_puct=1.25, fpu=0.0, follow=None):
        if not self.solver:
            return super().select(c_puct, fpu, follow=follow)
        G, N = self.games, self.nodes
        out_p = np.full(G, -1, dtype=np.int32)
        out_c = np.full(G, -1, dtype=np.int32)
        out_a = np.full(G, NONE, dtype=np.uint16)
        for g in range(G):
            k, D = 0, 0
            self.leaf_new[g] = 0
            while True:
                if self.n_children[g, k] == 0:  # (b)
                    self.leaf[g] = k
                    break
                dev = None
                if follow is not None:
                    assert D < N and follow[0][g, D, 0] == k, (g, D, k, follow[0][g, D])
                    dev = follow[0][g, D, 1]
                j = self._decide(g, k, c_puct, fpu, dev)
                self.path[g, D] = (k, j)
                D += 1
                ch = int(self.child[g, k, j])
                if self.edge_proven[g, k, j] != UNKNOWN:  # the descent ends at the proven child
                    assert ch >= 0, (g, k, j)
                    self.leaf[g] = ch
                    self.ended_proven += 1
                    break
                if ch >= 0:
                    k = ch
                    continue
                if self.n_nodes[g] < N:  # (a)
                    L = int(self.n_nodes[g])
                    self.n_nodes[g] += 1
                    self.leaf[g], self.leaf_new[g] = L, 1
                    out_p[g], out_c[g], out_a[g] = g * N + k, g * N + L, self.action[g, k, j]
                else:  # (c)
                    self.overflow[g] += 1
                    D -= 1
                    self.leaf[g] = k
                break
            self.depth[g] = D
            if follow is not None:
                assert follow[1][g] == D, (g, follow[1][g], D)
        return out_p, out_c, out_a

    # ------------------------------------------------------------------ backup
    def backup(self, value, done, reason, actions, priors, count):
        if not self.solver:
            return super().backup(value, done, reason, actions, priors, count)
        pri_cap = actions.shape[1]
        for g in range(self.games):
            D, L = int(self.depth[g]), int(self.leaf[g])
            if self.leaf_new[g]:
                k, j = self.path[g, D - 1]
                fin = bool(done[g])
                self._init_node(g, L, actions, priors, count, pri_cap, listed=not fin)
                self.parent[g, L], self.parent_slot[g, L] = k, j
                self.child[g, k, j] = L
                self.terminal[g, L] = 1 if fin else 0
                self.leaf_value[g, L] = np.float32((-1.0 if reason[g] == 1 else 0.0) if fin else value[g])
                if fin:
                    self.node_proven[g, L] = LOSS if reason[g] == 1 else DRAW
                    self._propagate(g, D)
            st = int(self.node_proven[g, L])
            v = np.float32(EXACT[st]) if st else np.float32(self.leaf_value[g, L])
            for d in range(D):
                k, j = self.path[g, d]
                self.edge_visits[g, k, j] += 1
                self.edge_value[g, k, j] = np.float32(self.edge_value[g, k, j] + (-v if (D - d) & 1 else v))

    # ------------------------------------------------------------------ the root
    def root_proof(self):
        """-> status uint8[G], plies uint16[G], move uint16[G]"""
        move = np.full(self.games, NONE, dtype=np.uint16)
        for g in range(self.games):
            st = int(self.node_proven[g, 0])
            if st in (WIN, LOSS):
                move[g] = self.action[g, 0, self.proof_slot(g, 0, st)]
        return self.node_proven[:, 0].copy(), self.node_plies[:, 0].copy(), move

    def root_policy(self, seed, draw, greedy, proof=False):
        out = super().root_policy(seed, draw, greedy)
        if not proof:
            return out
        x0 = P.philox_x0(seed, np.arange(self.games), draw)
        for g in range(self.games):
            nc = int(self.n_children[g, 0])
            st, v = self.edge_proven[g, 0, :nc], self.edge_visits[g, 0, :nc].astype(np.int64)
            cand = np.flatnonzero(st != LOSS)
            if (st == WIN).any():
                j = self.proof_slot(g, 0, WIN)
            elif not cand.size:
                j = self.proof_slot(g, 0, LOSS)
            elif v[cand].sum() == 0:
                j = int(cand[0]) if v.sum() > 0 else -1
            else:
                cv = np.where(st != LOSS, v, 0)
                j = int(cand[np.argmax(v[cand])]) if greedy else self.sample_slot(cv, x0[g])
            out["pick"][g] = self.action[g, 0, j] if j >= 0 else NONE
        return out

    # ------------------------------------------------------------------ advance
    def advance(self, moves, actions, priors, count, value=None):
        kept, remap = super().advance(moves, actions, priors, count, value=value)
        if self.solver:
            for g in range(self.games):
                old = np.flatnonzero(remap[g] >= 0)  # ascending: new index = rank
                for key in SOLVER_EDGE_KEYS + SOLVER_NODE_KEYS:
                    a = getattr(self, key)
                    a[g, : old.size] = a[g, old]
        return kept, remap

    def same_as(self, dev):
        """dev: the device's arrays (the tree's and, on a solver tree, the solver's)"""
        super().same_as(dev)
        if self.solver:
            for g in range(self.games):
                n = int(self.n_nodes[g])
                for key in SOLVER_EDGE_KEYS + SOLVER_NODE_KEYS:
                    a, b = getattr(self, key)[g, :n], dev[key][g, :n]
                    assert (a == b).all(), (key, g, np.argwhere(a != b)[:4])


# --------------------------------------------------------------------------- independent restatements
def check_recomputed(t):
    """every live node recomputed bottom-up from its edges (a child's index is above its parent's)
    equals the stored verdict, and every edge equals its child's flipped verdict, plies + 1 (an
    edge without an expanded child is unknown)"""
    for g in range(t.games):
        n = int(t.n_nodes[g])
        for k in range(n - 1, -1, -1):
            m = int(t.n_children[g, k])
            for s in range(t.cap):
                c = int(t.child[g, k, s]) if s < m else -1
                want = (UNKNOWN, 0)
                if c >= 0 and t.node_proven[g, c] != UNKNOWN:
                    want = (FLIP[int(t.node_proven[g, c])], min(65535, int(t.node_plies[g, c]) + 1))
                assert (int(t.edge_proven[g, k, s]), int(t.edge_plies[g, k, s])) == want, (g, k, s, want)
            if t.terminal[g, k]:
                want = (LOSS if t.leaf_value[g, k] == -1.0 else DRAW, 0)
                assert t.complete[g, k] == 1 and m == 0, (g, k)
            elif m == 0:
                want = (UNKNOWN, 0)
            else:
                want = t.node_rule(g, k)
            assert (int(t.node_proven[g, k]), int(t.node_plies[g, k])) == want, (g, k, want)


def minimax(t, g, k):
    """the verdict of node k by plain minimax over the terminal nodes of its subtree (None: not
    provable), recursively and without the solver's edge arrays; the plies ride along"""
    if t.terminal[g, k]:
        return (LOSS if t.leaf_value[g, k] == -1.0 else DRAW), 0
    m = int(t.n_children[g, k])
    below = [minimax(t, g, int(c)) if c >= 0 else None for c in t.child[g, k, :m]]
    wins = [p + 1 for r in below if r is not None for s, p in [r] if s == LOSS]  # the child's side is lost
    if wins:
        return WIN, min(wins)
    if m == 0 or not t.complete[g, k] or any(r is None for r in below):
        return None
    if any(s == DRAW for s, _ in below):
        return DRAW, 0
    return LOSS, max(p + 1 for _, p in below)


def check_sound(t):
    for g in range(t.games):
        for k in range(int(t.n_nodes[g])):
            st = int(t.node_proven[g, k])
            got = minimax(t, g, k)
            assert (got is None and st == UNKNOWN) or got == (st, int(t.node_plies[g, k])), (g, k, st, got)


# --------------------------------------------------------------------------- synthetic inputs
# (G, nodes, cap, pri_cap rule, seed, c_puct, fpu): G = 5 is ragged against the kernels' 4 games per
# workgroup, cap 1 a chain, cap 65 two slot chunks; a wide block cuts long lists at the tree's cap
# and a narrow one at pri_cap < cap (both leave the node incomplete)
SOLVER_CASES = [(5, 24, 1, "wide", 151, 1.25, 0.5), (5, 32, 3, "wide", 122, 2.5, 0.5),
                (5, 40, 7, "narrow", 123, 3.0, 0.25), (5, 32, 65, "wide", 134, 2.5, 0.5),
                (5, 12, 3, "narrow", 125, 2.0, 1.0)]
# (a high c_puct and an fpu above a draw's 0 keep the searches broad: otherwise a proven draw
# absorbs nearly every later descent; the seeds are chosen by test_the_inputs_exercise_the_rules)
DONE_RATE = 0.35


def solver_rows(rng, G, cap, pri_cap, kinds=None):
    """R.synth_rows with the counts that make proofs: mostly 1..3 moves (a list that long is cut
    out of a longer one, priors as they were), some lists longer than the tree holds (incomplete
    nodes), a few empty or dead ones"""
    if kinds is None:
        kinds = rng.choice(["few", "more", "zero", "dead", "some"], size=G, p=[0.7, 0.14, 0.04, 0.02, 0.1])
    kinds = np.asarray(kinds)
    a, p, c = R.synth_rows(rng, G, cap, pri_cap, ["some" if k == "few" else k for k in kinds])
    for g in np.flatnonzero(kinds == "few"):
        few = int(rng.randint(1, 4))
        if c[g] > few:
            c[g] = few
            a[g, few:] = NONE
            p[g, few:] = 0
    return a, p, c


def solver_run(G, nodes, cap, rule, seed):
    """the inputs of a run of 2 * nodes simulations in R.synth_run's layout: 35 % of the
    expansions end the game, 3 in 10 of those by reason 1 (mate) and the others by 2 (a draw);
    the roots are wide but for game 3's (a mate in one under a wide root proves it at once, so
    mates are the rarer end and most proofs have to climb)"""
    rng = np.random.RandomState(seed)
    pri_cap = R.pri_cap_of(cap, rule)
    sims = 2 * nodes
    root = solver_rows(rng, G, cap, pri_cap, ["some", "cap", "more", "few", "some"][:G])
    root_value = rng.uniform(-1, 1, size=G).astype(np.float32)
    A_ = np.zeros((sims, G, pri_cap), dtype=np.uint16)
    Pr = np.zeros((sims, G, pri_cap), dtype=np.float32)
    Cn = np.zeros((sims, G), dtype=np.int32)
    for s in range(sims):
        A_[s], Pr[s], Cn[s] = solver_rows(rng, G, cap, pri_cap)
    value = rng.uniform(-1, 1, size=(sims, G)).astype(np.float32)
    done = (rng.rand(sims, G) < DONE_RATE).astype(np.uint8)
    reason = np.where(done != 0, np.where(rng.rand(sims, G) < 0.3, 1, 2), 0).astype(np.uint8)
    return dict(root=root, root_value=root_value, actions=A_, priors=Pr, count=Cn, value=value, done=done,
                reason=reason, sims=sims, pri_cap=pri_cap)


# a chain of more than 64 nodes whose end is mate: (G, nodes, cap, rule, seed, c_puct, fpu, mate_at)
CHAIN_CASE = (3, 130, 1, "wide", 21, 1.25, 0.0, 99)


def chain_run(G, nodes, cap, rule, seed, mate_at):
    """R.open_run's chain (one node per simulation, no dead end) with the expansion of simulation
    `mate_at` terminal: mate in games 0 and 1, a draw in game 2.  Game 0's lists all have count 1
    (every node complete), so its mate climbs the whole path, past 64 entries, to the root; game
    1 keeps open_run's counts, of which those above 1 are incomplete and stop the climb."""
    inp = R.open_run(G, nodes, cap, rule, seed)
    inp["count"][:, 0] = 1
    inp["root"][2][0] = 1
    inp["done"][mate_at] = 1
    inp["reason"][mate_at] = (1, 1, 2)[:G]
    inp["sims"] = mate_at + 12
    return inp


def run_solver_reference(case, make=solver_run, check=None):
    """the reference driven alone; check(t, s) after every backup"""
    G, nodes, cap, rule, seed, c_puct, fpu = case[:7]
    inp = make(G, nodes, cap, rule, seed, *case[7:])
    t = RefSolverTree(G, nodes, cap)
    t.reset(*inp["root"], value=inp["root_value"])
    inp["max_depth"] = 0
    for s in range(inp["sims"]):
        t.select(c_puct, fpu)
        inp["max_depth"] = max(inp["max_depth"], int(t.depth.max()))
        t.backup(inp["value"][s], inp["done"][s], inp["reason"][s], inp["actions"][s], inp["priors"][s],
                 inp["count"][s])
        if check:
            check(t, s)
    return t, inp


# --------------------------------------------------------------------------- hand cases
def one(x, dt):
    return np.array([x], dtype=dt)


def sim(t, value=0.0, done=0, reason=0, row=((300, 1.0),), pri_cap=4, c_puct=1.0, fpu=0.0):
    """one simulation of a one-game tree: the new node (if any) gets `row`"""
    out = t.select(c_puct, fpu)
    t.backup(one(value, np.float32), one(done, np.uint8), one(reason, np.uint8), *R._block([list(row)], pri_cap))
    return out


def test_mate_in_one_under_the_root():
    """root (100: 0.6, 200: 0.4); the first simulation takes slot 0 and its node is mate: the edge
    is WIN in 1, the root WIN in 1, the proof's move 100; the mover's value +1 went up the edge.
    The next descent takes the WIN edge without scores and ends at the mated node."""
    t = RefSolverTree(1, 6, 2)
    t.reset(*R._block([[(100, 0.6), (200, 0.4)]], 4))
    assert t.complete[0, 0] == 1 and t.node_proven[0, 0] == UNKNOWN
    sim(t, done=1, reason=1)
    assert (t.node_proven[0, 1], t.node_plies[0, 1], t.complete[0, 1]) == (LOSS, 0, 1)
    assert (t.edge_proven[0, 0].tolist(), t.edge_plies[0, 0].tolist()) == ([WIN, UNKNOWN], [1, 0])
    assert (t.node_proven[0, 0], t.node_plies[0, 0]) == (WIN, 1)
    assert t.edge_value[0, 0, 0] == 1.0 and t.climbs == [1]
    st, pl, mv = t.root_proof()
    assert (st[0], pl[0], mv[0]) == (WIN, 1, 100)
    p, c, a = sim(t, value=0.5)
    assert (p[0], c[0], a[0]) == (-1, -1, NONE) and t.depth[0] == 1 and t.leaf[0] == 1 and not t.leaf_new[0]
    assert t.edge_visits[0, 0].tolist() == [2, 0] and t.edge_value[0, 0, 0] == 2.0 and t.ended_proven == 1
    assert t.n_nodes[0] == 2
    check_recomputed(t)
    check_sound(t)


def chain(complete_a):
    """root (two moves) -> A under slot 0 -> B (A's only listed move) -> mate"""
    t = RefSolverTree(1, 6, 2)
    t.reset(*R._block([[(100, 0.9), (200, 0.1)]], 4))
    sim(t, value=0.0, row=[(300, 1.0)])  # A = node 1, one move listed
    if not complete_a:  # the row A was made from held more moves than its list
        t.complete[0, 1] = 0
    sim(t, value=0.5, fpu=-2.0, row=[(400, 1.0)])  # B = node 2 (value +0.5: the root's slot 0 looks good)
    assert t.path[0, :2].tolist() == [[0, 0], [1, 0]]
    sim(t, fpu=-2.0, done=1, reason=1)  # node 3 under B: mate
    assert t.path[0, :3].tolist() == [[0, 0], [1, 0], [2, 0]] and t.terminal[0, 3] == 1
    return t


def test_a_forced_mate_in_three_plies():
    t = chain(True)
    assert (t.node_proven[0, 2], t.node_plies[0, 2]) == (WIN, 1)   # B mates
    assert (t.node_proven[0, 1], t.node_plies[0, 1]) == (LOSS, 2)  # A's only move leads there
    assert (t.node_proven[0, 0], t.node_plies[0, 0]) == (WIN, 3)
    assert (t.edge_proven[0, 0, 0], t.edge_plies[0, 0, 0]) == (WIN, 3)
    assert (t.edge_proven[0, 1, 0], t.edge_plies[0, 1, 0]) == (LOSS, 2)
    assert t.climbs[-1] == 3
    assert tuple(int(x[0]) for x in t.root_proof()) == (WIN, 3, 100)
    check_recomputed(t)
    check_sound(t)


def test_an_incomplete_node_is_never_lost():
    """the same chain with A incomplete (its list was cut): all its listed edges are LOSS, an
    unlisted move might save it: A stays unknown and so does the root"""
    t = chain(False)
    assert (t.node_proven[0, 2], t.node_plies[0, 2]) == (WIN, 1)
    assert (t.edge_proven[0, 1, 0], t.edge_plies[0, 1, 0]) == (LOSS, 2)
    assert (t.node_proven[0, 1], t.node_plies[0, 1]) == (UNKNOWN, 0)
    assert (t.node_proven[0, 0], t.edge_proven[0, 0, 0]) == (UNKNOWN, UNKNOWN) and t.climbs[-1] == 1
    assert tuple(int(x[0]) for x in t.root_proof()) == (UNKNOWN, 0, NONE)
    # A is entered again; its only listed edge is LOSS (all are: none is left out) and ends the descent
    sim(t, fpu=-2.0)
    assert t.depth[0] == 2 and t.leaf[0] == 2 and t.ended_proven == 1
    # A's edge: minus B's +0.5, the mate (-1 at the leaf, an even distance), then B's proven +1 negated
    assert t.edge_value[0, 1, 0] == np.float32(-0.5 - 1.0 - 1.0)
    check_sound(t)


def test_incomplete_comes_from_the_count():
    """complete is set from the row: 0 <= count <= min(pri_cap, cap)"""
    for cap, pri_cap, count, want in ((2, 4, 2, 1), (2, 4, 3, 0), (4, 2, 2, 1), (4, 2, 3, 0), (2, 4, 0, 1), (2, 4, -1, 0)):
        t = RefSolverTree(1, 2, cap)
        a, p, c = R._block([[(10 + i, 0.1) for i in range(min(max(count, 0), pri_cap))]], pri_cap)
        c[0] = count
        t.reset(a, p, c)
        assert t.complete[0, 0] == want, (cap, pri_cap, count)


def test_loss_loss_draw_is_a_draw():
    """a complete root with three moves.  Slots 0 and 1 lead to nodes whose only move mates (the
    nodes are WIN, so the root's edges are LOSS); slot 2's child is a drawn terminal node.  fpu +1
    makes the first three simulations take the three unvisited slots in turn."""
    t = RefSolverTree(1, 8, 3)
    t.reset(*R._block([[(100, 0.5), (200, 0.3), (300, 0.2)]], 4))
    sim(t, fpu=1.0, row=[(11, 1.0)])          # node 1 under slot 0
    sim(t, fpu=1.0, row=[(12, 1.0)])          # node 2 under slot 1
    sim(t, fpu=1.0, done=1, reason=2)         # node 3 under slot 2: a draw
    assert t.child[0, 0].tolist() == [1, 2, 3] and t.edge_proven[0, 0].tolist() == [0, 0, DRAW]
    assert t.node_proven[0, 0] == UNKNOWN
    for want_parent in (1, 2):                # mate below node 1, then below node 2
        p, c, a = sim(t, done=1, reason=1)
        assert p[0] == want_parent, (p, t.path[0, :2])
    assert t.node_proven[0, 1:4].tolist() == [WIN, WIN, DRAW]
    assert (t.edge_proven[0, 0].tolist(), t.edge_plies[0, 0].tolist()) == ([LOSS, LOSS, DRAW], [2, 2, 1])
    assert (t.node_proven[0, 0], t.node_plies[0, 0]) == (DRAW, 0)
    assert tuple(int(x[0]) for x in t.root_proof()) == (DRAW, 0, NONE)
    # the LOSS edges are left out: the only candidate is the drawn one, and the descent ends there
    sim(t)
    assert t.path[0, 0].tolist() == [0, 2] and t.leaf[0] == 3 and t.edge_value[0, 0, 2] == 0.0
    assert t.root_policy(5, 0, True, proof=True)["pick"][0] == 300
    check_recomputed(t)
    check_sound(t)


def test_a_faster_mate_found_later():
    """the root is first proven WIN in 3 through slot 0; an explicit descent through slot 1 then
    finds a mate in one: the plies drop to 1 and the proof's move changes"""
    t = chain(True)
    assert tuple(int(x[0]) for x in t.root_proof()) == (WIN, 3, 100)
    # a proven root always takes its WIN edge, so the second edge is walked by hand
    t.path[0, 0] = (0, 1)
    t.depth[0], t.leaf[0], t.leaf_new[0] = 1, 4, 1
    t.n_nodes[0] = 5
    t.backup(one(0, np.float32), one(1, np.uint8), one(1, np.uint8), *R._block([[(9, 1.0)]], 4))
    assert (t.edge_proven[0, 0].tolist(), t.edge_plies[0, 0].tolist()) == ([WIN, WIN], [3, 1])
    assert tuple(int(x[0]) for x in t.root_proof()) == (WIN, 1, 200)
    assert t.root_policy(5, 0, False, proof=True)["pick"][0] == 200
    check_recomputed(t)
    check_sound(t)
    sim(t)
    assert t.path[0, 0].tolist() == [0, 1] and t.leaf[0] == 4


# --------------------------------------------------------------------------- generated runs
@pytest.fixture(scope="module")
def runs():
    """every SOLVER_CASES run and the chain, driven once, with the two restatements checked after
    every backup"""
    def check(t, s):
        check_recomputed(t)
        check_sound(t)

    out = [run_solver_reference(c, check=check) for c in SOLVER_CASES]
    out.append(run_solver_reference(CHAIN_CASE, make=chain_run, check=check))
    return out


def test_propagation_is_complete_and_sound(runs):
    """(the fixture asserted both after every backup of every run) -- and the runs did prove things"""
    assert sum(len(t.climbs) for t, _ in runs) > 30


def test_the_inputs_exercise_the_rules(runs):
    counts = {WIN: 0, DRAW: 0, LOSS: 0}
    stuck = roots = 0
    for t, _ in runs[:-1]:
        for g in range(t.games):
            n = int(t.n_nodes[g])
            for st in counts:
                counts[st] += int((t.node_proven[g, :n] == st).sum())
            roots += int(t.node_proven[g, 0] != UNKNOWN)
            for k in range(n):
                m = int(t.n_children[g, k])
                if m and not t.complete[g, k] and t.node_proven[g, k] == UNKNOWN and (t.edge_proven[g, k, :m] != 0).all():
                    stuck += 1
    assert min(counts.values()) >= 5, counts
    assert max(max(t.climbs) for t, _ in runs[:-1]) >= 3
    assert stuck >= 1 and roots >= 1
    assert sum(t.ended_proven for t, _ in runs[:-1]) >= 1
    for t, inp in runs[:-1]:
        assert t.decisions > 100
        assert t.near_ties < 0.01 * t.decisions, (t.near_ties, t.decisions)
        assert {1, 2} <= set(inp["reason"].reshape(-1).tolist())
        assert t.complete.any() and not t.complete[:, : t.n_nodes.min()].all()


def test_the_chain_climbs_past_64_levels(runs):
    t, inp = runs[-1]
    mate_at = CHAIN_CASE[7]
    assert inp["max_depth"] == mate_at + 1 and mate_at + 1 > 64
    assert tuple(int(x[0]) for x in t.root_proof()) == (WIN if mate_at % 2 == 0 else LOSS, mate_at + 1,
                                                        int(t.action[0, 0, 0]))
    assert max(t.climbs) == mate_at + 1
    assert t.node_proven[1, 0] == UNKNOWN and t.node_proven[2, 0] in (UNKNOWN, DRAW)
    assert t.ended_proven >= 10


def brute_pick(t, g, greedy, x0):
    """root_policy(proof=True)'s pick restated over a list of the root's edges"""
    m = int(t.n_children[g, 0])
    edges = [(int(t.edge_proven[g, 0, s]), int(t.edge_plies[g, 0, s]), int(t.edge_visits[g, 0, s]), s) for s in range(m)]
    wins = [(pl, s) for st, pl, _, s in edges if st == WIN]
    if wins:
        return min(wins)[1]
    cand = [(v, s) for st, _, v, s in edges if st != LOSS]
    if not cand:
        return max(((pl, -s) for st, pl, _, s in edges), default=(0, 1))[1] * -1
    if sum(v for v, _ in cand) == 0:
        return cand[0][1] if sum(e[2] for e in edges) > 0 else -1
    if greedy:
        return max(cand, key=lambda c: (c[0], -c[1]))[1]
    line = [s for v, s in cand for _ in range(v)]  # slot of every unit of the candidates' visit mass
    return line[((int(x0) >> 8) * len(line)) >> 24]


def test_root_policy_and_proof_against_brute_force(runs):
    seen = set()
    for t, _ in runs:
        st, pl, mv = t.root_proof()
        for g in range(t.games):
            m = int(t.n_children[g, 0])
            want = NONE
            if st[g] in (WIN, LOSS):
                at = [(int(t.edge_plies[g, 0, s]) * (1 if st[g] == WIN else -1), s) for s in range(m)
                      if t.edge_proven[g, 0, s] == st[g]]
                want = t.action[g, 0, min(at)[1]]
            assert mv[g] == want and st[g] == t.node_proven[g, 0] and pl[g] == t.node_plies[g, 0]
        for greedy in (True, False):
            for draw in range(6):
                plain = A.AdvTree.root_policy(t, 9, draw, greedy)
                out = t.root_policy(9, draw, greedy, proof=True)
                x0 = P.philox_x0(9, np.arange(t.games), draw)
                for key in ("actions", "visits", "pi", "value"):
                    assert out[key].tobytes() == plain[key].tobytes(), key
                for g in range(t.games):
                    j = brute_pick(t, g, greedy, x0[g])
                    assert out["pick"][g] == (t.action[g, 0, j] if j >= 0 else NONE), (g, greedy, draw, j)
                    e = t.edge_proven[g, 0, : int(t.n_children[g, 0])]
                    seen.add("win" if (e == WIN).any() else "lost" if (e == LOSS).all() else
                             "excluded" if (e == LOSS).any() else "plain")
    assert {"win", "excluded", "plain"} <= seen, seen


def test_the_all_loss_root_and_candidates_without_visits():
    t = RefSolverTree(2, 4, 3)
    t.reset(*R._block([[(10, 0.5), (20, 0.3), (30, 0.2)]] * 2, 4))
    # game 0: every edge LOSS, in 2 / 6 / 6 plies: the longest, lowest slot
    t.edge_proven[0, 0] = LOSS
    t.edge_plies[0, 0] = (2, 6, 6)
    t.edge_visits[0, 0] = (5, 1, 0)
    # game 1: the visited edges are LOSS, the candidate (slot 2) has no visit
    t.edge_proven[1, 0] = (LOSS, LOSS, UNKNOWN)
    t.edge_visits[1, 0] = (3, 4, 0)
    for greedy in (True, False):
        for draw in range(4):
            assert t.root_policy(1, draw, greedy, proof=True)["pick"].tolist() == [20, 30]
            x0 = P.philox_x0(1, np.arange(2), draw)
            assert [brute_pick(t, g, greedy, x0[g]) for g in range(2)] == [1, 2]
    assert t.root_policy(1, 0, True)["pick"].tolist() == [10, 20]  # (without the flag: the visits alone)
    t.edge_visits[1, 0] = 0  # no visit at all: no pick
    assert t.root_policy(1, 0, False, proof=True)["pick"][1] == NONE
    t.edge_visits[1, 0] = (3, 4, 2)  # the candidate's visits are the whole mass
    assert all(t.root_policy(1, d, False, proof=True)["pick"][1] == 30 for d in range(8))


# --------------------------------------------------------------------------- advance
ADVANCE_CASES = (1, 2, 3)  # indices into SOLVER_CASES: the GPU test's advances


def advanced(idx):
    """SOLVER_CASES[idx] driven alone through `nodes` simulations and the GPU test's advance"""
    case = SOLVER_CASES[idx]
    G, nodes, cap, rule, seed, c_puct, fpu = case
    inp = solver_run(G, nodes, cap, rule, seed)
    t = RefSolverTree(G, nodes, cap)
    t.reset(*inp["root"], value=inp["root_value"])
    for s in range(nodes):
        t.select(c_puct, fpu)
        t.backup(inp["value"][s], inp["done"][s], inp["reason"][s], inp["actions"][s], inp["priors"][s],
                 inp["count"][s])
    mv = A.moves_for(t, t.root_policy(0, 0, True)["pick"], 0)
    old = {k: getattr(t, k).copy() for k in SOLVER_EDGE_KEYS + SOLVER_NODE_KEYS}
    act, pri, cnt, val = A.advance_blocks(case, 1)[0]
    kept, remap = t.advance(mv, act, pri, cnt, value=val)
    return t, mv, old, kept, remap, cnt, inp


def test_advance_keeps_proofs():
    """what the GPU test's advances cover, on the reference alone: games 0 and 4 are kept, 1..3
    fresh (0xFFFF, an unexpanded move, an absent one); every kept node's solver rows arrive at the
    new index bit for bit, so the tree is still consistent and sound; over the cases a kept root is
    LOSS, one is DRAW, one is unknown above proven nodes, and a kept subtree of several nodes
    holds proofs; a fresh game's root is unknown with complete from its row"""
    seen = set()
    for idx in ADVANCE_CASES:
        t, mv, old, kept, remap, cnt, inp = advanced(idx)
        A.check_links(t)
        check_recomputed(t)
        check_sound(t)
        assert kept[0] >= 1 and kept[4] >= 1 and not kept[1:4].any()
        assert mv[2] == NONE and mv[3] == A.ABSENT
        seen.add("unexpanded" if mv[1] != NONE else "none free")
        for g in (0, 4):
            ks = np.flatnonzero(remap[g] >= 0)
            for key in old:
                assert getattr(t, key)[g, : ks.size].tobytes() == old[key][g, ks].tobytes(), (key, g)
            proven = int((t.node_proven[g, : kept[g]] != UNKNOWN).sum())
            seen.add(("root", int(t.node_proven[g, 0])))
            if kept[g] > 2 and proven:
                seen.add("subtree")
        for g in (1, 2, 3):
            assert t.node_proven[g, 0] == UNKNOWN and not t.edge_proven[g, 0].any() and not t.edge_plies[g, 0].any()
            assert t.complete[g, 0] == int(0 <= cnt[g] <= min(inp["pri_cap"], t.cap))
    assert {("root", LOSS), ("root", DRAW), ("root", UNKNOWN), "subtree", "unexpanded"} <= seen, seen


# --------------------------------------------------------------------------- the chess positions
def test_the_chess_positions_under_fide_rules():
    """the GPU test's two positions with the host build of the FIDE generator: the roots have 20
    and 28 moves with the line's first moves among them, black's only reply to e8-f8 is h8-h7, and
    both final positions leave the side to move (in check on the rook's rank / the queen's
    diagonal) without a move.  (Under the reference rules the GPU test itself is the check: its
    reference follows the device's done / reason rows.)"""
    import sys

    sys.path.insert(0, os.path.join(R.ROOT, "tests", "core_host"))
    import corehost as H
    from gym_chess_amd.fen import fen_to_arrays

    def moves(fen):
        b, m = fen_to_arrays(fen, rules="fide")[:2]
        return H.fide_list(b, m)

    root = moves("7k/8/6K1/8/8/8/8/R7 w - - 0 1")
    assert len(root) == 20 and 3584 in root
    assert moves("R6k/8/6K1/8/8/8/8/8 b - - 0 1") == []
    root = moves("4K2k/8/8/6Q1/8/8/8/8 w - - 0 1")
    assert len(root) == 28 and 261 in root
    assert moves("5K1k/8/8/6Q1/8/8/8/8 b - - 0 1") == [463]
    assert 1934 in moves("5K2/7k/8/6Q1/8/8/8/8 w - - 0 1")
    assert moves("5K2/6Qk/8/8/8/8/8/8 b - - 0 1") == []


# --------------------------------------------------------------------------- the solver off
@pytest.mark.parametrize("case", R.SYNTH_CASES[:4])
def test_without_the_solver_it_is_the_parent_class(case):
    """RefSolverTree(solver=False) against AdvTree on R.SYNTH_CASES' inputs: select, backup,
    root_policy and advance give the same bits, and the solver's arrays stay zero"""
    G, nodes, cap, rule, seed, c_puct, fpu = case
    inp = R.synth_run(G, nodes, cap, rule, seed)
    a, b = RefSolverTree(G, nodes, cap, solver=False), A.AdvTree(G, nodes, cap)
    blocks = A.advance_blocks(case, 1)[0]
    for t in (a, b):
        t.reset(*inp["root"], value=inp["root_value"])
    for s in range(inp["sims"]):
        if s == nodes:
            mv = b.root_policy(0, 0, True)["pick"]
            ra, rb = a.advance(mv, *blocks[:3], value=blocks[3]), b.advance(mv, *blocks[:3], value=blocks[3])
            assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))
        outs = [t.select(c_puct, fpu) for t in (a, b)]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(*outs))
        for t in (a, b):
            t.backup(inp["value"][s], inp["done"][s], inp["reason"][s], inp["actions"][s], inp["priors"][s],
                     inp["count"][s])
    for key in R.NODE_KEYS + R.GAME_KEYS + ("path",):
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes(), key
    ra, rb = a.root_policy(3, 1, False), b.root_policy(3, 1, False)
    assert all(ra[k].tobytes() == rb[k].tobytes() for k in rb)
    assert not any(getattr(a, k).any() for k in SOLVER_EDGE_KEYS + SOLVER_NODE_KEYS)
    assert (a.decisions, a.near_ties) == (b.decisions, b.near_ties)


# --------------------------------------------------------------------------- the binding
def test_the_solver_is_declared_and_bound():
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv, SearchTree

    src = open(os.path.join(R.ROOT, "include", "gymchess.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(gc_[a-z0-9_]+)\s*\(", src))
    L = _lib.load()
    for s in SOLVER_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES, s
        assert getattr(L, s) is not None
    assert re.search(r"#define\s+GC_TREE_SOLVER_ARRAYS\s+5\b", src)
    assert len(_lib.SIGNATURES["gc_tree_root_proof"][1]) == 4
    assert SearchTree.SOLVER_ARRAYS == SOLVER_EDGE_KEYS + SOLVER_NODE_KEYS
    for name in ("enable_solver", "root_proof"):
        assert callable(getattr(SearchTree, name, None)), name
    import inspect

    assert "solver" in inspect.signature(BatchedChessEnv.search_tree).parameters
    assert "proof" in inspect.signature(SearchTree.root_policy).parameters
