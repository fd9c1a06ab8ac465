"""CPU: the reference of the device search tree (gc_tree_*, gym-chess_amd/csrc/gc_tree.h) and the
acceptance rule its GPU tests use, restated in numpy and checked against hand-computed cases.

RefTree keeps the device's arrays ([G][nodes][cap] action / prior / child / edge_visits /
edge_value, [G][nodes] n_children / parent / parent_slot / leaf_value / terminal, per game n_nodes /
overflow / depth / leaf / leaf_new / path).  Scores are float64; edge values accumulate in
np.float32, one add per edge per simulation, so they must match the device bit for bit.

Acceptance of a selection: at a node with reference scores ref[], the device's slot j is accepted
iff ref[j] >= max(ref) - 16 * 2^-24 * max(1, max|ref|) -- the device computes a score with five
correctly rounded fp32 operations after an exact sum (a division for Q, two multiplications, a
division, an addition; sqrt is one more, and the compiler may contract), each at most 2^-24
relative to a term no larger than max(1, max|ref|) in size; 16 leaves room on both sides of the
comparison.  Among the slots whose (prior, visits, value) triple is bitwise the chosen one's the
chosen slot must be the lowest.  The reference follows the device's accepted choice, so one
near-tie does not derail the rest of a run; decisions in which a second slot with DIFFERENT inputs
lies inside the tolerance must stay under 1 % of all decisions (the seeds below are chosen so that
the reference driven alone stays under it: test_near_ties_are_rare).
"""
import os

import numpy as np
import pytest

import test_policy_sample as P

NONE = 0xFFFF
TOL = 16 * 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_SYMBOLS = ("gc_tree_create", "gc_tree_destroy", "gc_tree_reset", "gc_tree_select", "gc_tree_backup",
                "gc_tree_root_policy", "gc_tree_pointers", "gc_tree_device_bytes")
NODE_KEYS = ("action", "prior", "child", "edge_visits", "edge_value", "n_children", "parent", "parent_slot",
             "leaf_value", "terminal")
GAME_KEYS = ("n_nodes", "overflow", "depth", "leaf", "leaf_new")


class RefTree:
    def __init__(self, games, nodes, cap):
        G, N, C = games, nodes, cap
        self.games, self.nodes, self.cap = G, N, C
        self.action = np.full((G, N, C), NONE, dtype=np.uint16)
        self.prior = np.zeros((G, N, C), dtype=np.float32)
        self.child = np.full((G, N, C), -1, dtype=np.int32)
        self.edge_visits = np.zeros((G, N, C), dtype=np.int32)
        self.edge_value = np.zeros((G, N, C), dtype=np.float32)
        self.n_children = np.zeros((G, N), dtype=np.int32)
        self.parent = np.full((G, N), -1, dtype=np.int32)
        self.parent_slot = np.full((G, N), -1, dtype=np.int32)
        self.leaf_value = np.zeros((G, N), dtype=np.float32)
        self.terminal = np.zeros((G, N), dtype=np.uint8)
        self.n_nodes = np.zeros(G, dtype=np.int32)
        self.overflow = np.zeros(G, dtype=np.int32)
        self.depth = np.zeros(G, dtype=np.int32)
        self.leaf = np.zeros(G, dtype=np.int32)
        self.leaf_new = np.zeros(G, dtype=np.int32)
        self.path = np.zeros((G, N, 2), dtype=np.int32)
        self.decisions = 0
        self.near_ties = 0

    # ------------------------------------------------------------------ node creation
    def _init_node(self, g, k, actions, priors, count, pri_cap, listed=True):
        m = max(0, min(int(count[g]), pri_cap, self.cap)) if listed else 0
        self.action[g, k] = NONE
        self.prior[g, k] = 0
        self.child[g, k] = -1
        self.edge_visits[g, k] = 0
        self.edge_value[g, k] = 0
        self.action[g, k, :m] = actions[g, :m]
        self.prior[g, k, :m] = priors[g, :m]
        self.n_children[g, k] = m

    def reset(self, actions, priors, count, value=None):
        """actions / priors [G][pri_cap], count [G], value [G] or None"""
        pri_cap = actions.shape[1]
        for g in range(self.games):
            self._init_node(g, 0, actions, priors, count, pri_cap)
            self.parent[g, 0] = self.parent_slot[g, 0] = -1
            self.leaf_value[g, 0] = np.float32(0 if value is None else value[g])
            self.terminal[g, 0] = 0
        self.n_nodes[:] = 1
        self.overflow[:] = 0
        self.depth[:] = 0
        self.leaf[:] = 0
        self.leaf_new[:] = 0

    # ------------------------------------------------------------------ selection
    def scores(self, g, k, c_puct, fpu):
        """float64 PUCT scores of node k's children; c_puct / fpu as the kernel gets them (float32)"""
        nc = int(self.n_children[g, k])
        ev = self.edge_visits[g, k, :nc].astype(np.float64)
        val = self.edge_value[g, k, :nc].astype(np.float64)
        pr = self.prior[g, k, :nc].astype(np.float64)
        n_k = 1.0 + ev.sum()
        q = np.where(ev > 0, val / np.maximum(ev, 1.0), float(np.float32(fpu)))
        return q + float(np.float32(c_puct)) * pr * np.sqrt(n_k) / (1.0 + ev)

    def _triples(self, g, k):
        nc = int(self.n_children[g, k])
        return np.stack([self.prior[g, k, :nc].view(np.uint32).astype(np.int64),
                         self.edge_visits[g, k, :nc].astype(np.int64),
                         self.edge_value[g, k, :nc].view(np.uint32).astype(np.int64)], axis=1)

    def _decide(self, g, k, c_puct, fpu, dev_slot):
        """the slot taken at node k: the reference's argmax (lowest slot), or the device's after
        the acceptance rule"""
        if self.n_children[g, k] == 1:  # nothing to score (most of a chain's cost otherwise)
            assert dev_slot is None or int(dev_slot) == 0, (g, k, dev_slot)
            self.decisions += 1
            return 0
        ref = self.scores(g, k, c_puct, fpu)
        best = float(ref.max())
        tol = TOL * max(1.0, float(np.abs(ref).max()))
        inside = np.flatnonzero(ref >= best - tol)
        tri = self._triples(g, k)
        j = int(np.flatnonzero(ref == best)[0]) if dev_slot is None else int(dev_slot)
        assert 0 <= j < ref.size, (g, k, j, ref.size)
        assert ref[j] >= best - tol, f"game {g} node {k}: slot {j} scores {ref[j]!r}, the best {best!r}"
        same = np.flatnonzero((tri == tri[j]).all(axis=1))
        assert j == same[0], f"game {g} node {k}: slot {j} chosen, slot {same[0]} has the same inputs"
        self.decisions += 1
        if any((tri[i] != tri[j]).any() for i in inside):
            self.near_ties += 1
        return j

    def select(self, c_puct=1.25, fpu=0.0, follow=None):
        """One descent per game.  follow = (path [G][nodes][2], depth [G]) fetched from the device:
        every level is then checked against the acceptance rule and followed (the pair a full
        tree drops stays readable at path[depth]).  -> (parent, child, action) [G]"""
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
            v = np.float32(self.leaf_value[g, L])
            for d in range(D):
                k, j = self.path[g, d]
                self.edge_visits[g, k, j] += 1
                self.edge_value[g, k, j] = np.float32(self.edge_value[g, k, j] + (-v if (D - d) & 1 else v))

    # ------------------------------------------------------------------ the root's policy
    @staticmethod
    def sample_slot(visits, x0):
        """the integer rule: r = ((x0 >> 8) * total) >> 24, the first slot whose inclusive visit
        prefix exceeds r"""
        total = int(visits.sum())
        r = ((int(x0) >> 8) * total) >> 24
        return int(np.flatnonzero(np.cumsum(visits.astype(np.int64)) > r)[0])

    def root_policy(self, seed, draw, greedy):
        G, C = self.games, self.cap
        out = dict(actions=self.action[:, 0].copy(), visits=np.zeros((G, C), dtype=np.int32),
                   pi=np.zeros((G, C), dtype=np.float64), value=np.zeros(G, dtype=np.float64),
                   pick=np.full(G, NONE, dtype=np.uint16))
        x0 = P.philox_x0(seed, np.arange(G), draw)
        for g in range(G):
            nc = int(self.n_children[g, 0])
            v = self.edge_visits[g, 0, :nc]
            out["visits"][g, :nc] = v
            total = int(v.sum())
            if total == 0:
                continue
            out["pi"][g, :nc] = v.astype(np.float64) / total
            out["value"][g] = self.edge_value[g, 0, :nc].astype(np.float64).sum() / total
            j = int(np.argmax(v)) if greedy else self.sample_slot(v, x0[g])
            out["pick"][g] = self.action[g, 0, j]
        return out

    def same_as(self, dev):
        """dev: the device's arrays (SearchTree.fetch()); every node below n_nodes bit for bit"""
        for key in GAME_KEYS:
            assert (getattr(self, key) == dev[key]).all(), (key, getattr(self, key), dev[key])
        for g in range(self.games):
            n = int(self.n_nodes[g])
            for key in NODE_KEYS:
                a, b = getattr(self, key)[g, :n], dev[key][g, :n]
                if a.dtype == np.float32:
                    a, b = a.view(np.uint32), b.view(np.uint32)
                assert (a == b).all(), (key, g, np.argwhere(a != b)[:4])


# --------------------------------------------------------------------------- synthetic inputs
# (G, nodes, cap, pri_cap rule, seed, c_puct, fpu); a low fpu makes the trees deep, a high one broad; G = 5 is ragged against the kernels' 4 games
# per workgroup; cap 65 and 256 walk more than one chunk of 64 slots
SYNTH_CASES = [(5, 12, 64, "wide", 1, 1.25, 0.0), (5, 12, 64, "narrow", 2, 2.0, -0.5),
               (3, 40, 1, "wide", 3, 1.25, 0.0), (3, 40, 7, "wide", 4, 1.25, -1.0),
               (3, 40, 7, "narrow", 5, 0.5, -1.0), (3, 40, 65, "wide", 6, 1.25, -1.0),
               (3, 40, 65, "narrow", 7, 1.25, -1.0), (3, 40, 256, "wide", 8, 2.0, -0.5),
               (3, 40, 256, "narrow", 9, 1.25, -1.0)]


def pri_cap_of(cap, rule):
    return cap + 5 if rule == "wide" else max(1, cap // 2)


KINDS = ["zero", "one", "cap", "more", "dead", "some"]
KIND_P = [0.04, 0.08, 0.14, 0.14, 0.04, 0.56]
KIND_P_CHAIN = [0.005, 0.3, 0.3, 0.39, 0.005, 0.0]  # cap 1: a chain, which every dead end stops for good


def synth_rows(rng, G, cap, pri_cap, kinds=None):
    """a priors block as policy_priors writes it (ascending actions, padding 0xFFFF / 0 past
    min(count, pri_cap)) with the counts that matter: 0, 1, cap, more than cap (which a narrow
    block cuts at pri_cap < cap and a wide one hands over to the tree's cap), -1, and random ones;
    a third of the rows carry equal priors (the tie rule)"""
    actions = np.full((G, pri_cap), NONE, dtype=np.uint16)
    priors = np.zeros((G, pri_cap), dtype=np.float32)
    count = np.zeros(G, dtype=np.int32)
    for g in range(G):
        kind = kinds[g] if kinds is not None else rng.choice(KINDS, p=KIND_P_CHAIN if cap == 1 else KIND_P)
        c = {"zero": 0, "one": 1, "cap": cap, "more": cap + 3, "dead": -1}.get(kind)
        if c is None:
            c = int(rng.randint(1, max(2, min(cap, 40)) + 1))
        count[g] = c
        m = max(0, min(c, pri_cap))
        if m:
            actions[g, :m] = np.sort(rng.choice(4100, size=m, replace=False))
            if rng.rand() < 1 / 3:
                priors[g, :m] = np.float32(1.0 / max(c, 1))
            else:
                w = rng.uniform(0.05, 1.0, size=max(c, 1))
                priors[g, :m] = (w / w.sum()).astype(np.float32)[:m]
    return actions, priors, count


def synth_run(G, nodes, cap, rule, seed):
    """the inputs of a whole synthetic run of 2 * nodes simulations: the root block and, per
    simulation, a block, values in [-1, 1], done flags (15 %) and reasons (1 mate / 2 draw)"""
    rng = np.random.RandomState(seed)
    pri_cap = pri_cap_of(cap, rule)
    sims = 2 * nodes
    kinds = ["some", "cap", "more", "zero", "some"][:G]
    root = synth_rows(rng, G, cap, pri_cap, kinds)
    root_value = rng.uniform(-1, 1, size=G).astype(np.float32)
    A = np.zeros((sims, G, pri_cap), dtype=np.uint16)
    Pr = np.zeros((sims, G, pri_cap), dtype=np.float32)
    Cn = np.zeros((sims, G), dtype=np.int32)
    for s in range(sims):
        A[s], Pr[s], Cn[s] = synth_rows(rng, G, cap, pri_cap)
    value = rng.uniform(-1, 1, size=(sims, G)).astype(np.float32)
    done = (rng.rand(sims, G) < (0.01 if cap == 1 else 0.08)).astype(np.uint8)
    reason = np.where(done != 0, rng.randint(1, 3, size=(sims, G)), 0).astype(np.uint8)
    return dict(root=root, root_value=root_value, actions=A, priors=Pr, count=Cn, value=value, done=done,
                reason=reason, sims=sims, pri_cap=pri_cap)


# trees of more than 64 nodes and paths deeper than 64 (the kernels walk nodes and path entries in
# chunks of 64, one lane each): (G, nodes, cap, rule, seed, c_puct, fpu) on open_run's inputs
LARGE_CASES = [(5, 200, 7, "wide", 31, 1.25, -0.5),   # four chunks, broad and deep mixed
               (3, 130, 1, "wide", 21, 1.25, 0.0),    # a chain: depth = n_nodes - 1
               (5, 130, 65, "wide", 35, 1.25, -1.0)]  # two slot chunks x three node chunks
# (the seeds are chosen by test_large_runs_reach_the_later_chunks and test_tree_advance's
# test_large_runs_cross_the_chunks: the last case's first candidate, 33, drops no node past 64 that
# has kept nodes after it)
# the search-only runs: once the chain is full every simulation walks all of it and the
# reference's cost grows with nodes squared, so there it is 70 nodes long
LARGE_SEARCH_CASES = [LARGE_CASES[0], (3, 70, 1, "wide", 21, 1.25, 0.0), LARGE_CASES[2]]


def open_run(G, nodes, cap, rule, seed):
    """synth_run without dead ends below the root (its terminal and childless expansions absorb
    most simulations of a run of more than 100 nodes, and the trees stop growing): no simulation
    block is done, and every row with count < 1 becomes the one-move list (7, prior 1); the root
    block stays, childless root of game 3 included"""
    inp = synth_run(G, nodes, cap, rule, seed)
    inp["done"][:] = 0
    inp["reason"][:] = 0
    dead = inp["count"] < 1
    inp["count"][dead] = 1
    inp["actions"][dead, 0] = 7
    inp["priors"][dead, 0] = 1.0
    return inp


def run_reference(G, nodes, cap, rule, seed, c_puct, fpu, make=None):
    """the reference driven alone through a synthetic run (make: synth_run, or open_run)"""
    inp = (make or synth_run)(G, nodes, cap, rule, seed)
    t = RefTree(G, nodes, cap)
    t.reset(*inp["root"], value=inp["root_value"])
    inp["ended_at_root"] = np.zeros(G, dtype=np.int64)  # simulations whose path is empty
    inp["max_depth"] = 0  # the longest path of the run
    for s in range(inp["sims"]):
        t.select(c_puct, fpu)
        inp["ended_at_root"] += t.depth == 0
        inp["max_depth"] = max(inp["max_depth"], int(t.depth.max()))
        t.backup(inp["value"][s], inp["done"][s], inp["reason"][s], inp["actions"][s], inp["priors"][s],
                 inp["count"][s])
    return t, inp


# --------------------------------------------------------------------------- self-checks
def _block(rows, pri_cap):
    """rows: per game a list of (action, prior)"""
    G = len(rows)
    a = np.full((G, pri_cap), NONE, dtype=np.uint16)
    p = np.zeros((G, pri_cap), dtype=np.float32)
    c = np.zeros(G, dtype=np.int32)
    for g, r in enumerate(rows):
        c[g] = len(r)
        for k, (x, y) in enumerate(r):
            a[g, k], p[g, k] = x, y
    return a, p, c


def test_three_simulations_by_hand():
    """c_puct 1, fpu 0, root priors (0.6, 0.4).
    1: n = 1: scores 0.6, 0.4 -> slot 0, node 1 with value +0.5: edge (0,0) gets -0.5.
    2: n = 2: -0.5 + 0.6 * sqrt2 / 2 = -0.0757, 0 + 0.4 * sqrt2 = 0.5657 -> slot 1, node 2 with
       value -0.25: edge (0,1) gets +0.25.
    3: n = 3: -0.5 + 0.6 * sqrt3 / 2 = 0.0196, 0.25 + 0.4 * sqrt3 / 2 = 0.5964 -> slot 1, down to
       node 2 (one child), slot 0, node 3: mate (done, reason 1) so its value is -1: edge (2,0)
       gets +1 (the mover at node 2 wins), edge (0,1) gets -1."""
    t = RefTree(1, 4, 2)
    t.reset(*_block([[(100, 0.6), (200, 0.4)]], 3))
    one = lambda x, dt: np.array([x], dtype=dt)
    leaf = _block([[(300, 1.0)]], 3)

    p, c, a = t.select(1.0, 0.0)
    assert (p[0], c[0], a[0]) == (0, 1, 100) and t.depth[0] == 1 and tuple(t.path[0, 0]) == (0, 0)
    t.backup(one(0.5, np.float32), one(0, np.uint8), one(0, np.uint8), *leaf)
    assert t.edge_visits[0, 0].tolist() == [1, 0] and t.edge_value[0, 0].tolist() == [-0.5, 0.0]
    assert np.allclose(t.scores(0, 0, 1.0, 0.0), [-0.5 + 0.6 * 2 ** 0.5 / 2, 0.4 * 2 ** 0.5])

    p, c, a = t.select(1.0, 0.0)
    assert (p[0], c[0], a[0]) == (0, 2, 200)
    t.backup(one(-0.25, np.float32), one(0, np.uint8), one(0, np.uint8), *leaf)
    assert t.edge_value[0, 0].tolist() == [-0.5, 0.25]
    assert np.allclose(t.scores(0, 0, 1.0, 0.0), [-0.5 + 0.6 * 3 ** 0.5 / 2, 0.25 + 0.4 * 3 ** 0.5 / 2])

    p, c, a = t.select(1.0, 0.0)
    assert (p[0], c[0], a[0]) == (2, 3, 300) and t.depth[0] == 2
    assert t.path[0, :2].tolist() == [[0, 1], [2, 0]]
    t.backup(one(0.9, np.float32), one(1, np.uint8), one(1, np.uint8), *leaf)  # mate: the value is not read
    assert t.terminal[0, 3] == 1 and t.n_children[0, 3] == 0 and t.leaf_value[0, 3] == -1.0
    assert t.edge_value[0, 2, 0] == 1.0 and t.edge_visits[0, 2, 0] == 1
    assert t.edge_value[0, 0].tolist() == [-0.5, -0.75] and t.edge_visits[0, 0].tolist() == [1, 2]
    assert (t.parent[0, 3], t.parent_slot[0, 3], t.child[0, 2, 0]) == (2, 0, 3)
    r = t.root_policy(0, 0, True)
    assert r["pick"][0] == 200 and r["pi"][0].tolist() == [1 / 3, 2 / 3] and r["value"][0] == -1.25 / 3


def test_terminal_rule_and_full_tree():
    """a drawn leaf is worth 0 and is never expanded; a visit that reaches it adds its value
    again; a full tree counts an overflow, drops the last pair and backs up the node's own value"""
    t = RefTree(1, 2, 1)
    t.reset(*_block([[(7, 1.0)]], 1))
    one = lambda x, dt: np.array([x], dtype=dt)
    row = _block([[(9, 1.0)]], 1)
    t.select()
    t.backup(one(0.7, np.float32), one(1, np.uint8), one(2, np.uint8), *row)  # a draw
    assert t.terminal[0, 1] == 1 and t.leaf_value[0, 1] == 0.0 and t.n_children[0, 1] == 0
    p, c, a = t.select()  # reaches the terminal node: (b)
    assert (p[0], c[0], a[0]) == (-1, -1, NONE) and t.depth[0] == 1 and t.leaf[0] == 1 and not t.leaf_new[0]
    t.backup(one(0.3, np.float32), one(0, np.uint8), one(0, np.uint8), *row)
    assert t.edge_visits[0, 0, 0] == 2 and t.edge_value[0, 0, 0] == 0.0 and t.n_nodes[0] == 2

    t = RefTree(1, 2, 1)
    t.reset(*_block([[(7, 1.0)]], 1))
    t.select()
    t.backup(one(0.5, np.float32), one(0, np.uint8), one(0, np.uint8), *row)
    p, c, a = t.select()  # node 1 wants a child, the tree is full: (c)
    assert (p[0], c[0], a[0]) == (-1, -1, NONE) and t.overflow[0] == 1
    assert t.depth[0] == 1 and t.leaf[0] == 1 and tuple(t.path[0, 1]) == (1, 0)
    t.backup(one(0.1, np.float32), one(0, np.uint8), one(0, np.uint8), *row)
    assert t.edge_visits[0, 0, 0] == 2 and t.edge_value[0, 0, 0] == -1.0 and t.edge_visits[0, 1, 0] == 0

    t = RefTree(1, 3, 4)  # a childless root: nothing to select, nothing backed up
    t.reset(*_block([[]], 2))
    p, c, a = t.select()
    assert (p[0], c[0], a[0]) == (-1, -1, NONE) and t.depth[0] == 0
    t.backup(one(0.1, np.float32), one(0, np.uint8), one(0, np.uint8), *row)
    assert t.root_policy(1, 0, False)["pick"][0] == NONE and t.edge_visits.sum() == 0


@pytest.mark.parametrize("case", SYNTH_CASES)
def test_root_visits_count_the_simulations(case):
    """every simulation adds one visit at the root -- but for those whose path is empty: a
    childless root, or a full tree whose root asks for a new child --; until a tree is full that
    is every simulation; the trees fill and overflow; each kind of count occurs"""
    G, nodes, cap, rule, seed, c_puct, fpu = case
    t, inp = run_reference(*case)
    for g in range(G):
        assert t.edge_visits[g, 0].sum() == inp["sims"] - inp["ended_at_root"][g]
        if t.n_children[g, 0] and not t.overflow[g]:
            assert t.edge_visits[g, 0].sum() == inp["sims"]
        if not t.n_children[g, 0]:
            assert inp["ended_at_root"][g] == inp["sims"]
        n = int(t.n_nodes[g])
        assert (t.edge_visits[g, :n].sum(axis=1)[1:] <= t.edge_visits[g, 0].sum()).all()
    assert t.overflow.sum() > 0 and (t.n_nodes == nodes).any()
    if cap > 1:  # (a chain of single children stops at its first dead end)
        assert t.terminal.sum() > 0
        assert {-1, 0, 1, cap, cap + 3} <= set(inp["count"].reshape(-1).tolist())


@pytest.mark.parametrize("case", SYNTH_CASES)
def test_near_ties_are_rare(case):
    t, _ = run_reference(*case)
    assert t.decisions > 100
    assert t.near_ties < 0.01 * t.decisions, (t.near_ties, t.decisions)


@pytest.mark.parametrize("case", LARGE_SEARCH_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_large_runs_reach_the_later_chunks(case):
    """what makes the GPU test over LARGE_SEARCH_CASES meaningful, on the reference alone: the
    trees fill (so nodes past the first 64 exist and are walked) and overflow, near-ties stay
    under the acceptance rule's cap, and the chain's paths are longer than 64 entries -- nodes - 1
    by construction: at cap 1 with no dead end every game fills (but game 3 of a G > 3 run, whose
    root is childless).  Another seed has to meet the same conditions."""
    G, nodes, cap = case[:3]
    t, inp = run_reference(*case, make=open_run)
    assert nodes > 64
    assert not inp["done"].any() and not inp["reason"].any() and (inp["count"] >= 1).all()
    assert t.overflow.sum() > 0 and (t.n_nodes == nodes).any()
    assert t.decisions > 100
    assert t.near_ties < 0.01 * t.decisions, (t.near_ties, t.decisions)
    if cap == 1:
        assert (t.n_nodes == nodes).all()
        assert inp["max_depth"] == nodes - 1 and inp["max_depth"] >= 65


def test_acceptance_rule_is_not_vacuous():
    """a slot one part in 10^5 below the best is refused, and so is the higher of two slots with
    the same inputs"""
    t = RefTree(1, 2, 3)
    t.reset(*_block([[(1, 0.5), (2, 0.5), (3, 0.49999)]], 3))
    path = np.zeros((1, 2, 2), dtype=np.int32)
    for slot in (1, 2):
        path[0, 0] = (0, slot)
        with pytest.raises(AssertionError):
            t.select(follow=(path, np.array([1])))
    path[0, 0] = (0, 0)
    t.select(follow=(path, np.array([1])))


def test_integer_sampling_against_a_brute_force_cdf():
    rng = np.random.RandomState(5)
    for _ in range(200):
        v = rng.randint(0, 6, size=rng.randint(1, 70)).astype(np.int32)
        if v.sum() == 0:
            v[rng.randint(v.size)] = 3
        line = np.repeat(np.arange(v.size), v)  # slot of every unit of visit mass
        x0 = int(rng.randint(0, 2 ** 32, dtype=np.uint64))
        r = ((x0 >> 8) * int(v.sum())) >> 24
        assert RefTree.sample_slot(v, x0) == line[r]
    v = np.array([0, 2, 0, 1], dtype=np.int32)
    assert RefTree.sample_slot(v, 0) == 1 and RefTree.sample_slot(v, 0xFFFFFFFF) == 3
    # the pick is proportional: over many words each slot's share is its visits' share
    picks = np.bincount([RefTree.sample_slot(v, int(x)) for x in P.philox_x0(3, np.arange(3000), 0)], minlength=4)
    assert picks[0] == picks[2] == 0 and abs(picks[1] / 3000 - 2 / 3) < 0.03


# --------------------------------------------------------------------------- the binding
def test_the_tree_is_declared_and_bound():
    import re

    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    src = open(os.path.join(ROOT, "include", "gymchess.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(gc_[a-z0-9_]+)\s*\(", src))
    for s in TREE_SYMBOLS:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
    assert callable(getattr(BatchedChessEnv, "search_tree", None))
    L = _lib.load()
    for s in TREE_SYMBOLS:
        assert getattr(L, s) is not None
