"""CPU: the reference of the search tree's batched calls (gc_tree_select_batch /
gc_tree_backup_batch: several leaves per game per call, steered apart by a virtual loss), restated
in numpy on top of test_tree_search.RefTree, and its self-checks.

RefTreeBatch adds the scratch of gc_tree_batch_reserve to RefTree's arrays: inflight u8
[G][nodes][cap], b_path i32 [G][K][nodes][2], b_depth / b_leaf / b_kind i32 [G][K], collisions i32
[G].  The descents l = 0 .. leaves - 1 of a game run one after another.  At node k, with f_j =
inflight[k][j]: n_j = edge_visits[j] + f_j, n = 1 + sum_j n_j, Q_j = n_j ? (edge_value[j] - vloss *
f_j) / n_j : fpu, score_j = Q_j + c_puct * prior_j * sqrt(n) / (1 + n_j).  Scores are float64;
edge values accumulate in np.float32, one add per edge per descent in l order, so they must match
the device bit for bit.

Acceptance of a selection, derived as test_tree_search.py derives its own: the device computes a
score with seven correctly rounded fp32 operations after an exact sum (a multiplication and a
subtraction for the numerator of Q -- one fma when the compiler contracts --, a division, then as
before two multiplications, a division and an addition; sqrt is one more), each at most 2^-24
relative to a term that is no larger than max(1, vloss, max|ref|): the new terms are vloss * f_j /
n_j <= vloss (f_j <= n_j) and edge_value[j] / n_j, which is at most 1 in size for values in [-1,
1].  Eight roundings on either side of the comparison are 16; the single-leaf rule leaves a third
more room than its count (12 -> 16), so here the device's slot j is accepted iff ref[j] >= max(ref)
- 24 * 2^-24 * max(1, vloss, max|ref|).  Among the slots whose (prior, visits, value, in flight)
tuple is bitwise the chosen one's the chosen slot must be the lowest.  The reference follows the
device's accepted choice; decisions in which a second slot with DIFFERENT inputs lies inside the
tolerance must stay under 1 % of all decisions (test_near_ties_are_rare chooses the seeds of
BATCH_CASES so that the reference driven alone stays under it).

A round's inputs: descent l of game g reads row g * leaves + l.  The synthetic runs take them from
test_tree_search.synth_run / open_run: round s, descent l reads that run's block s * leaves + l, so
with leaves == 1 the inputs are the single-leaf run's.
"""
import os
import re

import numpy as np
import pytest

import test_tree_search as R

NONE = R.NONE
TOL_B = 24 * 2.0 ** -24
BATCH_SYMBOLS = ("gc_tree_batch_reserve", "gc_tree_select_batch", "gc_tree_backup_batch", "gc_tree_batch_pointers")
BATCH_KEYS = ("inflight", "b_path", "b_depth", "b_leaf", "b_kind", "collisions")


class RefTreeBatch(R.RefTree):
    def __init__(self, games, nodes, cap, max_leaves):
        super().__init__(games, nodes, cap)
        G, N, C, K = games, nodes, cap, max_leaves
        assert 1 <= K <= 64
        self.K = K
        self.inflight = np.zeros((G, N, C), dtype=np.uint8)
        self.b_path = np.zeros((G, K, N, 2), dtype=np.int32)
        self.b_depth = np.zeros((G, K), dtype=np.int32)
        self.b_leaf = np.zeros((G, K), dtype=np.int32)
        self.b_kind = np.zeros((G, K), dtype=np.int32)
        self.collisions = np.zeros(G, dtype=np.int32)
        self.pending_leaves = 0
        self.ends = None  # the last batch's endings: [G][leaves] of "a" / "b" / "c" / "d"
        self.seen = {e: 0 for e in "abcd"}  # endings of every batch so far
        self.new_then_full = 0  # batches of a game in which a new node is followed by an overflow

    def reset(self, *a, **kw):
        super().reset(*a, **kw)
        self.inflight[:] = 0  # (the contract: only while a batch is pending is there anything to clear)
        self.pending_leaves = 0

    # ------------------------------------------------------------------ selection
    def scores_batch(self, g, k, c_puct, fpu, vloss):
        nc = int(self.n_children[g, k])
        f = self.inflight[g, k, :nc].astype(np.float64)
        n_j = self.edge_visits[g, k, :nc].astype(np.float64) + f
        val = self.edge_value[g, k, :nc].astype(np.float64)
        pr = self.prior[g, k, :nc].astype(np.float64)
        n = 1.0 + n_j.sum()
        q = np.where(n_j > 0, (val - float(np.float32(vloss)) * f) / np.maximum(n_j, 1.0), float(np.float32(fpu)))
        return q + float(np.float32(c_puct)) * pr * np.sqrt(n) / (1.0 + n_j)

    def _tuples(self, g, k):
        nc = int(self.n_children[g, k])
        return np.concatenate([self._triples(g, k), self.inflight[g, k, :nc].astype(np.int64)[:, None]], axis=1)

    def _decide_batch(self, g, k, c_puct, fpu, vloss, dev_slot):
        if self.n_children[g, k] == 1:  # nothing to score
            assert dev_slot is None or int(dev_slot) == 0, (g, k, dev_slot)
            self.decisions += 1
            return 0
        ref = self.scores_batch(g, k, c_puct, fpu, vloss)
        best = float(ref.max())
        tol = TOL_B * max(1.0, float(np.float32(vloss)), float(np.abs(ref).max()))
        inside = np.flatnonzero(ref >= best - tol)
        tup = self._tuples(g, k)
        j = int(np.flatnonzero(ref == best)[0]) if dev_slot is None else int(dev_slot)
        assert 0 <= j < ref.size, (g, k, j, ref.size)
        assert ref[j] >= best - tol, f"game {g} node {k}: slot {j} scores {ref[j]!r}, the best {best!r}"
        same = np.flatnonzero((tup == tup[j]).all(axis=1))
        assert j == same[0], f"game {g} node {k}: slot {j} chosen, slot {same[0]} has the same inputs"
        self.decisions += 1
        if any((tup[i] != tup[j]).any() for i in inside):
            self.near_ties += 1
        return j

    def select_batch(self, leaves, c_puct=1.25, fpu=0.0, vloss=1.0, follow=None):
        """`leaves` descents per game.  follow = (b_path [G][K][nodes][2], b_depth [G][K]) fetched
        from the device: every level is then checked against the acceptance rule and followed (the
        pair a full tree drops stays readable at b_path[b_depth]).
        -> (parent, child, action) [G * leaves]"""
        G, N = self.games, self.nodes
        assert 1 <= leaves <= self.K and not self.pending_leaves
        out_p = np.full(G * leaves, -1, dtype=np.int32)
        out_c = np.full(G * leaves, -1, dtype=np.int32)
        out_a = np.full(G * leaves, NONE, dtype=np.uint16)
        self.ends = np.full((G, leaves), "", dtype="U1")
        for g in range(G):
            for l in range(leaves):
                k, D, kind = 0, 0, 0
                while True:
                    if self.n_children[g, k] == 0:  # (b)
                        leaf, end = k, "b"
                        break
                    dev = None
                    if follow is not None:
                        assert D < N and follow[0][g, l, D, 0] == k, (g, l, D, k, follow[0][g, l, D])
                        dev = follow[0][g, l, D, 1]
                    j = self._decide_batch(g, k, c_puct, fpu, vloss, dev)
                    self.b_path[g, l, D] = (k, j)
                    ch, f = int(self.child[g, k, j]), int(self.inflight[g, k, j])
                    if ch < 0 and f == 0 and self.n_nodes[g] >= N:  # (c): the entry dropped, no mark left
                        self.overflow[g] += 1
                        leaf, end = k, "c"
                        break
                    self.inflight[g, k, j] += 1
                    D += 1
                    if ch >= 0:
                        k = ch
                        continue
                    if f > 0:  # (d)
                        leaf, kind, end = k, 2, "d"
                        self.collisions[g] += 1
                    else:  # (a)
                        leaf, kind, end = int(self.n_nodes[g]), 1, "a"
                        self.n_nodes[g] += 1
                        r = g * leaves + l
                        out_p[r], out_c[r], out_a[r] = g * N + k, g * N + leaf, self.action[g, k, j]
                    break
                self.b_depth[g, l], self.b_leaf[g, l], self.b_kind[g, l] = D, leaf, kind
                self.ends[g, l] = end
                self.seen[end] += 1
                if follow is not None:
                    assert follow[1][g, l] == D, (g, l, follow[1][g, l], D)
            e = "".join(self.ends[g])
            if "a" in e and "c" in e[e.index("a"):]:
                self.new_then_full += 1
        self.pending_leaves = leaves
        return out_p, out_c, out_a

    # ------------------------------------------------------------------ backup
    def backup_batch(self, value, done, reason, actions, priors, count):
        """value / done / reason / count [G * leaves], actions / priors [G * leaves][pri_cap]"""
        leaves = self.pending_leaves
        assert leaves
        pri_cap = actions.shape[1]
        for g in range(self.games):
            for l in range(leaves):  # 1. the new nodes
                if self.b_kind[g, l] != 1:
                    continue
                r, D, L = g * leaves + l, int(self.b_depth[g, l]), int(self.b_leaf[g, l])
                k, j = self.b_path[g, l, D - 1]
                fin = bool(done[r])
                # (row r of the block, seen as row g by _init_node)
                self._init_node(g, L, actions[r - g:], priors[r - g:], count[r - g:], pri_cap, listed=not fin)
                self.parent[g, L], self.parent_slot[g, L] = k, j
                self.child[g, k, j] = L
                self.terminal[g, L] = 1 if fin else 0
                self.leaf_value[g, L] = np.float32((-1.0 if reason[r] == 1 else 0.0) if fin else value[r])
            for l in range(leaves):  # 2., 3. the marks taken back, the values added, l ascending
                D, kind = int(self.b_depth[g, l]), int(self.b_kind[g, l])
                v = np.float32(self.leaf_value[g, self.b_leaf[g, l]])
                for d in range(D):
                    k, j = self.b_path[g, l, d]
                    assert self.inflight[g, k, j] > 0
                    self.inflight[g, k, j] -= 1
                    if kind == 2:
                        continue
                    self.edge_visits[g, k, j] += 1
                    self.edge_value[g, k, j] = np.float32(self.edge_value[g, k, j] + (-v if (D - d) & 1 else v))
        self.pending_leaves = 0

    def same_selection_as(self, dev, leaves):
        """dev: the device's scratch after a select_batch (SearchTree.fetch(*BATCH_KEYS))"""
        for key in ("b_depth", "b_leaf", "b_kind"):
            a, b = getattr(self, key)[:, :leaves], dev[key][:, :leaves]
            assert (a == b).all(), (key, a, b)
        for g in range(self.games):
            for l in range(leaves):
                D = int(self.b_depth[g, l])
                assert (self.b_path[g, l, :D] == dev["b_path"][g, l, :D]).all(), (g, l)
        assert (self.inflight == dev["inflight"]).all(), np.argwhere(self.inflight != dev["inflight"])[:4]
        assert (self.collisions == dev["collisions"]).all(), (self.collisions, dev["collisions"])


# --------------------------------------------------------------------------- synthetic inputs
# (G, nodes, cap, K, rule, seed, c_puct, fpu, vloss, inputs): the smallest shapes at which the lane /
# chunk logic can go wrong -- G = 5 ragged against 4 games per workgroup; cap 7 inside a chunk; cap
# 65 and 256 with more than one chunk of 64 slots (the chosen slot's in-flight byte then comes from
# the owner of slot j & 63); the chain (cap 1, 130 nodes, open_run's inputs): paths grow past 64
# entries and every descent after the first of a batch collides or overflows.  One case with
# vloss 0 (the marks then steer through the visit counts alone).
BATCH_CASES = [(5, 24, 64, 4, "wide", 2, 1.25, -1.0, 1.0, "synth"),
               (3, 40, 7, 3, "wide", 4, 1.25, -1.0, 1.0, "synth"),
               (3, 40, 7, 3, "narrow", 11, 1.25, 0.0, 0.0, "synth"),
               (3, 40, 65, 5, "wide", 6, 1.25, -1.0, 1.0, "synth"),
               (3, 40, 256, 2, "wide", 8, 2.0, -0.5, 1.0, "synth"),
               (3, 130, 1, 2, "wide", 21, 1.25, 0.0, 1.0, "open")]
MAKERS = {"synth": R.synth_run, "open": R.open_run}


def case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}k{c[3]}v{c[8]:g}"


def batch_run(G, nodes, cap, K, rule, seed, make="synth"):
    """a synthetic run's inputs regrouped into rounds of K descents: row g * K + l of round s is
    game g's row of the run's block s * K + l"""
    inp = MAKERS[make](G, nodes, cap, rule, seed)
    rounds = inp["sims"] // K

    def regroup(a):
        a = a[: rounds * K]
        a = a.reshape((rounds, K, G) + a.shape[2:])
        return np.ascontiguousarray(np.swapaxes(a, 1, 2)).reshape((rounds, G * K) + a.shape[3:])

    out = {k: regroup(inp[k]) for k in ("actions", "priors", "count", "value", "done", "reason")}
    out.update(root=inp["root"], root_value=inp["root_value"], pri_cap=inp["pri_cap"], rounds=rounds, leaves=K)
    return out


def run_batch_reference(case, vloss=None, K=None):
    """the reference driven alone through a batched synthetic run"""
    G, nodes, cap, K0, rule, seed, c_puct, fpu, vl, make = case
    K = K or K0
    vloss = vl if vloss is None else vloss
    inp = batch_run(G, nodes, cap, K, rule, seed, make)
    t = RefTreeBatch(G, nodes, cap, K)
    t.reset(*inp["root"], value=inp["root_value"])
    inp["ended_at_root"] = np.zeros(G, dtype=np.int64)
    inp["max_depth"] = 0
    for s in range(inp["rounds"]):
        p, c, a = t.select_batch(K, c_puct, fpu, vloss)
        new = c[c >= 0]
        assert np.unique(new).size == new.size  # the kind-1 child outputs are distinct
        assert ((c >= 0) == (t.b_kind[:, :K].reshape(-1) == 1)).all()
        inp["ended_at_root"] += (t.b_depth[:, :K] == 0).sum(axis=1)
        inp["max_depth"] = max(inp["max_depth"], int(t.b_depth.max()))
        t.backup_batch(inp["value"][s], inp["done"][s], inp["reason"][s], inp["actions"][s], inp["priors"][s],
                       inp["count"][s])
        assert not t.inflight.any()
    return t, inp


# --------------------------------------------------------------------------- self-checks
def _one(x, dt):
    return np.array(x, dtype=dt)


def test_two_descents_by_hand():
    """One game, root priors (0.6, 0.4), c_puct 1, fpu 0, vloss 1, K = 2.  Descent 0: n = 1, scores
    0.6 / 0.4 -> slot 0, node 1.  Descent 1: slot 0 is in flight, n = 2: slot 0 scores (0 - 1) / 1 +
    0.6 * sqrt2 / 2 = -0.576, slot 1 scores 0.4 * sqrt2 = 0.566 -> slot 1, node 2.  No collision;
    after the backup (values +0.5, -0.25) nothing is in flight and the edges hold -0.5 and +0.25."""
    t = RefTreeBatch(1, 4, 2, 2)
    t.reset(*R._block([[(100, 0.6), (200, 0.4)]], 3))
    assert np.allclose(t.scores_batch(0, 0, 1.0, 0.0, 1.0), [0.6, 0.4])
    p, c, a = t.select_batch(2, 1.0, 0.0, 1.0)
    assert p.tolist() == [0, 0] and c.tolist() == [1, 2] and a.tolist() == [100, 200]
    assert t.b_kind[0].tolist() == [1, 1] and t.b_depth[0].tolist() == [1, 1] and t.b_leaf[0].tolist() == [1, 2]
    assert t.b_path[0, 0, 0].tolist() == [0, 0] and t.b_path[0, 1, 0].tolist() == [0, 1]
    assert t.inflight[0, 0].tolist() == [1, 1] and t.n_nodes[0] == 3 and t.collisions[0] == 0
    # what descent 1 saw: slot 0 in flight alone
    t.inflight[0, 0, 1] = 0
    assert np.allclose(t.scores_batch(0, 0, 1.0, 0.0, 1.0), [-1 + 0.6 * 2 ** 0.5 / 2, 0.4 * 2 ** 0.5])
    t.inflight[0, 0, 1] = 1
    leaf = R._block([[(300, 1.0)], [(301, 1.0)]], 3)
    t.backup_batch(_one([0.5, -0.25], np.float32), _one([0, 0], np.uint8), _one([0, 0], np.uint8), *leaf)
    assert not t.inflight.any()
    assert t.edge_visits[0, 0].tolist() == [1, 1] and t.edge_value[0, 0].tolist() == [-0.5, 0.25]
    assert t.child[0, 0].tolist() == [1, 2] and t.action[0, 1, 0] == 300 and t.action[0, 2, 0] == 301
    assert t.parent[0, 1:3].tolist() == [0, 0] and t.parent_slot[0, 1:3].tolist() == [0, 1]


def test_one_child_three_descents_by_hand():
    """a root with one child, K = 3: descent 0 allots node 1, descents 1 and 2 find the edge in
    flight: two collisions, whose rows are -1 / -1 / 0xFFFF and whose paths add no visit"""
    t = RefTreeBatch(1, 4, 2, 3)
    t.reset(*R._block([[(7, 1.0)]], 2))
    p, c, a = t.select_batch(3, 1.0, 0.0, 1.0)
    assert p.tolist() == [0, -1, -1] and c.tolist() == [1, -1, -1] and a.tolist() == [7, NONE, NONE]
    assert t.b_kind[0].tolist() == [1, 2, 2] and t.b_depth[0].tolist() == [1, 1, 1] and t.b_leaf[0].tolist() == [1, 0, 0]
    assert t.inflight[0, 0, 0] == 3 and t.collisions[0] == 2 and t.n_nodes[0] == 2
    rows = R._block([[(9, 1.0)], [], []], 2)
    t.backup_batch(_one([0.5, 9, 9], np.float32), _one([0, 1, 1], np.uint8), _one([0, 1, 1], np.uint8), *rows)
    assert not t.inflight.any() and t.collisions[0] == 2
    assert t.edge_visits[0, 0, 0] == 1 and t.edge_value[0, 0, 0] == -0.5 and t.edge_visits[0].sum() == 1
    assert t.terminal[0, 1] == 0 and t.n_children[0, 1] == 1  # (the collision rows were not read)


def test_full_tree_inside_a_batch_by_hand():
    """two nodes, root priors (0.6, 0.4), K = 3: descent 0 allots node 1 and fills the tree;
    descent 1 turns to slot 1, which is not in flight: an overflow whose mark is taken back; descent
    2 sees the same marks as descent 1 and overflows again.  Neither leaves a visit: their paths
    are empty."""
    t = RefTreeBatch(1, 2, 2, 3)
    t.reset(*R._block([[(100, 0.6), (200, 0.4)]], 3), value=_one([0.25], np.float32))
    p, c, a = t.select_batch(3, 1.0, 0.0, 1.0)
    assert c.tolist() == [1, -1, -1] and "".join(t.ends[0]) == "acc" and t.new_then_full == 1
    assert t.overflow[0] == 2 and t.b_depth[0].tolist() == [1, 0, 0] and t.b_kind[0].tolist() == [1, 0, 0]
    assert t.b_path[0, 1, 0].tolist() == [0, 1] and t.inflight[0, 0].tolist() == [1, 0]
    t.backup_batch(_one([0.5, 0, 0], np.float32), _one([0] * 3, np.uint8), _one([0] * 3, np.uint8),
                   *R._block([[(1, 1.0)], [], []], 2))
    assert not t.inflight.any() and t.edge_visits[0, 0].tolist() == [1, 0]


@pytest.mark.parametrize("vloss", [0.0, 1.0, 3.5])
@pytest.mark.parametrize("case", R.SYNTH_CASES)
def test_one_leaf_is_the_single_search(case, vloss):
    """K = 1: nothing is ever in flight when a score is computed, so after every simulation every
    array is RefTree's bit for bit, whatever vloss is"""
    G, nodes, cap, rule, seed, c_puct, fpu = case
    inp = R.synth_run(G, nodes, cap, rule, seed)
    b = batch_run(G, nodes, cap, 1, rule, seed)
    one, bat = R.RefTree(G, nodes, cap), RefTreeBatch(G, nodes, cap, 1)
    one.reset(*inp["root"], value=inp["root_value"])
    bat.reset(*b["root"], value=b["root_value"])
    for s in range(inp["sims"]):
        o1 = one.select(c_puct, fpu)
        o2 = bat.select_batch(1, c_puct, fpu, vloss)
        assert all((x == y).all() for x, y in zip(o1, o2))
        assert (one.depth == bat.b_depth[:, 0]).all() and (one.leaf == bat.b_leaf[:, 0]).all()
        assert (one.leaf_new == bat.b_kind[:, 0]).all()
        for g in range(G):
            D = int(one.depth[g]) + (0 if one.leaf_new[g] or not one.n_children[g, one.leaf[g]] else 1)
            assert (one.path[g, :D] == bat.b_path[g, 0, :D]).all()  # (the pair a full tree dropped included)
        one.backup(inp["value"][s], inp["done"][s], inp["reason"][s], inp["actions"][s], inp["priors"][s], inp["count"][s])
        bat.backup_batch(b["value"][s], b["done"][s], b["reason"][s], b["actions"][s], b["priors"][s], b["count"][s])
        for key in R.NODE_KEYS + ("n_nodes", "overflow"):
            assert getattr(one, key).tobytes() == getattr(bat, key).tobytes(), (s, key)
        assert not bat.inflight.any() and not bat.collisions.any()
    assert one.overflow.sum() > 0


@pytest.fixture(scope="module")
def reference_runs():
    return {case_id(c): run_batch_reference(c) for c in BATCH_CASES}


@pytest.mark.parametrize("case", BATCH_CASES, ids=case_id)
def test_root_visits_count_the_descents(reference_runs, case):
    """after S rounds a game's root visit sum is S * K - collisions - the descents whose path is
    empty (a childless root, or a full tree whose root asks for a new child): a collision adds no
    visit anywhere, every other descent one at the root"""
    G, K = case[0], case[3]
    t, inp = reference_runs[case_id(case)]
    for g in range(G):
        assert t.edge_visits[g, 0].sum() == inp["rounds"] * K - t.collisions[g] - inp["ended_at_root"][g]
        n = int(t.n_nodes[g])
        assert (t.edge_visits[g, :n].sum(axis=1)[1:] <= t.edge_visits[g, 0].sum()).all()
    assert (t.n_nodes == case[1]).any()


@pytest.mark.parametrize("case", BATCH_CASES, ids=case_id)
def test_near_ties_are_rare(reference_runs, case):
    t, _ = reference_runs[case_id(case)]
    assert t.decisions > 100
    assert t.near_ties < 0.01 * t.decisions, (t.near_ties, t.decisions)


def test_the_cases_reach_every_ending(reference_runs):
    """(a) a new node, (b) a terminal or childless node, (c) a full tree and (d) a collision all
    occur, (a), (c) and (d) in every case; some game fills up in the middle of a batch (new nodes,
    then overflows, among the descents of one call); the chain's paths pass 64 entries and each of
    its batches is one real descent and one that collides or overflows"""
    total = {e: 0 for e in "abcd"}
    for c in BATCH_CASES:
        t, inp = reference_runs[case_id(c)]
        for e in "abcd":
            total[e] += t.seen[e]
        assert t.seen["a"] and t.seen["c"] and t.seen["d"], (case_id(c), t.seen)
        if c[2] == 1:
            assert inp["max_depth"] >= 65 and (t.n_nodes == c[1]).all()
            assert t.seen["a"] == 3 * (c[1] - 1) and t.seen["b"] == 0
    assert all(total.values()), total
    assert sum(reference_runs[case_id(c)][0].new_then_full for c in BATCH_CASES) > 0


def test_acceptance_rule_is_not_vacuous():
    """a slot one part in 10^5 below the best is refused, and so is the higher of two slots with the
    same inputs; once the lower one is in flight the inputs differ: the higher one is the best and
    the lower one is refused"""
    def fresh():
        t = RefTreeBatch(1, 4, 3, 2)
        t.reset(*R._block([[(1, 0.5), (2, 0.5), (3, 0.49999)]], 3))
        return t

    path = np.zeros((1, 2, 4, 2), dtype=np.int32)
    depth = np.array([[1, 1]])
    for slot in (1, 2):
        path[0, 0, 0] = (0, slot)
        with pytest.raises(AssertionError):
            fresh().select_batch(1, follow=(path, depth))
    path[0, 0, 0], path[0, 1, 0] = (0, 0), (0, 0)
    with pytest.raises(AssertionError):
        fresh().select_batch(2, follow=(path, depth))
    path[0, 1, 0] = (0, 1)
    t = fresh()
    t.select_batch(2, follow=(path, depth))
    assert t.b_kind[0].tolist() == [1, 1] and t.b_leaf[0].tolist() == [1, 2]


# --------------------------------------------------------------------------- the binding
def test_the_batch_calls_are_declared_and_bound():
    from gym_chess_amd import _lib
    from gym_chess_amd.env import SearchTree

    src = open(os.path.join(R.ROOT, "include", "gymchess.h")).read()
    assert re.search(r"#define\s+GC_TREE_BATCH_ARRAYS\s+6\b", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(gc_[a-z0-9_]+)\s*\(", src))
    for s in BATCH_SYMBOLS:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
    for name in ("reserve_batch", "select_batch", "backup_batch"):
        assert callable(getattr(SearchTree, name, None)), name
    assert SearchTree.BATCH_ARRAYS == BATCH_KEYS
    L = _lib.load()
    for s in BATCH_SYMBOLS:
        assert getattr(L, s) is not None
