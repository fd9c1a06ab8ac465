"""CPU: the reference of Gumbel root search on the device tree (gc_tree_gumbel_*,
gym-chess_amd/csrc/gc_tree.h) and the acceptance rule its GPU tests use, restated in numpy on top of
test_tree_search's RefTree (through test_tree_advance's AdvTree, for the runs that advance) and
checked against hand-computed cases.

RefGumbel adds the mode's state: the parameters and the sequential-halving table of enable(), the
three [G][cap] rows of begin() (gumbel, logit, base_visits) and the armed bit.  On an armed tree only
the root's decision changes: v_j = N_j - base_j, t = sum v, c = table[min(considered, nc)][min(t,
sims - 1)], candidates v_j == c (all, if none), score_j = (gumbel_j + logit_j) + ((c_visit + max N) *
c_scale) * qhat_j, qhat_j = Q_j if visited else v_mix.  policy() is gc_tree_gumbel_policy.

Acceptance of a root decision: the candidate set is integer and must match exactly -- the device's
slot must be a candidate.  Scores are float64, computed from the DEVICE's fetched gumbel / logit
rows (begin(rows=...)), so logf differences never enter.  A slot is accepted iff its score is within
32 * 2^-24 * max(1, max|score|) of the best candidate's (the maximum over the root's finite scores):
twice the PUCT rule's term count, for two wave reductions and two more multiplications.  Where
every candidate scores -inf the lowest candidate is the only slot accepted; among candidates with
bitwise equal inputs the chosen one must be the lowest; with a NaN score any slot in range is
accepted.  The reference follows the accepted choice.  Decisions with a second candidate of
different inputs inside the tolerance must stay under 1 % (test_near_ties_are_rare: the seeds of
CASES are chosen so that the reference driven alone stays under it).
"""
import os
import re

import numpy as np
import pytest

import test_policy_sample as P
import test_tree_advance as A
import test_tree_search as R

NONE = R.NONE
TOL = 32 * 2.0 ** -24
GUMBEL_SYMBOLS = ("gc_tree_gumbel_enable", "gc_tree_gumbel_begin", "gc_tree_gumbel_policy", "gc_tree_gumbel_pointers")


def halving_table(considered, sims):
    """table[k][t], k = 0 .. considered: the visits a considered move has when simulation t of a
    search over k considered moves goes to it"""
    t = np.zeros((considered + 1, sims), dtype=np.uint16)
    for k in range(1, considered + 1):
        if k == 1:
            t[k] = np.arange(sims)
            continue
        L = int(np.ceil(np.log2(k)))
        n, r, seq = [0] * k, k, []
        while len(seq) < sims:
            for _ in range(max(1, sims // (L * r))):
                seq += n[:r]
                n[:r] = [x + 1 for x in n[:r]]
            r = max(2, r // 2)
        t[k] = seq[:sims]
    return t


def gumbel_rows(seed, draw, prior, n_children):
    """float64: gumbel_j = -log(-log(u_j)), u_j = ((philox_x0(seed, g * 256 + j, draw) >> 8) + 0.5) *
    2^-24, logit_j = log(prior_j); slots at or past n_children 0 / -inf.  -> (gumbel, logit, words)"""
    G, C = prior.shape
    idx = (np.arange(G, dtype=np.uint64)[:, None] * np.uint64(256) + np.arange(C, dtype=np.uint64)[None, :]).reshape(-1)
    n = (P.philox_x0(int(seed), idx, int(draw)) >> np.uint32(8)).reshape(G, C)
    u = (n.astype(np.float64) + 0.5) * 2.0 ** -24
    on = np.arange(C)[None, :] < np.asarray(n_children)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        logit = np.log(prior.astype(np.float64))
    return np.where(on, -np.log(-np.log(u)), 0.0), np.where(on, logit, -np.inf), n


class RefGumbel(A.AdvTree):
    def __init__(self, games, nodes, cap):
        super().__init__(games, nodes, cap)
        self.params = None
        self.armed = False

    def enable(self, considered=16, sims=32, c_visit=50.0, c_scale=1.0):
        assert 1 <= considered <= self.cap and 1 <= sims <= 65535
        self.params = (int(considered), int(sims), float(np.float32(c_visit)), float(np.float32(c_scale)))
        self.table = halving_table(considered, sims)
        self.gumbel = np.zeros((self.games, self.cap), dtype=np.float32)
        self.logit = np.zeros((self.games, self.cap), dtype=np.float32)
        self.base_visits = np.zeros((self.games, self.cap), dtype=np.int32)
        self.armed = False

    def begin(self, seed, draw, rows=None):
        """rows = (gumbel, logit) fetched from the device; None: the float64 formula, rounded"""
        nc = self.n_children[:, 0]
        if rows is None:
            rows = gumbel_rows(seed, draw, self.prior[:, 0], nc)[:2]
        self.gumbel, self.logit = (np.array(r, dtype=np.float32) for r in rows)
        on = np.arange(self.cap)[None, :] < nc[:, None]
        self.base_visits = np.where(on, self.edge_visits[:, 0], 0).astype(np.int32)
        self.armed = True

    def reset(self, *a, **kw):
        super().reset(*a, **kw)
        self.armed = False

    def advance(self, *a, **kw):
        out = super().advance(*a, **kw)
        self.armed = False
        return out

    # ------------------------------------------------------------------ the root
    def root(self, g, final=False):
        """the root's decision in float64: nc, v, cand, scores, x (logit + sigma), vmix"""
        considered, sims, c_visit, c_scale = self.params
        nc = int(self.n_children[g, 0])
        N = self.edge_visits[g, 0, :nc].astype(np.int64)
        v = N - self.base_visits[g, :nc]
        val = self.edge_value[g, 0, :nc].astype(np.float64)
        pr = self.prior[g, 0, :nc].astype(np.float64)
        lv = float(self.leaf_value[g, 0])
        S, vis = int(N.sum()), N > 0
        q = np.where(vis, val / np.maximum(N, 1), 0.0)
        den = float(pr[vis].sum())
        vmix = lv if S == 0 or den == 0 else (lv + S * float((pr[vis] * q[vis]).sum()) / den) / (1 + S)
        scale = (c_visit + float(N.max() if nc else 0)) * c_scale
        lg = self.logit[g, :nc].astype(np.float64)
        with np.errstate(invalid="ignore"):
            x = lg + scale * np.where(vis, q, vmix)
            scores = (self.gumbel[g, :nc].astype(np.float64) + lg) + scale * np.where(vis, q, vmix)
        if final:
            want = int(v.max()) if nc else 0
        else:
            want = int(self.table[min(considered, nc), min(max(int(v.sum()), 0), sims - 1)])
        cand = v == want
        if not cand.any():
            cand = np.ones(nc, dtype=bool)
        return dict(nc=nc, v=v, cand=cand, scores=scores, x=x, vmix=vmix, want=want)

    def _inputs(self, g, nc):
        return np.stack([self.gumbel[g, :nc].view(np.uint32).astype(np.int64),
                         self.logit[g, :nc].view(np.uint32).astype(np.int64),
                         self.edge_visits[g, 0, :nc].astype(np.int64),
                         self.edge_value[g, 0, :nc].view(np.uint32).astype(np.int64),
                         self.base_visits[g, :nc].astype(np.int64)], axis=1)

    def decide_root(self, g, dev_slot=None, final=False):
        """the root's slot: the reference's (the best candidate, lowest slot), or the device's after
        the acceptance rule"""
        r = self.root(g, final)
        nc, sc, cand = r["nc"], r["scores"], r["cand"]
        first = int(np.flatnonzero(cand)[0])
        self.decisions += 1
        if np.isnan(sc).any():
            j = first if dev_slot is None else int(dev_slot)
            assert 0 <= j < nc, (g, j, nc)
            return j
        cs = np.where(cand, sc, -np.inf)
        best = float(cs.max())
        j = int(np.flatnonzero(cs == best)[0]) if dev_slot is None else int(dev_slot)
        assert 0 <= j < nc, (g, j, nc)
        assert cand[j], f"game {g}: slot {j} has {r['v'][j]} search visits, the candidates have {r['want']}"
        if best == -np.inf:
            assert j == first, (g, j, first)
            return j
        fin = sc[np.isfinite(sc)]
        tol = TOL * max(1.0, float(np.abs(fin).max()))
        assert sc[j] >= best - tol, f"game {g}: slot {j} scores {sc[j]!r}, the best candidate {best!r}"
        tri = self._inputs(g, nc)
        same = np.flatnonzero(cand & (tri == tri[j]).all(axis=1))
        assert j == same[0], f"game {g}: slot {j} chosen, slot {same[0]} has the same inputs"
        if any((tri[i] != tri[j]).any() for i in np.flatnonzero(cs >= best - tol)):
            self.near_ties += 1
        return j

    def _decide(self, g, k, c_puct, fpu, dev_slot):
        if self.armed and k == 0:
            return self.decide_root(g, dev_slot)
        return super()._decide(g, k, c_puct, fpu, dev_slot)

    # ------------------------------------------------------------------ gc_tree_gumbel_policy
    def policy(self):
        """actions / visits / pi (float64) / value (float64) / slot (the reference's own pick, -1
        without children) / pick"""
        assert self.armed
        G, C = self.games, self.cap
        out = dict(actions=self.action[:, 0].copy(), visits=np.zeros((G, C), dtype=np.int32),
                   pi=np.zeros((G, C), dtype=np.float64), value=np.zeros(G, dtype=np.float64),
                   slot=np.full(G, -1, dtype=np.int64), pick=np.full(G, NONE, dtype=np.uint16))
        for g in range(G):
            r = self.root(g, final=True)
            nc = r["nc"]
            out["value"][g] = r["vmix"]
            out["visits"][g, :nc] = self.edge_visits[g, 0, :nc]
            if nc == 0:
                continue
            x = r["x"]
            if np.isfinite(x).any():
                e = np.exp(x - x[np.isfinite(x)].max())
                out["pi"][g, :nc] = e / e.sum()
            n0, t0 = self.decisions, self.near_ties
            out["slot"][g] = self.decide_root(g, None, final=True)
            self.decisions, self.near_ties = n0, t0
            out["pick"][g] = self.action[g, 0, out["slot"][g]]
        return out


def target_of(pi32):
    """d_target from the device's own float32 pi: (int32)(pi * 1048576.0f + 0.5f), in fp32"""
    return (pi32.astype(np.float32) * np.float32(1048576.0) + np.float32(0.5)).astype(np.int32)


def implied_visits(table, k, sims):
    """the sorted search visits (descending) that `sims` simulations over k considered moves leave,
    when each goes to a move with the table's count"""
    n = [0] * k
    for t in range(sims if k else 0):
        n[n.index(int(table[k, t]))] += 1
    return sorted(n, reverse=True)


# --------------------------------------------------------------------------- synthetic runs
# (G, nodes, cap, considered, sims, c_visit, c_scale, seed, open): the GPU tests' runs.  Root child
# counts cycle through 0, 1, 3, cap and random ones, so `considered` lies below, at and above nc in
# every run; cap 200 gives a lane several slots; open = no terminal or childless leaf (the search
# visits then follow the table exactly); the last run's trees fill and overflow.
CASES = [(8, 9, 8, 3, 8, 50.0, 1.0, 41, True),
         (64, 17, 64, 16, 16, 50.0, 1.0, 42, True),
         (8, 6, 200, 100, 5, 50.0, 0.5, 43, True),
         (8, 2, 64, 4, 1, 10.0, 1.0, 44, True),
         (8, 9, 200, 3, 8, 0.0, 2.0, 45, False),
         (8, 6, 8, 4, 16, 50.0, 1.0, 46, False)]
ROOT_COUNTS = ("zero", "one", 3, "cap")
C_PUCT, FPU = 1.25, 0.0


def case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-k{c[3]}-s{c[4]}"


def root_block(rng, G, cap, pri_cap):
    """the roots' rows: child counts 0, 1, 3, cap, then random ones, in R.synth_rows' format"""
    kinds = [{"zero": "zero", "one": "one", "cap": "cap"}.get(ROOT_COUNTS[g], "some") if g < 4 else "some" for g in range(G)]
    a, p, c = R.synth_rows(rng, G, cap, pri_cap, kinds)
    g = 2  # exactly three children
    a[g], p[g], c[g] = NONE, 0, 3
    a[g, :3] = np.sort(rng.choice(4100, size=3, replace=False))
    w = rng.uniform(0.05, 1.0, size=3)
    p[g, :3] = (w / w.sum()).astype(np.float32)
    return a, p, c


def gumbel_run(G, nodes, cap, sims, seed, open_, moves=1):
    """the inputs of `moves` searches of `sims` simulations each: the root block and, per
    simulation, a block, values, done flags and reasons (R.synth_run's format; open_: R.open_run's
    changes), plus an advance block per further move"""
    rng = np.random.RandomState(seed)
    pri_cap = cap + 5
    n = sims * moves
    root = root_block(rng, G, cap, pri_cap)
    root_value = rng.uniform(-1, 1, size=G).astype(np.float32)
    blocks = [R.synth_rows(rng, G, cap, pri_cap) for _ in range(n)]
    inp = dict(root=root, root_value=root_value, actions=np.stack([b[0] for b in blocks]),
               priors=np.stack([b[1] for b in blocks]), count=np.stack([b[2] for b in blocks]),
               value=rng.uniform(-1, 1, size=(n, G)).astype(np.float32), sims=n, pri_cap=pri_cap)
    inp["done"] = (rng.rand(n, G) < 0.1).astype(np.uint8)
    inp["reason"] = np.where(inp["done"] != 0, rng.randint(1, 3, size=(n, G)), 0).astype(np.uint8)
    if open_:
        inp["done"][:] = 0
        inp["reason"][:] = 0
        dead = inp["count"] < 1
        inp["count"][dead] = 1
        inp["actions"][dead, 0] = 7
        inp["priors"][dead, 0] = 1.0
    inp["advance"] = [R.synth_rows(rng, G, cap, pri_cap) + (rng.uniform(-1, 1, size=G).astype(np.float32),)
                      for _ in range(moves - 1)]
    return inp


def run_alone(case):
    G, nodes, cap, considered, sims, c_visit, c_scale, seed, open_ = case
    inp = gumbel_run(G, nodes, cap, sims, seed, open_)
    t = RefGumbel(G, nodes, cap)
    t.enable(considered, sims, c_visit, c_scale)
    t.reset(*inp["root"], value=inp["root_value"])
    t.begin(seed, 3)
    for s in range(sims):
        t.select(C_PUCT, FPU)
        t.backup(inp["value"][s], inp["done"][s], inp["reason"][s], inp["actions"][s], inp["priors"][s], inp["count"][s])
    return t, inp


# --------------------------------------------------------------------------- self-checks
def test_the_table_by_hand():
    for k, sims, seq in ((4, 8, [0, 0, 0, 0, 1, 1, 2, 2]), (2, 4, [0, 0, 1, 1]), (3, 5, [0, 0, 0, 1, 1]), (1, 3, [0, 1, 2])):
        t = halving_table(k, sims)
        assert t.shape == (k + 1, sims) and t.dtype == np.uint16
        assert t[k].tolist() == seq, (k, sims, t[k])
        assert not t[0].any()
    t = halving_table(16, 32)  # 16 moves once, 8 twice (the paper's figure 1), 4 ... until 32 are spent
    assert t[16].tolist() == [0] * 16 + [1] * 8 + [2] * 4 + [3] * 4
    assert implied_visits(halving_table(4, 8), 4, 8) == [3, 3, 1, 1]
    assert halving_table(200, 5)[200].tolist() == [0] * 5 and halving_table(3, 1)[2].tolist() == [0]


def _hand_tree():
    """one game, priors (0.4, 0.3, 0.2, 0.1), root value 0.25, considered 2 of 4, four simulations
    (table 0 0 1 1), c_visit 50, c_scale 1, and chosen noise (0, 1, 0, 2): gumbel + logit =
    -0.916, -0.204, -1.609, -0.303"""
    t = RefGumbel(1, 8, 4)
    t.enable(2, 4, 50.0, 1.0)
    t.reset(*R._block([[(10, 0.4), (20, 0.3), (30, 0.2), (40, 0.1)]], 4), value=np.array([0.25], dtype=np.float32))
    lg = np.log(np.array([[0.4, 0.3, 0.2, 0.1]], dtype=np.float32).astype(np.float64))
    t.begin(0, 0, rows=(np.array([[0, 1, 0, 2]], dtype=np.float32), lg))
    return t


def test_four_simulations_by_hand():
    """1: no visit: v_mix = 0.25, sigma = 50 * 0.25 for every slot, all are candidates -> slot 1
       (the largest gumbel + logit); its leaf is worth +0.5 to its mover: Q_1 = -0.5.
    2: t = 1, c = 0: candidates 0, 2, 3.  v_mix = (0.25 + 1 * (0.3 * -0.5) / 0.3) / 2 = -0.125,
       scale 51: -0.916 - 6.375, -1.609 - 6.375, -0.303 - 6.375 -> slot 3; its leaf is worth -0.5
       to its mover: Q_3 = +0.5.
    3: t = 2, c = 1: candidates 1, 3: -0.204 - 25.5, -0.303 + 25.5 -> slot 3, down to its node
       (one child, PUCT), a leaf worth -0.5: Q_3 = (0.5 - 0.5) / 2 = 0.
    4: t = 3, c = 1: the only candidate is slot 1 (slot 3 has two visits), although it scores
       less; down to its node, a leaf worth +0.75 two plies below the root: Q_1 = (-0.5 + 0.75) / 2.
    policy: the most searched are slots 1 and 3 (2 visits each): scale 52: -0.204 + 52 * 0.125
       against -0.303 + 0 -> slot 1, action 20."""
    t = _hand_tree()
    one = lambda x, dt: np.array([x], dtype=dt)
    leaf = R._block([[(300, 1.0)]], 4)
    r = t.root(0)
    assert r["cand"].all() and r["vmix"] == 0.25 and r["want"] == 0
    assert np.allclose(r["scores"], np.log([0.4, 0.3, 0.2, 0.1]) + [0, 1, 0, 2] + 12.5, atol=1e-6)
    for value, slot, cands, depth in ((0.5, 1, [1, 1, 1, 1], 1), (-0.5, 3, [1, 0, 1, 1], 1), (-0.5, 3, [0, 1, 0, 1], 2),
                                      (0.75, 1, [0, 1, 0, 0], 2)):
        assert t.root(0)["cand"].tolist() == [bool(c) for c in cands]
        t.select(1.0, 0.0)
        assert tuple(t.path[0, 0]) == (0, slot) and t.depth[0] == depth
        t.backup(one(value, np.float32), one(0, np.uint8), one(0, np.uint8), *leaf)
        if slot == 1 and depth == 1:
            r = t.root(0)
            assert abs(r["vmix"] + 0.125) < 1e-12
            assert np.allclose(r["scores"], [-0.9163 - 6.375, -0.2040 - 25.5, -1.6094 - 6.375, -0.3026 - 6.375], atol=1e-3)
    assert t.edge_visits[0, 0].tolist() == [0, 2, 0, 2]
    assert t.edge_value[0, 0].tolist() == [0.0, 0.25, 0.0, 0.0]
    p = t.policy()
    assert p["slot"][0] == 1 and p["pick"][0] == 20 and p["visits"][0].tolist() == [0, 2, 0, 2]
    # v_mix = (0.25 + 4 * (0.3 * 0.125 + 0.1 * 0) / 0.4) / 5; sigma = 52 * (v_mix, 0.125, v_mix, 0)
    vmix = (0.25 + 4 * (0.3 * 0.125) / 0.4) / 5
    assert abs(p["value"][0] - vmix) < 1e-7  # (the priors are float32)
    x = np.log([0.4, 0.3, 0.2, 0.1]) + 52 * np.array([vmix, 0.125, vmix, 0.0])
    assert np.allclose(p["pi"][0], np.exp(x) / np.exp(x).sum(), atol=1e-6) and abs(p["pi"][0].sum() - 1) < 1e-12
    assert target_of(p["pi"][0].astype(np.float32)).sum() in range(1048576 - 4, 1048576 + 5)


def test_candidates_fall_back_and_kept_visits_do_not_count():
    """a root kept by advance carries visits: begin snapshots them and the table counts only the
    visits made since; where no slot has the table's count every slot is a candidate"""
    t = _hand_tree()
    t.edge_visits[0, 0] = [5, 0, 2, 0]
    t.edge_value[0, 0] = [1.0, 0.0, -1.0, 0.0]
    t.begin(0, 0, rows=(t.gumbel, t.logit))
    assert t.base_visits[0].tolist() == [5, 0, 2, 0]
    r = t.root(0)
    assert r["v"].tolist() == [0, 0, 0, 0] and r["cand"].all() and r["want"] == 0
    # S = 7, sum prior * q over the visited = 0.4 * 0.2 + 0.2 * -0.5, prior sum 0.6; max N = 5
    vmix = (0.25 + 7 * (0.4 * 0.2 + 0.2 * -0.5) / 0.6) / 8
    assert abs(r["vmix"] - vmix) < 1e-7  # (the priors are float32)
    assert np.allclose(r["scores"] - (t.gumbel[0] + t.logit[0].astype(np.float64)), 55 * np.array([0.2, vmix, -0.5, vmix]), atol=1e-5)
    t.base_visits[0] = [3, 0, 0, 0]  # v = 2 0 2 0, t = 4 -> the last entry, 1: no slot has one visit
    r = t.root(0)
    assert r["want"] == 1 and r["cand"].all()
    assert t.root(0, final=True)["cand"].tolist() == [True, False, True, False]
    t.reset(*R._block([[(10, 1.0)]], 4))
    assert not t.armed


def test_zero_priors_and_no_children():
    """a prior of 0 has logit -inf and is chosen only when every candidate has one (the lowest);
    pi gives it 0; a childless root has no pick and an all-zero row"""
    t = RefGumbel(2, 4, 3)
    t.enable(3, 2, 50.0, 1.0)
    t.reset(*R._block([[(1, 0.0), (2, 1.0), (3, 0.0)], []], 3), value=np.array([0.5, -0.5], dtype=np.float32))
    t.begin(9, 0)
    assert np.isneginf(t.logit[0, [0, 2]]).all() and t.logit[0, 1] == 0 and np.isneginf(t.logit[1]).all()
    assert not t.gumbel[1].any() and t.gumbel[0].all()
    assert t.decide_root(0) == 1
    t.edge_visits[0, 0, 1] = 1  # slot 1 searched: the candidates left are the two -inf slots
    assert t.decide_root(0) == 0
    with pytest.raises(AssertionError):
        t.decide_root(0, dev_slot=2)
    with pytest.raises(AssertionError):
        t.decide_root(0, dev_slot=1)  # not a candidate
    p = t.policy()
    assert p["pi"][0].tolist() == [0.0, 1.0, 0.0] and not p["pi"][1].any()
    assert p["pick"].tolist() == [2, NONE] and p["value"][1] == -0.5


def test_acceptance_rule_is_not_vacuous():
    """a candidate one part in 10^5 below the best is refused; the best is accepted"""
    t = _hand_tree()
    t.gumbel[0] = [0.71, 1.0, 0, 0]  # gumbel + logit: -0.2063 against -0.2040
    assert t.decide_root(0, dev_slot=1) == 1
    with pytest.raises(AssertionError):
        t.decide_root(0, dev_slot=0)
    t.gumbel[0, 0] = np.float32(1.0 + np.log(0.3) - np.log(0.4)) + np.float32(2e-7)  # inside the tolerance
    assert abs(np.diff(t.root(0)["scores"][:2])[0]) < TOL * 13
    assert t.decide_root(0, dev_slot=0) == 0 and t.decide_root(0, dev_slot=1) == 1 and t.near_ties == 2


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_search_visits_follow_the_table(case):
    """what the GPU runs reach, on the reference alone: every kind of root occurs, and in an open
    run the root's search visits are the multiset the table implies"""
    G, nodes, cap, considered, sims, _, _, _, open_ = case
    t, inp = run_alone(case)
    ncs = t.n_children[:, 0]
    assert ncs[:4].tolist() == [0, 1, 3, cap]
    assert (ncs < considered).any() and (ncs > considered).any() and (considered != 3 or (ncs == considered).any())
    for g in range(G):
        k = min(considered, int(ncs[g]))
        got = sorted(t.edge_visits[g, 0, : ncs[g]].tolist(), reverse=True)
        if open_ and sims <= nodes - 1:
            assert got[:k] == implied_visits(t.table, k, sims) and not any(got[k:]), (g, got)
    if not open_ and sims > nodes - 1:
        assert t.overflow.sum() > 0 and (t.n_nodes == nodes).any()


def test_near_ties_are_rare():
    n = d = 0
    for case in CASES:
        t, _ = run_alone(case)
        t.policy()
        n, d = n + t.near_ties, d + t.decisions
    assert d > 1000
    assert n < 0.01 * d, (n, d)


# --------------------------------------------------------------------------- the property
def _bandit(gumbel, seed=5, G=1024, M=16, sims=16):
    """depth-1 bandit roots: move j of game g is worth q[g, j] to the root's mover whenever it is
    searched (its node is childless, so every later visit backs the same value up).  -> the mean
    true value of the move picked after `sims` simulations"""
    rng = np.random.RandomState(seed)
    w = rng.uniform(0.05, 1.0, size=(G, M))
    prior = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    q = rng.uniform(-1, 1, size=(G, M)).astype(np.float32)
    actions = np.tile(np.arange(M, dtype=np.uint16) * 3, (G, 1))
    t = RefGumbel(G, sims + 1, M)
    t.reset(actions, prior, np.full(G, M, dtype=np.int32))
    if gumbel:
        t.enable(M, sims, 50.0, 1.0)
        t.begin(seed, 0)
    none = (np.full((G, 1), NONE, dtype=np.uint16), np.zeros((G, 1), dtype=np.float32), np.zeros(G, dtype=np.int32))
    zero = np.zeros(G, dtype=np.uint8)
    for _ in range(sims):
        t.select(1.25, 0.0)
        t.backup(-q[np.arange(G), t.path[:, 0, 1]], zero, zero, *none)
    pick = t.policy()["pick"] if gumbel else t.root_policy(seed, 0, False)["pick"]
    return float(q[np.arange(G), pick // 3].mean())


def test_gumbel_picks_better_moves_than_sampled_visit_counts():
    """1 024 bandit roots of 16 moves (values uniform in [-1, 1], independent of the priors), 16
    simulations, seed 5: the mean true value of gumbel_policy's pick is 0.8876, that of
    root_policy's pick sampled from the visit counts of 16 PUCT simulations (c_puct 1.25, fpu 0)
    0.5138.  The best move is worth 0.8897 on average, a uniformly drawn one 0.0035."""
    g, p = _bandit(True), _bandit(False)
    assert g >= p, (g, p)
    assert g > p + 0.2, (g, p)


# --------------------------------------------------------------------------- the binding
def test_gumbel_is_declared_and_bound():
    from gym_chess_amd import _lib
    from gym_chess_amd.env import SearchTree

    src = open(os.path.join(R.ROOT, "include", "gymchess.h")).read()
    assert re.search(r"#define\s+GC_TREE_GUMBEL_ARRAYS\s+4\b", src)
    assert re.search(r"#define\s+GC_TREE_ARRAYS\s+16\b", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(gc_[a-z0-9_]+)\s*\(", src))
    L = _lib.load()
    for s in GUMBEL_SYMBOLS:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
        assert getattr(L, s) is not None
    assert SearchTree.GUMBEL_ARRAYS == ("gumbel", "logit", "base_visits", "table")
    for m in ("enable_gumbel", "gumbel_begin", "gumbel_policy"):
        assert callable(getattr(SearchTree, m, None)), m
