"""GPU: Gumbel root search on the device tree (gc_tree_gumbel_* / SearchTree.enable_gumbel) against
RefGumbel and the acceptance rule of test_tree_gumbel.py: begin's rows, whole searches followed
simulation by simulation, searches on roots kept by advance, the improved policy, the sample
store's round trip, the paths the mode must leave alone, the refusals, and NaN / zero priors.
Synthetic trees driven like test_tree_search_gpu.Run; buffers come from gc_device_alloc /
gc_env_copy; no torch."""
import ctypes

import numpy as np
import pytest

import test_tree_advance_gpu as AG
import test_tree_gumbel as GU
import test_tree_search as R
import test_tree_search_gpu as T
from test_policy_priors_gpu import Dev

pytestmark = pytest.mark.gpu

NONE = R.NONE
ROWS = ("gumbel", "logit", "base_visits")


@pytest.fixture(scope="module")
def env():
    """boards for the largest run of GU.CASES (64 games x 17 nodes)"""
    from gym_chess_amd.env import BatchedChessEnv

    e = BatchedChessEnv(1100, device=0, seed=3)
    yield e
    e.close()


class GRun(T.Run):
    """T.Run on a tree with the mode enabled, RefGumbel following"""

    def __init__(self, env, case, moves=1, nodes=None, inp=None):
        G, n0, cap, considered, sims, c_visit, c_scale, seed, open_ = case
        nodes = nodes or n0
        inp = inp or GU.gumbel_run(G, nodes, cap, sims, seed, open_, moves)
        super().__init__(env, G, nodes, cap, inp, GU.C_PUCT, GU.FPU)
        self.ref = GU.RefGumbel(G, nodes, cap)
        self.seed, self.sims, self.considered, self.open = seed, sims, considered, open_
        self.tree.enable_gumbel(considered, sims, c_visit, c_scale)
        self.ref.enable(considered, sims, c_visit, c_scale)

    def begin(self, draw):
        """junk-filled rows -> gumbel_begin; the reference takes the device's gumbel / logit rows"""
        for k in ROWS:
            T.fill(self.env, self.tree.ptr[k], self.G * self.tree.cap * 4)
        self.tree.gumbel_begin(self.seed, draw)
        d = self.tree.fetch(*ROWS)
        self.ref.begin(self.seed, draw, rows=(d["gumbel"], d["logit"]))
        assert (d["base_visits"] == self.ref.base_visits).all()
        return d

    def search_visits(self, g):
        nc = int(self.ref.n_children[g, 0])
        return sorted((self.ref.edge_visits[g, 0, :nc] - self.ref.base_visits[g, :nc]).tolist(), reverse=True)

    def check_table(self):
        """an open search with room for its nodes: the root's search visits are the table's multiset"""
        for g in range(self.G):
            k = min(self.considered, int(self.ref.n_children[g, 0]))
            got = self.search_visits(g)
            assert got[:k] == GU.implied_visits(self.ref.table, k, self.sims) and not any(got[k:]), (g, got)


def check_policy(r):
    """gc_tree_gumbel_policy over junk-filled outputs against RefGumbel.policy()"""
    tree, ref = r.tree, r.ref
    T.fill_arrays(r.env, tree._gpol)
    gp = tree.gumbel_policy()
    assert gp is tree._gpol and gp.gumbel is True
    o, w = gp.fetch(), ref.policy()
    assert (o["actions"] == w["actions"]).all() and (o["visits"] == w["visits"]).all()
    assert np.isfinite(o["pi"]).all() and (np.abs(o["pi"].astype(np.float64) - w["pi"]) <= 1e-5).all()
    sums = o["pi"].astype(np.float64).sum(axis=1)
    empty = ~w["pi"].any(axis=1)
    assert (np.abs(sums[~empty] - 1) <= 1e-5).all() and not o["pi"][empty].any()
    assert (o["target"] == GU.target_of(o["pi"])).all()
    assert (np.abs(o["value"].astype(np.float64) - w["value"]) <= 1e-5).all()
    for g in range(r.G):
        nc = int(ref.n_children[g, 0])
        if nc == 0:
            assert o["pick"][g] == NONE
            continue
        slot = np.flatnonzero(ref.action[g, 0, :nc] == o["pick"][g])
        assert slot.size == 1, (g, o["pick"][g])
        ref.decide_root(g, int(slot[0]), final=True)
    return o, w


# --------------------------------------------------------------------------- 1. begin
@pytest.mark.parametrize("case", [GU.CASES[0], GU.CASES[1], GU.CASES[2]], ids=GU.case_id)
def test_begin(env, case):
    """base_visits exact; gumbel / logit within 2^-18 * max(1, |x|) of the float64 formula from
    the same Philox words (two logf of a few ulp each; a wrong word or formula is off by O(1));
    the padding 0 / -inf / 0 over junk; the same seed and draw give the same bits, another draw
    other noise; the table is the host's; the arrays are counted"""
    r = GRun(env, case)
    G, cap = r.G, r.tree.cap
    plain = env.search_tree(G, r.tree.nodes, cap)
    assert r.tree.device_bytes() >= plain.device_bytes() + 12 * G * cap + 2 * (r.considered + 1) * r.sims
    plain.close()
    assert (r.tree.fetch("table")["table"] == GU.halving_table(r.considered, r.sims)).all()
    r.reset()
    d = r.begin(3)
    nc = r.ref.n_children[:, 0]
    on = np.arange(cap)[None, :] < nc[:, None]
    assert not d["base_visits"].any()
    assert (d["gumbel"][~on] == 0).all() and np.isneginf(d["logit"][~on]).all()
    gum, lg, _ = GU.gumbel_rows(r.seed, 3, r.ref.prior[:, 0], nc)
    for got, want in ((d["gumbel"], gum), (d["logit"], lg)):
        err = np.abs(got[on].astype(np.float64) - want[on])
        assert (err <= 2.0 ** -18 * np.maximum(1, np.abs(want[on]))).all(), err.max()
    again = r.begin(3)
    assert all(d[k].tobytes() == again[k].tobytes() for k in ROWS)
    other = r.begin(4)
    assert other["logit"].tobytes() == d["logit"].tobytes()
    assert (other["gumbel"][on] != d["gumbel"][on]).mean() > 0.99
    r.close()


# --------------------------------------------------------------------------- 2. whole searches
@pytest.mark.parametrize("case", GU.CASES, ids=GU.case_id)
def test_searches(env, case):
    """reset, begin, `sims` simulations: after every selection the root's slot meets the Gumbel
    acceptance rule and every deeper level the PUCT one, the outputs are the reference's; after
    every backup every array of every live node matches bit for bit; an open search leaves the
    table's multiset of visits at the root; then the improved policy"""
    r = GRun(env, case)
    r.reset()
    r.begin(3)
    deepest = 0
    for s in range(r.sims):
        r.simulate(s)
        deepest = max(deepest, int(r.depth.max()))
    if r.open and r.sims <= r.tree.nodes - 1:
        r.check_table()
    if r.sims > r.tree.nodes - 1:
        assert r.ref.overflow.sum() > 0 and (r.ref.n_nodes == r.tree.nodes).any()
    if r.sims >= 8:  # (halving returns to searched moves: the levels below the root are walked)
        assert deepest >= 2
    o, w = check_policy(r)
    assert (w["pick"][r.ref.n_children[:, 0] > 0] != NONE).all()
    assert r.ref.near_ties < 0.01 * r.ref.decisions, (r.ref.near_ties, r.ref.decisions)
    r.close()


# --------------------------------------------------------------------------- 3. kept roots
@pytest.mark.parametrize("case", [(8, 17, 8, 3, 8, 50.0, 1.0, 51, True), (8, 11, 200, 100, 5, 50.0, 1.0, 52, True)],
                         ids=GU.case_id)
def test_search_on_kept_roots(env, case):
    """a search, the tree advanced on gumbel_policy's pick, a second search: advance disarms; begin
    snapshots the kept roots' visits; the second search's visits follow the table; reset disarms"""
    from gym_chess_amd import _lib

    r = GRun(env, case, moves=2)
    tree, ref = r.tree, r.ref
    r.reset()
    r.begin(0)
    for s in range(r.sims):
        r.simulate(s)
    o, w = check_policy(r)
    act, prs, cnt, val = r.inp["advance"][0]
    pri = env.priors_buffer(r.G, cap=r.inp["pri_cap"])
    AG.put_block(env, pri, (act, prs, cnt))
    dval = Dev(env, val)
    adv = tree.advance(tree._gpol.pick, pri, value=dval.ptr).fetch()
    kept, remap = ref.advance(o["pick"], act, prs, cnt, value=val)
    assert (adv["kept"] == kept).all() and (adv["remap"] == remap).all()
    ref.same_as(tree.fetch())
    assert (kept > 1).any() and (kept == 0).any()
    with pytest.raises(_lib.GymChessError, match="armed"):
        tree.gumbel_policy()
    d = r.begin(1)
    assert d["base_visits"].any()  # (kept roots carry visits)
    for s in range(r.sims, 2 * r.sims):
        r.simulate(s)
    r.check_table()
    check_policy(r)
    assert ref.near_ties < 0.01 * ref.decisions, (ref.near_ties, ref.decisions)
    r.reset()
    with pytest.raises(_lib.GymChessError, match="armed"):
        tree.gumbel_policy()
    env.synchronize()
    pri.close()
    dval.close()
    r.close()


# --------------------------------------------------------------------------- 4. the policy's outputs
def test_policy_outputs_are_optional(env):
    """every output may be NULL: a lone output is written as in the full call and the others'
    buffers keep their junk"""
    from gym_chess_amd import _lib

    r = GRun(env, GU.CASES[0])
    r.reset(check=False)
    r.begin(3)
    for s in range(r.sims):
        r.simulate(s, check=False)
    tree = r.tree
    full = tree.gumbel_policy().fetch()
    keys = ("actions", "visits", "pi", "target", "pick", "value")
    _lib.check(tree._L.gc_tree_gumbel_policy(tree._h, None, None, None, None, None, None))
    for k in keys:
        T.fill_arrays(env, tree._gpol)
        _lib.check(tree._L.gc_tree_gumbel_policy(tree._h, *[tree._gpol.ptr[x] if x == k else None for x in keys]))
        o = tree._gpol.fetch()
        assert o[k].tobytes() == full[k].tobytes(), k
        for x in keys:
            if x != k:
                assert (o[x].view(np.uint8) == 0xAB).all(), (k, x)
    r.close()


# --------------------------------------------------------------------------- 5. the sample store
def test_store_round_trip(env):
    """record((actions, target, cap)) and record(gp), commit, sample(index=...): the sparse pi is
    target / sum(target) as the store defines it (float32 quotient of the integers)"""
    r = GRun(env, GU.CASES[0])
    r.reset(check=False)
    r.begin(3)
    for s in range(r.sims):
        r.simulate(s, check=False)
    G, cap = r.G, r.tree.cap
    gp = r.tree.gumbel_policy()
    o = gp.fetch()
    store = env.sample_store(games=G, cap=cap, max_plies=2, capacity=2 * G)
    store.record((gp.actions, gp.target, cap))
    store.record(gp)
    done = Dev(env, np.ones(G, dtype=np.uint8))
    reason = Dev(env, np.full(G, 2, dtype=np.uint8))
    store.commit(done.ptr, reason=reason.ptr)
    live = [g for g in range(G) if o["target"][g].sum() > 0]
    assert len(live) == G - 1  # (game 0 has no children)
    assert store.counters()["total"] == 2 * len(live)
    b = store.sample(2 * len(live), index=np.arange(2 * len(live)), perspective=False, dense=False).fetch()
    for i, g in enumerate(np.repeat(live, 2)):
        n = int((o["actions"][g] != NONE).sum())
        t = o["target"][g, :n]
        want = t.astype(np.float32) / np.float32(t.sum())
        assert (b["pi_index"][i, :n] == o["actions"][g, :n]).all() and (b["pi_index"][i, n:] == -1).all()
        assert b["pi"][i, :n].tobytes() == want.tobytes() and not b["pi"][i, n:].any()
        assert np.abs(b["pi"][i, :n].astype(np.float64) - o["pi"][g, :n]).max() < 4e-6
    env.synchronize()
    store.close()
    done.close()
    reason.close()
    r.close()


# --------------------------------------------------------------------------- 6. untouched paths
def test_a_tree_that_is_not_armed_is_untouched(env):
    """the same inputs through a tree without the mode and through an enabled tree that was never
    armed: every array bitwise equal after every simulation (the junk past n_nodes included)"""
    case = GU.CASES[5]
    G, nodes, cap, considered, sims = case[:5]
    inp = GU.gumbel_run(G, nodes, cap, sims, case[7], False)
    plain = T.Run(env, G, nodes, cap, inp, GU.C_PUCT, GU.FPU)
    idle = GRun(env, case, inp=inp)
    for r in (plain, idle):
        r.reset(check=False)
    for s in range(sims):
        for r in (plain, idle):
            r.simulate(s, check=False)
        a, b = plain.tree.fetch(), idle.tree.fetch()
        assert all(a[k].tobytes() == b[k].tobytes() for k in a), s
        sa, sb = plain.tree._sel.fetch(), idle.tree._sel.fetch()
        assert all(sa[k].tobytes() == sb[k].tobytes() for k in sa), s
    assert a["overflow"].sum() > 0
    assert not idle.tree.fetch("gumbel")["gumbel"].any()  # (zero-filled, never written)
    plain.close()
    idle.close()


# --------------------------------------------------------------------------- 7. refusals
def test_refusals(env):
    from gym_chess_amd import _lib

    L, G, NODES, CAP = env._L, 4, 8, 16
    inp = R.synth_run(G, NODES, CAP, "wide", 12)
    a, p, c = (Dev(env, x) for x in inp["root"])
    v = Dev(env, inp["root_value"])
    done = Dev(env, np.zeros(G, dtype=np.uint8))
    pc = inp["pri_cap"]
    tree = env.search_tree(G, NODES, cap=CAP)
    t, sel = tree._h, tree._sel.ptr
    sp, sc, sa = sel["parent"], sel["child"], sel["action"]
    back = (v.ptr, done.ptr, done.ptr, a.ptr, p.ptr, c.ptr, pc)
    out = (ctypes.c_void_p * 4)()
    _lib.check(L.gc_tree_reset(t, a.ptr, p.ptr, c.ptr, pc, v.ptr))
    before = tree.fetch()

    def refused(fn, *args, match=None):
        with pytest.raises(_lib.GymChessError, match=match) as ei:
            _lib.check(fn(*args))
        assert str(ei.value), args

    def untouched():
        now = tree.fetch()
        assert all(before[k].tobytes() == now[k].tobytes() for k in before)

    # before enable
    refused(L.gc_tree_gumbel_begin, t, ctypes.c_uint64(1), 0)
    refused(L.gc_tree_gumbel_policy, t, None, None, None, None, None, None)
    refused(L.gc_tree_gumbel_pointers, t, out, 4)
    # enable's limits
    for args in ((None, 4, 8, 50.0, 1.0), (t, 0, 8, 50.0, 1.0), (t, CAP + 1, 8, 50.0, 1.0), (t, 4, 0, 50.0, 1.0),
                 (t, 4, 65536, 50.0, 1.0), (t, 4, 8, -1.0, 1.0), (t, 4, 8, float("nan"), 1.0), (t, 4, 8, float("inf"), 1.0),
                 (t, 4, 8, 50.0, 0.0), (t, 4, 8, 50.0, -1.0), (t, 4, 8, 50.0, float("nan")), (t, 4, 8, 50.0, float("inf"))):
        refused(L.gc_tree_gumbel_enable, *args)
    refused(L.gc_tree_gumbel_pointers, t, out, 4)  # (still not enabled)
    # a pending selection
    _lib.check(L.gc_tree_select(t, 1.25, 0.0, sp, sc, sa))
    refused(L.gc_tree_gumbel_enable, t, 4, 8, 50.0, 1.0, match="pending")
    _lib.check(L.gc_tree_backup(t, *back))
    before = tree.fetch()
    # enabled: limits of the extremes are values
    _lib.check(L.gc_tree_gumbel_enable(t, CAP, 65535, 0.0, 1e-3))
    bytes_big = tree.device_bytes()
    _lib.check(L.gc_tree_gumbel_enable(t, 1, 1, 50.0, 1.0))  # other parameters: reallocated
    assert tree.device_bytes() < bytes_big
    tree.enable_gumbel(4, 8, 50.0, 1.0)
    n = tree.device_bytes()
    tree.gumbel_begin(5, 0)
    tree.enable_gumbel(4, 8, 50.0, 1.0)  # the same parameters: nothing happens, still armed
    assert tree.device_bytes() == n
    tree.gumbel_policy()
    tree.enable_gumbel(4, 8, 50.0, 2.0)  # other parameters disarm
    refused(L.gc_tree_gumbel_policy, t, None, None, None, None, None, None, match="armed")
    refused(L.gc_tree_gumbel_pointers, t, out, 0)
    refused(L.gc_tree_gumbel_pointers, t, None, 4)
    refused(L.gc_tree_gumbel_pointers, None, out, 4)
    refused(L.gc_tree_gumbel_begin, None, ctypes.c_uint64(1), 0)
    refused(L.gc_tree_gumbel_policy, None, None, None, None, None, None, None)
    # the solver and the batch calls on a gumbel tree
    refused(L.gc_tree_solver_enable, t, match="gumbel")
    refused(L.gc_tree_batch_reserve, t, 4, match="gumbel")
    untouched()
    # every call while a selection is pending (an armed tree's)
    tree.gumbel_begin(5, 0)
    _lib.check(L.gc_tree_select(t, 1.25, 0.0, sp, sc, sa))
    before = tree.fetch()
    rows = tree.fetch(*ROWS)
    refused(L.gc_tree_gumbel_enable, t, 4, 8, 50.0, 1.0, match="pending")
    refused(L.gc_tree_gumbel_enable, t, 2, 8, 50.0, 1.0, match="pending")
    refused(L.gc_tree_gumbel_begin, t, ctypes.c_uint64(6), 0, match="pending")
    refused(L.gc_tree_gumbel_policy, t, None, None, None, None, None, None, match="pending")
    refused(L.gc_tree_select, t, 1.25, 0.0, sp, sc, sa)
    untouched()
    now = tree.fetch(*ROWS)
    assert all(rows[k].tobytes() == now[k].tobytes() for k in ROWS)
    _lib.check(L.gc_tree_gumbel_pointers(t, out, 4))  # (no launch: allowed at any time)
    assert [out[i] for i in range(4)] == [tree.ptr[k] for k in tree.GUMBEL_ARRAYS]
    _lib.check(L.gc_tree_backup(t, *back))
    refused(L.gc_tree_backup, t, *back)  # nothing was left pending
    tree.gumbel_policy()
    # enable on a solver tree / a tree with a batch scratch
    solver = env.search_tree(G, NODES, cap=CAP, solver=True)
    refused(L.gc_tree_gumbel_enable, solver._h, 4, 8, 50.0, 1.0, match="solver")
    batch = env.search_tree(G, NODES, cap=CAP)
    batch.reserve_batch(2)
    refused(L.gc_tree_gumbel_enable, batch._h, 4, 8, 50.0, 1.0, match="batch")
    with pytest.raises(ValueError):
        batch.gumbel_policy()
    env.synchronize()
    for x in (tree, solver, batch, a, p, c, v, done):
        x.close()


# --------------------------------------------------------------------------- 8. NaN and zero priors
@pytest.mark.parametrize("cap", [8, 200])
def test_nan_and_zero_priors_stay_in_range(env, cap):
    """roots whose priors are NaN, zero or both, in every slot or in some: every index the kernels
    produce is in range (slots below n_children, nodes below n_nodes, boards of the game)"""
    G, nodes, considered, sims = 8, 7, min(cap, 70), 6
    case = (G, nodes, cap, considered, sims, 50.0, 1.0, 61, True)
    inp = GU.gumbel_run(G, nodes, cap, sims, 61, True)
    pr = inp["root"][1]
    n = inp["root"][2].clip(0, cap)
    pr[1, :] = np.where(pr[1] > 0, np.nan, 0)  # all NaN
    pr[2, 0] = np.nan                          # one NaN of three
    pr[3, :] = 0                               # all zero, nc = cap
    pr[4, : n[4] // 2] = 0                     # the first half zero
    pr[5, n[5] - 1] = np.nan
    inp["root_value"][6] = np.nan              # a NaN root value: NaN v_mix
    inp["priors"][:, 7, 0] = np.nan            # NaN priors below the root
    r = GRun(env, case, inp=inp)
    r.reset(check=False)
    r.begin(2)
    for s in range(sims):
        r.simulate(s, check=False)
        d = r.tree.fetch()
        o = r.tree._sel.fetch()
        for g in range(G):
            D, nn = int(d["depth"][g]), int(d["n_nodes"][g])
            assert 0 <= D < nodes and 1 <= nn <= nodes
            for k, j in d["path"][g, :D]:
                assert 0 <= k < nn and 0 <= j < d["n_children"][g, k], (s, g, k, j)
            if o["child"][g] >= 0:
                assert g * nodes <= o["parent"][g] < o["child"][g] < g * nodes + nn and o["action"][g] != NONE
        assert (d["edge_visits"][:, 0].sum(axis=1) == (s + 1) * (d["n_children"][:, 0] > 0)).all()
    T.fill_arrays(env, r.tree._gpol)
    o = r.tree.gumbel_policy().fetch()
    for g in range(G):
        nc = int(d["n_children"][g, 0])
        assert (o["pick"][g] in d["action"][g, 0, :nc]) if nc else o["pick"][g] == NONE
        assert (o["actions"][g] == d["action"][g, 0]).all() and (o["visits"][g, nc:] == 0).all()
        assert not o["pi"][g, nc:].any() and not o["target"][g, nc:].any()
    assert not o["pi"][3].any() and not o["pi"][0].any()  # every logit -inf; no children
    assert o["pi"][4, : n[4] // 2].tolist() == [0.0] * (n[4] // 2) and abs(o["pi"][4].sum() - 1) < 1e-5
    r.close()


# --------------------------------------------------------------------------- 9. the documented loop
def test_the_move_loop_with_chess():
    """INTEGRATION's per-move loop on real positions, three moves of 8 games: advance (reset for
    the first move) -> the roots cloned -> gumbel_begin -> SIMS x six launches -> gumbel_policy ->
    record -> step, with seeded bf16 pseudo-logits and values in place of a network.  The reference
    follows every selection; the games play gumbel_policy's picks; the store ends up with the
    improved policies of the games that finished (commit with every game marked done)."""
    import test_policy_sample as P
    from gym_chess_amd.env import BatchedChessEnv

    G, SIMS, CAP, MOVES = 8, 8, 64, 3
    NODES = 2 * SIMS + 1
    rng = np.random.RandomState(71)
    game = BatchedChessEnv(G, device=0, seed=5)
    gio = game.device_io()
    for _ in range(2):  # (two random plies: real positions, and the mask of the position to move from)
        game.step_device(gio, autoreset=True)
    tenv = BatchedChessEnv(G * NODES, device=0, seed=6)
    tio = tenv.device_io(pick=False)
    n = MOVES * (SIMS + 1)
    raw, _ = P.quantise(rng.uniform(-3, 3, size=(n, G, 4100)).astype(np.float32), "bfloat16")
    values = rng.uniform(-1, 1, size=(n, G)).astype(np.float32)
    logits, vals = Dev(tenv, raw), Dev(tenv, values)
    row_bytes = G * 4100 * 2
    tree = tenv.search_tree(G, NODES, cap=CAP)
    tree.enable_gumbel(considered=4, sims=SIMS)
    ref = GU.RefGumbel(G, NODES, CAP)
    ref.enable(4, SIMS)
    store = game.sample_store(cap=CAP, max_plies=MOVES, capacity=G * MOVES)
    gpri, pri, rows = game.priors_buffer(G, cap=CAP), tenv.priors_buffer(G, cap=CAP), tenv.rows_buffer(G)
    roots = np.arange(G) * NODES
    moves, targets = None, []
    for m in range(MOVES):
        b = m * (SIMS + 1) + SIMS  # the root's block; the simulations' are m * (SIMS + 1) + s
        game.policy_priors(gio, logits.ptr + b * row_bytes, gpri, dtype="bfloat16")
        game.synchronize()
        h = gpri.fetch()
        if m == 0:
            tree.reset(gpri, value=vals.ptr + 4 * G * b)
            ref.reset(h["actions"], h["priors"], h["count"], value=values[b])
        else:
            adv = tree.advance(moves, gpri, value=vals.ptr + 4 * G * b).fetch()
            kept, _ = ref.advance(moves, h["actions"], h["priors"], h["count"], value=values[b])
            assert (adv["kept"] == kept).all() and (kept > 0).all()
        tenv.clone_boards(game, np.arange(G), roots)
        tree.gumbel_begin(draw=m)
        d = tree.fetch(*ROWS)
        ref.begin(tenv.seed, m, rows=(d["gumbel"], d["logit"]))
        assert (d["base_visits"] == ref.base_visits).all() and (m == 0 or d["base_visits"].any())
        ref.same_as(tree.fetch())
        for s in range(SIMS):
            k = m * (SIMS + 1) + s
            sel = tree.select(GU.C_PUCT, GU.FPU)
            tenv.clone_boards(tenv, sel.parent, sel.child, count=G)
            tenv.step_boards(tio, sel.child, sel.action, rows=G, out=rows)
            tenv.policy_priors(tio, logits.ptr + k * row_bytes, pri, boards=sel.child, rows=G, dtype="bfloat16")
            tree.backup(vals.ptr + 4 * G * k, rows, pri)
            f = tree.fetch("path", "depth")
            wp, wc, wa = ref.select(GU.C_PUCT, GU.FPU, follow=(f["path"], f["depth"]))
            o, st, pr = sel.fetch(), rows.fetch("done", "reason"), pri.fetch()
            assert (o["parent"] == wp).all() and (o["child"] == wc).all() and (o["action"] == wa).all()
            ref.backup(values[k], st["done"], st["reason"], pr["actions"], pr["priors"], pr["count"])
            ref.same_as(tree.fetch())
        gp = tree.gumbel_policy()
        o, w = gp.fetch(), ref.policy()
        assert (np.abs(o["pi"].astype(np.float64) - w["pi"]) <= 1e-5).all() and (o["pick"] != NONE).all()
        for g in range(G):
            ref.decide_root(g, int(np.flatnonzero(ref.action[g, 0] == o["pick"][g])[0]), final=True)
        lm = game.legal_mask()
        assert all(lm[g, o["pick"][g]] for g in range(G))
        tenv.synchronize()  # (gp's buffers were written on the tree env's stream, the store is the game env's)
        store.record(gp)
        targets.append(o["target"].copy())
        game.step_device(gio, actions=gp.pick, autoreset=True)
        assert not gio.fetch("done")["done"].any()  # three plies in: nobody is done
        moves = o["pick"]
    assert ref.near_ties < 0.01 * ref.decisions, (ref.near_ties, ref.decisions)
    done = Dev(game, np.ones(G, dtype=np.uint8))
    reason = Dev(game, np.full(G, 2, dtype=np.uint8))
    store.commit(done.ptr, reason=reason.ptr)
    assert store.counters()["total"] == G * MOVES
    vis = store.fetch("ring_vis")["ring_vis"].reshape(G, MOVES, CAP)
    for m in range(MOVES):
        assert (vis[:, m] == targets[m]).all()
    game.synchronize()
    tenv.synchronize()
    store.close()
    tree.close()
    for x in (logits, vals, pri, rows, gpri, tio, gio, done, reason):
        x.close()
    tenv.close()
    game.close()
