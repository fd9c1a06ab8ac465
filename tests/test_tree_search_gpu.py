"""GPU: the device search tree (gc_tree_* / BatchedChessEnv.search_tree) against RefTree and the
acceptance rule of test_tree_search.py: synthetic trees that fill and overflow at every cap that
takes another path, trees of more than 64 nodes with paths of more than 64 entries, placement, the root's policy, the full chess loop under both rule sets, and
the state and argument errors.  Buffers come from gc_device_alloc / gc_env_copy; no torch."""
import ctypes

import numpy as np
import pytest

import test_policy_sample as P
import test_tree_search as R
from test_policy_priors_gpu import Dev

pytestmark = pytest.mark.gpu

NONE = R.NONE


def fill(env, ptr, nbytes):
    """nbytes at ptr become 0xAB, so a store the kernel skips shows"""
    from gym_chess_amd import _lib

    junk = np.full(nbytes, 0xAB, dtype=np.uint8)
    if nbytes:
        _lib.check(env._L.gc_env_copy(env._h, ptr, _lib.ptr(junk), ctypes.c_uint64(nbytes), 1))


def fill_arrays(env, arrays):
    """every buffer of a SearchTree's selection / root-policy block"""
    for k, p in arrays.ptr.items():
        dt, shape = arrays._spec[k]
        fill(env, p, int(np.prod(shape)) * np.dtype(dt).itemsize)


def fill_tree(env, tree):
    for k in tree.ARRAYS:
        fill(env, tree.ptr[k], int(np.prod(tree._shape(k))) * np.dtype(tree._DTYPES.get(k, np.int32)).itemsize)


class Run:
    """one synthetic run on the device, simulation by simulation, with the reference following"""

    def __init__(self, env, G, nodes, cap, inp, c_puct, fpu):
        self.env, self.L, self.G, self.inp = env, env._L, G, inp
        self.c_puct, self.fpu = c_puct, fpu
        self.tree = env.search_tree(G, nodes, cap)
        self.ref = R.RefTree(G, nodes, cap)
        self.bufs = {k: Dev(env, inp[k]) for k in ("actions", "priors", "count", "value", "done", "reason")}
        self.root = [Dev(env, a) for a in inp["root"]] + [Dev(env, inp["root_value"])]
        self.pc = inp["pri_cap"]

    def reset(self, check=True):
        from gym_chess_amd import _lib

        fill_tree(self.env, self.tree)
        a, p, c, v = (b.ptr for b in self.root)
        _lib.check(self.L.gc_tree_reset(self.tree._h, a, p, c, self.pc, v))
        self.ref.reset(*self.inp["root"], value=self.inp["root_value"])
        if check:
            self.ref.same_as(self.tree.fetch())

    def simulate(self, s, check=True):
        from gym_chess_amd import _lib

        G, pc, b = self.G, self.pc, self.bufs
        fill_arrays(self.env, self.tree._sel)
        sel = self.tree.select(self.c_puct, self.fpu)
        if check:
            d = self.tree.fetch("path", "depth")
            self.depth = d["depth"]  # (the device's, of this selection)
            want = self.ref.select(self.c_puct, self.fpu, follow=(d["path"], d["depth"]))
            o = sel.fetch()
            for got, w, name in zip((o["parent"], o["child"], o["action"]), want, ("parent", "child", "action")):
                assert (got == w).all(), (s, name, got, w)
        _lib.check(self.L.gc_tree_backup(self.tree._h, b["value"].ptr + 4 * G * s, b["done"].ptr + G * s,
                                         b["reason"].ptr + G * s, b["actions"].ptr + 2 * G * pc * s,
                                         b["priors"].ptr + 4 * G * pc * s, b["count"].ptr + 4 * G * s, pc))
        if check:
            i = self.inp
            self.ref.backup(i["value"][s], i["done"][s], i["reason"][s], i["actions"][s], i["priors"][s], i["count"][s])
            self.ref.same_as(self.tree.fetch())

    def close(self):
        self.env.synchronize()
        self.tree.close()
        for b in list(self.bufs.values()) + self.root:
            b.close()


@pytest.fixture(scope="module")
def env():
    from gym_chess_amd.env import BatchedChessEnv

    e = BatchedChessEnv(160, device=0, seed=3)
    yield e
    e.close()


# --------------------------------------------------------------------------- 1. synthetic trees
@pytest.mark.parametrize("case", R.SYNTH_CASES)
def test_synthetic_trees(env, case):
    """2 * nodes simulations: after every selection each level of the device's path meets the
    acceptance rule and the outputs are the reference's; after every backup every array of every
    live node matches bit for bit"""
    G, nodes, cap, rule, seed, c_puct, fpu = case
    r = Run(env, G, nodes, cap, R.synth_run(G, nodes, cap, rule, seed), c_puct, fpu)
    r.reset()
    for s in range(r.inp["sims"]):
        r.simulate(s)
    assert r.ref.overflow.sum() > 0 and (r.ref.n_nodes == nodes).any()
    assert r.ref.near_ties < 0.01 * r.ref.decisions, (r.ref.near_ties, r.ref.decisions)
    r.close()


@pytest.fixture(scope="module")
def large_env():
    """boards for the trees of R.LARGE_CASES (5 x 200 nodes)"""
    from gym_chess_amd.env import BatchedChessEnv

    e = BatchedChessEnv(1000, device=0, seed=3)
    yield e
    e.close()


@pytest.mark.parametrize("case", R.LARGE_SEARCH_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_large_synthetic_trees(large_env, case):
    """test_synthetic_trees on trees of more than 64 nodes (R.open_run's inputs, which keep such
    trees growing): the same checks after every selection and every backup.  The chain's paths
    grow past 64 entries, so k_tree_backup's lanes take a second path entry each and all of them
    are compared bit for bit (edge_visits, edge_value)."""
    G, nodes, cap, rule, seed, c_puct, fpu = case
    r = Run(large_env, G, nodes, cap, R.open_run(G, nodes, cap, rule, seed), c_puct, fpu)
    r.reset()
    deepest = 0
    for s in range(r.inp["sims"]):
        r.simulate(s)
        deepest = max(deepest, int(r.depth.max()))
    assert r.ref.overflow.sum() > 0 and (r.ref.n_nodes == nodes).any()
    assert r.ref.near_ties < 0.01 * r.ref.decisions, (r.ref.near_ties, r.ref.decisions)
    if cap == 1:
        assert deepest >= 65, deepest
    r.close()


# --------------------------------------------------------------------------- 2. placement
def _game0(inp, g=0):
    """the inputs of game g alone"""
    one = {k: np.ascontiguousarray(inp[k][:, g: g + 1]) for k in ("actions", "priors", "count", "value", "done", "reason")}
    one["root"] = tuple(np.ascontiguousarray(a[g: g + 1]) for a in inp["root"])
    one["root_value"] = inp["root_value"][g: g + 1].copy()
    one["pri_cap"], one["sims"] = inp["pri_cap"], inp["sims"]
    return one


def test_placement_and_repeatability(env):
    """game 0 after 20 simulations: the same bits alone (G = 1) and as one of five, and in a
    second run"""
    inp = R.synth_run(5, 12, 64, "wide", 1)
    got = []
    for G, data in ((5, inp), (5, inp), (1, _game0(inp))):
        r = Run(env, G, 12, 64, data, 1.25, -1.0)
        r.reset(check=False)
        for s in range(20):
            r.simulate(s, check=False)
        got.append(r.tree.fetch())
        r.close()
    n = int(got[0]["n_nodes"][0])
    assert n > 3
    for key in R.NODE_KEYS + R.GAME_KEYS + ("path",):
        a, b, c = (g[key] for g in got)
        assert a.tobytes() == b.tobytes(), key  # the same run twice, all five games, junk included
        x, y = (a[0][:n], c[0][:n]) if key in R.NODE_KEYS else (a[0], c[0])
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), key


# --------------------------------------------------------------------------- 3. the root's policy
def _check_root(r, draws):
    from gym_chess_amd import _lib

    tree, ref = r.tree, r.ref
    for greedy in (True, False):
        for draw in draws:
            fill_arrays(r.env, tree._root)
            o = tree.root_policy(greedy=greedy, seed=77, draw=draw).fetch()
            w = ref.root_policy(77, draw, greedy)
            assert (o["actions"] == w["actions"]).all() and (o["visits"] == w["visits"]).all()
            assert (np.abs(o["pi"].astype(np.float64) - w["pi"]) <= 2.0 ** -22 * np.abs(w["pi"])).all()
            assert (np.abs(o["value"].astype(np.float64) - w["value"]) <= 2.0 ** -22 * np.abs(w["value"])).all()
            assert (o["pick"] == w["pick"]).all(), (greedy, draw, o["pick"], w["pick"])
    # every output is optional
    _lib.check(tree._L.gc_tree_root_policy(tree._h, ctypes.c_uint64(1), 0, 0, None, None, None, None, None))
    return w


@pytest.mark.parametrize("case", [R.SYNTH_CASES[0], R.SYNTH_CASES[5], R.SYNTH_CASES[8]])
def test_root_policy(env, case):
    """visits / actions exact, pi and the value within 2^-22 of the float64 quotients, the greedy
    and the sampled pick exact over 8 draws; before any visit (all zero, no pick), and after a
    run in which (case 0) game 3's root is childless"""
    G, nodes, cap, rule, seed, c_puct, fpu = case
    r = Run(env, G, nodes, cap, R.synth_run(G, nodes, cap, rule, seed), c_puct, fpu)
    r.reset()
    w = _check_root(r, (0,))
    assert (w["pick"] == NONE).all() and not w["visits"].any() and not w["pi"].any()
    for s in range(nodes + 3):
        r.simulate(s)
    w = _check_root(r, range(8))
    if G == 5:
        assert r.ref.n_children[3, 0] == 0 and w["pick"][3] == NONE and w["value"][3] == 0
    assert (w["pick"][r.ref.n_children[:, 0] > 0] != NONE).all()
    if fpu == 0.0:  # a broad search spreads the root's visits: the draws differ
        assert len({tuple(r.ref.root_policy(77, d, False)["pick"]) for d in range(8)}) > 1
    r.close()


# --------------------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("rules", ["reference", "fide"])
def test_end_to_end_with_chess(rules):
    """8 games 6 plies in, a tree env of 8 x 17 boards, 24 simulations of the documented loop
    with seeded bf16 pseudo-logits and values in place of a network.  The first 16 simulations
    search broadly (fpu 0) and cannot overflow: a 17-node tree is full after 16 expansions at the
    earliest.  The last 8 run with c_puct 1, fpu -6: an unvisited child then scores at most -6 + 5 *
    prior <= -1 (sqrt(1 + n) <= 5), below every visited child's Q + U > -1, so at the root -- which
    has a visited child -- the descent always goes down, every path holds the root's edge, and the
    root's visits count all 24 simulations while the full trees overflow further down."""
    from gym_chess_amd.env import BatchedChessEnv

    G, NODES, CAP, SIMS = 8, 17, 64, 24
    settings = [(1.25, 0.0)] * (NODES - 1) + [(1.0, -6.0)] * (SIMS - NODES + 1)
    rng = np.random.RandomState(31)
    game = BatchedChessEnv(G, device=0, seed=5, rules=rules)
    gio = game.device_io()
    for _ in range(6):
        game.step_device(gio, autoreset=True)
    tenv = BatchedChessEnv(G * NODES, device=0, seed=6, rules=rules)
    tio = tenv.device_io(pick=False)
    raw, _ = P.quantise(rng.uniform(-3, 3, size=(SIMS + 1, G, 4100)).astype(np.float32), "bfloat16")
    values = rng.uniform(-1, 1, size=(SIMS + 1, G)).astype(np.float32)
    logits, vals = Dev(tenv, raw), Dev(tenv, values)
    row_bytes = G * 4100 * 2

    # the roots: priors from the game env's mask, boards cloned into slot g * NODES
    gpri = game.priors_buffer(G, cap=CAP)
    game.policy_priors(gio, logits.ptr + SIMS * row_bytes, gpri, dtype="bfloat16")
    game.synchronize()  # (the tree lives on the tree env's stream)
    tree = tenv.search_tree(G, NODES, cap=CAP)
    ref = R.RefTree(G, NODES, CAP)
    tree.reset(gpri, value=vals.ptr + 4 * G * SIMS)
    h = gpri.fetch()
    ref.reset(h["actions"], h["priors"], h["count"], value=values[SIMS])
    tenv.clone_boards(game, np.arange(G), np.arange(G) * NODES)
    ref.same_as(tree.fetch())
    assert (ref.n_children[:, 0] >= 5).all()  # real positions

    pri = tenv.priors_buffer(G, cap=CAP)
    rows = tenv.rows_buffer(G)
    for s in range(SIMS):
        C_PUCT, FPU = settings[s]
        fill_arrays(tenv, tree._sel)
        sel = tree.select(C_PUCT, FPU)
        tenv.clone_boards(tenv, sel.parent, sel.child, count=G)
        tenv.step_boards(tio, sel.child, sel.action, rows=G, out=rows)
        tenv.policy_priors(tio, logits.ptr + s * row_bytes, pri, boards=sel.child, rows=G, dtype="bfloat16")
        tree.backup(vals.ptr + 4 * G * s, rows, pri)

        d = tree.fetch("path", "depth")
        wp, wc, wa = ref.select(C_PUCT, FPU, follow=(d["path"], d["depth"]))
        o, st, pr = sel.fetch(), rows.fetch("done", "reason"), pri.fetch()
        assert (o["parent"] == wp).all() and (o["child"] == wc).all() and (o["action"] == wa).all()
        for g in range(G):
            if wc[g] < 0:
                assert st["reason"][g] == 255 and pr["count"][g] == -1
                continue
            k = wp[g] - g * NODES
            assert o["action"][g] in ref.action[g, k, : ref.n_children[g, k]]
            assert st["reason"][g] not in (6, 255), (s, g, st["reason"][g])
        ref.backup(values[s], st["done"], st["reason"], pr["actions"], pr["priors"], pr["count"])
        ref.same_as(tree.fetch())

    assert (ref.edge_visits[:, 0].sum(axis=1) == SIMS).all()
    assert ref.overflow.sum() > 0  # (the -1 rows were exercised)
    assert ref.near_ties < 0.01 * ref.decisions
    assert (ref.n_nodes > 4).all()
    # every node's stored child list = the legal actions of its slot, ascending, cut at cap
    lm = tenv.legal_mask()
    for g in range(G):
        for k in range(int(ref.n_nodes[g])):
            if ref.terminal[g, k]:
                assert ref.n_children[g, k] == 0
                continue
            legal = np.flatnonzero(lm[g * NODES + k, :4100])[:CAP]
            assert ref.n_children[g, k] == legal.size and (ref.action[g, k, : legal.size] == legal).all(), (g, k)
    tenv.synchronize()
    tree.close()
    for b in (logits, vals, pri, rows, gpri, tio, gio):
        b.close()
    tenv.close()
    game.close()


# --------------------------------------------------------------------------- 5. state and argument errors
def test_state_and_argument_errors(env):
    from gym_chess_amd import _lib

    L, G, NODES, CAP = env._L, 4, 8, 16
    inp = R.synth_run(G, NODES, CAP, "wide", 12)
    a, p, c = (Dev(env, x) for x in inp["root"])
    v = Dev(env, inp["root_value"])
    done = Dev(env, np.zeros(G, dtype=np.uint8))
    pc = inp["pri_cap"]
    tree = env.search_tree(G, NODES, cap=CAP)
    t, sel, root = tree._h, tree._sel.ptr, tree._root.ptr

    def refused(fn, *args):
        with pytest.raises(_lib.GymChessError) as ei:
            _lib.check(fn(*args))
        assert str(ei.value), args

    # create
    h = ctypes.c_void_p()
    for args in ((None, G, NODES, CAP, ctypes.byref(h)), (env._h, G, NODES, CAP, None), (env._h, 0, NODES, CAP, ctypes.byref(h)),
                 (env._h, G, 0, CAP, ctypes.byref(h)), (env._h, G, NODES, 0, ctypes.byref(h)),
                 (env._h, G, NODES, 257, ctypes.byref(h)), (env._h, env.num_boards // NODES + 1, NODES, CAP, ctypes.byref(h)),
                 (env._h, 1, env.num_boards + 1, CAP, ctypes.byref(h))):
        refused(L.gc_tree_create, *args)
    assert not h.value
    with pytest.raises(_lib.GymChessError):
        env.search_tree(env.num_boards + 1, 1)

    _lib.check(L.gc_tree_reset(t, a.ptr, p.ptr, c.ptr, pc, None))  # the value is optional
    _lib.check(L.gc_tree_reset(t, a.ptr, p.ptr, c.ptr, pc, v.ptr))
    before = tree.fetch()

    def untouched():
        now = tree.fetch()
        assert all(before[k].tobytes() == now[k].tobytes() for k in before)

    for args in ((None, a.ptr, p.ptr, c.ptr, pc, v.ptr), (t, None, p.ptr, c.ptr, pc, v.ptr), (t, a.ptr, None, c.ptr, pc, v.ptr),
                 (t, a.ptr, p.ptr, None, pc, v.ptr), (t, a.ptr, p.ptr, c.ptr, 0, v.ptr)):
        refused(L.gc_tree_reset, *args)
    sp, sc, sa = sel["parent"], sel["child"], sel["action"]
    for args in ((None, 1.25, 0.0, sp, sc, sa), (t, 1.25, 0.0, None, sc, sa), (t, 1.25, 0.0, sp, None, sa),
                 (t, 1.25, 0.0, sp, sc, None), (t, -0.5, 0.0, sp, sc, sa), (t, float("nan"), 0.0, sp, sc, sa),
                 (t, float("inf"), 0.0, sp, sc, sa), (t, 1.25, float("nan"), sp, sc, sa)):
        refused(L.gc_tree_select, *args)
    back = (v.ptr, done.ptr, done.ptr, a.ptr, p.ptr, c.ptr, pc)
    refused(L.gc_tree_backup, t, *back)  # nothing is pending
    for flags in (2, 3, -1):
        refused(L.gc_tree_root_policy, t, ctypes.c_uint64(1), 0, flags, root["actions"], None, None, None, None)
    refused(L.gc_tree_root_policy, None, ctypes.c_uint64(1), 0, 0, root["actions"], None, None, None, None)
    out = (ctypes.c_void_p * 16)()
    refused(L.gc_tree_pointers, t, out, 0)
    refused(L.gc_tree_pointers, t, None, 16)
    refused(L.gc_tree_pointers, None, out, 16)
    refused(L.gc_tree_destroy, None)
    assert L.gc_tree_device_bytes(None) == 0 and tree.device_bytes() >= G * NODES * CAP * 18
    untouched()

    # the pending bit
    _lib.check(L.gc_tree_select(t, 0.0, float("inf"), sp, sc, sa))  # c_puct 0 and an infinite fpu are values
    before = tree.fetch()
    refused(L.gc_tree_select, t, 1.25, 0.0, sp, sc, sa)
    refused(L.gc_tree_root_policy, t, ctypes.c_uint64(1), 0, 1, root["actions"], None, None, None, None)
    for k in range(7):  # each argument of the backup in turn
        bad = list(back)
        bad[k] = 0 if k == 6 else None
        refused(L.gc_tree_backup, t, *bad)
    refused(L.gc_tree_backup, None, *back)
    untouched()
    _lib.check(L.gc_tree_backup(t, *back))
    refused(L.gc_tree_backup, t, *back)
    _lib.check(L.gc_tree_root_policy(t, ctypes.c_uint64(1), 0, 1, root["actions"], None, None, None, None))
    _lib.check(L.gc_tree_select(t, 1.25, 0.0, sp, sc, sa))
    _lib.check(L.gc_tree_reset(t, a.ptr, p.ptr, c.ptr, pc, v.ptr))  # clears the pending selection
    _lib.check(L.gc_tree_select(t, 1.25, 0.0, sp, sc, sa))
    _lib.check(L.gc_tree_backup(t, *back))

    # the wrapper's own checks
    small = env.priors_buffer(G - 1, cap=CAP)
    rows = env.rows_buffer(G)
    with pytest.raises(ValueError):
        tree.reset(small)
    with pytest.raises(TypeError):
        tree.reset(a.ptr)
    tree.select()
    with pytest.raises(TypeError):
        tree.backup(v.ptr, None, small)
    with pytest.raises(ValueError):
        tree.backup(None, rows, small)
    env.synchronize()
    tree.close()
    for b in (a, p, c, v, done, small, rows):
        b.close()
