"""GPU: the search tree's batched calls (gc_tree_select_batch / gc_tree_backup_batch,
SearchTree.select_batch / backup_batch: several leaves per game per call with a virtual loss)
against RefTreeBatch and the acceptance rule of test_tree_batch.py: synthetic trees at every shape
that takes another path, one leaf per call against the single-leaf calls on the device,
repeatability, the full chess loop with games * leaves rows under both rule sets, and the state and
argument errors.  Buffers come from gc_device_alloc / gc_env_copy; no torch."""
import ctypes

import numpy as np
import pytest

import test_clone_gpu as CG
import test_policy_sample as P
import test_tree_advance as A
import test_tree_batch as B
import test_tree_search as R
import test_tree_search_gpu as T
from test_policy_priors_gpu import Dev

pytestmark = pytest.mark.gpu

NONE = R.NONE


class BatchRun:
    """one batched synthetic run on the device, round by round, with the reference following"""

    def __init__(self, env, case, K=None, inp=None, ref=None):
        G, nodes, cap, K0, rule, seed, self.c_puct, self.fpu, self.vloss, make = case
        self.K = K = K or K0
        self.env, self.L, self.G = env, env._L, G
        self.inp = inp = inp or B.batch_run(G, nodes, cap, K, rule, seed, make)
        self.tree = env.search_tree(G, nodes, cap)
        self.ref = ref or B.RefTreeBatch(G, nodes, cap, K)
        self.bufs = {k: Dev(env, inp[k]) for k in ("actions", "priors", "count", "value", "done", "reason")}
        self.root = [Dev(env, a) for a in inp["root"]] + [Dev(env, inp["root_value"])]
        self.pc = inp["pri_cap"]

    def reset(self, check=True):
        from gym_chess_amd import _lib

        T.fill_tree(self.env, self.tree)  # the tree's arrays junk; the scratch as reserve leaves it: zeros
        self.tree.reserve_batch(self.K)
        a, p, c, v = (b.ptr for b in self.root)
        _lib.check(self.L.gc_tree_reset(self.tree._h, a, p, c, self.pc, v))
        self.ref.reset(*self.inp["root"], value=self.inp["root_value"])
        if check:
            self.ref.same_as(self.tree.fetch())
            d = self.tree.fetch(*B.BATCH_KEYS)
            assert not any(d[k].any() for k in B.BATCH_KEYS)

    def round(self, s, check=True):
        from gym_chess_amd import _lib

        n, pc, b, K = self.G * self.K, self.pc, self.bufs, self.K
        sel = self.tree.select_batch(K, self.c_puct, self.fpu, self.vloss)
        if check:
            d = self.tree.fetch(*B.BATCH_KEYS)
            self.depth = d["b_depth"]
            want = self.ref.select_batch(K, self.c_puct, self.fpu, self.vloss, follow=(d["b_path"], d["b_depth"]))
            self.ref.same_selection_as(d, K)
            o = sel.fetch()
            for name, w in zip(("parent", "child", "action"), want):
                assert o[name].shape == w.shape and (o[name] == w).all(), (s, name, o[name], w)
        _lib.check(self.L.gc_tree_backup_batch(self.tree._h, b["value"].ptr + 4 * n * s, b["done"].ptr + n * s,
                                               b["reason"].ptr + n * s, b["actions"].ptr + 2 * n * pc * s,
                                               b["priors"].ptr + 4 * n * pc * s, b["count"].ptr + 4 * n * s, pc))
        if check:
            i = self.inp
            self.ref.backup_batch(i["value"][s], i["done"][s], i["reason"][s], i["actions"][s], i["priors"][s],
                                  i["count"][s])
            self.ref.same_as(self.tree.fetch())
            d = self.tree.fetch("inflight", "collisions")
            assert not d["inflight"].any(), np.argwhere(d["inflight"])[:4]
            assert (d["collisions"] == self.ref.collisions).all(), (d["collisions"], self.ref.collisions)

    def close(self):
        self.env.synchronize()
        self.tree.close()
        for b in list(self.bufs.values()) + self.root:
            b.close()


@pytest.fixture(scope="module")
def env():
    """boards for the trees of B.BATCH_CASES (3 x 130 nodes)"""
    from gym_chess_amd.env import BatchedChessEnv

    e = BatchedChessEnv(400, device=0, seed=3)
    yield e
    e.close()


# --------------------------------------------------------------------------- 1. synthetic trees
@pytest.mark.parametrize("case", B.BATCH_CASES, ids=B.case_id)
def test_synthetic_batches(env, case):
    """2 * nodes / K rounds of K descents: after every select_batch each level of every descent's
    path meets the acceptance rule, b_path / b_depth / b_kind / b_leaf, the in-flight marks and the
    three outputs are the reference's; after every backup_batch every array of every live node
    matches bit for bit, nothing is in flight and the collision counts agree"""
    G, nodes, cap, K = case[:4]
    r = BatchRun(env, case)
    r.reset()
    deepest = 0
    for s in range(r.inp["rounds"]):
        r.round(s)
        deepest = max(deepest, int(r.depth.max()))
    ref = r.ref
    assert ref.seen["a"] and ref.seen["c"] and ref.seen["d"], ref.seen
    assert ref.overflow.sum() > 0 and (ref.n_nodes == nodes).any()
    assert ref.near_ties < 0.01 * ref.decisions, (ref.near_ties, ref.decisions)
    if cap == 1:
        assert deepest >= 65, deepest
    assert r.tree.device_bytes() >= G * nodes * cap * 19 + 8 * G * K * nodes
    r.close()


# --------------------------------------------------------------------------- 2. one leaf per call
def test_one_leaf_is_the_single_search_on_the_device(env):
    """the same inputs through select / backup on one tree and through select_batch(1) /
    backup_batch on another, both junk-filled first: after every simulation the ten node arrays,
    n_nodes and overflow are identical bit for bit over their whole extent (junk included), and
    the pending path is: depth / leaf / leaf_new / path of the one against b_depth / b_leaf /
    b_kind / b_path of the other (a path's entries up to its depth; what lies past it is the
    fill's junk in the one and the reservation's zeros in the other)"""
    G, nodes, cap, rule, seed, c_puct, fpu = case = R.SYNTH_CASES[0]
    inp = R.synth_run(G, nodes, cap, rule, seed)
    one = T.Run(env, G, nodes, cap, inp, c_puct, fpu)
    bat = BatchRun(env, (G, nodes, cap, 1, rule, seed, c_puct, fpu, 1.0, "synth"))
    one.reset(check=False)
    bat.reset(check=False)
    from gym_chess_amd import _lib

    for s in range(inp["sims"]):
        sel = one.tree.select(c_puct, fpu)
        bsel = bat.tree.select_batch(1, c_puct, fpu, 1.0)
        a, b = one.tree.fetch("depth", "leaf", "leaf_new", "path"), bat.tree.fetch(*B.BATCH_KEYS)
        assert (a["depth"] == b["b_depth"][:, 0]).all() and (a["leaf"] == b["b_leaf"][:, 0]).all()
        assert (a["leaf_new"] == b["b_kind"][:, 0]).all()
        for g in range(G):
            D = int(a["depth"][g])
            assert a["path"][g, :D].tobytes() == b["b_path"][g, 0, :D].tobytes(), (s, g)
        o, bo = sel.fetch(), bsel.fetch()
        assert all(o[k].tobytes() == bo[k].tobytes() for k in o), (s, o, bo)
        x = one.bufs
        _lib.check(one.L.gc_tree_backup(one.tree._h, x["value"].ptr + 4 * G * s, x["done"].ptr + G * s,
                                        x["reason"].ptr + G * s, x["actions"].ptr + 2 * G * one.pc * s,
                                        x["priors"].ptr + 4 * G * one.pc * s, x["count"].ptr + 4 * G * s, one.pc))
        x = bat.bufs
        _lib.check(bat.L.gc_tree_backup_batch(bat.tree._h, x["value"].ptr + 4 * G * s, x["done"].ptr + G * s,
                                              x["reason"].ptr + G * s, x["actions"].ptr + 2 * G * bat.pc * s,
                                              x["priors"].ptr + 4 * G * bat.pc * s, x["count"].ptr + 4 * G * s, bat.pc))
        a, b = one.tree.fetch(), bat.tree.fetch()
        for key in R.NODE_KEYS + ("n_nodes", "overflow"):
            assert a[key].tobytes() == b[key].tobytes(), (s, key)
        d = bat.tree.fetch("inflight", "collisions")
        assert not d["inflight"].any() and not d["collisions"].any()
    assert a["overflow"].sum() > 0 and (a["n_nodes"] == nodes).any()
    one.close()
    bat.close()


# --------------------------------------------------------------------------- 3. repeatability
def test_repeatability(env):
    """the same batch sequence twice: bit-identical trees (junk included) and scratch"""
    case = B.BATCH_CASES[3]  # two slot chunks, five leaves
    got = []
    for _ in range(2):
        r = BatchRun(env, case)
        r.reset(check=False)
        for s in range(r.inp["rounds"]):
            r.round(s, check=False)
        got.append(dict(r.tree.fetch(), **r.tree.fetch(*B.BATCH_KEYS)))
        r.close()
    assert (got[0]["n_nodes"] > 5).any() and got[0]["collisions"].sum() > 0
    for key in got[0]:
        assert got[0][key].tobytes() == got[1][key].tobytes(), key


# --------------------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("rules", ["reference", "fide"])
def test_end_to_end_with_chess(rules):
    """4 games 6 plies in, a tree env of 4 x 14 boards, 6 rounds of 4 leaves through the documented
    loop -- select_batch -> clone_boards -> step_boards -> encode_planes_rows -> policy_priors ->
    backup_batch, every env call with games * leaves = 16 rows -- on seeded bf16 pseudo-logits and
    values in place of a network.  The first three rounds search broadly (fpu 0), the others with
    c_puct 1, fpu -6 (the descents then go down through visited children, so the rows of a batch
    meet: collisions, and a 14-node tree overflows).  The rows without a new node (a collision, a
    full tree, a terminal node) are skipped by every env call as documented: reason 255, count -1,
    a zero planes row.  At the end every created node's board is the position reached by playing
    the node's path of actions from its root: replayed on a second env with the dense step (which
    the oracle's digests pin), and, under the reference rules, each step also against the C
    oracle's next_state from the parent's board."""
    from gym_chess_amd.env import BatchedChessEnv

    G, K, NODES, CAP, ROUNDS = 4, 4, 14, 64, 6
    N = G * K
    settings = [(1.25, 0.0)] * 3 + [(1.0, -6.0)] * (ROUNDS - 3)
    rng = np.random.RandomState(37)
    game = BatchedChessEnv(G, device=0, seed=5, rules=rules)
    gio = game.device_io()
    for _ in range(6):
        game.step_device(gio, autoreset=True)
    tenv = BatchedChessEnv(G * NODES, device=0, seed=6, rules=rules)
    tio = tenv.device_io(pick=False)
    raw, _ = P.quantise(rng.uniform(-3, 3, size=(ROUNDS + 1, N, 4100)).astype(np.float32), "bfloat16")
    values = rng.uniform(-1, 1, size=(ROUNDS + 1, N)).astype(np.float32)
    logits, vals = Dev(tenv, raw), Dev(tenv, values)
    row_bytes = N * 4100 * 2

    gpri = game.priors_buffer(G, cap=CAP)
    game.policy_priors(gio, logits.ptr + ROUNDS * row_bytes, gpri, dtype="bfloat16")
    game.synchronize()  # (the tree lives on the tree env's stream)
    tree = tenv.search_tree(G, NODES, cap=CAP)
    ref = B.RefTreeBatch(G, NODES, CAP, K)
    tree.reset(gpri, value=vals.ptr + 4 * N * ROUNDS)
    h = gpri.fetch()
    ref.reset(h["actions"], h["priors"], h["count"], value=values[ROUNDS, :G])
    tenv.clone_boards(game, np.arange(G), np.arange(G) * NODES)
    ref.same_as(tree.fetch())
    assert (ref.n_children[:, 0] >= 5).all()  # real positions

    pri = tenv.priors_buffer(N, cap=CAP)
    rows = tenv.rows_buffer(N)
    planes = tenv.planes_buffer(dtype="float16", rows=N)
    for s in range(ROUNDS):
        C_PUCT, FPU = settings[s]
        sel = tree.select_batch(K, C_PUCT, FPU, 1.0)
        tenv.clone_boards(tenv, sel.parent, sel.child, count=N)
        tenv.step_boards(tio, sel.child, sel.action, rows=N, out=rows)
        tenv.encode_planes_rows(planes, sel.child, rows=N, perspective=True)
        tenv.policy_priors(tio, logits.ptr + s * row_bytes, pri, boards=sel.child, rows=N, dtype="bfloat16")
        d = tree.fetch(*B.BATCH_KEYS)
        tree.backup_batch(vals.ptr + 4 * N * s, rows, pri)

        wp, wc, wa = ref.select_batch(K, C_PUCT, FPU, 1.0, follow=(d["b_path"], d["b_depth"]))
        ref.same_selection_as(d, K)
        o, st, pr = sel.fetch(), rows.fetch("done", "reason"), pri.fetch()
        assert o["child"].shape == (N,)
        assert (o["parent"] == wp).all() and (o["child"] == wc).all() and (o["action"] == wa).all()
        pl = planes.raw()
        for r in range(N):
            g = r // K
            if wc[r] < 0:
                assert st["reason"][r] == 255 and pr["count"][r] == -1 and not pl[r].any(), (s, r)
                continue
            k = wp[r] - g * NODES
            assert o["action"][r] in ref.action[g, k, : ref.n_children[g, k]]
            assert st["reason"][r] not in (6, 255), (s, r, st["reason"][r])
            assert pl[r].any()
        ref.backup_batch(values[s], st["done"], st["reason"], pr["actions"], pr["priors"], pr["count"])
        ref.same_as(tree.fetch())
        d = tree.fetch("inflight", "collisions")
        assert not d["inflight"].any() and (d["collisions"] == ref.collisions).all()

    assert ref.seen["a"] >= 3 * G and ref.seen["c"] and ref.seen["d"], ref.seen
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

    # every created node's board: its path of actions replayed from the root, right-aligned so that
    # a node's own move is the last step (the idle action before it leaves a board as it is)
    paths = {}
    for g in range(G):
        for k in range(1, int(ref.n_nodes[g])):
            acts, x = [], k
            while x > 0:
                p = int(ref.parent[g, x])
                acts.append(int(ref.action[g, p, ref.parent_slot[g, x]]))
                x = p
            paths[g * NODES + k] = acts[::-1]
    deepest = max(len(a) for a in paths.values())
    assert deepest >= 2
    rep = BatchedChessEnv(G * NODES, device=0, seed=9, rules=rules)
    rio = rep.device_io(select=False)
    everything = np.arange(G * NODES)
    rep.clone_boards(game, everything // NODES, everything)
    for t in range(deepest):
        acts = np.full(G * NODES, CG.IDLE, dtype=np.uint16)
        for i, a in paths.items():
            if t >= deepest - len(a):
                acts[i] = a[t - (deepest - len(a))]
        rio.upload_actions(acts)
        rep.step_device(rio, actions=rio.ptr["pick"], autoreset=False)
    made = np.array(sorted(paths))
    CG.assert_same_state(CG.state(rep), made, CG.state(tenv), made, "replayed")
    roots = np.arange(G) * NODES
    sg, st_ = CG.state(game), CG.state(tenv)
    for key in ("board", "meta", "ep"):
        assert (sg[key][np.arange(G)] == st_[key][roots]).all(), key
    if rules == "reference":
        import oracle as O

        tb, tm = tenv.boards()
        checked = 0
        for i, a in paths.items():
            g, k = divmod(i, NODES)
            p = g * NODES + int(ref.parent[g, k])
            rc, nb, nm, _ = O.next_state(tb[p], tm[p], int(tm[p, 0]), a[-1])
            if rc != 0:  # (a move that leaves both kings checked changes nothing)
                continue
            assert (tb[i] == nb).all() and (tm[i, 1:7] == nm[1:7]).all() and tm[i, 0] == 1 - tm[p, 0], (g, k)
            checked += 1
        assert checked >= len(paths) - 2
    rep.synchronize()
    tenv.synchronize()
    tree.close()
    for b in (logits, vals, pri, rows, planes, gpri, tio, gio, rio):
        b.close()
    for e in (rep, tenv, game):
        e.close()


# --------------------------------------------------------------------------- 5. state and argument errors
def test_state_and_argument_errors(env):
    from gym_chess_amd import _lib

    L, G, NODES, CAP, K = env._L, 4, 8, 16, 3
    inp = R.synth_run(G, NODES, CAP, "wide", 12)
    a, p, c = (Dev(env, np.repeat(x, K, axis=0)) for x in inp["root"])  # G * K rows
    v = Dev(env, np.repeat(inp["root_value"], K))
    done = Dev(env, np.zeros(G * K, dtype=np.uint8))
    pc = inp["pri_cap"]
    tree = env.search_tree(G, NODES, cap=CAP)
    t, sel, root = tree._h, tree._sel.ptr, tree._root.ptr
    out = (ctypes.c_void_p * 6)()
    from gym_chess_amd.env import _DeviceArrays

    bsel = _DeviceArrays(env, {"parent": (np.int32, (G * K,)), "child": (np.int32, (G * K,)),
                               "action": (np.uint16, (G * K,))})
    sp, sc, sa = bsel.ptr["parent"], bsel.ptr["child"], bsel.ptr["action"]

    def refused(fn, *args):
        with pytest.raises(_lib.GymChessError) as ei:
            _lib.check(fn(*args))
        assert str(ei.value), args
        return str(ei.value)

    T.fill_tree(env, tree)
    _lib.check(L.gc_tree_reset(t, a.ptr, p.ptr, c.ptr, pc, v.ptr))
    back = (v.ptr, done.ptr, done.ptr, a.ptr, p.ptr, c.ptr, pc)

    # nothing reserved
    bytes0 = tree.device_bytes()
    before = tree.fetch()
    refused(L.gc_tree_select_batch, t, 1, 1.25, 0.0, 1.0, sp, sc, sa)
    refused(L.gc_tree_batch_pointers, t, out, 6)
    refused(L.gc_tree_backup_batch, t, *back)
    for bad in (0, -1, 65):
        refused(L.gc_tree_batch_reserve, t, bad)
    refused(L.gc_tree_batch_reserve, None, K)
    assert tree.device_bytes() == bytes0 and "inflight" not in tree.ptr
    T.fill_arrays(env, bsel)
    tree.reserve_batch(K)
    scratch = G * NODES * CAP + 8 * G * K * NODES + 3 * 4 * G * K + 4 * G
    assert bytes0 + scratch <= tree.device_bytes() <= bytes0 + scratch + 6 * 256  # counted, 256-byte aligned
    assert tree.max_leaves == K and all(k in tree.ptr for k in B.BATCH_KEYS)
    bytes1 = tree.device_bytes()
    tree.reserve_batch(K)  # the same size: nothing happens
    assert tree.device_bytes() == bytes1
    refused(L.gc_tree_batch_pointers, t, out, 0)
    refused(L.gc_tree_batch_pointers, t, None, 6)
    refused(L.gc_tree_batch_pointers, None, out, 6)
    _lib.check(L.gc_tree_batch_pointers(t, out, 6))
    assert [out[i] for i in range(6)] == [tree.ptr[k] for k in B.BATCH_KEYS]

    def snapshot():
        return dict(tree.fetch(), **tree.fetch(*B.BATCH_KEYS), **bsel.fetch())

    def untouched():
        now = snapshot()
        assert all(before[k].tobytes() == now[k].tobytes() for k in before)

    before = snapshot()
    assert not any(before[k].any() for k in B.BATCH_KEYS)  # zero-filled
    good = (t, K, 1.25, 0.0, 1.0, sp, sc, sa)
    for k, bad in ((0, None), (1, 0), (1, -2), (1, K + 1), (2, -0.5), (2, float("nan")), (2, float("inf")),
                   (3, float("nan")), (4, -1.0), (4, float("nan")), (4, float("inf")), (5, None), (6, None), (7, None)):
        args = list(good)
        args[k] = bad
        refused(L.gc_tree_select_batch, *args)
    refused(L.gc_tree_backup_batch, t, *back)  # nothing is pending
    untouched()

    # a single selection is pending: the batch calls are refused
    _lib.check(L.gc_tree_select(t, 1.25, 0.0, sel["parent"], sel["child"], sel["action"]))
    before = snapshot()
    assert "pending" in refused(L.gc_tree_select_batch, *good)
    assert "pending" in refused(L.gc_tree_backup_batch, t, *back)
    assert "pending" in refused(L.gc_tree_batch_reserve, t, K + 1)
    untouched()
    _lib.check(L.gc_tree_backup(t, *back))

    # a batch is pending: everything but its backup (and reset) is refused
    _lib.check(L.gc_tree_select_batch(t, K - 1, 0.0, float("inf"), 0.0, sp, sc, sa))  # fewer leaves than reserved; 0 / inf / 0 are values
    before = snapshot()
    assert before["inflight"].any()
    mv = Dev(env, np.full(G, NONE, dtype=np.uint16))
    adv = tree._adv.ptr
    assert "pending" in refused(L.gc_tree_select_batch, *good)
    assert "pending" in refused(L.gc_tree_select, t, 1.25, 0.0, sel["parent"], sel["child"], sel["action"])
    assert "pending" in refused(L.gc_tree_backup, t, *back)
    assert "pending" in refused(L.gc_tree_root_policy, t, ctypes.c_uint64(1), 0, 1, root["actions"], None, None, None, None)
    assert "pending" in refused(L.gc_tree_advance, t, mv.ptr, a.ptr, p.ptr, c.ptr, pc, v.ptr, adv["kept"], adv["remap"])
    assert "pending" in refused(L.gc_tree_batch_reserve, t, K + 1)
    for k in range(7):  # each argument of the backup in turn
        bad = list(back)
        bad[k] = 0 if k == 6 else None
        refused(L.gc_tree_backup_batch, t, *bad)
    refused(L.gc_tree_backup_batch, None, *back)
    untouched()
    _lib.check(L.gc_tree_backup_batch(t, *back))
    refused(L.gc_tree_backup_batch, t, *back)
    d = tree.fetch("inflight")
    assert not d["inflight"].any()

    # reset during a pending batch: the marks are cleared, the batch is gone, the counts stay
    _lib.check(L.gc_tree_select_batch(*good))
    d = tree.fetch("inflight", "collisions")
    assert d["inflight"].any()
    _lib.check(L.gc_tree_reset(t, a.ptr, p.ptr, c.ptr, pc, v.ptr))
    d2 = tree.fetch("inflight", "collisions", "n_nodes")
    assert not d2["inflight"].any() and (d2["collisions"] == d["collisions"]).all() and (d2["n_nodes"] == 1).all()
    refused(L.gc_tree_backup_batch, t, *back)
    _lib.check(L.gc_tree_select_batch(*good))
    _lib.check(L.gc_tree_backup_batch(t, *back))
    _lib.check(L.gc_tree_root_policy(t, ctypes.c_uint64(1), 0, 1, root["actions"], None, None, None, None))

    # another size: reallocated, zero-filled again, the count follows
    tree.reserve_batch(K + 2)
    assert tree.max_leaves == K + 2 and tree.device_bytes() > bytes1
    d = tree.fetch(*B.BATCH_KEYS)
    assert d["b_depth"].shape == (G, K + 2) and not any(d[k].any() for k in B.BATCH_KEYS)

    # the wrapper's own checks
    small, full = env.priors_buffer(G * K - 1, cap=CAP), env.priors_buffer(G * K, cap=CAP)
    rows = env.rows_buffer(G * K)
    few = env.rows_buffer(G * K - 1)
    s = tree.select_batch(K)
    assert s.fetch()["child"].shape == (G * K,)
    with pytest.raises(TypeError):
        tree.backup_batch(v.ptr, None, full)
    with pytest.raises(TypeError):
        tree.backup_batch(v.ptr, rows, a.ptr)
    with pytest.raises(ValueError):
        tree.backup_batch(v.ptr, rows, small)
    with pytest.raises(ValueError):
        tree.backup_batch(v.ptr, few, full)
    with pytest.raises(ValueError):
        tree.backup_batch(None, rows, full)
    with pytest.raises(_lib.GymChessError):
        tree.select_batch(K + 3)  # more than reserved (and a batch is pending)
    env.synchronize()
    tree.close()
    bsel.close()
    for b in (a, p, c, v, done, mv, small, full, rows, few):
        b.close()


# --------------------------------------------------------------------------- 6. advance after batches
class AdvBatch(B.RefTreeBatch, A.AdvTree):
    """the batched reference with test_tree_advance's advance"""


def test_advance_after_batches(env):
    """a tree grown by batches advances as one grown by single simulations does: kept / remap and
    every array of the kept subtree against test_tree_advance's reference, every game on its greedy
    pick; then the batched search goes on in the kept tree"""
    case = (5, 24, 64, 4, "wide", 2, 1.25, -1.0, 1.0, "synth")
    G, nodes, cap, K = case[:4]
    r = BatchRun(env, case, ref=AdvBatch(G, nodes, cap, K))
    r.reset()
    half = r.inp["rounds"] // 4
    for s in range(half):
        r.round(s)
    assert (r.ref.n_nodes < nodes).any() and (r.ref.n_nodes > 4).any()
    T.fill_arrays(env, r.tree._root)
    rp = r.tree.root_policy(greedy=True)
    picks = rp.fetch("pick")["pick"]
    assert (picks == r.ref.root_policy(0, 0, True)["pick"]).all()
    act, prs, cnt, val = A.advance_blocks(case[:3] + case[4:6], 1)[0]
    from gym_chess_amd import _lib

    pri = env.priors_buffer(G, cap=r.pc)
    for k, x in zip(("actions", "priors", "count"), (act, prs, cnt)):
        x = np.ascontiguousarray(x)
        _lib.check(env._L.gc_env_copy(env._h, pri.ptr[k], _lib.ptr(x), ctypes.c_uint64(x.nbytes), 1))
    dval = Dev(env, val)
    T.fill_arrays(env, r.tree._adv)
    o = r.tree.advance(rp.pick, pri, value=dval.ptr).fetch()
    kept, remap = r.ref.advance(picks, act, prs, cnt, value=val)
    assert (o["kept"] == kept).all() and (o["remap"] == remap).all()
    assert (kept > 1).any()
    r.ref.same_as(r.tree.fetch())
    d = r.tree.fetch("inflight", "collisions")
    assert not d["inflight"].any() and (d["collisions"] == r.ref.collisions).all()  # (advance clears no count)
    for s in range(half, 2 * half):
        r.round(s)
    env.synchronize()
    dval.close()
    pri.close()
    r.close()
