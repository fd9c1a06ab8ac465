"""GPU: the search tree's solver (gc_tree_solver_* / gc_tree_root_proof / SearchTree(solver=True))
against RefSolverTree and the acceptance rule of test_tree_solver.py: synthetic runs in which
proofs climb, a chain whose mate climbs a path of more than 64 entries, advance with proofs
carried to the new indices, a tree without the solver against the plain reference, two chess
positions with forced mates under both rule sets, and the state and argument errors.  Buffers come
from gc_device_alloc / gc_env_copy; no torch."""
import ctypes

import numpy as np
import pytest

import test_tree_advance as A
import test_tree_search as R
import test_tree_solver as S
from test_policy_priors_gpu import Dev
from test_tree_search_gpu import Run, fill, fill_arrays

pytestmark = pytest.mark.gpu

NONE = R.NONE
UNKNOWN, WIN, DRAW, LOSS = S.UNKNOWN, S.WIN, S.DRAW, S.LOSS


def all_arrays(tree):
    return tree.fetch(*(tree.ARRAYS + tree.SOLVER_ARRAYS))


def fill_solver_tree(env, tree):
    """the tree's 16 arrays and the solver's 5 become 0xAB: a row a kernel forgets to write shows"""
    for k in tree.ARRAYS + tree.SOLVER_ARRAYS:
        fill(env, tree.ptr[k], int(np.prod(tree._shape(k))) * np.dtype(tree._DTYPES.get(k, np.int32)).itemsize)


class SolverRun:
    """one synthetic run on a solver tree, simulation by simulation, with the reference following"""

    def __init__(self, env, case, inp):
        G, nodes, cap, _, _, self.c_puct, self.fpu = case[:7]
        self.env, self.L, self.G, self.inp = env, env._L, G, inp
        self.tree = env.search_tree(G, nodes, cap, solver=True)
        self.ref = S.RefSolverTree(G, nodes, cap)
        self.bufs = {k: Dev(env, inp[k]) for k in ("actions", "priors", "count", "value", "done", "reason")}
        self.root = [Dev(env, a) for a in inp["root"]] + [Dev(env, inp["root_value"])]
        self.pc = inp["pri_cap"]
        self.deepest = 0

    def reset(self):
        from gym_chess_amd import _lib

        fill_solver_tree(self.env, self.tree)
        a, p, c, v = (b.ptr for b in self.root)
        _lib.check(self.L.gc_tree_reset(self.tree._h, a, p, c, self.pc, v))
        self.ref.reset(*self.inp["root"], value=self.inp["root_value"])
        self.ref.same_as(all_arrays(self.tree))

    def simulate(self, s):
        from gym_chess_amd import _lib

        G, pc, b, i = self.G, self.pc, self.bufs, self.inp
        fill_arrays(self.env, self.tree._sel)
        sel = self.tree.select(self.c_puct, self.fpu)
        d = self.tree.fetch("path", "depth")
        self.deepest = max(self.deepest, int(d["depth"].max()))
        want = self.ref.select(self.c_puct, self.fpu, follow=(d["path"], d["depth"]))  # (refuses an excluded LOSS slot)
        o = sel.fetch()
        for got, w, name in zip((o["parent"], o["child"], o["action"]), want, ("parent", "child", "action")):
            assert (got == w).all(), (s, name, got, w)
        _lib.check(self.L.gc_tree_backup(self.tree._h, b["value"].ptr + 4 * G * s, b["done"].ptr + G * s,
                                         b["reason"].ptr + G * s, b["actions"].ptr + 2 * G * pc * s,
                                         b["priors"].ptr + 4 * G * pc * s, b["count"].ptr + 4 * G * s, pc))
        self.ref.backup(i["value"][s], i["done"][s], i["reason"][s], i["actions"][s], i["priors"][s], i["count"][s])
        self.ref.same_as(all_arrays(self.tree))

    def check_root(self, draws=range(4)):
        """root_proof and root_policy(proof=True) against the reference"""
        tree, ref = self.tree, self.ref
        fill_arrays(self.env, tree._proof)
        o = tree.root_proof().fetch()
        for got, w, name in zip((o["status"], o["plies"], o["move"]), ref.root_proof(), ("status", "plies", "move")):
            assert (got == w).all(), (name, got, w)
        for greedy in (True, False):
            for draw in draws:
                fill_arrays(self.env, tree._root)
                o = tree.root_policy(greedy=greedy, seed=77, draw=draw, proof=True).fetch()
                w = ref.root_policy(77, draw, greedy, proof=True)
                assert (o["actions"] == w["actions"]).all() and (o["visits"] == w["visits"]).all()
                assert (np.abs(o["pi"].astype(np.float64) - w["pi"]) <= 2.0 ** -22 * np.abs(w["pi"])).all()
                assert (np.abs(o["value"].astype(np.float64) - w["value"]) <= 2.0 ** -22 * np.abs(w["value"])).all()
                assert (o["pick"] == w["pick"]).all(), (greedy, draw, o["pick"], w["pick"])
                plain = tree.root_policy(greedy=greedy, seed=77, draw=draw).fetch()["pick"]
                assert (plain == ref.root_policy(77, draw, greedy)["pick"]).all()  # (without the flag: the visits alone)

    def close(self):
        self.env.synchronize()
        self.tree.close()
        for b in list(self.bufs.values()) + self.root:
            b.close()


@pytest.fixture(scope="module")
def env():
    from gym_chess_amd.env import BatchedChessEnv

    e = BatchedChessEnv(400, device=0, seed=3)
    yield e
    e.close()


# --------------------------------------------------------------------------- 1. synthetic runs
@pytest.mark.parametrize("case", S.SOLVER_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}{c[3]}")
def test_synthetic_solver_trees(env, case):
    """2 * nodes simulations: after every selection each level of the device's path meets the
    acceptance rule over the candidates (never an excluded LOSS slot) and the outputs are the
    reference's; after every backup all 16 tree arrays and the 5 solver arrays of every live node
    match bit for bit; the roots' proofs and proof-respecting picks at the middle and the end"""
    r = SolverRun(env, case, S.solver_run(*case[:5]))
    r.reset()
    r.check_root((0,))
    for s in range(r.inp["sims"]):
        r.simulate(s)
        if s == r.inp["sims"] // 2:
            r.check_root()
    r.check_root()
    assert len(r.ref.climbs) >= 4 and r.ref.ended_proven >= 1 and (r.ref.node_proven != UNKNOWN).any()
    assert r.ref.near_ties < 0.01 * r.ref.decisions, (r.ref.near_ties, r.ref.decisions)
    assert r.tree.device_bytes() >= case[0] * case[1] * case[2] * 21
    r.close()


def test_a_mate_climbs_a_path_of_more_than_64_entries(env):
    """S.CHAIN_CASE: 130 nodes per game (three chunks of 64), cap 1; the mate at depth 100 is
    carried up all 100 levels of game 0 in one backup, stops at game 1's first incomplete node, and
    game 2's draw proves nothing above its incomplete nodes"""
    r = SolverRun(env, S.CHAIN_CASE, S.chain_run(*S.CHAIN_CASE[:5], S.CHAIN_CASE[7]))
    r.reset()
    for s in range(r.inp["sims"]):
        r.simulate(s)
    mate_at = S.CHAIN_CASE[7]
    assert r.deepest == mate_at + 1 and max(r.ref.climbs) == mate_at + 1
    r.check_root()
    o = r.tree.root_proof().fetch()
    assert (o["status"][0], o["plies"][0]) == (WIN if mate_at % 2 == 0 else LOSS, mate_at + 1)
    r.close()


# --------------------------------------------------------------------------- 2. advance
@pytest.mark.parametrize("idx", S.ADVANCE_CASES)
def test_advance_carries_the_proofs(env, idx):
    """`nodes` simulations of a synthetic run, then an advance in which game g follows
    A.MOVE_RULES[g % 4] (the most visited root move, the first unexpanded one or 0xFFFF, 0xFFFF, an
    action no list holds): kept games carry their proofs to the new indices bit for bit, fresh
    games are reset, root_proof reports the kept roots' proofs (S.test_advance_keeps_proofs has what
    the cases cover); then 8 more simulations still match"""
    from gym_chess_amd import _lib

    case = S.SOLVER_CASES[idx]
    G, nodes, cap = case[:3]
    r = SolverRun(env, case, S.solver_run(*case[:5]))
    r.reset()
    for s in range(nodes):
        r.simulate(s)
    ref, tree = r.ref, r.tree
    mv = A.moves_for(ref, ref.root_policy(0, 0, True)["pick"], 0)
    assert mv[2] == NONE and mv[3] == A.ABSENT and mv[0] != NONE
    act, pri, cnt, val = A.advance_blocks(case, 1)[0]
    blk = [Dev(env, x) for x in (act, pri, cnt, val)]
    moves = Dev(env, mv)
    fill_arrays(env, tree._adv)
    adv = tree._adv.ptr
    _lib.check(tree._L.gc_tree_advance(tree._h, moves.ptr, blk[0].ptr, blk[1].ptr, blk[2].ptr, r.pc, blk[3].ptr,
                                       adv["kept"], adv["remap"]))
    kept, remap = ref.advance(mv, act, pri, cnt, value=val)
    o = tree._adv.fetch()
    assert (o["kept"] == kept).all() and (o["remap"] == remap).all()
    ref.same_as(all_arrays(tree))
    assert kept[0] >= 1 and kept[4] >= 1 and not kept[1:4].any()
    assert sum(int((ref.node_proven[g, : kept[g]] != UNKNOWN).sum()) for g in (0, 4)) >= 1
    for g in (1, 2, 3):
        assert ref.node_proven[g, 0] == UNKNOWN and not ref.edge_proven[g, 0].any()
    r.check_root()
    for s in range(nodes, nodes + 8):
        r.simulate(s)
    r.check_root((0,))
    for b in blk + [moves]:
        b.close()
    r.close()


# --------------------------------------------------------------------------- 3. the solver off
def test_without_the_solver_it_is_the_old_tree(env):
    """R.SYNTH_CASES[0] on a tree that never enabled the solver: plain RefTree bit for bit, and
    the solver's calls and flag bit 1 are refused"""
    from gym_chess_amd import _lib

    G, nodes, cap, rule, seed, c_puct, fpu = R.SYNTH_CASES[0]
    r = Run(env, G, nodes, cap, R.synth_run(G, nodes, cap, rule, seed), c_puct, fpu)
    r.reset()
    for s in range(r.inp["sims"]):
        r.simulate(s)
    t, L = r.tree, r.tree._L
    assert not t.solver and "edge_proven" not in t.ptr
    out = (ctypes.c_void_p * 5)()
    for rc in (L.gc_tree_root_proof(t._h, None, None, None), L.gc_tree_solver_pointers(t._h, out, 5),
               L.gc_tree_root_policy(t._h, ctypes.c_uint64(1), 0, 2, None, None, None, None, None),
               L.gc_tree_root_policy(t._h, ctypes.c_uint64(1), 0, 3, None, None, None, None, None)):
        with pytest.raises(_lib.GymChessError):
            _lib.check(rc)
    with pytest.raises(ValueError):
        t.root_proof()
    r.ref.same_as(t.fetch())
    r.close()


# --------------------------------------------------------------------------- 4. chess
MATE_IN_ONE = "7k/8/6K1/8/8/8/8/R7 w - - 0 1"   # a1-a8 (3584) mates
MATE_IN_TWO = "4K2k/8/8/6Q1/8/8/8/8 w - - 0 1"  # e8-f8 (261), h8-h7 (463, the only reply), g5-g7 (1934) mate
LINE = (3584, 261, 463, 1934)


@pytest.mark.parametrize("rules", ["reference", "fide"])
def test_forced_mates_in_chess(rules):
    """2 games set by FEN, a tree env of 2 x 40 boards, cap 64, the documented six-launch loop with
    value 0 and logits 0 but +8 at the line's action ids in place of a network.  Up to 32
    simulations, each checked against the reference; then game 0's root is WIN in 1 by 3584, game
    1's WIN in 3 by 261 with the reply node LOSS in 2 and complete; root_policy(proof=True) picks
    those moves under sampling with any draw; once a root is WIN every later descent of that game
    ends at the proven child with an empty env row and adds one visit to that edge."""
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    G, NODES, CAP, SIMS = 2, 40, 64, 32
    game = BatchedChessEnv(G, device=0, seed=5, rules=rules)
    game.set_fens([MATE_IN_ONE, MATE_IN_TWO])
    tenv = BatchedChessEnv(G * NODES, device=0, seed=6, rules=rules)
    tio = tenv.device_io(pick=False)
    raw = np.zeros((G, 4100), dtype=np.float32)
    raw[:, list(LINE)] = 8.0
    zeros = np.zeros(G, dtype=np.float32)
    logits, vals = Dev(tenv, raw), Dev(tenv, zeros)

    # the roots' block, made on the host from the game env's legal moves (set_fens leaves no
    # device mask behind): action-id order, softmax of the same logits
    legal = game.legal_mask()[:, :4100]
    h = dict(actions=np.full((G, CAP), NONE, dtype=np.uint16), priors=np.zeros((G, CAP), dtype=np.float32),
             count=legal.sum(axis=1).astype(np.int32))
    for g in range(G):
        ids = np.flatnonzero(legal[g])
        w = np.exp(raw[g, ids].astype(np.float64))
        h["actions"][g, : ids.size], h["priors"][g, : ids.size] = ids, (w / w.sum()).astype(np.float32)
    groot = [Dev(tenv, h[k]) for k in ("actions", "priors", "count")]
    tree = tenv.search_tree(G, NODES, cap=CAP, solver=True)
    ref = S.RefSolverTree(G, NODES, CAP)
    fill_solver_tree(tenv, tree)
    _lib.check(tree._L.gc_tree_reset(tree._h, groot[0].ptr, groot[1].ptr, groot[2].ptr, CAP, vals.ptr))
    ref.reset(h["actions"], h["priors"], h["count"], value=zeros)
    tenv.clone_boards(game, np.arange(G), np.arange(G) * NODES)
    ref.same_as(all_arrays(tree))
    assert ref.n_children[:, 0].tolist() == [20, 28] and ref.complete[:, 0].tolist() == [1, 1]

    pri = tenv.priors_buffer(G, cap=CAP)
    rows = tenv.rows_buffer(G)
    won_at = [None, None]  # the simulation after which the root was WIN
    for s in range(SIMS):
        was = ref.node_proven[:, 0].copy()
        visits = ref.edge_visits[:, 0].copy()
        fill_arrays(tenv, tree._sel)
        sel = tree.select(1.25, 0.0)
        tenv.clone_boards(tenv, sel.parent, sel.child, count=G)
        tenv.step_boards(tio, sel.child, sel.action, rows=G, out=rows)
        tenv.policy_priors(tio, logits.ptr, pri, boards=sel.child, rows=G)
        tree.backup(vals.ptr, rows, pri)

        d = tree.fetch("path", "depth")
        wp, wc, wa = ref.select(1.25, 0.0, follow=(d["path"], d["depth"]))
        o, st, pr = sel.fetch(), rows.fetch("done", "reason"), pri.fetch()
        assert (o["parent"] == wp).all() and (o["child"] == wc).all() and (o["action"] == wa).all()
        for g in range(G):
            if wc[g] < 0:
                assert st["reason"][g] == 255 and pr["count"][g] == -1
            if was[g] == WIN:  # the proof's edge, its child, an empty row, one more visit
                j = ref.proof_slot(g, 0, WIN)
                assert d["depth"][g] == 1 and tuple(d["path"][g, 0]) == (0, j) and wc[g] < 0
                assert ref.leaf[g] == ref.child[g, 0, j] and not ref.leaf_new[g]
        ref.backup(zeros, st["done"], st["reason"], pr["actions"], pr["priors"], pr["count"])
        ref.same_as(all_arrays(tree))
        for g in range(G):
            if was[g] == WIN:
                j = ref.proof_slot(g, 0, WIN)
                assert ref.edge_visits[g, 0, j] == visits[g, j] + 1 and ref.edge_visits[g, 0].sum() == visits[g].sum() + 1
            elif ref.node_proven[g, 0] == WIN:
                won_at[g] = s
    assert won_at[0] == 0 and won_at[1] is not None and won_at[1] < SIMS - 4, won_at

    fill_arrays(tenv, tree._proof)
    o = tree.root_proof().fetch()
    assert (o["status"].tolist(), o["plies"].tolist(), o["move"].tolist()) == ([WIN, WIN], [1, 3], [3584, 261])
    a = int(ref.child[1, 0, np.flatnonzero(ref.action[1, 0] == 261)[0]])  # the reply node
    dev = all_arrays(tree)
    assert (dev["node_proven"][1, a], dev["node_plies"][1, a], dev["complete"][1, a]) == (LOSS, 2, 1)
    assert dev["n_children"][1, a] == 1 and dev["action"][1, a, 0] == 463
    for draw in range(8):
        assert tree.root_policy(greedy=False, seed=11, draw=draw, proof=True).fetch()["pick"].tolist() == [3584, 261]
    assert tree.root_policy(greedy=True, proof=True).fetch()["pick"].tolist() == [3584, 261]
    assert ref.near_ties < 0.01 * ref.decisions
    tenv.synchronize()
    tree.close()
    for b in [logits, vals, pri, rows, tio] + groot:
        b.close()
    tenv.close()
    game.close()


# --------------------------------------------------------------------------- 5. state and argument errors
def test_solver_state_and_argument_errors(env):
    from gym_chess_amd import _lib

    L, G, NODES, CAP = env._L, 4, 8, 16
    inp = R.synth_run(G, NODES, CAP, "wide", 12)
    a, p, c = (Dev(env, x) for x in inp["root"])
    v = Dev(env, inp["root_value"])
    done = Dev(env, np.zeros(G, dtype=np.uint8))
    pc = inp["pri_cap"]
    back = (v.ptr, done.ptr, done.ptr, a.ptr, p.ptr, c.ptr, pc)
    out = (ctypes.c_void_p * 5)()

    def refused(fn, *args):
        with pytest.raises(_lib.GymChessError) as ei:
            _lib.check(fn(*args))
        assert str(ei.value), args
        return str(ei.value)

    # NULL handles
    refused(L.gc_tree_solver_enable, None)
    refused(L.gc_tree_solver_pointers, None, out, 5)
    refused(L.gc_tree_root_proof, None, None, None, None)

    # enable: not with a selection pending, not with a batch scratch reserved
    tree = env.search_tree(G, NODES, cap=CAP)
    t, sel = tree._h, tree._sel.ptr
    refused(L.gc_tree_solver_pointers, t, out, 5)  # before enable
    _lib.check(L.gc_tree_reset(t, a.ptr, p.ptr, c.ptr, pc, v.ptr))
    _lib.check(L.gc_tree_select(t, 1.25, 0.0, sel["parent"], sel["child"], sel["action"]))
    refused(L.gc_tree_solver_enable, t)
    _lib.check(L.gc_tree_backup(t, *back))
    before = tree.device_bytes()
    tree.enable_solver()  # on a tree that already has nodes: they are unknown and incomplete
    assert tree.device_bytes() >= before + G * NODES * (3 * CAP + 4)
    now = tree.device_bytes()
    tree.enable_solver()  # a second call does nothing
    assert tree.device_bytes() == now
    s = tree.fetch(*tree.SOLVER_ARRAYS)
    assert not any(x.any() for x in s.values())
    refused(L.gc_tree_solver_pointers, t, out, 0)
    refused(L.gc_tree_solver_pointers, t, None, 5)
    _lib.check(L.gc_tree_solver_pointers(t, out, 2))
    assert out[0] == tree.ptr["edge_proven"] and out[1] == tree.ptr["edge_plies"] and not out[2]
    _lib.check(L.gc_tree_root_proof(t, None, None, None))  # every output is optional
    assert not tree.root_proof().fetch()["status"].any()
    # with a selection pending
    _lib.check(L.gc_tree_select(t, 1.25, 0.0, sel["parent"], sel["child"], sel["action"]))
    refused(L.gc_tree_root_proof, t, None, None, None)
    refused(L.gc_tree_root_policy, t, ctypes.c_uint64(1), 0, 2, None, None, None, None, None)
    _lib.check(L.gc_tree_backup(t, *back))
    refused(L.gc_tree_root_policy, t, ctypes.c_uint64(1), 0, 4, None, None, None, None, None)
    _lib.check(L.gc_tree_root_policy(t, ctypes.c_uint64(1), 0, 3, None, None, None, None, None))
    # the batch calls on a solver tree
    for msg in (refused(L.gc_tree_batch_reserve, t, 4),
                refused(L.gc_tree_select_batch, t, 2, 1.25, 0.0, 1.0, sel["parent"], sel["child"], sel["action"]),
                refused(L.gc_tree_backup_batch, t, *back)):
        assert "solver" in msg, msg
    with pytest.raises(_lib.GymChessError):
        tree.select_batch(2)
    env.synchronize()
    tree.close()

    tree = env.search_tree(G, NODES, cap=CAP)
    tree.reserve_batch(2)
    assert "batch" in refused(L.gc_tree_solver_enable, tree._h)
    with pytest.raises(_lib.GymChessError):
        tree.enable_solver()
    assert not tree.solver
    env.synchronize()
    tree.close()
    for b in (a, p, c, v, done):
        b.close()
