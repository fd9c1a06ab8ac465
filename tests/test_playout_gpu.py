"""GPU: gc_playout_run / BatchedChessEnv.playouts against the host build of the same playout body
(tests/core_host/playout_host.cpp, itself pinned to the oracle by tests/test_playout.py), bit for
bit; skipped rows, the env left untouched, scratch reuse across calls, the refusals, and the
network-free search loop of INTEGRATION.md end to end."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
import playout_cases as PC  # noqa: E402
import playouthost as PH  # noqa: E402
from test_policy_priors_gpu import Dev  # noqa: E402

pytestmark = pytest.mark.gpu

N, P, PLIES, SEED = 96, 8, 48, 31


@pytest.fixture(scope="module")
def cases():
    boards, metas = PC.positions()
    return boards[:N], metas[:N]


@pytest.fixture(scope="module")
def env(cases):
    from gym_chess_amd.env import BatchedChessEnv

    e = BatchedChessEnv(N, device=0, seed=9)
    e.set_states(*cases)
    yield e
    e.close()


def same(res, want, rows):
    """the device's value / tally rows equal the host build's, bit for bit"""
    got = res.fetch()
    value, tally = want
    assert (got["tally"][:rows] == tally).all(), np.flatnonzero((got["tally"][:rows] != tally).any(axis=1))
    assert got["value"][:rows].tobytes() == value.tobytes()


# --------------------------------------------------------------------------- host parity
def test_host_parity(env, cases):
    po = env.playouts(N, playouts=P, max_plies=PLIES)
    assert po.device_bytes() == (N * P + 63) // 64 * 64 * (256 * 64 + 4)
    res = po.run(seed=SEED, cut_weight=0.37)  # boards 0..N-1
    want = PH.run(*cases, np.arange(N), SEED, P, PLIES, cut_weight=0.37)
    same(res, want, N)
    t = want[1]
    assert (t[:, :4].sum(axis=1) == P).all() and t[:, 0].sum() and t[:, 1].sum() and t[:, 2].sum() and t[:, 3].sum()
    idx = np.random.RandomState(4).randint(0, N, size=70)  # shuffled, with duplicates
    assert len(set(idx.tolist())) < 70
    same(po.run(idx, seed=SEED, draw=1000), PH.run(*cases, idx, SEED, P, PLIES, draw=1000), 70)
    d = Dev(env, idx.astype(np.int32))  # the same list as a device pointer
    same(po.run(d.ptr, rows=70, seed=SEED, draw=1000), PH.run(*cases, idx, SEED, P, PLIES, draw=1000), 70)
    env.synchronize()
    d.close()
    po.close()


@pytest.mark.parametrize("playouts,rows", [(1, 1), (1, 70), (4, 1), (4, 21), (64, 1), (64, 3)])
def test_other_widths(env, cases, playouts, rows):
    """rows that do not fill a wave's 64 / P rows; one value and one tally array only"""
    po = env.playouts(rows, playouts=playouts, max_plies=PLIES)
    idx = (np.arange(rows) * 7 + 4) % N  # (4 = the one-move mate)
    same(po.run(idx, seed=SEED + playouts), PH.run(*cases, idx, SEED + playouts, playouts, PLIES), rows)
    from gym_chess_amd import _lib

    v = Dev(env, np.full(rows, 7.0, dtype=np.float32))
    _lib.check(env._L.gc_playout_run(po._h, None, rows, PLIES, ctypes.c_uint64(3), 0, 1.0, v.ptr, None))
    got = np.zeros(rows, dtype=np.float32)
    _lib.check(env._L.gc_env_copy(env._h, _lib.ptr(got), v.ptr, ctypes.c_uint64(got.nbytes), 2))
    assert got.tobytes() == PH.run(*cases, np.arange(rows), 3, playouts, PLIES)[0].tobytes()
    _lib.check(env._L.gc_playout_run(po._h, None, rows, PLIES, ctypes.c_uint64(3), 0, 1.0, None, None))
    _lib.check(env._L.gc_playout_run(po._h, None, 0, PLIES, ctypes.c_uint64(3), 0, 1.0, None, None))
    env.synchronize()
    v.close()
    po.close()


def test_the_one_move_that_mates(env):
    po = env.playouts(1, playouts=P, max_plies=PLIES)
    got = po.run([4], seed=1, cut_weight=0.25).fetch()
    assert list(got["tally"][0]) == [P, 0, 0, 0, 0, P] and got["value"][0] == 1.0
    po.close()


# --------------------------------------------------------------------------- skipped rows
def test_skipped_rows(cases):
    from gym_chess_amd.env import BatchedChessEnv

    e = BatchedChessEnv(N, device=0, seed=9)
    e.set_states(*cases)
    e.step_boards(None, [4], [PC.MATE_IN_ONE_ACTION])  # board 4 is mated: done
    assert e.outputs()["done"][4] == 1
    done = np.zeros(N, dtype=bool)
    done[4] = True
    idx = np.array([3, -1, 5, N, 4, 6, 2 ** 31 - 1, -2 ** 31, 7, 4, 0])
    po = e.playouts(len(idx), playouts=P, max_plies=PLIES)
    junk = np.full((len(idx), 6), -77, dtype=np.int32)
    from gym_chess_amd import _lib

    _lib.check(e._L.gc_env_copy(e._h, po.ptr["tally"], _lib.ptr(junk), ctypes.c_uint64(junk.nbytes), 1))
    _lib.check(e._L.gc_env_copy(e._h, po.ptr["value"], _lib.ptr(junk), ctypes.c_uint64(4 * len(idx)), 1))
    d = Dev(e, idx.astype(np.int64).astype(np.int32))  # (a device list: the binding clips nothing)
    res = po.run(d.ptr, rows=len(idx), seed=SEED)
    got = res.fetch()
    for j in (1, 3, 4, 6, 7, 9):
        assert not got["tally"][j].any() and got["value"][j].tobytes() == np.float32(0).tobytes(), j
    want = PH.run(*cases, np.where((idx >= 0) & (idx < N), idx, -1), SEED, P, PLIES, done=done)
    same(res, want, len(idx))
    assert want[1][[0, 2, 5, 8, 10]].any(axis=1).all()  # the rows around them played
    e.synchronize()
    d.close()
    po.close()
    e.close()


# --------------------------------------------------------------------------- the env is untouched
def test_env_untouched(cases):
    from gym_chess_amd.env import BatchedChessEnv

    envs = []
    for _ in range(2):
        e = BatchedChessEnv(N, device=0, seed=9)
        e.set_states(*cases)
        e.select_random()
        e.step_random(3)  # windows, counters and outputs that are not the fresh env's
        envs.append(e)
    e, twin = envs
    before = (e.checkpoint(), e.window_sum(), e.outputs())
    po = e.playouts(N, playouts=P, max_plies=PLIES)
    po.run(seed=SEED)
    po.run(np.arange(N)[::-1], seed=SEED, draw=77)
    e.synchronize()
    after = (e.checkpoint(), e.window_sum(), e.outputs())
    assert before[0] == after[0] and before[1] == after[1]
    for k in before[2]:
        assert (before[2][k] == after[2][k]).all(), k
    e.step_random(4)
    twin.step_random(4)
    for a, b in zip(e.boards(), twin.boards()):
        assert (a == b).all()
    assert e.checkpoint() == twin.checkpoint()
    po.close()
    e.close()
    twin.close()


# --------------------------------------------------------------------------- scratch reuse
def test_scratch_reuse(env, cases):
    po = env.playouts(N, playouts=P, max_plies=PLIES)
    same(po.run(seed=SEED, draw=0), PH.run(*cases, np.arange(N), SEED, P, PLIES, draw=0), N)
    same(po.run(seed=SEED, draw=48), PH.run(*cases, np.arange(N), SEED, P, PLIES, draw=48), N)
    other = (np.arange(N) * 5 + 2) % N  # other boards on the same lanes
    want = PH.run(*cases, other, SEED, P, PLIES, draw=96)
    same(po.run(other, seed=SEED, draw=96), want, N)
    again = po.playout_buffer()
    same(po.run(other, seed=SEED, draw=96, out=again), want, N)  # the same call twice
    a, b = po.fetch(), again.fetch()
    assert a["value"].tobytes() == b["value"].tobytes() and (a["tally"] == b["tally"]).all()
    again.close()
    po.close()


def test_longest_window(env, cases):
    """max_plies = 128 on the two bare kings: no capture or pawn move ever clears the window, so
    the playouts fill it as far as a playout can"""
    assert (cases[0][2] == PC.TWO_KINGS).all()
    po = env.playouts(3, playouts=P, max_plies=128)
    idx = [2, 2, 2]
    for draw in (0, 128):
        want = PH.run(*cases, idx, SEED, P, 128, draw=draw)
        same(po.run(idx, plies=128, seed=SEED, draw=draw), want, 3)
    assert want[1][:, 5].max() > 8 * 20  # long playouts
    po.close()


# --------------------------------------------------------------------------- refusals
def test_refusals(env):
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    L = env._L

    def refused(fn, *args):
        assert fn(*args) == -1
        assert L.gc_last_error()

    h = ctypes.c_void_p()
    for bad in (0, 3, 12, 65, 128, -8):
        refused(L.gc_playout_create, env._h, 4, bad, 16, ctypes.byref(h))
    for bad in (0, 129, -1):
        refused(L.gc_playout_create, env._h, 4, 8, bad, ctypes.byref(h))
    refused(L.gc_playout_create, env._h, 0, 8, 16, ctypes.byref(h))
    refused(L.gc_playout_create, None, 4, 8, 16, ctypes.byref(h))
    refused(L.gc_playout_create, env._h, 4, 8, 16, None)
    with pytest.raises(RuntimeError):
        env.playouts(4, playouts=6)

    po = env.playouts(4, playouts=8, max_plies=16)
    out = po.fetch()
    run = L.gc_playout_run
    seed = ctypes.c_uint64(1)
    v, t = po.ptr["value"], po.ptr["tally"]
    refused(run, None, None, 4, 16, seed, 0, 1.0, v, t)
    refused(run, po._h, None, 5, 16, seed, 0, 1.0, v, t)
    refused(run, po._h, None, -1, 16, seed, 0, 1.0, v, t)
    refused(run, po._h, None, 4, 17, seed, 0, 1.0, v, t)
    refused(run, po._h, None, 4, 0, seed, 0, 1.0, v, t)
    for cw in (float("nan"), -0.001, 1.001, float("inf")):
        refused(run, po._h, None, 4, 16, seed, 0, cw, v, t)
    with pytest.raises(ValueError):
        po.run(np.arange(5))
    after = po.fetch()  # nothing was launched
    assert (out["tally"] == after["tally"]).all() and out["value"].tobytes() == after["value"].tobytes()
    assert L.gc_playout_destroy(None) == -1
    assert L.gc_playout_device_bytes(None) == 0
    po.close()

    fide = BatchedChessEnv(4, device=0, rules="fide")
    refused(L.gc_playout_create, fide._h, 4, 8, 16, ctypes.byref(h))
    fide.close()
    opp = BatchedChessEnv(4, device=0, opponent="random")
    refused(L.gc_playout_create, opp._h, 4, 8, 16, ctypes.byref(h))
    opp.close()
    late = BatchedChessEnv(4, device=0)  # the env changes after the handle exists
    po = late.playouts(4, playouts=8, max_plies=16)
    _lib.check(L.gc_env_set_rules(late._h, 1))
    refused(run, po._h, None, 4, 16, seed, 0, 1.0, po.ptr["value"], po.ptr["tally"])
    po.close()
    late.close()


# --------------------------------------------------------------------------- end to end
# WHITE: Kg1, Rd1; BLACK: Kg8, Qd5.  Rxd5 (action 59 * 64 + 27) takes the undefended queen; WHITE has
# no other capture.  Observed on an MI355X with the sizes and seeds below: Rxd5 gets 37 of the 48
# root visits, each of the other 11 moves exactly 1 -- the margin is not marginal.
QUEEN_HANGS = PC.board_of({62: 1, 59: 3, 6: -1, 27: -2})
TAKE_QUEEN = 59 * 64 + 27


def network_free_search(boards, metas, seed):
    """INTEGRATION.md's network-free loop: G games, NODES slots each, SIMS simulations whose leaf
    values are random playouts and whose priors are uniform -> (root policy, tree visits)"""
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    G, NODES, CAP, SIMS, PO, PLIES_ = len(boards), 64, 64, 48, 16, 6
    game = BatchedChessEnv(G, device=0, seed=5)
    game.set_states(boards, metas)
    gio = game.device_io(pick=False)
    raw = np.zeros((G, 65), dtype=np.uint64)  # the roots' legal masks into the game env's io (word-major)
    cnt = np.zeros(G, dtype=np.int32)
    _lib.check(game._L.gc_env_legal_mask(game._h, _lib.ptr(raw), _lib.ptr(cnt)))
    wm = np.zeros((65, gio.mask_stride), dtype=np.uint64)
    wm[:, :G] = raw.T
    _lib.check(game._L.gc_env_copy(game._h, gio.ptr["mask"], _lib.ptr(wm), ctypes.c_uint64(wm.nbytes), 1))

    tenv = BatchedChessEnv(G * NODES, device=0, seed=6)
    tio = tenv.device_io(pick=False)
    zeros = Dev(tenv, np.zeros((G, 4100), dtype=np.float32))  # zero logits: uniform priors
    gpri = game.priors_buffer(G, cap=CAP)
    game.policy_priors(gio, zeros.ptr, gpri)
    game.synchronize()
    tree = tenv.search_tree(G, NODES, cap=CAP)
    tree.reset(gpri)
    tenv.clone_boards(game, np.arange(G), np.arange(G) * NODES)
    po = tenv.playouts(G, playouts=PO, max_plies=PLIES_)
    pri, rows = tenv.priors_buffer(G, cap=CAP), tenv.rows_buffer(G)
    for s in range(SIMS):
        sel = tree.select(c_puct=1.25, fpu=0.0)
        tenv.clone_boards(tenv, sel.parent, sel.child, count=G)
        tenv.step_boards(tio, sel.child, sel.action, rows=G, out=rows)
        leaf = po.run(sel.child, rows=G, seed=seed, draw=PLIES_ * s)  # -1 and finished rows: value 0
        tenv.policy_priors(tio, zeros.ptr, pri, boards=sel.child, rows=G)
        tree.backup(leaf.value, rows, pri)
    root = tree.root_policy(greedy=True).fetch()
    tenv.synchronize()
    tree.close()
    po.close()
    for b in (zeros, pri, rows, gpri, tio, gio):
        b.close()
    tenv.close()
    game.close()
    return root, SIMS


def test_network_free_search_end_to_end(cases):
    boards = np.stack([QUEEN_HANGS] + [cases[0][k] for k in (0, 1, 2, 3, 10, 20, 30)])
    metas = np.stack([PC.settle(QUEEN_HANGS, [1, 0, 0, 0, 0, 0, 0, 0])] + [cases[1][k] for k in (0, 1, 2, 3, 10, 20, 30)])
    root, sims = network_free_search(boards, metas, seed=17)
    again, _ = network_free_search(boards, metas, seed=17)
    for k in root:
        assert root[k].tobytes() == again[k].tobytes(), k
    print("root visits", root["visits"].sum(axis=1), "game 0:",
          sorted(zip(root["visits"][0].tolist(), root["actions"][0].tolist()), reverse=True)[:4])
    assert (root["visits"].sum(axis=1) == sims).all()
    assert root["pick"][0] == TAKE_QUEEN
