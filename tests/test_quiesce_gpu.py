"""GPU: gc_env_minimax_q / BatchedChessEnv.minimax(quiesce=...) against the host build of the same
search (tests/core_host/quiesce_host.cpp, itself pinned to the oracle by tests/test_quiesce.py), bit
for bit, nodes included: every list shape, skipped rows, both tie rules, quiesce=0 against
gc_env_minimax, the env left untouched, the refusals, dirty memory in a child process and the
defended pawn through the search loop."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import playout_cases as PC  # noqa: E402
import quiescehost as QH  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("pick", "score", "value", "count")
# WHITE Kg1 Qd1, BLACK Kg8 behind pawns f7 g7 h7, pawns d5 and e6 (tests/test_quiesce.py's defended
# pawn): Qxd5 wins a pawn at the horizon and loses the queen to exd5 one ply further
DEFENDED = {62: 1, 59: 2, 6: -1, 13: -6, 14: -6, 15: -6, 27: -6, 20: -6}
QXD5 = 59 * 64 + 27


def positions():
    """the 206 shared positions, the defended pawn as board 206 and a board that gets done (207)"""
    b, m = PC.positions()
    pawn = PC.board_of(DEFENDED)
    boards = np.concatenate([b, pawn[None], PC.MATE_IN_ONE[None]])
    metas = np.concatenate([m, PC.settle(pawn, [1, 0, 0, 0, 0, 0, 0, 0])[None],
                            PC.settle(PC.MATE_IN_ONE, [1, 0, 0, 0, 0, 0, 0, 0])[None]])
    return boards, metas


def index_list(n, rows=None):
    """boards 0..rows-1 with duplicates, -1, an out-of-range index and the done board among them"""
    lst = list(range(n - 1 if rows is None else rows))
    return np.array(lst[:5] + [-1, 3, n, n - 1, 3] + lst[5:] + [n - 1, 0], dtype=np.int64)


@pytest.fixture(scope="module")
def cases():
    boards, metas = positions()
    n = len(boards)
    done = np.zeros(n, dtype=bool)
    done[n - 1] = True
    one = QH.run(boards, metas, np.arange(n), 1)
    import minimaxhost as MH

    wide = [i for i in range(n) if one["count"][i] > 64]
    big = [i for i in range(n) if MH.big(boards[i], metas[i])]
    stuck = [i for i in range(n) if one["count"][i] == 0]
    assert wide and big and stuck
    return boards, metas, done, index_list(n)


def make_env(cases, seed=9):
    from gym_chess_amd.env import BatchedChessEnv

    e = BatchedChessEnv(len(cases[0]), device=0, seed=seed)
    e.set_states(cases[0], cases[1])
    n = e.num_boards
    e.step_boards(None, [n - 1], [PC.MATE_IN_ONE_ACTION])  # the last board is mated: done
    assert e.outputs()["done"][n - 1] == 1
    return e


@pytest.fixture(scope="module")
def env(cases):
    e = make_env(cases)
    yield e
    e.close()


_WANT = {}


def want(cases, idx, depth, quiesce, cap, seed=None, draw=0):
    """the host build's rows, computed once per shape and never changed"""
    key = (idx.tobytes(), depth, quiesce, cap, seed, draw)
    if key not in _WANT:
        boards, metas, done = cases[:3]
        clean = np.where((idx >= 0) & (idx < len(boards)), idx, -1)
        _WANT[key] = QH.run(boards, metas, clean, depth, quiesce=quiesce, seed=seed, draw=draw, cap=cap, done=done)
    return _WANT[key]


def with_random_ties(w, idx, seed, draw):
    """the rows `w` (tiebreak first, full lists) under the random tie rule, from the definition: the
    search below the root is the same, so only the pick moves -- to T[i*], i* the largest i with
    policy_index(seed, board, draw + i, i + 1) == 0 (tests/test_quiesce.py pins the host build's
    own random pick to this).  Saves a second host search where one takes seconds."""
    out = {k: v.copy() for k, v in w.items()}
    for j in np.flatnonzero(w["count"] > 0):
        c = int(w["count"][j])
        assert c <= w["actions"].shape[1]
        ties = w["actions"][j, :c][w["scores"][j, :c] == w["score"][j]]
        keep = [i for i in range(len(ties)) if QH.policy_index(seed, int(idx[j]), (draw + i) & 0xFFFFFFFF, i + 1) == 0]
        out["pick"][j] = ties[max(keep)]
    return out


def same(buf, w, rows, nodes=True, cap=None):
    """the device's first `rows` rows equal the host build's rows `w`, bit for bit"""
    got = buf.fetch()
    for k in KEYS + (("nodes",) if nodes else ()):
        assert got[k][:rows].tobytes() == w[k][:rows].tobytes(), (k, np.flatnonzero(got[k][:rows] != w[k][:rows]))
    if buf.cap:
        c = buf.cap if cap is None else cap
        for k in ("actions", "scores"):
            bad = (got[k][:rows] != w[k][:rows, :c]).any(axis=1)
            assert not bad.any(), (k, np.flatnonzero(bad))


def junk(env, buf):
    """prefill every array of the buffer with a pattern no result holds"""
    from gym_chess_amd import _lib

    for k, (dt, shape) in buf._spec.items():
        a = np.full(int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize, 0x5B, dtype=np.uint8)
        if a.nbytes:
            _lib.check(env._L.gc_env_copy(env._h, buf.ptr[k], _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))


# --------------------------------------------------------------------------- 1. host parity
@pytest.mark.parametrize("depth,quiesce", [(1, 1), (1, 4), (2, 1), (2, 4), (3, 2)])
def test_host_parity(env, cases, depth, quiesce):
    idx = cases[3]
    n = len(idx)
    deep = depth == 3  # the host build takes seconds per search of the 206 boards: one search, no cap-0 twin
    listed = want(cases, idx, depth, quiesce, 256)
    plain = listed if deep else want(cases, idx, depth, quiesce, 0)
    assert (listed["count"] > 64).any() and (listed["count"] == -1).sum() >= 2 and (listed["count"] == 0).any()
    for k in KEYS:  # the list changes nothing but the nodes
        assert listed[k].tobytes() == plain[k].tobytes()
    assert (plain["nodes"] <= listed["nodes"]).all()
    big, cut, bare = env.minimax_buffer(n, cap=256), env.minimax_buffer(n, cap=8), env.minimax_buffer(n)
    for b in (big, cut, bare):
        junk(env, b)
    same(env.minimax(idx, depth=depth, quiesce=quiesce, out=big, nodes=True), listed, n)
    same(env.minimax(idx, depth=depth, quiesce=quiesce, out=cut, nodes=True), listed, n, cap=8)
    same(env.minimax(idx, depth=depth, quiesce=quiesce, out=bare, nodes=True), plain, n, nodes=not deep)
    junk(env, bare)
    same(env.minimax(idx, depth=depth, quiesce=quiesce, out=bare), plain, n, nodes=False)  # nodes off: not written
    assert (bare.fetch("nodes")["nodes"] == 0x5B5B5B5B).all()
    # the random tie rule, with and without the list
    wr = with_random_ties(listed, idx, 77, 3) if deep else want(cases, idx, depth, quiesce, 256, seed=77, draw=3)
    assert wr["score"].tobytes() == listed["score"].tobytes() and (wr["pick"] != listed["pick"]).any()
    same(env.minimax(idx, depth=depth, quiesce=quiesce, seed=77, draw=3, out=big, nodes=True), wr, n)
    same(env.minimax(idx, depth=depth, quiesce=quiesce, seed=77, draw=3, out=bare, nodes=True),
         wr if deep else want(cases, idx, depth, quiesce, 0, seed=77, draw=3), n, nodes=not deep)
    # fewer rows than a CU has SIMDs, and one row alone: the rows beyond them stay
    for rows in (1, 3):
        junk(env, cut)
        same(env.minimax(idx[:rows], depth=depth, quiesce=quiesce, out=cut, nodes=True), listed, rows, cap=8)
        rest = cut.fetch()
        assert all((rest[k][rows:].view(np.uint8) == 0x5B).all() for k in rest), rows
    env.synchronize()
    for b in (big, cut, bare):
        b.close()


# --------------------------------------------------------------------------- 2. quiesce=0
def test_quiesce_0_is_gc_env_minimax(env, cases):
    idx = cases[3]
    n = len(idx)
    a, b = env.minimax_buffer(n, cap=16), env.minimax_buffer(n, cap=16)
    for depth, seed in ((1, None), (2, None), (2, 5), (3, None)):
        junk(env, a)
        junk(env, b)
        env.minimax(idx, depth=depth, seed=seed, draw=9, quiesce=0, out=a, nodes=True)
        p = b.ptr
        from gym_chess_amd import _lib
        from test_policy_priors_gpu import Dev

        d = Dev(env, idx.astype(np.int32))
        _lib.check(env._L.gc_env_minimax(env._h, d.ptr, n, depth, int(seed is not None), ctypes.c_uint64(seed or 0), 9,
                                         p["pick"], p["score"], p["value"], p["count"], 16, p["actions"], p["scores"],
                                         p["nodes"]))
        ga, gb = a.fetch(), b.fetch()
        for k in ga:
            assert ga[k].tobytes() == gb[k].tobytes(), (depth, seed, k)
        w = want(cases, idx, depth, 0, 16, seed=seed, draw=9)
        same(a, w, n)
        env.synchronize()
        d.close()
    a.close()
    b.close()


# --------------------------------------------------------------------------- 3. the env is untouched
def test_env_untouched(cases):
    envs = []
    for _ in range(2):
        e = make_env(cases)
        e.select_random()
        e.step_random(3)  # windows, counters and outputs that are not the fresh env's
        envs.append(e)
    e, twin = envs
    before = (e.checkpoint(), e.window_sum(), e.outputs(), e.boards())
    buf = e.minimax_buffer(e.num_boards, cap=16)
    e.minimax(depth=2, quiesce=2, out=buf, nodes=True)
    e.minimax(np.arange(e.num_boards)[::-1], depth=1, quiesce=4, seed=3, draw=77, out=buf)
    e.synchronize()
    after = (e.checkpoint(), e.window_sum(), e.outputs(), e.boards())
    assert before[0] == after[0] and before[1] == after[1]
    for k in before[2]:
        assert (before[2][k] == after[2][k]).all(), k
    for x, y in zip(before[3], after[3]):
        assert x.tobytes() == y.tobytes()
    e.step_random(4)
    twin.step_random(4)
    for x, y in zip(e.boards(), twin.boards()):
        assert (x == y).all()
    assert e.checkpoint() == twin.checkpoint()
    buf.close()
    e.close()
    twin.close()


# --------------------------------------------------------------------------- 4. refusals
def test_refusals(env):
    from gym_chess_amd.env import BatchedChessEnv

    L = env._L
    buf = env.minimax_buffer(4, cap=8)
    junk(env, buf)
    p = buf.ptr
    seed = ctypes.c_uint64(1)
    outs = (p["pick"], p["score"], p["value"], p["count"], 8, p["actions"], p["scores"], p["nodes"])

    def refused(h, rows, depth, quiesce, tb, *rest):
        assert L.gc_env_minimax_q(h, None, rows, depth, quiesce, tb, seed, 0, *rest) == -1
        assert L.gc_last_error()

    for q in (-1, 5, 64):
        refused(env._h, 4, 2, q, 0, *outs)
        assert b"quiesce" in L.gc_last_error()
    refused(None, 4, 2, 2, 0, *outs)
    refused(env._h, -1, 2, 2, 0, *outs)
    for depth in (0, 5):
        refused(env._h, 4, depth, 2, 0, *outs)
    refused(env._h, 4, 2, 2, 2, *outs)
    refused(env._h, 4, 2, 2, 0, *outs[:4], -1, None, None, None)
    refused(env._h, 4, 2, 2, 0, *outs[:4], 0, p["actions"], None, None)
    with pytest.raises(RuntimeError):
        env.minimax(depth=2, quiesce=5, out=buf)
    with pytest.raises(RuntimeError):
        env.minimax(depth=2, quiesce=-1, out=buf)
    env.synchronize()
    after = buf.fetch()  # nothing was launched
    assert all((after[k].view(np.uint8) == 0x5B).all() for k in after)
    assert L.gc_env_minimax_q(env._h, None, 0, 2, 4, 0, seed, 0, *outs) == 0  # no rows: nothing to do
    assert L.gc_env_minimax_q(env._h, None, 4, 1, 4, 1, seed, 0, None, None, None, None, 0, None, None, None) == 0
    env.synchronize()
    buf.close()

    fide = BatchedChessEnv(4, device=0, rules="fide")
    fb = fide.minimax_buffer(4)
    junk(fide, fb)
    refused(fide._h, 4, 2, 2, 0, fb.ptr["pick"], fb.ptr["score"], fb.ptr["value"], fb.ptr["count"], 0, None, None, None)
    assert b"fide" in L.gc_last_error()
    with pytest.raises(RuntimeError):
        fide.minimax(depth=1, quiesce=1, out=fb)
    fide.synchronize()
    after = fb.fetch()
    assert all((after[k].view(np.uint8) == 0x5B).all() for k in after)
    fb.close()
    fide.close()


# --------------------------------------------------------------------------- 5. dirty memory
def fill_child(path):
    """(the child process) every buffer of this process starts as GC_ALLOC_FILL's byte; the rows the
    parent computed on the host must come back whole, the list padding included"""
    from gym_chess_amd import _lib

    fill = int(os.environ["GC_ALLOC_FILL"], 16)
    z = np.load(path)
    cases = (z["boards"], z["metas"])
    e = make_env(cases)
    idx, n = z["idx"], len(z["idx"])
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(_lib.load().gc_alloc_fill_stats(ctypes.byref(a), ctypes.byref(b)))
    assert a.value > 0
    for cap in (256, 0):
        buf = e.minimax_buffer(n, cap=cap)
        assert (buf.fetch("count")["count"].view(np.uint8) == fill).all()  # the fill is live
        e.minimax(idx, depth=2, quiesce=4, seed=77, draw=3, out=buf, nodes=True)
        same(buf, {k: z[f"{k}_{cap}"] for k in KEYS + ("nodes", "actions", "scores")}, n)
        buf.close()
    got = e.minimax(depth=1, quiesce=2).fetch()  # the env's own buffer
    for k in KEYS:
        assert got[k][: e.num_boards].tobytes() == z[f"own_{k}"].tobytes(), k
    e.close()
    print("fill child ok")


def test_dirty_memory_in_a_child_process(cases, tmp_path):
    boards, metas, done, idx = cases[:4]
    arrays = dict(boards=boards, metas=metas, idx=idx)
    for cap in (256, 0):
        w = want(cases, idx, 2, 4, cap, seed=77, draw=3)
        arrays.update({f"{k}_{cap}": v for k, v in w.items()})
    own = QH.run(boards, metas, np.arange(len(boards)), 1, quiesce=2, done=done)
    arrays.update({f"own_{k}": own[k] for k in KEYS})
    path = str(tmp_path / "rows.npz")
    np.savez(path, **arrays)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "fill-child", path], capture_output=True, text=True,
                       env=dict(os.environ, GC_ALLOC_FILL="a5"), timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "fill child ok" in r.stdout


# --------------------------------------------------------------------------- 6. through the search loop
def test_the_defended_pawn_through_the_search_loop():
    """one step_device(actions=bot.pick): with quiesce=0 the depth-1 bot plays Qxd5, with quiesce=2 it
    does not"""
    from gym_chess_amd.env import BatchedChessEnv

    pawn = PC.board_of(DEFENDED)
    meta = PC.settle(pawn, [1, 0, 0, 0, 0, 0, 0, 0])
    played = {}
    for q in (0, 2):
        e = BatchedChessEnv(4, device=0, seed=3)
        e.set_states(np.stack([pawn] * 4), np.stack([meta] * 4))
        io = e.device_io(pick=False)
        bot = e.minimax_buffer(4)
        e.minimax(depth=1, quiesce=q, out=bot)
        e.step_device(io, actions=bot.pick)
        got = bot.fetch("pick", "score")
        after = e.boards()[0]
        assert (got["pick"] == got["pick"][0]).all()
        played[q] = (int(got["pick"][0]), int(got["score"][0]), int(after[0][27]))
        for x in (io, bot):
            x.close()
        e.close()
    assert played[0] == (QXD5, 6, 2)  # the queen stands on d5
    assert played[2][0] != QXD5 and played[2][1:] == (5, -6)  # the pawn still does


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "fill-child":
    sys.path.insert(0, os.path.join(ROOT, "gym-chess_amd"))
    fill_child(sys.argv[2])
