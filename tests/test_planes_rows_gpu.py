"""GPU: the plane encoder of the listed boards (gc_env_encode_planes_rows /
BatchedChessEnv.encode_planes_rows) against the dense encoder (encode_planes, pinned to the numpy
reference by test_planes_gpu.py): row j must equal the dense tensor's row of board idx[j], bit for
bit.

Boards: test_clone_gpu's three recipes on 130 boards (mid-game, both sides to move), half of the
shuffle boards one ply further so that their position has occurred twice (plane 21 as well as 20);
and three FIDE boards, two with an en-passant square.  Index lists: a duplicate-bearing permuted
one of 67 rows and a single row."""
import ctypes

import numpy as np
import pytest

from test_clone_gpu import IDLE, SEED, SHUFFLE, play_recipes, recipe
from test_planes_gpu import FENS
from test_policy_sample_gpu import Dev

pytestmark = pytest.mark.gpu

N = 130
ELEMS = 1536
ITEM = {"float32": 4, "float16": 2, "bfloat16": 2}
DTYPES = ("float32", "float16", "bfloat16")
LAYOUTS = ("nchw", "nhwc")
GUARD = 4096


def index_lists():
    rng = np.random.RandomState(8)
    idx = rng.permutation(N)[:60]
    idx = np.concatenate([idx, idx[:5], [129, 128]])  # 67 rows: duplicates, the partial block of 64
    return [rng.permutation(idx).astype(np.int32), np.array([129], dtype=np.int32)]


def dense_raw(env, dtype, layout, perspective):
    buf = env.planes_buffer(dtype=dtype, layout=layout)
    env.encode_planes(buf, perspective=perspective)
    a = buf.raw()
    buf.close()
    return np.ascontiguousarray(a).view(np.uint8).reshape(env.num_boards, ELEMS * ITEM[dtype])


def rows_raw(env, idx, dtype, layout, perspective, stride):
    """encode_planes_rows into a 0xAB-filled block with a guard behind it -> (bytes [rows][stride *
    item], the guard's bytes)"""
    from gym_chess_amd import _lib

    nb = len(idx) * stride * ITEM[dtype]
    buf = Dev(env, np.full(nb + GUARD, 0xAB, dtype=np.uint8))
    env.encode_planes_rows(buf.ptr, idx, dtype=dtype, layout=layout, perspective=perspective, row_stride=stride)
    back = np.zeros(nb + GUARD, dtype=np.uint8)
    _lib.check(env._L.gc_env_copy(env._h, _lib.ptr(back), buf.ptr, ctypes.c_uint64(back.nbytes), 2))
    buf.close()
    return back[:nb].reshape(len(idx), stride * ITEM[dtype]), back[nb:]


def check_rows(env, want, idx, dtype, layout, perspective, stride):
    raw, guard = rows_raw(env, idx, dtype, layout, perspective, stride)
    used = ELEMS * ITEM[dtype]
    bad = np.flatnonzero((raw[:, :used] != want[idx]).any(axis=1))
    assert bad.size == 0, (dtype, layout, perspective, stride, bad[:5])
    assert (raw[:, used:] == 0xAB).all(), "the padding between rows was written"
    assert (guard == 0xAB).all(), "the guard behind the block was written"


@pytest.fixture(scope="module")
def env130():
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(N, device=0, seed=SEED)
    play_recipes(env)
    acts = np.full(N, IDLE)
    acts[[i for i in range(N) if i % 13 == 8]] = SHUFFLE[3]  # Ng8: the start position, seen twice before
    env.step(acts)
    _, m = env.boards()
    assert 10 <= int(m[:, 0].sum()) <= N - 10  # both colours to move
    yield env
    env.close()


@pytest.fixture(scope="module")
def want130(env130):
    """the dense encoder's bytes, once per (dtype, layout, perspective)"""
    want = {(d, lay, p): dense_raw(env130, d, lay, p) for d in DTYPES for lay in LAYOUTS for p in (False, True)}
    pl = want[("float32", "nchw", False)].view(np.float32).reshape(N, 24, 64)
    sh7 = [i for i in range(N) if i % 13 == 7]
    sh8 = [i for i in range(N) if i % 13 == 8]
    assert recipe(sh7[0]) == recipe(sh8[0]) == "shuffle"
    assert (pl[sh7, 20] == 1).all() and (pl[sh7, 21] == 0).all()
    assert (pl[sh8, 20] == 1).all() and (pl[sh8, 21] == 1).all()
    return want


@pytest.mark.parametrize("perspective", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_equal_dense(env130, want130, dtype, layout, perspective):
    want = want130[(dtype, layout, perspective)]
    for idx in index_lists():
        for stride in (1536, 1544):
            check_rows(env130, want, idx, dtype, layout, perspective, stride)


def test_planes_buffer_rows_and_device_index(env130, want130):
    idx = index_lists()[0]
    buf = env130.planes_buffer(dtype="bfloat16", layout="nhwc", board_stride=1544, rows=len(idx))
    assert buf.rows == len(idx) and buf.nbytes == len(idx) * 1544 * 2
    ip = Dev(env130, idx)
    env130.encode_planes_rows(buf, ip.ptr, rows=len(idx), perspective=True)
    raw = buf.raw()
    assert raw.shape == (len(idx), 1544)
    want = want130[("bfloat16", "nhwc", True)].view(np.uint16)
    assert (raw[:, :ELEMS] == want[idx]).all()
    dense = env130.planes_buffer(dtype="bfloat16", layout="nhwc")
    env130.encode_planes(dense, perspective=True)
    assert buf.fetch().shape == (len(idx), 8, 8, 24) and (buf.fetch() == dense.fetch()[idx]).all()
    with pytest.raises(ValueError):
        env130.encode_planes_rows(buf, np.arange(len(idx) + 1))  # more rows than the buffer holds
    with pytest.raises(ValueError):
        env130.encode_planes_rows(buf, ip.ptr)  # a device pointer needs rows
    for x in (buf, dense, ip):
        x.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_out_of_range_rows_are_zero(env130, want130, dtype):
    idx = np.array([5, -1, 64, N, 2 ** 31 - 1, 129, -(2 ** 31)], dtype=np.int64)
    ok = np.array([0, 2, 5])
    for layout in LAYOUTS:
        raw, guard = rows_raw(env130, idx, dtype, layout, True, 1544)
        used = ELEMS * ITEM[dtype]
        assert (raw[ok, :used] == want130[(dtype, layout, True)][idx[ok]]).all()
        bad = np.setdiff1d(np.arange(len(idx)), ok)
        assert (raw[bad, :used] == 0).all()
        assert (raw[:, used:] == 0xAB).all() and (guard == 0xAB).all()


def test_fide_en_passant_rows():
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(3, device=0, seed=2, rules="fide")
    env.set_fens(FENS)
    assert env.en_passant().tolist() == [4, 3, -1]
    idx = np.array([2, 0, 0, 1], dtype=np.int32)
    for dtype in DTYPES:
        for layout in LAYOUTS:
            for perspective in (False, True):
                check_rows(env, dense_raw(env, dtype, layout, perspective), idx, dtype, layout, perspective, 1536)
    buf = env.planes_buffer(dtype="float32", rows=4)
    env.encode_planes_rows(buf, idx, perspective=True)
    r = buf.fetch()
    assert r[1, 22].sum() == 1 and r[1, 22, 2, 4] == 1 and (r[2] == r[1]).all()  # e3, mirrored (BLACK to move)
    assert r[3, 22].sum() == 1 and r[3, 22, 2, 3] == 1 and r[0, 22].sum() == 0
    buf.close()
    env.close()


def test_black_agent_env_rows():
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(70, device=0, seed=6, opponent="random", player_color="BLACK")
    env.step_random(25)
    idx = np.array([69, 0, 64, 63, 69], dtype=np.int32)
    check_rows(env, dense_raw(env, "float16", "nchw", True), idx, "float16", "nchw", True, 1536)
    env.close()


def test_argument_errors(env130):
    from gym_chess_amd import _lib

    e = env130
    buf = e.planes_buffer(dtype="float32", board_stride=1544, rows=4)
    idx = Dev(e, np.arange(4, dtype=np.int32))

    def call(env=e._h, ip=idx.ptr, rows=4, ptr=buf.ptr, dtype=1, stride=0, flags=0):
        _lib.check(e._L.gc_env_encode_planes_rows(env, ip, rows, ptr, dtype, stride, flags))

    call()
    call(dtype=0, stride=1544, flags=3)
    call(rows=0)
    call(rows=0, ip=None)
    e.encode_planes_rows(buf, [])
    for kw in (dict(env=None), dict(ptr=None), dict(ip=None), dict(rows=-1), dict(dtype=3), dict(dtype=-1), dict(flags=4),
               dict(flags=-1), dict(stride=8), dict(stride=1528), dict(stride=-8), dict(stride=1540), dict(stride=1537),
               dict(ptr=buf.ptr + 8), dict(ptr=buf.ptr + 2)):
        with pytest.raises(_lib.GymChessError) as ei:
            call(**kw)
        assert str(ei.value), kw
    with pytest.raises(ValueError):
        e.encode_planes_rows(buf, [0], dtype="float64")
    with pytest.raises(ValueError):
        e.encode_planes_rows(buf, [0], layout="chwn")
    with pytest.raises(ValueError):
        e.planes_buffer(rows=-1)
    e.synchronize()
    buf.close()
    idx.close()
