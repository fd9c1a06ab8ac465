"""GPU: the device plane encoder (gc_env_encode_planes / BatchedChessEnv.encode_planes) and the
sampler's side-to-move-relative logits (gc_env_sample_policy flags bit 1) against the numpy
restatements of tests/test_planes.py.

Expected planes always come from the host API read back from the same env -- env.boards(),
env.en_passant(), gc_env_window_boards -- never from the inputs (set_states forces effective
castle rights), and equality is bit-exact on the raw elements."""
import ctypes

import numpy as np
import pytest

import test_planes as R
import test_policy_sample as P
from conftest import random_positions
from test_policy_sample_gpu import Dev, upload_mask
from test_spill import kb_board

pytestmark = pytest.mark.gpu

ELEMS = R.PLANES * 64
ITEM = {"float32": 4, "float16": 2, "bfloat16": 2}
GUARD = 4096
SPILL_PLIES = 1181


# ----------------------------------------------------------------------------- helpers
def rep_counts(env, boards, ids=None):
    """per board: the count of the window entry equal to its current board, else 0
    (gc_env_window_boards); also the window lengths"""
    from gym_chess_amd import _lib

    n = env.num_boards
    cnt = np.zeros(n, dtype=np.int64)
    length = np.zeros(n, dtype=np.int64)
    cap = 2048
    wb = np.zeros((cap, 64), dtype=np.int8)
    wc = np.zeros(cap, dtype=np.uint8)
    for i in (range(n) if ids is None else ids):
        k = ctypes.c_int(0)
        _lib.check(env._L.gc_env_window_boards(env._h, int(i), _lib.ptr(wb), _lib.ptr(wc), cap, ctypes.byref(k)))
        assert k.value <= cap
        length[i] = k.value
        hit = np.flatnonzero((wb[: k.value] == boards[i]).all(axis=1))
        assert hit.size <= 1
        if hit.size:
            cnt[i] = wc[hit[0]]
    return cnt, length


def expected(env, perspective, layout, rep=None):
    """the restatement on the env's host readback -> float32 planes"""
    b, m = env.boards()
    if rep is None:
        rep = rep_counts(env, b)[0]
    return R.ref_planes(b, m, rep, env.en_passant(), perspective, layout)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)


def encode_guarded(env, dtype, layout, perspective, stride):
    """encode into a 0xA5-filled buffer with a 4 KiB guard behind it -> (raw bytes [N][stride *
    item], the guard's bytes)"""
    from gym_chess_amd import _lib

    n = env.num_boards
    nb = n * stride * ITEM[dtype]
    buf = Dev(env, np.full(nb + GUARD, 0xA5, dtype=np.uint8))
    env.encode_planes(buf.ptr, dtype=dtype, layout=layout, perspective=perspective, board_stride=stride)
    back = np.zeros(nb + GUARD, dtype=np.uint8)
    _lib.check(env._L.gc_env_copy(env._h, _lib.ptr(back), buf.ptr, ctypes.c_uint64(back.nbytes), 2))
    buf.close()
    return back[:nb].reshape(n, stride * ITEM[dtype]), back[nb:]


def check_guarded(env, want, dtype, layout, perspective, stride):
    raw, guard = encode_guarded(env, dtype, layout, perspective, stride)
    exp = as_bytes(R.encode_raw(want.reshape(env.num_boards, ELEMS), dtype))
    used = ELEMS * ITEM[dtype]
    bad = np.flatnonzero((raw[:, :used] != exp).any(axis=1))
    assert bad.size == 0, (dtype, layout, perspective, stride, bad[:5])
    assert (raw[:, used:] == 0xA5).all(), "the padding between boards was written"
    assert (guard == 0xA5).all(), "the guard behind the buffer was written"


def make_env(n, seed, **kw):
    """an env of n boards set to random_positions(n, seed, weird=True) with random move counts"""
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(n, device=0, seed=seed, **kw)
    boards, metas = random_positions(n, seed, weird=True)
    metas[:, 7] = np.random.RandomState(seed).randint(0, 150, size=n)
    env.set_states(boards, metas)
    return env


# ----------------------------------------------------------------------------- 1. shapes and views
@pytest.fixture(scope="module")
def env200():
    env = make_env(200, 3)
    b, m = env.boards()
    assert 40 <= int(m[:, 0].sum()) <= 160  # both colours to move
    assert len(set(m[:, 7].tolist())) > 50
    return env


@pytest.fixture(scope="module")
def want200(env200):
    rep = rep_counts(env200, env200.boards()[0])[0]
    return {(p, lay): expected(env200, p, lay, rep) for p in (False, True) for lay in R.LAYOUTS}


@pytest.mark.parametrize("stride", [1536, 1544])
@pytest.mark.parametrize("perspective", [False, True])
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_shapes_and_views(env200, want200, dtype, layout, perspective, stride):
    """N = 200 (three full waves of boards plus a ragged tail), weird random positions: every
    raw element equals the restatement's; the padding and a 4 KiB guard stay 0xA5"""
    check_guarded(env200, want200[(perspective, layout)], dtype, layout, perspective, stride)


@pytest.mark.parametrize("n", [1, 65])
def test_small_batches(n):
    env = make_env(n, 3)
    rep = rep_counts(env, env.boards()[0])[0]
    for perspective in (False, True):
        for layout in R.LAYOUTS:
            want = expected(env, perspective, layout, rep)
            for dtype in R.DTYPES:
                check_guarded(env, want, dtype, layout, perspective, 1536)
    env.close()


def test_board_result_does_not_depend_on_n(env200):
    """boards 0..63 of N = 64 equal boards 0..63 of N = 200 (the same positions)"""
    from gym_chess_amd.env import BatchedChessEnv

    b, m = env200.boards()
    small = BatchedChessEnv(64, device=0, seed=3)
    small.set_states(b[:64], m[:64])
    for dtype in R.DTYPES:
        for layout in R.LAYOUTS:
            for perspective in (False, True):
                big = encode_guarded(env200, dtype, layout, perspective, 1536)[0]
                lit = encode_guarded(small, dtype, layout, perspective, 1536)[0]
                assert (big[:64] == lit).all(), (dtype, layout, perspective)
    small.close()


def test_planes_buffer_fetch(env200, want200):
    """the Python buffer class: fetch() decodes the raw elements to float32 in the layout's shape"""
    for dtype in R.DTYPES:
        for layout, shape in (("nchw", (200, 24, 8, 8)), ("nhwc", (200, 8, 8, 24))):
            buf = env200.planes_buffer(dtype=dtype, layout=layout, board_stride=1544 if dtype == "float16" else None)
            env200.encode_planes(buf, perspective=True)
            got = buf.fetch()
            assert got.shape == shape and got.dtype == np.float32
            assert (got == want200[(True, layout)]).all(), (dtype, layout)
            buf.close()
            assert buf.ptr is None


# ----------------------------------------------------------------------------- 2. repetition
def test_repetition_planes():
    """N = 130, opponent "none", host step(): knight shuffles (g-knights on even boards, b-knights
    on odd ones; boards with i % 3 == 0 open with a pawn move, which empties the window).  After
    each of 8 plies planes 20 / 21 equal the window's count of the current board; the run sees
    boards with plane 20 only, with both planes, and with neither."""
    from gym_chess_amd import codec as C
    from gym_chess_amd.env import BatchedChessEnv

    n = 130
    env = BatchedChessEnv(n, device=0, seed=1)
    g = [C.str_to_action(s) for s in ("g1f3", "g8f6", "f3g1", "f6g8")]
    bk = [C.str_to_action(s) for s in ("b1c3", "b8c6", "c3b1", "c6b8")]
    pawn = C.str_to_action("e2e3")
    buf = env.planes_buffer(dtype="float16")
    seen = set()
    for ply in range(8):
        acts = np.zeros(n, dtype=np.int64)
        for i in range(n):
            cyc = bk if i % 2 else g
            if i % 3 == 0:  # the pawn move, then the shuffle starting with BLACK's knight
                acts[i] = pawn if ply == 0 else [cyc[1], cyc[0], cyc[3], cyc[2]][(ply - 1) % 4]
            else:
                acts[i] = cyc[ply % 4]
        rw, dn, why = env.step(acts)
        assert not dn.any() and not np.isin(why, (6, 7)).any(), (ply, why)
        env.encode_planes(buf)
        got = buf.fetch()
        b, m = env.boards()
        rep, length = rep_counts(env, b)
        assert (got[:, 20] == (rep >= 1)[:, None, None]).all(), ply
        assert (got[:, 21] == (rep >= 2)[:, None, None]).all(), ply
        assert (got == R.ref_planes(b, m, rep, env.en_passant(), False, "nchw")).all(), ply
        seen |= set(np.minimum(rep, 2).tolist())
        if ply == 7:
            plain = np.arange(n) % 3 != 0
            assert (rep[plain] == 2).all() and (rep[~plain] == 1).all() and (length[plain] == 4).all()
    assert seen == {0, 1, 2}
    buf.close()
    env.close()


# ----------------------------------------------------------------------------- 3. spill
def test_spilled_windows():
    """tests/test_spill.py's workload (a BLACK agent against the random opponent from the sparse
    kings-and-bishops board, its first 96 boards), rolled out on the device for 1181 plies, then
    encoded: planes 20 / 21 of all 96 boards equal the window's count of the current board, and
    at least one board's window is longer than the 511 entries of its table at that moment, so
    the find covers the env's spill table.  (1181 plies: on the CPU, replaying the oracle's
    trajectories of these boards, 5 of the 96 windows are longer than 511 there, the longest
    609 -- the most at any ply count up to 3 000.  Whether a spilled board's current position
    recurs at that ply is not required.)"""
    from gym_chess_amd.env import BatchedChessEnv

    n = 96
    env = BatchedChessEnv(n, device=0, seed=7, initial_board=kb_board(), opponent="random", player_color="BLACK")
    env.rollout_device(SPILL_PLIES)
    env.synchronize()
    assert env.spill_info()["live"] > 0
    buf = env.planes_buffer(dtype="bfloat16", layout="nhwc")
    env.encode_planes(buf, perspective=True)
    got = buf.fetch()
    b, m = env.boards()
    rep, length = rep_counts(env, b)
    print(f"windows longer than 511: {(length > 511).sum()} boards, longest {length.max()}; "
          f"current board in its window on {(rep >= 1).sum()} boards ({(rep >= 2).sum()} twice), "
          f"{((rep >= 1) & (length > 511)).sum()} of them spilled")
    assert (length > 511).sum() >= 1
    assert (got[..., 20] == (rep >= 1)[:, None, None]).all()
    assert (got[..., 21] == (rep >= 2)[:, None, None]).all()
    assert (got == R.ref_planes(b, m, rep, env.en_passant(), True, "nhwc")).all()
    buf.close()
    env.close()


# ----------------------------------------------------------------------------- 4. FIDE
FENS = ["rnbqkbnr/ppp1pppp/8/8/3pP3/8/PPPP1PPP/RNBQKBNR b KQkq e3 0 3",   # BLACK to move, target e3
        "rnbqkbnr/ppp1pppp/8/3pP3/8/8/PPPP1PPP/RNBQKBNR w KQkq d6 0 3",   # WHITE to move, target d6
        "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"]


def test_fide_en_passant_plane():
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(3, device=0, seed=2, rules="fide")
    env.set_fens(FENS)
    assert env.en_passant().tolist() == [4, 3, -1]
    for dtype in R.DTYPES:
        for layout in R.LAYOUTS:
            for perspective in (False, True):
                check_guarded(env, expected(env, perspective, layout), dtype, layout, perspective, 1536)
    buf = env.planes_buffer(dtype="float32")
    env.encode_planes(buf)
    a = buf.fetch()
    env.encode_planes(buf, perspective=True)
    r = buf.fetch()
    assert a[0, 22].sum() == 1 and a[0, 22, 5, 4] == 1 and r[0, 22].sum() == 1 and r[0, 22, 2, 4] == 1
    assert a[1, 22].sum() == 1 and a[1, 22, 2, 3] == 1 and (r[1] == a[1]).all()
    assert a[2, 22].sum() == 0 and r[2, 22].sum() == 0
    assert a[0, 5, 4, 4] == 1 and a[0, 11, 4, 3] == 1  # the e4 pawn, the d4 pawn
    assert r[0, 5, 3, 3] == 1 and r[0, 11, 3, 4] == 1  # BLACK first, rows mirrored
    buf.close()
    env.close()
    # the reference's rules have no en passant: the same boards, plane 22 all zero
    ref = BatchedChessEnv(3, device=0, seed=2)
    ref.set_fens(FENS)
    buf = ref.planes_buffer(dtype="float32")
    ref.encode_planes(buf)
    got = buf.fetch()
    assert (got[:, 22] == 0).all() and (got[:, :12] == a[:, :12]).all()
    assert (got == expected(ref, False, "nchw")).all()
    buf.close()
    ref.close()


# ----------------------------------------------------------------------------- 5. the loop
def _loop(opponent, encode, steps=50, n=256, seed=9):
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(n, device=0, seed=seed, opponent=opponent)
    # late middle games, so that episodes end inside the 50 steps (a random game from the start
    # position lasts longer: the move cap falls at ~300 plies, 150 steps against the opponent)
    env.step_random(270 if opponent == "none" else 120)
    io = env.device_io()
    buf = env.planes_buffer(dtype="float16", layout="nhwc") if encode else None
    trace, mcs = [], set()
    for it in range(steps):
        env.step_device(io, autoreset=True)
        if encode:
            env.encode_planes(buf, perspective=True)  # no synchronize between
            got = buf.fetch()
            b, m = env.boards()
            last = it == steps - 1
            rep = rep_counts(env, b)[0] if last else np.zeros(n, dtype=np.int64)
            want = R.ref_planes(b, m, rep, env.en_passant(), True, "nhwc")
            keep = np.ones(R.PLANES, dtype=bool)
            keep[20:22] = last  # the windows are read out (256 single-thread scans) once, at the end
            assert (got[..., keep] == want[..., keep]).all(), it
            assert (got[..., 21] <= got[..., 20]).all()
            mcs |= set(m[:, 7].tolist())
        o = io.fetch("reward", "done", "reason", "pick")
        trace.append((o["reward"].copy(), o["done"].copy(), o["reason"].copy(), o["pick"].copy()))
    if encode:
        assert len(mcs) > 5  # plane 19 varies
        buf.close()
    io.close()
    env.close()
    return [np.stack(t) for t in zip(*trace)]


@pytest.mark.parametrize("opponent", ["none", "random"])
def test_step_encode_loop_and_non_interference(opponent):
    """50 x (step_device(autoreset) on io.pick -> encode_planes, no synchronize between -> fetch
    and compare with env.boards()): games end and reset inside the loop, move_count varies, and
    the same 50 steps without any encode call give identical reward / done / reason / pick"""
    a = _loop(opponent, True)
    b = _loop(opponent, False)
    assert a[1].any(), "no game ended inside the loop"
    for x, y in zip(a, b):
        assert (x == y).all()


# ----------------------------------------------------------------------------- 6. relative sampler
@pytest.fixture(scope="module")
def rel_rig():
    """N = 200 random positions of both colours to move, their legal masks uploaded"""
    from gym_chess_amd import _lib

    n = 200
    env = make_env(n, 12)
    io = env.device_io(obs=False, count=False, select=False, mask_stride=256, policy=True)
    masks = np.zeros((n, 65), dtype=np.uint64)
    cnt = np.zeros(n, dtype=np.int32)
    _lib.check(env._L.gc_env_legal_mask(env._h, _lib.ptr(masks), _lib.ptr(cnt)))
    upload_mask(env, io, masks)
    black = env.boards()[1][:, 0] == 0
    assert 50 <= black.sum() <= 150 and (cnt[black] > 0).sum() >= 40
    return env, io, masks, black


def _sample(rig, raw, dtype, **kw):
    env, io = rig[0], rig[1]
    buf = Dev(env, raw)
    env.sample_policy(io, buf.ptr, dtype=dtype, row_stride=raw.shape[1], **kw)
    o = io.fetch("pick", "logprob", "entropy")
    buf.close()
    return o["pick"], o["logprob"], o["entropy"]


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_relative_sampler(rel_rig, dtype):
    """flags bit 1: on BLACK-to-move boards the logit of action a is read at mirror(a) -- the
    reference and acceptance rule of test_policy_sample.py, unchanged, on val_rel[i, a] =
    val[i, mirror(a)]; greedy equals the float64 argmax of val_rel exactly"""
    env, io, masks, black = rel_rig
    n = env.num_boards
    raw, val = P.synthetic_logits(n, 4100, dtype, 4)
    val_rel = val.copy()
    val_rel[black] = val[black][:, R.mirror_action(np.arange(4100))]
    us = P.uniform(env.seed, np.arange(n), 3)
    act, lp, ent = _sample(rel_rig, raw, dtype, draw=3, relative=True)
    exact, small = P.check_sampler(act, lp, ent, val_rel, masks, 1.0, us)
    print(f"{dtype}: exact picks {exact}/{small}")
    # not vacuous: the absolute reading of the same logits picks other actions on BLACK's boards
    # (two independent softmaxes over >= 4 actions share the action at quantile u less than
    # half the time; a fifth of the boards differing is far below that)
    plain = _sample(rel_rig, raw, dtype, draw=3)
    multi = black & np.array([P.legal_actions(m).size >= 4 for m in masks])
    assert multi.sum() >= 30 and (plain[0][multi] != act[multi]).mean() > 0.2
    assert (plain[0][~black] == act[~black]).all()
    gact, glp, gent = _sample(rel_rig, raw, dtype, greedy=True, relative=True)
    for i in range(n):
        acts = P.legal_actions(masks[i])
        if acts.size == 0:
            assert gact[i] == P.NONE
            continue
        j, want_lp = P.ref_greedy(val_rel[i], masks[i], 1.0)
        assert gact[i] == acts[j], (i, gact[i], acts[j])
        assert abs(glp[i] - want_lp) <= 4 * P.eps(acts.size)


def test_relative_flag_off_is_todays_sampler(rel_rig):
    from gym_chess_amd import _lib

    env, io, masks, black = rel_rig
    raw, _ = P.synthetic_logits(env.num_boards, 4104, "bfloat16", 5)
    buf = Dev(env, raw)
    p = io.ptr

    def call(flags):
        _lib.check(env._L.gc_env_sample_policy(env._h, buf.ptr, 2, 4104, p["mask"], io.mask_stride, 1.0,
                                               ctypes.c_uint64(env.seed), 6, flags, p["pick"], p["logprob"], p["entropy"]))
        o = io.fetch("pick", "logprob", "entropy")
        return [o[k].copy() for k in ("pick", "logprob", "entropy")]

    for greedy in (False, True):
        direct = call(int(greedy))
        env.sample_policy(io, buf.ptr, dtype="bfloat16", row_stride=4104, draw=6, greedy=greedy, relative=False)
        o = io.fetch("pick", "logprob", "entropy")
        for x, k in zip(direct, ("pick", "logprob", "entropy")):
            assert (x.view(np.uint8) == o[k].view(np.uint8)).all(), (greedy, k)
    call(2)
    call(3)
    for flags in (4, 5, 8, -1):
        with pytest.raises(_lib.GymChessError) as ei:
            call(flags)
        assert str(ei.value)
    buf.close()


# ----------------------------------------------------------------------------- 7. argument errors
def test_argument_errors(env200):
    from gym_chess_amd import _lib

    e = env200
    buf = e.planes_buffer(dtype="float32", board_stride=1544)

    def call(env=e._h, ptr=buf.ptr, dtype=1, stride=0, flags=0):
        _lib.check(e._L.gc_env_encode_planes(env, ptr, dtype, stride, flags))

    call()
    call(dtype=0, stride=1544, flags=3)
    for kw in (dict(env=None), dict(ptr=None), dict(dtype=3), dict(dtype=-1), dict(flags=4), dict(flags=-1),
               dict(stride=8), dict(stride=1528), dict(stride=-8), dict(stride=1540), dict(stride=1537),
               dict(ptr=buf.ptr + 8), dict(ptr=buf.ptr + 2)):
        with pytest.raises(_lib.GymChessError) as ei:
            call(**kw)
        assert str(ei.value), kw
    with pytest.raises(ValueError):
        e.encode_planes(buf, dtype="float64")
    with pytest.raises(ValueError):
        e.encode_planes(buf, layout="chwn")
    with pytest.raises(ValueError):
        e.planes_buffer(dtype="int8")
    with pytest.raises(ValueError):
        e.planes_buffer(layout="nchw8")
    with pytest.raises(ValueError):
        e.planes_buffer(board_stride=1540)
    e.synchronize()
    buf.close()
