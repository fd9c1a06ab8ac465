"""GPU: the device policy head (gc_env_sample_policy / BatchedChessEnv.sample_policy) against the
float64 reference and acceptance rule of test_policy_sample.py: synthetic masks (one family per
way the mapping can go wrong), the three logit types, greedy, poisoned entries, the random
stream, the sample -> step loop, and argument errors.  Buffers come from gc_device_alloc /
gc_env_copy; bf16 / fp16 logits are quantised in numpy and the reference reads those values."""
import ctypes

import numpy as np
import pytest

import test_policy_sample as P

pytestmark = pytest.mark.gpu

N, STRIDE, SEED = 200, 256, 11


class Dev:
    """a device buffer holding a host array (gc_device_alloc + an h2d copy on the env's stream)"""

    def __init__(self, env, host):
        from gym_chess_amd import _lib

        self.env, self._lib = env, _lib
        host = np.ascontiguousarray(host)
        v = ctypes.c_void_p()
        _lib.check(env._L.gc_device_alloc(env.device, ctypes.c_uint64(max(host.nbytes, 1)), ctypes.byref(v)))
        self.ptr = v.value
        if host.nbytes:
            _lib.check(env._L.gc_env_copy(env._h, self.ptr, _lib.ptr(host), ctypes.c_uint64(host.nbytes), 1))

    def close(self):
        if self.ptr:
            self.env._L.gc_device_free(self.env.device, ctypes.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def upload_mask(env, io, masks):
    """masks [n][65] -> io's word-major device mask [65][mask_stride]"""
    from gym_chess_amd import _lib

    w = np.zeros((65, io.mask_stride), dtype=np.uint64)
    w[:, : masks.shape[0]] = masks.T
    _lib.check(env._L.gc_env_copy(env._h, io.ptr["mask"], _lib.ptr(w), ctypes.c_uint64(w.nbytes), 1))


class Rig:
    """an env of n boards, its policy io (mask stride as given) and one sampler call"""

    def __init__(self, n, mask_stride, seed=SEED):
        from gym_chess_amd.env import BatchedChessEnv

        self.n = n
        self.env = BatchedChessEnv(n, device=0, seed=seed)
        self.io = self.env.device_io(obs=False, count=False, select=False, mask_stride=mask_stride, policy=True)

    def run(self, masks, raw, dtype, row_stride, **kw):
        upload_mask(self.env, self.io, masks)
        buf = Dev(self.env, raw)
        self.env.sample_policy(self.io, buf.ptr, dtype=dtype, row_stride=row_stride, **kw)
        o = self.io.fetch("pick", "logprob", "entropy")
        buf.close()
        return o["pick"], o["logprob"], o["entropy"]


@pytest.fixture(scope="module")
def rig():
    return Rig(N, STRIDE)


@pytest.fixture(scope="module")
def masks():
    return P.synthetic_masks(N, 1)


@pytest.fixture(scope="module")
def us():
    return {d: P.uniform(SEED, np.arange(N), d) for d in range(4)}


def same_bits(a, b):
    return all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b))


# --------------------------------------------------------------------------- 1. synthetic masks
@pytest.mark.parametrize("row_stride", [4100, 4101, 4104])
@pytest.mark.parametrize("dtype", P.DTYPES)
def test_synthetic_masks(rig, masks, us, dtype, row_stride):
    """N = 200 (tiles plus a ragged tail), mask stride 256, every mask family: the acceptance
    rule on every board, the 99 % cap, log-prob and entropy in tolerance, empty boards 0xFFFF/0/0"""
    raw, val = P.synthetic_logits(N, row_stride, dtype, 2)
    act, lp, ent = rig.run(masks, raw, dtype, row_stride, draw=0)
    exact, small = P.check_sampler(act, lp, ent, val, masks, 1.0, us[0])
    print(f"{dtype} stride {row_stride}: exact picks {exact}/{small} boards with 1 <= m <= 64")
    empty = np.arange(N) % 9 == 0
    assert (act[empty] == P.NONE).all() and (lp[empty] == 0).all() and (ent[empty] == 0).all()
    assert (act[~empty] < 4100).all()


def test_temperature(rig, masks, us):
    T = np.float32(0.8)
    raw, val = P.synthetic_logits(N, 4104, "bfloat16", 3)
    act, lp, ent = rig.run(masks, raw, "bfloat16", 4104, draw=1, temperature=float(T))
    P.check_sampler(act, lp, ent, val, masks, T, us[1])


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_one_board_packed_stride(dtype):
    """N = 1, mask stride = N"""
    r = Rig(1, 1, seed=5)
    for fam in range(9):
        m = P.synthetic_masks(9, 4)[fam: fam + 1]
        raw, val = P.synthetic_logits(1, 4101, dtype, 6 + fam)
        act, lp, ent = r.run(m, raw, dtype, 4101, draw=fam)
        P.check_sampler(act, lp, ent, val, m, 1.0, P.uniform(5, np.arange(1), fam))
    r.env.close()


# --------------------------------------------------------------------------- 2. greedy
@pytest.mark.parametrize("dtype", P.DTYPES)
def test_greedy(rig, masks, dtype):
    """greedy == the float64 argmax exactly; a maximum duplicated at two legal ids goes to the
    lower; log-prob (at the temperature) and entropy as in sampling mode"""
    x = np.random.RandomState(7).uniform(-8.0, 8.0, size=(N, 4100)).astype(np.float32)
    dup = 0
    for i in range(N):
        acts = P.legal_actions(masks[i])
        if acts.size >= 2 and i % 2:
            a = np.random.RandomState(i).choice(acts, size=2, replace=False)
            x[i, a] = 8.0  # the top of the range, exact in every type
            dup += 1
    assert dup >= 60
    raw, val = P.quantise(x, dtype)
    T = np.float32(0.8)
    act, lp, ent = rig.run(masks, raw, dtype, 4100, greedy=True, temperature=float(T))
    for i in range(N):
        acts = P.legal_actions(masks[i])
        if acts.size == 0:
            assert act[i] == P.NONE and lp[i] == 0 and ent[i] == 0
            continue
        j, want_lp = P.ref_greedy(val[i], masks[i], T)
        assert act[i] == acts[j], (i, act[i], acts[j])
        assert abs(lp[i] - want_lp) <= 4 * P.eps(acts.size), (i, lp[i], want_lp)
        H = P.ref_sample(val[i], masks[i], T, 0.5)[2]
        assert abs(ent[i] - H) <= 16 * P.eps(acts.size), (i, ent[i], H)


# --------------------------------------------------------------------------- 3. poisoned entries
def test_illegal_logits_are_never_used(rig, masks, us):
    """every illegal logit NaN: bit-identical outputs, all three types, both modes"""
    for dtype in P.DTYPES:
        x = np.random.RandomState(8).uniform(-8.0, 8.0, size=(N, 4101)).astype(np.float32)
        y = np.full_like(x, np.nan)
        for i in range(N):
            a = P.legal_actions(masks[i])
            y[i, a] = x[i, a]
        for greedy in (False, True):
            clean = rig.run(masks, P.quantise(x, dtype)[0], dtype, 4101, draw=2, greedy=greedy)
            poisoned = rig.run(masks, P.quantise(y, dtype)[0], dtype, 4101, draw=2, greedy=greedy)
            assert same_bits(clean, poisoned), (dtype, greedy)
            assert not np.isnan(poisoned[1]).any() and not np.isnan(poisoned[2]).any()


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_legal_minus_inf_and_unusable_rows(rig, masks, us, dtype):
    """a legal -inf is never chosen (and the rest still meets the rule); an all -inf board and a
    board with a legal NaN give 0xFFFF and NaN"""
    x = np.random.RandomState(9).uniform(-8.0, 8.0, size=(N, 4100)).astype(np.float32)
    kind = np.zeros(N, dtype=int)  # 1 some -inf, 2 all -inf, 3 a legal NaN
    for i in range(N):
        a = P.legal_actions(masks[i])
        rs = np.random.RandomState(100 + i)
        if a.size == 0:
            continue
        kind[i] = 1 + (i // 9) % 3
        if kind[i] == 1 and a.size >= 2:
            x[i, rs.choice(a, size=max(1, a.size // 2), replace=False)] = -np.inf
        elif kind[i] == 1:
            kind[i] = 0
        elif kind[i] == 2:
            x[i, a] = -np.inf
        else:
            x[i, rs.choice(a)] = np.nan
    raw, val = P.quantise(x, dtype)
    for greedy in (False, True):
        act, lp, ent = rig.run(masks, raw, dtype, 4100, draw=3, greedy=greedy)
        bad = kind >= 2
        assert (act[bad] == P.NONE).all() and np.isnan(lp[bad]).all() and np.isnan(ent[bad]).all()
        ok = (kind < 2) & (np.arange(N) % 9 != 0)
        assert (act[ok] < 4100).all() and np.isfinite(lp[ok]).all() and np.isfinite(ent[ok]).all()
        assert np.isfinite(val[np.flatnonzero(ok), act[ok]]).all()  # never a -inf one
        if not greedy:
            P.check_sampler(act, lp, ent, val, masks, 1.0, us[3])
        else:
            for i in np.flatnonzero(ok):
                acts = P.legal_actions(masks[i])
                assert act[i] == acts[P.ref_greedy(val[i], masks[i], 1.0)[0]]


# --------------------------------------------------------------------------- 4. the random stream
def test_random_stream(rig, masks):
    raw, val = P.synthetic_logits(N, 4100, "float32", 2)
    a0 = rig.run(masks, raw, "float32", 4100, draw=5)
    a1 = rig.run(masks, raw, "float32", 4100, draw=5)
    assert same_bits(a0, a1)
    b = rig.run(masks, raw, "float32", 4100, draw=6)
    multi = np.array([P.legal_actions(m).size >= 40 for m in masks])
    assert multi.sum() >= 80 and (a0[0][multi] != b[0][multi]).mean() > 0.8
    c = rig.run(masks, raw, "float32", 4100, draw=5, seed=SEED + 1)
    assert (a0[0][multi] != c[0][multi]).mean() > 0.8
    # the env's seed is the default
    d = rig.run(masks, raw, "float32", 4100, draw=5, seed=SEED)
    assert same_bits(a0, d)


def test_board_result_does_not_depend_on_n(rig, masks):
    """boards 0..63 inside N = 64 (packed mask) and inside N = 200 (stride 256)"""
    raw, val = P.synthetic_logits(N, 4101, "bfloat16", 2)
    big = rig.run(masks, raw, "bfloat16", 4101, draw=7)
    r = Rig(64, 64)
    small = r.run(masks[:64], raw[:64], "bfloat16", 4101, draw=7)
    assert same_bits([o[:64] for o in big], small)
    r.env.close()


def test_explicit_action_buffer_and_no_policy_buffers(masks):
    """action= a caller's buffer; an io without logprob / entropy"""
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(N, device=0, seed=SEED)
    io = env.device_io(obs=False, count=False, select=False, mask_stride=STRIDE)
    assert "logprob" not in io.ptr and "entropy" not in io.ptr
    upload_mask(env, io, masks)
    raw, val = P.synthetic_logits(N, 4100, "float32", 2)
    buf, out = Dev(env, raw), Dev(env, np.zeros(N, dtype=np.uint16))
    env.sample_policy(io, buf.ptr, action=out.ptr)
    got = np.zeros(N, dtype=np.uint16)
    _lib.check(env._L.gc_env_copy(env._h, _lib.ptr(got), out.ptr, ctypes.c_uint64(got.nbytes), 2))
    u = P.uniform(SEED, np.arange(N), 0)
    for i in range(N):
        j, _, _, C, acts = P.ref_sample(val[i], masks[i], 1.0, u[i])
        if acts.size == 0:
            assert got[i] == P.NONE
        else:
            k = int(np.searchsorted(acts, got[i]))
            assert acts[k] == got[i] and P.accepted(k, C, u[i])
    env.close()


# --------------------------------------------------------------------------- 5. end to end
def _host_mask(env):
    from gym_chess_amd import _lib

    raw = np.zeros((env.num_boards, 65), dtype=np.uint64)
    cnt = np.zeros(env.num_boards, dtype=np.int32)
    _lib.check(env._L.gc_env_legal_mask(env._h, _lib.ptr(raw), _lib.ptr(cnt)))
    return raw


def _loop(opponent, seed, iters=200, n=256):
    """The policy loop.  The env's rules have positions with no legal move that are not done
    (a stalemate; about one per run here): the sampler answers 0xFFFF there and a step of that
    would be an invalid action, so -- as the library's own self-play driver does -- such a board
    is reset without a step, and the io mask is refreshed for it, before the next sample."""
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(n, device=0, seed=seed, opponent=opponent)
    io = env.device_io(select=False, policy=True)
    mask = _host_mask(env)
    upload_mask(env, io, mask)
    logits = Dev(env, P.quantise(np.random.RandomState(21).uniform(-8, 8, size=(n, 4100)).astype(np.float32),
                                 "bfloat16")[0])
    trace = []
    resets = 0
    for it in range(iters):
        env.sample_policy(io, logits.ptr, dtype="bfloat16", draw=it)
        act = io.fetch("pick")["pick"]
        env.step_device(io, autoreset=True)
        o = io.fetch("reward", "done", "reason", "mask", "count", "logprob")
        assert not np.isin(o["reason"], (6, 7)).any(), (it, o["reason"][np.isin(o["reason"], (6, 7))])
        assert (act < 4100).all(), it
        word = mask[np.arange(n), act >> 6]
        assert ((word >> (act & 63).astype(np.uint64)) & np.uint64(1)).all(), it
        assert np.isfinite(o["logprob"]).all() and (o["logprob"] <= 0).all()
        trace.append((act, o["reward"], o["done"]))
        mask = o["mask"]
        stuck = o["count"] == 0
        if stuck.any():
            resets += int(stuck.sum())
            env.reset(stuck.astype(np.uint8))
            mask[stuck] = _host_mask(env)[stuck]
            upload_mask(env, io, mask)
    assert resets <= iters * n // 1000  # rare
    env.close()
    return [np.stack(t) for t in zip(*trace)]


@pytest.mark.parametrize("opponent", ["none", "random"])
def test_sample_then_step_loop(opponent):
    """200 x (sample_policy -> step_device(autoreset)) on N = 256: never an invalid action or a
    step after done, every action set in the mask it was sampled from, reproducible, and
    another seed plays another game"""
    a = _loop(opponent, 31)
    b = _loop(opponent, 31)
    assert all((x == y).all() for x, y in zip(a, b))
    c = _loop(opponent, 32)
    assert (a[0] != c[0]).any()
    assert a[2].any()  # games ended and were reset inside the loop


# --------------------------------------------------------------------------- 6. argument errors
def test_argument_errors(rig, masks):
    from gym_chess_amd import _lib

    raw, _ = P.synthetic_logits(N, 4100, "float32", 2)
    buf = Dev(rig.env, raw)
    e, p = rig.env, rig.io.ptr

    def call(logits=buf.ptr, dtype=0, row_stride=4100, mask=p["mask"], mask_stride=STRIDE, T=1.0, action=p["pick"]):
        _lib.check(e._L.gc_env_sample_policy(e._h, logits, dtype, row_stride, mask, mask_stride, T,
                                             ctypes.c_uint64(1), 0, 0, action, None, None))

    call()  # the baseline is fine (log-prob and entropy are optional)
    call(mask_stride=N)
    for kw in (dict(row_stride=4099), dict(dtype=3), dict(dtype=-1), dict(T=0.0), dict(T=-1.0), dict(T=float("nan")),
               dict(T=float("inf")), dict(mask_stride=N - 1), dict(logits=None), dict(mask=None), dict(action=None)):
        with pytest.raises(_lib.GymChessError) as ei:
            call(**kw)
        assert str(ei.value), kw
    with pytest.raises(ValueError):
        e.sample_policy(rig.io, buf.ptr, dtype="float64")
    e.synchronize()
    buf.close()
