"""GPU: the device legal-move priors (gc_env_policy_priors / BatchedChessEnv.policy_priors) against
the float64 reference and acceptance rule of test_policy_priors.py: synthetic masks (one family per
way the mapping can go wrong), the three logit types, every cap that takes another path, the board
index, the side-to-move view, poisoned entries, the sampler's log-probs, placement, the step loop
and argument errors.  Buffers come from gc_device_alloc / gc_env_copy; bf16 / fp16 logits are
quantised in numpy and the reference reads those values."""
import ctypes

import numpy as np
import pytest

import test_policy_priors as R
import test_policy_sample as P

pytestmark = pytest.mark.gpu

N, STRIDE, SEED = 200, 256, 11
PAD = R.PAD


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


def prefill(env, buf):
    """every byte of a priors buffer 0xAB, so a slot the kernel skips shows"""
    from gym_chess_amd import _lib

    for k, p in buf.ptr.items():
        junk = np.full(buf._shape(k)[1], 0xAB, dtype=np.uint8)
        if junk.size:
            _lib.check(env._L.gc_env_copy(env._h, p, _lib.ptr(junk), ctypes.c_uint64(junk.nbytes), 1))


class Rig:
    """an env of n boards, its io (mask stride as given) and one policy_priors call"""

    def __init__(self, n, mask_stride, seed=SEED):
        from gym_chess_amd.env import BatchedChessEnv

        self.n = n
        self.env = BatchedChessEnv(n, device=0, seed=seed)
        self.io = self.env.device_io(obs=False, count=False, select=False, mask_stride=mask_stride, policy=True)
        self.masks = None

    def set_masks(self, masks):
        if self.masks is not masks:
            upload_mask(self.env, self.io, masks)
            self.masks = masks

    def run(self, masks, raw, dtype, row_stride, cap=64, boards=None, rows=None, **kw):
        self.set_masks(masks)
        buf = Dev(self.env, raw)
        nrows = (len(boards) if boards is not None else self.n) if rows is None else rows
        out = self.env.priors_buffer(nrows, cap=cap, logit_index=True)
        prefill(self.env, out)
        self.env.policy_priors(self.io, buf.ptr, out, boards=boards, rows=rows, dtype=dtype, row_stride=row_stride,
                               **kw)
        o = out.fetch()
        out.close()
        buf.close()
        return o["actions"], o["priors"], o["count"], o["logit_index"]


@pytest.fixture(scope="module")
def rig():
    return Rig(N, STRIDE)


@pytest.fixture(scope="module")
def masks():
    return P.synthetic_masks(N, 1)


@pytest.fixture(scope="module")
def logits():
    """(raw, exact values) per (dtype, row_stride), seed 2: computed once, never changed"""
    return {(d, s): P.synthetic_logits(N, s, d, 2) for d in P.DTYPES for s in (4100, 4101, 4104)}


@pytest.fixture(scope="module")
def refs(masks, logits):
    """the float64 reference at cap 4100 per (dtype, row stride) -- the seeded draw depends on the
    stride --, computed once; a smaller cap is a prefix of it"""
    return {k: [R.ref_priors(v[1][i], masks[i], 1.0, 4100) for i in range(N)] for k, v in logits.items()}


def same_bits(a, b):
    def raw(x):
        return np.atleast_1d(x).view(np.uint8)

    return all(np.shape(x) == np.shape(y) and (raw(x) == raw(y)).all() for x, y in zip(a, b))


def check_against(ref_row, act, pri, cnt, lidx, cap, mirror_row=False):
    """one output row against its cap-4100 reference (actions, priors, count, logit index)"""
    ra, rp, m, rl = ref_row
    w = min(m, cap)
    assert cnt == m
    assert (act[:w] == ra[:w]).all() and (act[w:] == PAD).all()
    want_l = R.mirror(ra[:w].astype(np.int64)) if mirror_row else rl[:w]
    assert (lidx[:w] == want_l).all() and (lidx[w:] == PAD).all()
    assert R.accepted(pri, np.concatenate([rp[:w], np.zeros(cap - w)]), m, cap), (m, cap, pri[:4], rp[:4])
    if m and not np.isnan(rp[:w]).any():
        s, want = float(pri[:w].astype(np.float64).sum()), float(rp[:w].sum())
        assert abs(s - want) <= P.eps(m) * max(want, 1e-300) + 1e-300, (s, want, m)


# --------------------------------------------------------------------------- 1. synthetic masks
@pytest.mark.parametrize("cap", R.CAPS)
@pytest.mark.parametrize("row_stride", [4100, 4101, 4104])
@pytest.mark.parametrize("dtype", P.DTYPES)
def test_synthetic_masks(rig, masks, logits, refs, dtype, row_stride, cap):
    """N = 200 (12 tiles plus a ragged 8), mask stride 256, every mask family: the rule on every
    row, the padding fully written over the 0xAB pre-fill, the written priors' sum"""
    raw, _ = logits[dtype, row_stride]
    act, pri, cnt, lidx = rig.run(masks, raw, dtype, row_stride, cap=cap)
    assert act.shape == (N, cap) and pri.shape == (N, cap) and cnt.shape == (N,)
    for i in range(N):
        check_against(refs[dtype, row_stride][i], act[i], pri[i], cnt[i], lidx[i], cap)


def test_temperature(rig, masks):
    T = np.float32(0.8)
    raw, val = P.synthetic_logits(N, 4104, "bfloat16", 3)
    act, pri, cnt, lidx = rig.run(masks, raw, "bfloat16", 4104, cap=64, temperature=float(T))
    for i in range(N):
        R.check_row(act[i], pri[i], cnt[i], lidx[i], val[i], masks[i], T, 64)


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_one_board_packed_stride(dtype):
    """N = 1, mask stride = N, every family"""
    r = Rig(1, 1, seed=5)
    fam = P.synthetic_masks(9, 4)
    for f in range(9):
        raw, val = P.synthetic_logits(1, 4101, dtype, 6 + f)
        for cap in (64, 4100):
            act, pri, cnt, lidx = r.run(fam[f: f + 1], raw, dtype, 4101, cap=cap)
            R.check_row(act[0], pri[0], cnt[0], lidx[0], val[0], fam[f], 1.0, cap)
    r.env.close()


# --------------------------------------------------------------------------- 2. the board index
def board_index():
    """37 rows over the N = 200 env: a shuffled subset with duplicates, and three entries out of
    range"""
    rs = np.random.RandomState(13)
    idx = rs.permutation(N)[:30].tolist() + [4, 4, 13, 199]  # 4 = the 4100-action family, 13 again
    idx = [int(v) for v in idx]
    idx[3] = idx[0]
    idx[5], idx[17], idx[29] = -1, 200, 2 ** 31 - 1
    idx += [0, 3, 198]
    assert len(idx) == 37
    return np.array(idx, dtype=np.int64)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_board_index(rig, masks, logits, dtype):
    """row j = board idx[j]'s legal list with logits row j: bit for bit the identity run's row of
    that board (given the same logits row); out-of-range entries give count -1 and padding"""
    idx = board_index()
    raw, val = logits[dtype, 4101]
    dead = (idx < 0) | (idx >= N)
    safe = np.where(dead, 0, idx)
    ident = rig.run(masks, raw, dtype, 4101, cap=65)
    got = rig.run(masks, raw[safe], dtype, 4101, cap=65, boards=idx)  # row j brings its board's logits
    act, pri, cnt, lidx = got
    assert act.shape == (37, 65)
    assert (cnt[dead] == -1).all() and (act[dead] == PAD).all() and (pri[dead] == 0).all() and (lidx[dead] == PAD).all()
    assert dead.sum() == 3
    for j in np.flatnonzero(~dead):
        assert same_bits([o[j] for o in got], [o[idx[j]] for o in ident]), (j, int(idx[j]))
        R.check_row(act[j], pri[j], cnt[j], lidx[j], val[idx[j]], masks[idx[j]], 1.0, 65)


def test_board_index_with_more_rows_than_boards(rig, masks):
    """400 rows of indices mod 200, as a device pointer"""
    rows = 400
    idx = np.arange(rows, dtype=np.int32) % N
    raw, val = P.synthetic_logits(rows, 4100, "float16", 17)
    d_idx = Dev(rig.env, idx)
    act, pri, cnt, lidx = rig.run(masks, raw, "float16", 4100, cap=64, boards=d_idx.ptr, rows=rows)
    d_idx.close()
    for j in range(rows):
        R.check_row(act[j], pri[j], cnt[j], lidx[j], val[j], masks[idx[j]], 1.0, 64)


# --------------------------------------------------------------------------- 3. the relative view
@pytest.fixture(scope="module")
def black_rig(masks):
    """odd boards have BLACK to move (the masks stay the synthetic ones: only the side is read)"""
    r = Rig(N, STRIDE)
    b, m = r.env.boards()
    m = m.copy()
    m[1::2, 0] = 0
    r.env.set_states(b, m)
    assert (r.env.boards()[1][:, 0] == np.arange(N) % 2 ^ 1).all()
    return r


def mirrored_rows(val_or_raw, odd_rows):
    """row i's elements 0..4099 permuted by the mirror on the given rows: M[i, a] = L[i, mirror(a)]"""
    out = val_or_raw.copy()
    perm = R.mirror(np.arange(4100))
    for i in np.flatnonzero(odd_rows):
        out[i, :4100] = val_or_raw[i, perm]
    return out


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_relative(black_rig, masks, logits, dtype):
    """relative=True on L == relative=False on L mirrored in numpy on the odd rows, bit for bit in
    priors and actions; logit_index = a on even rows, mirror(a) on odd rows"""
    raw, val = logits[dtype, 4104]
    odd = np.arange(N) % 2 == 1
    rel = black_rig.run(masks, raw, dtype, 4104, cap=65, relative=True)
    ab = black_rig.run(masks, mirrored_rows(raw, odd), dtype, 4104, cap=65, relative=False)
    assert same_bits(rel[:3], ab[:3])
    act, pri, cnt, lidx = rel
    for i in range(N):
        R.check_row(act[i], pri[i], cnt[i], lidx[i], val[i], masks[i], 1.0, 65, mirrored=bool(odd[i]))
        w = min(int(cnt[i]), 65)
        a = act[i, :w].astype(np.int64)
        assert (lidx[i, :w] == (R.mirror(a) if odd[i] else a)).all()
    # without the flag the env's state is not read
    plain = black_rig.run(masks, raw, dtype, 4104, cap=65)
    assert (plain[3][plain[0] != PAD] == plain[0][plain[0] != PAD]).all()


def test_relative_with_board_index(black_rig, masks, logits):
    idx = board_index()
    dead = (idx < 0) | (idx >= N)
    raw, val = logits["bfloat16", 4100]
    rows = len(idx)
    odd = (idx % 2 == 1) & ~dead
    rel = black_rig.run(masks, raw[:rows], "bfloat16", 4100, cap=64, boards=idx, relative=True)
    ab = black_rig.run(masks, mirrored_rows(raw[:rows], odd), "bfloat16", 4100, cap=64, boards=idx)
    assert same_bits(rel[:3], ab[:3])
    act, pri, cnt, lidx = rel
    assert (cnt[dead] == -1).all() and (act[dead] == PAD).all() and (pri[dead] == 0).all()
    for j in np.flatnonzero(~dead):
        R.check_row(act[j], pri[j], cnt[j], lidx[j], val[j], masks[idx[j]], 1.0, 64, mirrored=bool(odd[j]))


# --------------------------------------------------------------------------- 4. poisoned entries
def test_illegal_logits_are_never_used(rig, masks):
    """every illegal logit NaN: bit-identical outputs, all three types"""
    for dtype in P.DTYPES:
        x = np.random.RandomState(8).uniform(-8.0, 8.0, size=(N, 4101)).astype(np.float32)
        y = np.full_like(x, np.nan)
        for i in range(N):
            a = P.legal_actions(masks[i])
            y[i, a] = x[i, a]
        clean = rig.run(masks, P.quantise(x, dtype)[0], dtype, 4101, cap=4100)
        poisoned = rig.run(masks, P.quantise(y, dtype)[0], dtype, 4101, cap=4100)
        assert same_bits(clean, poisoned), dtype
        assert not np.isnan(poisoned[1]).any()


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_legal_minus_inf_and_unusable_rows(rig, masks, dtype):
    """a legal -inf has prior exactly 0 (and the rest still meets the rule); an all -inf row and a
    row with a legal NaN keep actions and count, with NaN in every written prior"""
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
    for cap in (64, 4100):
        act, pri, cnt, lidx = rig.run(masks, raw, dtype, 4100, cap=cap)
        for i in range(N):
            R.check_row(act[i], pri[i], cnt[i], lidx[i], val[i], masks[i], 1.0, cap)
            a = P.legal_actions(masks[i])
            w = min(a.size, cap)
            if kind[i] >= 2:
                assert cnt[i] == a.size and (act[i, :w] == a[:w]).all() and np.isnan(pri[i, :w]).all()
                assert (pri[i, w:] == 0).all()
            elif kind[i] == 1:
                assert (pri[i, :w][np.isinf(val[i, a[:w]])] == 0.0).all() and np.isfinite(pri[i]).all()


# --------------------------------------------------------------------------- 5. the sampler's maths
@pytest.mark.parametrize("dtype", P.DTYPES)
def test_consistency_with_the_sampler(rig, masks, logits, dtype):
    """sample_policy chose a_i with log-prob lp_i on the same inputs: the prior written for a_i is
    exp(lp_i) within 4 eps(m) relative"""
    raw, _ = logits[dtype, 4101]
    act, pri, cnt, _ = rig.run(masks, raw, dtype, 4101, cap=4100)
    buf = Dev(rig.env, raw)
    rig.env.sample_policy(rig.io, buf.ptr, dtype=dtype, row_stride=4101, draw=3)
    o = rig.io.fetch("pick", "logprob")
    buf.close()
    tried = 0
    for i in range(N):
        if cnt[i] == 0:
            assert o["pick"][i] == P.NONE
            continue
        k = int(np.searchsorted(act[i, : cnt[i]], o["pick"][i]))
        assert act[i, k] == o["pick"][i]
        want = np.exp(np.float64(o["logprob"][i]))
        assert abs(float(pri[i, k]) - want) <= 4 * P.eps(int(cnt[i])) * want, (i, pri[i, k], want)
        tried += 1
    assert tried >= 170


# --------------------------------------------------------------------------- 6. placement
def test_rows_do_not_depend_on_n_or_on_the_run(rig, masks, logits):
    """rows 0..63 inside N = 64 (packed mask) and inside N = 200 (stride 256); the same call twice"""
    raw, _ = logits["bfloat16", 4101]
    big = rig.run(masks, raw, "bfloat16", 4101, cap=320)
    again = rig.run(masks, raw, "bfloat16", 4101, cap=320)
    assert same_bits(big, again)
    r = Rig(64, 64)
    small = r.run(masks[:64], raw[:64], "bfloat16", 4101, cap=320)
    assert same_bits([o[:64] for o in big], small)
    r.env.close()


# --------------------------------------------------------------------------- 7. end to end
def _host_lists(env):
    """per board the legal actions ascending, from env.legal_mask() unpacked on the host"""
    lm = env.legal_mask()
    return [np.flatnonzero(lm[i, :4100]) for i in range(env.num_boards)]


@pytest.mark.parametrize("opponent,rules", [("none", "reference"), ("random", "reference"), ("none", "fide")])
def test_end_to_end(opponent, rules):
    """n = 256, 40 x step_device(autoreset), then priors with bf16 random logits: count = io's
    count, the action lists = env.legal_mask() ascending, the priors meet the rule"""
    from gym_chess_amd.env import BatchedChessEnv

    n = 256
    env = BatchedChessEnv(n, device=0, seed=41, opponent=opponent, rules=rules)
    io = env.device_io()
    for _ in range(40):
        env.step_device(io, autoreset=True)
    raw, val = P.quantise(np.random.RandomState(21).uniform(-8, 8, size=(n, 4100)).astype(np.float32), "bfloat16")
    logits = Dev(env, raw)
    out = env.priors_buffer(n, cap=64, logit_index=True)
    prefill(env, out)
    env.policy_priors(io, logits.ptr, out, dtype="bfloat16")
    o, st = out.fetch(), io.fetch("count", "mask")
    lists = _host_lists(env)
    assert (o["count"] == st["count"]).all()
    assert np.median(o["count"]) >= 5  # real positions, not a batch of finished games
    for i in range(n):
        m = int(o["count"][i])
        assert m == lists[i].size and (o["actions"][i, : min(m, 64)] == lists[i][:64]).all()
        R.check_row(o["actions"][i], o["priors"][i], m, o["logit_index"][i], val[i], st["mask"][i], 1.0, 64)
    out.close()
    logits.close()
    env.close()


# --------------------------------------------------------------------------- 8. argument errors
def test_argument_errors(rig, masks):
    from gym_chess_amd import _lib

    rig.set_masks(masks)
    raw, _ = P.synthetic_logits(N, 4100, "float32", 2)
    buf = Dev(rig.env, raw)
    out = rig.env.priors_buffer(N, cap=64, logit_index=True)
    idx = Dev(rig.env, np.arange(N, dtype=np.int32))
    e, p, q = rig.env, rig.io.ptr, out.ptr

    def call(env=e._h, logits=buf.ptr, dtype=0, row_stride=4100, mask=p["mask"], mask_stride=STRIDE, boards=None,
             rows=N, T=1.0, flags=0, cap=64, actions=q["actions"], priors=q["priors"], count=q["count"],
             lidx=q["logit_index"]):
        _lib.check(e._L.gc_env_policy_priors(env, logits, dtype, row_stride, mask, mask_stride, boards, rows, T, flags,
                                             cap, actions, priors, count, lidx))

    call()  # the baseline is fine; count and the logit index are optional
    call(count=None, lidx=None)
    call(mask_stride=N, flags=2)
    call(rows=0)
    call(rows=0, boards=idx.ptr)
    call(boards=idx.ptr, rows=N)
    for kw in (dict(env=None), dict(logits=None), dict(mask=None), dict(actions=None), dict(priors=None),
               dict(dtype=3), dict(dtype=-1), dict(row_stride=4099), dict(mask_stride=N - 1), dict(T=0.0),
               dict(T=-1.0), dict(T=float("nan")), dict(T=float("inf")), dict(flags=1), dict(flags=3), dict(flags=4),
               dict(cap=0), dict(cap=4101), dict(rows=-1), dict(rows=N + 1)):
        with pytest.raises(_lib.GymChessError) as ei:
            call(**kw)
        assert str(ei.value), kw
    with pytest.raises(ValueError):
        e.policy_priors(rig.io, buf.ptr, out, dtype="float64")
    with pytest.raises(ValueError):
        e.policy_priors(rig.io, buf.ptr, out, rows=N + 1)
    with pytest.raises(ValueError):
        e.policy_priors(rig.io, buf.ptr, out, boards=np.arange(N + 1))
    with pytest.raises(ValueError):
        e.policy_priors(rig.io, buf.ptr, out, boards=idx.ptr)  # a device pointer needs rows
    nomask = e.device_io(mask=False, obs=False, count=False, pick=False)
    with pytest.raises(ValueError):
        e.policy_priors(nomask, buf.ptr, out)
    nomask.close()
    e.synchronize()
    for b in (buf, idx, out):
        b.close()
