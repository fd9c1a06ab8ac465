"""CPU: the reference of the device legal-move priors (gc_env_policy_priors) and the acceptance
rule its GPU tests use -- restated in numpy, and shown here to be neither vacuous nor too tight.

Per row: legal actions a_1 < ... < a_m = the board's mask bits in action-id order, x_k =
logit[a_k] / T (read at mirror(a_k) on a mirrored board), p = softmax(x) over all m; the first
min(m, cap) of them are written, the other slots hold the padding 0xFFFF / 0.0 / 0xFFFF.

Rule: actions, count, logit indices and padding exact; a legal -inf gives exactly 0; unusable rows
(a legal NaN, every legal logit -inf) are NaN in every written prior; otherwise
|p - p_ref| <= eps(m) * p_ref with the project's eps(m) = 2e-5 + m * 2^-23 (test_policy_sample):
rounding of logit / T, of x - max and of expf is below 1e-5 relative for |x| <= 16, the range the
test logits stay in (checked below), plus m fp32 additions in S.  The bound is relative, so it
does not go vacuous at m = 4100.
"""
import ctypes

import numpy as np
import pytest

import test_policy_sample as P

PAD = 0xFFFF
CAPS = (1, 64, 65, 320, 4100)


def mirror(a):
    """where the logit of action a sits in a side-to-move-relative row of a BLACK-to-move board:
    from and to each ^ 56, the castles' colours swapped (gc_policy.h pol_mirror)"""
    a = np.asarray(a, dtype=np.int64)
    return np.where(a < 4096, a ^ 0xE38, 4096 + ((a - 4096) ^ 2))


# ----------------------------------------------------------------------------- reference + rule
def ref_priors(logits_row, mask65, T, cap, mirrored=False):
    """float64 reference of one row: logits_row = the row's exact values, T the temperature as the
    kernel gets it (a float32) -> (actions u16[cap], priors f64[cap], count, logit_idx u16[cap])"""
    acts = P.legal_actions(mask65)
    m = int(acts.size)
    w = min(m, cap)
    actions = np.full(cap, PAD, dtype=np.uint16)
    priors = np.zeros(cap, dtype=np.float64)
    lidx = np.full(cap, PAD, dtype=np.uint16)
    if m == 0:
        return actions, priors, 0, lidx
    at = mirror(acts) if mirrored else acts
    actions[:w] = acts[:w]
    lidx[:w] = at[:w]
    x = np.asarray(logits_row, dtype=np.float64)[at] / np.float64(np.float32(T))
    if np.isnan(x).any() or x.max() == -np.inf:
        priors[:w] = np.nan
        return actions, priors, m, lidx
    mx = x.max()
    with np.errstate(invalid="ignore"):
        d = np.where(x == mx, 0.0, x - mx)
    e = np.exp(d)
    priors[:w] = (e / e.sum())[:w]
    return actions, priors, m, lidx


def accepted(priors, ref, m, cap):
    """the rule for one row's priors against the reference's"""
    w = min(m, cap)
    got, want = np.asarray(priors, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not (got[w:] == 0.0).all():
        return False
    if np.isnan(want[:w]).any():
        return bool(np.isnan(got[:w]).all())
    if np.isnan(got[:w]).any() or not (got[:w][want[:w] == 0.0] == 0.0).all():
        return False
    return bool((np.abs(got[:w] - want[:w]) <= P.eps(m) * want[:w]).all())


def check_row(actions, priors, count, lidx, logits_row, mask65, T, cap, mirrored=False, dead=False):
    """one row of an implementation's output against the reference (lidx None = not produced)"""
    ra, rp, rm, rl = ref_priors(logits_row, np.zeros(65, dtype=np.uint64) if dead else mask65, T, cap, mirrored)
    assert count == (-1 if dead else rm), (count, rm, dead)
    assert (np.asarray(actions) == ra).all(), (actions[:8], ra[:8])
    if lidx is not None:
        assert (np.asarray(lidx) == rl).all(), (lidx[:8], rl[:8])
    assert accepted(priors, rp, rm, cap), (rm, cap, np.asarray(priors)[:4], rp[:4])
    return rp


# ----------------------------------------------------------------------------- fp32 restatements
def f32_priors(logits_row, mask65, T, cap, order, mirrored=False):
    """the same maths in float32 (what a kernel does), the sum in the given order: 'forward' (a
    running sum), 'pairwise' (numpy's) or 'lanes' (64 strided partial sums, then their sum)"""
    f = np.float32
    acts = P.legal_actions(mask65)
    out = np.zeros(cap, dtype=f)
    if acts.size == 0:
        return out
    at = mirror(acts) if mirrored else acts
    x = np.asarray(logits_row)[at].astype(f) / f(T)
    e = np.exp((x - x.max()).astype(f)).astype(f)
    if order == "forward":
        S = np.cumsum(e, dtype=f)[-1]
    elif order == "pairwise":
        S = e.sum(dtype=f)
    else:
        part = np.zeros(64, dtype=f)
        for k in range(e.size):
            part[k & 63] = f(part[k & 63] + e[k])
        S = part.sum(dtype=f)
    w = min(acts.size, cap)
    out[:w] = (e * (f(1) / S))[:w]
    return out


# three wrong implementations, each in float32 ('lanes'), as a kernel with that bug would compute
def wrong_first_cap_only(logits_row, mask65, T, cap, mirrored=False):
    """normalises over the cap entries it writes instead of all m"""
    acts = P.legal_actions(mask65)[:cap]
    return f32_priors(logits_row, P.mask_from_actions([int(a) for a in acts]), T, cap, "lanes", mirrored)


def wrong_shifted(logits_row, mask65, T, cap, mirrored=False):
    """slot k holds the prior of action k + 1 (the last one wraps)"""
    m = P.legal_actions(mask65).size
    p = f32_priors(logits_row, mask65, T, max(m, 1), "lanes", mirrored)
    out = np.zeros(cap, dtype=np.float32)
    w = min(m, cap)
    out[:w] = np.roll(p[:m], -1)[:w]
    return out


def wrong_unmirrored(logits_row, mask65, T, cap, mirrored=False):
    return f32_priors(logits_row, mask65, T, cap, "lanes", False)


def differs(priors, ref, m, cap):
    """Does a wrong result differ from the reference at all, as far as fp32 can tell?  An error
    below the fp32 noise of a correct kernel (the rule's eps, by its derivation) cannot be refused
    by any rule that accepts correct fp32 kernels: the 65th action of a row with e_65 / S < 2e-5
    changes S by less than the order of summation does.  So a row counts as differing when some
    written entry is off by more than 2 eps(m) relative (or in its zeros / NaNs)."""
    w = min(m, cap)
    got, want = np.asarray(priors, dtype=np.float64)[:w], np.asarray(ref, dtype=np.float64)[:w]
    if np.isnan(want).any() or np.isnan(got).any():
        return bool((np.isnan(want) != np.isnan(got)).any())
    return bool((np.abs(got - want) > 2 * P.eps(m) * want).any())


# ----------------------------------------------------------------------------- tests
def test_mirror_is_an_involution():
    a = np.arange(4100)
    assert (mirror(mirror(a)) == a).all() and sorted(mirror(a).tolist()) == a.tolist()
    assert (mirror(a[:4096]) == (a[:4096] ^ 0xE38)).all()
    assert mirror(np.array([4096, 4097, 4098, 4099])).tolist() == [4098, 4099, 4096, 4097]
    # from and to each ^ 56: e2e4 (52 -> 36) becomes e7e5 (12 -> 28)
    assert int(mirror(52 * 64 + 36)) == 12 * 64 + 28


def test_reference_on_hand_cases():
    mask = P.mask_from_actions([5, 70, 4097])
    row = np.zeros(4100)
    row[[5, 70, 4097]] = np.log([1.0, 2.0, 1.0])
    a, p, m, li = ref_priors(row, mask, 1.0, 8)
    assert m == 3 and a.tolist() == [5, 70, 4097] + [PAD] * 5 and li.tolist() == a.tolist()
    assert np.allclose(p[:3], [0.25, 0.5, 0.25], rtol=0, atol=1e-15) and (p[3:] == 0).all()
    # temperature 0.5 squares the odds: 1/6, 4/6, 1/6
    a, p, m, _ = ref_priors(row, mask, 0.5, 8)
    assert np.allclose(p[:3], [1 / 6, 4 / 6, 1 / 6], rtol=0, atol=1e-15)
    # cap below m: the entries written are still normalised over all m
    a, p, m, li = ref_priors(row, mask, 1.0, 2)
    assert m == 3 and a.tolist() == [5, 70] and np.allclose(p, [0.25, 0.5], rtol=0, atol=1e-15)
    # a mirrored board reads elsewhere, the actions stay absolute
    row2 = np.full(4100, np.nan)
    row2[mirror(np.array([5, 70, 4097]))] = np.log([1.0, 2.0, 1.0])
    a, p, m, li = ref_priors(row2, mask, 1.0, 4, mirrored=True)
    assert a.tolist() == [5, 70, 4097, PAD] and li.tolist() == [5 ^ 0xE38, 70 ^ 0xE38, 4099, PAD]
    assert np.allclose(p[:3], [0.25, 0.5, 0.25], rtol=0, atol=1e-15)
    # a legal -inf is exactly 0; illegal entries are never looked at
    row3 = np.full(4100, np.nan)
    row3[[5, 70, 4097]] = [-np.inf, 0.0, -np.inf]
    a, p, m, _ = ref_priors(row3, mask, 1.0, 4)
    assert p.tolist() == [0.0, 1.0, 0.0, 0.0] and m == 3
    # every legal logit -inf, or a legal NaN: the actions, count = m, NaN priors, exact padding
    for v in (-np.inf, np.nan):
        row3[70] = v
        a, p, m, _ = ref_priors(row3, mask, 1.0, 4)
        assert m == 3 and a.tolist() == [5, 70, 4097, PAD] and np.isnan(p[:3]).all() and p[3] == 0.0
    # no legal action
    a, p, m, li = ref_priors(row, np.zeros(65, dtype=np.uint64), 1.0, 3)
    assert m == 0 and a.tolist() == [PAD] * 3 and p.tolist() == [0.0] * 3 and li.tolist() == [PAD] * 3


def test_truncation_m65_cap64():
    mask = P.synthetic_masks(9, 4)[3]  # the "exactly65" family
    acts = P.legal_actions(mask)
    assert acts.size == 65
    _, val = P.synthetic_logits(1, 4100, "float32", 5)
    a, p, m, li = ref_priors(val[0], mask, 1.0, 64)
    full = ref_priors(val[0], mask, 1.0, 65)[1]
    assert m == 65 and a.tolist() == acts[:64].tolist() and (p == full[:64]).all()
    assert abs(p.sum() + full[64] - 1.0) < 1e-12 and p.sum() < 1.0
    for order in ("forward", "pairwise", "lanes"):
        assert accepted(f32_priors(val[0], mask, 1.0, 64, order), p, 65, 64)
    # the rule's own edges: a wrong padding slot, a NaN, a non-zero where the reference is 0
    good = f32_priors(val[0], mask, 1.0, 64, "lanes")
    assert not accepted(np.where(np.arange(64) == 10, np.nan, good), p, 65, 64)
    assert not accepted(good * np.float32(1.0001), p, 65, 64)
    assert not accepted(np.append(good[:63], 0.0), p, 65, 64)


@pytest.fixture(scope="module")
def inputs():
    """the GPU tests' inputs: N = 200, masks seed 1, logits seed 2, every dtype (exact values)"""
    masks = P.synthetic_masks(200, 1)
    return masks, {d: P.synthetic_logits(200, 4100, d, 2)[1] for d in P.DTYPES}


def test_inputs_stay_inside_the_derivation(inputs):
    """|logit / T| <= 16 at every temperature the tests use, every family present"""
    masks, vals = inputs
    for d in P.DTYPES:
        for T in (1.0, 0.8, 0.5):
            assert np.abs(vals[d]).max() / np.float32(T) <= 16.0
    _, v3 = P.synthetic_logits(200, 4104, "bfloat16", 3)
    assert np.abs(v3).max() / np.float32(0.8) <= 16.0
    ms = {int(P.legal_actions(m).size) for m in masks}
    assert {0, 1, 64, 65, 4100} <= ms and max(ms) == 4100
    assert P.eps(4100) < 6e-4  # relative: still a real bound on the longest list


def test_rule_is_not_too_tight(inputs):
    """float32 restatements in three summation orders pass on every row, every dtype, and a
    truncating cap; mirrored odd rows too"""
    masks, vals = inputs
    for d in P.DTYPES:
        for order in ("forward", "pairwise", "lanes"):
            for i in range(200):
                m = int(P.legal_actions(masks[i]).size)
                for cap in (64, 4100) if order == "lanes" else (64,):
                    for mir in (False, True) if i % 2 else (False,):
                        ref = ref_priors(vals[d][i], masks[i], 1.0, cap, mir)[1]
                        got = f32_priors(vals[d][i], masks[i], 1.0, cap, order, mir)
                        assert accepted(got, ref, m, cap), (d, order, i, m, cap, mir)


def test_rule_is_not_vacuous(inputs):
    """three wrong implementations are each refused on >= 99 % of the rows where they differ
    from the reference (differs(): beyond fp32 noise); each differs on most rows it can touch"""
    masks, vals = inputs
    cap = 64
    tally = {}
    for name, wrong, mir in (("first_cap_only", wrong_first_cap_only, False), ("shifted", wrong_shifted, False),
                             ("unmirrored", wrong_unmirrored, True)):
        rows = diff = refused = 0
        for d in P.DTYPES:
            for i in range(200):
                m = int(P.legal_actions(masks[i]).size)
                if name == "first_cap_only" and m <= cap:
                    continue
                if name == "unmirrored" and not (i % 2 and m >= 2):
                    continue
                if m < 2:
                    continue
                rows += 1
                ref = ref_priors(vals[d][i], masks[i], 1.0, cap, mir)[1]
                got = wrong(vals[d][i], masks[i], 1.0, cap, mir)
                if differs(got, ref, m, cap):
                    diff += 1
                    refused += not accepted(got, ref, m, cap)
        tally[name] = (rows, diff, refused)
        print(f"{name}: {rows} rows, differs on {diff}, refused on {refused}")
        assert refused >= 0.99 * diff, (name, rows, diff, refused)
    # the first wrong one drops the 65th of 65 actions (a real difference on the rows where that
    # action carries more than fp32 noise) or 4036 of 4100 (always)
    assert tally["first_cap_only"][0] == 3 * 44 and tally["first_cap_only"][1] >= 3 * 22 + 20
    assert tally["shifted"][1] >= 0.95 * tally["shifted"][0] >= 300
    assert tally["unmirrored"][1] >= 0.95 * tally["unmirrored"][0] >= 150


# ----------------------------------------------------------------------------- the ABI, no GPU
def test_symbol_is_exported_and_bound():
    from gym_chess_amd import _lib

    assert "gc_env_policy_priors" in _lib.SIGNATURES
    L = _lib.load()
    fn = L.gc_env_policy_priors
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    rc = fn(None, None, 0, 4100, None, 0, None, 0, 1.0, 0, 64, None, None, None, None)
    assert rc != 0
    assert L.gc_last_error()
    from gym_chess_amd.env import BatchedChessEnv, PriorsBuffer  # noqa: F401

    assert callable(BatchedChessEnv.policy_priors) and callable(BatchedChessEnv.priors_buffer)
