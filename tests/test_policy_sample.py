"""CPU: the reference of the device policy head (gc_env_sample_policy) and the acceptance rule
its GPU tests use -- restated in numpy, and shown here to be neither vacuous nor too tight.

Per board: legal actions a_1 < ... < a_m = the mask's set bits in action-id order, x_k =
logit[a_k] / T, p = softmax(x), C = cumsum(p), u = (philox_x0(seed, board, draw) >> 8) * 2^-24;
the pick is the first k with u < C_k (the last k with p_k > 0 if rounding leaves none).

Acceptance (a kernel sums in fp32 in its own order): with eps(m) = 2e-5 + m * 2^-23 a pick a_j
is accepted iff C_{j-1} - eps <= u <= C_j + eps -- up to m fp32 additions at half an ulp each,
plus the per-term error of fp32 exp and of rounding x - max (< 1e-5 for |x| <= 16; the test
logits stay inside).  Log-prob within 4 eps(m); entropy within 16 eps(m) (H + 1 <= 9.4 with
margin).  On boards with m <= 64 an fp32 implementation may disagree with the float64 pick on at
most 2 * 64 * eps ~ 0.4 % of them: the tests cap it at 1 %.
"""
import numpy as np

N_MOVE_ACTIONS = 4100
NONE = 0xFFFF
DTYPES = ("float32", "float16", "bfloat16")
FAMILIES = ("empty", "single", "exactly64", "exactly65", "all", "castles", "full_word", "last_bit", "sparse")


# ----------------------------------------------------------------------------- the random stream
def philox_x0(seed, board, draw):
    """gc::philox_x0 (Philox4x32-10, key = seed, counter = {board, draw, 0x5EED, 0}), first word;
    board may be an array"""
    M = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    x0 = np.asarray(board, dtype=np.uint64) & M
    x1 = np.full_like(x0, draw & 0xFFFFFFFF)
    x2 = np.full_like(x0, 0x5EED)
    x3 = np.zeros_like(x0)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * x0
        p1 = np.uint64(0xCD9E8D57) * x2
        x0, x1, x2, x3 = (p1 >> s32) ^ x1 ^ k0, p1 & M, (p0 >> s32) ^ x3 ^ k1, p0 & M
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return x0.astype(np.uint32)


def uniform(seed, board, draw):
    """u in [0, 1): the top 24 bits of philox_x0, exact in fp32"""
    return (philox_x0(seed, board, draw) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


# ----------------------------------------------------------------------------- masks and logits
def legal_actions(mask65):
    """action ids of a board's mask words u64[65] (word f bit t = action f*64+t; word 64 bits
    0..3 = 4096..4099), ascending"""
    bits = np.unpackbits(np.ascontiguousarray(mask65[:64]).view(np.uint8), bitorder="little")
    castles = [4096 + c for c in range(4) if (int(mask65[64]) >> c) & 1]
    return np.concatenate([np.flatnonzero(bits), np.array(castles, dtype=np.int64)]).astype(np.int64)


def mask_from_actions(actions):
    m = np.zeros(65, dtype=np.uint64)
    for a in actions:
        m[a >> 6] |= np.uint64(1) << np.uint64(a & 63)
    return m


def synthetic_masks(n, seed):
    """board i's mask from family i % 9 (FAMILIES): every way the kernel's mapping can go wrong"""
    rng = np.random.RandomState(seed)
    out = np.zeros((n, 65), dtype=np.uint64)
    for i in range(n):
        fam = FAMILIES[i % len(FAMILIES)]
        if fam == "empty":
            acts = []
        elif fam == "single":
            acts = [rng.randint(N_MOVE_ACTIONS)]
        elif fam == "exactly64":
            acts = rng.choice(N_MOVE_ACTIONS, size=64, replace=False)
        elif fam == "exactly65":
            acts = rng.choice(N_MOVE_ACTIONS, size=65, replace=False)
        elif fam == "all":
            acts = range(N_MOVE_ACTIONS)
        elif fam == "castles":
            acts = [4096 + c for c in range(4) if (rng.randint(1, 16) >> c) & 1]
        elif fam == "full_word":
            f = rng.randint(64)
            acts = range(f * 64, f * 64 + 64)
        elif fam == "last_bit":
            acts = [4095]
        else:
            acts = rng.choice(N_MOVE_ACTIONS, size=rng.randint(1, 41), replace=False)
        out[i] = mask_from_actions([int(a) for a in acts])
    return out


def quantise(x, dtype):
    """float32 values -> (the raw elements as they sit in device memory, their exact values)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "float32":
        return x.copy(), x.astype(np.float64)
    if dtype == "float16":
        h = x.astype(np.float16)
        return h.view(np.uint16).copy(), h.astype(np.float64)
    assert dtype == "bfloat16"
    b = x.view(np.uint32)
    nan = np.isnan(x)
    r = ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    r[nan] = 0x7FC0
    return r, (r.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def synthetic_logits(n, row_stride, dtype, seed):
    """uniform in [-8, 8]; the row's padding (row_stride > 4100) is filled too"""
    rng = np.random.RandomState(seed)
    return quantise(rng.uniform(-8.0, 8.0, size=(n, row_stride)).astype(np.float32), dtype)


# ----------------------------------------------------------------------------- reference + rule
def eps(m):
    return 2e-5 + m * 2.0 ** -23


def ref_sample(logits, mask65, T, u):
    """float64 reference of one board: logits = the row's exact values, T the temperature as the
    kernel gets it (a float32).  -> (j, logprob, entropy, C, acts): j indexes acts; j = -1 with
    (0, 0) when there is no legal action, j = -1 with NaNs when the legal logits are unusable."""
    acts = legal_actions(mask65)
    if acts.size == 0:
        return -1, 0.0, 0.0, np.zeros(0), acts
    x = np.asarray(logits, dtype=np.float64)[acts] / np.float64(np.float32(T))
    if np.isnan(x).any() or x.max() == -np.inf:
        return -1, np.nan, np.nan, np.zeros(0), acts
    mx = x.max()
    with np.errstate(invalid="ignore"):
        d = np.where(x == mx, 0.0, x - mx)
    e = np.exp(d)
    S = e.sum()
    p = e / S
    C = np.cumsum(p)
    hit = np.flatnonzero(u < C)
    j = int(hit[0]) if hit.size else int(np.flatnonzero(p > 0)[-1])
    pos = p > 0
    H = float(-(p[pos] * np.log(p[pos])).sum())
    return j, float(d[j] - np.log(S)), H, C, acts


def ref_greedy(logits, mask65, T):
    """-> (j, logprob at T) of the largest x, ties to the lowest action id"""
    acts = legal_actions(mask65)
    x = np.asarray(logits, dtype=np.float64)[acts] / np.float64(np.float32(T))
    j = int(np.argmax(x))
    d = x - x[j]
    return j, float(-np.log(np.exp(d).sum()))


def accepted(j, C, u):
    """the acceptance rule for the pick acts[j] against the float64 cumulative C"""
    e = eps(C.size)
    lo = C[j - 1] if j > 0 else 0.0
    return lo - e <= u <= C[j] + e


def check_board(action, logprob, entropy, logits, mask65, T, u):
    """One board of a sampler's output against the reference -> exact (bool: the pick equals the
    float64 pick).  Asserts the acceptance rule and the log-prob / entropy tolerances."""
    j, lp, H, C, acts = ref_sample(logits, mask65, T, u)
    if acts.size == 0:
        assert action == NONE and logprob == 0.0 and entropy == 0.0, (action, logprob, entropy)
        return True
    if j < 0:
        assert action == NONE and np.isnan(logprob) and np.isnan(entropy), (action, logprob, entropy)
        return True
    k = np.searchsorted(acts, action)
    assert k < acts.size and acts[k] == action, f"action {action} is not legal"
    m = acts.size
    assert C[k] - (C[k - 1] if k else 0.0) > 0.0, f"action {action} has probability 0"
    assert accepted(int(k), C, u), (action, int(acts[j]), u, C[k - 1] if k else 0.0, C[k], eps(m))
    x = np.asarray(logits, dtype=np.float64)[acts] / np.float64(np.float32(T))
    lp_k = lp + (x[k] - x[j]) if np.isfinite(x[k]) else -np.inf
    assert abs(logprob - lp_k) <= 4 * eps(m), (logprob, lp_k, m)
    assert abs(entropy - H) <= 16 * eps(m), (entropy, H, m)
    return int(k) == j


def check_sampler(actions, logprobs, entropies, logits, masks, T, us):
    """every board of a batch; the 99 % cap on boards with 1 <= m <= 64"""
    small = exact = 0
    for i in range(len(actions)):
        ok = check_board(int(actions[i]), float(logprobs[i]), float(entropies[i]), logits[i], masks[i], T, us[i])
        m = int(legal_actions(masks[i]).size)
        if 1 <= m <= 64:
            small += 1
            exact += bool(ok)
    assert small == 0 or exact >= 0.99 * small, (exact, small)
    return exact, small


# ----------------------------------------------------------------------------- an fp32 sampler
def f32_sample(logits, mask65, T, u, order):
    """The same maths in float32 (what a kernel does), summing in the given order: 'forward'
    (a running sum), 'pairwise' (numpy's), or 'lanes' (64 strided partial sums, then their sum)."""
    f = np.float32
    acts = legal_actions(mask65)
    if acts.size == 0:
        return NONE, f(0), f(0)
    x = np.asarray(logits)[acts].astype(f) / f(T)
    mx = x.max()
    d = (x - mx).astype(f)
    e = np.exp(d).astype(f)
    if order == "forward":
        C = np.cumsum(e, dtype=f)
        S = C[-1]
    elif order == "pairwise":
        S = e.sum(dtype=f)
        C = np.cumsum(e, dtype=f)
    else:
        part = np.zeros(64, dtype=f)
        for k in range(e.size):
            part[k & 63] = f(part[k & 63] + e[k])
        S = part.sum(dtype=f)
        C = np.cumsum(e.astype(np.float64)).astype(f)  # a scan rounded once per entry
    hit = np.flatnonzero((f(u) * S < C) & (e > 0))
    j = int(hit[0]) if hit.size else int(np.flatnonzero(e > 0)[-1])
    logS = np.log(S).astype(f)
    H = f(logS - f((e * d).sum(dtype=f)) / S)
    return int(acts[j]), f(d[j] - logS), H


# ----------------------------------------------------------------------------- tests
def test_philox_restatement_matches_the_oracle(oracle):
    """policy_index(seed, board, draw, 2^24) = (x0 * 2^24) >> 32 = x0 >> 8: the bits u is made of"""
    for seed in (0, 7, 0x123456789ABCDEF0):
        for draw in (0, 1, 4000000000):
            boards = np.array([0, 1, 63, 64, 199, 65535, 2 ** 31 + 5], dtype=np.uint32)
            got = philox_x0(seed, boards, draw) >> np.uint32(8)
            want = [oracle.policy_index(seed, int(b), draw, 1 << 24) for b in boards]
            assert got.tolist() == want, (seed, draw)
    u = uniform(7, np.arange(4096), 3)
    assert u.min() >= 0.0 and u.max() < 1.0 and 0.45 < u.mean() < 0.55
    assert (u.astype(np.float32).astype(np.float64) == u).all()


def test_mask_helpers_and_families():
    masks = synthetic_masks(200, 1)
    counts = [legal_actions(m).size for m in masks]
    for i, c in enumerate(counts):
        fam = FAMILIES[i % 9]
        want = {"empty": 0, "single": 1, "exactly64": 64, "exactly65": 65, "all": 4100, "full_word": 64,
                "last_bit": 1}.get(fam)
        if want is not None:
            assert c == want, (i, fam, c)
        elif fam == "castles":
            assert 1 <= c <= 4 and legal_actions(masks[i]).min() >= 4096
        else:
            assert 1 <= c <= 40
    assert legal_actions(masks[7]).tolist() == [4095]
    a = np.array([0, 63, 64, 4095, 4096, 4099])
    assert legal_actions(mask_from_actions(a)).tolist() == a.tolist()


def test_quantise_is_exact_and_round_to_nearest_even():
    x = np.array([1.0, -8.0, 0.1, 3.14159, 1.00390625, 1.01171875, -np.inf, np.nan], dtype=np.float32)
    raw, val = quantise(x, "bfloat16")
    assert raw.dtype == np.uint16
    assert val[0] == 1.0 and val[1] == -8.0 and val[6] == -np.inf and np.isnan(val[7])
    assert val[4] == 1.0 and val[5] == 1.015625  # ties: to the even mantissa, both ways
    assert abs(val[2] - 0.1) < 2.0 ** -11 and abs(val[3] - 3.14159) < 2.0 ** -6
    raw, val = quantise(x, "float16")
    assert raw.dtype == np.uint16 and val[2] == float(np.float16(0.1))
    raw, val = quantise(x, "float32")
    assert raw.dtype == np.float32 and val[2] == float(np.float32(0.1))


def test_reference_on_hand_cases():
    mask = mask_from_actions([5, 70, 4097])
    row = np.zeros(4100)
    row[[5, 70, 4097]] = np.log([1.0, 2.0, 1.0])
    for u, want in ((0.0, 0), (0.2499, 0), (0.25, 1), (0.7499, 1), (0.75, 2), (0.999999, 2)):
        j, lp, H, C, acts = ref_sample(row, mask, 1.0, u)
        assert j == want and acts.tolist() == [5, 70, 4097]
        assert abs(lp - np.log([0.25, 0.5, 0.25][want])) < 1e-12
        assert abs(H - 1.5 * np.log(2.0)) < 1e-12
    # temperature 0.5 squares the odds: p = 1/6, 4/6, 1/6
    j, lp, H, C, _ = ref_sample(row, mask, 0.5, 0.5)
    assert j == 1 and abs(C[0] - 1 / 6) < 1e-12 and abs(lp - np.log(4 / 6)) < 1e-12
    # a legal -inf is never chosen; illegal entries are never looked at
    row2 = np.full(4100, np.nan)
    row2[[5, 70, 4097]] = [-np.inf, 0.0, -np.inf]
    for u in (0.0, 0.5, 0.999999):
        j, lp, H, _, _ = ref_sample(row2, mask, 1.0, u)
        assert j == 1 and lp == 0.0 and H == 0.0
    row2[70] = -np.inf
    assert np.isnan(ref_sample(row2, mask, 1.0, 0.5)[1])
    row2[70] = np.nan
    assert np.isnan(ref_sample(row2, mask, 1.0, 0.5)[1])
    assert ref_sample(row, np.zeros(65, dtype=np.uint64), 1.0, 0.5)[:3] == (-1, 0.0, 0.0)
    row[70] = row[4097] = 3.0
    assert ref_greedy(row, mask, 1.0)[0] == 1  # a tie goes to the lowest action id


def test_rule_is_neither_vacuous_nor_too_tight():
    """On the GPU tests' inputs, float32 restatements in three summation orders pass the rule on
    every board and agree exactly with the float64 pick on >= 99 % of the boards with m <= 64;
    a pick one action off (what a wrong scan or offset gives) is refused on >= 99 % of the boards
    with 2 <= m <= 65 (it passes only where u lies within eps <= 2.8e-5 of the shared boundary; at
    m = 4100 eps exceeds the mean probability, so neighbours there may pass)."""
    n, seed, T = 200, 11, 1.0
    masks = synthetic_masks(n, 1)
    us = uniform(seed, np.arange(n), 0)
    refused = tried = 0
    for dtype in DTYPES:
        raw, val = synthetic_logits(n, 4100, dtype, 2)
        for order in ("forward", "pairwise", "lanes"):
            out = [f32_sample(val[i], masks[i], T, us[i], order) for i in range(n)]
            exact, small = check_sampler([o[0] for o in out], [o[1] for o in out], [o[2] for o in out], val, masks,
                                         T, us)
            assert small >= 100 and exact >= 0.99 * small
        # not vacuous: the neighbour of the reference pick fails the rule
        for i in range(n):
            j, _, _, C, acts = ref_sample(val[i], masks[i], T, us[i])
            if not 2 <= acts.size <= 65:
                continue
            tried += 1
            refused += not accepted(j + 1 if j + 1 < acts.size else j - 1, C, us[i])
    assert tried >= 300 and refused >= 0.99 * tried, (refused, tried)


def test_rule_at_another_temperature():
    n, T = 200, np.float32(0.8)
    masks = synthetic_masks(n, 1)
    us = uniform(5, np.arange(n), 9)
    raw, val = synthetic_logits(n, 4104, "bfloat16", 3)
    out = [f32_sample(val[i], masks[i], T, us[i], "lanes") for i in range(n)]
    check_sampler([o[0] for o in out], [o[1] for o in out], [o[2] for o in out], val, masks, T, us)
