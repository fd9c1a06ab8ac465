"""Full-trajectory oracle digests of the device API step (gc_env_step_device, auto-reset on): the
quad kernels k_env_step_api4 (opponent "none") and k_env_step_api4_vs<false / true> (the random
opponent with a WHITE / BLACK agent) -- their action validation, mask writer, observation writer
and action-id-order pick -- on all 16 347 boards x 2 000 steps per case against the oracle.

The loop, per board (state: `a` the action to feed, at first the env's creation-time pick; `d` the
digest, at first 0); step p = 0 .. STEPS - 1:
  1. s = policy_index(seed ^ 0x5EEDAC7105, board, p, 16), r = policy_index(same, board, p + 2^31,
     4101).  s == 0: act = r, an arbitrary action.  s == 1: a near miss of the pick -- a < 4096:
     act = (a & 0xFC0) | (r & 63), the pick's own piece with another target (blocked rays, pinned
     pieces, wrong pawn pushes); else act = 4096 + (r & 3).  Otherwise act = a.
  2. step(act) with auto-reset; both kings checked (the engine raises) is done = 1, reason = 5.
     pick = the k-th legal action of the new position in action-id order, k = policy_index(seed,
     board, draw++, count); 0xFFFF without a legal move.
  3. d = (d ^ w) * 0x100000001B3 for w = the trace word (act, reward, done, reason), then for
     w = pick | count << 16; when (p + 1) % 100 == 0 also for the 65 mask words and the eight
     words of the observation; when (p + 1) % 500 == 0, d is kept as a snapshot.
  4. count == 0 (no legal move, not done): the board is reset as the host reset does -- with one
     policy pick in move-set order, the next `a` -- so no step is spent on a stuck board.
  5. Otherwise a = pick.
After the last step the board's eight words and its meta word are folded: `final`.

tests/golden/api_digests_<case>.npz (tests/golden/make_api_digests.py) holds the oracle's
snapshots, final digests and statistics (oracle/gc_oracle.c oracle_api_digests).  The CPU part
pins the fixture to the current oracle, ties the C loop to OracleEnv's per-step semantics (which
tests/test_api_step.py compares with the kernels field by field) through a Python restatement, and
reads the coverage conditions; the GPU part runs the loop on the device and compares every board.

Measured by the generator on the full runs (16 347 boards x 2 000 steps per case, in the order
none / random_white / random_black): 9.39 % / 9.39 % / 9.81 % of the 2.04 M near misses are legal
(five in six of those another action than the pick), 0.57 % / 0.56 % / 0.44 % of the 2.04 M
arbitrary actions; 6 198 / 6 287 / 6 522 stuck resets; 87 211 / 190 249 / 112 358 episode ends; the
longest legal list 82 / 78 / 78.  The move cap (reason 3) is never met by the BLACK agent's run.
Reference: chess_v2.py:219-294 (step), 183-217 (reset), 333-335 (possible_actions)."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "api_digests_{}.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_api_digests import BOARDS, CASES, MASK_EVERY, SNAP_EVERY, STEPS, coverage_gaps  # noqa: E402
from test_policy_sample import philox_x0  # noqa: E402

PRIME = np.uint64(0x100000001B3)
ACTION_STREAM = 0x5EEDAC7105
NONE = 0xFFFF
CASE_IDS = [c[0] for c in CASES]


def fold(d, w):
    """d = (d ^ w) * PRIME elementwise, uint64 wrap-around (oracle/gc_oracle.c digest_fold)"""
    with np.errstate(over="ignore"):
        return (d ^ w) * PRIME


def trace_words(act, reward, done, reason):
    """oracle_trace_word on arrays: action u16 | reward i16 << 16 | done << 32 | reason << 40"""
    u = np.uint64
    return (np.asarray(act).astype(np.uint16).astype(u) | (np.asarray(reward).astype(np.int16).view(np.uint16).astype(u) << u(16))
            | (np.asarray(done).astype(np.uint8).astype(u) << u(32)) | (np.asarray(reason).astype(np.uint8).astype(u) << u(40)))


def schedule(seed, boards, steps, threads=8):
    """step 1's draws for every (step, board): s uint8[steps][n], r uint16[steps][n] (r only
    where s < 2, else 0).  index = (x0 * n) >> 32 over the vectorised Philox."""
    boards = np.asarray(boards, dtype=np.uint64)
    s_all = np.zeros((steps, len(boards)), dtype=np.uint8)
    r_all = np.zeros((steps, len(boards)), dtype=np.uint16)

    def chunk(p0):
        p = np.arange(p0, min(p0 + 32, steps), dtype=np.uint64)
        b, d = np.broadcast_arrays(boards[None, :], p[:, None])
        s = (philox_x0(seed ^ ACTION_STREAM, b, d).astype(np.uint64) * np.uint64(16)) >> np.uint64(32)
        sel = s < 2
        r = (philox_x0(seed ^ ACTION_STREAM, b[sel], d[sel] + np.uint64(1 << 31)).astype(np.uint64) * np.uint64(4101)) >> np.uint64(32)
        s_all[p0:p0 + len(p)] = s
        r_all[p0:p0 + len(p)][sel] = r

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(chunk, range(0, steps, 32)))
    return s_all, r_all


def choose(a, s, r):
    """step 1: the actions to feed, from the carried picks a and the step's draws"""
    a = np.asarray(a, dtype=np.int64)
    r = np.asarray(r, dtype=np.int64)
    near = np.where(a < 4096, (a & 0xFC0) | (r & 63), 4096 + (r & 3))
    return np.where(s == 0, r, np.where(s == 1, near, a))


def mask_words(legal):
    """a legal list as the API step's 65 mask words: word f bit t = action f * 64 + t, word 64
    bits 0..3 = actions 4096..4099"""
    m = np.zeros(65, dtype=np.uint64)
    for x in legal:
        m[x >> 6] |= np.uint64(1) << np.uint64(x & 63)
    return m


def load(name):
    if not os.path.exists(FIXTURE.format(name)):
        pytest.fail(f"tests/golden/api_digests_{name}.npz is missing (tests/golden/make_api_digests.py)")
    f = np.load(FIXTURE.format(name))
    assert (int(f["boards"]), int(f["steps"])) == (BOARDS, STEPS)
    assert f["snap"].shape == (STEPS // SNAP_EVERY, BOARDS) and f["final"].shape == (BOARDS,)
    return f


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name,seed,opp,color", CASES, ids=CASE_IDS)
def test_fixture_pinned_to_oracle(oracle, name, seed, opp, color):
    """a strided sample of the fixture's boards (the first, the last, six between) regenerated by
    oracle_api_digests: the same snapshots and final digests"""
    f = load(name)
    assert int(f["seed"]) == seed
    for i in list(range(0, BOARDS, 2333)) + [BOARDS - 1]:
        snap, final, _ = oracle.api_digests(seed, 1, STEPS, opponent=opp, agent_white=color == "WHITE", b_begin=i,
                                            mask_every=MASK_EVERY, snap_every=SNAP_EVERY)
        assert (snap[:, 0] == f["snap"][:, i]).all() and final[0] == f["final"][i], i


def python_loop(oracle, seed, opp, color, board, steps, mask_every, snap_every):
    """the loop of this module's docstring on one board, stepping OracleEnv, with the masks and
    the folds in numpy -> (snapshots, final, steps fed to a board without a legal move)"""
    o = oracle.OracleEnv(opponent=opp, agent_white=color == "WHITE", seed=seed, board=board)
    s, r = schedule(seed, [board], steps, threads=1)
    a = o.pick()
    d = np.zeros(1, dtype=np.uint64)
    snaps, stuck_steps = [], 0
    for p in range(steps):
        act = int(choose([a], s[p], r[p])[0])
        stuck_steps += not o.moves()
        rc, rw, dn, why = o.step(act)
        if rc == 1:
            dn, why = 1, 5
        if dn:
            o.reset()
        legal = sorted(o.moves())
        pick = NONE
        if legal:
            pick = legal[oracle.policy_index(seed, board, o.draw, len(legal))]
            o.pick()  # the pick's draw
        d = fold(d, trace_words([act], [rw], [dn], [why]))
        d = fold(d, np.uint64(pick | len(legal) << 16))
        if (p + 1) % mask_every == 0:
            for w in mask_words(legal):
                d = fold(d, w)
            for w in o.state()[0].view(np.uint64):
                d = fold(d, w)
        if (p + 1) % snap_every == 0:
            snaps.append(d[0])
        if not legal:
            o.reset()
            a = o.pick()
        else:
            a = pick
    b, m = o.state()
    for w in b.view(np.uint64):
        d = fold(d, w)
    d = fold(d, m.view(np.uint64)[0])
    return np.array(snaps, dtype=np.uint64), d[0], stuck_steps


@pytest.mark.parametrize("name,seed,opp,color", CASES, ids=CASE_IDS)
def test_c_loop_is_the_python_loop(oracle, name, seed, opp, color):
    """3 boards x 300 steps: oracle_api_digests == the Python restatement over OracleEnv's step /
    moves / reset / pick / draw / state (mask and snapshot periods short enough to fall inside);
    and the vectorised schedule == the oracle's scalar policy_index"""
    steps, mask_every, snap_every = 300, 50, 100
    for board in (0, 5000, BOARDS - 1):
        s, r = schedule(seed, [board], steps, threads=1)
        for p in range(steps):
            assert s[p, 0] == oracle.policy_index(seed ^ ACTION_STREAM, board, p, 16)
            if s[p, 0] < 2:
                assert r[p, 0] == oracle.policy_index(seed ^ ACTION_STREAM, board, p + (1 << 31), 4101)
        snap, final, st = oracle.api_digests(seed, 1, steps, opponent=opp, agent_white=color == "WHITE", b_begin=board,
                                             mask_every=mask_every, snap_every=snap_every)
        psnap, pfinal, stuck_steps = python_loop(oracle, seed, opp, color, board, steps, mask_every, snap_every)
        assert snap.shape == (3, 1) and (snap[:, 0] == psnap).all() and final[0] == pfinal, board
        assert stuck_steps == 0 and st["stuck_steps"] == 0
        assert int(st["reasons"].sum()) == steps


@pytest.mark.parametrize("name", CASE_IDS)
def test_fixture_coverage(name):
    """what the fixture's run met, from its statistics: reasons 0 (a plain step), 1 (the opponent
    mated), 2 (3-fold), 5 (both kings checked) and 6 (invalid action) in every case; 3 (the move
    cap) for a WHITE agent (a BLACK agent's move count never advances, chess_v2.py:291-292); 8 (the
    agent mated) and 9 (the opponent without a reply) against the random opponent; arbitrary
    actions and near misses both accepted and refused; boards reset for lack of a legal move, and
    no step fed to one"""
    f = load(name)
    stats = {k: f[k] for k in f.files}
    assert coverage_gaps(name, stats) == []
    assert int(f["reasons"].sum()) == BOARDS * STEPS
    assert int(f["stuck_steps"]) == 0 and int(f["stuck_resets"]) > 0


# ----------------------------------------------------------------------------- GPU
def device_loop(seed, opp, color, n, steps, mask_every=MASK_EVERY, snap_every=SNAP_EVERY):
    """the loop on a BatchedChessEnv(n) with device_io() at its default mask stride -> (snapshots
    uint64[steps // snap_every][n], final uint64[n], steps fed to a board without a legal move,
    stuck resets)"""
    from gym_chess_amd.env import BatchedChessEnv

    s, r = schedule(seed, np.arange(n), steps, threads=max(1, min(16, os.cpu_count() or 1)))
    env = BatchedChessEnv(n, device=0, seed=seed, opponent="random" if opp else "none", player_color=color)
    io = env.device_io()  # pick = the env's creation-time picks (one draw each)
    assert io.mask_stride == io.default_mask_stride(n)
    act_buf = env.device_io(mask=False, obs=False, count=False, pick=True, select=False)
    a = io.fetch("pick")["pick"].astype(np.int64)
    d = np.zeros(n, dtype=np.uint64)
    snaps, stuck_steps, stuck_resets = [], 0, 0
    for p in range(steps):
        stuck_steps += int((a == NONE).sum())
        act = choose(a, s[p], r[p]).astype(np.uint16)
        act_buf.upload_actions(act)
        env.step_device(io, actions=act_buf.ptr["pick"], autoreset=True)
        fold_step = (p + 1) % mask_every == 0
        o = io.fetch("reward", "done", "reason", "pick", "count", *(("mask", "obs") if fold_step else ()))
        d = fold(d, trace_words(act, o["reward"], o["done"], o["reason"]))
        d = fold(d, o["pick"].astype(np.uint64) | (o["count"].astype(np.uint64) << np.uint64(16)))
        if fold_step:
            for f in range(65):
                d = fold(d, o["mask"][:, f])
            obs = np.ascontiguousarray(o["obs"]).view(np.uint64)
            for q in range(8):
                d = fold(d, obs[:, q])
        if (p + 1) % snap_every == 0:
            snaps.append(d.copy())
        a = o["pick"].astype(np.int64)
        stuck = o["count"] == 0
        if stuck.any():  # no legal move, not done: the host reset and its policy pick
            env.reset(stuck.astype(np.uint8), states=False)
            a[stuck] = env.outputs()["next_action"][stuck]
            stuck_resets += int(stuck.sum())
    b, m = env.boards()
    bw = np.ascontiguousarray(b).view(np.uint64)
    for q in range(8):
        d = fold(d, bw[:, q])
    d = fold(d, np.ascontiguousarray(m).view(np.uint64)[:, 0])
    act_buf.close()
    io.close()
    env.close()
    return np.array(snaps, dtype=np.uint64).reshape(steps // snap_every, n), d, stuck_steps, stuck_resets


def describe_mismatch(name, snap, final, want_snap, want_final):
    """None if every board's snapshots and final digest equal the fixture's, else the message:
    how many boards differ, the first ids, and the earliest window of SNAP_EVERY steps that differs"""
    got = np.concatenate([snap, final[None]], axis=0)
    want = np.concatenate([want_snap, want_final[None]], axis=0)
    diff = got != want
    bad = np.nonzero(diff.any(axis=0))[0]
    if len(bad) == 0:
        return None
    first = diff[:, bad].argmax(axis=0)  # per differing board, its first differing snapshot
    k = int(first.min())
    lo, hi = k * SNAP_EVERY, min((k + 1) * SNAP_EVERY, STEPS)
    where = f"steps {lo}..{hi - 1}" if k < len(snap) else "the final state"
    ids = bad[first == k][:8].tolist()
    return (f"{name}: {len(bad)} of {got.shape[1]} boards differ from the oracle: {bad[:16].tolist()}; the earliest "
            f"difference is in {where} (boards {ids}).  Replay one step by step against the oracle env: "
            f"python tools/soak.py --api-digest {name} --board {ids[0]}")


def test_mismatch_report_names_boards_and_window():
    """the GPU test's report, on the fixture with digests changed by hand: equal arrays give none;
    a board that differs from its third snapshot on and one that differs only in the final digest
    are both counted, and the earliest window and its board are named"""
    f = load("none")
    snap, final = f["snap"].copy(), f["final"].copy()
    assert describe_mismatch("none", snap, final, f["snap"], f["final"]) is None
    snap[2:, 12345] ^= np.uint64(1)
    final[12345] ^= np.uint64(1)
    final[7] ^= np.uint64(1) << np.uint64(63)
    msg = describe_mismatch("none", snap, final, f["snap"], f["final"])
    assert "2 of 16347 boards differ" in msg and "[7, 12345]" in msg
    assert "steps 1000..1499 (boards [12345])" in msg and "--api-digest none --board 12345" in msg
    only_final = describe_mismatch("none", f["snap"], final, f["snap"], f["final"])
    assert "the final state (boards [7, 12345])" in only_final


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,opp,color", CASES, ids=CASE_IDS)
def test_api_digests_vs_oracle(oracle, name, seed, opp, color):
    """every board's four snapshots and final digest == the fixture's; no step spent on a board
    without a legal move, and as many stuck resets as the oracle's run"""
    f = load(name)
    t0 = time.time()
    snap, final, stuck_steps, stuck_resets = device_loop(seed, opp, color, BOARDS, STEPS)
    secs = time.time() - t0
    msg = describe_mismatch(name, snap, final, f["snap"], f["final"])
    print(f"api digest {name}: {BOARDS} boards x {STEPS} steps, {'equal' if msg is None else 'DIFFERENT'}, "
          f"{stuck_resets} stuck resets, {secs:.1f} s")
    assert msg is None, msg
    assert stuck_steps == 0 and stuck_resets == int(f["stuck_resets"])
