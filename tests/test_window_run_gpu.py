"""The 3-fold commit's probes beyond the home slot (k_env_rollout4<true>): a slot whose bit in Q1's
occupancy bitmap is clear is not loaded while the bitmap mirrors the window -- the probe ends there
as it would after loading a free slot -- and a slot whose bit is set is loaded and compared.

64, 65 and 129 boards run three back-to-back launches of gc_env_rollout_occ_min_plies plies with the
state carried, so launches 2 and 3 begin on windows that predate them (every slot loaded, as
before) and turn to the bitmap at the first reset or irreversible move; every board's whole
trajectory is compared with the oracle's by digest (tests/test_full_width_digest.py's fold).

Whether those plies meet the cases at all is counted on the CPU first (window_events: the oracle's
trajectory replayed over a restatement of the device's table -- gc_core.h board_key, gc_env.h
rep_commit's linear probing over 512 slots, cleared by an irreversible move or a reset): on lanes
whose bitmap mirrors the window, (a) a second probe that meets a free slot, (b) a third probe,
(c) a repetition found beyond the home slot, (d) a probe run crossing a 64-bit word of the bitmap,
(e) a run wrapping from slot 511 to slot 0.  The seed is chosen so that each occurs within the
first 64 boards.
Reference: test_benchmark.py:9-43 (the driver), chess_v2.py:183-294, 393-420."""
import ctypes

import numpy as np
import pytest

SEED = 0x77A1
BOARDS = (64, 65, 129)
LAUNCHES = 3
HTAB = 512
PRIME = np.uint64(0x100000001B3)
EVENTS = ("second_probe_free", "third_probe", "repetition_beyond_home", "word_crossing", "wrap")
M32 = np.uint64(0xFFFFFFFF)


def fold(d, w):
    """d = (d ^ w) * PRIME elementwise, uint64 wrap-around (oracle/gc_oracle.c digest_fold)"""
    with np.errstate(over="ignore"):
        return (d ^ w) * PRIME


def _rotl64(x, r):
    return (x << np.uint64(r)) | (x >> np.uint64(64 - r))


def board_keys(boards):
    """gc_core.h board_key of mailbox boards int8[T][64] -> uint32[T] (as uint64)"""
    b = np.asarray(boards, dtype=np.int8).reshape(-1, 64)
    w = np.uint64(1) << np.arange(64, dtype=np.uint64)
    zero = np.uint64(0)

    def bb(mask):
        return np.where(mask, w, zero).sum(axis=1, dtype=np.uint64)

    t = np.abs(b)
    k, q, r, bi, n, p = (bb(t == v) for v in (1, 2, 3, 4, 5, 6))
    x = k ^ _rotl64(q, 11) ^ _rotl64(r, 22) ^ _rotl64(bi, 37) ^ _rotl64(n, 46) ^ _rotl64(p, 55) ^ _rotl64(bb(b > 0), 5)
    with np.errstate(over="ignore"):
        hi = ((x >> np.uint64(32)) * np.uint64(0x85EBCA77)) & M32
        y = (((x & M32) * np.uint64(0x9E3779B1)) & M32) ^ (((hi << np.uint64(16)) | (hi >> np.uint64(16))) & M32)
        y ^= y >> np.uint64(15)
        y = (y * np.uint64(0x2C1B3C6D)) & M32
    return y ^ (y >> np.uint64(12))


def _trajectory(O, seed, board, plies):
    """the driver's loop on OracleEnv, per ply: the pre-move board, whether the ply commits it to
    the window, whether the window is empty after the ply, the oracle's window length"""
    L = O.lib()
    env = O.OracleEnv(seed=seed, board=board)
    h = env.h
    rw, dn, why = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    pre = np.zeros((plies, 64), dtype=np.int8)
    meta = np.zeros(8, dtype=np.uint8)
    commit = np.zeros(plies, dtype=bool)
    empty = np.zeros(plies, dtype=bool)
    win = np.zeros(plies, dtype=np.int32)
    for p in range(plies):
        a = L.oracle_env_pick(h)
        if a < 0:  # no legal move: the driver resets
            L.oracle_env_reset(h)
            empty[p] = True
            continue
        L.oracle_env_state(h, pre[p].ctypes.data, meta.ctypes.data)
        rc = L.oracle_env_step(h, a, ctypes.byref(rw), ctypes.byref(dn), ctypes.byref(why))
        # the window is probed unless the step ends before its move: the move cap (3), an env already
        # done (7), both kings checked (rc 1)
        commit[p] = rc == 0 and why.value not in (3, 7)
        win[p] = L.oracle_env_window(h)
        if rc == 1 or dn.value:
            L.oracle_env_reset(h)
            empty[p] = True
        elif commit[p] and win[p] == 0:  # an irreversible move
            empty[p] = True
    return pre, commit, empty, win


def window_events(O, seed, n_boards, launch_plies, launches):
    """int64[n_boards][5]: per board, how often EVENTS occur over `launches` launches of `launch_plies`
    plies on a lane whose bitmap mirrors its window (from the first emptying of the window within
    the launch, or from the launch's start on an empty window)"""
    out = np.zeros((n_boards, len(EVENTS)), dtype=np.int64)
    plies = launch_plies * launches
    for i in range(n_boards):
        pre, commit, empty, win = _trajectory(O, seed, i, plies)
        keys = board_keys(pre)
        table = {}  # slot -> board
        ev = out[i]
        valid = True
        for p in range(plies):
            if p % launch_plies == 0:
                valid = not table
            if commit[p]:
                b = pre[p].tobytes()
                pos, n, cross, wrap = int(keys[p]) & (HTAB - 1), 0, 0, 0
                while True:
                    cur = table.get(pos)
                    if cur is None or cur == b:
                        break
                    wrap += pos == HTAB - 1
                    cross += pos & 63 == 63 and pos != HTAB - 1
                    pos = (pos + 1) & (HTAB - 1)
                    n += 1
                if valid and n:
                    ev[0] += n == 1 and cur is None
                    ev[1] += n >= 2
                    ev[2] += cur is not None
                    ev[3] += cross
                    ev[4] += wrap
                if cur is None and not empty[p]:
                    table[pos] = b
                    # the replayed table holds the oracle's window
                    assert len(table) == win[p], (i, p, len(table), int(win[p]))
            if empty[p]:
                table.clear()
                valid = True
    return out


@pytest.fixture(scope="module")
def launch_plies():
    from gym_chess_amd import _lib

    return int(_lib.load().gc_env_rollout_occ_min_plies())


@pytest.fixture(scope="module")
def events(oracle, launch_plies):
    return window_events(oracle, SEED, max(BOARDS), launch_plies, LAUNCHES)


def test_board_keys_consistent(oracle):
    """the restated key: distinct boards, one key per board, every slot index in range"""
    pre, commit, _, _ = _trajectory(oracle, SEED, 0, 200)
    keys = board_keys(pre[commit])
    assert keys.max() < 1 << 32
    same = {}
    for b, k in zip(pre[commit], keys):
        assert same.setdefault(b.tobytes(), int(k)) == int(k)
    assert len(set(same.values())) > len(same) * 0.99


@pytest.mark.parametrize("n", BOARDS)
def test_window_events_present(events, n):
    """the committed seed meets every case within the boards and plies the GPU test runs"""
    got = dict(zip(EVENTS, events[:n].sum(axis=0).tolist()))
    print(f"{n} boards: {got}")
    assert all(v >= 1 for v in got.values()), got


@pytest.fixture(scope="module")
def want(oracle, launch_plies):
    """the oracle's digests of the widest env's boards over the whole schedule, computed once (a
    board's trajectory depends on the seed and its index only, so a narrower env's are a prefix)"""
    return oracle.rollout_digests(SEED, max(BOARDS), LAUNCHES * launch_plies, threads=16)


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOARDS)
def test_window_run_digests_vs_oracle(want, events, launch_plies, n):
    from gym_chess_amd.env import BatchedChessEnv

    got = dict(zip(EVENTS, events[:n].sum(axis=0).tolist()))
    assert all(v >= 1 for v in got.values()), got
    env = BatchedChessEnv(n, device=0, seed=SEED)
    assert env.rollout_waves() == 4  # the quad kernel
    m = env.rollout_occ_min_plies()
    assert m == launch_plies
    tbs = [env.trace_buffer(m) for _ in range(LAUNCHES)]
    for tb in tbs:  # back to back, the state carried: launches 2 and 3 start on windows that predate them
        env.rollout_device(m, tb)
    env.wait_rollout()
    env.synchronize()
    d = np.zeros(n, dtype=np.uint64)
    for tb in tbs:
        for row in tb.raw(m):
            d = fold(d, row)
    b, mt = env.boards()
    for q in range(8):
        d = fold(d, np.ascontiguousarray(b).view(np.uint64)[:, q])
    d = fold(d, np.ascontiguousarray(mt).view(np.uint64)[:, 0])
    for tb in tbs:
        tb.close()
    env.close()
    bad = np.nonzero(d != want[:n])[0]
    assert len(bad) == 0, f"{len(bad)} of {n} boards differ from the oracle: {bad[:16].tolist()}"
