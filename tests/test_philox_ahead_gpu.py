"""The fused ply's Philox word a ply ahead (k_env_rollout4): Q3 makes the next draw's word and
the reset table's pick in its wait for the ply's last barrier, from the draw counter's usual
step, and makes them again at the next ply's top where the counter stayed -- the ply after a
stalemate, the driver's no-move reset (action -1).  A launch's first ply takes its word from
the counter loaded at entry.  (a) Launches of m, m, 93, 93, 7, 7 plies back to back on one env
(m = gc_env_rollout_occ_min_plies) run the three forms <true, 1>, <false, 1> and <false, 2>
with a no-move ply inside each form's launches; (b) a schedule cut at a board's first no-move
ply p -- launches of p, 1, 1 and 50 plies -- ends a launch with the stalemate, runs the no-move
ply as a launch of its own (its word from the entry load) and the ply after it as another.
Every board's whole trajectory, boards' state included, is compared with the oracle's by
digest, as tests/test_ply_prework_gpu.py does.
Reference: test_benchmark.py:9-43 (the driver), chess_v2.py:183-294."""
import numpy as np
import pytest

from test_rollout_geometry_gpu import fold

SEED = 0xB12
BOARDS = (64, 193)
SCAN = 400  # plies searched for a board's first no-move ply


def launch_lengths(m):
    return (m, m, 93, 93, 7, 7)


@pytest.fixture(scope="module")
def occ_min():
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(1, device=0, seed=SEED)
    m = env.rollout_occ_min_plies()
    env.close()
    assert m > 93
    return m


@pytest.fixture(scope="module")
def traces(oracle, occ_min):
    """the oracle's actions of every board over the longer schedule, computed once"""
    plies = sum(launch_lengths(occ_min))
    return [oracle.rollout_trace(SEED, i, plies)["action"].astype(np.int64) for i in range(max(BOARDS))]


def cut(traces, n):
    """(p, board): the earliest no-move ply among the first n boards"""
    p, b = min((int(np.nonzero(t[:SCAN] == -1)[0][0]), i) for i, t in enumerate(traces[:n]) if (t[:SCAN] == -1).any())
    return p, b


@pytest.fixture(scope="module")
def want_a(oracle, occ_min):
    return oracle.rollout_digests(SEED, max(BOARDS), sum(launch_lengths(occ_min)), threads=16)


def run_digests(n, ks):
    """launches of ks plies back to back on one env of n boards: every board's digest"""
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(n, device=0, seed=SEED)
    assert env.rollout_waves() == 4  # the quad kernel
    tbs = [env.trace_buffer(max(ks)) for _ in ks]
    for k, tb in zip(ks, tbs):
        env.rollout_device(k, tb)
    env.wait_rollout()
    env.synchronize()
    d = np.zeros(n, dtype=np.uint64)
    for k, tb in zip(ks, tbs):
        for row in tb.raw(k):
            d = fold(d, row)
    b, mt = env.boards()
    for q in range(8):
        d = fold(d, np.ascontiguousarray(b).view(np.uint64)[:, q])
    d = fold(d, np.ascontiguousarray(mt).view(np.uint64)[:, 0])
    for tb in tbs:
        tb.close()
    env.close()
    return d


@pytest.mark.gpu
def test_schedules_hold_the_cases(traces, occ_min):
    """by the oracle alone: (a) a no-move ply inside each form's launches; (b) the cut's ply is a
    no-move ply, the ply before it was played and ended nothing (the stalemate), p >= 1"""
    ks = launch_lengths(occ_min)
    edges = np.concatenate([[0], np.cumsum(ks)])
    nomove = np.zeros(len(ks), dtype=np.int64)
    for act in traces:
        for j in range(len(ks)):
            nomove[j] += int((act[edges[j]:edges[j + 1]] == -1).sum())
    print("no-move plies per launch", nomove.tolist())
    for form in range(3):  # <true, 1>, <false, 1>, <false, 2>
        assert nomove[2 * form] + nomove[2 * form + 1] >= 1, (form, nomove.tolist())
    for n in BOARDS:
        p, b = cut(traces, n)
        print("boards", n, "cut at ply", p, "of board", b)
        assert b < n and 1 <= p < SCAN - 52
        assert traces[b][p] == -1 and traces[b][p - 1] >= 0 and traces[b][p + 1] >= 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOARDS)
def test_forms_digests_vs_oracle(want_a, occ_min, n):
    d = run_digests(n, launch_lengths(occ_min))
    bad = np.nonzero(d != want_a[:n])[0]
    assert len(bad) == 0, f"{len(bad)} of {n} boards differ from the oracle: {bad[:16].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOARDS)
def test_cut_at_no_move_ply_digests_vs_oracle(oracle, traces, n):
    p, _ = cut(traces, n)
    ks = (p, 1, 1, 50)
    want = oracle.rollout_digests(SEED, n, sum(ks), threads=16)
    d = run_digests(n, ks)
    bad = np.nonzero(d != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {n} boards differ from the oracle: {bad[:16].tolist()}"
