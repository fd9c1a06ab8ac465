"""The fused ply's chain from the pick to the apply (k_env_rollout4): the origin of a slider's
move from the line's stride (gc_core.h sw_origin), the sets' counts handed to Q2 as byte prefixes
of the words each role owns (sw_locate_pre), and the apply's castle terms made only on the plies
where a lane of the wave castles (apply_legal_krw / apply_legal_qbnp / apply_legal_with<false>
elsewhere).  Launches of 7, 7, 7, 7, 93 and m plies back to back on one env (m =
gc_env_rollout_occ_min_plies) run the three forms <false, 2>, <false, 1> and <true, 1>.  By the
oracle's traces alone each form's plies hold a castle -- so its waves take both paths of the
apply -- and the last form's hold both castle ids and a no-move ply.  Every board's whole
trajectory, boards' state included, is compared with the oracle's by digest, as
tests/test_philox_ahead_gpu.py does.
Reference: test_benchmark.py:9-43 (the driver), chess_v2.py:183-294, lib.rs:740-773."""
import numpy as np
import pytest

from test_philox_ahead_gpu import run_digests

SEED = 0xB12
BOARDS = (64, 193)
A_KSW, A_QSW = 4096, 4097


def launch_lengths(m):
    return (7, 7, 7, 7, 93, m)


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
    """the oracle's actions of every board over the schedule, computed once"""
    plies = sum(launch_lengths(occ_min))
    return [oracle.rollout_trace(SEED, i, plies)["action"].astype(np.int64) for i in range(max(BOARDS))]


@pytest.fixture(scope="module")
def want(oracle, occ_min):
    return oracle.rollout_digests(SEED, max(BOARDS), sum(launch_lengths(occ_min)), threads=16)


def form_counts(traces, n, lo, hi):
    """castles of either id and no-move plies among the first n boards' plies lo .. hi - 1"""
    part = np.stack([t[lo:hi] for t in traces[:n]])
    return int((part == A_KSW).sum()), int((part == A_QSW).sum()), int((part == -1).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOARDS)
def test_schedule_holds_the_cases(traces, occ_min, n):
    """by the oracle alone: a castle in each form's plies; both castle ids and a no-move ply in
    the last form's"""
    ks = launch_lengths(occ_min)
    forms = ((0, 28), (28, 28 + 93), (28 + 93, sum(ks)))  # <false, 2>, <false, 1>, <true, 1>
    counts = [form_counts(traces, n, lo, hi) for lo, hi in forms]
    print("boards", n, "castles 4096 / 4097 and no-move plies per form", counts)
    for ksw, qsw, _ in counts:
        assert ksw + qsw >= 1, counts
    ksw, qsw, nomove = counts[2]
    assert ksw >= 1 and qsw >= 1 and nomove >= 1, counts


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOARDS)
def test_forms_digests_vs_oracle(traces, want, occ_min, n):
    test_schedule_holds_the_cases(traces, occ_min, n)  # (nothing is proved by a schedule without the cases)
    d = run_digests(n, launch_lengths(occ_min))
    bad = np.nonzero(d != want[:n])[0]
    assert len(bad) == 0, f"{len(bad)} of {n} boards differ from the oracle: {bad[:16].tolist()}"
