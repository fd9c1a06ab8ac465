"""The fused ply's straight-line phase 3 (k_env_rollout4): the count words made as running prefixes
by their makers, the pick without multiplies or per-lane regions (sw_locate_pre, sw_finish,
sw_origin), the pending action resolved by one read and a select, the outcome as flags and selects.
Launches of 1, 7, 49, 50 and m plies (m = gc_env_rollout_occ_min_plies) back to back on one env,
ROUNDS times over, run the three forms <false, 2>, <false, 1> and <true, 1> and both sides of the
split threshold (49 / 50) at every stage of the games.  By the oracle's traces alone the plies of
each form hold a castle of each id that is ever legal (a black castle never is: the reference
tests the white ids), a no-move ply, a mate, a move-cap or 3-fold end and a reset followed by a
pick from the start position's table; then every board's whole trajectory, boards' state included,
is compared with the oracle's by digest (run_digests of tests/test_philox_ahead_gpu.py).
Reference: test_benchmark.py:9-43 (the driver), chess_v2.py:183-294."""
import numpy as np
import pytest

import test_philox_ahead_gpu as PA

SEED = 0x5719  # chosen by the oracle alone: test_schedule_holds_the_cases
BOARDS = (64, 65, 193)
ROUNDS = 6
A_KSW, A_QSW = 4096, 4097
R_MATE, R_REPETITION, R_MOVE_CAP = 1, 2, 3
FORMS = ("<false, 2>", "<false, 1>", "<true, 1>")


def launch_lengths(m):
    return (1, 7, 49, 50, m) * ROUNDS


def form_of(k, m):
    """the kernel instance a launch of k plies runs (gc_host_env.h roll_quads_wg, occ_min_plies)"""
    return 0 if k < 50 else 1 if k < m else 2


@pytest.fixture(scope="module")
def occ_min():
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(1, device=0, seed=SEED)
    m = env.rollout_occ_min_plies()
    env.close()
    assert m > 50
    return m


@pytest.fixture(scope="module")
def traces(oracle, occ_min):
    plies = sum(launch_lengths(occ_min))
    return [oracle.rollout_trace(SEED, i, plies) for i in range(max(BOARDS))]


@pytest.fixture(scope="module")
def want(oracle, occ_min):
    """the oracle's digests of the widest env's boards over the whole schedule, computed once (a
    board's trajectory depends on the seed and its index only, so a narrower env's are a prefix)"""
    return oracle.rollout_digests(SEED, max(BOARDS), sum(launch_lengths(occ_min)), threads=16)


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOARDS)
def test_schedule_holds_the_cases(traces, occ_min, n):
    ks = launch_lengths(occ_min)
    edges = np.concatenate([[0], np.cumsum(ks)])
    names = ("castle KS", "castle QS", "no-move ply", "mate", "move-cap or 3-fold end", "reset then table pick")
    seen = np.zeros((3, len(names)), dtype=np.int64)
    for t in traces[:n]:
        a, d, why = t["action"].astype(np.int64), t["done"], t["reason"]
        for j, k in enumerate(ks):
            lo, hi = edges[j], edges[j + 1]
            aa, ww = a[lo:hi], why[lo:hi]
            # a ply that resets (an episode's end, or the driver's no-move reset) and the next ply, of
            # the same launch, that plays the table's pick
            reset = ((d[lo:hi - 1] == 1) | (aa[:-1] == -1)) & (aa[1:] >= 0)
            seen[form_of(k, occ_min)] += [(aa == A_KSW).sum(), (aa == A_QSW).sum(), (aa == -1).sum(), (ww == R_MATE).sum(),
                                          ((ww == R_REPETITION) | (ww == R_MOVE_CAP)).sum(), reset.sum()]
        assert not (a >= 4098).any()  # a black castle is never legal under the reference's rules
    print("boards", n, {FORMS[f]: dict(zip(names, seen[f].tolist())) for f in range(3)})
    for f in range(3):
        assert (seen[f] > 0).all(), (FORMS[f], dict(zip(names, seen[f].tolist())))


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOARDS)
def test_digests_vs_oracle(monkeypatch, want, occ_min, n):
    monkeypatch.setattr(PA, "SEED", SEED)  # run_digests makes its env with the module's seed
    d = PA.run_digests(n, launch_lengths(occ_min))
    bad = np.nonzero(d != want[:n])[0]
    assert len(bad) == 0, f"{len(bad)} of {n} boards differ from the oracle: {bad[:16].tolist()}"
