"""The fused ply's work ahead of its data (k_env_rollout4): Q0 makes what the apply needs of the
settled state alone (State::new's rights, the occupancy, the white kings and rooks) at the end
of phase 3 and holds it across the ply's last barrier -- after a reset (the ply after a
stalemate is a no-move ply: the driver's reset) it is the start position's, after a castle the
rights are gone -- and takes the first ply's action as a pending table pick.  Launches of
m, m, 93, 93, 7, 7 plies back to back on one env (m = gc_env_rollout_occ_min_plies) run the
three forms <true, 1>, <false, 1> and <false, 2>, the state carried from launch to launch;
every board's whole trajectory is compared with the oracle's by digest, as
tests/test_rollout_geometry_gpu.py does, and the oracle's trace shows that the schedule holds
the cases: a no-move ply inside the launches of every form, a castle inside those of the first two.
Reference: test_benchmark.py:9-43 (the driver), chess_v2.py:183-294."""
import numpy as np
import pytest

from test_rollout_geometry_gpu import fold

SEED = 0x9A1
BOARDS = (64, 193)


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
def want(oracle, occ_min):
    """the oracle's digests of the wider env's boards over the whole schedule, computed once (a
    board's trajectory depends on the seed and its index only: the narrower env's are a prefix)"""
    return oracle.rollout_digests(SEED, max(BOARDS), sum(launch_lengths(occ_min)), threads=16)


@pytest.mark.gpu
def test_schedule_holds_the_cases(oracle, occ_min):
    """no-move plies (action -1: the draw counter stayed) and castles per launch, by the oracle"""
    ks = launch_lengths(occ_min)
    edges = np.concatenate([[0], np.cumsum(ks)])
    nomove = np.zeros(len(ks), dtype=np.int64)
    castles = np.zeros(len(ks), dtype=np.int64)
    for i in range(max(BOARDS)):
        act = oracle.rollout_trace(SEED, i, int(edges[-1]))["action"].astype(np.int64)
        for j in range(len(ks)):
            seg = act[edges[j]:edges[j + 1]]
            nomove[j] += int((seg == -1).sum())
            castles[j] += int((seg >= 4096).sum())
    print("no-move plies per launch", nomove.tolist(), "castles per launch", castles.tolist())
    for form in range(3):  # <true, 1>, <false, 1>, <false, 2>
        assert nomove[2 * form] + nomove[2 * form + 1] >= 1, (form, nomove.tolist())
    for form in range(2):
        assert castles[2 * form] + castles[2 * form + 1] >= 1, (form, castles.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOARDS)
def test_ply_prework_digests_vs_oracle(want, occ_min, n):
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(n, device=0, seed=SEED)
    assert env.rollout_waves() == 4  # the quad kernel
    m = env.rollout_occ_min_plies()
    assert m == occ_min
    ks = launch_lengths(m)
    tbs = [env.trace_buffer(m) for _ in ks]
    for k, tb in zip(ks, tbs):  # back to back on one env
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
    bad = np.nonzero(d != want[:n])[0]
    assert len(bad) == 0, f"{len(bad)} of {n} boards differ from the oracle: {bad[:16].tolist()}"
