"""The quad rollout's launch geometry at small board counts.  k_env_rollout4 runs one quad (64
boards, four waves) per workgroup in all but short launches, which keep two; the workgroups
that share a CU take turns by their place in the launch, and the last workgroup re-arms the
completion word from the workgroup count.  Board counts of 1 to 6 workgroups -- fewer than the
four that share a CU, counts not divisible by four, a partial last wave -- run pairs of
back-to-back launches of 3 plies (two quads per workgroup) and just below and at
gc_env_rollout_occ_min_plies (one; without and with the occupancy filter), the state carried
from launch to launch, and every board's whole trajectory is compared with the oracle's by
digest (tests/test_full_width_digest.py's fold).
Reference: test_benchmark.py:9-43 (the driver), chess_v2.py:183-294."""
import numpy as np
import pytest

SEED = 0x6E0
BOARDS = (1, 64, 65, 129, 193, 257, 321)
PRIME = np.uint64(0x100000001B3)


def fold(d, w):
    """d = (d ^ w) * PRIME elementwise, uint64 wrap-around (oracle/gc_oracle.c digest_fold)"""
    with np.errstate(over="ignore"):
        return (d ^ w) * PRIME


def launch_lengths(m):
    """pairs of launches: far below the occupancy filter's threshold, at it and just below it"""
    return (3, m, m - 1)


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's digests of the widest env's boards over the whole schedule, computed once (a
    board's trajectory depends on the seed and its index only, so a narrower env's are a prefix)"""
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(1, device=0, seed=SEED)
    m = env.rollout_occ_min_plies()
    env.close()
    assert m >= 2
    return oracle.rollout_digests(SEED, max(BOARDS), 2 * sum(launch_lengths(m)), threads=16)


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOARDS)
def test_rollout_geometry_digests_vs_oracle(want, n):
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(n, device=0, seed=SEED)
    assert env.rollout_waves() == 4  # the quad kernel, not the paired one
    m = env.rollout_occ_min_plies()
    tbs = [env.trace_buffer(m), env.trace_buffer(m)]
    d = np.zeros(n, dtype=np.uint64)
    for k in launch_lengths(m):
        for tb in tbs:  # two launches back to back: the second re-arms the completion counter
            env.rollout_device(k, tb)
        env.wait_rollout()
        env.synchronize()
        for tb in tbs:
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
