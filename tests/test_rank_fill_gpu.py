"""The rank fills by carry propagation on the device: the fused rollouts (both variants of the
quad kernel, whose Q2 / Q3 carry the fills' operands across a barrier), the paired kernel and
the perft leaf from a start position crowded with rooks and queens, against the oracle."""
import numpy as np
import pytest

from test_rank_fill import HEAVY_BOARD

pytestmark = pytest.mark.gpu

N = 128  # one workgroup of the quad kernel: two quads
NAMES = ("action", "reward", "done", "reason")


def test_heavy_board_is_a_quad_start_position():
    ib = HEAVY_BOARD
    assert (ib == 1).sum() == 1 and (ib == -1).sum() == 1
    assert 0 < (ib > 0).sum() <= 16 and 0 < (ib < 0).sum() <= 16
    assert ((np.abs(ib) == 2) | (np.abs(ib) == 3)).sum() >= 16  # rooks and queens


@pytest.fixture(scope="module")
def heavy_refs(oracle):
    """the oracle driver's traces of the N boards from HEAVY_BOARD, one ply past the longest launch"""
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(N, device=0, seed=4242, initial_board=HEAVY_BOARD)
    m = env.rollout_occ_min_plies()
    env.close()
    return m, [oracle.rollout_trace(4242, i, m + 1, init=HEAVY_BOARD) for i in range(N)]


@pytest.mark.parametrize("variant", ["below", "at"])
def test_fused_rollout_heavy_board_vs_oracle(oracle, heavy_refs, variant):
    """k_env_rollout4<false> (a launch of m - 1 plies) and <true> (m plies: the occupancy filter)
    with a device trace: every ply's action / reward / done / reason, the next action and the
    final states."""
    from gym_chess_amd.env import BatchedChessEnv

    m, refs = heavy_refs
    plies = m - 1 if variant == "below" else m
    assert plies >= 1
    env = BatchedChessEnv(N, device=0, seed=4242, initial_board=HEAVY_BOARD)
    assert env.rollout_waves() == 4
    buf = env.trace_buffer(plies)
    env.rollout_device(plies, trace=buf)
    tr = buf.fetch()
    buf.close()
    for name in NAMES:
        want = np.stack([r[name][:plies] for r in refs], axis=1)
        bad = np.argwhere(tr[name] != want)
        assert bad.size == 0, (variant, name, bad[:4].tolist())
    nxt = np.array([0xFFFF if r["action"][plies] < 0 else r["action"][plies] for r in refs], dtype=np.uint16)
    assert (env.outputs()["next_action"] == nxt).all(), variant
    b, mt = env.boards()
    env.close()
    for i in range(N):
        fin = oracle.rollout_trace(4242, i, plies, init=HEAVY_BOARD)
        assert (b[i] == fin["final_board"]).all() and list(mt[i]) == list(fin["final_meta"]), (variant, i)


def test_paired_rollout_random_opponent_heavy_board_vs_oracle(oracle):
    """the paired kernel (opponent="random"), 300 plies: every ply against the oracle's trace"""
    from gym_chess_amd.env import BatchedChessEnv

    plies, seed = 300, 777
    env = BatchedChessEnv(N, device=0, seed=seed, initial_board=HEAVY_BOARD, opponent="random")
    assert env.paired()
    _, tr = env.rollout(plies, trace=True)
    b, mt = env.boards()
    env.close()
    for i in range(N):
        ref = oracle.rollout_trace(seed, i, plies, init=HEAVY_BOARD, opponent=1, agent_white=True)
        for name in NAMES:
            bad = np.nonzero(tr[name][:, i] != ref[name])[0]
            assert bad.size == 0, (i, name, bad[:4].tolist())
        assert (b[i] == ref["final_board"]).all() and list(mt[i]) == list(ref["final_meta"]), i


def test_perft3_heavy_board_vs_oracle(oracle, engine):
    b = HEAVY_BOARD[None]
    m = oracle.make_meta()[None]
    ref = oracle.perft_by_children(b, m, 3, threads=4)
    assert (engine.perft(b, m, 3) == ref).all(), (engine.perft(b, m, 3), ref)
    # and from the other side, with enough roots to fill a wave
    mb = oracle.make_meta(False)[None]
    refb = int(oracle.perft_by_children(b, mb, 3, threads=4)[0])
    assert (engine.perft(np.tile(b, (64, 1)), np.tile(mb, (64, 1)), 3) == refb).all()
