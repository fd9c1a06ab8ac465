"""configs[3] at full width: bench.py's 65 536 mid-game perft roots,
every root's perft(4) and every 64th root's perft(5) pinned by the oracle
(tests/golden/configs3_perft_*.npz, made by tests/golden/make_perft_roots.py: the roots
regenerated from the oracle's restatement of the random self-play driver, the counts by the
oracle's perft = lib.rs:460-486 move lists composed with lib.rs:679-784 next_state).

CPU: the fixture's roots are the oracle's (a strided sample regenerated), a few perft(4)
values recomputed.  GPU: the device's roots (bench.midgame_fens, the bench's own code path)
equal the fixture's, and the device's perft(4) of all 65 536 roots and perft(5) on the stride
equal the fixture's -- so the bench line's 2.55e12-node total is pinned root by root at depth 4
and on 1 024 roots at depth 5 (the bench leg repeats that check, bench.py perft_leg)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


@pytest.fixture(scope="module")
def fixture():
    import make_perft_roots as M

    return M.load()  # plain arrays (allow_pickle stays False)


def test_fixture_shape(fixture):
    assert fixture["boards"].shape == (65536, 64) and fixture["metas"].shape == (65536, 8)
    assert fixture["perft4"].shape == (65536,) and (fixture["perft4"] > 0).all()
    assert (fixture["stride5"] == np.arange(0, 65536, 64)).all() and fixture["perft5"].shape == (1024,)
    # the depth-5 stride against depth 4: a mid-game position's branching factor
    r = fixture["perft5"].astype(np.float64) / fixture["perft4"][fixture["stride5"]]
    assert 5 < np.median(r) < 60


def test_fixture_roots_are_the_oracles(oracle, fixture):
    import make_perft_roots as M

    idx = np.arange(0, 65536, 257)
    ply = M.root_plies()
    for i in idx:
        r = oracle.rollout_trace(M.SEED, int(i), int(ply[i]))
        m = np.zeros(8, np.uint8)
        m[:5] = r["final_meta"][:5]
        b, mm = oracle.update_state(r["final_board"], m)
        assert (b == fixture["boards"][i]).all() and list(mm[:7]) == list(fixture["metas"][i, :7]), int(i)
    sub = np.arange(0, 65536, 8192)
    got = oracle.perft_batch(fixture["boards"][sub], fixture["metas"][sub], 4, threads=min(8, os.cpu_count() or 1))
    assert (got == fixture["perft4"][sub]).all()


@pytest.mark.gpu
def test_configs3_roots_and_perft_full_width_vs_fixture(fixture):
    sys.path.insert(0, ROOT)
    import bench
    from gym_chess_amd.engine import Engine
    from gym_chess_amd.fen import fen_to_arrays

    fens = bench.midgame_fens(65536, 0x5EED + 4, 0)  # bench.perft_leg's roots (replica 0)
    arr = [fen_to_arrays(f) for f in fens]
    b = np.stack([a[0] for a in arr])
    m = np.stack([a[1] for a in arr])
    eng = Engine(0)
    b, m = eng.update_state(b, m)
    bad = np.nonzero((b != fixture["boards"]).any(axis=1) | (m[:, :7] != fixture["metas"][:, :7]).any(axis=1))[0]
    assert len(bad) == 0, f"roots differ from the oracle's at {bad[:8]}"
    p4 = eng.perft(b, m, 4)
    bad = np.nonzero(p4 != fixture["perft4"])[0]
    assert len(bad) == 0, f"perft(4) differs at roots {bad[:8]}"
    p5 = eng.perft(b, m, 5)
    s5 = fixture["stride5"]
    bad = s5[np.nonzero(p5[s5] != fixture["perft5"])[0]]
    assert len(bad) == 0, f"perft(5) differs at roots {bad[:8]}"
    print(f"perft(4) of 65536 roots: {int(p4.sum())} nodes equal; perft(5) of {len(s5)} roots: "
          f"{int(p5[s5].sum())} equal; device total perft(5) {int(p5.sum())}")
    eng.close()
