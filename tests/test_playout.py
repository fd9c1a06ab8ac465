"""CPU: the playout body of gc_playout.h (what k_playout runs per lane) in its host build
(tests/core_host/playout_host.cpp), pinned to the C oracle move by move -- every action legal
where it is played, the oracle's first `done` at the playout's last ply and for its reason, none
before -- plus the pick rule against the existing self-play driver, the value formula and the
material term against numpy, and a sanitized stand-alone run.

The oracle env always starts with WHITE to move, so the oracle-pinned playouts start from the
shared positions with WHITE to move; the GPU suite runs both sides against this host build."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
import corehost as CH  # noqa: E402
import playout_cases as PC  # noqa: E402
import playouthost as PH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, PLIES, SEED = 8, 48, 31
WIN, LOSS, OTHER, CUT = range(4)
R_MATE, R_REPETITION, R_BOTH_CHECKED = 1, 2, 5
VALUES = {2: 10, 3: 5, 4: 3, 5: 3, 6: 1}


def np_material(board, own_white):
    """clamp(sum of value * (own - enemy), -16, 16) from a mailbox board"""
    d = sum(VALUES.get(abs(int(v)), 0) * (1 if (v > 0) == bool(own_white) else -1) for v in board if v)
    return int(np.clip(d, -16, 16))


def np_value(tally, cut_weight, playouts):
    t = np.asarray(tally, dtype=np.int64)
    cut = np.float32(cut_weight) * (np.float32(t[4]) * np.float32(0.0625))
    return np.float32((np.float32(t[0] - t[1]) + np.float32(cut)) / np.float32(playouts))


@pytest.fixture(scope="module")
def white_rows():
    """the shared positions with WHITE to move and every row's host playouts (computed once)"""
    boards, metas = PC.positions(side=1)
    rows = [PH.row(boards[i], metas[i], SEED, i * P, P, PLIES) for i in range(len(boards))]
    return boards, metas, rows


def test_playouts_against_the_oracle(white_rows):
    from oracle_engine import OracleBoard

    boards, metas, rows = white_rows
    seen = dict(win=0, loss=0, repetition=0, no_move=0, cut=0)
    for i, r in enumerate(rows):
        for p in range(P):
            kind, plies, m = (int(x) for x in r["ends"][p])
            acts, why = r["actions"][p], r["reasons"][p]
            assert (acts[:plies] >= 0).all() and (acts[plies:] == -1).all()
            ob = OracleBoard()
            rec = ob.set_state(boards[i], metas[i][1:7])
            done, reason = False, 0
            for t in range(plies):
                assert not done, f"board {i} playout {p}: the oracle is done before ply {t}"
                legal = rec["moves"][: rec["nmoves"]]
                assert acts[t] in legal, f"board {i} playout {p} ply {t}: action {acts[t]} is not legal"
                rec = ob.call(1, int(acts[t]))
                done = bool(rec["done"]) or int(rec["status"]) == 1
                reason = R_BOTH_CHECKED if int(rec["status"]) == 1 else int(rec["reason"])
                assert reason == int(why[t]), f"board {i} playout {p} ply {t}: reason {why[t]}, the oracle's {reason}"
            where = f"board {i} playout {p}: {PH.KINDS[kind]} after {plies} plies"
            if kind in (WIN, LOSS):
                assert done and reason == R_MATE, where
                assert kind == (WIN if (plies - 1) % 2 == 0 else LOSS), where
                seen["win" if kind == WIN else "loss"] += 1
            elif kind == CUT:
                assert not done and plies == PLIES, where
                assert m == np_material(rec["board"], True), where
                seen["cut"] += 1
            elif done:  # another ending of the step
                assert reason not in (0, R_MATE), where
                seen["repetition"] += reason == R_REPETITION
            else:  # no legal move: nothing picked, nothing played
                assert plies < PLIES and rec["nmoves"] == 0, where
                seen["no_move"] += 1
            assert kind == CUT or m == 0
    assert all(seen.values()), f"the inputs must show every ending: {seen}"


def test_tally_and_value(white_rows):
    boards, metas, rows = white_rows
    for i, r in enumerate(rows):
        ends = r["ends"]
        t = [int((ends[:, 0] == k).sum()) for k in range(4)] + [int(ends[:, 2].sum()), int(ends[:, 1].sum())]
        assert list(r["tally"]) == t, i
        assert r["value"].tobytes() == np_value(t, 1.0, P).tobytes(), i
        assert -1.0 <= r["value"] <= 1.0
    for cw in (0.0, 0.37, 1.0):  # the formula alone, over tallies no playout need reach
        for w, l, ms, n in ((3, 1, 37, 8), (0, 0, -64, 4), (0, 5, 1, 8), (1, 0, 0, 1), (20, 3, -333, 64)):
            assert PH.value(w, l, ms, cw, n).tobytes() == np_value([w, l, 0, 0, ms, 0], cw, n).tobytes()
    for i in range(len(boards)):
        for white in (0, 1):
            assert PH.material(boards[i], white) == np_material(boards[i], white), i


def test_the_one_move_that_mates():
    b = PC.MATE_IN_ONE
    m = PC.settle(b, [1, 0, 0, 0, 0, 0, 0, 0])
    assert CH.get_list(b, m, 1) == [PC.MATE_IN_ONE_ACTION]
    r = PH.row(b, m, 5, 0, P, PLIES, cut_weight=0.25)
    assert list(r["tally"]) == [P, 0, 0, 0, 0, P]
    assert r["value"].tobytes() == np.float32(1.0).tobytes()
    assert (r["actions"][:, 0] == PC.MATE_IN_ONE_ACTION).all()


def test_pick_rule_against_the_selfplay_driver():
    """rank policy_index(seed, L, draw + t, n), the k-th in move-set order: the same actions as the
    host self-play driver's set-wise pick (corehost.HostEnv) on the lane's stream, ply after ply"""
    boards, _ = PC.positions(side=1)
    checked = 0
    for i in range(len(boards)):
        m = PC.settle(boards[i], [1, 1, 1, 1, 1, 0, 0, 0])  # as the driver's reset: all rights, forced
        lane = 1000 + i
        r = PH.row(boards[i], m, SEED, lane, 1, 6)
        he = CH.HostEnv(boards[i], seed=SEED, board=lane)
        for t in range(int(r["ends"][0][1])):
            a = he.pick()
            assert a == r["actions"][0][t], (i, t)
            assert he.draw == t + 1
            he.step(a)
            checked += 1
        if r["ends"][0][1] == 0:
            assert he.pick() == -1
    assert checked > 500
    # `draw` is where the lane's counter starts: the driver's t-th pick at the start position is
    # the first pick of a run at draw = t
    b, m = boards[0], PC.settle(boards[0], [1, 1, 1, 1, 1, 0, 0, 0])
    firsts = [int(PH.row(b, m, SEED, 3, 1, 1, draw=d)["actions"][0][0]) for d in range(40)]
    he = CH.HostEnv(b, seed=SEED, board=3)
    assert firsts == [he.pick() for _ in range(40)]  # (pick() draws without stepping)
    assert len(set(firsts)) > 5


def test_skipped_and_short_rows():
    boards, metas = PC.positions()
    r = PH.row(boards[0], metas[0], 1, 0, P, PLIES, done=True)
    assert r["skipped"] and not r["tally"].any() and r["value"] == 0.0
    r = PH.row(boards[0], metas[0], 1, 0, 4, 3)
    assert list(r["tally"]) == [0, 0, 0, 4, int(r["ends"][:, 2].sum()), 12]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_playout_body_under_asan_ubsan(tmp_path):
    """the host playout body over seeded fuzz boards as a stand-alone sanitized program
    (tests/core_host/playout_sanitize_main.cpp)"""
    exe = tmp_path / "playout_sanitize"
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-o", str(exe),
                    os.path.join(ROOT, "tests", "core_host", "playout_sanitize_main.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "fails 0" in r.stdout
