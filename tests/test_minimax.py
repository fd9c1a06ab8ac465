"""CPU: the minimax search of gc_minimax.h (what k_minimax computes per row) in its host build
(tests/core_host/minimax_host.cpp), pinned to a plain negamax without pruning over the C oracle's
get_possible_moves / next_state -- count, the whole (action, score) list, the score, the first-tie
pick and the value -- plus pruned against full-width at depth 4, the tie rule against numpy, the
value mapping bit for bit, hand positions and a sanitized stand-alone run."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import minimaxhost as MH  # noqa: E402
import oracle as O  # noqa: E402
import playout_cases as PC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATE, BAND = 30000, 128
VALUES = {2: 10, 3: 5, 4: 3, 5: 3, 6: 1}
SMALL = 6000  # depth 3 and 4 run on the boards with len(moves) * perft(2) <= SMALL

# WHITE: Kg1, Rd1; BLACK: Kg8, Qd5 (tests/test_playout_gpu.py's board).  Rxd5 (action 59 * 64 + 27)
# takes the undefended queen; WHITE has no other capture.
QUEEN_HANGS = PC.board_of({62: 1, 59: 3, 6: -1, 27: -2})
TAKE_QUEEN = 59 * 64 + 27


# --------------------------------------------------------------------------- the reference
def np_material(board, white_to_move):
    return sum(VALUES.get(abs(int(v)), 0) * (1 if (v > 0) == bool(white_to_move) else -1) for v in board if v)


def np_value(score):
    if score >= MATE - BAND:
        return np.float32(1.0)
    if score <= -(MATE - BAND):
        return np.float32(-1.0)
    return np.float32(np.float32(np.clip(score, -16, 16)) * np.float32(0.0625))


def ref_v(board, meta, d, ply, seen):
    """V(pos, d, ply) from the definition, on the oracle alone"""
    white = int(meta[0])
    moves = O.get_possible_moves(board, meta, white)
    seen["nodes"] += 1
    if not moves:
        checked = O.update_state(board, meta)[1][5 if white else 6]
        return -(MATE - ply) if checked else 0
    if d == 0:
        return np_material(board, white)
    return max(ref_e(board, meta, a, d, ply, seen) for a in moves)


def ref_e(board, meta, a, d, ply, seen):
    rc, nb, nm, _ = O.next_state(board, meta, int(meta[0]), a)
    assert rc in (0, 1)
    if rc == 1:  # both kings in check: the step ends the episode and rewards nobody
        seen["both_checked"] += 1
        return 0
    return -ref_v(nb, nm, d - 1, ply + 1, seen)


def ref_root(board, meta, depth, seen):
    """[(action, s_a)] in ascending action id"""
    return [(a, ref_e(board, meta, a, depth, 0, seen)) for a in sorted(O.get_possible_moves(board, meta, int(meta[0])))]


@pytest.fixture(scope="module")
def cases():
    boards, metas = PC.positions()
    moves = [len(O.get_possible_moves(boards[i], metas[i], int(metas[i][0]))) for i in range(len(boards))]
    small = [i for i in range(len(boards)) if moves[i] * O.perft(boards[i], metas[i], 2) <= SMALL]
    return boards, metas, moves, small


@pytest.fixture(scope="module")
def reference(cases):
    """the oracle's root lists, computed once: {depth: {board: [(action, score)]}} and what was seen"""
    boards, metas, moves, small = cases
    seen = dict(nodes=0, both_checked=0)
    ref = {d: {i: ref_root(boards[i], metas[i], d, seen) for i in (range(len(boards)) if d < 3 else small)}
           for d in (1, 2, 3)}
    return ref, seen


# --------------------------------------------------------------------------- 1. against the oracle
def test_against_the_oracle_from_the_definition(cases, reference):
    boards, metas, moves, small = cases
    ref, seen = reference
    assert len(boards) == 206
    shown = dict(mate_for=0, mate_against=0, tie=0, no_move=0, wide=0, big=0, white=0, black=0)
    for d in (1, 2, 3):
        for i, lst in ref[d].items():
            r = MH.row(boards[i], metas[i], d, board_index=i, cap=256)
            where = f"board {i} depth {d}"
            assert r["count"] == len(lst) == moves[i], where
            assert len(lst) <= 256
            assert [(int(a), int(s)) for a, s in zip(r["actions"][: len(lst)], r["scores"][: len(lst)])] == lst, where
            assert (r["actions"][len(lst):] == 0xFFFF).all() and (r["scores"][len(lst):] == MH.INT32_MIN).all(), where
            white = int(metas[i][0])
            if not lst:
                checked = metas[i][5 if white else 6]
                score, pick = (-MATE if checked else 0), 0xFFFF
                shown["no_move"] += 1
            else:
                score = max(s for _, s in lst)
                pick = [a for a, s in lst if s == score][0]
                shown["tie"] += sum(s == score for _, s in lst) > 1
            assert (r["score"], r["pick"]) == (score, pick), where
            assert r["value"].tobytes() == np_value(score).tobytes(), where
            plain = MH.row(boards[i], metas[i], d, board_index=i)  # without the list: the same row
            assert all(plain[k] == r[k] for k in ("count", "pick", "score")) and plain["value"] == r["value"], where
            assert plain["nodes"] <= r["nodes"], where
            shown["mate_for"] += score >= MATE - BAND
            shown["mate_against"] += bool(lst) and score <= -(MATE - BAND)
            shown["wide"] += len(lst) > 64
            shown["big"] += MH.big(boards[i], metas[i])
            shown["white" if white else "black"] += 1
    shown["both_checked"] = seen["both_checked"]
    assert all(shown.values()), f"the inputs must show every case: {shown}"
    print(f"oracle nodes {seen['nodes']}, {len(small)} small boards, shown {shown}")


# --------------------------------------------------------------------------- 2. pruned = full-width
def test_pruned_equals_full_width_at_depth_4(cases):
    boards, metas, _, small = cases
    pruned_nodes = full_nodes = 0
    for i in small:
        full = MH.row(boards[i], metas[i], 4, board_index=i, cap=256, prune=False)
        listed = MH.row(boards[i], metas[i], 4, board_index=i, cap=256)
        plain = MH.row(boards[i], metas[i], 4, board_index=i)
        for r in (listed, plain):
            assert all(r[k] == full[k] for k in ("count", "pick", "score")), i
            assert r["value"].tobytes() == full["value"].tobytes(), i
        assert (listed["actions"] == full["actions"]).all() and (listed["scores"] == full["scores"]).all(), i
        assert plain["nodes"] <= listed["nodes"] <= full["nodes"], i
        pruned_nodes += plain["nodes"]
        full_nodes += full["nodes"]
    print(f"depth 4 on {len(small)} boards: {pruned_nodes} nodes pruned, {full_nodes} full-width")
    assert pruned_nodes < full_nodes


# --------------------------------------------------------------------------- 3. the tie rule
def np_pick(actions, scores, count, seed, board, draw):
    """the random pick from the definition: T[i*], i* the largest i with policy_index(...) == 0"""
    lst = list(zip(actions[:count].tolist(), scores[:count].tolist()))
    best = max(s for _, s in lst)
    ties = [a for a, s in lst if s == best]
    keep = [i for i in range(len(ties)) if MH.policy_index(seed, board, draw + i, i + 1) == 0]
    return ties[max(keep)], ties


def test_policy_index_is_the_oracles():
    for seed, board, draw, n in ((0, 0, 0, 1), (31, 5, 7, 20), (2 ** 63 + 9, 2 ** 31, 2 ** 32 - 1, 218), (1, 2, 3, 4)):
        assert MH.policy_index(seed, board, draw, n) == O.policy_index(seed, board, draw, n)


def test_the_tie_rule(cases):
    boards, metas, moves, _ = cases
    checked = 0
    for i in range(len(boards)):
        if not moves[i]:
            continue
        lists = MH.row(boards[i], metas[i], 2, board_index=i, cap=256)
        for draw in (0, 3, 2 ** 32 - 2):
            r = MH.row(boards[i], metas[i], 2, seed=77, board_index=i, draw=draw)
            want, ties = np_pick(lists["actions"], lists["scores"], lists["count"], 77, i, draw)
            assert r["pick"] == want and r["score"] == lists["score"], (i, draw)
            checked += len(ties) > 1
    assert checked > 50
    # the start position at depth 1: all 20 moves tie, and the picks over 256 draws are all of them
    start = MH.row(boards[0], metas[0], 1, cap=64)
    assert start["count"] == 20 and (start["scores"][:20] == 0).all()
    picks = {MH.row(boards[0], metas[0], 1, seed=5, board_index=0, draw=d)["pick"] for d in range(256)}
    assert picks == set(start["actions"][:20].tolist())
    # keyed by the board index, not the row
    a = [MH.row(boards[0], metas[0], 1, seed=5, board_index=0, draw=d)["pick"] for d in range(32)]
    b = [MH.row(boards[0], metas[0], 1, seed=5, board_index=9, draw=d)["pick"] for d in range(32)]
    assert a != b
    both = np.stack([boards[0]] * 10), np.stack([metas[0]] * 10)
    res = MH.run(*both, [9, 0, 9], 1, seed=5, draw=4)
    assert list(res["pick"]) == [b[4], a[4], b[4]]


# --------------------------------------------------------------------------- 4. the value mapping
def test_value_mapping_bit_for_bit(cases):
    boards = cases[0]
    scores = list(range(-40, 41)) + [MATE, MATE - 1, MATE - BAND, MATE - BAND - 1, -MATE, -(MATE - 1), -(MATE - BAND),
                                     -(MATE - BAND) + 1, 103, -103, 17, -17, 16, -16]
    for s in scores:
        assert MH.value(s).tobytes() == np_value(s).tobytes(), s
    assert MH.value(103) == 1.0 and MH.value(-17) == -1.0 and MH.value(MATE - BAND - 1) == 1.0  # clamped material
    assert MH.value(8) == 0.5 and MH.value(-1) == -0.0625
    for i in range(len(boards)):
        for white in (0, 1):
            assert MH.material(boards[i], white) == np_material(boards[i], white), i
    assert max(abs(MH.material(b, 1)) for b in boards) > 16  # the material is not clamped


# --------------------------------------------------------------------------- 5. hand positions
def test_hand_positions():
    m = PC.settle(PC.MATE_IN_ONE, [1, 0, 0, 0, 0, 0, 0, 0])
    r = MH.row(PC.MATE_IN_ONE, m, 1)
    assert (r["pick"], r["score"], r["value"]) == (PC.MATE_IN_ONE_ACTION, MATE - 1, 1.0)
    m = PC.settle(QUEEN_HANGS, [1, 0, 0, 0, 0, 0, 0, 0])
    for depth in (1, 2):
        r = MH.row(QUEEN_HANGS, m, depth, cap=32)
        assert r["pick"] == TAKE_QUEEN and r["score"] == 5, depth
        assert (r["scores"][: r["count"]] == 5).sum() == 1
    m = PC.settle(PC.TWO_KINGS, [1, 0, 0, 0, 0, 0, 0, 0])
    for depth in (1, 2, 3, 4):
        r = MH.row(PC.TWO_KINGS, m, depth, cap=16)
        assert r["score"] == 0 and r["value"] == 0.0 and (r["scores"][: r["count"]] == 0).all()
    done = MH.row(PC.TWO_KINGS, m, 2, cap=4, done=True)
    assert done["skipped"] and (done["count"], done["pick"], done["score"], done["nodes"]) == (0, 0xFFFF, 0, 0)
    assert (done["actions"] == 0xFFFF).all() and (done["scores"] == MH.INT32_MIN).all()


# --------------------------------------------------------------------------- 6. sanitized
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_minimax_under_asan_ubsan(tmp_path):
    """the host minimax over seeded fuzz boards as a stand-alone sanitized program
    (tests/core_host/minimax_sanitize_main.cpp)"""
    exe = tmp_path / "minimax_sanitize"
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-o", str(exe),
                    os.path.join(ROOT, "tests", "core_host", "minimax_sanitize_main.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "40"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "fails 0" in r.stdout
