"""CPU: the minimax search with a quiescence search at the leaves (gc_minimax.h's mm_qs under
minimax_row, what k_minimax<NODES, true> computes per row) in its host build
(tests/core_host/quiesce_host.cpp), pinned to a plain QS / V written from include/gymchess.h's
definition over the C oracle's get_possible_moves / next_state / update_state -- count, the whole
(action, score) list, the score, the first-tie pick and the value -- plus quiesce=0 against the
plain host build, pruned against full-width (depth 2 on the boards of the oracle comparison, depth
3 and 4 on a narrower set: see DEEP_SMALL), hand positions, the tie rule and a sanitized run."""
import ctypes
import multiprocessing as mp
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
import quiescehost as QH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATE, BAND = 30000, 128
VALUES = {2: 10, 3: 5, 4: 3, 5: 3, 6: 1}
# depth 2 runs on the boards with len(moves) * perft(2) <= SMALL: the median of that product over
# the 206 boards is 1947, so this keeps a little over half of them (asserted below)
SMALL = 2000
# Pruned against full-width at depth 3 / 4 with quiesce 4 does NOT run on all of the SMALL boards: a
# full-width tree with four capture plies below it grows with the men that can take each other, not
# with perft -- the 64 smallest of them by that product already hold 81 M full-width positions at
# depth 3 (50 s of one core), and depth 4 is far beyond that.  It runs on a narrower set, bounded by
# both DEEP_SMALL and DEEP_PIECES men on the board (39 boards, 13.9 M full-width positions at
# depth 4, about 10 s), and the test asserts that the quiescence nest is at work there: on most
# of those boards quiesce 4 visits more positions than quiesce 0.  Depth 2 / quiesce 4 does run
# pruned against full-width on every SMALL board.
DEEP_SMALL, DEEP_PIECES = 1000, 12


def sq(name):
    """'e4' -> row * 8 + col, row 0 = rank 8"""
    return (8 - int(name[1])) * 8 + "abcdefgh".index(name[0])


def mv(a, b):
    return sq(a) * 64 + sq(b)


def hand(pieces, white=1):
    b = PC.board_of({sq(k): v for k, v in pieces.items()})
    return b, PC.settle(b, [white, 0, 0, 0, 0, 0, 0, 0])


DEFENDED_MEN = {"g1": 1, "d1": 2, "g8": -1, "f7": -6, "g7": -6, "h7": -6, "d5": -6, "e6": -6}
DEFENDED_PAWN = hand(DEFENDED_MEN)
QXD5 = mv("d1", "d5")


# --------------------------------------------------------------------------- the reference
def np_material(board, white_to_move):
    return sum(VALUES.get(abs(int(v)), 0) * (1 if (v > 0) == bool(white_to_move) else -1) for v in board if v)


def np_value(score):
    if score >= MATE - BAND:
        return np.float32(1.0)
    if score <= -(MATE - BAND):
        return np.float32(-1.0)
    return np.float32(np.float32(np.clip(score, -16, 16)) * np.float32(0.0625))


# the oracle's get_possible_moves / next_state as oracle.py calls them, without its per-call
# conversions: QS visits a few million positions here.  MATERIAL: white's view by piece byte.
MATERIAL = np.zeros(256, dtype=np.int64)
for _id, _v in VALUES.items():
    MATERIAL[_id], MATERIAL[256 - _id] = _v, -_v
_MOVES = np.zeros(1024, dtype=np.uint16)
_VP = ctypes.c_void_p


def fast_moves(board, meta, white):
    """O.get_possible_moves as an int64 array (a copy)"""
    n = O.lib().oracle_get_possible_moves(_VP(board.ctypes.data), _VP(meta.ctypes.data), white, 0,
                                          _VP(_MOVES.ctypes.data), 1024)
    return _MOVES[:n].astype(np.int64)


def fast_next(board, meta, white, action):
    """O.next_state -> (rc, board, meta)"""
    ob, om, rw = np.empty(64, dtype=np.int8), np.zeros(8, dtype=np.uint8), ctypes.c_int(0)
    rc = O.lib().oracle_next_state(_VP(board.ctypes.data), _VP(meta.ctypes.data), white, action, _VP(ob.ctypes.data),
                                   _VP(om.ctypes.data), ctypes.byref(rw))
    return rc, ob, om


SEEN = ("nodes", "both_checked", "both_checked_qs", "stand_pat", "leaf_in_check", "mate_in_qs", "cutoff", "king_capture")


class Ref:
    """V / QS from the definition on the oracle alone, full-width.  QS(pos, q, ply) is kept per
    (position, q, ply): capture sequences transpose, and the value is a function of exactly that"""

    def __init__(self):
        self.seen = dict.fromkeys(SEEN, 0)
        self.memo = {}

    def qs(self, board, meta, q, ply, leaf=False):
        """leaf: the position is the depth-0 leaf itself (ply == depth), not one below it"""
        key = (board.tobytes(), meta[:7].tobytes(), q, ply)
        if key not in self.memo:
            self.memo[key] = self._qs(board, meta, q, ply, leaf)
        return self.memo[key]

    def _qs(self, board, meta, q, ply, leaf):
        white = int(meta[0])
        moves = fast_moves(board, meta, white)
        self.seen["nodes"] += 1
        if not len(moves):  # rule 1
            checked = O.update_state(board, meta)[1][5 if white else 6]
            self.seen["mate_in_qs"] += bool(checked) and not leaf  # ply > depth: the plain search never sees it
            return -(MATE - ply) if checked else 0
        stand = int(MATERIAL[board.view(np.uint8)].sum()) * (1 if white else -1)
        if q == 0 and self.seen["cutoff"]:  # rule 2 (most positions end here: nothing more is computed)
            return stand
        hit = board[moves & 63]
        captures = moves[(moves < 4096) & (hit != 0) & ((hit > 0) != bool(white))]
        if q == 0:  # rule 2, until one cut-off has left a capture unsearched
            self.seen["cutoff"] += len(captures) > 0
            return stand
        if O.update_state(board, meta)[1][5 if white else 6]:  # rule 3: every evasion, no stand-pat
            self.seen["leaf_in_check"] += 1
            return max(self.eq(board, meta, int(a), q, ply) for a in moves)
        self.seen["king_capture"] += bool((np.abs(board[captures & 63]) == 1).any())
        best = max([stand] + [self.eq(board, meta, int(a), q, ply) for a in captures])  # rule 4
        self.seen["stand_pat"] += len(captures) > 0 and best == stand
        return best

    def eq(self, board, meta, a, q, ply):
        rc, nb, nm = fast_next(board, meta, int(meta[0]), a)
        assert rc in (0, 1)
        if rc == 1:
            self.seen["both_checked_qs"] += 1
            return 0
        return -self.qs(nb, nm, q - 1, ply + 1)

    def v(self, board, meta, d, q, ply):
        if d == 0:
            return self.qs(board, meta, q, ply, leaf=True)  # (rule 1 is QS's first rule too)
        white = int(meta[0])
        moves = O.get_possible_moves(board, meta, white)
        self.seen["nodes"] += 1
        if not moves:
            checked = O.update_state(board, meta)[1][5 if white else 6]
            return -(MATE - ply) if checked else 0
        return max(self.e(board, meta, a, d, q, ply) for a in moves)

    def e(self, board, meta, a, d, q, ply):
        rc, nb, nm, _ = O.next_state(board, meta, int(meta[0]), a)
        assert rc in (0, 1)
        if rc == 1:  # both kings in check: the step ends the episode and rewards nobody
            self.seen["both_checked"] += 1
            return 0
        return -self.v(nb, nm, d - 1, q, ply + 1)

    def root(self, board, meta, depth, q):
        """[(action, s_a)] in ascending action id"""
        return [(a, self.e(board, meta, a, depth, q, 0)) for a in sorted(O.get_possible_moves(board, meta, int(meta[0])))]


_POOL = {}  # the parent sets "cases" before it forks; a worker keeps its own "ref"


def _ref_task(task):
    """(a pool worker) the reference's root list of one (depth, quiesce, board) and what it saw there"""
    d, q, i = task
    ref = _POOL.setdefault("ref", Ref())
    before = dict(ref.seen)
    boards, metas = _POOL["cases"]
    lst = ref.root(boards[i], metas[i], d, q)
    return task, lst, {k: ref.seen[k] - before[k] for k in SEEN}


@pytest.fixture(scope="module")
def cases():
    boards, metas = PC.positions()
    n = len(boards)
    moves = [len(O.get_possible_moves(boards[i], metas[i], int(metas[i][0]))) for i in range(n)]
    size = [moves[i] * O.perft(boards[i], metas[i], 2) for i in range(n)]
    small = [i for i in range(n) if size[i] <= SMALL]
    deep = [i for i in range(n) if size[i] <= DEEP_SMALL and int((boards[i] != 0).sum()) <= DEEP_PIECES]
    return boards, metas, moves, small, deep


def check_row(r, lst, where):
    """the host row r (cap 256) against the reference's root list"""
    assert r["count"] == len(lst) <= 256, where
    assert [(int(a), int(s)) for a, s in zip(r["actions"][: len(lst)], r["scores"][: len(lst)])] == lst, where
    assert (r["actions"][len(lst):] == 0xFFFF).all() and (r["scores"][len(lst):] == QH.INT32_MIN).all(), where
    score = max(s for _, s in lst)
    pick = [a for a, s in lst if s == score][0]
    assert (r["score"], r["pick"]) == (score, pick), where
    assert r["value"].tobytes() == np_value(score).tobytes(), where
    return score


# --------------------------------------------------------------------------- 1. against the oracle
def test_against_the_oracle_from_the_definition(cases):
    boards, metas, moves, small, _ = cases
    assert len(boards) == 206
    assert 2 * len(small) >= len(boards), "the depth-2 bound must leave at least half of the boards in"
    shown = dict(differs=0, wide=0, no_move=0, mate_for=0, mate_against=0)
    runs = ((2, 4, small), (1, 4, range(len(boards))), (1, 2, range(len(boards))), (2, 1, small),
            (1, 1, range(len(boards))))  # (the longest first: the pool's tail is short)
    # the reference's root lists: 5.3 M oracle positions, minutes of one core, so the boards are dealt
    # to processes (each its own Ref; what they saw is summed)
    _POOL["cases"] = (boards, metas)
    tasks = [(d, q, i) for d, q, rows in runs for i in rows if moves[i]]
    seen = dict.fromkeys(SEEN, 0)
    lists = {}
    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        for key, lst, saw in pool.imap_unordered(_ref_task, tasks, chunksize=1):
            lists[key] = lst
            for k in SEEN:
                seen[k] += saw[k]
    for d, q, rows in runs:
        for i in rows:
            where = f"board {i} depth {d} quiesce {q}"
            r = QH.row(boards[i], metas[i], d, q, board_index=i, cap=256)
            plain = QH.row(boards[i], metas[i], d, q, board_index=i)  # without the list: the same row
            assert all(plain[k] == r[k] for k in ("count", "pick", "score")) and plain["value"] == r["value"], where
            assert plain["nodes"] <= r["nodes"], where
            if not moves[i]:
                checked = metas[i][5 if metas[i][0] else 6]
                assert (r["count"], r["pick"], r["score"]) == (0, 0xFFFF, -MATE if checked else 0), where
                assert r["value"].tobytes() == np_value(r["score"]).tobytes(), where
                shown["no_move"] += 1
                continue
            score = check_row(r, lists[d, q, i], where)
            base = QH.row(boards[i], metas[i], d, 0, board_index=i, cap=256)
            shown["differs"] += int((base["scores"] != r["scores"]).any())
            shown["wide"] += moves[i] > 64
            shown["mate_for"] += score >= MATE - BAND
            shown["mate_against"] += score <= -(MATE - BAND)
    shown.update({k: seen[k] for k in SEEN if k not in ("both_checked", "king_capture")})
    print(f"{len(small)} boards at depth 2, oracle positions {seen['nodes']}, shown {shown}")
    assert all(shown.values()), f"the inputs must show every case: {shown}"


# --------------------------------------------------------------------------- 2. quiesce=0 is today's search
def test_quiesce_0_is_the_plain_search(cases):
    boards, metas = cases[0], cases[1]
    for i in range(len(boards)):
        for d in (1, 2, 3):
            for kw in (dict(cap=0), dict(cap=256), dict(cap=8, seed=77, draw=5)):
                a = QH.row(boards[i], metas[i], d, 0, board_index=i, **kw)
                b = MH.row(boards[i], metas[i], d, board_index=i, **kw)
                assert all(a[k] == b[k] for k in ("count", "pick", "score", "nodes", "skipped")), (i, d, kw)
                assert a["value"].tobytes() == b["value"].tobytes(), (i, d, kw)
                if kw["cap"]:
                    assert (a["actions"] == b["actions"]).all() and (a["scores"] == b["scores"]).all(), (i, d, kw)
    with pytest.raises(ValueError):
        QH.row(boards[0], metas[0], 1, 5)
    with pytest.raises(ValueError):
        QH.row(boards[0], metas[0], 1, -1)


# --------------------------------------------------------------------------- 3. pruned = full-width
def test_pruned_equals_full_width(cases):
    boards, metas, moves, small, deep = cases
    assert len(deep) >= 32
    for depth, rows in ((2, small), (3, deep), (4, deep)):
        pruned_nodes = full_nodes = deeper = 0
        for i in rows:
            full = QH.row(boards[i], metas[i], depth, 4, board_index=i, cap=256, prune=False)
            deeper += full["nodes"] > QH.row(boards[i], metas[i], depth, 0, board_index=i, prune=False)["nodes"]
            listed = QH.row(boards[i], metas[i], depth, 4, board_index=i, cap=256)
            plain = QH.row(boards[i], metas[i], depth, 4, board_index=i)
            for r in (listed, plain):
                assert all(r[k] == full[k] for k in ("count", "pick", "score")), (depth, i)
                assert r["value"].tobytes() == full["value"].tobytes(), (depth, i)
            assert (listed["actions"] == full["actions"]).all() and (listed["scores"] == full["scores"]).all(), (depth, i)
            assert plain["nodes"] <= listed["nodes"] <= full["nodes"], (depth, i)
            pruned_nodes += plain["nodes"]
            full_nodes += full["nodes"]
        print(f"depth {depth} quiesce 4 on {len(rows)} boards: {pruned_nodes} nodes pruned, {full_nodes} full-width, "
              f"{deeper} boards on which quiescence searched below a leaf")
        assert pruned_nodes < full_nodes
        assert 3 * deeper >= 2 * len(rows), "the boards must exercise the quiescence levels"


# --------------------------------------------------------------------------- 4. hand positions
def by_action(r):
    return dict(zip(r["actions"][: r["count"]].tolist(), r["scores"][: r["count"]].tolist()))


def test_hand_positions():
    ref = Ref()

    def rows(board, meta, depth, qs):
        out = {}
        for q in qs:
            out[q] = QH.row(board, meta, depth, q, cap=128)
            if q:
                check_row(out[q], ref.root(board, meta, depth, q), f"depth {depth} quiesce {q}")
        return out

    # Defended pawn.  WHITE Kg1 Qd1, BLACK Kg8 behind pawns f7 g7 h7 (no queen move checks it) with
    # pawns d5 and e6: e6 defends d5, and Qxd5 is WHITE's only capture.  The material is 10 - 5 = 5.
    # At the horizon Qxd5 wins a pawn (6); one ply further exd5 takes the queen (5 + 1 - 10 = -4),
    # and every quiet move keeps 5: no pawn attacks a square the queen reaches.
    b, m = DEFENDED_PAWN
    r = rows(b, m, 1, (0, 1, 2, 4))
    assert (r[0]["pick"], r[0]["score"]) == (QXD5, 6)
    for q in (1, 2, 4):
        assert by_action(r[q])[QXD5] == 5 + 1 - 10, q
        assert r[q]["pick"] != QXD5 and r[q]["score"] == 5, q

    # Losing capture only.  The same men with BLACK to move: after the quiet Kg8-h8 WHITE's only
    # capture is the losing Qxd5, so QS is the stand-pat and the move scores -5 -- once QS sees the
    # recapture: quiesce 1 stops on Qxd5 (the q == 0 cut-off) and still believes in the pawn.
    b, m = hand(DEFENDED_MEN, white=0)
    r = rows(b, m, 1, (0, 1, 2, 3, 4))
    assert [by_action(r[q])[mv("g8", "h8")] for q in (0, 1, 2, 3, 4)] == [-5, -6, -5, -5, -5]

    # Capture chain on d4.  WHITE Kg1 Qd4 Bb2, BLACK Kg8 Rd7 Rd8; after the quiet Kg1-h1 BLACK to move
    # stands at -3.  Rxd4 wins the queen (+10), Bxd4 the rook (-5), the second rook the bishop (+3):
    # one capture ply sees 7, two see 2, three see 5, and nothing can take after that.
    b, m = hand({"g1": 1, "d4": 2, "b2": 4, "g8": -1, "d7": -3, "d8": -3})
    r = rows(b, m, 1, (0, 1, 2, 3, 4))
    assert [by_action(r[q])[mv("g1", "h1")] for q in (0, 1, 2, 3, 4)] == [3, -7, -2, -5, -5]

    # Mate past the leaf.  WHITE Kg1 Re4 Qe1, BLACK Kh8 Ra8 with pawns g7 h7.  Re8+ at the leaf leaves
    # BLACK in check (rule 3) with Rxe8 its one evasion, and Qxe8 is a capture that mates: BLACK has
    # no move at ply 3 > depth 1.  quiesce 1 stops after Rxe8 and counts the lost rook.
    b, m = hand({"g1": 1, "e4": 3, "e1": 2, "h8": -1, "a8": -3, "g7": -6, "h7": -6})
    r = rows(b, m, 1, (0, 1, 2, 4))
    for q in (2, 4):
        assert (r[q]["pick"], r[q]["score"], r[q]["value"]) == (mv("e4", "e8"), MATE - 3, 1.0), q
    assert by_action(r[0])[mv("e4", "e8")] == 8 and by_action(r[1])[mv("e4", "e8")] == 8 - 5
    assert r[1]["score"] < MATE - BAND

    # King capture.  WHITE has two kings, a1 (the tracked one: the lowest file of the highest row) and
    # d1, pawns a2 b2 h2; BLACK Kh8 Rd8.  After h2-h3 the rook takes the king on d1 -- a capture, worth
    # 0 -- and that mates the king on a1 (b1 is the rook's): -(MATE - 2).  Without the b2 pawn the king
    # steps to b2, and the capture changes no material: the score stays the stand-pat, now -3.
    b, m = hand({"a1": 1, "d1": 1, "a2": 6, "b2": 6, "h2": 6, "h8": -1, "d8": -3})
    r = rows(b, m, 1, (0, 1, 2))
    assert by_action(r[0])[mv("h2", "h3")] == -2
    assert by_action(r[1])[mv("h2", "h3")] == by_action(r[2])[mv("h2", "h3")] == -(MATE - 2)
    before = ref.seen["king_capture"]
    b, m = hand({"a1": 1, "d1": 1, "a2": 6, "h2": 6, "h8": -1, "d8": -3})
    r = rows(b, m, 1, (0, 1, 2))
    assert by_action(r[0])[mv("h2", "h3")] == -3 and by_action(r[1])[mv("h2", "h3")] == -3
    assert ref.seen["king_capture"] > before > 0


# --------------------------------------------------------------------------- 5. the tie rule
def test_the_tie_rule_with_quiescence(cases):
    boards, metas, moves = cases[0], cases[1], cases[2]
    checked = 0
    for i in range(0, len(boards), 4):
        if not moves[i]:
            continue
        lists = QH.row(boards[i], metas[i], 1, 2, board_index=i, cap=256)
        lst = list(zip(lists["actions"][: lists["count"]].tolist(), lists["scores"][: lists["count"]].tolist()))
        ties = [a for a, s in lst if s == lists["score"]]
        for draw in (0, 3, 2 ** 32 - 2):
            keep = [k for k in range(len(ties)) if O.policy_index(77, i, (draw + k) & 0xFFFFFFFF, k + 1) == 0]
            r = QH.row(boards[i], metas[i], 1, 2, seed=77, board_index=i, draw=draw)
            assert r["pick"] == ties[max(keep)] and r["score"] == lists["score"], (i, draw)
        checked += len(ties) > 1
    assert checked > 10
    assert QH.policy_index(31, 5, 7, 20) == O.policy_index(31, 5, 7, 20)


# --------------------------------------------------------------------------- 6. sanitized
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_quiesce_under_asan_ubsan(tmp_path):
    """the host search with quiescence over seeded fuzz boards as a stand-alone sanitized program
    (tests/core_host/quiesce_sanitize_main.cpp)"""
    exe = tmp_path / "quiesce_sanitize"
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-o", str(exe),
                    os.path.join(ROOT, "tests", "core_host", "quiesce_sanitize_main.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "24"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "fails 0" in r.stdout


# --------------------------------------------------------------------------- 7. the binding
def test_the_binding_takes_quiesce():
    import inspect

    sys.path.insert(0, os.path.join(ROOT, "gym-chess_amd"))
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    assert inspect.signature(BatchedChessEnv.minimax).parameters["quiesce"].default == 0
    assert len(_lib.SIGNATURES["gc_env_minimax_q"][1]) == len(_lib.SIGNATURES["gc_env_minimax"][1]) + 1
