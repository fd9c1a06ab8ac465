"""The oracle and the host build of the kernels' core pinned to the reference's own v1 engine on
fuzzed boards (CPU only): tests/golden/v1_fuzz.json.gz, made by tests/golden/make_v1_fuzz.py
from gym_chess/envs/chess_v1.py run in the build container.

Families sparse / castle / pawns / checks / late (the generator's header says what each holds);
every position has one king per side, passes the D1/D2 filters and has its four rights all on
or all off (D3).  For EVERY listed move the fixture holds v1's next board, reward, both check
flags and the other side's move count; with the rights off also v1 perft(1..2[,3])."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
import corehost as H  # noqa: E402

FAMILIES = ("sparse", "castle", "pawns", "checks", "late")
REFERENCE = "/root/reference"


def load_fuzz():
    """[(entry, board int8[64], meta uint8[8])] of the fixture, decoded once per process"""
    if not hasattr(load_fuzz, "cache"):
        from gym_chess_amd import codec as C

        out = []
        for e in load_golden("v1_fuzz.json.gz")["positions"]:
            m = np.zeros(8, dtype=np.uint8)
            m[0] = e["white"]
            m[1:5] = e["rights"]
            out.append((e, C.text_to_board(e["board"]), m))
        load_fuzz.cache = out
    return load_fuzz.cache


def is_q1_jump(board, a):
    """a pawn double push whose jumped square is occupied"""
    f, t = a >> 6, a & 63
    return a < 4096 and abs(int(board[f])) == 6 and abs(t // 8 - f // 8) == 2 and board[(f + t) // 2] != 0


def next_meta(e):
    """engine-call meta for the recorded next boards: the other side to move, the same rights"""
    m = np.zeros(8, dtype=np.uint8)
    m[0] = not e["white"]
    m[1:5] = e["rights"]
    return m


# ------------------------------------------------------------------ the fixture itself
def test_fixture_holds_what_it_is_for():
    """the fixture cannot thin out silently: family sizes, castles, capture values, Q1 jumps,
    last-rank pawns, Q6 retreats, the perft entries' classification and its cap"""
    from gym_chess_amd import codec as C

    fx = load_fuzz()
    for fam in FAMILIES:
        assert sum(e["family"] == fam for e, _, _ in fx) >= 150, fam
    castle_lists = castle_moves = q1 = last_rank = q6 = q4 = pairs = 0
    rewards = set()
    for e, b, m in fx:
        assert int((b == 1).sum()) == 1 and int((b == -1).sum()) == 1
        assert len(set(e["rights"])) == 1  # D3: the mover's two rights are equal
        n = len(e["moves"])
        assert len(e["next_boards"]) == len(e["rewards"]) == len(e["flags"]) == len(e["next_n"]) == n
        k = sum(a >= 4096 for a in e["moves"])
        castle_lists += k > 0 and e["family"] == "castle"
        castle_moves += k
        for a, t in zip(e["moves"], e["next_boards"]):  # a castle move's next board is the castled one
            if a >= 4096:
                assert a in (4096, 4097)  # Q4: Black never castles
                nb = C.text_to_board(t)
                assert nb[{4096: 62, 4097: 58}[a]] == 1 and nb[{4096: 61, 4097: 59}[a]] == 3 and nb[60] == 0
        rewards |= set(e["rewards"])
        q1 += any(is_q1_jump(b, a) for a in e["moves"])
        last_rank += bool((b[:8] == 6).any() or (b[56:] == -6).any())
        mover = 0 if e["white"] else 1
        q6 += sum(1 for fl in e["flags"] if fl is not None and fl[mover])
        q4 += e["family"] == "castle" and not e["white"] and b[4] == 1 and (b[0] == 3 or b[7] == 3)
        mv = e["moves"]  # a black pawn's two captures, toward col + 1 first (D4: lib.rs:921-924)
        pairs += any(b[mv[k] >> 6] == -6 and mv[k] >> 6 == mv[k + 1] >> 6 and (mv[k] & 7) == (mv[k] >> 6 & 7) + 1
                     and (mv[k + 1] & 7) == (mv[k] >> 6 & 7) - 1 for k in range(len(mv) - 1) if mv[k + 1] < 4096)
    assert castle_lists >= 60 and castle_moves >= 100, (castle_lists, castle_moves)
    assert {0, 1, 3, 5, 10} <= rewards, rewards  # no capture, pawn, knight / bishop, rook, queen
    assert q1 >= 50 and last_rank >= 50 and q6 >= 50 and q4 >= 10 and pairs >= 20, (q1, last_rank, q6, q4, pairs)
    perft = [e for e, _, _ in fx if "v1_perft" in e]
    assert len(perft) >= 300 and sum("3" in e["v1_perft"] for e in perft) >= 60
    assert all(not any(e["rights"]) for e in perft)
    differ = [e for e in perft if not e["v1_equals_v2"]]
    assert all(e["all_divergences_are_D1"] for e in differ)
    assert len(differ) <= 0.25 * len(perft), (len(differ), len(perft))


# ------------------------------------------------------------------ the oracle
def test_oracle_lists_next_states_rewards_and_flags(oracle):
    from gym_chess_amd import codec as C

    pairs = 0
    for i, (e, b, m) in enumerate(load_fuzz()):
        assert oracle.get_possible_moves(b, m, e["white"]) == e["moves"], i
        nm = next_meta(e)
        for a, t, rw, fl in zip(e["moves"], e["next_boards"], e["rewards"], e["flags"]):
            rc, nb, _, r = oracle.next_state(b, m, e["white"], a)
            assert C.board_to_text(nb) == t and r == rw, (i, a)
            if fl is not None:
                assert rc == int(fl[0] and fl[1]), (i, a)  # D9: both kings checked is the one error
                _, um = oracle.update_state(C.text_to_board(t), nm)
                assert [int(um[5]), int(um[6])] == fl, (i, a)
            pairs += 1
    assert pairs > 13000


def test_oracle_next_move_counts(oracle):
    """the other side's list length on every recorded next board (with mates among them: count 0
    and checked), where v1 and v2 count the same moves"""
    from gym_chess_amd import codec as C

    mates = n = 0
    for i, (e, b, m) in enumerate(load_fuzz()):
        nm = next_meta(e)
        for t, cnt, fl in zip(e["next_boards"], e["next_n"], e["flags"]):
            if cnt is None:
                continue
            assert len(oracle.get_possible_moves(C.text_to_board(t), nm, not e["white"])) == cnt, (i, t)
            mates += cnt == 0 and fl is not None and fl[1 if e["white"] else 0]
            n += 1
    assert n > 13000 and mates >= 10


def test_oracle_perft(oracle):
    """counts where v1 == v2; elsewhere every divergence is D1: v2-only moves that land on the
    enemy king (lib.rs:1074, 1130), all of them in the oracle's list"""
    from gym_chess_amd import codec as C

    for i, (e, b, m) in enumerate(load_fuzz()):
        if "v1_perft" not in e:
            continue
        if e["v1_equals_v2"]:
            for d, v in e["v1_perft"].items():
                assert oracle.perft(b, m, int(d)) == v, (i, d)
            continue
        for dv in e["d1_divergences"]:
            bb = C.text_to_board(dv["board"])
            ours = set(oracle.get_possible_moves(bb, oracle.make_meta(dv["white"], 0, 0, 0, 0), dv["white"]))
            assert not dv["v1_only"] and set(dv["v2_only"]) <= ours, i
            assert all(bb[a % 64] == (-1 if dv["white"] else 1) for a in dv["v2_only"]), i


# ------------------------------------------------------------------ the kernels' core, host-built
def test_core_host_lists_and_apply():
    """gc_core.h on the CPU: the set-wise generator's moves (count2 / select2: the rollout's) as
    a set, the ordered lists (get_list, and for_targets_ordered's), apply per move"""
    from gym_chess_amd import codec as C

    for i, (e, b, m) in enumerate(load_fuzz()):
        w = e["white"]
        n = H.count2(b, m, w)
        assert n == len(e["moves"]) == H.count(b, m, w), i
        assert {H.select2(b, m, w, k) for k in range(n)} == set(e["moves"]), i
        assert [H.select_action(b, m, w, k) for k in range(n)] == sorted(e["moves"]), i  # the API step's pick order
        assert H.get_list(b, m, w) == e["moves"] and H.get_list_emit(b, m, w) == e["moves"], i
        nm = next_meta(e)
        for a, t, rw, fl in zip(e["moves"], e["next_boards"], e["rewards"], e["flags"]):
            assert H.action_legal(b, m, w, a), (i, a)
            rc, nb, _, r = H.next_state(b, m, w, a)
            assert C.board_to_text(nb) == t and r == rw, (i, a)
            if fl is not None:
                assert rc == int(fl[0] and fl[1]), (i, a)
                _, um = H.update_state(C.text_to_board(t), nm)
                assert [int(um[5]), int(um[6])] == fl, (i, a)


def test_core_host_perft():
    for i, (e, b, m) in enumerate(load_fuzz()):
        if e.get("v1_equals_v2"):
            for d, v in e["v1_perft"].items():
                assert H.perft(b, m, int(d)) == v and H.perft_small(b, m, int(d)) == v, (i, d)


# ------------------------------------------------------------------ the fixture == the generator's output
@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference checkout (build container only)")
def test_regenerated_family_is_byte_equal():
    """the checks family made again from the reference: the same entries, byte for byte"""
    import multiprocessing as mp

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_v1_fuzz as F

    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        entries, stats = F.generate_family("checks", pool)
    have = [e for e in load_golden("v1_fuzz.json.gz")["positions"] if e["family"] == "checks"]
    assert len(entries) == len(have) == stats["kept"]
    for got, want in zip(entries, have):
        assert json.dumps(got, separators=(",", ":")) == json.dumps(want, separators=(",", ":"))
