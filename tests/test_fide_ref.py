"""rules="fide" against an independent reference (tests/fide_ref.py), move by move, on the CPU.

Every other FIDE test compares the device with the host build of the SAME source, or counts
moves (perft).  Here the host build of gc_fide.h (tests/core_host) is compared with a plain
mailbox reference written from the rules: move sets, every byte of the next state, rights, both
check flags, the en-passant file, rewards, the env step's endings, move_count and the refusal of
illegal actions -- on the depth-2 trees of the perft positions, along the random self-play
driver, and along scripted games (tests/fide_cases.py) that castle, capture en passant, promote,
mate, stalemate, repeat and hit the move cap far more often than random play does.
tests/test_fide_ref_gpu.py runs the same comparisons against the device kernels.
"""
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
import corehost as H  # noqa: E402
import fide_cases as FC  # noqa: E402
import fide_ref as F  # noqa: E402
from test_fide import EDGE, STANDARD  # noqa: E402  (the published perft totals)

WALK_FENS = [f for f, _ in STANDARD] + [f for f, *_ in EDGE]  # 7 standard + 14 edge positions
SELF_CHECK_NODES = 100_000
EDGE_DEPTH = 3


# ------------------------------------------------------------------ the reference checks itself
def test_reference_reproduces_published_perft():
    """Four-way promotions, en passant, castling: the reference alone equals every published
    total of at most 100 000 nodes; only then are the edge positions, at a lower depth, taken
    from the host perft."""
    n = 0
    for fen, dn in STANDARD:
        for d, nodes in dn.items():
            if nodes <= SELF_CHECK_NODES:
                assert F.perft(F.from_fen(fen), d) == nodes, (fen, d)
                n += 1
    assert n >= 16
    for fen, *_ in EDGE:
        st = F.from_fen(fen)
        assert F.perft(st, EDGE_DEPTH) == H.fide_perft(*F.to_engine(st), EDGE_DEPTH), fen


def test_reference_conversions_round_trip():
    for tl in FC.timelines():
        b, m, ep = tl.start
        st, mc = F.from_env(b, m, ep)
        b2, m2, ep2 = F.to_env(st, mc)
        assert (b2 == b).all() and (m2 == m).all() and ep2 == ep
        eb, em = F.to_engine(st)
        st2 = F.from_engine(eb, em)
        assert (st2.board, st2.white, st2.rights, st2.ep) == (st.board, st.white, st.rights, st.ep)
        mm = FC.mirror_state(FC.mirror_state(st))
        assert (mm.board, mm.white, mm.rights, mm.ep) == (st.board, st.white, st.rights, st.ep)
        assert len(F.legal_actions(FC.mirror_state(st))) == len(F.legal_actions(st))


# ------------------------------------------------------------------ tree walk
def walk_nodes():
    """(state, depth) of every node of the depth-2 trees of the 21 perft positions"""
    out = []
    for fen in WALK_FENS:
        level = [F.from_fen(fen)]
        for d in range(3):
            out += [(s, d) for s in level]
            if d < 2:
                level = [F.apply(s, a)[0] for s in level for a in F.legal_actions(s)]
    return out


def test_tree_walk_lists_and_next_states():
    """At all 10 557 nodes: the host list as a set == legal_actions.  At every (node, move) of
    depths 0 and 1: host_fide_next_state (fapply + fcheck_flags) == apply in the 64 board bytes,
    the side to move, the four rights, both check flags, meta8[7] (file + 1) and the reward."""
    nodes = walk_nodes()
    assert len(nodes) == 10557
    pairs = 0
    for st, d in nodes:
        b, m = F.to_engine(st)
        legal = F.legal_actions(st)
        lst = H.fide_list(b, m)
        assert len(lst) == len(set(lst)) and set(lst) == set(legal), (b.tolist(), m.tolist())
        assert [a for a in lst if a >= 4096] == lst[len(lst) - sum(a >= 4096 for a in lst):]  # castles last
        if d < 2:
            for a in legal:
                ns, rw = F.apply(st, a)
                nb, nm = F.to_engine(ns)
                rc, ob, om, hrw = H.host_fide_next_state(b, m, a)
                assert rc == 0 and (ob == nb).all() and (om == nm).all() and hrw == rw, (b.tolist(), m.tolist(), a)
                pairs += 1
    assert pairs == 10557 - 21


# ------------------------------------------------------------------ the self-play driver
def follow(trace, start, plies, first=None):
    """the reference follows a driver trace ply by ply from `start` (the reset position), or from
    first = (state, move_count) with `start` after the first reset; returns the reference env
    and counts of what it saw"""
    env = F.RefEnv(start)
    if first is not None:
        env.set(*first)
    seen = Counter()
    for p in range(plies):
        a = int(trace["action"][p])
        got = (int(trace["reward"][p]), int(trace["done"][p]), int(trace["reason"][p]))
        if a < 0:  # the driver found no move: reset, reason 4
            assert not F.legal_actions(env.s), p
            assert got == (0, 0, 4), (p, got)
            seen["stalemate" if not F.in_check(env.s.board, env.s.white) else "no_move"] += 1
            env.reset()
            continue
        exp = env.step(a)  # reason 6 here would mean the driver played an illegal move
        assert got == (exp[0], int(exp[1]), exp[2]), (p, a, got, exp)
        seen[exp[2]] += 1
        if exp[1]:
            env.reset()
    return env, seen


START = F.from_fen(F.STARTPOS)
# white to move with few pieces: random play stalemates black (Kf8) every few plies
STALEMATE_PRONE = F.from_fen("7k/5K1p/7P/8/8/8/8/8 w KQkq - 0 1")


def test_follower_driver_from_start():
    """H.fide_rollout (fenv_step<false> + the set-wise pick) from the start position, 12 boards
    x 600 plies: every played action legal in the reference, reward / done / reason equal,
    no-move plies exactly where the reference has no legal move, mates and move caps seen."""
    tot = Counter()
    init = np.array(START.board, dtype=np.int8)
    for bd in range(12):
        _, seen = follow(H.fide_rollout(0xF1DE, bd, 600, init), START, 600)
        tot += seen
    assert tot[6] == 0 and tot[1] > 0 and tot[3] > 0, tot


def test_follower_driver_reaches_stalemates():
    """the same from a position where random play stalemates: the ply after a stalemating move
    is a no-move ply (reason 4, reward 0), and the next episode starts from the reset position"""
    tot = Counter()
    init = np.array(STALEMATE_PRONE.board, dtype=np.int8)
    for bd in range(4):
        _, seen = follow(H.fide_rollout(0x57A1, bd, 300, init), STALEMATE_PRONE, 300)
        tot += seen
    assert tot["stalemate"] >= 2 and tot[6] == 0, tot


# ------------------------------------------------------------------ scripted games
def host_step(prev, ply, hist, validate=True):
    b, m, ep, done = prev
    return H.host_fide_step(b, m, ep, m[7], ply.action, validate=validate, hist=hist, done=done)


def check_step(tl, i, got, ply):
    where = (tl.name, i, ply.action)
    assert (got["reward"], got["done"], got["reason"]) == (ply.reward, ply.done, ply.reason), where
    assert (got["board"] == ply.board).all(), where
    assert (got["meta8"] == ply.meta8).all(), (where, got["meta8"].tolist(), ply.meta8.tolist())
    assert got["ep"] == ply.ep and got["state_done"] == ply.state_done, where


@pytest.mark.parametrize("probes", [False, True])
def test_scripted_games_through_host_step(probes):
    """Every case of fide_cases.CASES and its colour mirror through fenv_step<true> with one
    3-fold window per game: after every ply the reward, done, reason, the 64 board bytes, meta8
    (side, rights, both check flags, move_count), the en-passant file and the state's done flag
    equal the reference's.  probes=True puts an invalid action in front of every move."""
    for tl in FC.timelines(probes):
        hist = H.FideHist()
        prev = tl.start + (False,)
        for i, ply in enumerate(tl.plies):
            check_step(tl, i, host_step(prev, ply, hist), ply)
            prev = (ply.board, ply.meta8, ply.ep, ply.state_done)


def test_scripted_games_unvalidated_step():
    """fenv_step<false> (the driver's form) on the scripts' legal moves gives the same"""
    for tl in FC.timelines():
        hist = H.FideHist()
        prev = tl.start + (False,)
        for i, ply in enumerate(tl.plies):
            if ply.reason == 6:
                continue
            check_step(tl, i, host_step(prev, ply, hist, validate=False), ply)
            prev = (ply.board, ply.meta8, ply.ep, ply.state_done)


def test_invalid_actions_change_nothing():
    """At every scripted position: each pseudo-legal but illegal id (pinned piece, king into
    check, refused castles and en passants), 4100, an enemy piece's move and an empty
    from-square give reason 6, reward -10, done as it was and a bit-identical state."""
    tried = Counter()
    for tl in FC.timelines():
        prev = tl.start + (False,)
        for i, ply in enumerate(tl.plies):
            b, m, ep, done = prev
            st, _ = F.from_env(b, m, ep)
            legal = set(F.legal_actions(st))
            for a in tl.invalid[i]:
                assert a not in legal
                got = H.host_fide_step(b, m, ep, m[7], a, validate=True, done=done)
                assert (got["reward"], got["done"], got["reason"]) == (-10, done, 6), (tl.name, i, a)
                assert (got["board"] == b).all() and (got["meta8"] == m).all(), (tl.name, i, a)
                assert got["ep"] == ep and got["state_done"] == done, (tl.name, i, a)
                tried["castle" if 4096 <= a < 4100 else "move"] += 1
            tried["refused_ep"] += any(a < 4096 and a % 64 == st.ep and abs(st.board[a // 64]) == F.P
                                       for a in F.illegal_pseudo_actions(st))
            prev = (ply.board, ply.meta8, ply.ep, ply.state_done)
    assert tried["castle"] >= 100 and tried["move"] >= 1000 and tried["refused_ep"] >= 4, tried


# ------------------------------------------------------------------ what the scripts contain
def test_scripts_contain_the_rare_moves():
    """Counted by the reference alone over the scripted plies (conditions, not measurements)."""
    c = Counter()
    for tl in FC.timelines():
        for ply in tl.plies:
            k = ply.kind
            if k is not None and ply.reason != 3:
                c["ep"] += k["ep"]
                c["promo"] += k["promo"]
                c["promo_capture"] += k["promo"] and k["capture"]
                c["mate"] += k["mate"]
                c["stalemate"] += k["stalemate"]
                c["corner"] += k["corner"]
                if k["castle"]:
                    c[k["castle"]] += 1
                assert k["mate"] == (ply.reason == 1)
            c["repetition"] += ply.reason == 2 and not ply.probe
        c["cap"] += any(p.reason == 3 for p in tl.plies)
        c["after_done"] += any(p.reason == 7 for p in tl.plies)
    assert c["ep"] >= 20, c
    assert all(c[a] >= 5 for a in (4096, 4097, 4098, 4099)), c
    assert c["promo"] >= 20 and c["promo_capture"] >= 6, c
    assert c["mate"] >= 8 and c["stalemate"] >= 2, c
    assert c["repetition"] >= 4 and c["cap"] >= 4 and c["corner"] >= 4 and c["after_done"] >= 4, c


def test_scripts_show_what_they_are_named_for():
    """the positions behind the case names, stated through the reference"""
    tl = {t.name: t for t in FC.timelines()}

    def before(name, i):
        t = tl[name]
        b, m, ep = t.start if i == 0 else (t.plies[i - 1].board, t.plies[i - 1].meta8, t.plies[i - 1].ep)
        return F.from_env(b, m, ep)[0]

    for name, refused in (("castle_refused_f1", 4096), ("castle_refused_g1", 4096), ("castle_refused_d1", 4097),
                          ("castle_refused_c1", 4097)):
        legal = F.legal_actions(before(name, 0))
        assert refused not in legal and (refused ^ 1) in legal, name
    assert not {4096, 4097} & set(F.legal_actions(before("castle_refused_in_check", 0)))
    assert 4097 in F.legal_actions(before("castle_b_file_attacked", 0))
    assert F.attacked(before("castle_b_file_attacked", 0).board, 57, False)  # b1
    for name in ("ep_refused_rank_pin", "ep_refused_diagonal_pin"):
        st = before(name, 1)
        refused = [a for a in F.illegal_pseudo_actions(st) if a % 64 == st.ep and abs(st.board[a // 64]) == F.P]
        assert st.ep >= 0 and len(refused) == 1, name
    st = before("ep_no_capturer_file_still_set", 1)  # after e2e4: no black pawn beside e4
    assert st.ep == 44 and not [a for a in F.legal_actions(st) if a % 64 == 44]
    for name in ("rights_king_move", "rights_rook_moves"):
        n = 4 if name == "rights_king_move" else 8
        assert tl[name].plies[n - 1].meta8[1:5].tolist() == [0, 0, 0, 0], name
        assert not any(p.action >= 4096 and p.reason == 0 for p in tl[name].plies)
    assert tl["rights_corner_captures"].plies[3].meta8[1:5].tolist() == [0, 0, 0, 0]
    t = tl["repeat_rook_other_rights"]  # the third occurrence's rights differ from the first's
    assert t.start[1][1] == 1 and t.plies[7].meta8[1] == 0 and (t.plies[7].board == t.start[0]).all()
    assert t.plies[8].reason == 2
    assert tl["mate_on_third_occurrence"].plies[8].reason == 1 and tl["mate_on_third_occurrence"].plies[8].reward == 90
