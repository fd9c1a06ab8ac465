"""TEST INFRASTRUCTURE ONLY -- chosen FIDE positions with move scripts, expanded by the
reference (tests/fide_ref.py) alone into per-ply expectations that the CPU and the GPU tests
share.  Random play from the start position almost never castles, captures en passant or repeats
a board; these scripts do.

A script is a list of tokens: "e2e4" plays that move, "*" lets the reference pick BY RULE -- an
en-passant capture if one is legal, else a castle, else a promotion, else a capture on a corner
that takes a castling right, else a mating move, else a seeded random move -- and "*1" does the
same after asserting that exactly one move is legal.  Past the script's end the rule goes on to
the case's ply count.  Every case also runs colour-mirrored (board flipped, colours, rights and
moves swapped), so whatever is listed for one colour is tested for both.
"""
import random

import numpy as np

import fide_ref as F

KQ = "r3k2r/8/8/8/8/8/8/R3K2R"
SHUFFLE_K = ["e1d1", "e8d8", "d1e1", "d8e8"]

# (name, FEN, move_count, script, plies)
CASES = [
    # en passant: both flanks (a5xb6 / c5xb6 ...), the other flank alone, for both colours by the mirror
    ("ep_right", "4k3/1p1p1p1p/8/P1P1P1P1/8/8/8/4K3 b - - 0 1", 0, ["b7b5", "*", "d7d5", "*", "f7f5", "*", "h7h5", "*"], 10),
    ("ep_left", "4k3/p1p1p1p1/8/1P1P1P1P/8/8/8/4K3 b - - 0 1", 0, ["a7a5", "*", "c7c5", "*", "e7e5", "*", "g7g5", "*"], 10),
    ("ep_two_capturers", "4k3/3p4/8/2P1P3/8/8/8/4K3 b - - 0 1", 0, ["d7d5", "*"], 6),
    ("ep_from_fen", "8/8/1k6/2b5/2pP4/8/5K2/8 b - d3 0 1", 0, ["*"], 6),
    ("ep_refused_rank_pin", "3k4/3p4/8/K1P4r/8/8/8/8 b - - 0 1", 0, ["d7d5", "*"], 6),
    ("ep_refused_diagonal_pin", "8/8/4k3/8/2p5/8/B2P2K1/8 w - - 0 1", 0, ["d2d4", "*"], 6),
    ("ep_only_move_out_of_check", "1R6/8/p7/k7/b1p5/8/1P6/7K w - - 0 1", 0, ["b2b4", "*1"], 6),
    ("ep_no_capturer_file_still_set", F.STARTPOS, 0, ["e2e4", "e7e5", "a2a4", "h7h5", "a4a5", "b7b5", "*"], 10),
    # castles: all four, through the rule
    ("castle_king_sides", KQ + " w KQkq - 0 1", 0, ["*", "*"], 8),
    ("castle_queen_sides", KQ + " w Qq - 0 1", 0, ["*", "*"], 8),
    ("castle_b_file_attacked", "r3k2r/pR5p/8/8/8/8/Pr5P/R3K2R w Qq - 0 1", 0, ["*", "*"], 6),
    ("castle_kiwipete", "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1", 0, ["*", "*"], 8),
    ("castle_pawns_king", "r3k2r/pppppppp/8/8/8/8/PPPPPPPP/R3K2R w KQkq - 0 1", 0, ["*", "*"], 8),
    ("castle_pawns_queen", "r3k2r/pppppppp/8/8/8/8/PPPPPPPP/R3K2R w Qq - 0 1", 0, ["*", "*"], 8),
    ("castle_short_gives_check", "5k2/8/8/8/8/8/8/4K2R w K - 0 1", 0, ["*"], 6),
    ("castle_long_gives_check", "3k4/8/8/8/8/8/8/R3K3 w Q - 0 1", 0, ["*"], 6),
    # castles refused: one attacked square at a time (the other side stays legal), both, in check
    ("castle_refused_f1", "4kr2/8/8/8/8/8/8/R3K2R w KQ - 0 1", 0, ["*"], 5),
    ("castle_refused_g1", "4k1r1/8/8/8/8/8/8/R3K2R w KQ - 0 1", 0, ["*"], 5),
    ("castle_refused_d1", "3rk3/8/8/8/8/8/8/R3K2R w KQ - 0 1", 0, ["*"], 5),
    ("castle_refused_c1", "2r1k3/8/8/8/8/8/8/R3K2R w KQ - 0 1", 0, ["*"], 5),
    ("castle_refused_f_and_d", "r3k2r/8/3Q4/8/8/5q2/8/R3K2R b KQkq - 0 1", 0, ["*", "*"], 6),
    ("castle_refused_in_check", "4k3/8/8/8/8/8/4r3/R3K2R w KQ - 0 1", 0, ["*"], 5),
    # rights lost
    ("rights_king_move", KQ + " w KQkq - 0 1", 0, ["e1e2", "e8e7", "e2e1", "e7e8", "*", "*"], 8),
    ("rights_rook_moves", KQ + " w KQkq - 0 1", 0,
     ["a1a2", "a8a7", "h1h2", "h8h7", "a2a1", "a7a8", "h2h1", "h7h8", "*", "*"], 12),
    ("rights_corner_captures", "r3k2r/p6p/1N4N1/8/8/1n4n1/P6P/R3K2R w KQkq - 0 1", 0, ["*", "*", "*", "*"], 8),
    # promotions
    ("promo_push", "8/P6k/8/8/8/8/p6K/8 w - - 0 1", 0, ["*", "*"], 6),
    ("promo_capture", "1n2k3/P7/8/8/8/8/p7/1N2K3 w - - 0 1", 0, ["*", "*"], 6),
    ("promo_capture_corner", "r1n1k3/1P6/8/8/8/8/1p6/R1N1K3 w - - 0 1", 0, ["*", "*"], 6),
    ("promo_many", "8/PPPP3k/8/8/8/8/pppp3K/8 w - - 0 1", 0, ["*"] * 8, 10),
    ("promo_mates", "7k/4P3/6K1/8/8/8/8/8 w - - 0 1", 0, ["*"], 2),
    # mates
    ("mate_rook", "6k1/5ppp/8/8/8/8/8/R5K1 w - - 0 1", 0, ["*"], 2),
    ("mate_queen", "k7/8/1K6/8/8/8/8/7Q w - - 0 1", 0, ["*"], 2),
    ("mate_fools", "rnbqkbnr/pppp1ppp/8/4p3/6P1/5P2/PPPPP2P/RNBQKBNR b KQkq - 0 1", 0, ["*"], 2),
    ("mate_on_third_occurrence", "6k1/5ppp/8/8/8/8/8/R5K1 w - - 0 1", 0,
     ["g1h1", "g8h8", "h1g1", "h8g8"] * 2 + ["*"], 10),
    # stalemates: the side to move is left without a move and not in check
    ("stalemate_queen", "7k/5K2/8/6Q1/8/8/8/8 w - - 0 1", 0, ["g5g6"], 2),
    ("stalemate_pawn", "7k/5K1p/7P/8/8/8/8/8 w - - 0 1", 0, ["f7f8"], 2),
    # 3-fold on the board alone
    ("repeat_knights", F.STARTPOS, 0, ["g1f3", "g8f6", "f3g1", "f6g8"] * 2 + ["g1f3"], 10),
    ("repeat_rook_other_rights", "4k3/8/8/8/8/8/8/4K2R w K - 0 1", 0, ["h1g1", "e8d8", "g1h1", "d8e8"] * 2 + ["h1g1"], 10),
    ("repeat_kings", "4k3/8/8/8/8/8/8/4K3 w - - 0 1", 0, SHUFFLE_K * 2 + ["e1d1"], 10),
    # the move cap, reached from a move_count set through the state
    ("cap_148", F.STARTPOS, 148, [], 8),
    ("cap_149", F.STARTPOS, 149, [], 8),
    ("cap_150", F.STARTPOS, 150, [], 3),
]


def mirror_state(st):
    b = [0] * 64
    for sq in range(64):
        b[(7 - sq // 8) * 8 + sq % 8] = -st.board[sq]
    ep = -1 if st.ep < 0 else (7 - st.ep // 8) * 8 + st.ep % 8
    return F.State(b, not st.white, st.rights[2:] + st.rights[:2], ep)


def mirror_token(tok):
    if tok[0] == "*":
        return tok
    return tok[0] + str(9 - int(tok[1])) + tok[2] + str(9 - int(tok[3]))


def token_action(tok):
    sq = lambda s: (8 - int(s[1])) * 8 + "abcdefgh".index(s[0])  # noqa: E731
    return sq(tok[:2]) * 64 + sq(tok[2:])


def rule_pick(st, legal, rng):
    """the scripts' rule; within a class a mating move first, then a capturing one, then the
    lowest id"""
    kinds = {a: F.describe_quick(st, a) for a in legal}
    for cls in ("ep", "castle", "promo", "corner"):
        c = [a for a in legal if kinds[a][cls]]
        if c:
            return min(c, key=lambda a: (not F.mates(st, a), not kinds[a]["capture"], a))
    for a in legal:
        if F.mates(st, a):
            return a
    return legal[rng.randrange(len(legal))]


class Ply:
    """one step of a timeline: the action and everything the step must return, then the state"""
    __slots__ = ("action", "reward", "done", "reason", "board", "meta8", "ep", "legal", "kind", "probe", "state_done")


def _invalid_ids(st):
    """the invalid actions tried at a position: every pseudo-legal but illegal id, resign, an
    enemy piece's move, an empty from-square"""
    out = F.illegal_pseudo_actions(st) + [F.A_RESIGN]
    flipped = st.copy()
    flipped.white = not st.white
    flipped.ep = -1
    enemy = [f * 64 + t for f, t in F.pseudo_moves(flipped)]
    if enemy:
        out.append(enemy[0])
    empty = [sq for sq in range(64) if st.board[sq] == 0]
    if empty:
        out.append(empty[0] * 64 + empty[-1])
    return out


def _record(env, action, res, kind, probe):
    p = Ply()
    p.action, (p.reward, p.done, p.reason) = action, res
    p.board, p.meta8, p.ep = F.to_env(env.s, env.mc)
    p.legal = F.legal_actions(env.s)
    p.kind, p.probe, p.state_done = kind, probe, env.done
    return p


class Timeline:
    """A case expanded by the reference: the start state and the plies.  probes=False: the
    scripted moves, then one legal action (if any is left) and a resign after the end; each ply's
    .invalid lists the invalid ids of the position BEFORE it.  probes=True: one invalid action in
    front of every scripted move, cycling through that position's invalid ids."""

    def __init__(self, name, st, move_count, script, plies, seed, probes=False):
        self.name = name
        self.start = F.to_env(st, move_count)
        env = F.RefEnv(st, move_count)
        rng = random.Random(seed)
        self.plies, self.invalid = [], []
        k = 0
        for i in range(plies):
            legal = F.legal_actions(env.s)
            if env.done or not legal:
                break
            tok = script[i] if i < len(script) else "*"
            if tok == "*1":
                assert len(legal) == 1, (name, i, legal)
            a = rule_pick(env.s, legal, rng) if tok[0] == "*" else token_action(tok)
            assert a in legal, (name, i, tok, legal)
            inv = _invalid_ids(env.s)
            if probes:
                bad = inv[k % len(inv)]
                k += 1
                self.plies.append(_record(env, bad, env.step(bad), None, True))
            kind = F.describe(env.s, a) if env.mc <= F.MOVES_MAX else None
            self.invalid.append(inv)
            self.plies.append(_record(env, a, env.step(a), kind, False))
            if self.plies[-1].reason == 3:
                break
        # after the end: a legal action (reason 7 once done, 3 at the cap) and a resign
        legal = F.legal_actions(env.s)
        for a in ([legal[0]] if legal else []) + [F.A_RESIGN]:
            self.invalid.append(_invalid_ids(env.s))
            self.plies.append(_record(env, a, env.step(a), None, a == F.A_RESIGN))
        self.env = env  # the reference env after the last ply


_CACHE = {}


def timelines(probes=False):
    """every case and its colour mirror, expanded once per process"""
    if probes not in _CACHE:
        out = []
        for k, (name, fen, mc, script, plies) in enumerate(CASES):
            st = F.from_fen(fen)
            out.append(Timeline(name, st, mc, script, plies, 1000 + k, probes))
            out.append(Timeline(name + "/mirrored", mirror_state(st), mc, [mirror_token(t) for t in script], plies,
                                2000 + k, probes))
        _CACHE[probes] = out
    return _CACHE[probes]


def padded(tls, length=None):
    """the timelines' per-ply fields as arrays [ply][case], each padded to one length with resign
    steps (invalid: -10, reason 6, the state and done as they were)"""
    n = length or max(len(t.plies) for t in tls)
    cols = []
    for t in tls:
        last = t.plies[-1]
        assert last.action == F.A_RESIGN and last.reason == 6
        cols.append(t.plies + [last] * (n - len(t.plies)))
    f = lambda name, dt: np.array([[getattr(c[p], name) for c in cols] for p in range(n)], dtype=dt)  # noqa: E731
    return dict(action=f("action", np.int64), reward=f("reward", np.int32), done=f("done", bool),
                reason=f("reason", np.uint8), board=f("board", np.int8), meta8=f("meta8", np.uint8),
                ep=f("ep", np.int8), legal=[[c[p].legal for c in cols] for p in range(n)])
