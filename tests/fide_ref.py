"""TEST INFRASTRUCTURE ONLY -- an independent reference for rules="fide", in plain Python.

Written from the rules of chess and from the contract stated in gc_fide.h's header comment and
include/gymchess.h, not from the engine's code: a mailbox board, pseudo-legal moves, and
legality by making the move and asking whether the mover's king is attacked.  No bitboards,
no pins, no check masks, nothing compiled, nothing imported from the package's engine.

Board: int8[64], square 0 = a8, 63 = h1 (row 0 = rank 8); K 1, Q 2, R 3, B 4, N 5, P 6, white
positive.  Action ids: from * 64 + to (a promotion once: env actions promote to a queen), castles
4096 / 4097 white king / queen side, 4098 / 4099 black; 4100 (resign) is never legal.

The env contract (RefEnv): -10 per valid move + the captured piece's value (Q 10, R 5, B 3, N 3,
P 1; en passant 1) + 10 for a promotion; an invalid action -10 / reason 6 / nothing changes; a
done state reason 7; move_count > 149 reason 3; the PRE-move board's third occurrence since the
last reset (the board alone: no side, rights or en passant in the key) reason 2; mate +100 /
reason 1, which wins over a repetition on the same ply; move_count grows after a black move that
did not end the game.  With the random opponent: the reply's move reward is subtracted, -100 /
reason 8 when the reply mates the agent, reason 9 when the opponent has no reply, and
move_count grows after a reply that leaves WHITE to move (a BLACK agent's stays at the 1 its
opening ply at reset gives it).
"""
from collections import Counter

import numpy as np

K, Q, R, B, N, P = 1, 2, 3, 4, 5, 6
VALUE = {0: 0, K: 0, Q: 10, R: 5, B: 3, N: 3, P: 1}
A_KSW, A_QSW, A_KSB, A_QSB, A_RESIGN = 4096, 4097, 4098, 4099, 4100
MOVES_MAX = 149
STARTPOS = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
# castle id -> (king from, king to, rook from, rook to)
CASTLES = {A_KSW: (60, 62, 63, 61), A_QSW: (60, 58, 56, 59), A_KSB: (4, 6, 7, 5), A_QSB: (4, 2, 0, 3)}
# squares whose touching (from or to) drops rights: index into rights [wk, wq, bk, bq]
RIGHTS_LOST = {63: (0,), 56: (1,), 60: (0, 1), 7: (2,), 0: (3,), 4: (2, 3)}


def _table(deltas):
    out = []
    for sq in range(64):
        r, c = divmod(sq, 8)
        out.append([(r + dr) * 8 + c + dc for dr, dc in deltas if 0 <= r + dr < 8 and 0 <= c + dc < 8])
    return out


def _rays():
    out = []
    for sq in range(64):
        r, c = divmod(sq, 8)
        rays = []
        for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)):  # 4 straight, 4 diagonal
            ray, rr, cc = [], r + dr, c + dc
            while 0 <= rr < 8 and 0 <= cc < 8:
                ray.append(rr * 8 + cc)
                rr, cc = rr + dr, cc + dc
            rays.append(ray)
        out.append(rays)
    return out


KNIGHT_T = _table([(-2, -1), (-2, 1), (-1, -2), (-1, 2), (1, -2), (1, 2), (2, -1), (2, 1)])
KING_T = _table([(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)])
RAYS = _rays()


class State:
    __slots__ = ("board", "white", "rights", "ep")

    def __init__(self, board, white, rights, ep=-1):
        self.board = [int(x) for x in board]  # 64 ints
        self.white = bool(white)
        self.rights = [bool(x) for x in rights]  # wk, wq, bk, bq
        self.ep = int(ep)  # en-passant target square (where the capturing pawn lands) or -1

    def copy(self):
        return State(self.board, self.white, self.rights, self.ep)

    def key(self):
        return bytes(x & 0xFF for x in self.board)


def from_fen(fen):
    """placement, side, castling and en-passant fields (the clocks are not part of the state)"""
    f = fen.split()
    board = []
    for ch in f[0]:
        if ch == "/":
            continue
        if ch.isdigit():
            board += [0] * int(ch)
        else:
            v = " KQRBNP".index(ch.upper())
            board.append(v if ch.isupper() else -v)
    assert len(board) == 64, fen
    rights = [c in f[2] for c in "KQkq"]
    ep = -1
    if f[3] != "-":
        ep = (8 - int(f[3][1])) * 8 + "abcdefgh".index(f[3][0])
    return State(board, f[1] == "w", rights, ep)


def attacked(b, sq, by_white):
    """is square sq attacked by the side by_white on board b?"""
    sg = 1 if by_white else -1
    for t in KNIGHT_T[sq]:
        if b[t] == N * sg:
            return True
    for t in KING_T[sq]:
        if b[t] == K * sg:
            return True
    r, c = divmod(sq, 8)
    pr = r + 1 if by_white else r - 1  # a white pawn attacks towards rank 8 (lower rows)
    if 0 <= pr < 8:
        for pc in (c - 1, c + 1):
            if 0 <= pc < 8 and b[pr * 8 + pc] == P * sg:
                return True
    for d, ray in enumerate(RAYS[sq]):
        line = (R if d < 4 else B) * sg
        for t in ray:
            v = b[t]
            if v:
                if v == Q * sg or v == line:
                    return True
                break
    return False


def king_square(b, white):
    k = K if white else -K
    return b.index(k) if k in b else -1


def in_check(b, white):
    ks = king_square(b, white)
    return ks >= 0 and attacked(b, ks, not white)


def check_flags(st):
    """(white king attacked, black king attacked)"""
    return in_check(st.board, True), in_check(st.board, False)


def pseudo_moves(st):
    """pseudo-legal non-castle moves (from, to) of the side to move: own pieces' moves by their
    geometry, en passant included; a king is never a target"""
    b, white = st.board, st.white
    sg = 1 if white else -1
    out = []
    for frm in range(64):
        v = b[frm] * sg
        if v <= 0:
            continue
        if v == P:
            r, c = divmod(frm, 8)
            d = -1 if white else 1
            nr = r + d
            if not 0 <= nr < 8:
                continue
            one = nr * 8 + c
            if b[one] == 0:
                out.append((frm, one))
                if r == (6 if white else 1) and b[one + 8 * d] == 0:
                    out.append((frm, one + 8 * d))
            for cc in (c - 1, c + 1):
                if not 0 <= cc < 8:
                    continue
                t = nr * 8 + cc
                tv = b[t] * sg
                if tv < 0:
                    if tv != -K:
                        out.append((frm, t))
                elif t == st.ep and tv == 0 and b[r * 8 + cc] == -P * sg:
                    out.append((frm, t))
        elif v == N or v == K:
            for t in (KNIGHT_T if v == N else KING_T)[frm]:
                tv = b[t] * sg
                if tv <= 0 and tv != -K:
                    out.append((frm, t))
        else:
            rays = RAYS[frm]
            for ray in (rays if v == Q else rays[:4] if v == R else rays[4:]):
                for t in ray:
                    tv = b[t] * sg
                    if tv > 0:
                        break
                    if tv != -K:
                        out.append((frm, t))
                    if tv:
                        break
    return out


def castle_legal(st, action):
    """the right held, king and rook at home, nothing between them, the king not in check, and
    the two squares it crosses and lands on not attacked (b1 / b8 may be)"""
    kf, kt, rf, rt = CASTLES[action]
    if (action in (A_KSW, A_QSW)) != st.white:
        return False
    b, sg = st.board, 1 if st.white else -1
    if not st.rights[action - 4096]:
        return False
    if b[kf] != K * sg or b[rf] != R * sg:
        return False
    if any(b[x] for x in range(min(kf, rf) + 1, max(kf, rf))):
        return False
    return not any(attacked(b, x, not st.white) for x in (kf, rt, kt))


def apply(st, action, promo=Q):
    """-> (next state, move reward): capture value, +1 en passant, +10 promotion"""
    n = st.copy()
    b = n.board
    white = st.white
    sg = 1 if white else -1
    n.white = not white
    n.ep = -1
    if action >= 4096:
        kf, kt, rf, rt = CASTLES[action]
        b[kf] = b[rf] = 0
        b[kt], b[rt] = K * sg, R * sg
        n.rights[0 if white else 2] = n.rights[1 if white else 3] = False
        return n, 0
    frm, to = divmod(action, 64)
    pt = b[frm] * sg
    assert pt > 0, (action, "no piece of the side to move")
    reward = VALUE[abs(b[to])]
    if pt == P and to == st.ep and (frm - to) % 8 and b[to] == 0:  # en passant: the pawn beside
        b[(frm // 8) * 8 + to % 8] = 0
        reward = 1
    b[frm] = 0
    b[to] = pt * sg
    if pt == P:
        if to // 8 == (0 if white else 7):
            b[to] = promo * sg
            reward += 10
        if abs(frm - to) == 16:
            n.ep = (frm + to) // 2  # after EVERY double step, capturer or not
    for sq in (frm, to):
        for k in RIGHTS_LOST.get(sq, ()):
            n.rights[k] = False
    return n, reward


def is_legal_after(st, action):
    n, _ = apply(st, action)
    return not in_check(n.board, st.white)


def legal_actions(st):
    """sorted legal action ids"""
    out = [f * 64 + t for f, t in pseudo_moves(st) if is_legal_after(st, f * 64 + t)]
    out += [a for a in CASTLES if castle_legal(st, a)]
    return sorted(set(out))


def illegal_pseudo_actions(st):
    """ids the geometry allows and the rules refuse: pseudo-legal moves that leave the own king
    attacked, and the mover's castles that are not legal"""
    legal = set(legal_actions(st))
    out = {f * 64 + t for f, t in pseudo_moves(st)} - legal
    out |= {a for a in CASTLES if (a in (A_KSW, A_QSW)) == st.white and a not in legal}
    return sorted(out)


def perft(st, depth):
    """leaf count with the four promotion pieces"""
    if depth == 0:
        return 1
    n = 0
    last = 0 if st.white else 7
    for a in legal_actions(st):
        promo = a < 4096 and abs(st.board[a // 64]) == P and (a % 64) // 8 == last
        if depth == 1:
            n += 4 if promo else 1
            continue
        for pc in ((Q, R, B, N) if promo else (Q,)):
            n += perft(apply(st, a, pc)[0], depth - 1)
    return n


def describe_quick(st, action):
    """what kind of move a legal action is, from the position alone (for move scripts)"""
    b = st.board
    d = dict(ep=False, castle=None, promo=False, capture=False, corner=False)
    if action >= 4096:
        d["castle"] = action
        return d
    frm, to = divmod(action, 64)
    pawn = abs(b[frm]) == P
    d["ep"] = pawn and to == st.ep and (frm - to) % 8 != 0 and b[to] == 0
    d["promo"] = pawn and to // 8 == (0 if st.white else 7)
    d["capture"] = b[to] != 0 or d["ep"]
    # a capture on a rook's corner that takes a right the other side still held
    d["corner"] = b[to] != 0 and to in (0, 7, 56, 63) and any(st.rights[k] for k in RIGHTS_LOST[to])
    return d


def mates(st, action):
    n, _ = apply(st, action)
    return in_check(n.board, n.white) and not legal_actions(n)


def describe(st, action):
    """describe_quick, and whether the move mates or stalemates"""
    d = describe_quick(st, action)
    n, _ = apply(st, action)
    d["mate"] = d["stalemate"] = False
    if not legal_actions(n):
        d["mate" if in_check(n.board, n.white) else "stalemate"] = True
    return d


# ---- conversions ------------------------------------------------------------------------------
def _meta(st):
    wc, bc = check_flags(st)
    m = np.zeros(8, dtype=np.uint8)
    m[0] = st.white
    m[1:5] = st.rights
    m[5], m[6] = wc, bc
    return m


def ep_file(st):
    return st.ep % 8 if st.ep >= 0 else -1


def _ep_square(white, file):
    """the en-passant target for the side to move: rank 6 for WHITE, rank 3 for BLACK"""
    return -1 if file < 0 else (16 if white else 40) + file


def to_engine(st):
    """(board int8[64], meta8) as the FIDE engine calls take them: meta8[7] = file + 1"""
    m = _meta(st)
    m[7] = ep_file(st) + 1
    return np.array(st.board, dtype=np.int8), m


def from_engine(board, meta8):
    m = [int(x) for x in np.asarray(meta8).reshape(8)]
    return State(np.asarray(board).reshape(64), m[0], m[1:5], _ep_square(bool(m[0]), m[7] - 1))


def to_env(st, move_count=0):
    """(board, meta8, file) as the env's boards() / en_passant(): meta8[7] = move_count"""
    m = _meta(st)
    m[7] = move_count
    return np.array(st.board, dtype=np.int8), m, ep_file(st)


def from_env(board, meta8, ep=-1):
    """-> (state, move_count)"""
    m = [int(x) for x in np.asarray(meta8).reshape(8)]
    return State(np.asarray(board).reshape(64), m[0], m[1:5], _ep_square(bool(m[0]), int(ep))), m[7]


# ---- the env step contract --------------------------------------------------------------------
class RefEnv:
    """One board of the FIDE env.  step(action) -> (reward, done, reason).  With opponent=True,
    step(action, reply) takes `reply`, a callable (RefEnv) -> the opponent's action, asked only
    when a reply is due (the position then is the one after the agent's move)."""

    def __init__(self, state=None, move_count=0, opponent=False):
        self.start = (state or from_fen(STARTPOS)).copy()
        self.opponent = opponent
        self.set(self.start, move_count)

    def set(self, state, move_count=0):
        self.s = state.copy()
        self.mc = int(move_count)
        self.done = False
        self.seen = Counter()

    def reset(self, opening=None):
        """back to the start position; opening = a BLACK agent's opponent's first move"""
        self.set(self.start, 0)
        if opening is not None:
            self._ply(opening)  # its 3-fold verdict is discarded
            self.mc = 1

    def _ply(self, action):
        key = self.s.key()
        self.seen[key] += 1
        self.s, mr = apply(self.s, action)
        return mr, self.seen[key]

    def _mated(self):
        return in_check(self.s.board, self.s.white) and not legal_actions(self.s)

    def step(self, action, reply=None):
        if action not in legal_actions(self.s):
            return -10, self.done, 6
        if self.done:
            return 0, True, 7
        if self.mc > MOVES_MAX:
            return 0, True, 3
        white = self.s.white
        mr, c = self._ply(action)
        reward, done, reason = -10 + mr, False, 0
        if c >= 3:
            done, reason = True, 2
        if self._mated():
            reward, done, reason = reward + 100, True, 1
        if not self.opponent:
            if not done and not white:
                self.mc += 1
            self.done = done
            return reward, done, reason
        if not done and not legal_actions(self.s):
            done, reason = True, 9
        if done:
            self.done = True
            return reward, done, reason
        mr, c = self._ply(reply(self))
        reward -= mr
        if c >= 3:
            done, reason = True, 2
        if self._mated():
            reward, done, reason = reward - 100, True, 8
        if self.s.white:
            self.mc += 1
        self.done = done
        return reward, done, reason
