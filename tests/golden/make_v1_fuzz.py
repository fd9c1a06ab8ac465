#!/usr/bin/env python3
"""Generate tests/golden/v1_fuzz.json.gz: the reference's own v1 engine on fuzzed boards.

Runs ONLY in the build container (needs the reference checkout, like make_golden.py, whose
loader, D4 transform, v1 perft, divergence walk and D1/D2 filters it imports).  Data only.

Every position has exactly one king per side and passes the D1/D2 filters (the mover cannot
capture the enemy king; the kings are not adjacent); the four rights are all on or all off, so
v1's AND gate and v2's OR gate agree (D3).  Families:
  sparse  random_positions(weird=False) boards, 2-25 pieces, both sides to move
  castle  kings and rooks on home squares: path squares occupied / attacked, rights on / off,
          the king checked or not; the Q4 shape (Black to move, positive ids on a8/e8/h8)
  pawns   Q1 jumps, last-rank pawns of both colours (Q2), black capture pairs (D4), pawn
          captures of every piece type
  checks  slider checks with the square behind the king free (Q6 retreat), double checks, one
          and two pins (a pinned pawn on its start square next to its king), knight checks
  late    positions from plies >= 100 of ten further seeded v1 random games

Per position: board, side to move, rights; v1's ordered list (D4-transformed); for EVERY listed
move v1's next board and reward (next_state(commit=False)), v1's king_is_checked for both
colours on the next board (null where v1 raises) and the length of v1's list for the other side
there (null where v1 raises or where v1 and v2 count differently: D1/D2 on the next board);
with the rights off, v1 perft(1), perft(2) and, for every fifth such position, perft(3), stored
as v1_perft_midgame.json stores them (v1_equals_v2, or the v1_divergences list).

Usage:  python tests/golden/make_v1_fuzz.py [--procs N]
"""
import argparse
import multiprocessing as mp
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402
from make_golden import C, O  # noqa: E402

FAMILIES = ("sparse", "castle", "pawns", "checks", "late")
CANDIDATES = {"sparse": 330, "castle": 400, "pawns": 320, "checks": 300, "late": 170}
SEEDS = {"sparse": 9101, "castle": 9102, "pawns": 9103, "checks": 9104, "late": 9105}
ORTH = [(-1, 0), (1, 0), (0, -1), (0, 1)]
DIAG = [(-1, -1), (-1, 1), (1, -1), (1, 1)]
KNIGHT = [(-2, -1), (-2, 1), (2, -1), (2, 1), (-1, -2), (-1, 2), (1, -2), (1, 2)]


def _on(r, c):
    return 0 <= r < 8 and 0 <= c < 8


def _free(b, avoid=()):
    return [s for s in range(64) if b[s] == 0 and s not in avoid]


def _drop(rng, b, ids, n, avoid=(), rows=range(8)):
    """n random pieces from ids on free squares of the given rows"""
    for _ in range(n):
        fr = [s for s in _free(b, avoid) if s // 8 in rows]
        if not fr:
            return
        b[fr[rng.randint(len(fr))]] = ids[rng.randint(len(ids))]


def _far_king(rng, b, v, other_king, avoid=()):
    """king v on a free square not next to the other king"""
    fr = [s for s in _free(b, avoid)
          if max(abs(s // 8 - other_king // 8), abs(s % 8 - other_king % 8)) > 1]
    b[fr[rng.randint(len(fr))]] = v


# --------------------------------------------------------------------------- candidates
def cand_sparse(n, seed):
    from conftest import random_positions

    boards, metas = random_positions(n, seed, weird=False)
    return [(boards[i].copy(), bool(metas[i, 0]), bool(metas[i, 1])) for i in range(n)]


def cand_castle(n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        b = np.zeros(64, dtype=np.int8)
        shape = i % 8
        if shape <= 5:  # White at home, White to move
            b[60] = 1
            for s in (56, 63):
                if rng.rand() < 0.95:
                    b[s] = 3
            avoid = set()
            if i % 16 == 0:  # a check down the e-file
                r = rng.randint(0, 6)
                b[r * 8 + 4] = -3 if rng.rand() < 0.5 else -2
                avoid = {k * 8 + 4 for k in range(8)}
            for s in (57, 58, 59, 61, 62):
                if rng.rand() < 0.08:
                    b[s] = [5, 4, 2, -5, -4][rng.randint(5)]
            _far_king(rng, b, -1, 60, avoid | set(range(32, 64)))
            _drop(rng, b, [-2, -3, -4, -5, -6, -6, -6], rng.randint(1, 4), avoid, rows=range(0, 7))
            _drop(rng, b, [2, 4, 5, 6, 6], rng.randint(0, 3), avoid, rows=range(1, 7))
            white = True
        else:  # Black to move; shape 6 = the Q4 shape: POSITIVE ids on a8/e8/h8
            k, rk = (1, 3) if shape == 6 else (-1, -3)
            b[4] = k
            for s in (0, 7):
                if rng.rand() < 0.9:
                    b[s] = rk
            for s in (1, 2, 3, 5, 6):
                if rng.rand() < 0.12:
                    b[s] = [5, 4, -5, -4][rng.randint(4)]
            _far_king(rng, b, -k, 4, set(range(0, 16)))
            _drop(rng, b, [2, 3, 4, 5, 6], rng.randint(1, 4), rows=range(2, 8))
            _drop(rng, b, [-2, -4, -5, -6, -6], rng.randint(1, 5), rows=range(1, 7))
            white = False
        out.append((b, white, rng.rand() < 0.85))
    return out


def cand_pawns(n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        b = np.zeros(64, dtype=np.int8)
        wk = rng.randint(64)
        b[wk] = 1
        _far_king(rng, b, -1, wk)
        for sgn, start, last, first in ((1, 6, 0, 7), (-1, 1, 7, 0)):
            for _ in range(rng.randint(3, 8)):
                u = rng.rand()
                row = start if u < 0.45 else last if u < 0.58 else first if u < 0.62 else rng.randint(1, 7)
                s = row * 8 + rng.randint(8)
                if b[s] != 0:
                    continue
                b[s] = 6 * sgn
                fwd = row - sgn
                if row == start and rng.rand() < 0.65 and b[fwd * 8 + s % 8] == 0:  # Q1: a blocker to jump
                    b[fwd * 8 + s % 8] = [2, 3, 4, 5, 6, -2, -3, -4, -5, -6][rng.randint(10)]
                pair = rng.rand() < 0.4  # both diagonals: the D4 capture pair
                for dc in (-1, 1):
                    if _on(fwd, s % 8 + dc) and b[fwd * 8 + s % 8 + dc] == 0 and (pair or rng.rand() < 0.3):
                        b[fwd * 8 + s % 8 + dc] = -sgn * [2, 3, 4, 5, 6][rng.randint(5)]
        out.append((b, i % 2 == 0, rng.rand() < 0.5))
    return out


def _ray(b, k, d, length):
    """the squares k + d .. k + length * d if all on the board and empty, else None"""
    sq = []
    for j in range(1, length + 1):
        r, c = k // 8 + j * d[0], k % 8 + j * d[1]
        if not _on(r, c) or b[r * 8 + c] != 0:
            return None
        sq.append(r * 8 + c)
    return sq


def _slider(rng, d, sgn):
    ids = [3, 2] if d in ORTH else [4, 2]
    return sgn * ids[rng.randint(2)]


def cand_checks(n, seed):
    rng = np.random.RandomState(seed)
    out = []
    i = 0
    while len(out) < n:
        kind = i % 5
        i += 1
        white = bool(rng.randint(2))
        me = 1 if white else -1
        b = np.zeros(64, dtype=np.int8)
        keep = set()  # squares the shape needs as they are
        two_file = kind == 3 and rng.rand() < 0.5
        if two_file:  # the pawn on its start square, its king in front of it, both on a pinning file
            c = rng.randint(8)
            k = (5 if white else 2) * 8 + c
            back = (1, 0) if white else (-1, 0)
            b[k] = me
            b[k + 8 * back[0]] = 6 * me
            b[k + 16 * back[0]] = -me * [3, 2][rng.randint(2)]
            front = _ray(b, k, (-back[0], 0), rng.randint(2, 5))
            b[front[rng.randint(len(front) - 1)]] = me * [2, 3, 4, 5, 6][rng.randint(5)]
            b[front[-1]] = -me * [3, 2][rng.randint(2)]
            keep = {k, k + 8 * back[0], k + 16 * back[0]} | set(front)
        else:
            k = rng.randint(64)
            b[k] = me
            keep.add(k)
            dirs = [ORTH[j] for j in rng.permutation(4)] + [DIAG[j] for j in rng.permutation(4)]
            dirs = [dirs[j] for j in rng.permutation(8)]
            ok = True
            if kind == 0:  # slider check, the square behind the king free (Q6 retreat)
                ok = False
                for d in dirs:
                    behind = _ray(b, k, (-d[0], -d[1]), 1)
                    ray = _ray(b, k, d, rng.randint(2, 5))
                    if behind and ray:
                        b[ray[-1]] = _slider(rng, d, -me)
                        keep |= set(behind) | set(ray)
                        ok = True
                        break
            elif kind == 1:  # double check: slider + knight, or two sliders
                got = 0
                for d in dirs:
                    ray = _ray(b, k, d, rng.randint(1, 5))
                    if ray and got < (1 if i % 2 else 2):
                        b[ray[-1]] = _slider(rng, d, -me)
                        keep |= set(ray)
                        got += 1
                if i % 2:
                    for j in rng.permutation(8):
                        r, c = k // 8 + KNIGHT[j][0], k % 8 + KNIGHT[j][1]
                        if _on(r, c) and b[r * 8 + c] == 0:
                            b[r * 8 + c] = -5 * me
                            keep.add(r * 8 + c)
                            got += 1
                            break
                ok = got == 2
            elif kind in (2, 3):  # one / two pinned pieces
                got = 0
                for d in dirs:
                    ray = _ray(b, k, d, rng.randint(2, 6))
                    if ray and got < kind - 1:
                        pin = ray[rng.randint(len(ray) - 1)]
                        b[pin] = me * [2, 3, 4, 5, 6, 6][rng.randint(6)]
                        b[ray[-1]] = _slider(rng, d, -me)
                        keep |= set(ray)
                        got += 1
                ok = got == kind - 1
            else:  # knight check
                ok = False
                for j in rng.permutation(8):
                    r, c = k // 8 + KNIGHT[j][0], k % 8 + KNIGHT[j][1]
                    if _on(r, c):
                        b[r * 8 + c] = -5 * me
                        keep.add(r * 8 + c)
                        ok = True
                        break
            if not ok:
                continue
        _far_king(rng, b, -me, k, keep)
        _drop(rng, b, [2, 3, 4, 5, 6, 6, -2, -3, -4, -5, -6, -6], rng.randint(0, 7), keep)
        # Q6 retreats make v1 != v2 one ply later (D1): those shapes mostly carry the rights, so
        # that the perft entries (rights off) stay under the issue's cap on non-equal entries
        rights = rng.rand() < (0.95 if kind == 0 else 0.5)
        out.append((b, white, rights))
    return out


def cand_late(n, seed):
    v1 = G.load_reference()[0] if G._V1 is None else G._V1
    G._V1 = v1
    out = []
    for g in range(10):
        rng = np.random.RandomState(seed + g)
        env = v1.ChessEnvV1(opponent="none", log=False)
        env.state = env.state.copy()
        for ply in range(320):
            try:
                moves = env.possible_moves
                if not moves:
                    break
                if ply >= 100 and ply % 3 == g % 3:
                    out.append((np.asarray(env.state, dtype=np.int8).reshape(64).copy(),
                                env.current_player == "WHITE", bool(rng.randint(2))))
                _, _, done, _ = env.step(env.move_to_action(moves[rng.randint(len(moves))]))
            except Exception:  # D10 after a king capture: v1 cannot go on
                break
            if done:
                break
    return out[:n]


CAND = {"sparse": cand_sparse, "castle": cand_castle, "pawns": cand_pawns, "checks": cand_checks, "late": cand_late}


# --------------------------------------------------------------------------- v1 runs
def _set_rights(env, on):
    env.white_king_castle_possible = env.white_queen_castle_possible = bool(on)
    env.black_king_castle_possible = env.black_queen_castle_possible = bool(on)


def screen(board, white):
    """the drop reason of a candidate, or None"""
    if int((board == 1).sum()) != 1 or int((board == -1).sum()) != 1:
        return "kings"
    if G.attack_hits_king(board, white):
        return "D1"
    if G.kings_adjacent(board):
        return "D2"
    return None


def _env():
    if G._V1 is None:
        G._V1 = G.load_reference()[0]
    return G._V1.ChessEnvV1(opponent="none", log=False)


def build_entry(job):
    """(family, board, white, rights on) -> the entry, or the drop reason (a str)"""
    family, board, white, on = job
    why = screen(board, white)
    if why:
        return why
    env = _env()
    me, other = ("WHITE", "BLACK") if white else ("BLACK", "WHITE")
    st = board.reshape(8, 8).copy()
    env.state = st  # D5
    _set_rights(env, on)
    try:
        moves = env.get_possible_moves(state=st, player=me)
        acts = G.d4_transform(G.v1_list_to_actions(moves), board)
    except Exception:
        return "v1_raised"
    by_action = dict(zip(G.v1_list_to_actions(moves), moves))
    nxt, rewards, flags, next_n, raw_n = [], [], [], [], []
    for a in acts:
        _set_rights(env, on)  # D7/D12: a castle run clears the env's flags even uncommitted
        env.state = st
        try:
            ns, rw = env.next_state(st, me, by_action[a], commit=False)
        except Exception:
            return "v1_raised"
        nb = np.asarray(ns, dtype=np.int8).reshape(64)
        nxt.append(C.board_to_text(nb))
        rewards.append(int(rw))
        env.state = ns
        try:
            flags.append([int(bool(env.king_is_checked(state=ns, player="WHITE"))),
                          int(bool(env.king_is_checked(state=ns, player="BLACK")))])
        except Exception:
            flags.append(None)
        _set_rights(env, on)
        try:
            cnt = len(env.get_possible_moves(state=ns, player=other))
        except Exception:
            cnt = None
        raw_n.append(cnt)
        same_count = cnt is not None and screen(nb, not white) is None
        next_n.append(cnt if same_count else None)
    e = dict(family=family, board=C.board_to_text(board), white=bool(white), rights=[int(on)] * 4, moves=acts,
             next_boards=nxt, rewards=rewards, flags=flags, next_n=next_n)
    if not on:
        e["v1_perft"] = {"1": len(acts)}
        if all(c is not None for c in raw_n):
            e["v1_perft"]["2"] = int(sum(raw_n))
    return e


def perft3(job):
    board_text, white = job
    env = _env()
    _set_rights(env, False)
    st = C.text_to_board(board_text).reshape(8, 8).copy()
    try:
        return int(G.v1_perft(env, st, "WHITE" if white else "BLACK", 3, env.get_other_player))
    except Exception:  # D2/D10 inside the tree: v1 cannot arbitrate
        return None


def classify(e):
    """v1_perft_midgame.json's form: v1_equals_v2, or else the divergence walk"""
    board = C.text_to_board(e["board"])
    meta = O.make_meta(e["white"], 0, 0, 0, 0)
    e["v1_equals_v2"] = all(O.perft(board, meta, int(d)) == v for d, v in e["v1_perft"].items())
    if not e["v1_equals_v2"]:
        _env()  # loads G._V1 in a fresh worker
        divs, all_d1 = G.v1_divergences(G._V1, board, e["white"], len(e["v1_perft"]))
        e["d1_divergences"] = divs
        e["all_divergences_are_D1"] = bool(all_d1)
    return e


def generate_family(name, pool=None):
    """-> (entries, stats) of one family; deterministic (seeded candidates, ordered maps)"""
    cands = CAND[name](CANDIDATES[name], SEEDS[name])
    run = pool.map if pool is not None else lambda f, xs, chunksize=1: [f(x) for x in xs]
    res = run(build_entry, [(name, b, w, on) for b, w, on in cands], chunksize=4)
    drops = {}
    for r in res:
        if isinstance(r, str):
            drops[r] = drops.get(r, 0) + 1
    entries = [r for r in res if not isinstance(r, str)]
    off = [e for e in entries if "v1_perft" in e]
    deep = [e for e in off[::5] if "2" in e["v1_perft"]]
    for e, v in zip(deep, run(perft3, [(e["board"], e["white"]) for e in deep], chunksize=1)):
        if v is not None:
            e["v1_perft"]["3"] = v
    for e, c in zip(off, run(classify, off, chunksize=2)):
        e.update(c)
    lists_equal = sum(O.get_possible_moves(C.text_to_board(e["board"]), O.make_meta(e["white"], *e["rights"]),
                                           e["white"]) == e["moves"] for e in entries)
    stats = dict(candidates=len(cands), kept=len(entries), drops=drops, moves=sum(len(e["moves"]) for e in entries),
                 lists_equal_to_oracle=int(lists_equal), perft_entries=len(off),
                 perft3_entries=sum("3" in e["v1_perft"] for e in off),
                 perft_equal=sum(e["v1_equals_v2"] for e in off),
                 perft_not_equal_all_D1=sum(not e["v1_equals_v2"] and e["all_divergences_are_D1"] for e in off),
                 perft_not_equal_other=sum(not e["v1_equals_v2"] and not e["all_divergences_are_D1"] for e in off))
    return entries, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    G._V1 = G.load_reference()[0]
    positions, summary = [], {}
    with mp.Pool(args.procs) as pool:
        for name in FAMILIES:
            t0 = time.time()
            entries, stats = generate_family(name, pool)
            positions += entries
            summary[name] = stats
            print(name, stats, f"({time.time() - t0:.0f} s)", flush=True)
    n_perft = sum(s["perft_entries"] for s in summary.values())
    n_neq = n_perft - sum(s["perft_equal"] for s in summary.values())
    summary["perft_not_equal_share"] = round(n_neq / max(n_perft, 1), 4)
    print(f"positions {len(positions)}, moves {sum(len(e['moves']) for e in positions)}, perft entries {n_perft}, "
          f"v1 != v2 on {n_neq} ({100.0 * n_neq / max(n_perft, 1):.1f} %; cap 25 %)", flush=True)
    G.dump("v1_fuzz.json.gz", dict(summary=summary, positions=positions), gz=True)


if __name__ == "__main__":
    main()
