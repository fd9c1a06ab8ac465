"""The rank-direction fills by carry propagation (gc_core.h: rank_fill_att / rank_fill_to /
rank_fill_pair) against the Kogge-Stone templates they replace along a rank, on the host build.
Precondition of the new forms: the generators are pieces (gen within occ)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import random_positions

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
import rankfillhost as RF  # noqa: E402

FORMS = ("att east", "att west", "to east", "to west", "pair east (1st)", "pair east (2nd)", "pair west (1st)",
         "pair west (2nd)", "att east (shared operands)", "att west (shared)", "to east (shared)", "to west (shared)")
FILE_A = 0x0101010101010101
FILE_H = 0x8080808080808080
ROW = [0xFF << (8 * r) for r in range(8)]

# A start position crowded with rooks and queens (12 pieces a side, both kings): sliders on
# files A and H and along the back ranks, three adjacent on a rank, two ranks with a slider on
# both edge files.  Row 0 is black's back rank; positive ids are white (K Q R B N P = 1..6).
HEAVY_BOARD = np.array([
    -3, -2, -3, 0, -1, 0, -2, -3,
    -3, 0, 0, -6, -6, 0, 0, -2,
    -2, 0, 0, 0, 0, 0, 0, -3,
    0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0,
    3, 0, 0, 0, 0, 0, 0, 2,
    2, 0, 0, 6, 6, 0, 0, 3,
    3, 2, 3, 0, 1, 0, 2, 3,
], dtype=np.int8)


def _rand64(rng, n):
    return rng.randint(0, 2**32, size=n, dtype=np.uint64) << np.uint64(32) | rng.randint(0, 2**32, size=n, dtype=np.uint64)


def _check(occ, ge, go, tm, what):
    occ, ge, go, tm = (np.ascontiguousarray(x, dtype=np.uint64) for x in (occ, ge, go, tm))
    assert not (ge & ~occ).any() and not (go & ~occ).any()  # the precondition
    first = np.zeros(2, dtype=np.int64)
    bad = RF.lib().rf_compare(occ.ctypes.data, ge.ctypes.data, go.ctypes.data, tm.ctypes.data, len(occ),
                              first.ctypes.data)
    if bad:
        i = int(first[0])
        out = np.zeros(4, dtype=np.uint64)
        RF.lib().rf_eval(int(occ[i]), int(ge[i]), out.ctypes.data)
        forms = [FORMS[k] for k in range(len(FORMS)) if first[1] >> k & 1]
        pytest.fail(f"{what}: {bad} of {len(occ)} cases differ; first: case {i} occ {int(occ[i]):#018x} "
                    f"gen {int(ge[i]):#018x} 2nd gen {int(go[i]):#018x} tm {int(tm[i]):#018x} forms {forms} "
                    f"(new east/west {int(out[0]):#x} {int(out[1]):#x}, Kogge-Stone {int(out[2]):#x} {int(out[3]):#x})")


def _rank_pairs():
    """all 6 561 (occupancy byte, generators within it)"""
    o, g = [], []
    for occ in range(256):
        sub = occ
        while True:  # every subset of occ
            o.append(occ)
            g.append(sub)
            if sub == 0:
                break
            sub = (sub - 1) & occ
    assert len(o) == 6561
    return np.array(o, dtype=np.uint64), np.array(g, dtype=np.uint64)


@pytest.mark.parametrize("which", ["first", "second"])
def test_rank_fills_exhaustive_on_one_rank(which):
    """Every (occupancy, generators) of one rank, in each of the 8 ranks, the other ranks random
    (a rank's result depends on that rank alone: nothing may leak across); both directions, the
    attack and the target forms (random target masks), the paired form's two generator sets."""
    rng = np.random.RandomState(11 if which == "first" else 12)
    ob, gb = _rank_pairs()
    occs, ges, gos, tms = [], [], [], []
    for r in range(8):
        n = len(ob)
        keep = np.uint64(~ROW[r] & (2**64 - 1))
        occ = (_rand64(rng, n) & _rand64(rng, n) & keep) | (ob << np.uint64(8 * r))
        if r & 1:  # dense neighbours every other rank
            occ = (_rand64(rng, n) | _rand64(rng, n)) & keep | (ob << np.uint64(8 * r))
        ex = (occ & keep & _rand64(rng, n)) | (gb << np.uint64(8 * r))  # the exhaustive generator set
        other = occ & _rand64(rng, n)
        occs.append(occ)
        ges.append(ex if which == "first" else other)
        gos.append(other if which == "first" else ex)
        tms.append(_rand64(rng, n))
    _check(np.concatenate(occs), np.concatenate(ges), np.concatenate(gos), np.concatenate(tms), f"exhaustive ({which})")


def test_rank_fills_random_boards():
    """10^5 random full boards with the generators within the occupancy, and the edge cases by
    hand: gen == occ, the empty board, sliders on files A and H, adjacent sliders, full ranks."""
    rng = np.random.RandomState(5)
    n = 100000
    occ = _rand64(rng, n)
    dens = rng.randint(4, size=n)
    occ = np.where(dens == 0, occ & _rand64(rng, n) & _rand64(rng, n), occ)
    occ = np.where(dens == 1, occ & _rand64(rng, n), occ)
    occ = np.where(dens == 3, occ | _rand64(rng, n), occ)
    ge = occ & _rand64(rng, n)
    go = occ & _rand64(rng, n) & _rand64(rng, n)
    k = n // 20
    ge[:k] = occ[:k]  # gen == occ
    go[k:2 * k] = occ[k:2 * k]
    ge[2 * k:3 * k] = occ[2 * k:3 * k] & np.uint64(FILE_A | FILE_H)  # sliders on the edge files only
    ge[3 * k:4 * k] = occ[3 * k:4 * k] & (occ[3 * k:4 * k] << np.uint64(1))  # ... next to a piece
    tm = _rand64(rng, n)
    full = 2**64 - 1
    hand = [  # (occ, gen, 2nd gen)
        (0, 0, 0), (full, full, full), (full, 0, FILE_A), (full, FILE_H, FILE_A),
        (FILE_A, FILE_A, FILE_A), (FILE_H, FILE_H, FILE_H), (FILE_A | FILE_H, FILE_A, FILE_H),
        (FILE_A | FILE_H, FILE_A | FILE_H, 0), (0xFF, 0xFF, 0x81), (0xFF << 56, 0xFF << 56, 0x81 << 56),
        (0x03, 0x03, 0x01), (0xC0 << 56, 0xC0 << 56, 0x80 << 56), (0x18 << 24, 0x18 << 24, 0x10 << 24),
        (0x8100000000000081, 0x8100000000000081, 0x8000000000000001), (1, 1, 1), (1 << 63, 1 << 63, 1 << 63),
        (0x00FF00FF00FF00FF, 0x0081008100810081, 0x00FF00FF00FF00FF), (0x7E7E7E7E7E7E7E7E, 0x7E7E7E7E7E7E7E7E, 0),
    ]
    ho = np.array([h[0] for h in hand], dtype=np.uint64)
    hg = np.array([h[1] for h in hand], dtype=np.uint64)
    h2 = np.array([h[2] for h in hand], dtype=np.uint64)
    for t in (np.uint64(full), np.uint64(0x5A5A5A5A5A5A5A5A)):
        _check(ho, hg, h2, np.full(len(hand), t), "edge cases")
    _check(occ, ge, go, tm, "random boards")


def heavy_positions(n, seed):
    """rook/queen-heavy positions: HEAVY_BOARD with pieces dropped, moved and recoloured at random"""
    rng = np.random.RandomState(seed)
    boards = np.zeros((n, 64), dtype=np.int8)
    metas = np.zeros((n, 8), dtype=np.uint8)
    for i in range(n):
        b = HEAVY_BOARD.copy()
        for sq in np.nonzero(b)[0]:
            if abs(b[sq]) == 1:
                continue
            u = rng.rand()
            if u < 0.15:
                b[sq] = 0
            elif u < 0.45:  # to a random empty square (often onto a slider's rank)
                free = np.nonzero(b == 0)[0]
                to = int(free[rng.randint(len(free))])
                b[to], b[sq] = b[sq], 0
            elif u < 0.55:
                b[sq] = -b[sq]
        boards[i] = b
        metas[i, 0] = rng.randint(2)
        metas[i, 1:5] = rng.randint(2, size=4)
    boards[0] = HEAVY_BOARD
    return boards, metas


@pytest.mark.parametrize("kind", ["fuzz", "heavy"])
def test_converted_callers_on_positions(oracle, kind):
    """side_attacks_orth, sw_orth (plain and with the carried operands) and count_moves /
    count_position on whole positions: the same sets as with the Kogge-Stone templates in all
    directions, and the oracle's move count."""
    boards, metas = random_positions(400, 91) if kind == "fuzz" else heavy_positions(400, 92)
    L = RF.lib()
    for i in range(len(boards)):
        b, m = np.ascontiguousarray(boards[i]), np.ascontiguousarray(metas[i])
        for white in (0, 1):
            c = ctypes.c_int(-1)
            bad = L.rf_position(b.ctypes.data, m.ctypes.data, white, ctypes.byref(c))
            assert bad == 0, (kind, i, white, bin(bad))
            assert c.value == len(oracle.get_possible_moves(b, m, white)), (kind, i, white)
