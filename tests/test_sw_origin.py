"""The tail of the self-play pick (gc_core.h), host-compiled.

sw_origin turns a move set and a target into the origin.  For a slider set that is the nearest
occupied square behind the target on the set's line; the function finds it at the line's stride
without clipping the line to the board, so every slider set, target and origin is run here on
occupancies that fill the rest of the board at will -- the squares the stride reaches past a
board edge among them -- against a plain walk over rows and columns.  The leaper sets return the
target plus the set's offset.

sw_locate_pre finds a rank's set from the byte prefixes of the count words, which the fused ply's
three makers (Q0, Q2, Q3) hand over summed; it must return what sw_locate returns from the words.

The apply without the castle terms (the fused ply uses it where no lane of a wave castles) must
equal apply_legal on every move that is no castle."""
import os
import sys

import numpy as np

from conftest import random_positions

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
import corehost as H  # noqa: E402
import sworiginhost as S  # noqa: E402

SW_ORTH, SW_K, SW_SETS = 12, 20, 28
# slider set SW_ORTH + d: the step (rows, columns) from the origin to its targets (gc_core.h sw_orth, sw_diag)
SLIDER_STEP = [(-1, 0), (1, 0), (0, 1), (0, -1), (-1, 1), (-1, -1), (1, 1), (1, -1)]
# leaper set -> target - origin (sw_pawns_kl by colour, sw_knights, sw_kings)
PAWN_WHITE = [-8, -16, -7, -9]
PAWN_BLACK = [8, 16, 9, 7]
KNIGHT = [15, 17, -17, -15, 6, 10, -10, -6]
KING = [-8, 8, -1, 1, -9, -7, 7, 9]
RANDOM_FILLS = 64


def walk_back(occ, to, step):
    """the first occupied square behind `to`, square by square against the set's step (None: the edge)"""
    r, c = divmod(to, 8)
    while True:
        r, c = r - step[0], c - step[1]
        if not (0 <= r < 8 and 0 <= c < 8):
            return None
        if (occ >> (8 * r + c)) & 1:
            return 8 * r + c


def run_origin(occ, white, j, to):
    L = S.lib()
    occ = np.ascontiguousarray(occ, dtype=np.uint64)
    white = np.ascontiguousarray(white, dtype=np.uint8)
    j = np.ascontiguousarray(j, dtype=np.int32)
    to = np.ascontiguousarray(to, dtype=np.int32)
    out = np.zeros(len(occ), dtype=np.int32)
    L.so_origin(occ.ctypes.data, white.ctypes.data, j.ctypes.data, to.ctypes.data, len(occ), out.ctypes.data)
    return out


def test_slider_origins_exhaustive():
    rng = np.random.RandomState(0x51DE)
    full = (1 << 64) - 1
    occs, js, tos, want = [], [], [], []
    lines = 0
    for d, step in enumerate(SLIDER_STEP):
        for to in range(64):
            r, c = divmod(to, 8)
            between = 0  # the squares the ray came through
            while True:
                r, c = r - step[0], c - step[1]
                if not (0 <= r < 8 and 0 <= c < 8):
                    break
                origin = 8 * r + c
                lines += 1
                # the origin occupied, the squares between empty, the rest (the target too: a capture) at will
                free = full & ~between & ~(1 << origin)
                rnd = rng.randint(0, 1 << 32, size=RANDOM_FILLS, dtype=np.uint64) << np.uint64(32) | \
                    rng.randint(0, 1 << 32, size=RANDOM_FILLS, dtype=np.uint64)
                for fill in [0, full] + [int(x) for x in rnd]:
                    occ = (1 << origin) | (fill & free)
                    occs.append(occ)
                    js.append(SW_ORTH + d)
                    tos.append(to)
                    want.append(walk_back(occ, to, step))
                between |= 1 << origin
    assert lines == 4 * 224 + 4 * 140  # the squares behind every target: 28 per file or row, min(row, column) sums
    want = np.array(want, dtype=np.int32)
    # by construction the walk ends on the origin the case was built around
    got = run_origin(occs, np.ones(len(occs)), js, tos)
    got_black = run_origin(occs, np.zeros(len(occs)), js, tos)
    bad = np.nonzero((got != want) | (got_black != want))[0]
    assert len(bad) == 0, (len(bad), js[bad[0]], tos[bad[0]], hex(occs[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))
    print(f"{lines} (set, target, origin) lines x {RANDOM_FILLS + 2} fills = {len(occs)} cases")
    assert len(occs) == lines * (RANDOM_FILLS + 2)


def test_leaper_sets_return_target_plus_offset():
    occs, whites, js, tos, want = [], [], [], [], []
    rng = np.random.RandomState(0x1EA9)
    for white in (1, 0):
        offs = {j: o for j, o in enumerate(PAWN_WHITE if white else PAWN_BLACK)}
        offs.update({4 + k: o for k, o in enumerate(KNIGHT)})
        offs.update({SW_K + k: o for k, o in enumerate(KING)})
        assert sorted(offs) == [j for j in range(SW_SETS) if not SW_ORTH <= j < SW_K]
        for j, off in offs.items():
            for to in range(64):
                for occ in (0, (1 << 64) - 1, int(rng.randint(0, 1 << 62, dtype=np.int64))):
                    occs.append(occ)
                    whites.append(white)
                    js.append(j)
                    tos.append(to)
                    want.append(to - off)  # the origin: the target less the set's step
    got = run_origin(occs, whites, js, tos)
    bad = np.nonzero(got != np.array(want, dtype=np.int32))[0]
    assert len(bad) == 0, (len(bad), whites[bad[0]], js[bad[0]], tos[bad[0]], int(got[bad[0]]), want[bad[0]])


def locate_cases():
    """28 counts per case, totals 1 .. 255: a lone move in every set, totals of 255 packed in few
    sets and spread over many, makers' words left empty, and seeded random counts"""
    rng = np.random.RandomState(0x10CA)
    cases = []
    for j in range(SW_SETS):  # total 1
        c = np.zeros(SW_SETS, dtype=np.int64)
        c[j] = 1
        cases.append(c)
    for j in range(SW_SETS):  # total 255 in one set, and in two
        c = np.zeros(SW_SETS, dtype=np.int64)
        c[j] = 255
        cases.append(c)
        c = np.zeros(SW_SETS, dtype=np.int64)
        c[j], c[(j + 9) % SW_SETS] = 64, 191
        cases.append(c)
    groups = {"q0": range(0, 12), "q2": list(range(12, 16)) + list(range(20, 28)), "q3": range(16, 20),
              "word0": range(0, 8), "word1": range(8, 16), "word2": range(16, 24), "word3": range(24, 28)}
    for rep in range(400):
        hi = (2, 8, 28, 64)[rep % 4]
        c = rng.randint(0, hi + 1, size=SW_SETS).astype(np.int64)
        if rep % 5 == 1:  # sparse
            c *= rng.randint(0, 2, size=SW_SETS)
        if rep % 3 == 2:  # a maker's sets, or a word's, left empty
            c[list(groups[sorted(groups)[rep % len(groups)]])] = 0
        while c.sum() > 255:  # scaled back below 256
            c = c * 3 // 4
        if rep % 10 == 9 and c.sum() > 0:  # topped up to exactly 255
            c[int(np.flatnonzero(c)[0])] += 255 - c.sum()
        if c.sum() > 0:
            cases.append(c)
    return np.array(cases, dtype=np.uint8)


def test_locate_from_prefixes_equals_locate_from_words():
    L = S.lib()
    cases = np.ascontiguousarray(locate_cases())
    totals = cases.astype(np.int64).sum(axis=1)
    assert totals.min() == 1 and totals.max() == 255 and (totals == 255).sum() > 28
    words = np.stack([cases[:, 8 * w:8 * w + 8].astype(np.int64).sum(axis=1) for w in range(4)], axis=1)
    assert all((words[:, w] == 0).any() for w in range(4))  # empty words occur
    ranks = np.zeros(1, dtype=np.int64)
    first = np.zeros(2, dtype=np.int64)
    bad = L.so_locate(cases.ctypes.data, len(cases), ranks.ctypes.data, first.ctypes.data)
    assert bad == 0, (bad, cases[first[0]].tolist(), int(first[1]))
    assert ranks[0] == totals.sum()


def test_apply_without_castle_terms_equals_apply_legal():
    L = S.lib()
    first = np.zeros(1, dtype=np.int64)
    moves = 0
    boards, metas = random_positions(1500, 74)
    for b, m in zip(boards, metas):
        b = np.ascontiguousarray(b, dtype=np.int8)
        m = np.ascontiguousarray(m, dtype=np.uint8)
        acts = np.array([a for a in H.get_list(b, m, int(m[0])) if a < 4096], dtype=np.uint16)
        if len(acts) == 0:
            continue
        bad = L.so_apply_plain(b.ctypes.data, m.ctypes.data, acts.ctypes.data, len(acts), first.ctypes.data)
        assert bad == 0, (b.tolist(), m.tolist(), int(acts[first[0]]))
        moves += len(acts)
    assert moves > 10000, moves
