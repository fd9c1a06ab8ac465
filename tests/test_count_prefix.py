"""The fused ply's count words and pick (gc_core.h), host-compiled.

The ply's three makers of move sets (Q0: pawns and knights, Q2: rook / queen and king sets, Q3:
bishop / queen sets) hand the pick the byte prefixes of the sets' counts.  They make them as
running sums carried through the popcounts (sw_prefix_make), not from packed counts by a pass of
byte_prefix: here the makers' words, summed, must be byte_prefix of sw_pack's words bit for bit,
and each maker's own words hold 0 before its first set and the word's total after its last.
sw_locate_pre compares on 32-bit halves without a multiply: it must return the (set, rank) of its
multiply form and of a plain scan for every rank.  The pick from fetched sets (sw_pick_sets:
sw_locate_pre, sw_finish with the straight-line sw_origin, the scan for 256 moves and more behind
the wave's flag) must be sw_select for every rank -- on the move sets of the 206 shared positions
with either side to move, whose list must also be the host core's legal list, and on synthetic
sets; totals of 256 and more never occur in play, so that path runs on synthetic sets only.
kth_set_bit is unchanged.  sw_select and sw_pick_sets both call sw_origin, so a fault in sw_origin
would be common to both sides of those comparisons -- the synthetic-set test, the 256-move path
included, would not see it: sw_origin's own checks are the comparison with the host core's legal
list on the 206 positions here and tests/test_sw_origin.py, which walks its lines square by square."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
import corehost as H  # noqa: E402
import countprefixhost as CP  # noqa: E402
import playout_cases as PC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SW_ORTH, SW_DIAG, SW_K, SW_SETS = 12, 16, 20, 28
FULL = (1 << 64) - 1
MAKERS = {"q0": list(range(0, 12)), "q2": list(range(12, 16)) + list(range(20, 28)), "q3": list(range(16, 20))}


def rand_set(rng, bits):
    """a 64-bit set of `bits` distinct random squares"""
    x = 0
    for sq in rng.choice(64, size=bits, replace=False):
        x |= 1 << int(sq)
    return x


def sets_of_counts(rng, counts):
    return [rand_set(rng, int(c)) for c in counts]


def prefix_cases():
    """cases of 28 sets, totals 0 .. 255: empty sets, one full word (64 squares in one set), all of
    a word's moves in one byte, totals of exactly 255, makers' and words' sets left empty, random"""
    rng = np.random.RandomState(0xC0DE)
    cases = [[0] * SW_SETS]
    for j in range(SW_SETS):
        cases.append([FULL if i == j else 0 for i in range(SW_SETS)])  # one full word, the rest empty
        c = np.zeros(SW_SETS, dtype=np.int64)
        c[j] = 1
        cases.append(sets_of_counts(rng, c))
        c[j] = 63
        c[(j + 1) % SW_SETS] = 64
        c[(j + 13) % SW_SETS] = 64
        c[(j + 20) % SW_SETS] = 64  # 255 in four sets
        cases.append(sets_of_counts(rng, c))
    for w in range(4):  # all of a word in one byte, the other words busy
        for b in range(8 if w < 3 else 4):
            c = rng.randint(0, 5, size=SW_SETS).astype(np.int64)
            c[8 * w:8 * w + 8] = 0
            c[8 * w + b] = 40
            cases.append(sets_of_counts(rng, c))
    groups = dict(MAKERS, word0=range(0, 8), word1=range(8, 16), word2=range(16, 24), word3=range(24, 28))
    for rep in range(500):
        hi = (2, 8, 28, 64)[rep % 4]
        c = rng.randint(0, hi + 1, size=SW_SETS).astype(np.int64)
        if rep % 5 == 1:
            c *= rng.randint(0, 2, size=SW_SETS)
        if rep % 3 == 2:
            c[list(groups[sorted(groups)[rep % len(groups)]])] = 0
        while c.sum() > 255:
            c = c * 3 // 4
        if rep % 10 == 9 and c.sum() > 0:  # topped up to exactly 255
            j = int(np.flatnonzero(c)[0])
            c[j] = min(64, c[j] + 255 - c.sum())
            k = 0
            while c.sum() < 255:
                c[k] = min(64, c[k] + 255 - c.sum())
                k += 1
        cases.append(sets_of_counts(rng, c))
    return np.array(cases, dtype=np.uint64)


@pytest.fixture(scope="module")
def cases():
    c = np.ascontiguousarray(prefix_cases())
    counts = np.array([[bin(int(x)).count("1") for x in row] for row in c], dtype=np.int64)
    return c, counts


def test_cases_hold_the_adversarial_inputs(cases):
    _, counts = cases
    totals = counts.sum(axis=1)
    assert totals.min() == 0 and totals.max() == 255 and (totals == 255).sum() >= 28 + 40
    assert (counts == 64).any(axis=1).sum() >= 28 and (counts == 0).all(axis=1).any()
    words = np.stack([counts[:, 8 * w:8 * w + 8].sum(axis=1) for w in range(4)], axis=1)
    for w in range(4):  # a word empty; all of a busy word in one byte
        assert (words[:, w] == 0).any()
        assert ((counts[:, 8 * w:8 * w + 8].max(axis=1) == words[:, w]) & (words[:, w] >= 40)).any()
    for sets in MAKERS.values():  # every maker with nothing, and with everything
        assert (counts[:, sets].sum(axis=1) == 0).any()
        assert ((counts[:, sets].sum(axis=1) == totals) & (totals > 0)).any()


def test_makers_words_are_byte_prefix_of_sw_pack(cases):
    c, _ = cases
    first = np.zeros(2, dtype=np.int64)
    bad = CP.lib().cp_words(c.ctypes.data, len(c), first.ctypes.data)
    assert bad == 0, (bad, int(first[0]), [hex(int(x)) for x in c[first[0]]])


def test_locate_pre_returns_the_set_and_rank_for_every_rank(cases):
    c, counts = cases
    ranks = np.zeros(1, dtype=np.int64)
    first = np.zeros(2, dtype=np.int64)
    bad = CP.lib().cp_locate(c.ctypes.data, len(c), ranks.ctypes.data, first.ctypes.data)
    assert bad == 0, (bad, counts[first[0]].tolist(), int(first[1]))
    assert ranks[0] == counts.sum()


def test_pick_equals_sw_select_on_the_shared_positions():
    L = CP.lib()
    ranks = np.zeros(1, dtype=np.int64)
    moves = castles = sliders = 0
    for side in (1, 0):
        boards, metas = PC.positions(side)
        assert len(boards) == 206
        for i in range(len(boards)):
            b = np.ascontiguousarray(boards[i], dtype=np.int8)
            m = np.ascontiguousarray(metas[i], dtype=np.uint8)
            acts = np.full(256, 0xFFFF, dtype=np.uint16)
            first = np.zeros(2, dtype=np.int64)
            n = L.cp_pick_board(b.ctypes.data, m.ctypes.data, acts.ctypes.data, ranks.ctypes.data, first.ctypes.data)
            assert n >= 0 and first[1] == 0, (side, i, n, first.tolist())
            got = [int(a) for a in acts[:n]]
            assert sorted(got) == sorted(H.get_list(b, m, side)), (side, i)
            moves += n
            castles += sum(a >= 4096 for a in got)
            sliders += sum(abs(int(b[a >> 6])) in (2, 3, 4) for a in got if a < 4096)
    assert ranks[0] == moves and moves > 5000 and castles > 0 and sliders > 1000, (moves, castles, sliders)


def test_pick_on_synthetic_sets_below_and_above_the_byte_sums():
    """totals below 256 take the located set, 256 and more the scan (never in play)"""
    L = CP.lib()
    rng = np.random.RandomState(0xB16)
    ranks = np.zeros(1, dtype=np.int64)
    want_ranks = big = 0
    for rep in range(60):
        if rep < 30:  # 256 and more: exactly 256, a little over, far over
            total = (256, 257, 300, 511, 1000, 28 * 64)[rep % 6]
            c = np.zeros(SW_SETS, dtype=np.int64)
            while c.sum() < total:
                j = rng.randint(SW_SETS)
                c[j] = min(64, c[j] + min(rng.randint(1, 65), total - c.sum()))
        else:
            c = rng.randint(0, 10, size=SW_SETS).astype(np.int64)
        # every target of a slider set gets an occupied square somewhere: the occupancy is random
        sets = np.array(sets_of_counts(rng, c), dtype=np.uint64)
        occ = rand_set(rng, 20 + rep % 30)
        castles = rep % 4
        tot = int(c.sum()) + bin(castles).count("1")
        if rep < 30 and castles == 0:
            assert tot >= 256
        big += tot >= 256
        first = np.zeros(2, dtype=np.int64)
        bad = L.cp_pick_sets(sets.ctypes.data, occ, rep & 1, castles, ranks.ctypes.data, first.ctypes.data)
        assert bad == 0, (rep, c.tolist(), int(first[0]))
        want_ranks += tot
    assert ranks[0] == want_ranks and big >= 30


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_sanitized_standalone_run(tmp_path):
    """the same shim under AddressSanitizer and UBSan, as a program of its own"""
    exe = str(tmp_path / "count_prefix_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                    os.path.join(ROOT, "tests", "core_host", "count_prefix_sanitize_main.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "fails 0" in r.stdout
