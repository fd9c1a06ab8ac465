"""CPU: the numpy restatement of the device plane encoder (gc_env_encode_planes) and of the
relative sampler's action mirror that tests/test_planes_gpu.py compares the kernels with -- and
proof that neither is vacuous.

Planes (include/gymchess.h): 0-5 / 6-11 the first / second side's K Q R B N P, 12 WHITE to move,
13-16 castle rights (first side's king-side, queen-side, then the second side's), 17 / 18 the
first / second side's king in check, 19 move_count / 256, 20 / 21 the current board's count in
its 3-fold window >= 1 / >= 2, 22 the FIDE en-passant target square, 23 ones.  "First" is WHITE,
or in the side-to-move view the side to move, with every square mirrored (sq ^ 56) on boards
where BLACK is to move.
"""
import os
import re

import numpy as np

from conftest import random_positions
from test_policy_sample import quantise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = 24
DTYPES = ("float32", "float16", "bfloat16")
LAYOUTS = ("nchw", "nhwc")


# ----------------------------------------------------------------------------- the restatement
def ref_planes(boards, meta8, rep_count, ep_file, perspective, layout):
    """float32 [N,24,8,8] ("nchw") or [N,8,8,24] ("nhwc") from the host API's arrays: boards
    int8[N,64], meta8 uint8[N,8] (gc_env_get_states), rep_count[N] (the current board's count in
    its 3-fold window), ep_file int8[N] (-1 none; gc_env_get_en_passant)."""
    boards = np.asarray(boards, dtype=np.int8).reshape(-1, 64)
    meta8 = np.asarray(meta8, dtype=np.uint8).reshape(-1, 8)
    n = boards.shape[0]
    out = np.zeros((n, PLANES, 64), dtype=np.float32)
    for i in range(n):
        b, m = boards[i].astype(np.int64), meta8[i]
        white = bool(m[0])
        flip = bool(perspective) and not white
        sign = -1 if flip else 1
        for k in range(6):
            out[i, k] = b * sign == k + 1
            out[i, 6 + k] = b * sign == -(k + 1)
        out[i, 12] = white
        rights = [m[3], m[4], m[1], m[2]] if flip else [m[1], m[2], m[3], m[4]]
        for k in range(4):
            out[i, 13 + k] = bool(rights[k])
        out[i, 17] = bool(m[6] if flip else m[5])
        out[i, 18] = bool(m[5] if flip else m[6])
        out[i, 19] = np.float32(int(m[7]) / 256.0)
        out[i, 20] = int(rep_count[i]) >= 1
        out[i, 21] = int(rep_count[i]) >= 2
        if int(ep_file[i]) >= 0:
            out[i, 22, (16 if white else 40) + int(ep_file[i])] = 1.0
        out[i, 23] = 1.0
        if flip:
            out[i] = out[i].reshape(PLANES, 8, 8)[:, ::-1, :].reshape(PLANES, 64)
    out = out.reshape(n, PLANES, 8, 8)
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1)) if layout == "nhwc" else out


def encode_raw(x, dtype):
    """float32 values -> the raw elements as they sit in device memory"""
    return quantise(x, dtype)[0]


def mirror_action(a):
    """where a side-to-move-relative policy head holds the logit of absolute action a on a board
    with BLACK to move: from and to each ^ 56, the castles' colours swapped"""
    a = np.asarray(a)
    return np.where(a < 4096, a ^ 0xE38, 4096 + ((a - 4096) ^ 2))


def colour_flip(board, meta):
    """the same position with the colours exchanged: pieces negated, rows flipped, side to move
    and castle rights swapped"""
    b = (-np.asarray(board, dtype=np.int8).reshape(8, 8)[::-1]).reshape(64).copy()
    m = np.asarray(meta, dtype=np.uint8).copy()
    m[0] = 1 - m[0]
    m[1], m[2], m[3], m[4] = meta[3], meta[4], meta[1], meta[2]
    m[5], m[6] = meta[6], meta[5]
    return b, m


# ----------------------------------------------------------------------------- mirror_action
def test_mirror_action_is_an_involution():
    a = np.arange(4100)
    m = mirror_action(a)
    assert sorted(m.tolist()) == a.tolist()
    assert (mirror_action(m) == a).all()
    assert mirror_action(52 * 64 + 36) == 12 * 64 + 28  # e2e4 <-> e7e5
    assert mirror_action(np.array([4096, 4097, 4098, 4099])).tolist() == [4098, 4099, 4096, 4097]
    frm, to = a[:4096] >> 6, a[:4096] & 63
    assert (m[:4096] == ((frm ^ 56) << 6 | (to ^ 56))).all()


def test_mirror_action_is_the_engines_colour_symmetry(oracle):
    """Pinned to the engine: on random_positions(300, seed, weird=False) the legal action set of
    the colour-flipped position equals mirror_action of the original's, wherever the reference's
    rules are colour-symmetric.  They are not everywhere (castling looks at
    fixed squares and piece ids, pawns promote and double-step by absolute row); the boards where
    the sets differ are counted and printed, and agreement is required on at least 90 % of the
    boards.  The oracle alone meets that cap on these inputs unrestricted (weird=False has no
    castling-geometry boards), so no further restriction is applied."""
    total = differ = moves = 0
    for seed in (1, 2, 3):
        boards, metas = random_positions(300, seed, weird=False)
        for b, m in zip(boards, metas):
            a = set(oracle.get_possible_moves(b, m, bool(m[0])))
            fb, fm = colour_flip(b, m)
            f = set(oracle.get_possible_moves(fb, fm, bool(fm[0])))
            want = set(int(x) for x in mirror_action(np.array(sorted(a), dtype=np.int64))) if a else set()
            total += 1
            moves += len(a)
            differ += f != want
    print(f"colour-flip legal sets differ on {differ} of {total} boards ({moves} legal actions in all)")
    assert moves > 10 * total
    assert total - differ >= 0.9 * total, (differ, total)
    # not vacuous: the identity map, or a column mirror, fails on nearly every board
    boards, metas = random_positions(100, 4, weird=False)
    wrong = 0
    for b, m in zip(boards, metas):
        a = sorted(oracle.get_possible_moves(b, m, bool(m[0])))
        fb, fm = colour_flip(b, m)
        f = set(oracle.get_possible_moves(fb, fm, bool(fm[0])))
        wrong += bool(a) and f == set(a)
    assert wrong <= 5, wrong


# ----------------------------------------------------------------------------- ref_planes
START = np.array([-3, -5, -4, -2, -1, -4, -5, -3] + [-6] * 8 + [0] * 32 + [6] * 8 + [3, 5, 4, 2, 1, 4, 5, 3],
                 dtype=np.int8)


def _start_expected(first_is_white_rows):
    """hand-written: the start position's planes with the first side on rows 6-7 (its pieces
    at the bottom, as WHITE's are), the second side on rows 0-1"""
    e = np.zeros((PLANES, 8, 8), dtype=np.float32)
    back = {0: [4], 1: [3], 2: [0, 7], 3: [2, 5], 4: [1, 6]}  # K Q R B N columns
    for k, cols in back.items():
        e[k, 7, cols] = 1
        e[6 + k, 0, cols] = 1
    e[5, 6, :] = 1
    e[11, 1, :] = 1
    e[13:17] = 1  # all four rights
    e[23] = 1
    return e


def test_start_position_by_hand():
    meta = np.array([[1, 1, 1, 1, 1, 0, 0, 0]], dtype=np.uint8)
    for persp in (False, True):
        got = ref_planes(START[None], meta, [0], [-1], persp, "nchw")[0]
        want = _start_expected(True)
        want[12] = 1
        assert (got == want).all(), persp
    # BLACK to move after 1.e4 ... (move_count 0, no en passant): absolute view
    b = START.copy()
    b[52], b[36] = 0, 6
    meta = np.array([[0, 1, 1, 1, 1, 0, 0, 0]], dtype=np.uint8)
    got = ref_planes(b[None], meta, [0], [-1], False, "nchw")[0]
    want = _start_expected(True)
    want[5, 6, 4], want[5, 4, 4] = 0, 1
    assert (got == want).all()
    # the side-to-move view: BLACK first, the board mirrored -- its own pieces at the bottom, and
    # WHITE's e4 pawn (row 4) appears on row 3 of the second side's pawn plane
    got = ref_planes(b[None], meta, [0], [-1], True, "nchw")[0]
    want = _start_expected(True)
    want[11, 1, 4], want[11, 3, 4] = 0, 1
    assert (got == want).all()
    # counts, flags, en passant, move_count, channels-last
    meta = np.array([[0, 1, 0, 0, 1, 0, 1, 37]], dtype=np.uint8)
    got = ref_planes(b[None], meta, [2], [4], False, "nchw")[0]
    assert (got[19] == np.float32(37 / 256)).all() and (got[20] == 1).all() and (got[21] == 1).all()
    assert got[22].sum() == 1 and got[22, 5, 4] == 1  # e3 = square 44, BLACK to move: 40 + file
    assert (got[13] == 1).all() and (got[14] == 0).all() and (got[15] == 0).all() and (got[16] == 1).all()
    assert (got[17] == 0).all() and (got[18] == 1).all()
    rel = ref_planes(b[None], meta, [1], [4], True, "nchw")[0]
    assert rel[22, 2, 4] == 1 and rel[22].sum() == 1 and (rel[20] == 1).all() and (rel[21] == 0).all()
    assert (rel[13] == 0).all() and (rel[14] == 1).all() and (rel[15] == 1).all() and (rel[16] == 0).all()
    assert (rel[17] == 1).all() and (rel[18] == 0).all()
    last = ref_planes(b[None], meta, [2], [4], False, "nhwc")
    assert last.shape == (1, 8, 8, PLANES) and (last[0].transpose(2, 0, 1) == got).all()


def test_perspective_symmetry():
    """the side-to-move planes of a position and of its colour flip are equal on every plane but
    12 (en passant and counts included)"""
    for seed in (5, 6):
        boards, metas = random_positions(200, seed, weird=True)
        rng = np.random.RandomState(seed)
        metas[:, 5:7] = rng.randint(2, size=(200, 2))
        metas[:, 7] = rng.randint(256, size=200)
        rep = rng.randint(3, size=200)
        ep = rng.randint(-1, 8, size=200).astype(np.int8)
        flipped = [colour_flip(b, m) for b, m in zip(boards, metas)]
        fb, fm = np.stack([f[0] for f in flipped]), np.stack([f[1] for f in flipped])
        for layout in LAYOUTS:
            a = ref_planes(boards, metas, rep, ep, True, layout)
            b = ref_planes(fb, fm, rep, ep, True, layout)
            keep = np.arange(PLANES) != 12
            if layout == "nchw":
                assert (a[:, keep] == b[:, keep]).all()
                assert (a[:, 12] != b[:, 12]).all()
            else:
                assert (a[..., keep] == b[..., keep]).all()
        # the absolute view is not symmetric: the restatement does look at the flag
        assert (ref_planes(boards, metas, rep, ep, False, "nchw")[:, :12] !=
                ref_planes(fb, fm, rep, ep, False, "nchw")[:, :12]).any()


def test_every_value_is_exact_in_all_three_types():
    x = (np.arange(256) / 256.0).astype(np.float32)
    for dtype in DTYPES:
        raw, val = quantise(np.concatenate([x, [1.0]]).astype(np.float32), dtype)
        assert (val[:256] == np.arange(256) / 256.0).all() and val[256] == 1.0, dtype
        assert (encode_raw(x, dtype) == raw[:256]).all()
    assert encode_raw(np.array([1.0], dtype=np.float32), "float16")[0] == 0x3C00
    assert encode_raw(np.array([1.0], dtype=np.float32), "bfloat16")[0] == 0x3F80


# ----------------------------------------------------------------------------- the boundary
def test_header_declares_and_binding_covers_encode_planes():
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    src = open(os.path.join(ROOT, "include", "gymchess.h")).read()
    assert re.search(r"#define\s+GC_PLANES\s+24\b", src)
    assert re.search(r"int\s+gc_env_encode_planes\s*\(\s*gc_env\s*\*\s*e\s*,\s*void\s*\*\s*d_planes\s*,\s*int\s+dtype\s*,"
                     r"\s*int64_t\s+board_stride\s*,\s*int\s+flags\s*\)", src)
    assert "gc_env_encode_planes" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gc_env_encode_planes"][1]) == 5
    assert hasattr(_lib.load(), "gc_env_encode_planes")
    assert BatchedChessEnv.PLANES == PLANES
    for name in ("planes_buffer", "encode_planes"):
        assert callable(getattr(BatchedChessEnv, name))
