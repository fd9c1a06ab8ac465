"""TEST INFRASTRUCTURE ONLY -- the positions tests/test_playout.py and tests/test_playout_gpu.py
share: hand-made endings first, then seeded fuzz boards, each with the flags the env would hold
(rights forced, check flags from the board)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
import corehost as CH  # noqa: E402
from conftest import random_positions  # noqa: E402

START = np.array([-3, -5, -4, -2, -1, -4, -5, -3] + [-6] * 8 + [0] * 32 + [6] * 8 + [3, 5, 4, 2, 1, 4, 5, 3], dtype=np.int8)


def board_of(pieces):
    """{square: piece id} -> int8[64]; square = row * 8 + col, row 0 = rank 8"""
    b = np.zeros(64, dtype=np.int8)
    for sq, v in pieces.items():
        b[sq] = v
    return b


# WHITE: Kh1, pawns g2 h2 b2, Re7, Bh8; BLACK: Ka1, pawn a2, Re1 (check).  WHITE's one legal move
# is Rxe1 (action 12 * 64 + 60), which mates: b1 is the rook's, b2 the bishop's.
MATE_IN_ONE = board_of({63: 1, 54: 6, 55: 6, 12: 3, 7: 4, 49: 6, 60: -3, 56: -1, 48: -6})
MATE_IN_ONE_ACTION = 12 * 64 + 60
TWO_KINGS = board_of({60: 1, 4: -1})
HAND = [
    START,
    board_of({60: 1, 59: 2, 51: 2, 4: -1}),   # K + Q + Q v K
    TWO_KINGS,                                # K v K
    board_of({42: 1, 49: 3, 56: -1}),         # K + R v K in the corner (Kc3, Rb2, ka1)
    MATE_IN_ONE,
    board_of({63: 1, 5: -1, 13: 6, 21: 1}),   # two white kings, a pawn on the seventh
]
N_RANDOM = 200
SEED = 20260


def settle(board, meta):
    """the flags the env holds for this board: rights forced, check flags from the board"""
    m = CH.update_state(board, meta)[1].copy()
    m[7] = 0
    return m


def positions(side=None):
    """(boards int8[n][64], metas uint8[n][8]): HAND (WHITE to move, all rights) then N_RANDOM fuzz
    boards (their own side and rights); side=1 / 0 forces the side to move of every board"""
    rb, rm = random_positions(N_RANDOM, SEED, weird=True)
    boards = np.concatenate([np.stack(HAND), rb])
    metas = np.zeros((len(boards), 8), dtype=np.uint8)
    metas[: len(HAND), :5] = 1
    metas[len(HAND):] = rm
    if side is not None:
        metas[:, 0] = side
    for i in range(len(boards)):
        metas[i] = settle(boards[i], metas[i])
    return boards, metas
