"""The fused ply's apply in two halves (gc_core.h apply_legal_krw on Q0: kings, rooks, colours,
the meta word; apply_legal_qbnp on Q1: queens, bishops, knights, pawns, the captured value, the
irreversible flag), host-compiled: together they equal apply_legal on every legal move of the
weird random positions test_mover_check_shortcut_every_legal_move uses (several / no kings,
castling geometry), and neither half writes a member that is the other's.  The cases that take
the apply's separate paths are counted and must occur.

A black castle is never in a legal list: the reference tests the POSITIVE king and rook ids on
black's home squares too (lib.rs:966-1056, gen_castles), so the king that would castle is the
enemy's and attacks the squares the castle needs safe -- no seed can give one.  The apply still
has the path (lib.rs:740-773), so all four castle ids are applied to every position as well,
legal or not, and the halves must equal apply_legal there too; the legal lists give the white
castles.  Reference: lib.rs:679-784."""
import os
import sys

import numpy as np

from conftest import random_positions

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
import applysplithost as A  # noqa: E402
import corehost as H  # noqa: E402

SEEDS = (71, 72, 73)
CASTLES = np.array([4096, 4097, 4098, 4099], dtype=np.uint16)  # A_KSW, A_QSW, A_KSB, A_QSB
NEVER_LEGAL = ("castle_ksb", "castle_qsb")


def test_halves_equal_apply_legal_every_legal_move():
    L = A.lib()
    counts = np.zeros(len(A.CASES), dtype=np.int64)  # over the legal lists
    forced = np.zeros(len(A.CASES), dtype=np.int64)  # over the four castle ids applied to every position
    first = np.zeros(2, dtype=np.int64)
    for seed in SEEDS:
        boards, metas = random_positions(1500, seed)
        for b, m in zip(boards, metas):
            b = np.ascontiguousarray(b, dtype=np.int8)
            m = np.ascontiguousarray(m, dtype=np.uint8)
            legal = np.array(H.get_list(b, m, int(m[0])), dtype=np.uint16)
            for acts, cnt in ((legal, counts), (CASTLES, forced)):
                if len(acts) == 0:
                    continue
                bad = L.as_compare(b.ctypes.data, m.ctypes.data, acts.ctypes.data, len(acts), cnt.ctypes.data,
                                   first.ctypes.data)
                assert bad == 0, (seed, b.tolist(), m.tolist(), int(acts[first[0]]), bin(int(first[1])))
    seen = dict(zip(A.CASES, counts.tolist()))
    seen_forced = dict(zip(A.CASES, forced.tolist()))
    print("legal moves:", seen)
    print("castle ids on every position:", {k: v for k, v in seen_forced.items() if k.startswith("castle")})
    assert all(v > 0 for k, v in seen.items() if k not in NEVER_LEGAL), seen
    assert all(seen_forced[k] == 3 * 1500 for k in A.CASES if k.startswith("castle")), seen_forced
