"""TEST INFRASTRUCTURE ONLY -- ctypes view of apply_split_host.cpp (the two halves of the
branch-free apply of gc_core.h against apply_legal), built as corehost.py builds its library."""
import ctypes
import hashlib
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "apply_split_host.cpp")
_SO = os.path.join(_HERE, "_build", "libapplysplithost.so")
_STAMP = _SO + ".srchash"
_CSRC = os.path.join(_HERE, "..", "..", "gym-chess_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas"]
_L = None
P = ctypes.c_void_p
CASES = ("castle_ksw", "castle_qsw", "castle_ksb", "castle_qsb", "capture_queen", "capture_rook", "capture_bishop",
         "capture_knight", "capture_pawn", "white_king_move", "white_rook_leaves_a", "white_rook_leaves_h", "pawn_move",
         "moves")


def source_hash():
    h = hashlib.sha256(" ".join(FLAGS).encode())
    for path in [_SRC] + sorted(os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h")):
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def ensure_built():
    """(re)build libapplysplithost.so unless its stamp holds the current source hash"""
    want = source_hash()
    if os.path.exists(_SO) and os.path.exists(_STAMP) and open(_STAMP).read().strip() == want:
        return
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    tmp = f"{_SO}.{os.getpid()}.tmp"  # build aside, then rename (parallel test workers)
    subprocess.run(["g++"] + FLAGS + ["-o", tmp, _SRC], check=True)
    os.replace(tmp, _SO)
    with open(f"{_STAMP}.{os.getpid()}.tmp", "w") as f:
        f.write(want)
    os.replace(f"{_STAMP}.{os.getpid()}.tmp", _STAMP)


def lib():
    global _L
    if _L is None:
        ensure_built()
        L = ctypes.CDLL(_SO)
        L.as_compare.argtypes = [P, P, P, ctypes.c_int, P, P]
        _L = L
    return _L
