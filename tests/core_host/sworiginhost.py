"""TEST INFRASTRUCTURE ONLY -- ctypes view of sw_origin_host.cpp (the pick's tail of gc_core.h:
sw_origin, the prefix form of sw_locate, the apply without the castle terms), built as
applysplithost.py builds its library."""
import ctypes
import hashlib
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "sw_origin_host.cpp")
_SO = os.path.join(_HERE, "_build", "libsworiginhost.so")
_STAMP = _SO + ".srchash"
_CSRC = os.path.join(_HERE, "..", "..", "gym-chess_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas"]
_L = None
P = ctypes.c_void_p


def source_hash():
    h = hashlib.sha256(" ".join(FLAGS).encode())
    for path in [_SRC] + sorted(os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h")):
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def ensure_built():
    """(re)build libsworiginhost.so unless its stamp holds the current source hash"""
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
        L.so_origin.argtypes = [P, P, P, P, ctypes.c_int, P]
        L.so_origin.restype = None
        L.so_locate.argtypes = [P, ctypes.c_int, P, P]
        L.so_apply_plain.argtypes = [P, P, P, ctypes.c_int, P]
        _L = L
    return _L
