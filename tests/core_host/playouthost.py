"""TEST INFRASTRUCTURE ONLY -- ctypes view of playout_host.cpp (gc_playout.h's playout body on the
host, the private window a plain array), built by _hostlib.py."""
import ctypes

import numpy as np

try:
    from . import _hostlib  # imported as core_host.playouthost
except ImportError:
    import _hostlib  # imported from this directory

_L = None
P = ctypes.c_void_p
KINDS = ("win", "loss", "other", "cut")


def ensure_built():
    """(re)build libplayouthost.so unless its stamp holds the current source hash; -> its path"""
    return _hostlib.ensure_built("playout_host.cpp", "libplayouthost.so")


def lib():
    global _L
    if _L is None:
        L = ctypes.CDLL(ensure_built())
        L.ph_row.argtypes = [P, P, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32,
                             ctypes.c_int, ctypes.c_float, P, P, P, P, P]
        L.ph_material.argtypes = [P, ctypes.c_int]
        L.ph_value.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int]
        L.ph_value.restype = ctypes.c_float
        _L = L
    return _L


def _p(a):
    return a.ctypes.data_as(P)


def row(board, meta, seed, lane0, playouts, n_plies, draw=0, cut_weight=1.0, done=False):
    """one row of gc_playout_run on the host -> dict(actions i32[P][n_plies] (-1 past the end),
    reasons u8[P][n_plies], ends i32[P][3] = kind / plies / m, tally i32[6], value f32, skipped)"""
    b = np.ascontiguousarray(board, dtype=np.int8).reshape(64)
    m = np.ascontiguousarray(meta, dtype=np.uint8).reshape(8)
    act = np.zeros((playouts, n_plies), dtype=np.int32)
    why = np.zeros((playouts, n_plies), dtype=np.uint8)
    ends = np.zeros((playouts, 3), dtype=np.int32)
    tally = np.zeros(6, dtype=np.int32)
    value = np.zeros(1, dtype=np.float32)
    skipped = lib().ph_row(_p(b), _p(m), int(bool(done)), int(seed), int(lane0), int(playouts), int(draw) & 0xFFFFFFFF,
                           int(n_plies), float(cut_weight), _p(act), _p(why), _p(ends), _p(tally), _p(value))
    return dict(actions=act, reasons=why, ends=ends, tally=tally, value=value[0], skipped=bool(skipped))


def run(boards, metas, idx, seed, playouts, n_plies, draw=0, cut_weight=1.0, done=None):
    """gc_playout_run on the host: row j = board idx[j] of (boards, metas) on lanes j * P ...; an
    index outside [0, len(boards)) or a done board gives zeros -> (value f32[rows], tally i32[rows][6])"""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    value = np.zeros(len(idx), dtype=np.float32)
    tally = np.zeros((len(idx), 6), dtype=np.int32)
    for j, b in enumerate(idx):
        if not 0 <= b < len(boards):
            continue
        r = row(boards[b], metas[b], seed, j * playouts, playouts, n_plies, draw, cut_weight,
                done=bool(done[b]) if done is not None else False)
        value[j], tally[j] = r["value"], r["tally"]
    return value, tally


def material(board, own_white):
    b = np.ascontiguousarray(board, dtype=np.int8).reshape(64)
    return int(lib().ph_material(_p(b), int(bool(own_white))))


def value(wins, losses, msum, cut_weight, playouts):
    return np.float32(lib().ph_value(int(wins), int(losses), int(msum), float(cut_weight), int(playouts)))
