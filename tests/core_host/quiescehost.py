"""TEST INFRASTRUCTURE ONLY -- ctypes view of quiesce_host.cpp (gc_minimax.h's first half on the
host with the quiescence nest below the leaves, with and without pruning), built by _hostlib.py."""
import ctypes

import numpy as np

try:
    from . import _hostlib  # imported as core_host.quiescehost
except ImportError:
    import _hostlib  # imported from this directory

_L = None
P = ctypes.c_void_p
MATE = 30000
NO_PICK = 0xFFFF
INT32_MIN = -2 ** 31


def ensure_built():
    """(re)build libquiescehost.so unless its stamp holds the current source hash; -> its path"""
    return _hostlib.ensure_built("quiesce_host.cpp", "libquiescehost.so")


def lib():
    global _L
    if _L is None:
        L = ctypes.CDLL(ensure_built())
        L.qh_row.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                             ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, P, P, P, P]
        L.qh_policy_index.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        L.qh_policy_index.restype = ctypes.c_uint32
        _L = L
    return _L


def _p(a):
    return a.ctypes.data_as(P) if a is not None else None


def max_quiesce():
    return int(lib().qh_max_quiesce())


def row(board, meta, depth, quiesce=0, seed=None, board_index=0, draw=0, prune=True, cap=0, done=False):
    """one row of gc_env_minimax_q on the host -> dict(count, pick, score, nodes, value f32, actions
    u16[cap], scores i32[cap], skipped); seed None = tiebreak first"""
    b = np.ascontiguousarray(board, dtype=np.int8).reshape(64)
    m = np.ascontiguousarray(meta, dtype=np.uint8).reshape(8)
    acts = np.zeros(cap, dtype=np.uint16) if cap else None
    scs = np.zeros(cap, dtype=np.int32) if cap else None
    out = np.zeros(4, dtype=np.int32)
    value = np.zeros(1, dtype=np.float32)
    rc = lib().qh_row(_p(b), _p(m), int(bool(done)), int(depth), int(quiesce), int(seed is not None), int(seed or 0),
                      int(board_index), int(draw) & 0xFFFFFFFF, int(bool(prune)), int(cap), _p(acts), _p(scs),
                      _p(out), _p(value))
    if rc < 0:
        raise ValueError(f"depth {depth} / quiesce {quiesce} out of range")
    return dict(count=int(out[0]), pick=int(out[1]), score=int(out[2]), nodes=int(out[3]) & 0xFFFFFFFF, value=value[0],
                actions=acts, scores=scs, skipped=bool(rc))


def run(boards, metas, idx, depth, quiesce=0, seed=None, draw=0, cap=0, done=None, prune=True):
    """gc_env_minimax_q on the host: row j = board idx[j] of (boards, metas); an index outside
    [0, len(boards)) gives count -1, a done board count 0, both with pick 0xFFFF and zeros ->
    dict(pick u16[rows], score i32, value f32, count i32, nodes u32, actions u16[rows][cap], scores i32[rows][cap])"""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    n = len(idx)
    res = dict(pick=np.full(n, NO_PICK, dtype=np.uint16), score=np.zeros(n, dtype=np.int32),
               value=np.zeros(n, dtype=np.float32), count=np.full(n, -1, dtype=np.int32),
               nodes=np.zeros(n, dtype=np.uint32), actions=np.full((n, cap), NO_PICK, dtype=np.uint16),
               scores=np.full((n, cap), INT32_MIN, dtype=np.int32))
    memo = {}  # a board listed twice is searched once
    for j, b in enumerate(idx):
        if not 0 <= b < len(boards):
            continue
        if b not in memo:
            memo[b] = row(boards[b], metas[b], depth, quiesce=quiesce, seed=seed, board_index=b, draw=draw, prune=prune,
                          cap=cap, done=bool(done[b]) if done is not None else False)
        r = memo[b]
        for k in ("pick", "score", "value", "count", "nodes"):
            res[k][j] = r[k]
        if cap:
            res["actions"][j], res["scores"][j] = r["actions"], r["scores"]
    return res


def policy_index(seed, board, draw, n):
    return int(lib().qh_policy_index(int(seed), int(board) & 0xFFFFFFFF, int(draw) & 0xFFFFFFFF, int(n)))
