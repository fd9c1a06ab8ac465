"""TEST INFRASTRUCTURE ONLY -- ctypes view of rank_fill_host.cpp (the carry-propagation rank
fills of gc_core.h against the Kogge-Stone templates), built by _hostlib.py."""
import ctypes

try:
    from . import _hostlib  # imported as core_host.rankfillhost
except ImportError:
    import _hostlib  # imported from this directory

_L = None
P = ctypes.c_void_p


def ensure_built():
    """(re)build librankfillhost.so unless its stamp holds the current source hash; -> its path"""
    return _hostlib.ensure_built("rank_fill_host.cpp", "librankfillhost.so")


def lib():
    global _L
    if _L is None:
        L = ctypes.CDLL(ensure_built())
        L.rf_compare.argtypes = [P, P, P, P, ctypes.c_int, P]
        L.rf_eval.argtypes = [ctypes.c_uint64, ctypes.c_uint64, P]
        L.rf_position.argtypes = [P, P, ctypes.c_int, P]
        _L = L
    return _L
