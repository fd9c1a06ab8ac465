"""TEST INFRASTRUCTURE ONLY -- ctypes view of count_prefix_host.cpp (the fused ply's count words
as running prefixes, sw_locate_pre and the pick from fetched sets of gc_core.h), built by
_hostlib.py."""
import ctypes

try:
    from . import _hostlib  # imported as core_host.countprefixhost
except ImportError:
    import _hostlib  # imported from this directory

_L = None
P = ctypes.c_void_p


def ensure_built():
    """(re)build libcountprefixhost.so unless its stamp holds the current source hash; -> its path"""
    return _hostlib.ensure_built("count_prefix_host.cpp", "libcountprefixhost.so")


def lib():
    global _L
    if _L is None:
        L = ctypes.CDLL(ensure_built())
        L.cp_words.argtypes = [P, ctypes.c_int, P]
        L.cp_locate.argtypes = [P, ctypes.c_int, P, P]
        L.cp_pick_board.argtypes = [P, P, P, P, P]
        L.cp_pick_sets.argtypes = [P, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, P, P]
        _L = L
    return _L
