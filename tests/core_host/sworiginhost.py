"""TEST INFRASTRUCTURE ONLY -- ctypes view of sw_origin_host.cpp (the pick's tail of gc_core.h:
sw_origin, the prefix form of sw_locate, the apply without the castle terms), built by
_hostlib.py."""
import ctypes

try:
    from . import _hostlib  # imported as core_host.sworiginhost
except ImportError:
    import _hostlib  # imported from this directory

_L = None
P = ctypes.c_void_p


def ensure_built():
    """(re)build libsworiginhost.so unless its stamp holds the current source hash; -> its path"""
    return _hostlib.ensure_built("sw_origin_host.cpp", "libsworiginhost.so")


def lib():
    global _L
    if _L is None:
        L = ctypes.CDLL(ensure_built())
        L.so_origin.argtypes = [P, P, P, P, ctypes.c_int, P]
        L.so_origin.restype = None
        L.so_locate.argtypes = [P, ctypes.c_int, P, P]
        L.so_apply_plain.argtypes = [P, P, P, ctypes.c_int, P]
        _L = L
    return _L
