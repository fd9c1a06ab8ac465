"""TEST INFRASTRUCTURE ONLY -- ctypes view of clone_host.cpp (the window-clone rule of gc_env.h on
host tables), built by _hostlib.py."""
import ctypes

try:
    from . import _hostlib  # imported as core_host.clonehost
except ImportError:
    import _hostlib  # imported from this directory

_L = None
P = ctypes.c_void_p


def ensure_built():
    """(re)build libclonehost.so unless its stamp holds the current source hash; -> its path"""
    return _hostlib.ensure_built("clone_host.cpp", "libclonehost.so")


def lib():
    global _L
    if _L is None:
        L = ctypes.CDLL(ensure_built())
        L.ch_scenario.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                                  ctypes.c_uint32, P]
        L.ch_scenario.restype = ctypes.c_int
        _L = L
    return _L
