"""TEST INFRASTRUCTURE ONLY -- ctypes view of apply_split_host.cpp (the two halves of the
branch-free apply of gc_core.h against apply_legal), built by _hostlib.py."""
import ctypes

try:
    from . import _hostlib  # imported as core_host.applysplithost
except ImportError:
    import _hostlib  # imported from this directory

_L = None
P = ctypes.c_void_p
CASES = ("castle_ksw", "castle_qsw", "castle_ksb", "castle_qsb", "capture_queen", "capture_rook", "capture_bishop",
         "capture_knight", "capture_pawn", "white_king_move", "white_rook_leaves_a", "white_rook_leaves_h", "pawn_move",
         "moves")


def ensure_built():
    """(re)build libapplysplithost.so unless its stamp holds the current source hash; -> its path"""
    return _hostlib.ensure_built("apply_split_host.cpp", "libapplysplithost.so")


def lib():
    global _L
    if _L is None:
        L = ctypes.CDLL(ensure_built())
        L.as_compare.argtypes = [P, P, P, ctypes.c_int, P, P]
        _L = L
    return _L
