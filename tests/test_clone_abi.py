"""CPU: the board-clone calls exist at every layer of the boundary -- declared in
include/gymchess.h, bound in _lib.SIGNATURES, exported by the built library, wrapped by
BatchedChessEnv."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gc_env_clone_boards", "gc_env_clone_errors")


def test_header_declares_the_clone_calls():
    src = open(os.path.join(ROOT, "include", "gymchess.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+gc_env_clone_boards\s*\(\s*gc_env\s*\*\s*dst\s*,\s*gc_env\s*\*\s*src\s*,\s*const\s+int32_t\s*\*"
                     r"\s*d_src_idx\s*,\s*const\s+int32_t\s*\*\s*d_dst_idx\s*,\s*int\s+m\s*\)\s*;", code)
    assert re.search(r"\bint\s+gc_env_clone_errors\s*\(\s*gc_env\s*\*\s*dst\s*,\s*uint64_t\s*\*\s*skipped\s*\)\s*;", code)
    # the spill-table exclusion and the stale "Reference rules only" sentence
    assert "player_color BLACK" in src[src.index("gc_env_clone_boards") - 4000: src.index("gc_env_clone_boards")]
    assert "Reference rules only" not in src


def test_signatures_bind_the_clone_calls():
    from gym_chess_amd import _lib

    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["gc_env_clone_boards"] == (I, [P, P, P, P, I])
    assert _lib.SIGNATURES["gc_env_clone_errors"] == (I, [P, P])


def test_library_exports_the_clone_calls():
    from gym_chess_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (gc_\w+)", out))
    assert set(NAMES) <= exported
    L = _lib.load()  # loads without a GPU
    # host-side argument checks need no device
    assert L.gc_env_clone_boards(None, None, None, None, 0) != 0 and b"null env" in L.gc_last_error()
    v = ctypes.c_uint64()
    assert L.gc_env_clone_errors(None, ctypes.byref(v)) != 0


def test_env_wraps_the_clone_calls():
    from gym_chess_amd.env import BatchedChessEnv

    assert callable(BatchedChessEnv.clone_boards) and callable(BatchedChessEnv.clone_errors)
