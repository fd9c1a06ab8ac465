"""CPU: the indexed step and the indexed plane encoder exist at every layer of the boundary --
declared in include/gymchess.h, exported by the built library, bound in _lib.SIGNATURES with the
declared arity, wrapped by BatchedChessEnv."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gc_env_step_boards", "gc_env_encode_planes_rows")


def declared_args(name):
    """the argument list of `name`'s declaration in the header, comments stripped"""
    src = open(os.path.join(ROOT, "include", "gymchess.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_calls():
    assert declared_args("gc_env_step_boards") == [
        "gc_env* e", "const int32_t* d_board_idx", "const uint16_t* d_actions", "int rows", "int32_t* d_reward",
        "uint8_t* d_done", "uint8_t* d_reason", "int32_t* d_count", "uint64_t* d_mask", "int64_t mask_stride",
        "int8_t* d_obs", "int flags"]
    assert declared_args("gc_env_encode_planes_rows") == [
        "gc_env* e", "const int32_t* d_board_idx", "int rows", "void* d_planes", "int dtype", "int64_t row_stride",
        "int flags"]
    src = open(os.path.join(ROOT, "include", "gymchess.h")).read()
    assert re.search(r"#define\s+GC_REASON_BAD_INDEX\s+255\b", src)
    doc = src[: src.index("int gc_env_step_boards")][-4000:]
    assert "player_color BLACK" in doc and "distinct" in doc


def test_signatures_bind_the_calls_with_the_declared_arity():
    from gym_chess_amd import _lib

    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _lib.SIGNATURES["gc_env_step_boards"] == (I, [P, P, P, I, P, P, P, P, P, L, P, I])
    assert _lib.SIGNATURES["gc_env_encode_planes_rows"] == (I, [P, P, I, P, I, L, I])
    for name in NAMES:
        assert len(_lib.SIGNATURES[name][1]) == len(declared_args(name))


def test_library_exports_the_calls():
    from gym_chess_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (gc_\w+)", out))
    assert set(NAMES) <= exported
    lib = _lib.load()  # loads without a GPU
    # host-side argument checks need no device
    assert lib.gc_env_step_boards(None, None, None, 0, None, None, None, None, None, 0, None, 0) != 0
    assert b"null env" in lib.gc_last_error()
    assert lib.gc_env_encode_planes_rows(None, None, 0, None, 0, 0, 0) != 0
    assert b"null" in lib.gc_last_error()


def test_env_wraps_the_calls():
    from gym_chess_amd.env import BatchedChessEnv, RowsBuffer

    assert callable(BatchedChessEnv.step_boards) and callable(BatchedChessEnv.encode_planes_rows)
    assert callable(BatchedChessEnv.rows_buffer) and BatchedChessEnv.BAD_INDEX == 255
    assert set(RowsBuffer._SPEC) == {"reward", "done", "reason", "count", "obs"}
