"""The Python binding's device buffers (gym_chess_amd.buffers) against a fake library: what each
class allocates, that fetch() returns what the device holds, that everything is freed exactly
once and a borrowed address never, the staging buffer's growth and the index upload.  No GPU and
no libgymchess.so: "device" memory is host ctypes buffers, the copy a memmove."""
import ctypes
import gc

import numpy as np
import pytest

from gym_chess_amd import buffers as B
from gym_chess_amd.env import (DeviceIO, PlanesBuffer, PriorsBuffer, RowsBuffer, TraceBuffer, _DeviceArrays,
                               _GumbelPolicy)

N = 5  # boards of the fake env


class FakeLib:
    """gc_device_alloc / gc_device_free / gc_env_copy on host memory, with the books kept"""

    def __init__(self):
        self.live = {}  # address -> (ctypes buffer, bytes asked for)
        self.asked = []  # bytes of every allocation, in order
        self.freed = []
        self.copies = []  # (bytes, kind)

    def gc_device_alloc(self, device, nbytes, out):
        assert device == 3
        buf = ctypes.create_string_buffer(max(nbytes.value, 1))  # as the library: never a null address
        addr = ctypes.addressof(buf)
        self.live[addr] = (buf, nbytes.value)
        self.asked.append(nbytes.value)
        out._obj.value = addr
        return 0

    def gc_device_free(self, device, p):
        assert device == 3
        assert p.value in self.live, f"free of an unknown or already freed address {p.value:#x}"
        del self.live[p.value]
        self.freed.append(p.value)
        return 0

    def gc_env_copy(self, h, dst, src, nbytes, kind):
        assert h == "handle" and kind in (1, 2) and nbytes.value > 0
        dev = dst if kind == 1 else src
        base = max(a for a in self.live if a <= dev)  # inside one live allocation
        assert dev + nbytes.value <= base + max(self.live[base][1], 1), "copy past the end of the allocation"
        ctypes.memmove(dst, src, nbytes.value)
        self.copies.append((nbytes.value, kind))
        return 0


class FakeEnv:
    def __init__(self, n=N):
        self._L, self._h, self.device, self.num_boards, self.syncs = FakeLib(), "handle", 3, n, 0

    def synchronize(self):
        self.syncs += 1


@pytest.fixture
def env():
    e = FakeEnv()
    yield e
    gc.collect()
    assert not e._L.live, "device memory left allocated"


def poke(env, addr, a):
    """device memory at addr := the bytes of host array a"""
    a = np.ascontiguousarray(a)
    assert addr in env._L.live and a.nbytes <= max(env._L.live[addr][1], 1)
    ctypes.memmove(addr, a.ctypes.data, a.nbytes)


def pattern(dtype, shape, salt=0):
    n = int(np.prod(shape, dtype=np.int64))
    return ((np.arange(n, dtype=np.int64) * 37 + salt) % 251).astype(dtype).reshape(shape)


def nbytes(spec):
    return [int(np.prod(sh, dtype=np.int64)) * np.dtype(dt).itemsize for dt, sh in spec.values()]


def check_arrays(env, make, spec):
    """allocates exactly spec's bytes, round-trips a pattern per array, frees everything once by
    close() (twice) and by del"""
    L = env._L
    buf = make()
    assert L.asked == nbytes(spec) and list(buf.ptr) == list(spec)
    want = {}
    for j, (k, (dt, sh)) in enumerate(spec.items()):
        assert getattr(buf, k) == buf.ptr[k] and buf._shape(k) == (tuple(sh), nbytes(spec)[j])
        want[k] = pattern(dt, sh, j)
        poke(env, buf.ptr[k], want[k])
    got = buf.fetch()
    assert list(got) == list(spec)
    for k, (dt, sh) in spec.items():
        assert got[k].dtype == np.dtype(dt) and got[k].shape == tuple(sh) and (got[k] == want[k]).all(), k
    one = list(spec)[-1]
    assert list(buf.fetch(one)) == [one]
    owned = sorted(buf.ptr.values())
    buf.close()
    assert sorted(L.freed) == owned and not L.live and buf.ptr == {}
    buf.close()  # (the fake refuses a second free of an address)
    assert len(L.freed) == len(owned)
    buf = make()
    assert len(L.live) == len(spec)
    del buf
    gc.collect()
    assert not L.live and len(L.freed) == 2 * len(owned)
    with pytest.raises(AttributeError):
        make().no_such_array


def test_device_arrays(env):
    spec = {"parent": (np.int32, (7,)), "pi": (np.float32, (7, 3)), "pick": (np.uint16, (7,))}
    check_arrays(env, lambda: _DeviceArrays(env, spec), spec)
    gp = _GumbelPolicy(env, spec)
    assert gp.gumbel is True and not getattr(_DeviceArrays(env, spec), "gumbel", False)


@pytest.mark.parametrize("obs,count", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("rows", [0, 1, 9])
def test_rows_buffer(env, rows, obs, count):
    spec = {"reward": (np.int32, (rows,)), "done": (np.uint8, (rows,)), "reason": (np.uint8, (rows,))}
    if count:
        spec["count"] = (np.int32, (rows,))
    if obs:
        spec["obs"] = (np.int8, (rows, 64))
    check_arrays(env, lambda: RowsBuffer(env, rows, obs=obs, count=count), spec)
    assert RowsBuffer(env, rows).rows == rows
    with pytest.raises(ValueError, match="rows -1 < 0"):
        RowsBuffer(env, -1)


@pytest.mark.parametrize("logit_index", [False, True])
@pytest.mark.parametrize("rows,cap", [(0, 64), (1, 1), (6, 7)])
def test_priors_buffer(env, rows, cap, logit_index):
    spec = {"actions": (np.uint16, (rows, cap)), "priors": (np.float32, (rows, cap)), "count": (np.int32, (rows,))}
    if logit_index:
        spec["logit_index"] = (np.uint16, (rows, cap))
    check_arrays(env, lambda: PriorsBuffer(env, rows, cap=cap, logit_index=logit_index), spec)
    pb = PriorsBuffer(env, rows, cap=cap)
    assert (pb.rows, pb.cap) == (rows, cap)
    for bad in (0, 4101):
        with pytest.raises(ValueError, match=f"cap {bad}: between 1 and 4100"):
            PriorsBuffer(env, rows, cap=bad)
    with pytest.raises(ValueError, match="rows -2 < 0"):
        PriorsBuffer(env, -2)


def test_zero_row_buffers_copy_nothing(env):
    for buf in (RowsBuffer(env, 0), PriorsBuffer(env, 0, logit_index=True), PlanesBuffer(env, rows=0)):
        got = buf.fetch()
        if isinstance(got, dict):
            assert all(a.size == 0 for a in got.values())
        else:
            assert got.shape == (0, 24, 8, 8) and got.dtype == np.float32
        buf.close()
    assert env._L.copies == [] and set(env._L.asked) == {0}


OPTIONAL = ("mask", "obs", "count", "pick", "policy")


@pytest.mark.parametrize("off", [None] + list(OPTIONAL))
@pytest.mark.parametrize("stride", [N, N + 3])
def test_device_io(env, off, stride):
    on = {k: k != off for k in OPTIONAL}
    on["policy"] = off != "policy" and off is not None  # (off by default)
    spec = {"reward": (np.int32, (N,)), "done": (np.uint8, (N,)), "reason": (np.uint8, (N,))}
    for k, dt, sh in (("mask", np.uint64, (65, stride)), ("obs", np.int8, (N, 64)), ("count", np.int32, (N,)),
                      ("pick", np.uint16, (N,))):
        if on[k]:
            spec[k] = (dt, sh)
    if on["policy"]:
        spec.update(logprob=(np.float32, (N,)), entropy=(np.float32, (N,)))

    def make():
        return DeviceIO(env, mask=on["mask"], obs=on["obs"], count=on["count"], pick=on["pick"], select=False,
                        mask_stride=stride, policy=on["policy"])

    io = make()
    assert env._L.asked == nbytes(spec) and list(io.ptr) == list(spec) and io.mask_stride == stride
    want = {k: pattern(dt, sh, j) for j, (k, (dt, sh)) in enumerate(spec.items())}
    for k, a in want.items():
        poke(env, io.ptr[k], a)
    got = io.fetch()
    assert list(got) == list(spec)
    for k in spec:
        if k == "mask":  # word-major [65][stride] on the device, [N][65] on the host
            assert got[k].shape == (N, 65) and got[k].flags.c_contiguous
            assert all(got[k][i, f] == want[k][f, i] for i in range(N) for f in range(65))
        else:
            assert got[k].dtype == want[k].dtype and (got[k] == want[k]).all(), k
    if on["mask"]:
        assert io.fetch("mask")["mask"].shape == (N, 65)
    if on["pick"]:
        io.upload_actions([4099, 0, 7, 65, 1])
        assert io.fetch("pick")["pick"].tolist() == [4099, 0, 7, 65, 1]
    owned = sorted(io.ptr.values())
    io.close()
    io.close()
    assert sorted(env._L.freed) == owned
    io = make()
    del io
    gc.collect()
    assert not env._L.live


def test_device_io_mask_stride(env, monkeypatch):
    with pytest.raises(ValueError, match=f"mask_stride {N - 1} < num_boards {N}"):
        DeviceIO(env, select=False, mask_stride=N - 1)
    monkeypatch.delenv("GC_MASK_PAD", raising=False)
    assert DeviceIO.default_mask_stride(4095) == 4095 and DeviceIO.default_mask_stride(4097) == 4608 + 512
    assert DeviceIO(env, select=False).mask_stride == N


def bits(dtype, values):
    """float32 values -> the raw elements a planes buffer of `dtype` holds"""
    v = np.asarray(values, dtype=np.float32)
    if dtype == "float32":
        return v
    if dtype == "float16":
        return v.astype(np.float16).view(np.uint16)
    return (v.view(np.uint32) >> np.uint32(16)).astype(np.uint16)  # bfloat16: exact for the values below


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("rows,stride", [(None, None), (3, 1544), (0, None)])
def test_planes_buffer(env, dtype, layout, rows, stride):
    L, size = env._L, 4 if dtype == "float32" else 2
    r, s = N if rows is None else rows, 1536 if stride is None else stride
    buf = PlanesBuffer(env, dtype=dtype, layout=layout, board_stride=stride, rows=rows)
    assert L.asked == [r * s * size] and buf.nbytes == r * s * size and isinstance(buf.ptr, int)
    assert (buf.rows, buf.board_stride, buf.dtype, buf.layout) == (r, s, dtype, layout)
    vals = (np.arange(r * s) % 7 - 3).astype(np.float32).reshape(r, s) * 0.25  # exact in all three formats
    poke(env, buf.ptr, bits(dtype, vals))
    raw = buf.raw()
    assert raw.shape == (r, s) and raw.dtype == (np.float32 if dtype == "float32" else np.uint16)
    assert (raw == bits(dtype, vals)).all()
    got = buf.fetch()
    shape = (24, 8, 8) if layout == "nchw" else (8, 8, 24)
    assert got.dtype == np.float32 and got.shape == (r,) + shape
    assert (got == vals[:, :1536].reshape((r,) + shape)).all()  # (the padding past 24 * 64 is left out)
    addr = buf.ptr
    buf.close()
    buf.close()
    assert L.freed == [addr] and buf.ptr is None
    buf = PlanesBuffer(env, dtype=dtype, layout=layout, rows=rows)
    del buf
    gc.collect()
    assert not L.live and len(L.freed) == 2


def test_planes_buffer_arguments(env):
    for kw, msg in ((dict(dtype="float64"), "dtype must be one of"), (dict(layout="chwn"), "layout must be one of"),
                    (dict(board_stride=1528), "board_stride 1528: at least 1536, a multiple of 8"),
                    (dict(board_stride=1540), "board_stride 1540"), (dict(rows=-1), "rows -1 < 0")):
        with pytest.raises(ValueError, match=msg):
            PlanesBuffer(env, **kw)
    assert env._L.asked == []


@pytest.mark.parametrize("plies", [0, 1, 4])
def test_trace_buffer(env, plies):
    L = env._L
    tb = TraceBuffer(env, plies)
    assert L.asked == [8 * plies * N] and tb.plies == plies and isinstance(tb.ptr, int)
    act = pattern(np.int64, (plies, N), 1) - 1  # -1 = the driver's no-move reset
    rew = pattern(np.int64, (plies, N), 2) % 3 - 1
    done, why = pattern(np.int64, (plies, N), 3) % 2, pattern(np.int64, (plies, N), 4) % 11
    words = ((act & 0xFFFF) | ((rew & 0xFFFF) << 16) | (done << 32) | (why << 40)).astype(np.uint64)
    poke(env, tb.ptr, words)
    assert (tb.raw() == words).all() and tb.raw().shape == (plies, N) and tb.raw().dtype == np.uint64
    got = tb.fetch()
    assert (got["action"] == act).all() and (got["reward"] == rew).all()
    assert (got["done"] == done).all() and (got["reason"] == why).all()
    assert got["action"].dtype == np.int16 and got["done"].dtype == np.uint8
    if plies > 1:
        assert (tb.raw(1) == words[:1]).all() and tb.fetch(2)["action"].shape == (2, N)
    addr = tb.ptr
    tb.close()
    tb.close()
    assert L.freed == [addr] and tb.ptr is None
    tb = TraceBuffer(env, plies)
    del tb
    gc.collect()
    assert not L.live and len(L.freed) == 2


def test_a_borrowed_address_is_never_freed(env):
    L = env._L
    theirs = PlanesBuffer(env, dtype="float32", rows=2)  # a caller's memory
    vals = pattern(np.float32, (2, 1536), 5)
    poke(env, theirs.ptr, vals)
    arr = _DeviceArrays(env, {"z": (np.float32, (2,))})
    mine = arr.ptr["z"]
    arr.adopt("planes", theirs.ptr, np.float32, (2, 1536))
    assert arr.planes == theirs.ptr and list(arr.ptr) == ["z", "planes"]
    assert (arr.fetch()["planes"] == vals).all() and (arr.fetch("planes")["planes"] == vals).all()
    arr.adopt("planes", theirs.ptr, np.float32, (1, 1536))  # again, as sample() does on every call
    assert arr.fetch("planes")["planes"].shape == (1, 1536)
    arr.close()
    assert L.freed == [mine] and theirs.ptr in L.live
    arr = _DeviceArrays(env, {})
    arr.adopt("planes", theirs.ptr, np.float32, (2, 1536))
    del arr
    gc.collect()
    assert L.freed == [mine] and (theirs.raw() == vals).all()
    theirs.close()


def test_c_pointers():
    calls = []

    def fn(handle, addr, n):
        calls.append((handle, n))
        for i in range(n):
            addr[i] = 0x1000 * (i + 1)
        return 0

    assert B.c_pointers(fn, "tree", ("action", "prior", "child")) == {"action": 0x1000, "prior": 0x2000,
                                                                       "child": 0x3000}
    assert calls == [("tree", 3)]


def test_staging_growth(env):
    L = env._L
    st = B._Staging(env, 6)
    assert (st.cap, st.ptr, L.asked) == (0, None, [])
    seen = []
    for m, cap in ((1, 256), (256, 256), (257, 512), (3, 512)):
        p = st.reserve(m)
        assert p == st.ptr and st.cap == cap and L.live[p][1] == 6 * cap
        seen.append((p, len(L.freed), env.syncs))
    assert L.asked == [6 * 256, 6 * 512]
    assert seen[0][0] == seen[1][0] and seen[2][0] == seen[3][0]
    assert [s[1:] for s in seen] == [(0, 0), (0, 0), (1, 1), (1, 1)]  # one free and one synchronize, at the growth
    assert L.freed == [seen[0][0]]
    st.close()
    assert (st.cap, st.ptr) == (0, None) and (len(L.freed), env.syncs) == (2, 2) and not L.live
    st.close()
    assert (len(L.freed), env.syncs) == (2, 2)
    assert st.reserve(1000) and st.cap == 1024
    del st
    gc.collect()
    assert not L.live and (len(L.freed), env.syncs) == (3, 3)


def test_upload_indices(env):
    L = env._L
    st = B._Staging(env, 4)
    assert B.upload_indices(st, []) == (None, 0) and B.upload_indices(st, [], rows=0) == (None, 0)
    assert L.asked == [] and L.copies == []  # nothing allocated, nothing uploaded
    p, m = B.upload_indices(st, [-5, 0, 7, 2 ** 40])
    assert (p, m) == (st.ptr, 4) and L.copies == [(16, 1)]
    got = np.frombuffer(ctypes.string_at(p, 16), dtype=np.int32)
    assert got.tolist() == [-1, 0, 7, 2 ** 31 - 1]
    assert [0 <= x < 8 for x in got.tolist()] == [False, True, True, False]  # out of range (of 8) where they were
    p, m = B.upload_indices(st, np.array([[-2 ** 40, 3], [2 ** 31, 65535]], dtype=np.int64), rows=4)  # (flattened)
    assert np.frombuffer(ctypes.string_at(p, 16), dtype=np.int32).tolist() == [-1, 3, 2 ** 31 - 1, 65535]
    p, m = B.upload_indices(st, np.array([4, 65535], dtype=np.uint16))
    assert np.frombuffer(ctypes.string_at(p, 8), dtype=np.int32).tolist() == [4, 65535]
    del L.copies[1:]
    with pytest.raises(ValueError, match=r"rows 3 != the board array's length 4"):
        B.upload_indices(st, [1, 2, 3, 4], rows=3)
    with pytest.raises(ValueError, match=r"4 slots for 6 rows"):
        B.upload_indices(st, [1, 2, 3, 4], 6, "{size} slots for {rows} rows")
    assert L.copies == [(16, 1)]
    # the second part of a two-part buffer sits one capacity of int32 further, and moves with it
    st2 = B._Staging(env, 8)
    p0, _ = B.upload_indices(st2, [1, 2])
    p1, _ = B.upload_indices(st2, [3, 4], part=1)
    assert p1 == p0 + 4 * 256 and st2.cap == 256
    p0, _ = B.upload_indices(st2, list(range(300)), rows=300)
    p1, m = B.upload_indices(st2, list(range(300, 600)), part=1)
    assert (p1, m, st2.cap) == (p0 + 4 * 512, 300, 512) and L.live[p0][1] == 8 * 512
    assert np.frombuffer(ctypes.string_at(p1, 1200), dtype=np.int32).tolist() == list(range(300, 600))
    st.close()
    st2.close()


def test_planes_format(env):
    buf = PlanesBuffer(env, dtype="bfloat16", layout="nhwc", board_stride=1544, rows=2)
    assert B.planes_format(buf) == (buf, "bfloat16", "nhwc", 1544)
    assert B.planes_format(buf, "float32", "nchw", 1600) == (buf, "float32", "nchw", 1600)
    assert B.planes_format(0x7000) == (None, "float16", "nchw", 0)
    assert B.planes_format(None, default_stride=1536) == (None, "float16", "nchw", 1536)
    assert B.planes_format(0x7000, stride=1552, default_stride=1536)[3] == 1552
    with pytest.raises(ValueError, match=r"dtype must be one of \['bfloat16', 'float16', 'float32'\], got 'int8'"):
        B.planes_format(buf, dtype="int8")
    with pytest.raises(ValueError, match=r"layout must be one of \['nchw', 'nhwc'\], got 'hwc'"):
        B.planes_format(0x7000, layout="hwc")
    buf.close()


def test_record_names_what_it_needs(env):
    """SampleStore.record takes a root_policy() / gumbel_policy() result, not any device buffer"""
    from gym_chess_amd.env import SampleStore

    calls = []

    class L:
        @staticmethod
        def gc_replay_record(h, a, v, rc):
            calls.append((a, v, rc))
            return 0

    store = SampleStore.__new__(SampleStore)
    store._L, store._h = L, None
    root = _DeviceArrays(env, {"actions": (np.uint16, (2, 9)), "visits": (np.int32, (2, 9)), "pick": (np.uint16, (2,))})
    gp = _GumbelPolicy(env, {"actions": (np.uint16, (2, 9)), "visits": (np.int32, (2, 9)), "target": (np.int32, (2, 9))})
    store.record(root)
    store.record(gp)
    store.record((0x10, 0x20, 5))
    assert calls == [(root.actions, root.visits, 9), (gp.actions, gp.target, 9), (0x10, 0x20, 5)]
    for wrong in (PriorsBuffer(env, 2, cap=9), RowsBuffer(env, 2), DeviceIO(env, select=False)):
        with pytest.raises(TypeError, match=f"this {type(wrong).__name__} has no actions / visits"):
            store.record(wrong)
    assert len(calls) == 3
