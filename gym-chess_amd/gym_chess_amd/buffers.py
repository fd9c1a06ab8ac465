"""Device memory of the Python binding: who allocates, copies and frees what.

    _DeviceArrays   named device arrays, owned (allocated here, freed by close() / __del__) or
                    adopted (someone else's address: fetched like the others, never freed)
    RowsBuffer, PriorsBuffer, PlayoutBuffer, MinimaxBuffer, DeviceIO, _GumbelPolicy
                    subclasses: their spec and what is their own
    PlanesBuffer, TraceBuffer   one owned array whose `ptr` is the address itself
    _Staging        the grow-by-doubling upload buffer; upload_indices fills it with a host index list

Allocation, host copies and frees go through device_alloc / fetch_arrays / device_free below and
nowhere else.  A free waits for the device (hipFree); an upload buffer that a launch on the env's
stream may still read is freed after env.synchronize().
"""
import ctypes
import os
import weakref

import numpy as np

from . import _lib
from . import codec as C

POLICY_DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2}
PLANES = 24
PLANES_LAYOUTS = {"nchw": 0, "nhwc": 2}


def device_alloc(L, device, nbytes):
    """gc_device_alloc: a device address (a zero-byte request still gets its own)"""
    v = ctypes.c_void_p()
    _lib.check(L.gc_device_alloc(device, ctypes.c_uint64(nbytes), ctypes.byref(v)))
    return v.value


def device_free(L, device, addr):
    L.gc_device_free(device, ctypes.c_void_p(addr))


def upload(env, addr, a):
    """host array -> device on the env's stream (a synchronous copy)"""
    _lib.check(env._L.gc_env_copy(env._h, addr, _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))


def fetch_arrays(env, ptr, keys, layout):
    """host copies of ptr[k] for k in keys (waits for the env's stream); layout(k) = (dtype, shape).
    An empty array is not copied."""
    out = {}
    for k in keys:
        dt, shape = layout(k)
        a = np.zeros(shape, dtype=dt)
        if a.nbytes:
            _lib.check(env._L.gc_env_copy(env._h, _lib.ptr(a), ptr[k], ctypes.c_uint64(a.nbytes), 2))
        out[k] = a
    return out


def c_pointers(fn, handle, names):
    """{name: device address} of a C-side object's arrays (gc_*_pointers, in the order of names)"""
    addr = (ctypes.c_void_p * len(names))()
    _lib.check(fn(handle, addr, len(names)))
    return {k: addr[i] for i, k in enumerate(names)}


class _DeviceArrays:
    """Named device arrays: ptr[name] (and the attribute `name`) device addresses, fetch() host
    copies.  spec: name -> (dtype, shape), each allocated here and freed by close(); adopt() adds
    an address this object does not own."""

    def __init__(self, env, spec):
        self.env, self._spec, self.ptr, self._owned = env, dict(spec), {}, []
        for k, (dt, shape) in spec.items():
            self.ptr[k] = device_alloc(env._L, env.device, self._shape(k)[1])
            self._owned.append(self.ptr[k])

    def adopt(self, k, addr, dtype, shape):
        """ptr[k] = addr, someone else's memory: fetched like the rest, not freed"""
        self.ptr[k], self._spec[k] = addr, (dtype, shape)

    def __getattr__(self, k):
        ptr = self.__dict__.get("ptr", {})
        if k in ptr:
            return ptr[k]
        raise AttributeError(k)

    def _shape(self, k):
        """(shape, bytes) of array k"""
        dt, shape = self._spec[k]
        return tuple(shape), int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize

    def fetch(self, *keys):
        """host copies (waits for the env's stream): dict of arrays"""
        return fetch_arrays(self.env, self.ptr, keys or self.ptr, self._spec.__getitem__)

    def close(self):
        owned = self.__dict__.get("_owned", [])
        while owned:
            device_free(self.env._L, self.env.device, owned.pop())
        self.ptr = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _GumbelPolicy(_DeviceArrays):
    """gumbel_policy()'s buffers: a root_policy()-like result whose training target is `target`
    (the improved policy in units of 2^-20) where root_policy's is `visits`"""

    @property
    def gumbel(self):
        return True


def _rows(rows):
    if int(rows) < 0:
        raise ValueError(f"rows {rows} < 0")
    return int(rows)


class RowsBuffer(_DeviceArrays):
    """Device memory of step_boards' row-compact outputs: reward int32[rows], done uint8[rows],
    reason uint8[rows] and optionally count int32[rows], obs int8[rows][64] (ptr[...] are device
    pointers; row j belongs to the j-th listed board of the call)."""

    _SPEC = {"reward": (np.int32, ()), "done": (np.uint8, ()), "reason": (np.uint8, ()), "count": (np.int32, ()),
             "obs": (np.int8, (64,))}

    def __init__(self, env, rows, obs=True, count=True):
        self.rows = _rows(rows)
        keys = ("reward", "done", "reason") + (("count",) if count else ()) + (("obs",) if obs else ())
        super().__init__(env, {k: (self._SPEC[k][0], (self.rows,) + self._SPEC[k][1]) for k in keys})


class PriorsBuffer(_DeviceArrays):
    """Device memory of policy_priors' output: actions uint16[rows][cap], priors float32[rows][cap],
    count int32[rows] and optionally logit_index uint16[rows][cap] (ptr[...] are device pointers)."""

    _SPEC = {"actions": np.uint16, "priors": np.float32, "count": np.int32, "logit_index": np.uint16}

    def __init__(self, env, rows, cap=64, logit_index=False):
        self.rows, self.cap = _rows(rows), int(cap)
        if not 1 <= self.cap <= C.N_ACTIONS - 1:
            raise ValueError(f"cap {cap}: between 1 and {C.N_ACTIONS - 1}")
        keys = ("actions", "priors", "count") + (("logit_index",) if logit_index else ())
        super().__init__(env, {k: (self._SPEC[k], (self.rows,) if k == "count" else (self.rows, self.cap))
                               for k in keys})


class PlayoutBuffer(_DeviceArrays):
    """Device memory of a playout run's outputs: value float32[rows] (the mean outcome from the
    view of the side to move at the board) and tally int32[rows][6] (wins, losses, other endings,
    cut-offs, the cut-offs' material sum, plies played); ptr[...] are device pointers."""

    TALLY = ("wins", "losses", "others", "cutoffs", "material", "plies")

    def __init__(self, env, rows):
        self.rows = _rows(rows)
        super().__init__(env, {"value": (np.float32, (self.rows,)), "tally": (np.int32, (self.rows, len(self.TALLY)))})


class MinimaxBuffer(_DeviceArrays):
    """Device memory of minimax's outputs: pick uint16[rows] (0xFFFF: no move), score int32[rows],
    value float32[rows] (from the view of the side to move at the board), count int32[rows], nodes
    uint32[rows] (written only by a call with nodes=True) and, with cap > 0, the root lists actions
    uint16[rows][cap] / scores int32[rows][cap] (padding 0xFFFF / INT32_MIN); ptr[...] are device
    pointers."""

    def __init__(self, env, rows, cap=0):
        self.rows, self.cap = _rows(rows), int(cap)
        if not 0 <= self.cap <= C.N_ACTIONS - 1:
            raise ValueError(f"cap {cap}: between 0 and {C.N_ACTIONS - 1}")
        spec = {k: (dt, (self.rows,)) for k, dt in (("pick", np.uint16), ("score", np.int32), ("value", np.float32),
                                                    ("count", np.int32), ("nodes", np.uint32))}
        if self.cap:
            spec.update(actions=(np.uint16, (self.rows, self.cap)), scores=(np.int32, (self.rows, self.cap)))
        super().__init__(env, spec)


class DeviceIO(_DeviceArrays):
    """Device buffers of one env's step_device outputs: reward i32, done u8, reason u8 and
    optionally mask u64[65][stride] (word-major: word f of board i at f * stride + i, stride >= N),
    obs i8[N][64], count i32, pick u16 (the random policy's next action, which step_device uses
    as the actions when given none), and with policy=True logprob f32 and entropy f32
    (sample_policy's outputs).  fetch() copies them to host arrays; upload_actions() fills
    the pick buffer from the host."""

    _SPEC = {"reward": (np.int32, ()), "done": (np.uint8, ()), "reason": (np.uint8, ()),
             "mask": (np.uint64, (65,)), "obs": (np.int8, (64,)), "count": (np.int32, ()), "pick": (np.uint16, ()),
             "logprob": (np.float32, ()), "entropy": (np.float32, ())}

    @staticmethod
    def default_mask_stride(n):
        """From N = 4096 on: N rounded up to a multiple of 512, plus GC_MASK_PAD words (default
        MASK_PAD).  Packed rows of N = 65 536 sit 512 KiB apart and fall on the same HBM
        channels; measured on the quad API step (same box): packed 17.0 us per launch, padded by
        8 words 16.4, by 64 16.2, by 256-4096 15.6-15.8 -- 512 (4 KiB) kept; N = 65 472 packed
        (511.5 KiB apart) 16.8 against 16.2 for 65 536 padded."""
        pad = int(os.environ.get("GC_MASK_PAD", DeviceIO.MASK_PAD))
        return (n + 511) // 512 * 512 + pad if n >= 4096 and pad else n

    MASK_PAD = 512

    def __init__(self, env, mask=True, obs=True, count=True, pick=True, select=True, mask_stride=None,
                 policy=False):
        n = env.num_boards
        self.mask_stride = int(self.default_mask_stride(n) if mask_stride is None else mask_stride)
        if self.mask_stride < n:
            raise ValueError(f"mask_stride {self.mask_stride} < num_boards {n}")
        want = {"reward": True, "done": True, "reason": True, "mask": mask, "obs": obs, "count": count, "pick": pick,
                "logprob": policy, "entropy": policy}
        super().__init__(env, {k: (self._SPEC[k][0], (65, self.mask_stride) if k == "mask" else (n,) + self._SPEC[k][1])
                               for k, on in want.items() if on})
        if pick and select:  # the policy's picks for the current states
            self.select()

    def select(self):
        """pick = the env's current random-policy actions (picked at creation, reset(),
        step_random(), rollout(); after set_states / set_fens call env.select_random() first)"""
        self.upload_actions(self.env.outputs()["next_action"])

    def upload_actions(self, actions):
        upload(self.env, self.ptr["pick"], np.ascontiguousarray(actions, dtype=np.uint16).reshape(self.env.num_boards))

    def fetch(self, *keys):
        """host copies; the mask comes back as [N][65] (the device buffer is word-major
        [65][mask_stride])"""
        out = super().fetch(*keys)
        if "mask" in out:
            out["mask"] = np.ascontiguousarray(out["mask"][:, : self.env.num_boards].T)
        return out


class _OneArray:
    """One owned device array whose `ptr` is the address itself (callers hand it to torch and to
    C); None once closed.  The memory is a one-entry _DeviceArrays, which also frees it when
    this object is dropped."""

    def _allocate(self, env, dtype, shape):
        self.env, self._mem = env, _DeviceArrays(env, {"data": (dtype, shape)})

    @property
    def ptr(self):
        return self._mem.ptr.get("data")

    def _host(self, shape):
        """host copy of the leading `shape` of the array"""
        dt = self._mem._spec["data"][0]
        return fetch_arrays(self.env, self._mem.ptr, ("data",), lambda k: (dt, shape))["data"]

    def close(self):
        self._mem.close()


class TraceBuffer(_OneArray):
    """Device trace of rollout_device: one uint64 word per board per ply ([ply][board]):
    action played (int16, -1 = the driver's no-move reset), reward (int16), done, reason."""

    def __init__(self, env, plies):
        self.plies = int(plies)
        self._allocate(env, np.uint64, (self.plies, env.num_boards))

    def fetch(self, plies=None):
        """host copy of the first `plies` plies as dict(action, reward, done, reason) [ply][board]"""
        w = self.raw(plies)
        return dict(action=(w & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16),
                    reward=((w >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16),
                    done=((w >> np.uint64(32)) & np.uint64(0xFF)).astype(np.uint8),
                    reason=((w >> np.uint64(40)) & np.uint64(0xFF)).astype(np.uint8))

    def raw(self, plies=None):
        """host copy of the first `plies` plies as the packed words, uint64 [ply][board]"""
        return self._host((self.plies if plies is None else int(plies), self.env.num_boards))


class PlanesBuffer(_OneArray):
    """Device memory of encode_planes' output: [rows][board_stride] raw elements of `dtype`
    (board_stride >= 24 * 64 elements, a multiple of 8; rows = N, or the row count of an
    encode_planes_rows batch)."""

    _RAW = {"float32": np.float32, "float16": np.uint16, "bfloat16": np.uint16}

    def __init__(self, env, dtype="float16", layout="nchw", board_stride=None, rows=None):
        if dtype not in self._RAW:
            raise ValueError(f"dtype must be one of {sorted(self._RAW)}, got {dtype!r}")
        if layout not in PLANES_LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(PLANES_LAYOUTS)}, got {layout!r}")
        self.dtype, self.layout = dtype, layout
        self.board_stride = int(PLANES * 64 if board_stride is None else board_stride)
        if self.board_stride < PLANES * 64 or self.board_stride % 8:
            raise ValueError(f"board_stride {self.board_stride}: at least {PLANES * 64}, a multiple of 8")
        self.rows = env.num_boards if rows is None else _rows(rows)
        self._allocate(env, self._RAW[dtype], (self.rows, self.board_stride))
        self.nbytes = self._mem._shape("data")[1]

    def raw(self):
        """host copy of the raw elements, [rows][board_stride] (float32, or uint16 bit patterns)"""
        return self._host((self.rows, self.board_stride))

    def fetch(self):
        """host copy decoded to float32: [rows,24,8,8] ("nchw") or [rows,8,8,24] ("nhwc")"""
        a = self.raw()[:, : PLANES * 64]
        if self.dtype == "float16":
            a = a.view(np.float16).astype(np.float32)
        elif self.dtype == "bfloat16":
            a = (a.astype(np.uint32) << np.uint32(16)).view(np.float32)
        shape = (24, 8, 8) if self.layout == "nchw" else (8, 8, 24)
        return np.ascontiguousarray(a).reshape((self.rows,) + shape)


def planes_format(out, dtype=None, layout=None, stride=None, default_stride=0):
    """(buffer or None, dtype, layout, stride) of a planes output: `out` a PlanesBuffer (whose
    dtype, layout and stride stand where the overrides are None) or anything else (a device
    pointer, None: float16, "nchw", default_stride)"""
    buf = out if isinstance(out, PlanesBuffer) else None
    dtype = dtype if dtype is not None else (buf.dtype if buf else "float16")
    layout = layout if layout is not None else (buf.layout if buf else "nchw")
    if stride is None:
        stride = buf.board_stride if buf else default_stride
    if dtype not in POLICY_DTYPES:
        raise ValueError(f"dtype must be one of {sorted(POLICY_DTYPES)}, got {dtype!r}")
    if layout not in PLANES_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(PLANES_LAYOUTS)}, got {layout!r}")
    return buf, dtype, layout, int(stride)


class _Staging:
    """The grow-by-doubling device buffer a host list is uploaded into before a launch reads it:
    `cap` items of bytes_per_item bytes at `ptr`.  The env is held weakly (it owns its staging
    buffers)."""

    def __init__(self, env, bytes_per_item):
        self._env, self._L, self._device = weakref.ref(env), env._L, env.device
        self.item, self.ptr, self.cap = int(bytes_per_item), None, 0

    @property
    def env(self):
        return self._env()

    def reserve(self, m):
        """the address of room for m items: max(256, m rounded up to a power of two) of them"""
        if m > self.cap:
            self.close()  # (waits for the device: no launch still reads the old buffer)
            cap = max(256, 1 << (m - 1).bit_length())
            self.ptr, self.cap = device_alloc(self._L, self._device, self.item * cap), cap
        return self.ptr

    def close(self):
        if self.ptr:
            if self.env is not None:
                self.env.synchronize()
            device_free(self._L, self._device, self.ptr)
        self.ptr, self.cap = None, 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def upload_indices(staging, values, rows=None, what="rows {rows} != the board array's length {size}", part=0):
    """(device pointer to int32[m], m) of a host index list, uploaded into part `part` of
    `staging` (int32[cap] each) on its env's stream; (None, 0) for an empty list, which uploads
    nothing.  rows: the length the caller stated, None = the list's; `what` words the mismatch."""
    b = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
    b = np.clip(b, -1, 2 ** 31 - 1).astype(np.int32)  # (anything out of range stays out of range)
    if rows is not None and int(rows) != b.size:
        raise ValueError(what.format(rows=rows, size=b.size))
    if not b.size:
        return None, 0
    p = staging.reserve(b.size) + 4 * part * staging.cap
    upload(staging.env, p, b)
    return p, int(b.size)
