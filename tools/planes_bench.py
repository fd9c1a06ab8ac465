"""Measurement: the device plane encoder (gc_env_encode_planes) at N = 65 536 on mid-game boards.

Prints one JSON line: per leg (float16 / bfloat16 / float32, each NCHW and channels-last) the
encoder's us per launch with plain and with non-temporal stores (GC_PLANES_NT, read per call;
device events on the env's stream, a warm-up, then REPS windows of LAUNCHES launches, median),
the bytes it writes, and the time of a device-to-device copy of a buffer of the same byte count
on the same stream (gc_env_copy kind 3) timed the same way: the copy reads and writes those
bytes, the encoder only writes them, so encode_us <= d2d_copy_us is the expectation.  If torch
imports and sees the GPU, a child process times the framework path on the same boards: the
absolute-view tensor built from the int8 observation and the host-fetched meta bytes with dense
ops (compare, cat, cast, permute); it cannot build planes 20-22, which it leaves zero.

    python tools/planes_bench.py [--boards N] [--plies P] [--out profiles/planes_encode.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-chess_amd"))

PLANES, ELEMS = 24, 24 * 64
WARMUP, LAUNCHES, REPS = 10, 100, 3
COPIES = 20
DTYPES = ("float16", "bfloat16", "float32")
LAYOUTS = ("nchw", "nhwc")
ITEM = {"float32": 4, "float16": 2, "bfloat16": 2}


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def torch_leg(path):
    """child process: the same tensor from obs and meta with framework ops -> one JSON line"""
    import torch

    if not torch.cuda.is_available():
        print(json.dumps({"torch": None}))
        return
    z = np.load(path)
    obs = torch.from_numpy(z["boards"]).cuda()  # int8 [N][64], what step_device's d_obs holds
    meta_h = torch.from_numpy(z["meta"]).pin_memory()  # uint8 [N][8], a host fetch every step
    n = obs.shape[0]
    ids = torch.tensor([1, 2, 3, 4, 5, 6, -1, -2, -3, -4, -5, -6], dtype=torch.int8, device="cuda")
    tdt = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}
    out = {"torch": torch.__version__}
    for dtype in DTYPES:
        for layout in LAYOUTS:
            def once():
                m = meta_h.cuda(non_blocking=True)
                pieces = (obs[:, None, :] == ids[None, :, None]).to(tdt[dtype])
                flags = (m[:, :7] != 0).to(tdt[dtype])[:, :, None].expand(n, 7, 64)
                mc = (m[:, 7:8].to(torch.float32) / 256.0).to(tdt[dtype])[:, :, None].expand(n, 1, 64)
                zeros = torch.zeros((n, 3, 64), dtype=tdt[dtype], device="cuda")
                ones = torch.ones((n, 1, 64), dtype=tdt[dtype], device="cuda")
                x = torch.cat([pieces, flags, mc, zeros, ones], dim=1)
                return x.permute(0, 2, 1).contiguous() if layout == "nhwc" else x

            for _ in range(3):
                once()
            torch.cuda.synchronize()
            times = []
            for _ in range(REPS):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(COPIES):
                    once()
                t1.record()
                torch.cuda.synchronize()
                times.append(t0.elapsed_time(t1) * 1e3 / COPIES)
            out[f"{dtype}_{layout}"] = {"torch_dense_us": round(median(times), 2),
                                        "torch_dense_us_reps": [round(t, 2) for t in times]}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=65536)
    ap.add_argument("--plies", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-leg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.torch_leg:
        torch_leg(args.torch_leg)
        return

    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    n = args.boards
    env = BatchedChessEnv(n, device=0, seed=11)
    io = env.device_io()
    for _ in range(args.plies):  # random plies: mid-game boards, windows in use
        env.step_device(io, autoreset=True)
    env.synchronize()
    boards, meta = env.boards()
    default_nt = os.environ.get("GC_PLANES_NT")
    res = {"boards": n, "plies": args.plies, "launches": LAUNCHES, "reps": REPS,
           "white_to_move": round(float(meta[:, 0].mean()), 3), "mean_move_count": round(float(meta[:, 7].mean()), 2)}

    def dalloc(nbytes):
        v = ctypes.c_void_p()
        _lib.check(env._L.gc_device_alloc(env.device, ctypes.c_uint64(nbytes), ctypes.byref(v)))
        return v.value

    def window(fn, k):
        env.record_event(4)
        for _ in range(k):
            fn()
        env.record_event(5)
        env.synchronize()
        return env.elapsed_ms(4, 5) * 1e3 / k

    def store_form(nt):
        if nt is None:
            os.environ.pop("GC_PLANES_NT", None)
        else:
            os.environ["GC_PLANES_NT"] = nt

    checked = False
    for dtype in DTYPES:
        nbytes = n * ELEMS * ITEM[dtype]
        src, dst = dalloc(nbytes), dalloc(nbytes)
        for layout in LAYOUTS:
            buf = env.planes_buffer(dtype=dtype, layout=layout)

            def encode(persp=False):
                env.encode_planes(buf, perspective=persp)

            def copy():
                _lib.check(env._L.gc_env_copy(env._h, dst, src, ctypes.c_uint64(nbytes), 3))

            for _ in range(WARMUP):
                encode()
            copy()
            env.synchronize()
            if not checked:  # the buffer holds the boards' planes (the tests compare every element)
                got = buf.fetch()
                assert (got[:, 23] == 1).all() and (got[:, 12, 0, 0] == meta[:, 0]).all()
                assert (got[:, :12].sum(axis=(1, 2, 3)) == (boards != 0).sum(axis=1)).all()
                checked = True
                del got
            # alternate the three, so that drift of the machine falls on all
            tp, tn, tc = [], [], []
            for _ in range(REPS):
                store_form("0")
                tp.append(window(encode, LAUNCHES))
                store_form("1")
                tn.append(window(encode, LAUNCHES))
                tc.append(window(copy, COPIES))
            store_form(default_nt)
            td = window(encode, LAUNCHES)  # the library's default store form
            tv = window(lambda: encode(True), LAUNCHES)
            best = min(median(tp), median(tn))
            res[f"{dtype}_{layout}"] = {
                "bytes": nbytes, "encode_plain_us": round(median(tp), 2), "encode_plain_us_reps": [round(t, 2) for t in tp],
                "encode_nt_us": round(median(tn), 2), "encode_nt_us_reps": [round(t, 2) for t in tn],
                "encode_default_us": round(td, 2), "encode_side_to_move_us": round(tv, 2),
                "d2d_copy_us": round(median(tc), 2), "d2d_copy_us_reps": [round(t, 2) for t in tc],
                "write_GBps": round(nbytes / best / 1e3, 1), "encode_le_copy": bool(best <= median(tc))}
            buf.close()
        for p in (src, dst):
            env._L.gc_device_free(env.device, ctypes.c_void_p(p))
    io.close()
    env.close()

    if not args.no_torch:
        try:
            import importlib.util

            have = importlib.util.find_spec("torch") is not None
        except Exception:
            have = False
        if have:  # a fresh process: torch brings its own HIP runtime
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "boards.npz")
                np.savez(path, boards=boards, meta=meta)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-leg", path],
                                   capture_output=True, text=True)
            try:
                t = json.loads(r.stdout.strip().splitlines()[-1])
                res["torch"] = t.pop("torch")
                for k, v in t.items():
                    res[k].update(v)
            except Exception:
                res["torch"] = None
                res["torch_error"] = (r.stderr or r.stdout)[-300:]
        else:
            res["torch"] = None
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
