"""Measurement: the device policy head (gc_env_sample_policy) at N = 65 536 on mid-game masks.

Prints one JSON line: per logit type (float32, bfloat16) the sampler's us per launch (device
events on the env's stream, a warm-up, then REPS windows of LAUNCHES launches), the mean legal
count, the bytes one dense read of the logits would move, and the time of a device-to-device
copy of the same logits buffer on the same stream (gc_env_copy kind 3) timed the same way.  If
torch imports and sees the GPU, a child process times the dense framework path on the same
data: masked_fill + softmax + multinomial + log-prob gather (the mask already unpacked to bool,
which a framework user would also have to do every step).

    python tools/policy_sample_bench.py [--boards N] [--plies P] [--out profiles/policy_sample.json]
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

ROW = 4100
WARMUP, LAUNCHES, REPS = 10, 100, 3
COPIES = 20


def make_logits(n, dtype, seed=21):
    """standard-normal logits [n][4100] as the raw device elements (bf16: round to nearest even)"""
    x = np.random.default_rng(seed).standard_normal((n, ROW), dtype=np.float32)
    if dtype == "float32":
        return x
    b = x.view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def unpack_mask(raw):
    """u64[n][65] -> bool[n][4100]"""
    n = raw.shape[0]
    bits = np.unpackbits(np.ascontiguousarray(raw[:, :64]).view(np.uint8).reshape(n, 512), axis=1, bitorder="little")
    out = np.zeros((n, ROW), dtype=bool)
    out[:, :4096] = bits.astype(bool)
    for c in range(4):
        out[:, 4096 + c] = (raw[:, 64] >> np.uint64(c)) & np.uint64(1) != 0
    return out


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def torch_leg(mask_path, dtypes):
    """child process: the dense path in torch on the same logits and masks -> one JSON line"""
    import torch

    if not torch.cuda.is_available():
        print(json.dumps({"torch": None}))
        return
    raw = np.load(mask_path)
    n = raw.shape[0]
    mask = torch.from_numpy(unpack_mask(raw)).cuda()
    out = {"torch": torch.__version__}
    for dtype in dtypes:
        host = make_logits(n, dtype)
        if dtype == "float32":
            logits = torch.from_numpy(host).cuda()
        else:
            logits = torch.from_numpy(host.view(np.int16)).cuda().view(torch.bfloat16)

        def once():
            x = logits.float().masked_fill(~mask, float("-inf"))
            p = torch.softmax(x, dim=1)
            a = torch.multinomial(p, 1)
            return a.squeeze(1).to(torch.int16), torch.log(p.gather(1, a)).squeeze(1)

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
        out[dtype] = {"torch_dense_us": round(median(times), 2), "torch_dense_us_reps": [round(t, 2) for t in times]}
        del logits
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=65536)
    ap.add_argument("--plies", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-leg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    dtypes = ("float32", "bfloat16")
    if args.torch_leg:
        torch_leg(args.torch_leg, dtypes)
        return

    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    n = args.boards
    env = BatchedChessEnv(n, device=0, seed=11)
    io = env.device_io(policy=True)
    for _ in range(args.plies):  # random plies: the masks are mid-game ones
        env.step_device(io, autoreset=True)
    env.synchronize()
    o = io.fetch("mask", "count")
    res = {"boards": n, "plies": args.plies, "mean_legal": round(float(o["count"].mean()), 2),
           "max_legal": int(o["count"].max()), "launches": LAUNCHES, "reps": REPS, "mask_stride": io.mask_stride}

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

    for dtype in dtypes:
        host = make_logits(n, dtype)
        src, dst = dalloc(host.nbytes), dalloc(host.nbytes)
        _lib.check(env._L.gc_env_copy(env._h, src, _lib.ptr(host), ctypes.c_uint64(host.nbytes), 1))
        draw = [0]

        def sample():
            env.sample_policy(io, src, dtype=dtype, draw=draw[0])
            draw[0] += 1

        def copy():
            _lib.check(env._L.gc_env_copy(env._h, dst, src, ctypes.c_uint64(host.nbytes), 3))

        for _ in range(WARMUP):
            sample()
        copy()
        env.synchronize()
        # alternate the two, so that drift of the machine falls on both
        ts, tc = [], []
        for _ in range(REPS):
            ts.append(window(sample, LAUNCHES))
            tc.append(window(copy, COPIES))
        # every sampled action is legal in the mask it came from
        pick = io.fetch("pick")["pick"]
        live = o["count"] > 0
        word = o["mask"][np.arange(n), np.minimum(pick, 4099) >> 6]
        legal = ((word >> (np.minimum(pick, 4099) & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
        assert (legal[live]).all() and (pick[~live] == 0xFFFF).all(), "sampled an illegal action"
        res[dtype] = {"sample_us": round(median(ts), 2), "sample_us_reps": [round(t, 2) for t in ts],
                      "dense_bytes": int(host.nbytes), "d2d_copy_us": round(median(tc), 2),
                      "d2d_copy_us_reps": [round(t, 2) for t in tc],
                      "copy_over_sample": round(median(tc) / median(ts), 1)}
        for p in (src, dst):
            env._L.gc_device_free(env.device, ctypes.c_void_p(p))
        del host
    raw_mask = o["mask"]
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
                path = os.path.join(d, "mask.npy")
                np.save(path, raw_mask)
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
