"""Measurement: the device legal-move priors (gc_env_policy_priors) at N = 65 536 on mid-game masks.

Prints one JSON line: per logit type (float32, bfloat16) the us per launch (device events on the
env's stream, a warm-up, then REPS windows of LAUNCHES launches; every time is the median of the
windows, the per-window values beside it) of
  priors_us          identity rows (rows = N), cap = 64
  priors_indexed_us  rows = N / 8 through a random board index (the shape of a batched search)
  priors_permuted_us rows = N through a random permutation (what the gathered mask reads cost)
  sample_us          gc_env_sample_policy on the same logits and mask, in the same process
and, once, the write bandwidth gc_env_encode_planes reaches in this session (float16, NCHW),
from which store_us = rows * cap * 6 bytes at that bandwidth; the yardstick for the identity leg
is sample_us + store_us.  If torch imports and sees the GPU, a child process times the dense
framework path on the same data: unpack the mask to bool, masked_fill, softmax, topk(cap).

    python tools/priors_bench.py [--boards N] [--plies P] [--out profiles/policy_priors.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from policy_sample_bench import ROW, make_logits, median, unpack_mask  # noqa: E402

WARMUP, LAUNCHES, REPS = 10, 100, 3
DENSE = 20
CAP = 64


def torch_leg(mask_path, dtypes):
    """child process: the dense path in torch on the same logits and masks -> one JSON line"""
    import torch

    if not torch.cuda.is_available():
        print(json.dumps({"torch": None}))
        return
    raw = np.load(mask_path)
    n = raw.shape[0]
    words = torch.from_numpy(raw.view(np.int64)).cuda()  # [n][65], what step_device leaves (transposed)
    shifts = torch.arange(64, device="cuda", dtype=torch.int64)
    assert (unpack_mask(raw[:64]) == ((words[:64, :, None] >> shifts) & 1).bool().reshape(64, -1)[:, :ROW].cpu().numpy()).all()
    out = {"torch": torch.__version__}
    for dtype in dtypes:
        host = make_logits(n, dtype)
        if dtype == "float32":
            logits = torch.from_numpy(host).cuda()
        else:
            logits = torch.from_numpy(host.view(np.int16)).cuda().view(torch.bfloat16)

        def once():
            mask = ((words[:, :, None] >> shifts) & 1).bool().reshape(n, -1)[:, :ROW]
            x = logits.float().masked_fill(~mask, float("-inf"))
            p = torch.softmax(x, dim=1)
            return torch.topk(p, CAP, dim=1)

        for _ in range(3):
            once()
        torch.cuda.synchronize()
        times = []
        for _ in range(REPS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(DENSE):
                once()
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1) * 1e3 / DENSE)
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
    rows_idx = max(1, n // 8)
    res = {"boards": n, "plies": args.plies, "cap": CAP, "mean_legal": round(float(o["count"].mean()), 2),
           "max_legal": int(o["count"].max()), "launches": LAUNCHES, "reps": REPS, "mask_stride": io.mask_stride,
           "indexed_rows": rows_idx}

    def window(fn, k):
        env.record_event(4)
        for _ in range(k):
            fn()
        env.record_event(5)
        env.synchronize()
        return env.elapsed_ms(4, 5) * 1e3 / k

    # the write bandwidth of this session: encode_planes, float16 NCHW, its default stores
    planes = env.planes_buffer(dtype="float16")
    for _ in range(WARMUP):
        env.encode_planes(planes)
    env.synchronize()
    tp = [window(lambda: env.encode_planes(planes), LAUNCHES) for _ in range(REPS)]
    gbps = planes.nbytes / (median(tp) * 1e-6) / 1e9
    res["planes"] = {"bytes": int(planes.nbytes), "encode_us": round(median(tp), 2),
                     "encode_us_reps": [round(t, 2) for t in tp], "write_GBps": round(gbps, 1)}
    planes.close()

    out_full = env.priors_buffer(n, cap=CAP, logit_index=True)
    out_idx = env.priors_buffer(rows_idx, cap=CAP, logit_index=True)
    boards = np.random.default_rng(5).integers(0, n, size=rows_idx).astype(np.int32)
    perm = np.random.default_rng(6).permutation(n).astype(np.int32)

    def upload(a):
        v = ctypes.c_void_p()
        _lib.check(env._L.gc_device_alloc(env.device, ctypes.c_uint64(a.nbytes), ctypes.byref(v)))
        _lib.check(env._L.gc_env_copy(env._h, v.value, _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))
        return v.value

    d_boards, d_perm = upload(boards), upload(perm)

    for dtype in dtypes:
        host = make_logits(n, dtype)
        src = upload(host)
        draw = [0]

        def sample():
            env.sample_policy(io, src, dtype=dtype, draw=draw[0])
            draw[0] += 1

        def priors():
            env.policy_priors(io, src, out_full, dtype=dtype)

        def indexed():
            env.policy_priors(io, src, out_idx, boards=d_boards, rows=rows_idx, dtype=dtype)

        def permuted():
            env.policy_priors(io, src, out_full, boards=d_perm, rows=n, dtype=dtype)

        for _ in range(WARMUP):
            sample()
            priors()
            indexed()
            permuted()
        env.synchronize()
        # alternate the legs, so that drift of the machine falls on all of them
        ts, tf, ti, tq = [], [], [], []
        for _ in range(REPS):
            ts.append(window(sample, LAUNCHES))
            tq.append(window(permuted, LAUNCHES))
            tf.append(window(priors, LAUNCHES))  # (the identity leg is the last writer of out_full)
            ti.append(window(indexed, LAUNCHES))
        # what was timed is right: counts, ascending legal actions, priors summing to 1
        got = out_full.fetch()
        assert (got["count"] == o["count"]).all(), "count differs from the step's"
        k = np.minimum(got["count"], CAP)
        inside = np.arange(CAP)[None, :] < k[:, None]
        a = np.where(inside, got["actions"], 0).astype(np.int64)
        word = o["mask"][np.arange(n)[:, None], a >> 6]
        assert (((word >> (a & 63).astype(np.uint64)) & np.uint64(1)).astype(bool) | ~inside).all(), "an illegal action"
        assert (got["actions"][~inside] == 0xFFFF).all() and (got["priors"][~inside] == 0).all(), "padding"
        full = got["count"] <= CAP
        s = got["priors"].astype(np.float64).sum(axis=1)
        assert (np.abs(s[full & (k > 0)] - 1.0) < 1e-4).all(), "priors do not sum to 1"
        gi = out_idx.fetch("count", "actions")
        assert (gi["count"] == o["count"][boards]).all() and (gi["actions"] == got["actions"][boards]).all()
        store_us = n * CAP * 6 / (gbps * 1e9) * 1e6
        spread = max(max(t) - min(t) for t in (ts, tf))
        res[dtype] = {"priors_us": round(median(tf), 2), "priors_us_reps": [round(t, 2) for t in tf],
                      "priors_indexed_us": round(median(ti), 2), "priors_indexed_us_reps": [round(t, 2) for t in ti],
                      "priors_permuted_us": round(median(tq), 2), "priors_permuted_us_reps": [round(t, 2) for t in tq],
                      "sample_us": round(median(ts), 2), "sample_us_reps": [round(t, 2) for t in ts],
                      "out_bytes": n * CAP * 6 + n * 4, "store_us": round(store_us, 2),
                      "yardstick_us": round(median(ts) + store_us, 2),
                      "over_yardstick_us": round(median(tf) - median(ts) - store_us, 2),
                      "window_spread_us": round(spread, 2)}
        env._L.gc_device_free(env.device, ctypes.c_void_p(src))
        del host
    raw_mask = o["mask"]
    for p in (d_boards, d_perm):
        env._L.gc_device_free(env.device, ctypes.c_void_p(p))
    out_full.close()
    out_idx.close()
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
