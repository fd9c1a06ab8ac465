"""Measurement: the sample store's minibatch launch (gc_replay_sample) against the same batch
assembled in torch.

Prints one JSON line.  A store of GAMES games (cap 64) is filled from real mid-game positions
(step_device with auto-reset) and synthetic roots of 35 entries until its ring of CAPACITY samples
is full.  Then, per batch size (256, 1 024, 4 096 rows; float16 NCHW planes in the side-to-move
view, the dense [rows][4100] float32 target, the sparse target, z and slot; slots drawn on the
device), the us per launch: device events on the env's stream, a warm-up, then REPS windows of
LAUNCHES launches, plain and non-temporal stores alternating window by window; every time is the
median of the windows, the per-window values beside it.  rows = 4 is the launch floor.
written_bytes / time is set against the HBM rates of MI355X_MICROARCH.md (8 TB/s peak, about 6.3
achievable).  If torch imports and sees the GPU, a child process times the torch formulation on
the same box: float16 planes kept encoded, [capacity][1536], index_select of planes and z, and
scatter_ of the gathered (index, value) lists into zeros (no mirroring, no division: the lists are
kept ready-made, which favours torch).

    python tools/replay_bench.py [--out profiles/replay.json] [--no-torch]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-chess_amd"))

GAMES, CAP, MAX_PLIES, CAPACITY = 4096, 64, 8, 65536
ENTRIES = 35
ROWS = (256, 1024, 4096)
ROW = 4100
WARMUP, LAUNCHES, REPS = 20, 200, 5
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12


def median(x):
    s = sorted(x)
    return s[len(s) // 2]


def written_bytes(rows):
    return rows * (24 * 64 * 2 + ROW * 4 + CAP * 8 + 8)


def torch_leg():
    """child process: the batch assembled in torch from stored encoded planes -> one JSON line"""
    import torch

    if not torch.cuda.is_available():
        print(json.dumps({"torch": None}))
        return
    g = torch.Generator(device="cuda").manual_seed(1)
    planes = (torch.rand(CAPACITY, 24 * 64, device="cuda", generator=g) < 0.1).half()
    aidx = torch.rand(4096, ROW, device="cuda", generator=g).argsort(dim=1)[:, :CAP]  # distinct within a row
    aidx = aidx.repeat(CAPACITY // 4096, 1).contiguous()
    vals = torch.rand(CAPACITY, CAP, device="cuda", generator=g)
    vals[:, ENTRIES:] = 0
    z = torch.rand(CAPACITY, device="cuda", generator=g)
    out = {"torch": torch.__version__}
    for rows in ROWS:
        def once():
            idx = torch.randint(CAPACITY, (rows,), device="cuda")
            p = planes.index_select(0, idx)
            pi = torch.zeros(rows, ROW, device="cuda").scatter_(1, aidx.index_select(0, idx), vals.index_select(0, idx))
            return p, pi, z.index_select(0, idx)

        for _ in range(WARMUP):
            once()
        torch.cuda.synchronize()
        times = []
        for _ in range(REPS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(LAUNCHES):
                once()
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1) * 1e3 / LAUNCHES)
        out[str(rows)] = {"torch_us": round(median(times), 2), "torch_us_reps": [round(t, 2) for t in times]}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-leg", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.torch_leg:
        torch_leg()
        return

    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(GAMES, device=0, seed=11)
    io = env.device_io()
    store = env.sample_store(cap=CAP, max_plies=MAX_PLIES, capacity=CAPACITY)
    rng = np.random.default_rng(3)
    actions = np.full((GAMES, CAP), 0xFFFF, dtype=np.uint16)
    visits = np.zeros((GAMES, CAP), dtype=np.int32)
    for g in range(GAMES):
        actions[g, :ENTRIES] = rng.choice(ROW, size=ENTRIES, replace=False)
    visits[:, :ENTRIES] = rng.integers(1, 200, size=(GAMES, ENTRIES))

    def upload(a):
        v = ctypes.c_void_p()
        _lib.check(env._L.gc_device_alloc(env.device, ctypes.c_uint64(a.nbytes), ctypes.byref(v)))
        _lib.check(env._L.gc_env_copy(env._h, v.value, _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))
        return v.value

    d_act, d_vis = upload(actions), upload(visits)
    d_done, d_reason = upload(np.ones(GAMES, dtype=np.uint8)), upload(np.ones(GAMES, dtype=np.uint8))
    for _ in range(30):  # mid-game positions
        env.step_device(io, autoreset=True)
    for _ in range(CAPACITY // (GAMES * MAX_PLIES)):
        for _ in range(MAX_PLIES):
            store.record((d_act, d_vis, CAP))
            env.step_device(io, autoreset=True)
        store.commit(d_done, reason=d_reason)
    c = store.counters()
    assert c["live"] == CAPACITY and c["dropped"] == 0, c
    res = {"games": GAMES, "cap": CAP, "capacity": CAPACITY, "entries": ENTRIES, "launches": LAUNCHES, "reps": REPS,
           "store_bytes": store.device_bytes(), "dtype": "float16", "layout": "nchw",
           "hbm_peak_TBps": HBM_PEAK / 1e12, "hbm_achievable_TBps": HBM_ACHIEVABLE / 1e12}

    def window(fn, k):
        env.record_event(4)
        for _ in range(k):
            fn()
        env.record_event(5)
        env.synchronize()
        return env.elapsed_ms(4, 5) * 1e3 / k

    draw = [0]
    for rows in (4,) + ROWS:
        def sample():
            store.sample(rows, seed=5, draw=draw[0])
            draw[0] += 1

        t = {"0": [], "1": []}
        for nt in t:
            os.environ["GC_REPLAY_NT"] = nt
            for _ in range(WARMUP):
                sample()
        env.synchronize()
        for _ in range(REPS):  # alternate the forms, so that drift of the machine falls on both
            for nt in t:
                os.environ["GC_REPLAY_NT"] = nt
                t[nt].append(window(sample, LAUNCHES))
        del os.environ["GC_REPLAY_NT"]
        # what was timed is right: slots of the ring, the same rows again through an explicit
        # index, targets of ENTRIES entries that sum to 1
        got = store.sample(rows, seed=5, draw=7).fetch("slot", "pi_dense", "z")
        assert (got["slot"] >= 0).all() and (got["slot"] < CAPACITY).all(), "slots"
        again = store.sample(rows, index=got["slot"]).fetch("slot", "pi_dense", "z")
        assert all(got[k].tobytes() == again[k].tobytes() for k in got), "the explicit index gives another batch"
        assert (np.abs(got["pi_dense"].astype(np.float64).sum(axis=1) - 1.0) < 1e-5).all(), "targets do not sum to 1"
        assert (np.count_nonzero(got["pi_dense"], axis=1) == ENTRIES).all() and (np.abs(got["z"]) == 1).all()
        wb = written_bytes(rows)
        r = {"written_bytes": wb}
        for nt, name in (("0", "plain"), ("1", "nt")):
            us = median(t[nt])
            r[f"{name}_us"] = round(us, 2)
            r[f"{name}_us_reps"] = [round(v, 2) for v in t[nt]]
            r[f"{name}_TBps"] = round(wb / (us * 1e-6) / 1e12, 3)
            r[f"{name}_frac_hbm_peak"] = round(wb / (us * 1e-6) / HBM_PEAK, 3)
        res[str(rows)] = r
    for p in (d_act, d_vis, d_done, d_reason):
        env._L.gc_device_free(env.device, ctypes.c_void_p(p))
    store.close()
    io.close()
    env.close()

    res["torch"] = None
    if not args.no_torch:
        import importlib.util

        if importlib.util.find_spec("torch") is not None:  # a fresh process: torch brings its own HIP runtime
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-leg"], capture_output=True, text=True)
            try:
                t = json.loads(r.stdout.strip().splitlines()[-1])
                res["torch"] = t.pop("torch")
                for k, v in t.items():
                    res[k].update(v)
            except Exception:
                res["torch_error"] = (r.stderr or r.stdout)[-300:]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
