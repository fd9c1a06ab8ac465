"""Measurement: boards cloned between envs on the device (gc_env_clone_boards) at N = 65 536.

A game env after PLIES random plies (windows in use) and a search env of the same size that has
played other games.  Per pair count m (4 096 and 65 536; random distinct sources, random distinct
destinations, the index arrays in device memory): the clone's us per launch by device events on
the destination's stream (a warm-up, then REPS windows of LAUNCHES launches, median) -- once with
the windows as they are and once with every source freshly reset (empty windows: no table is
touched).  Beside it: a device-to-device copy of m * (32 KiB + 80 B), the bytes of m whole boards
with their tables, on the same stream (gc_env_copy kind 3, timed the same way), and the wall
time of checkpoint() + load() of the search env, the route to a board's full state without the
clone.  Prints one JSON line and writes it to --out.

    python tools/clone_bench.py [--boards N] [--plies P] [--out profiles/clone_boards.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-chess_amd"))

WARMUP, LAUNCHES, REPS = 3, 20, 3
COPIES = 10
BOARD_BYTES = 32 * 1024 + 80  # a board's window table and its slab fields


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=65536)
    ap.add_argument("--plies", type=int, default=40)
    ap.add_argument("--pairs", type=int, nargs="*", default=[4096, 65536])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clone_boards.json"))
    args = ap.parse_args()

    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    n = args.boards
    game = BatchedChessEnv(n, device=0, seed=11)
    search = BatchedChessEnv(n, device=0, seed=12)
    for env in (game, search):
        io = env.device_io()
        for _ in range(args.plies):
            env.step_device(io, autoreset=True)
        env.synchronize()
        io.close()
    res = {"boards": n, "plies": args.plies, "launches": LAUNCHES, "reps": REPS, "board_bytes": BOARD_BYTES,
           "mean_window": round(game.window_sum() / n, 2), "mean_window_search": round(search.window_sum() / n, 2)}

    def dalloc(nbytes):
        v = ctypes.c_void_p()
        _lib.check(search._L.gc_device_alloc(search.device, ctypes.c_uint64(nbytes), ctypes.byref(v)))
        return v.value

    def upload(a):
        p = dalloc(a.nbytes)
        _lib.check(search._L.gc_env_copy(search._h, p, _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))
        return p

    def window(fn, k):
        search.record_event(4)
        for _ in range(k):
            fn()
        search.record_event(5)
        search.synchronize()
        return search.elapsed_ms(4, 5) * 1e3 / k

    rng = np.random.RandomState(3)
    legs = {}
    for m in args.pairs:
        m = min(m, n)
        s, d = upload(rng.permutation(n)[:m].astype(np.int32)), upload(rng.permutation(n)[:m].astype(np.int32))
        nbytes = m * BOARD_BYTES
        a, b = dalloc(nbytes), dalloc(nbytes)
        legs[m] = dict(s=s, d=d, a=a, b=b, nbytes=nbytes, clone=[], empty=[], copy=[])

    def run(tag):
        for m, g in legs.items():
            def clone():
                search.clone_boards(game, g["s"], g["d"], count=m)

            def copy():
                _lib.check(search._L.gc_env_copy(search._h, g["b"], g["a"], ctypes.c_uint64(g["nbytes"]), 3))

            for _ in range(WARMUP):
                clone()
            copy()
            search.synchronize()
            for _ in range(REPS):  # alternate, so that drift of the machine falls on both
                g[tag].append(window(clone, LAUNCHES))
                if tag == "clone":
                    g["copy"].append(window(copy, COPIES))

    run("clone")
    assert search.clone_errors() == 0
    # the route without the clone: the whole env through a host blob
    walls = []
    for _ in range(REPS):
        search.synchronize()
        t0 = time.perf_counter()
        search.load(search.checkpoint())
        search.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    res["checkpoint_load_ms"] = round(median(walls), 2)
    res["checkpoint_load_ms_reps"] = [round(t, 2) for t in walls]
    res["checkpoint_bytes"] = len(search.checkpoint())
    game.reset(states=False)  # every source's window empty
    assert game.window_sum() == 0
    run("empty")

    for m, g in legs.items():
        res[f"m{m}"] = {
            "pairs": m, "copy_bytes": g["nbytes"],
            "clone_us": round(median(g["clone"]), 2), "clone_us_reps": [round(t, 2) for t in g["clone"]],
            "clone_empty_us": round(median(g["empty"]), 2), "clone_empty_us_reps": [round(t, 2) for t in g["empty"]],
            "d2d_copy_us": round(median(g["copy"]), 2), "d2d_copy_us_reps": [round(t, 2) for t in g["copy"]],
            "clone_over_copy": round(median(g["clone"]) / median(g["copy"]), 3),
            "copy_GBps": round(2 * g["nbytes"] / median(g["copy"]) / 1e3, 1)}
        for p in (g["s"], g["d"], g["a"], g["b"]):
            search._L.gc_device_free(search.device, ctypes.c_void_p(p))

    game.close()
    search.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
