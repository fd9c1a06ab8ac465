"""Measurement: the indexed expansion of a batched search -- step_boards, encode_planes_rows and
the three-call sequence clone_boards + step_boards + encode_planes_rows -- on an env of N = 65 536
boards after 40 random plies, against the dense pair it replaces (step_device with the padded
mask stride + encode_planes over all N), in the same process.

Prints one JSON line.  Every time is us per launch (or per sequence) from device events on the
env's stream: a warm-up, then REPS windows of LAUNCHES launches, the legs alternated so that drift
of the machine falls on all of them; the median of the windows, the per-window values beside it.
The calls go straight to the C ABI with device pointers, so a window holds no host copy.

  rows in {256, 1024, 4096} distinct random boards:
    step_us      step_boards, mask / count / obs on.  Every launch of a window steps the same boards
                 under the next recorded action: the actions are the picks a dense twin env played
                 from the same checkpoint (always legal, auto-reset on), and the env is put back to
                 that checkpoint before every window, so each window times the same LAUNCHES steps.
    encode_us    encode_planes_rows, float16 NCHW, side-to-move view
    expand_us    clone_boards(parent -> child) + step_boards(child) + encode_planes_rows(child),
                 parents and children disjoint; the clone rewinds the children, so the sequence
                 repeats exactly
  dense_step_us / dense_encode_us / dense_pair_us: the dense calls over all N on the twin
  A/B at rows = 1024: step_boards with 64-lane and with 256-lane workgroups (GC_ROWS_BLOCK);
  at rows = 1024 and 4096: encode_planes_rows with plain and non-temporal stores (GC_PLANES_NT).
Both switches are read per call.

    python tools/expand_bench.py [--boards N] [--plies P] [--out profiles/step_boards.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-chess_amd"))

WARMUP, LAUNCHES, REPS = 10, 100, 3
ROWS = (256, 1024, 4096)


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=65536)
    ap.add_argument("--plies", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    n = args.boards
    rows_all = [r for r in ROWS if 2 * r <= n]
    L = _lib.load()
    tree = BatchedChessEnv(n, device=0, seed=11)
    dense = BatchedChessEnv(n, device=0, seed=11)
    dio = dense.device_io()
    for _ in range(args.plies):  # random plies with auto-reset: mid-game boards
        dense.step_device(dio, autoreset=True)
    dense.synchronize()
    blob = dense.checkpoint()
    tree.load(blob)
    tio = tree.device_io(pick=False)

    def upload(a):
        a = np.ascontiguousarray(a)
        v = ctypes.c_void_p()
        _lib.check(L.gc_device_alloc(tree.device, ctypes.c_uint64(max(a.nbytes, 1)), ctypes.byref(v)))
        _lib.check(L.gc_env_copy(tree._h, v.value, _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))
        return v.value

    # the dense twin's next LAUNCHES steps: the actions it plays (its picks), board by board
    picks = np.zeros((LAUNCHES, n), dtype=np.uint16)
    for k in range(LAUNCHES):
        picks[k] = dio.fetch("pick")["pick"]
        dense.step_device(dio, autoreset=True)
    dense.synchronize()

    def window(env, fn, k):
        env.record_event(4)
        for j in range(k):
            fn(j)
        env.record_event(5)
        env.synchronize()
        return env.elapsed_ms(4, 5) * 1e3 / k

    perm = np.random.default_rng(5).permutation(n).astype(np.int32)
    res = {"boards": n, "plies": args.plies, "launches": LAUNCHES, "reps": REPS, "mask_stride": tio.mask_stride,
           "planes": "float16 nchw perspective"}
    freed, keep = [], []  # device arrays to free; buffer objects the closures' pointers belong to

    # ---- the dense pair on the twin
    planes_d = dense.planes_buffer(dtype="float16")
    p = dio.ptr

    def dense_step(_):
        _lib.check(L.gc_env_step_device2(dense._h, p["pick"], p["reward"], p["done"], p["reason"], p["mask"], p["obs"],
                                         p["count"], p["pick"], 1, dio.mask_stride))

    def dense_encode(_):
        _lib.check(L.gc_env_encode_planes(dense._h, planes_d.ptr, 1, 0, 1))

    def dense_pair(j):
        dense_step(j)
        dense_encode(j)

    for j in range(WARMUP):
        dense_pair(j)
    dense.synchronize()

    legs = {"dense_step_us": (dense, dense_step, None), "dense_encode_us": (dense, dense_encode, None),
            "dense_pair_us": (dense, dense_pair, None)}

    # ---- the indexed calls on the tree env
    for rows in rows_all:
        boards, kids = perm[:rows], perm[rows: 2 * rows]
        d_boards, d_kids = upload(boards), upload(kids)
        d_acts = upload(picks[:, boards])          # [LAUNCHES][rows]
        d_kid_acts = upload(picks[0][boards])      # the parents' legal moves, played by their clones
        rb = tree.rows_buffer(rows)
        planes_r = tree.planes_buffer(dtype="float16", rows=rows)
        freed += [d_boards, d_kids, d_acts, d_kid_acts]
        keep += [rb, planes_r]
        q = rb.ptr

        def step(j, rows=rows, d_boards=d_boards, d_acts=d_acts, q=q):
            _lib.check(L.gc_env_step_boards(tree._h, d_boards, d_acts + 2 * rows * (j % LAUNCHES), rows, q["reward"],
                                            q["done"], q["reason"], q["count"], tio.ptr["mask"], tio.mask_stride,
                                            q["obs"], 1))

        def encode(_, rows=rows, d_boards=d_boards, planes_r=planes_r):
            _lib.check(L.gc_env_encode_planes_rows(tree._h, d_boards, rows, planes_r.ptr, 1, 0, 1))

        def expand(_, rows=rows, d_boards=d_boards, d_kids=d_kids, d_kid_acts=d_kid_acts, q=q, planes_r=planes_r):
            _lib.check(L.gc_env_clone_boards(tree._h, tree._h, d_boards, d_kids, rows))
            _lib.check(L.gc_env_step_boards(tree._h, d_kids, d_kid_acts, rows, q["reward"], q["done"], q["reason"],
                                            q["count"], tio.ptr["mask"], tio.mask_stride, q["obs"], 0))
            _lib.check(L.gc_env_encode_planes_rows(tree._h, d_kids, rows, planes_r.ptr, 1, 0, 1))

        legs[f"rows{rows}.step_us"] = (tree, step, None)
        legs[f"rows{rows}.encode_us"] = (tree, encode, None)
        legs[f"rows{rows}.expand_us"] = (tree, expand, None)
        if rows == 1024:
            for b in (64, 256):
                legs[f"rows{rows}.step_block{b}_us"] = (tree, step, ("GC_ROWS_BLOCK", str(b)))
        if rows in (1024, 4096):
            for nt in (0, 1):
                legs[f"rows{rows}.encode_nt{nt}_us"] = (tree, encode, ("GC_PLANES_NT", str(nt)))

    def run(name, k):
        env, fn, switch = legs[name]
        if switch:
            os.environ[switch[0]] = switch[1]
        try:
            if ".step" in name or ".expand" in name:  # every window starts from the same boards
                tree.load(blob)
            return window(env, fn, k)
        finally:
            if switch:
                del os.environ[switch[0]]

    for name in legs:
        run(name, WARMUP)
    times = {name: [] for name in legs}
    for _ in range(REPS):
        for name in legs:
            times[name].append(run(name, LAUNCHES))

    # what was timed is right: the replayed steps end where the dense twin's did
    tree.load(blob)
    rows = rows_all[-1]
    boards = perm[:rows]
    window(tree, legs[f"rows{rows}.step_us"][1], LAUNCHES)
    dense.load(blob)
    for k in range(LAUNCHES):
        _lib.check(L.gc_env_copy(dense._h, dio.ptr["pick"], _lib.ptr(picks[k]), ctypes.c_uint64(picks[k].nbytes), 1))
        dense.step_device(dio, autoreset=True)
    bt, mt = tree.boards()
    bd, md = dense.boards()
    assert (bt[boards] == bd[boards]).all() and (mt[boards] == md[boards]).all(), "the replayed steps differ from the dense twin's"
    res["checked"] = f"{rows} boards after {LAUNCHES} replayed steps equal the dense twin's"

    for name, v in times.items():
        d = res
        parts = name.split(".")
        for part in parts[:-1]:
            d = d.setdefault(part, {})
        d[parts[-1]] = round(median(v), 2)
        d[parts[-1] + "_reps"] = [round(t, 2) for t in v]
    for rows in rows_all:
        r = res[f"rows{rows}"]
        r["step_plus_encode_us"] = round(r["step_us"] + r["encode_us"], 2)
        r["dense_pair_over_indexed"] = round(res["dense_pair_us"] / r["step_plus_encode_us"], 2)
    if "rows1024" in res:
        res["indexed_faster_than_dense_at_1024"] = bool(res["rows1024"]["step_plus_encode_us"] < res["dense_pair_us"])

    for ptr in freed:
        L.gc_device_free(tree.device, ctypes.c_void_p(ptr))
    for b in keep:
        b.close()
    planes_d.close()
    dio.close()
    tio.close()
    dense.close()
    tree.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
