"""Measurement: gc_env_minimax (fixed-depth minimax search, gc_minimax.h) beside the other
network-free leaf evaluator and the full-width enumeration of the same generator, on the same
boards in the same process:

    minimax_us   one minimax call (tiebreak first, lists off, nodes off), device events
    playout_us   one playout launch (P = 8, 64 plies), device events
    perft_us     gc_engine_perft of the same depth and of depth + 1 over the same boards: a
                 host-synchronous call on host arrays, so HOST wall time, copies included.  perft(d)
                 generates down to ply d - 1 and counts the moves there; a depth-d search generates
                 down to ply d - 1 and counts the moves at ply d, so its full-width twin in generator
                 work is perft(d + 1)
    host         the CPU test's host build of the same search on one core (the first 64 rows)

Shapes: rows in {64, 1024}, depth in {1, 2, 3, 4}; the boards are `--plies` (40) random plies into
self-play.  One child process per row count (a fresh HIP context each); in a child, per depth, a
warm-up of every leg, then REPS windows of LAUNCHES[depth] calls per leg, the legs alternated so
that drift of the machine falls on all of them; times are us per CALL, reported as median
[min, max] over the windows.  nodes = the positions one call visits (its nodes output, summed over
the rows).  Prints one JSON line; --out also writes it to a file.

    python tools/minimax_bench.py [--out profiles/minimax.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-chess_amd"))

WARMUP, REPS = 3, 5
LAUNCHES = {1: 100, 2: 100, 3: 20, 4: 5}
PERFT_CALLS = 3
ROWS, DEPTHS, P, PLAYOUT_PLIES, HOST_ROWS = (64, 1024), (1, 2, 3, 4), 8, 64, 64


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 2), min=round(float(v.min()), 2), max=round(float(v.max()), 2))


def child(rows, plies0):
    from gym_chess_amd.engine import Engine
    from gym_chess_amd.env import BatchedChessEnv

    sys.path.insert(0, os.path.join(ROOT, "tests", "core_host"))
    import minimaxhost as MH

    game = BatchedChessEnv(rows, device=0, seed=11)
    game.step_random(plies0)  # mid-game boards (finished games restart)
    game.synchronize()
    boards, metas = game.boards()
    done = game.outputs()["done"].astype(bool)
    po = game.playouts(rows, playouts=P, max_plies=PLAYOUT_PLIES)
    out = game.minimax_buffer(rows)
    eng = Engine(0)

    def window(call, n):
        game.record_event(0)
        for _ in range(n):
            call()
        game.record_event(1)
        game.synchronize()
        return game.elapsed_ms(0, 1) * 1000.0 / n

    def wall(call, n):
        t = time.perf_counter()
        for _ in range(n):
            call()
        return (time.perf_counter() - t) * 1e6 / n

    res = dict(rows=rows, live_rows=int((~done).sum()), depths={})
    for d in DEPTHS:
        draw = [0]

        def run_playouts():
            po.run(plies=PLAYOUT_PLIES, draw=draw[0])
            draw[0] += PLAYOUT_PLIES

        legs = (("minimax_us", lambda: game.minimax(depth=d, out=out), window, LAUNCHES[d]),
                ("playout_us", run_playouts, window, LAUNCHES[1]),
                ("perft_us", lambda: eng.perft(boards, metas, d), wall, PERFT_CALLS),
                ("perft_next_us", lambda: eng.perft(boards, metas, d + 1), wall, PERFT_CALLS))
        for _, call, _, _ in legs:
            for _ in range(WARMUP):
                call()
            game.synchronize()
        times = {k: [] for k, _, _, _ in legs}
        for _ in range(REPS):
            for k, call, clock, n in legs:
                times[k].append(clock(call, n))
        rec = {k: spread(v) for k, v in times.items()}
        nodes = int(game.minimax(depth=d, out=out, nodes=True).fetch("nodes")["nodes"].astype(np.int64).sum())
        per_row = out.fetch("nodes")["nodes"]
        rec["nodes"] = nodes
        rec["nodes_row_max"] = int(per_row.max())
        rec["nodes_per_s"] = round(nodes / (rec["minimax_us"]["median"] * 1e-6))
        for k, dd in (("perft", d), ("perft_next", d + 1)):
            leaves = int(eng.perft(boards, metas, dd).astype(np.float64).sum())
            rec[k + "_leaves"] = leaves
            rec[k + "_leaves_per_s"] = round(leaves / (rec[k + "_us"]["median"] * 1e-6))
        n = min(rows, HOST_ROWS)
        t = time.perf_counter()
        host = MH.run(boards, metas, np.arange(n), d, done=done)
        dt = time.perf_counter() - t
        assert (host["nodes"] == per_row[:n]).all() and (host["score"] == out.fetch("score")["score"][:n]).all()
        rec["host_rows"] = n
        rec["host_nodes"] = int(host["nodes"].astype(np.int64).sum())
        if d < 4:  # the same rows without pruning (a minute of one core at depth 4)
            full = MH.run(boards, metas, np.arange(n), d, done=done, prune=False)
            rec["host_nodes_full_width"] = int(full["nodes"].astype(np.int64).sum())
        rec["host_nodes_per_s_one_core"] = round(rec["host_nodes"] / dt)
        res["depths"][str(d)] = rec
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plies", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0, help="(internal) the row count this process measures")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.plies)
        return
    shapes = []
    for rows in ROWS:  # a fresh process, so a fresh HIP context, per row count
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(rows), "--plies",
                            str(args.plies)], check=True, capture_output=True, text=True, timeout=420)
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = dict(tool="tools/minimax_bench.py",
               unit="us per call: median [min, max] over windows; device events, perft legs host wall time",
               warmup=WARMUP, launches_per_window=LAUNCHES, perft_calls_per_window=PERFT_CALLS, windows=REPS,
               start_plies=args.plies, tiebreak="first", lists="off", playouts=P, playout_plies=PLAYOUT_PLIES,
               shapes=shapes)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
