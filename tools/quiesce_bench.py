"""Measurement: gc_env_minimax_q (minimax with a quiescence search at the leaves, gc_minimax.h)
against quiesce=0 of the same depth -- the plain search on the plain kernels -- on the same boards in
the same process:

    us          one minimax call (tiebreak first, lists off, nodes off), device events
    base_us     the same depth at quiesce=0, its windows alternated with the leg's
    nodes       the positions one call visits (its nodes output, summed over the rows), and the
                largest row: the wave of that row is the call's critical path

Shapes: rows in {64, 1024}, depth in {1, 2}, quiesce in {0, 1, 2, 4}; the boards are `--plies` (40)
random plies into self-play (tools/minimax_bench.py's boards: the same seed).  One child process per
(rows, depth, quiesce) (a fresh HIP context each); in a child a warm-up of both legs, then REPS
windows per leg, alternated so that drift of the machine falls on both.  A window holds as many
calls as fit WINDOW_MS by the warm-up's own timing, between 1 and LAUNCHES (a quiesce=4 call at
depth 2 takes 0.4 s: fixed 50-call windows would run for minutes), recorded per leg; times are
us per CALL, reported as median [min, max] over the windows.  Every child also checks its first
rows against the host build of the same search.  Prints one JSON line; --out also writes it.

    python tools/quiesce_bench.py [--out profiles/quiesce.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-chess_amd"))

WARMUP, REPS, LAUNCHES, WINDOW_MS = 3, 5, 50, 100.0
CHILD_TIMEOUT = 180  # s; a child's GPU work is bounded by (WARMUP + REPS windows) of WINDOW_MS or of one call each
ROWS, DEPTHS, QUIESCE, HOST_ROWS = (1024, 64), (1, 2), (0, 1, 2, 4), 32


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 2), min=round(float(v.min()), 2), max=round(float(v.max()), 2))


def child(rows, depth, quiesce, plies0):
    from gym_chess_amd.env import BatchedChessEnv

    sys.path.insert(0, os.path.join(ROOT, "tests", "core_host"))
    import quiescehost as QH

    game = BatchedChessEnv(rows, device=0, seed=11)
    game.step_random(plies0)  # mid-game boards (finished games restart)
    game.synchronize()
    boards, metas = game.boards()
    done = game.outputs()["done"].astype(bool)
    out = game.minimax_buffer(rows)

    def window(q, n):
        game.record_event(0)
        for _ in range(n):
            game.minimax(depth=depth, quiesce=q, out=out)
        game.record_event(1)
        game.synchronize()
        return game.elapsed_ms(0, 1) * 1000.0 / n

    launches = {}
    for q in (quiesce, 0):
        us = window(q, WARMUP)  # the warm-up, timed: it sizes the windows
        launches[q] = int(min(LAUNCHES, max(1, WINDOW_MS * 1000.0 / us)))
    times = {"us": [], "base_us": []}
    for _ in range(REPS):
        times["us"].append(window(quiesce, launches[quiesce]))
        times["base_us"].append(window(0, launches[0]))
    rec = dict(rows=rows, live_rows=int((~done).sum()), depth=depth, quiesce=quiesce,
               launches_per_window=launches[quiesce], base_launches_per_window=launches[0])
    rec.update({k: spread(v) for k, v in times.items()})
    rec["ratio_to_base"] = round(rec["us"]["median"] / rec["base_us"]["median"], 2)
    got = game.minimax(depth=depth, quiesce=quiesce, out=out, nodes=True).fetch()
    per_row = got["nodes"].astype(np.int64)
    rec["nodes"], rec["nodes_row_max"] = int(per_row.sum()), int(per_row.max())
    rec["nodes_per_s"] = round(rec["nodes"] / (rec["us"]["median"] * 1e-6))
    base = game.minimax(depth=depth, quiesce=0, out=out, nodes=True).fetch()
    rec["base_nodes"] = int(base["nodes"].astype(np.int64).sum())
    rec["rows_whose_pick_differs_from_base"] = int((base["pick"] != got["pick"]).sum())
    n = min(rows, HOST_ROWS)
    host = QH.run(boards, metas, np.arange(n), depth, quiesce=quiesce, done=done)
    assert all((host[k] == got[k][:n]).all() for k in ("nodes", "score", "pick", "count"))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plies", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(internal) rows,depth,quiesce this process measures")
    args = ap.parse_args()
    if args.child:
        child(*(int(x) for x in args.child.split(",")), args.plies)
        return
    runs = []
    for rows in ROWS:
        for depth in DEPTHS:
            for q in QUIESCE:  # a fresh process, so a fresh HIP context, per configuration
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{rows},{depth},{q}", "--plies",
                                    str(args.plies)], check=True, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
                runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    res = dict(tool="tools/quiesce_bench.py", unit="us per call: median [min, max] over windows; device events",
               warmup=WARMUP, max_launches_per_window=LAUNCHES, window_ms=WINDOW_MS, windows=REPS, start_plies=args.plies, tiebreak="first",
               lists="off", runs=runs)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
