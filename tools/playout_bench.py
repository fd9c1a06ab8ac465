"""Measurement: gc_playout_run (random-playout leaf values, gc_playout.h) beside what a user had
before it at the same lane count and plies -- step_random(n_plies) and rollout_device(n_plies) on
a scratch env of rows * P boards.  Both are LOWER bounds on the earlier formulation: the clone of
every leaf into the scratch env and the reduction of the trace are left out.

Shapes: rows in {1024, 64}, P = 8, n_plies in {16, 32, 64}; the boards are `--plies` (40) random
plies into self-play.  One child process per row count (a fresh HIP context each); in a child,
per n_plies, a warm-up of every leg, then REPS windows of LAUNCHES calls per leg, the legs
alternated so that drift of the machine falls on all of them; times are us per CALL from device
events on the stream the call runs on, reported as median [min, max] over the windows.
plies_per_s = the playouts' plies actually played in one call (tally column 5) over its median
time.  Prints one JSON line; --out also writes it to a file.

    python tools/playout_bench.py [--out profiles/playout.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-chess_amd"))

WARMUP, LAUNCHES, REPS = 10, 100, 5
ROWS, P, PLIES = (1024, 64), 8, (16, 32, 64)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 2), min=round(float(v.min()), 2), max=round(float(v.max()), 2))


def child(rows, plies0):
    from gym_chess_amd.env import BatchedChessEnv

    game = BatchedChessEnv(rows, device=0, seed=11)
    game.step_random(plies0)  # mid-game boards (finished games restart)
    game.synchronize()
    po = game.playouts(rows, playouts=P, max_plies=max(PLIES))
    scratch = BatchedChessEnv(rows * P, device=0, seed=12)  # today's formulation: a board per playout
    scratch.clone_boards(game, np.repeat(np.arange(rows), P), np.arange(rows * P))
    scratch.select_random()
    scratch.synchronize()

    def window(env, call):
        env.record_event(0)
        for _ in range(LAUNCHES):
            call()
        env.record_event(1)
        env.synchronize()
        return env.elapsed_ms(0, 1) * 1000.0 / LAUNCHES

    out = dict(rows=rows, playouts=P, lanes=rows * P, playout_device_bytes=po.device_bytes(), scratch_env_device_bytes=scratch.device_bytes(), plies={})
    for n in PLIES:
        draw = [0]

        def run_playouts():
            po.run(plies=n, draw=draw[0])
            draw[0] += n

        legs = (("playout_us", game, run_playouts), ("step_random_us", scratch, lambda: scratch.step_random(n)),
                ("rollout_device_us", scratch, lambda: scratch.rollout_device(n)))
        for _, env, call in legs:
            for _ in range(WARMUP):
                call()
            env.synchronize()
        times = {k: [] for k, _, _ in legs}
        for _ in range(REPS):
            for k, env, call in legs:
                times[k].append(window(env, call))
        rec = {k: spread(v) for k, v in times.items()}
        played = int(po.run(plies=n, draw=0).fetch()["tally"][:, 5].sum())
        rec["plies_played_per_call"] = played
        rec["plies_per_s"] = round(played / (rec["playout_us"]["median"] * 1e-6))
        out["plies"][str(n)] = rec
    print(json.dumps(out))


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
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(rows), "--plies", str(args.plies)],
                           check=True, capture_output=True, text=True, timeout=600)
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = dict(tool="tools/playout_bench.py", unit="us per call, device events: median [min, max] over windows",
               warmup=WARMUP, launches_per_window=LAUNCHES, windows=REPS, start_plies=args.plies, shapes=shapes)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
