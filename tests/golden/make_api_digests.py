"""Generate tests/golden/api_digests_<case>.npz (one file per case): the oracle's per-board digests
of 16 347 boards x 2 000 steps of the device API step's loop, for opponent "none" and the random
opponent with a WHITE and with a BLACK agent.

The loop (oracle/gc_oracle.c oracle_api_digests, restated in tests/test_api_digest.py): every
board feeds the auto-reset step its previous pick, one step in 16 an arbitrary action and one in
16 a near miss of the pick (same piece, another target); a board left without a legal move is
reset as the host reset does, so no step is spent on it.  Each digest folds every step's action,
reward, done, reason, pick and count, every 100th step's mask words and observation, and the
final state; a snapshot of it is kept every 500 steps.  16 347 = 127 x 128 + 91: a partial last
workgroup and a partial last wave of the quad kernels, and a padded default mask stride.

Each file: snap uint64[4][boards], final uint64[boards], boards, steps, seed, reasons int64[16]
(steps by reason code) and the counters of oracle.API_STAT_NAMES.  The coverage conditions that
tests/test_api_digest.py reads from them are asserted here too.

    python tests/golden/make_api_digests.py [--threads 8]     (~1-2 min per case on 8 cores)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

OUT = os.path.join(ROOT, "tests", "golden", "api_digests_{}.npz")
BOARDS = 16347
STEPS = 2000
MASK_EVERY = 100
SNAP_EVERY = 500
# (name, seed, opponent, agent colour)
CASES = (("none", 780001, 0, "WHITE"), ("random_white", 780002, 1, "WHITE"), ("random_black", 780003, 1, "BLACK"))
# reason codes every case / only some cases must reach (gc_oracle.c o_env_step; 5 = both kings checked)
REASONS = {"none": (0, 1, 2, 3, 5, 6), "random_white": (0, 1, 2, 3, 5, 6, 8, 9), "random_black": (0, 1, 2, 5, 6, 8, 9)}


def coverage_gaps(name, stats):
    """the coverage conditions a case's statistics miss (empty = all hold)"""
    gaps = [f"reason {r} never occurs" for r in REASONS[name] if stats["reasons"][r] == 0]
    for cls in ("arbitrary", "near_miss"):
        fed, acc = int(stats[cls]), int(stats[cls + "_accepted"])
        if acc == 0:
            gaps.append(f"no {cls} action accepted")
        if fed - acc == 0:
            gaps.append(f"no {cls} action refused")
    if int(stats["stuck_resets"]) == 0:
        gaps.append("no stuck reset")
    if int(stats["stuck_steps"]) != 0:
        gaps.append(f"{int(stats['stuck_steps'])} steps fed to a board with no legal move")
    return gaps


def main():
    import oracle as O

    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=os.cpu_count() or 1)
    a = ap.parse_args()
    O.build()
    for name, seed, opp, color in CASES:
        t0 = time.time()
        snap, final, st = O.api_digests(seed, BOARDS, STEPS, opponent=opp, agent_white=color == "WHITE",
                                        threads=a.threads, mask_every=MASK_EVERY, snap_every=SNAP_EVERY)
        print(f"{name}: {BOARDS} boards x {STEPS} steps, {time.time() - t0:.0f} s", flush=True)
        print("  reasons", {r: int(c) for r, c in enumerate(st["reasons"]) if c}, flush=True)
        print("  " + ", ".join(f"{k} {st[k]}" for k in O.API_STAT_NAMES), flush=True)
        print(f"  near misses legal: {st['near_miss_accepted'] / st['near_miss']:.4f} "
              f"({st['near_miss_changed_accepted']} of them another action than the pick), "
              f"arbitrary legal: {st['arbitrary_accepted'] / st['arbitrary']:.4f}", flush=True)
        gaps = coverage_gaps(name, st)
        assert not gaps, (name, gaps)
        np.savez(OUT.format(name), snap=snap, final=final, boards=np.int64(BOARDS), steps=np.int64(STEPS),
                 seed=np.int64(seed), reasons=st["reasons"], **{k: np.int64(st[k]) for k in O.API_STAT_NAMES})
        print("wrote", OUT.format(name))


if __name__ == "__main__":
    main()
