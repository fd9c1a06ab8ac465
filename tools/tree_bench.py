"""Measurement: the device search tree (gc_tree_select + gc_tree_backup) per simulation as the trees
fill, against a straightforward torch implementation of the same select / backup.

G = 1 024 games, 256 nodes, cap = 64, synthetic child lists (8..40 children, random priors, values
in [-1, 1], 3 % terminal leaves) -- no chess: the tree kernels see only priors blocks.  Two
settings of the search: "broad" (c_puct 1.25, fpu 0: shallow trees) and "deep" (c_puct 1.25, fpu
-1: the descent follows visited children).  Per setting the trees grow over SIMS simulations; the
us per simulation (select + backup, device events on the env's stream around a window of
simulations issued without a host synchronisation) is taken in an early window (simulations
8..40) and a late one (the last 48), with the mean and the largest path length at the end of each
window; every time is the median of REPS runs after a warm-up run (the per-run values beside it).
last_select_us / last_backup_us split one simulation on the final trees by events around each
call (these carry the gaps of the extra event records and are a guide only).

If torch imports and sees the GPU, a child process runs the same simulations on the same inputs
with the tree as [G][nodes][cap] tensors: per level a gather of the node's rows, the score, an
argmax and a test whether any game descends further; the backup is a masked scatter along the
stored paths.  Its windows are timed the same way.  agree = the fraction of games whose root visit
counts equal the device's at the end.

--advance measures gc_tree_advance instead (the played move's subtree kept across moves): per
setting the trees grow over nodes - 1 simulations, root_policy picks greedily and the trees advance
on that pick.  advance_us and reset_us (a gc_tree_reset of the same trees) are medians of REPS runs
after a warm-up, by events on the env's stream around the call; kept_mean / kept_max are the kept
subtrees' sizes, retained_visits_mean the mean of the new roots' visit sums (what the next search
starts with), tree_us_per_sim the mean select + backup time over the same run's simulations, and
saved_us_lower_bound = retained_visits_mean * tree_us_per_sim (the tree's share alone of
re-searching the retained visits; the network's time comes on top).  The tree env's boards all
stand at the start position, whose 3-fold window is empty: the board move copies the per-board
fields only, a window costs what tools/clone_bench.py measures per pair.

--leaves measures the batched calls (gc_tree_select_batch + gc_tree_backup_batch: K leaves per game
per call, virtual loss 1) on the same synthetic inputs, for G in {32, 1 024} games and K in {1, 4, 8,
16}, nodes and cap as above.  Per G, setting and K the trees grow from the root over nodes / K
calls (nodes descents, as the single-leaf run's nodes simulations) and two windows of calls are
timed by events on the env's stream, issued without a host synchronisation: early (the calls
covering descents 8..40, two calls at least) and late (the calls covering the last 48 descents, two
at least).  us_per_call, us_per_leaf = us_per_call / K, collisions_per_call (per game: the mean over
the games of the collisions counter's growth across the window, per call) and new_nodes_per_call
(per game) are recorded, medians of REPS_LEAVES runs after a warm-up.  "single" is the single-leaf
pair (gc_tree_select + gc_tree_backup) in the same process, on the same env, inputs and geometry,
windows 8..40 and the last 48 simulations: us_per_sim.  The trees of a window are those each
search grew by then -- a batch and K single simulations do not expand the same nodes.  Two ratios
are derived per G, setting and window: k1_over_single (one K = 1 call against one single
simulation: the same work plus the in-flight traffic) and k8_over_8_single (one K = 8 call against
eight single simulations).

--solver measures what the solver (gc_tree_solver_enable) costs the single-leaf pair, per
simulation, on the search measurement's shapes, inputs and windows, three ways: "parent" (another
checkout of this project, normally the parent commit, given by --parent-root and built there),
"off" (this checkout, a tree that never enabled the solver) and "on" (this checkout, solver=True).
Each leg runs in a child process of its own (two builds of the library cannot share one), and the
legs alternate -- parent, off, on, SOLVER_ROUNDS times -- so that drift of the box falls on all
three; a child warms up with one run and times REPS runs.  Per leg, setting and window: every
window's us_per_sim, their median, min and max.  off_within_parent_spread says whether the median
of "off" lies inside [min, max] of the parent's own windows (it is meant to be the same code);
on_over_off is the ratio of the medians, reported only.  same_visits: the roots' visit counts of
"off" equal the parent's (a digest), so the same code also computed the same thing.  For "on" the
proven nodes, the proven roots and the mean path length at the end of each window are recorded
(with the bench's 3 % terminal leaves and 8..40 moves per node few proofs climb: the cost measured
is the extra row per level and the propagation's first step).

--gumbel measures Gumbel root search (gc_tree_gumbel_*), cap 64, 16 considered moves, for G in {1 024,
32} games and sims in {16, 64}, in a child process per round.  Per G and sims: "search" = a whole
search from the root, us per simulation (select + backup, one window of `sims` simulations by
events on the env's stream, no host synchronisation inside), armed (reset, gumbel_begin, the
simulations) against a plain PUCT search of as many simulations on a tree without the mode -- the
two grow different trees.  "same_trees" = the armed search's final trees copied into both handles
(the armed one and the plain one, through the host), then a window of GUMBEL_WINDOW further
simulations on each: the backup is the same kernel on the same kind of path, so armed - plain is
what the Gumbel rule adds to a select; the copy is repeated before every timed window.  begin_us /
policy_us: events around one call, medians of 20.  Every figure is the median over the rounds'
windows, with min and max.  The same rounds also time the plain single-leaf pair of a tree without
the mode on the search measurement's shapes ("parent": another checkout, normally the parent
commit, given by --parent-root and built there; "off": this checkout), alternating, exactly as
--solver does: off_within_parent_spread says whether this checkout's median lies inside [min,
max] of the parent's own windows, same_visits that both computed the same root visits.

    python tools/tree_bench.py [--games G] [--nodes N] [--out profiles/tree_search.json]
    python tools/tree_bench.py --advance [--out profiles/tree_advance.json]
    python tools/tree_bench.py --leaves [--out profiles/tree_batch.json]
    python tools/tree_bench.py --solver --parent-root DIR [--out profiles/tree_solver.json]
    python tools/tree_bench.py --gumbel --parent-root DIR [--out profiles/tree_gumbel.json]
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

CAP = 64
SETTINGS = {"broad": (1.25, 0.0), "deep": (1.25, -1.0)}
EARLY = (8, 40)
LATE_LEN = 48
REPS = 3


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def make_inputs(G, sims, seed=7):
    """per simulation a priors block [G][CAP] (ascending actions, padded), values, done, reason"""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(8, 41, size=(sims + 1, G)).astype(np.int32)
    w = rng.uniform(0.05, 1.0, size=(sims + 1, G, CAP)).astype(np.float32)
    on = np.arange(CAP)[None, None, :] < cnt[:, :, None]
    w = np.where(on, w, 0)
    pri = (w / w.sum(axis=2, keepdims=True)).astype(np.float32)
    act = np.where(on, np.arange(CAP, dtype=np.uint16)[None, None, :] * 7, 0xFFFF).astype(np.uint16)
    val = rng.uniform(-1, 1, size=(sims + 1, G)).astype(np.float32)
    done = (rng.random((sims + 1, G)) < 0.03).astype(np.uint8)
    reason = np.where(done != 0, rng.integers(1, 3, size=(sims + 1, G)), 0).astype(np.uint8)
    return dict(actions=act, priors=pri, count=cnt, value=val, done=done, reason=reason)


def windows(sims):
    return {"early": EARLY, "late": (sims - LATE_LEN, sims)}


# ----------------------------------------------------------------------------- the torch leg
def torch_leg(path, G, nodes, sims):
    import torch

    if not torch.cuda.is_available():
        print(json.dumps({"torch": None}))
        return
    dev = "cuda"
    z = np.load(path)
    inp = {k: torch.from_numpy(z[k].astype(np.int32) if z[k].dtype == np.uint16 else z[k]).to(dev) for k in
           ("actions", "priors", "count", "value", "done", "reason")}
    ar = torch.arange(G, device=dev)
    slots = torch.arange(CAP, device=dev)[None, :]
    levels = torch.arange(nodes, device=dev)[None, :]
    out = {"torch": torch.__version__}
    for name, (c_puct, fpu) in SETTINGS.items():
        action = torch.full((G, nodes, CAP), 0xFFFF, dtype=torch.int32, device=dev)
        prior = torch.zeros((G, nodes, CAP), device=dev)
        child = torch.full((G, nodes, CAP), -1, dtype=torch.int64, device=dev)
        ev = torch.zeros((G, nodes, CAP), dtype=torch.int32, device=dev)
        val = torch.zeros((G, nodes, CAP), device=dev)
        nch = torch.zeros((G, nodes), dtype=torch.int64, device=dev)
        leaf_value = torch.zeros((G, nodes), device=dev)
        n_nodes = torch.ones(G, dtype=torch.int64, device=dev)
        pn = torch.zeros((G, nodes), dtype=torch.int64, device=dev)
        ps = torch.zeros((G, nodes), dtype=torch.int64, device=dev)

        def make(rows, node, s, listed):
            """nodes `node` of games `rows` from block s"""
            m = torch.where(listed, inp["count"][s][rows].clamp(0, CAP).long(), 0)
            keep = slots < m[:, None]
            action[rows, node] = torch.where(keep, inp["actions"][s][rows], 0xFFFF)
            prior[rows, node] = torch.where(keep, inp["priors"][s][rows], 0.0)
            child[rows, node] = -1
            ev[rows, node] = 0
            val[rows, node] = 0.0
            nch[rows, node] = m

        make(ar, torch.zeros(G, dtype=torch.int64, device=dev), sims, torch.ones(G, dtype=torch.bool, device=dev))

        def select():
            k = torch.zeros(G, dtype=torch.int64, device=dev)
            D = torch.zeros(G, dtype=torch.int64, device=dev)
            live = torch.ones(G, dtype=torch.bool, device=dev)
            new = torch.zeros(G, dtype=torch.bool, device=dev)
            while True:
                e, v, p, nc = ev[ar, k], val[ar, k], prior[ar, k], nch[ar, k]
                n_k = (1 + e.sum(1)).float()
                q = torch.where(e > 0, v / e.clamp(min=1), fpu)
                score = q + c_puct * p * n_k.sqrt()[:, None] / (1 + e)
                j = score.masked_fill(slots >= nc[:, None], float("-inf")).argmax(1)
                has = live & (nc > 0)
                pn[ar, D] = torch.where(has, k, pn[ar, D])
                ps[ar, D] = torch.where(has, j, ps[ar, D])
                D = D + has
                ch = child[ar, k, j]
                down = has & (ch >= 0)
                ends = has & ~down
                room = n_nodes < nodes
                new = new | (ends & room)
                D = D - (ends & ~room).long()  # a full tree: the path ends at k
                k = torch.where(down, ch, k)
                live = down
                if not bool(down.any()):
                    break
            leaf = torch.where(new, n_nodes, k)
            n_nodes.add_(new.long())
            return D, leaf, new

        def backup(D, leaf, new, s):
            rows = ar[new]
            L = leaf[new]
            fin = inp["done"][s][rows] != 0
            make(rows, L, s, ~fin)
            last = (D[new] - 1).clamp(min=0)
            child[rows, pn[rows, last], ps[rows, last]] = L
            leaf_value[rows, L] = torch.where(fin, torch.where(inp["reason"][s][rows] == 1, -1.0, 0.0),
                                              inp["value"][s][rows])
            v = leaf_value[ar, leaf]
            on = levels < D[:, None]
            sign = torch.where(((D[:, None] - levels) & 1) == 1, -v[:, None], v[:, None])
            flat = ((ar[:, None] * nodes + pn) * CAP + ps)[on]
            ev.view(-1).index_add_(0, flat, torch.ones_like(flat, dtype=torch.int32))
            val.view(-1).index_add_(0, flat, sign[on])

        res, marks = {}, {a: w for w, (a, b) in windows(sims).items()}
        ends = {b: w for w, (a, b) in windows(sims).items()}
        t0 = {}
        for s in range(sims):
            if s in marks:
                torch.cuda.synchronize()
                t0[marks[s]] = torch.cuda.Event(enable_timing=True)
                t0[marks[s]].record()
            D, leaf, new = select()
            backup(D, leaf, new, s)
            if s + 1 in ends:
                w = ends[s + 1]
                t1 = torch.cuda.Event(enable_timing=True)
                t1.record()
                torch.cuda.synchronize()
                a, b = windows(sims)[w]
                res[w] = {"torch_us_per_sim": round(t0[w].elapsed_time(t1) * 1e3 / (b - a), 2),
                          "torch_mean_depth": round(float(D.float().mean()), 2)}
        agree = (ev[:, 0].cpu().numpy() == z["root_visits_" + name]).all(axis=1).mean()
        res["agree"] = round(float(agree), 4)
        out[name] = res
    print(json.dumps(out))


# ----------------------------------------------------------------------------- advance
def advance_leg(G, nodes, out_path):
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    sims = nodes - 1
    env = BatchedChessEnv(G * nodes, device=0, seed=11)
    L = env._L
    inp = make_inputs(G, sims + 1)

    def upload(a):
        v = ctypes.c_void_p()
        _lib.check(L.gc_device_alloc(env.device, ctypes.c_uint64(a.nbytes), ctypes.byref(v)))
        _lib.check(L.gc_env_copy(env._h, v.value, _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))
        return v.value

    d = {k: upload(np.ascontiguousarray(v)) for k, v in inp.items()}
    tree = env.search_tree(G, nodes, cap=CAP)
    sel, adv = tree._sel.ptr, tree._adv.ptr
    res = {"games": G, "nodes": nodes, "cap": CAP, "sims": sims, "reps": REPS}

    def block(s):
        return (d["actions"] + 2 * G * CAP * s, d["priors"] + 4 * G * CAP * s, d["count"] + 4 * G * s, CAP)

    for name, (c_puct, fpu) in SETTINGS.items():
        t_adv, t_reset, t_sim = [], [], []
        out = {}
        for rep in range(REPS + 1):  # the first run warms up; the trees are the same every run
            _lib.check(L.gc_tree_reset(tree._h, *block(sims), None))
            env.synchronize()
            env.record_event(0)
            for s in range(sims):
                _lib.check(L.gc_tree_select(tree._h, c_puct, fpu, sel["parent"], sel["child"], sel["action"]))
                _lib.check(L.gc_tree_backup(tree._h, d["value"] + 4 * G * s, d["done"] + G * s, d["reason"] + G * s,
                                            *block(s)))
            env.record_event(1)
            pick = tree.root_policy(greedy=True).pick
            env.synchronize()
            nodes_before = tree.fetch("n_nodes")["n_nodes"]
            env.record_event(2)
            _lib.check(L.gc_tree_advance(tree._h, pick, *block(sims + 1), None, adv["kept"], adv["remap"]))
            env.record_event(3)
            env.synchronize()
            kept = tree._adv.fetch("kept")["kept"]
            retained = tree.fetch("edge_visits")["edge_visits"][:, 0].sum(axis=1)
            env.record_event(4)
            _lib.check(L.gc_tree_reset(tree._h, *block(sims), None))
            env.record_event(5)
            env.synchronize()
            if rep:
                t_sim.append(env.elapsed_ms(0, 1) * 1e3 / sims)
                t_adv.append(env.elapsed_ms(2, 3) * 1e3)
                t_reset.append(env.elapsed_ms(4, 5) * 1e3)
            out = {"nodes_before_mean": round(float(nodes_before.mean()), 1),
                   "kept_mean": round(float(kept.mean()), 2), "kept_max": int(kept.max()),
                   "fresh_games": int((kept == 0).sum()),
                   "retained_visits_mean": round(float(retained.mean()), 2)}
        out.update({"advance_us": round(median(t_adv), 2), "advance_us_reps": [round(x, 2) for x in t_adv],
                    "reset_us": round(median(t_reset), 2), "reset_us_reps": [round(x, 2) for x in t_reset],
                    "tree_us_per_sim": round(median(t_sim), 2)})
        out["advance_minus_reset_us"] = round(out["advance_us"] - out["reset_us"], 2)
        out["saved_us_lower_bound"] = round(out["retained_visits_mean"] * out["tree_us_per_sim"], 1)
        res[name] = out
    env.synchronize()
    tree.close()
    for p in d.values():
        L.gc_device_free(env.device, ctypes.c_void_p(p))
    env.close()
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


# ----------------------------------------------------------------------------- several leaves per call
LEAVES_GAMES = (32, 1024)
LEAVES_K = (1, 4, 8, 16)
REPS_LEAVES = 5
VLOSS = 1.0


def leaves_windows(nodes, K):
    """the calls that cover descents 8..40 and the last 48 descents, two calls each at least"""
    calls = nodes // K
    a = max(1, EARLY[0] // K)
    n_early, n_late = max(2, (EARLY[1] - EARLY[0]) // K), max(2, LATE_LEN // K)
    return {"early": (a, a + n_early), "late": (calls - n_late, calls)}


def leaves_leg(nodes, out_path):
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    res = {"nodes": nodes, "cap": CAP, "vloss": VLOSS, "reps": REPS_LEAVES, "settings": SETTINGS, "runs": []}
    for G in LEAVES_GAMES:
        env = BatchedChessEnv(G * nodes, device=0, seed=11)
        L = env._L
        tree = env.search_tree(G, nodes, cap=CAP)
        sel = tree._sel.ptr

        def upload(a):
            v = ctypes.c_void_p()
            _lib.check(L.gc_device_alloc(env.device, ctypes.c_uint64(a.nbytes), ctypes.byref(v)))
            _lib.check(L.gc_env_copy(env._h, v.value, _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))
            return v.value

        def timed(rows, calls, wins, d, step, counters):
            """REPS_LEAVES + 1 runs of `calls` calls from the root; per window the times per call and
            the counters' growth per call (mean over the games)"""
            def block(s):
                return (d["actions"] + 2 * rows * CAP * s, d["priors"] + 4 * rows * CAP * s, d["count"] + 4 * rows * s, CAP)

            starts = {a: w for w, (a, b) in wins.items()}
            ends = {b: w for w, (a, b) in wins.items()}
            times = {w: [] for w in wins}
            grow = {}
            for rep in range(REPS_LEAVES + 1):  # the first run warms up; the trees are the same every run
                _lib.check(L.gc_tree_reset(tree._h, *block(calls), None))
                for s in range(calls):
                    if s in starts:
                        env.synchronize()
                        c0 = tree.fetch(*counters)
                        env.record_event(4)
                    step(s, block(s))
                    if s + 1 in ends:
                        w = ends[s + 1]
                        env.record_event(5)
                        env.synchronize()
                        a, b = wins[w]
                        if rep:
                            times[w].append(env.elapsed_ms(4, 5) * 1e3 / (b - a))
                        c1 = tree.fetch(*counters)
                        grow[w] = {k: round(float((c1[k] - c0[k]).mean()) / (b - a), 3) for k in counters}
            return times, grow

        for name, (c_puct, fpu) in SETTINGS.items():
            # the single-leaf pair: nodes simulations, the windows of the search measurement
            d = {k: upload(np.ascontiguousarray(v)) for k, v in make_inputs(G, nodes).items()}

            def single(s, blk):
                _lib.check(L.gc_tree_select(tree._h, c_puct, fpu, sel["parent"], sel["child"], sel["action"]))
                _lib.check(L.gc_tree_backup(tree._h, d["value"] + 4 * G * s, d["done"] + G * s, d["reason"] + G * s, *blk))

            times, grow = timed(G, nodes, windows(nodes), d, single, ("n_nodes",))
            one = {w: {"us_per_sim": round(median(t), 2), "us_per_sim_reps": [round(x, 2) for x in t],
                       "new_nodes_per_sim": grow[w]["n_nodes"]} for w, t in times.items()}
            env.synchronize()
            for ptr in d.values():
                L.gc_device_free(env.device, ctypes.c_void_p(ptr))
            run = {"games": G, "setting": name, "windows_single": {w: list(ab) for w, ab in windows(nodes).items()},
                   "single": one, "batch": {}}
            for K in LEAVES_K:
                rows, calls = G * K, nodes // K
                tree.reserve_batch(K)
                b = tree._bsel.ptr
                d = {k: upload(np.ascontiguousarray(v)) for k, v in make_inputs(rows, calls).items()}

                def batch(s, blk):
                    _lib.check(L.gc_tree_select_batch(tree._h, K, c_puct, fpu, VLOSS, b["parent"], b["child"], b["action"]))
                    _lib.check(L.gc_tree_backup_batch(tree._h, d["value"] + 4 * rows * s, d["done"] + rows * s,
                                                      d["reason"] + rows * s, *blk))

                wins = leaves_windows(nodes, K)
                times, grow = timed(rows, calls, wins, d, batch, ("n_nodes", "collisions"))
                out = {"calls": calls, "windows": {w: list(ab) for w, ab in wins.items()}}
                for w, t in times.items():
                    us = median(t)
                    out[w] = {"us_per_call": round(us, 2), "us_per_leaf": round(us / K, 2),
                              "us_per_call_reps": [round(x, 2) for x in t],
                              "collisions_per_call": grow[w]["collisions"], "new_nodes_per_call": grow[w]["n_nodes"],
                              "single_us_for_K_sims": round(K * one[w]["us_per_sim"], 2),
                              "call_over_K_single": round(us / (K * one[w]["us_per_sim"]), 3)}
                run["batch"][str(K)] = out
                env.synchronize()
                for ptr in d.values():
                    L.gc_device_free(env.device, ctypes.c_void_p(ptr))
            run["k1_over_single"] = {w: run["batch"]["1"][w]["call_over_K_single"] for w in ("early", "late")}
            run["k8_over_8_single"] = {w: run["batch"]["8"][w]["call_over_K_single"] for w in ("early", "late")}
            run["tree_bytes"] = tree.device_bytes()
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
        env.synchronize()
        tree.close()
        env.close()
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


# ----------------------------------------------------------------------------- the solver
SOLVER_ROUNDS = 5


def solver_child(G, nodes, solver):
    """one leg in this process: the search measurement's loop on a tree with the solver on or off"""
    import hashlib

    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    sims = nodes
    env = BatchedChessEnv(G * nodes, device=0, seed=11)
    L = env._L
    inp = make_inputs(G, sims)

    def upload(a):
        v = ctypes.c_void_p()
        _lib.check(L.gc_device_alloc(env.device, ctypes.c_uint64(a.nbytes), ctypes.byref(v)))
        _lib.check(L.gc_env_copy(env._h, v.value, _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))
        return v.value

    d = {k: upload(np.ascontiguousarray(v)) for k, v in inp.items()}
    tree = env.search_tree(G, nodes, cap=CAP, solver=True) if solver else env.search_tree(G, nodes, cap=CAP)
    sel = tree._sel.ptr
    res = {"tree_bytes": tree.device_bytes()}

    def block(s):
        return (d["actions"] + 2 * G * CAP * s, d["priors"] + 4 * G * CAP * s, d["count"] + 4 * G * s, CAP)

    wins = windows(sims)
    starts = {a: w for w, (a, b) in wins.items()}
    ends = {b: w for w, (a, b) in wins.items()}
    for name, (c_puct, fpu) in SETTINGS.items():
        times = {w: [] for w in wins}
        out = {}
        for rep in range(REPS + 1):  # the first run warms up; the trees and so the work are the same every run
            _lib.check(L.gc_tree_reset(tree._h, *block(sims), None))
            for s in range(sims):
                if s in starts:
                    env.synchronize()
                    env.record_event(4)
                _lib.check(L.gc_tree_select(tree._h, c_puct, fpu, sel["parent"], sel["child"], sel["action"]))
                _lib.check(L.gc_tree_backup(tree._h, d["value"] + 4 * G * s, d["done"] + G * s, d["reason"] + G * s,
                                            *block(s)))
                if s + 1 in ends:
                    w = ends[s + 1]
                    env.record_event(5)
                    env.synchronize()
                    a, b = wins[w]
                    if rep:
                        times[w].append(env.elapsed_ms(4, 5) * 1e3 / (b - a))
                    dep = tree.fetch("depth", "n_nodes")
                    out[w] = {"mean_depth": round(float(dep["depth"].mean()), 2),
                              "mean_nodes": round(float(dep["n_nodes"].mean()), 1)}
                    if solver:
                        pr = tree.fetch("node_proven")["node_proven"]
                        live = np.arange(nodes)[None, :] < dep["n_nodes"][:, None]
                        out[w]["proven_nodes_per_game"] = round(float(((pr != 0) & live).sum()) / G, 2)
                        out[w]["proven_roots"] = int((pr[:, 0] != 0).sum())
        for w, t in times.items():
            out[w]["us_per_sim_reps"] = [round(x, 3) for x in t]
        out["root_visits_sha"] = hashlib.sha256(tree.fetch("edge_visits")["edge_visits"][:, 0].tobytes()).hexdigest()[:16]
        res[name] = out
    env.synchronize()
    tree.close()
    for p in d.values():
        L.gc_device_free(env.device, ctypes.c_void_p(p))
    env.close()
    print(json.dumps(res), flush=True)


def solver_leg(G, nodes, parent_root, out_path):
    legs = {"parent": ["--solver-child", "off", "--package-root", os.path.abspath(parent_root)],
            "off": ["--solver-child", "off"], "on": ["--solver-child", "on"]}
    raw = {k: [] for k in legs}
    for _ in range(SOLVER_ROUNDS):
        for leg, extra in legs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--games", str(G), "--nodes", str(nodes)] + extra,
                               capture_output=True, text=True)
            if r.returncode:
                raise SystemExit(f"the {leg} leg failed:\n{(r.stderr or r.stdout)[-2000:]}")
            raw[leg].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(leg, "done", flush=True)
    res = {"games": G, "nodes": nodes, "cap": CAP, "sims": nodes, "rounds": SOLVER_ROUNDS, "reps": REPS,
           "windows": {w: list(ab) for w, ab in windows(nodes).items()},
           "tree_bytes": {leg: raw[leg][0]["tree_bytes"] for leg in legs}}
    for name in SETTINGS:
        out = {"same_visits": len({r[name]["root_visits_sha"] for leg in ("parent", "off") for r in raw[leg]}) == 1}
        for w in windows(nodes):
            row = {}
            for leg in legs:
                t = [x for r in raw[leg] for x in r[name][w]["us_per_sim_reps"]]
                row[leg] = {"us_per_sim": round(median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3),
                            "us_per_sim_windows": t}
                row[leg].update({k: v for k, v in raw[leg][-1][name][w].items() if k != "us_per_sim_reps"})
            row["off_within_parent_spread"] = row["parent"]["min"] <= row["off"]["us_per_sim"] <= row["parent"]["max"]
            row["off_over_parent"] = round(row["off"]["us_per_sim"] / row["parent"]["us_per_sim"], 4)
            row["on_over_off"] = round(row["on"]["us_per_sim"] / row["off"]["us_per_sim"], 4)
            out[w] = row
        res[name] = out
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


# ----------------------------------------------------------------------------- Gumbel root search
GUMBEL_GAMES = (1024, 32)
GUMBEL_SIMS = (16, 64)
GUMBEL_CONSIDERED = 16
GUMBEL_WINDOW = 16
GUMBEL_ROUNDS = 5


def gumbel_child():
    """one round in this process: every (G, sims) of the Gumbel measurement"""
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    c_puct, fpu = SETTINGS["broad"]
    res = {"runs": []}
    for G in GUMBEL_GAMES:
        for sims in GUMBEL_SIMS:
            total = sims + GUMBEL_WINDOW
            nodes = total + 1
            env = BatchedChessEnv(G * nodes, device=0, seed=11)
            L = env._L
            inp = make_inputs(G, total)

            def upload(a):
                v = ctypes.c_void_p()
                _lib.check(L.gc_device_alloc(env.device, ctypes.c_uint64(a.nbytes), ctypes.byref(v)))
                _lib.check(L.gc_env_copy(env._h, v.value, _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))
                return v.value

            d = {k: upload(np.ascontiguousarray(v)) for k, v in inp.items()}
            armed = env.search_tree(G, nodes, cap=CAP)
            armed.enable_gumbel(GUMBEL_CONSIDERED, sims)
            plain = env.search_tree(G, nodes, cap=CAP)

            def block(s):
                return (d["actions"] + 2 * G * CAP * s, d["priors"] + 4 * G * CAP * s, d["count"] + 4 * G * s, CAP)

            def simulate(tree, s):
                sel = tree._sel.ptr
                _lib.check(L.gc_tree_select(tree._h, c_puct, fpu, sel["parent"], sel["child"], sel["action"]))
                _lib.check(L.gc_tree_backup(tree._h, d["value"] + 4 * G * s, d["done"] + G * s, d["reason"] + G * s,
                                            *block(s)))

            def window(tree, a, b):
                env.synchronize()
                env.record_event(4)
                for s in range(a, b):
                    simulate(tree, s)
                env.record_event(5)
                env.synchronize()
                return env.elapsed_ms(4, 5) * 1e3 / (b - a)

            t = {k: [] for k in ("search_armed", "search_plain", "same_armed", "same_plain", "begin", "policy")}
            snap = None
            for rep in range(REPS + 1):  # the first run warms up; the trees are the same every run
                _lib.check(L.gc_tree_reset(armed._h, *block(total), None))
                armed.gumbel_begin(seed=5, draw=0)
                ta = window(armed, 0, sims)
                _lib.check(L.gc_tree_reset(plain._h, *block(total), None))
                tp = window(plain, 0, sims)
                if snap is None:
                    snap = armed.fetch()
                    visits = snap["edge_visits"][:, 0].copy()
                for tree in (armed, plain):  # the armed search's trees in both handles
                    for k, a in snap.items():
                        _lib.check(L.gc_env_copy(env._h, tree.ptr[k], _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))
                sa = window(armed, sims, total)
                sp = window(plain, sims, total)
                if rep:
                    for k, x in zip(("search_armed", "search_plain", "same_armed", "same_plain"), (ta, tp, sa, sp)):
                        t[k].append(round(x, 3))
            for _ in range(20):
                env.record_event(0)
                armed.gumbel_begin(seed=5, draw=1)
                env.record_event(1)
                armed.gumbel_policy()
                env.record_event(2)
                env.synchronize()
                t["begin"].append(round(env.elapsed_ms(0, 1) * 1e3, 3))
                t["policy"].append(round(env.elapsed_ms(1, 2) * 1e3, 3))
            t["begin"], t["policy"] = [median(t["begin"])], [median(t["policy"])]
            nc = snap["n_children"][:, 0]
            res["runs"].append({"games": G, "sims": sims, "nodes": nodes, "times": t,
                                "searched_moves_mean": round(float((visits > 0).sum(axis=1).mean()), 2),
                                "root_children_mean": round(float(nc.mean()), 2),
                                "gumbel_bytes": armed.device_bytes() - plain.device_bytes()})
            env.synchronize()
            armed.close()
            plain.close()
            for ptr in d.values():
                L.gc_device_free(env.device, ctypes.c_void_p(ptr))
            env.close()
    print(json.dumps(res), flush=True)


def gumbel_leg(G, nodes, parent_root, out_path):
    me = [sys.executable, os.path.abspath(__file__)]
    plain = me + ["--games", str(G), "--nodes", str(nodes), "--solver-child", "off"]
    legs = {"parent": plain + ["--package-root", os.path.abspath(parent_root)], "off": plain,
            "gumbel": me + ["--gumbel-child"]}
    raw = {k: [] for k in legs}
    for _ in range(GUMBEL_ROUNDS):
        for leg, cmd in legs.items():
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode:
                raise SystemExit(f"the {leg} leg failed:\n{(r.stderr or r.stdout)[-2000:]}")
            raw[leg].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(leg, "done", flush=True)

    def stats(xs):
        return {"us": round(median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "windows": xs}

    res = {"cap": CAP, "considered": GUMBEL_CONSIDERED, "window": GUMBEL_WINDOW, "rounds": GUMBEL_ROUNDS, "reps": REPS,
           "setting": SETTINGS["broad"], "gumbel": []}
    for i, run in enumerate(raw["gumbel"][0]["runs"]):
        row = {k: v for k, v in run.items() if k != "times"}
        t = {k: stats([x for r in raw["gumbel"] for x in r["runs"][i]["times"][k]]) for k in run["times"]}
        row.update({"search_us_per_sim": {"armed": t["search_armed"], "plain": t["search_plain"]},
                    "same_trees_us_per_sim": {"armed": t["same_armed"], "plain": t["same_plain"]},
                    "armed_select_extra_us": round(t["same_armed"]["us"] - t["same_plain"]["us"], 3),
                    "begin_us": t["begin"], "policy_us": t["policy"]})
        res["gumbel"].append(row)
    plain_res = {"games": G, "nodes": nodes, "sims": nodes, "windows": {w: list(ab) for w, ab in windows(nodes).items()}}
    for name in SETTINGS:
        out = {"same_visits": len({r[name]["root_visits_sha"] for leg in ("parent", "off") for r in raw[leg]}) == 1}
        for w in windows(nodes):
            row = {leg: stats([x for r in raw[leg] for x in r[name][w]["us_per_sim_reps"]]) for leg in ("parent", "off")}
            row["off_within_parent_spread"] = row["parent"]["min"] <= row["off"]["us"] <= row["parent"]["max"]
            row["off_over_parent"] = round(row["off"]["us"] / row["parent"]["us"], 4)
            out[w] = row
        plain_res[name] = out
    res["plain_path"] = plain_res
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


# ----------------------------------------------------------------------------- the device leg
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--advance", action="store_true", help="measure gc_tree_advance (see the module text)")
    ap.add_argument("--leaves", action="store_true", help="measure the batched calls (see the module text)")
    ap.add_argument("--solver", action="store_true", help="measure the solver's cost (see the module text)")
    ap.add_argument("--gumbel", action="store_true", help="measure Gumbel root search (see the module text)")
    ap.add_argument("--parent-root", default=None, help="--solver / --gumbel: another checkout of the project, built")
    ap.add_argument("--gumbel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--torch-leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--solver-child", default=None, choices=("off", "on"), help=argparse.SUPPRESS)
    ap.add_argument("--package-root", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    G, nodes = args.games, args.nodes
    sims = nodes
    if args.solver_child:
        if args.package_root:  # (ahead of this checkout's package)
            sys.path.insert(0, os.path.join(args.package_root, "gym-chess_amd"))
        solver_child(G, nodes, args.solver_child == "on")
        return
    if args.gumbel_child:
        gumbel_child()
        return
    if args.gumbel:
        if not args.parent_root:
            ap.error("--gumbel needs --parent-root")
        gumbel_leg(G, nodes, args.parent_root, args.out)
        return
    if args.solver:
        if not args.parent_root:
            ap.error("--solver needs --parent-root")
        solver_leg(G, nodes, args.parent_root, args.out)
        return
    if args.torch_leg:
        torch_leg(args.torch_leg, G, nodes, sims)
        return
    if args.advance:
        advance_leg(G, nodes, args.out)
        return
    if args.leaves:
        leaves_leg(nodes, args.out)
        return

    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(G * nodes, device=0, seed=11)
    L = env._L
    inp = make_inputs(G, sims)

    def upload(a):
        v = ctypes.c_void_p()
        _lib.check(L.gc_device_alloc(env.device, ctypes.c_uint64(a.nbytes), ctypes.byref(v)))
        _lib.check(L.gc_env_copy(env._h, v.value, _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))
        return v.value

    d = {k: upload(np.ascontiguousarray(v)) for k, v in inp.items()}
    tree = env.search_tree(G, nodes, cap=CAP)
    sel = tree._sel.ptr
    res = {"games": G, "nodes": nodes, "cap": CAP, "sims": sims, "tree_bytes": tree.device_bytes(),
           "windows": {w: list(ab) for w, ab in windows(sims).items()}}
    root_visits = {}

    def block(s):
        return (d["actions"] + 2 * G * CAP * s, d["priors"] + 4 * G * CAP * s, d["count"] + 4 * G * s, CAP)

    for name, (c_puct, fpu) in SETTINGS.items():
        def select():
            _lib.check(L.gc_tree_select(tree._h, c_puct, fpu, sel["parent"], sel["child"], sel["action"]))

        def backup(s):
            _lib.check(L.gc_tree_backup(tree._h, d["value"] + 4 * G * s, d["done"] + G * s, d["reason"] + G * s,
                                        *block(s)))

        starts = {a: w for w, (a, b) in windows(sims).items()}
        ends = {b: w for w, (a, b) in windows(sims).items()}
        times = {w: [] for w in windows(sims)}
        out = {}
        for rep in range(REPS + 1):  # the first run warms up; the trees and so the work are the same every run
            _lib.check(L.gc_tree_reset(tree._h, *block(sims), None))
            for s in range(sims):
                if s in starts:
                    env.synchronize()
                    env.record_event(4)
                select()
                backup(s)
                if s + 1 in ends:
                    w = ends[s + 1]
                    env.record_event(5)
                    env.synchronize()
                    a, b = windows(sims)[w]
                    if rep:
                        times[w].append(env.elapsed_ms(4, 5) * 1e3 / (b - a))
                    dep = tree.fetch("depth", "n_nodes", "overflow")
                    out[w] = {"mean_depth": round(float(dep["depth"].mean()), 2), "max_depth": int(dep["depth"].max()),
                              "mean_nodes": round(float(dep["n_nodes"].mean()), 1)}
        for w, t in times.items():
            out[w].update({"us_per_sim": round(median(t), 2), "us_per_sim_reps": [round(x, 2) for x in t]})
        root_visits[name] = tree.fetch("edge_visits")["edge_visits"][:, 0].copy()  # (what the torch leg reaches)
        # the split of one simulation after the last one (events around each call)
        ts, tb = [], []
        for _ in range(20):
            env.record_event(0)
            select()
            env.record_event(1)
            backup(sims - 1)
            env.record_event(2)
            env.synchronize()
            ts.append(env.elapsed_ms(0, 1) * 1e3)
            tb.append(env.elapsed_ms(1, 2) * 1e3)
        out["last_select_us"] = round(median(ts), 2)
        out["last_backup_us"] = round(median(tb), 2)
        res[name] = out
    env.synchronize()
    tree.close()
    for p in d.values():
        L.gc_device_free(env.device, ctypes.c_void_p(p))
    env.close()

    res["torch"] = None
    if not args.no_torch:
        import importlib.util

        if importlib.util.find_spec("torch") is not None:  # a fresh process: torch brings its own HIP runtime
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "tree.npz")
                np.savez(path, **inp, **{"root_visits_" + k: v for k, v in root_visits.items()})
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-leg", path, "--games", str(G),
                                    "--nodes", str(nodes)], capture_output=True, text=True)
            try:
                t = json.loads(r.stdout.strip().splitlines()[-1])
                res["torch"] = t.pop("torch")
                for name, v in t.items():
                    for w, x in v.items():
                        if isinstance(x, dict):
                            res[name][w].update(x)
                        else:
                            res[name]["torch_" + w] = x
            except Exception:
                res["torch_error"] = (r.stderr or r.stdout)[-400:]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
