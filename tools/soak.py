"""Diagnostic soak (not in the test suite: minutes of GPU time): long full-size fused
rollouts against the oracle on sampled boards, for several seeds and opponent modes.

Each case: 65 536 boards, `--plies` plies of the device random self-play as fused launches of
`--chunk` plies with the per-ply trace; every ply's action / reward / done / reason of the
sampled boards (strided + the first / last 64 + the middle) == the oracle driver's, and the
sampled final states.  Long games reach the move cap, deep 3-fold windows and (BLACK agent)
the spill table.

    python tools/soak.py [--plies 4000] [--chunk 1000] [--seeds 5]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gym-chess_amd"), os.path.join(ROOT, "oracle")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plies", type=int, default=4000)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--boards", type=int, default=65536)
    ap.add_argument("--seed-base", type=int, default=1000, help="the opponent-none cases' seeds: base + 7919 k")
    ap.add_argument("--api", action="store_true",
                    help="instead: the API step's auto-reset pick loop (gc_env_step_device) vs the oracle driver "
                         "in action-id order, on every sampled board until it first meets a position with no move")
    ap.add_argument("--api-opp", choices=["WHITE", "BLACK"],
                    help="instead: the random opponent's API step (the quad kernel k_env_step_api4_vs, either "
                         "colour), actions = the previous "
                         "pick, auto-reset, in lockstep with the oracle env on the sampled boards")
    ap.add_argument("--launched", action="store_true",
                    help="drive the cases with one launch per ply (step_random: k_env_step2) instead of fused launches")
    ap.add_argument("--fide", action="store_true",
                    help="instead: rules='fide' fused rollouts vs the host build of gc_fide.h (tests/core_host)")
    ap.add_argument("--random-inits", type=int, default=0,
                    help="instead: K random (also weird) initial boards, 4 096 boards each (tests/conftest.py)")
    ap.add_argument("--api-digest", choices=["none", "random_white", "random_black"],
                    help="instead: replay --board of this tests/test_api_digest.py case step by step (the API "
                         "step fed picks, arbitrary actions and near misses) against the oracle env, every field")
    ap.add_argument("--board", type=int, default=0, help="the board id for --api-digest")
    a = ap.parse_args()
    if a.api_digest:
        return api_digest_replay(a)
    if a.api:
        return api_soak(a)
    if a.api_opp:
        return api_opp_soak(a)
    n = a.boards
    inits = [None]
    rules = "fide" if a.fide else "reference"
    if a.random_inits:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from conftest import random_positions

        n = 4096
        inits = list(random_positions(a.random_inits, 977)[0])
    idx = default_sample(n)
    threads = max(1, min(16, os.cpu_count() or 1))
    if a.fide:
        cases = [(0xF1DE + 7919 * k, "none", "WHITE", None) for k in range(a.seeds)]
    elif a.random_inits:
        cases = [(2000 + k, "none", "WHITE", ib) for k, ib in enumerate(inits)]
    else:
        cases = [(a.seed_base + 7919 * k, "none", "WHITE", None) for k in range(a.seeds)]
        cases += [(424242, "random", "WHITE", None), (434343, "random", "BLACK", None)]
    for seed, opp, color, ib in cases:
        bad, spill, secs = fused_case(seed, opp, color, ib, a.plies, a.chunk, n, idx, rules, a.launched, threads)
        print(json.dumps({"seed": seed, "form": "launched" if a.launched else "fused", "rules": rules,
                          "opponent": opp, "color": color, "boards": n, "plies": a.plies,
                          "sampled": len(idx), "mismatches": bad[:8], "spill": spill,
                          "seconds": secs}), flush=True)
        if bad:
            sys.exit(1)


def default_sample(n):
    """strided boards + the first / last 64 + the middle 32"""
    return np.array(sorted(set(range(0, n, 1021 if n > 8192 else 131)) | set(range(64)) | set(range(n - 64, n)) |
                           set(range(n // 2 - 16, n // 2 + 16))), dtype=np.int64)


def fused_case(seed, opp, color, ib, plies, chunk, n, idx, rules="reference", launched=False, threads=16):
    """One soak case: n boards x plies of device random self-play (fused launches of `chunk`
    plies with the per-ply trace, or one launch per ply) against the oracle driver (the host
    build of gc_fide.h for rules="fide") on the sampled boards idx.  Returns (mismatches
    [(what, ply, board)], the spill table's info for a BLACK agent, seconds)."""
    import oracle as O
    from gym_chess_amd.env import BatchedChessEnv

    fide = rules == "fide"
    if fide:
        sys.path.insert(0, os.path.join(ROOT, "tests", "core_host"))
        import corehost as H
        from gym_chess_amd import codec as C

        start = np.array(C.DEFAULT_BOARD, dtype=np.int8).reshape(64)
    t0 = time.time()
    env = BatchedChessEnv(n, device=0, seed=seed, opponent=opp, player_color=color, initial_board=ib, rules=rules)
    tb = env.trace_buffer(chunk)
    got = {k: [] for k in ("action", "reward", "done", "reason")}
    for p in range(plies if launched else 0):
        played = env.outputs()["next_action"].astype(np.int32)[idx]
        env.step_random(1)
        o = env.outputs()
        got["action"].append(np.where(played == 0xFFFF, -1, played)[None])
        for key in ("reward", "done", "reason"):
            got[key].append(o[key][idx][None])
    for p in range(0, 0 if launched else plies, chunk):
        k = min(chunk, plies - p)
        env.rollout_device(k, tb)
        env.synchronize()
        tr = tb.fetch(k)
        for key in got:
            got[key].append(tr[key][:, idx])
        del tr
    b, m = env.boards()
    spill = env.spill_info() if color == "BLACK" else None
    tb.close()
    env.close()
    kw = dict(opponent=1 if opp == "random" else 0, agent_white=color == "WHITE")
    if ib is not None:
        kw["init"] = ib
    with ThreadPoolExecutor(threads) as ex:
        if fide:  # the host build's trace (no final state: the boards are compared by trace only)
            refs = list(ex.map(lambda i: H.fide_rollout(seed, int(i), plies, start), idx))
        else:
            refs = list(ex.map(lambda i: O.rollout_trace(seed, int(i), plies, **kw), idx))
    bad = []
    for key in got:
        g = np.concatenate(got[key], axis=0)
        w = np.stack([r[key][:plies] for r in refs], axis=1)
        for p_, j in np.argwhere(g != w)[:4]:
            bad.append((key, int(p_), int(idx[j])))
    for j, i in enumerate(idx if not fide else []):
        if not ((b[i] == refs[j]["final_board"]).all() and list(m[i]) == list(refs[j]["final_meta"])):
            bad.append(("final", plies, int(i)))
            break
    return bad, spill, round(time.time() - t0, 1)


def api_soak(a):
    import oracle as O
    from gym_chess_amd.env import BatchedChessEnv

    n = a.boards
    idx = np.array(sorted(set(range(0, n, 1021)) | set(range(64)) | set(range(n - 64, n))), dtype=np.int64)
    threads = max(1, min(16, os.cpu_count() or 1))
    for seed in (2718 + 31 * k for k in range(a.seeds)):
        t0 = time.time()
        with ThreadPoolExecutor(threads) as ex:
            refs = list(ex.map(lambda i: O.rollout_trace(seed, int(i), a.plies + 1, order="action"), idx))
        env = BatchedChessEnv(n, device=0, seed=seed)
        io = env.device_io()
        first = np.zeros(n, dtype=np.uint16)
        first[idx] = [max(int(r["action"][0]), 0) for r in refs]
        io.upload_actions(first)
        live = np.ones(len(idx), dtype=bool)
        bad, checked = [], 0
        for p in range(a.plies):
            env.step_device(io, autoreset=True)
            o = io.fetch("reward", "done", "pick")
            live &= np.array([r["reason"][p] != 4 and r["action"][p] >= 0 for r in refs])
            rr = np.array([r["reward"][p] for r in refs])
            rd = np.array([r["done"][p] for r in refs])
            nx = np.array([r["action"][p + 1] for r in refs])
            ok = live & (nx >= 0)
            for j in np.nonzero(live & ((o["reward"][idx] != rr) | (o["done"][idx] != rd)))[0][:2]:
                bad.append(("reward/done", p, int(idx[j])))
            for j in np.nonzero(ok & (o["pick"][idx] != nx))[0][:2]:
                bad.append(("pick", p, int(idx[j])))
            checked += int(live.sum())
            if bad:
                break
        env.close()
        print(json.dumps({"api_seed": seed, "boards": n, "plies": a.plies, "sampled": len(idx),
                          "board_plies_checked": checked, "mismatches": bad[:8],
                          "seconds": round(time.time() - t0, 1)}), flush=True)
        if bad:
            sys.exit(1)


def api_opp_case(seed, color, plies, n, idx):
    """The random opponent's device API step (auto-reset, actions = the previous picks) against
    the oracle env on the boards idx: every step's reward / done / reason and pick, the states
    every 500 plies.  A board left without a legal move and not done (pick 0xFFFF) is reset by
    the host reset, whose policy pick is its next action (the oracle: reset and one pick), so
    every checked step is a real step.
    -> (mismatches, board steps checked, spill info, seconds, steps fed to a board with no
    legal move)"""
    import oracle as O
    from gym_chess_amd.env import BatchedChessEnv

    t0 = time.time()
    env = BatchedChessEnv(n, device=0, seed=seed, opponent="random", player_color=color)
    io = env.device_io(mask=False, obs=False, count=False)
    ors = {int(i): O.OracleEnv(opponent=1, agent_white=color == "WHITE", seed=seed, board=int(i)) for i in idx}
    for o in ors.values():
        o.pick()
    prev = io.fetch("pick")["pick"].astype(np.int64)
    bad, steps, stuck_steps = [], 0, 0
    for p in range(plies):
        stuck_steps += int((prev == 0xFFFF).sum())  # over all n boards, not only the sampled ones
        acts = np.where(prev == 0xFFFF, 0, prev).astype(np.uint16)
        io.upload_actions(acts)
        env.step_device(io, autoreset=True)
        out = io.fetch("reward", "done", "reason", "pick")
        for i, o in ors.items():
            rc, rw, dn, why = o.step(int(acts[i]))
            if rc == 1:
                dn, why = 1, 5
            if (rw, dn, why) != (int(out["reward"][i]), int(out["done"][i]), int(out["reason"][i])):
                bad.append(("step", p, i))
                break
            if dn:
                o.reset()
            legal = sorted(o.moves())
            want = legal[O.policy_index(seed, i, o.draw, len(legal))] if legal else 0xFFFF
            if int(out["pick"][i]) != want:
                bad.append(("pick", p, i))
                break
            if legal:
                o.pick()
            else:  # stuck: the host reset below, and its policy pick
                o.reset()
                o.pick()
            steps += 1
        prev = out["pick"].astype(np.int64)
        stuck = prev == 0xFFFF
        if stuck.any() and not bad:
            env.reset(stuck.astype(np.uint8), states=False)
            prev[stuck] = env.outputs()["next_action"][stuck]
        if p % 500 == 499 or p == plies - 1:
            b, m = env.boards()
            for i, o in ors.items():
                ob, om = o.state()
                if not ((b[i] == ob).all() and list(m[i]) == list(om)):
                    bad.append(("state", p, i))
                    break
        if bad:
            break
    spill = env.spill_info() if color == "BLACK" else None
    io.close()
    env.close()
    return bad, steps, spill, round(time.time() - t0, 1), stuck_steps


def api_opp_soak(a):
    n, color = a.boards, a.api_opp
    idx = np.array(sorted(set(range(0, n, 1021)) | set(range(64)) | set(range(n - 64, n))), dtype=np.int64)
    for seed in (0x0A11 + 97 * k for k in range(a.seeds)):
        bad, steps, spill, secs, stuck_steps = api_opp_case(seed, color, a.plies, n, idx)
        print(json.dumps({"api_opp_seed": seed, "color": color, "boards": n, "plies": a.plies,
                          "sampled": len(idx), "board_steps_checked": steps, "stuck_steps": stuck_steps,
                          "mismatches": bad[:8], "spill": spill, "seconds": secs}), flush=True)
        if bad:
            sys.exit(1)


def api_digest_replay(a):
    """One board of a tests/test_api_digest.py case, step by step: the device loop (an env of
    board + 1 boards: the boards are independent) against the oracle env, every field of every
    step; prints the first step that differs and the fields."""
    import oracle as O
    from gym_chess_amd.env import BatchedChessEnv

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_api_digest as T

    name, seed, opp, color = next(c for c in T.CASES if c[0] == a.api_digest)
    i, n, steps = a.board, a.board + 1, min(a.plies, T.STEPS)
    s, r = T.schedule(seed, [i], steps, threads=1)
    env = BatchedChessEnv(n, device=0, seed=seed, opponent="random" if opp else "none", player_color=color)
    io = env.device_io()
    act_buf = env.device_io(mask=False, obs=False, count=False, pick=True, select=False)
    o = O.OracleEnv(opponent=opp, agent_white=color == "WHITE", seed=seed, board=i)
    acts = io.fetch("pick")["pick"].astype(np.uint16)
    want_a = o.pick()
    for p in range(steps):
        if int(acts[i]) != want_a:
            print(json.dumps({"case": name, "board": i, "step": p, "field": "carried action", "device": int(acts[i]),
                              "oracle": want_a}))
            sys.exit(1)
        acts[i] = T.choose([want_a], s[p], r[p])[0]
        act_buf.upload_actions(acts)
        env.step_device(io, actions=act_buf.ptr["pick"], autoreset=True)
        out = io.fetch()
        rc, rw, dn, why = o.step(int(acts[i]))
        if rc == 1:
            dn, why = 1, 5
        if dn:
            o.reset()
        legal = sorted(o.moves())
        pick = 0xFFFF
        if legal:
            pick = legal[O.policy_index(seed, i, o.draw, len(legal))]
            o.pick()
        want = {"reward": rw, "done": dn, "reason": why, "pick": pick, "count": len(legal),
                "mask": T.mask_words(legal).tolist(), "obs": o.state()[0].tolist()}
        got = {k: out[k][i].tolist() for k in want}
        diff = [k for k in want if want[k] != got[k]]
        if diff:
            print(json.dumps({"case": name, "board": i, "step": p, "action": int(acts[i]), "fields": diff,
                              "device": {k: got[k] for k in diff}, "oracle": {k: want[k] for k in diff}}))
            sys.exit(1)
        acts = out["pick"].copy()
        if not legal:
            o.reset()
            want_a = o.pick()
            stuck = np.zeros(n, dtype=np.uint8)
            stuck[i] = 1
            env.reset(stuck, states=False)
            acts[i] = env.outputs()["next_action"][i]
        else:
            want_a = pick
        acts[acts == 0xFFFF] = 0  # the other boards only keep the launch shape
    b, m = env.boards()
    ob, om = o.state()
    ok = bool((b[i] == ob).all() and list(m[i]) == list(om))
    print(json.dumps({"case": name, "board": i, "steps": steps, "equal": ok}))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
