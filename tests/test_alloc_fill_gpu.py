"""GPU: every kernel family on device memory that starts as garbage (GC_ALLOC_FILL).

A fresh process gets zeroed pages from hipMalloc almost every time, so a missing clear, a buffer
that is "always fully written" but is not, or a count or flag word assumed to be 0 passes every
other test and misbehaves in a long-lived process, where freed memory comes back dirty.  With
GC_ALLOC_FILL=<hex byte> the library fills every fresh device buffer (and every pinned host
buffer) with that byte before it hands it out (gc_host_hip.h).  Every object under test here --
engine, env, tree, store, playout handle, the tests' own device buffers -- is created while the
variable is set, under two patterns:

    0xA5   negative as int32, huge as uint32, NaN-free garbage as float32
    0xFF   -1, every flag set, NaN as a float, maximal generation words

and must compute what it computes on clean memory: the oracle's or the family's own reference's
results where the family's test has one (imported from that test, unchanged), else the same run
in objects created with the variable unset.  Every comparison is bit-exact, except the tree's
selections, which keep the acceptance rule of test_tree_search.py.  Each test also proves through
gc_alloc_fill_stats that fills happened while it ran; test_the_switch_is_live reads a filled
buffer back, so none of this can be vacuous.  DESIGN.md ("Device buffers: who writes first") has
the reading audit that these tests confirm."""
import contextlib
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import load_golden, random_positions

pytestmark = pytest.mark.gpu

VAR = "GC_ALLOC_FILL"


@pytest.fixture(scope="module", params=[0xA5, 0xFF], ids=["a5", "ff"])
def fill(request):
    """the fill byte, set for every allocation of the tests that take it"""
    os.environ[VAR] = f"{request.param:02x}"
    yield request.param
    os.environ.pop(VAR, None)


def fill_stats():
    """(allocations filled, bytes filled) since the library was loaded"""
    from gym_chess_amd import _lib

    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(_lib.load().gc_alloc_fill_stats(ctypes.byref(a), ctypes.byref(b)))
    return int(a.value), int(b.value)


@contextlib.contextmanager
def filling():
    """the body allocated under the fill: the counter rose"""
    assert os.environ.get(VAR), "the fill fixture is not active"
    a0, b0 = fill_stats()
    yield
    a1, b1 = fill_stats()
    assert a1 > a0 and b1 > b0, "no allocation was filled during the test"


@contextlib.contextmanager
def clean():
    """the body allocates with the variable unset: the counter does not move"""
    saved = os.environ.pop(VAR, None)
    before = fill_stats()
    try:
        yield
        assert fill_stats() == before, "an allocation was filled with the variable unset"
    finally:
        if saved is not None:
            os.environ[VAR] = saved


_ONCE = {}


def once(key, fn):
    """fn() computed once per process (references: the oracle's results, a clean run's): shared
    by both fill bytes and never changed"""
    if key not in _ONCE:
        _ONCE[key] = fn()
    return _ONCE[key]


def clean_once(key, fn):
    def run():
        with clean():
            return fn()

    return once(("clean",) + tuple(key), run)


def _pool():
    return ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1)))


def same_bytes(got, want, what=""):
    """two dicts (or sequences) of arrays / bytes, bit for bit"""
    keys = got.keys() if isinstance(got, dict) else range(len(got))
    assert len(got) == len(want), what
    for k in keys:
        a, b = got[k], want[k]
        if isinstance(a, (bytes, bytearray)):
            assert a == b, (what, k)
        else:
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, k)


# --------------------------------------------------------------------------- 1. the switch is live
def test_the_switch_is_live(fill):
    """gc_device_alloc of 1 000 003 bytes reads back as the fill byte throughout and is counted;
    with the variable unset nothing is counted"""
    from gym_chess_amd import _lib
    from gym_chess_amd.buffers import device_alloc, device_free
    from gym_chess_amd.env import BatchedChessEnv

    NB = 1_000_003
    with filling():
        env = BatchedChessEnv(8, device=0, seed=1)
        a0, b0 = fill_stats()
        p = device_alloc(env._L, 0, NB)
        a1, b1 = fill_stats()
        assert (a1 - a0, b1 - b0) == (1, NB)
        back = np.zeros(NB, dtype=np.uint8)
        _lib.check(env._L.gc_env_copy(env._h, _lib.ptr(back), p, ctypes.c_uint64(NB), 2))
        assert (back == fill).all(), np.flatnonzero(back != fill)[:4]
        device_free(env._L, 0, p)
    with clean():
        q = device_alloc(env._L, 0, NB)
        device_free(env._L, 0, q)
        for bad in ("", "1a5", "zz"):  # not a byte: the switch stays off
            os.environ[VAR] = bad
            q = device_alloc(env._L, 0, 64)
            device_free(env._L, 0, q)
        os.environ.pop(VAR, None)
    env.close()


# --------------------------------------------------------------------------- 2. perft, every path
def _paths():
    from gym_chess_amd.engine import perft_path_counts

    return perft_path_counts()


def _delta(c0, c1):
    return {k: c1[k] - c0[k] for k in c1 if c1[k] != c0[k]}


@contextlib.contextmanager
def setenv(name, value):
    os.environ[name] = value
    try:
        yield
    finally:
        del os.environ[name]


def _midgame(n, plies, seed):
    """test_gpu_parity._midgame_roots: random play's positions after `plies` plies (from a clean
    env, once: the roots are inputs, the same for both fill bytes)"""
    import test_gpu_parity as GP

    return clean_once(("midgame", n, plies, seed), lambda: GP._midgame_roots(n, plies, seed))


def test_perft3_of_4096_start_boards(fill, oracle):
    """The historic shape ("Tried and reverted: perft's temporaries from the
    stream-ordered pool": 8 782-8 785 instead of 8 982 for some roots): two expanded levels
    (4 096 -> 81 920 -> 1 638 400 nodes; both below perft_nodes' 131 072-node bar or above depth
    1) and the one-ply leaf pass.  Every root counts 8 982 (the reference rules' perft(3))."""
    from gym_chess_amd.engine import Engine

    b = np.tile(oracle.DEFAULT_BOARD, (4096, 1))
    m = np.tile(oracle.make_meta(), (4096, 1))
    with filling():
        eng = Engine(0)
        c0 = _paths()
        got = eng.perft(b, m, 3)
        assert _delta(c0, _paths()) == {"small": 1}
        assert (got == 8982).all(), (np.flatnonzero(got != 8982)[:8], got[got != 8982][:8])
        again = eng.perft(b, m, 3)  # the same call on the buffers the first one left
        assert (again == 8982).all(), (np.flatnonzero(again != 8982)[:8], again[again != 8982][:8])
        eng.close()


def test_perft5_split_pass_with_the_transposition_merge(fill, oracle):
    """200 mid-game roots at depth 5: the split pass with the merge (k_expand_range_rec, the sort,
    k_dedup_runs_f, k_leader_hist_f, k_place_leaders_f, k_perft2_val) == every record counted
    (GC_PERFT_DEDUP=0: k_expand_count / k_expand_place / k_perft2_rec) == the sorted leaf pass
    (GC_PERFT_SPLIT=0: k_perft_small_perm), per root; roots 0, 25, ..., 175 == the oracle"""
    from gym_chess_amd.engine import Engine, perft_dedup_stats

    b, m = _midgame(200, 21, 0x5EED + 5)
    pick = np.arange(0, 200, 25)
    ref = once("perft5", lambda: oracle.perft_by_children(b[pick], m[pick], 5, threads=16))
    with filling():
        eng = Engine(0)
        c0, (r0, s0) = _paths(), perft_dedup_stats()
        merged = eng.perft(b, m, 5)
        c1, (r1, s1) = _paths(), perft_dedup_stats()
        with setenv("GC_PERFT_DEDUP", "0"):
            every = eng.perft(b, m, 5)
        c2, (r2, s2) = _paths(), perft_dedup_stats()
        with setenv("GC_PERFT_SPLIT", "0"):
            whole = eng.perft(b, m, 5)
        c3 = _paths()
        eng.close()
    assert _delta(c0, c1) == {"split": 1} and _delta(c1, c2) == {"split": 1} and _delta(c2, c3) == {"sorted": 1}
    assert r1 - r0 == r2 - r1 == s2 - s1 > 0 and s1 - s0 < 0.8 * (r1 - r0)  # the merge happened
    assert (merged == every).all(), (np.flatnonzero(merged != every)[:4], merged[merged != every][:4])
    assert (merged == whole).all(), (np.flatnonzero(merged != whole)[:4], merged[merged != whole][:4])
    assert (merged[pick] == ref).all(), (pick, merged[pick], ref)
    assert merged.sum() > 200 * 10**6


def test_perft4_chunked_levels(fill, oracle):
    """48 roots, depth 4, a 1 000-node level cap: every expanded level runs in chunks of parents on
    child buffers that a larger chunk leaves to a smaller one (`held`) == unchunked == the oracle"""
    from gym_chess_amd.engine import Engine

    b, m = _midgame(48, 17, 0x5EED + 9)
    ref = once("perft4", lambda: oracle.perft_batch(b, m, 4, threads=16))
    with filling():
        eng = Engine(0)
        with setenv("GC_PERFT_LEVEL_CAP", "1000"):
            chunked = eng.perft(b, m, 4)
        whole = eng.perft(b, m, 4)
        eng.close()
    assert (chunked == ref).all(), (np.flatnonzero(chunked != ref)[:4], chunked[chunked != ref][:4])
    assert (whole == ref).all(), (np.flatnonzero(whole != ref)[:4], whole[whole != ref][:4])


def test_perft_small_and_fide_paths(fill, oracle):
    """48 random positions at depths 1-3 against the oracle (depth 1: the small pass alone; 2 and 3:
    expanded levels above it), and two published FIDE totals of test_fide.py through the FIDE pass"""
    import test_fide as F
    from gym_chess_amd.engine import Engine

    b, m = random_positions(48, 77)
    refs = once("perft_small", lambda: [oracle.perft_batch(b, m, d, threads=16) for d in (1, 2, 3)])
    with filling():
        eng = Engine(0)
        for d, ref in zip((1, 2, 3), refs):
            c0 = _paths()
            got = eng.perft(b, m, d)
            assert _delta(c0, _paths()) == {"small": 1}, d
            assert (got == ref).all(), (d, np.flatnonzero(got != ref)[:4])
        eng.close()
        feng = Engine(0, rules="fide")
        for (fen, totals), d in ((F.STANDARD[0], 4), (F.STANDARD[1], 3)):
            fb, fm = F.fide_arrays(fen)
            c0 = _paths()
            got = int(feng.perft(fb, fm, d)[0])
            assert _delta(c0, _paths()) == {"fide": 1}
            assert got == totals[d], (fen, d, got)
        feng.close()


def test_perft_larger_batch_then_smaller(fill, oracle):
    """Two calls in a row on one engine: 600 positions (the staging grows past the 256 it is
    created with), then 48 of them on the larger buffers"""
    from gym_chess_amd.engine import Engine

    b, m = random_positions(600, 78)
    ref = once("perft_grow", lambda: oracle.perft_batch(b, m, 2, threads=16))
    with filling():
        eng = Engine(0)
        a0 = fill_stats()[0]
        big = eng.perft(b, m, 2)
        assert fill_stats()[0] > a0  # (the growth allocated)
        small = eng.perft(b[100:148], m[100:148], 2)
        moves, cnt = eng.possible_moves(b[:300], m[:300], m[:300, 0])  # a list capacity grown after n
        eng.close()
    assert (big == ref).all() and (small == ref[100:148]).all()
    for i in range(0, 300, 7):
        assert [int(x) for x in moves[i, : cnt[i]]] == oracle.get_possible_moves(b[i], m[i], int(m[i, 0])), i


# --------------------------------------------------------------------------- 3. env lifecycle
ENV_KW = {"none": dict(), "random": dict(opponent="random"), "random_black": dict(opponent="random", player_color="BLACK"),
          "fide": dict(rules="fide")}
ENV_N, ENV_SEED, SINGLE_PLIES, LAUNCH_PLIES = 256, 4711, 300, 700
OUT_KEYS = ("reward", "done", "reason", "next_action", "nsteps")


def _lifecycle(kw):
    """300 single plies with their outputs, then one 700-ply launch with its trace"""
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(ENV_N, device=0, seed=ENV_SEED, **kw)
    assert LAUNCH_PLIES >= env.rollout_occ_min_plies()
    waves = env.rollout_waves()
    per = {k: [] for k in OUT_KEYS}
    for _ in range(SINGLE_PLIES):
        env.step_random(1)
        o = env.outputs()
        for k in OUT_KEYS:
            per[k].append(o[k])
    out = {"ply_" + k: np.stack(v) for k, v in per.items()}
    tb = env.trace_buffer(LAUNCH_PLIES)
    env.rollout_device(LAUNCH_PLIES, tb)
    out["trace"] = tb.raw()
    o = env.outputs()
    out.update({"last_" + k: o[k] for k in OUT_KEYS})
    out["boards"], out["meta"] = env.boards()
    out["window_sum"] = np.array([env.window_sum()])
    out["blob"] = env.checkpoint()
    tb.close()
    env.close()
    return out, waves


@pytest.mark.parametrize("name", list(ENV_KW))
def test_env_lifecycle(fill, oracle, name):
    """both opponent modes, a BLACK agent and the FIDE rules on 256 boards: every ply's outputs,
    the long launch's trace (over the occupancy filter's threshold), the final states, windows and
    the checkpoint equal those of an env created with the variable unset; reference rules without
    an opponent also equal the oracle's trajectories"""
    want, _ = clean_once(("lifecycle", name), lambda: _lifecycle(ENV_KW[name]))
    with filling():
        got, waves = _lifecycle(ENV_KW[name])
    same_bytes(got, want, name)
    if name != "none":
        return
    assert waves == 4  # the quad rollout, whose occupancy filter the 700 plies switch on
    total = SINGLE_PLIES + LAUNCH_PLIES

    def refs():
        with _pool() as ex:
            return list(ex.map(lambda i: oracle.rollout_trace(ENV_SEED, i, total + 1), range(ENV_N)))

    refs = once("lifecycle_oracle", refs)
    act = np.stack([r["action"] for r in refs], axis=1)  # [ply][board]
    rew = np.stack([r["reward"] for r in refs], axis=1)
    why = np.stack([r["reason"] for r in refs], axis=1)
    S = SINGLE_PLIES
    assert (got["ply_reward"] == rew[:S]).all() and (got["ply_reason"] == why[:S]).all()
    nxt = np.where(act < 0, 0xFFFF, act).astype(np.uint16)
    assert (got["ply_next_action"] == nxt[1: S + 1]).all()
    w = got["trace"]
    t_act = (w & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16)
    t_rew = ((w >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16)
    t_why = ((w >> np.uint64(40)) & np.uint64(0xFF)).astype(np.uint8)
    assert (t_act == act[S:total]).all() and (t_rew == rew[S:total]).all() and (t_why == why[S:total]).all()
    assert (got["last_next_action"] == nxt[total]).all()


def _api_steps(kw):
    """40 auto-reset API steps with mask, observation, count and pick"""
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(ENV_N, device=0, seed=ENV_SEED, **kw)
    io = env.device_io()
    outs = {}
    for s in range(40):
        env.step_device(io, autoreset=True)
        for k, v in io.fetch().items():
            outs.setdefault(k, []).append(v)
    out = {k: np.stack(v) for k, v in outs.items()}
    out["boards"], out["meta"] = env.boards()
    out["blob"] = env.checkpoint()
    env.synchronize()
    io.close()
    env.close()
    return out


@pytest.mark.parametrize("name", list(ENV_KW))
def test_env_api_step(fill, name):
    """step_device on the same boards: reward, done, reason, mask, observation, count and pick of
    every step, and the env afterwards, equal the clean env's"""
    want = clean_once(("api", name), lambda: _api_steps(ENV_KW[name]))
    with filling():
        got = _api_steps(ENV_KW[name])
    same_bytes(got, want, name)
    assert (got["count"] > 0).all(axis=1).any()
    if name != "fide":  # (the oracle's trajectories at this seed: episodes end within the 40 steps)
        assert got["done"].any()


# --------------------------------------------------------------------------- 4. spill table growth
def test_spill_table_grows_within_one_call(fill, oracle, monkeypatch):
    """test_spill.py's growth inside one call (a BLACK agent on the sparse board, 96 boards, a table
    started at 2^8 slots, ONE 2 000-step fused rollout with its trace): every table the growth
    allocates is filled first; every step == the oracle's, as there"""
    import test_spill as S
    from gym_chess_amd.env import BatchedChessEnv

    monkeypatch.setenv("GC_SPILL_BITS", "8")
    init, n, plies = S.kb_board(), 96, 2000

    def refs():
        with _pool() as ex:
            return list(ex.map(lambda i: oracle.rollout_trace(S.SEED, i, plies, init=init, opponent=1, agent_white=False),
                               range(n)))

    refs = once("spill_oracle", refs)
    with filling():
        env = BatchedChessEnv(n, device=0, seed=S.SEED, initial_board=init, opponent="random", player_color="BLACK")
        assert env.spill_info()["bits"] == 8
        tb = env.trace_buffer(plies)
        a0 = fill_stats()[0]
        env.rollout_device(plies, tb)
        info = env.spill_info()  # raises if an insert failed
        assert fill_stats()[0] >= a0 + 2  # (a grown table and its counters, at least)
        assert info["bits"] > 8 and info["live"] > 0, info
        b, m = env.boards()
        tr = tb.fetch()
        tb.close()
        env.close()
    for i, ref in enumerate(refs):
        assert (b[i] == ref["final_board"]).all() and list(m[i]) == list(ref["final_meta"]), i
        for k in ("action", "reward", "done", "reason"):
            assert (tr[k][:, i] == ref[k]).all(), (i, k, np.nonzero(tr[k][:, i] != ref[k])[0][:3])


# --------------------------------------------------------------------------- 5. checkpoint
def _checkpoint_run(kw):
    import test_checkpoint as CK
    from gym_chess_amd.env import BatchedChessEnv

    n, seed = 256, 2024
    env = BatchedChessEnv(n, device=0, seed=seed, **kw)
    env.step_random(150)
    blob = env.checkpoint()
    first = CK._plies(env, 100)
    bf, mf = env.boards()
    fresh = BatchedChessEnv(n, device=0, seed=seed, **kw)
    fresh.step_random(37)  # the fresh env's own windows and streams must not leak through
    fresh.load(blob)
    again = CK._plies(fresh, 100)
    b2, m2 = fresh.boards()
    assert CK._same(first, again) and (bf == b2).all() and (mf == m2).all()
    out = {"blob": blob, "boards": bf, "meta": mf, "blob_after": env.checkpoint(), "blob_fresh": fresh.checkpoint()}
    for j, k in enumerate(("reward", "done", "reason", "next_action")):
        out[k] = np.stack([p[j] for p in first])
    env.close()
    fresh.close()
    return out


@pytest.mark.parametrize("name", ["none", "random_black"])
def test_checkpoint_round_trip(fill, name):
    """save at ply 150, run 100 plies, load into a fresh env, rerun: identical outputs and final
    boards, equal to a clean env's; the blob's bytes equal the clean env's blob at the same ply
    (same seeds, same inserts in the same order: the live entries sit in the same table order, so
    no sorting is needed)"""
    want = clean_once(("ckpt", name), lambda: _checkpoint_run(ENV_KW[name]))
    with filling():
        got = _checkpoint_run(ENV_KW[name])
    same_bytes({k: got[k] for k in got if k != "blob_fresh"}, {k: want[k] for k in want if k != "blob_fresh"}, name)
    assert len(got["blob_fresh"]) == len(want["blob_fresh"])


# --------------------------------------------------------------------------- 6. the search tree
@pytest.fixture
def tree_env(fill):
    from gym_chess_amd.env import BatchedChessEnv

    with filling():
        e = BatchedChessEnv(160, device=0, seed=3)
        yield e
        e.close()


def test_tree_synthetic(tree_env):
    """test_tree_search_gpu's run of SYNTH_CASES[0] (5 trees of 12 nodes: they fill and overflow)
    against RefTree under the acceptance rule, on a tree, an env and buffers allocated under fill"""
    import test_tree_search as R
    import test_tree_search_gpu as T

    T.test_synthetic_trees(tree_env, R.SYNTH_CASES[0])


def test_tree_batch(tree_env):
    """select_batch / backup_batch (test_tree_batch_gpu, BATCH_CASES[0]) against RefTreeBatch: the
    batch scratch is compared as gc_tree_batch_reserve leaves it"""
    import test_tree_batch as B
    import test_tree_batch_gpu as TB

    TB.test_synthetic_batches(tree_env, B.BATCH_CASES[0])


def test_tree_solver(tree_env):
    import test_tree_solver as S
    import test_tree_solver_gpu as TS

    TS.test_synthetic_solver_trees(tree_env, S.SOLVER_CASES[0])


def test_tree_gumbel(tree_env):
    import test_tree_gumbel as GU
    import test_tree_gumbel_gpu as TG

    TG.test_searches(tree_env, GU.CASES[0])


def test_tree_advance(tree_env):
    """advance with its remap and kept outputs, and the in-place board move (test_tree_advance_gpu)"""
    import test_tree_advance as A
    import test_tree_advance_gpu as TA

    TA.test_synthetic_trees(tree_env, A.ADV_CASES[0])


# --------------------------------------------------------------------------- 7. the sample store
def test_sample_store_round_trip(fill):
    """test_replay_gpu's smallest synthetic sequence (5 games, cap 3) on a store left as
    gc_replay_create leaves it (no junk written over it: RefStore starts from zeros), then
    clear() and the sequence again on the cleared store; a drawn sample of the ring at the end"""
    import test_replay as R
    import test_replay_gpu as RG

    games, cap, row_cap, MAXP = 5, 3, 3, 4
    with filling():
        env = RG.make_env(8, 3)
        store = env.sample_store(games=games, cap=cap, max_plies=MAXP, capacity=games * MAXP)
        pos = RG.host_positions(env, games)
        for rnd in range(2):
            ref = R.RefStore(games, cap, MAXP, games * MAXP, alternate=True, fill=0)
            ref.same_as(store.fetch(), pos_mask=R.W7_KNOWN)
            rng = np.random.RandomState(games * 1000 + cap + rnd)
            target = rng.randint(1, 10, size=games)
            for call in range(18):
                actions = np.stack([rng.choice(4100, size=row_cap, replace=False) for _ in range(games)]).astype(np.uint16)
                visits = rng.randint(0, 1 << 20, size=(games, row_cap)).astype(np.int32)
                hole = rng.rand(games, row_cap) < 0.3
                actions[hole], visits[hole] = R.NONE, 0
                visits[rng.rand(games) < 0.2] = 0
                RG.record(env, store, ref, actions, visits, pos)
                ref.same_as(store.fetch(), pos_mask=R.W7_KNOWN)
                done = ((ref.plies >= target) | (rng.rand(games) < 0.1)).astype(np.uint8)
                reason = rng.choice([0, 1, 2, 3, 8], size=games).astype(np.uint8)
                outcome = rng.choice([-1.0, -0.0, 0.0, 0.5, 1.0], size=games).astype(np.float32) if call % 3 == 2 else None
                target[done != 0] = rng.randint(1, 10, size=int(done.sum()))
                RG.commit(env, store, ref, done, reason, outcome)
                ref.same_as(store.fetch(), pos_mask=R.W7_KNOWN)
            c = store.counters()
            assert c == {"total": ref.total, "live": ref.live, "plies": int(ref.plies.sum()),
                         "dropped": int(ref.dropped.sum())}
            assert ref.total > ref.R  # the ring wrapped
            batch = store.sample(16, seed=5, draw=rnd)
            got = batch.fetch("slot", "z", "pi_index")
            want = ref.sample(16, seed=5, draw=rnd)
            assert (got["slot"] == want["slot"]).all() and got["z"].tobytes() == want["z"].tobytes()
            assert (got["pi_index"] == want["pi_index"]).all()
            store.clear()
            assert all(not a.any() for a in store.fetch().values())
        env.synchronize()
        store.close()
        env.close()


# --------------------------------------------------------------------------- 8. playouts
def test_playouts_one_handle_run_again(fill):
    """test_playout_gpu's scratch reuse: one handle, four runs (the lanes' generation words persist
    across calls), other boards on the same lanes, against the host build of the playout body"""
    import test_playout_gpu as PG
    from gym_chess_amd.env import BatchedChessEnv

    boards, metas = PG.PC.positions()
    cases = boards[:PG.N], metas[:PG.N]
    assert 0 < int(cases[1][:, 0].sum()) < PG.N  # both sides to move
    with filling():
        env = BatchedChessEnv(PG.N, device=0, seed=9)
        env.set_states(*cases)
        PG.test_scratch_reuse(env, cases)
        env.close()


# --------------------------------------------------------------------------- 9. the rows APIs
ROWS_N = 130


def _rows_apis():
    """clone_boards, policy_priors, sample_policy, encode_planes / _rows and step_boards on a small
    env: every output's bytes, and the envs afterwards"""
    import test_planes_gpu as PG
    from gym_chess_amd.env import BatchedChessEnv
    from test_policy_priors_gpu import Dev

    n, out = ROWS_N, {}
    src = PG.make_env(n, 3)
    src.select_random()
    src.step_random(40)  # live 3-fold windows
    env = BatchedChessEnv(n, device=0, seed=4)
    idx = (np.arange(n) * 7 + 3) % n  # a permutation
    env.clone_boards(src, idx[:97], np.arange(97))
    assert env.clone_errors() == 0
    out["clone_blob"] = env.checkpoint()
    out["clone_boards"], out["clone_meta"] = env.boards()

    rng = np.random.RandomState(12)
    logits = Dev(env, rng.uniform(-3, 3, size=(n, 4100)).astype(np.float32))
    io = env.device_io(policy=True)
    env.step_device(io)  # the masks of the positions after one step
    out.update({"io_" + k: v for k, v in io.fetch().items() if k not in ("logprob", "entropy")})
    pri = env.priors_buffer(n, cap=64, logit_index=True)
    env.policy_priors(io, logits.ptr, pri)
    out.update({"priors_" + k: v for k, v in pri.fetch().items()})
    some = np.array([5, 5, 129, 0, 64, 63, 77])
    pri2 = env.priors_buffer(len(some), cap=7)
    env.policy_priors(io, logits.ptr, pri2, boards=some, relative=True)
    out.update({"priors_rows_" + k: v for k, v in pri2.fetch().items()})
    env.sample_policy(io, logits.ptr, seed=5, draw=2, temperature=0.7)
    out.update({"sample_" + k: v for k, v in io.fetch("pick", "logprob", "entropy").items()})

    for dtype, layout, persp in (("float16", "nchw", False), ("float32", "nhwc", True), ("bfloat16", "nchw", True)):
        buf = env.planes_buffer(dtype=dtype, layout=layout)
        env.encode_planes(buf, perspective=persp)
        out[f"planes_{dtype}_{layout}"] = buf.raw()
        rows = env.planes_buffer(dtype=dtype, layout=layout, rows=len(some))
        env.encode_planes_rows(rows, some[[0, 2, 3, 4, 5, 6, 1]], perspective=persp)
        out[f"planes_rows_{dtype}_{layout}"] = rows.raw()
        buf.close()
        rows.close()

    moves, cnt = env.legal_moves()
    listed = np.array([3, 129, 64, 0, 70, 65, 1])
    acts = np.array([moves[i, cnt[i] // 2] if cnt[i] else 0 for i in listed])
    rb = env.rows_buffer(len(listed))
    env.step_boards(io, listed, acts, out=rb)
    out.update({"rows_" + k: v for k, v in rb.fetch().items()})
    out["rows_mask"] = io.fetch("mask")["mask"]
    kept = env.step_boards(io, listed[:3], np.zeros(3, dtype=np.int64))  # the env's own rows buffer (a8a8: refused)
    out.update({"rows2_" + k: v[:3] for k, v in kept.fetch().items()})
    out["end_blob"] = env.checkpoint()
    env.synchronize()
    for b in (logits, io, pri, pri2, rb):
        b.close()
    env.close()
    src.close()
    return out


def test_rows_apis(fill):
    """the outputs land in device buffers that were themselves filled: bit-equal to a clean env's"""
    want = clean_once(("rows",), _rows_apis)
    with filling():
        got = _rows_apis()
    same_bytes(got, want)
    assert (got["priors_count"] > 0).any() and got["rows_reason"].size == 7


# --------------------------------------------------------------------------- 10. single-board env
def test_single_env_trace_and_one_position_calls(fill, oracle):
    """one reference trace of each kind of test_single_env.py on a ChessEnv created under fill (the
    server's mailbox and the step record are pinned host buffers), and the engine's one-position
    calls (the engine server) and batched calls on 48 fuzz boards against the oracle"""
    import test_single_env as SE
    from gym_chess_amd.engine import ChessEngine, Engine
    from gym_chess_amd.single import ChessEnv

    traces = load_golden("v2_env_traces.json.gz")
    scripted = next(t for t in traces if t.get("scripted"))
    driven = next(t for t in traces if not t.get("scripted") and t["opponent"] == "random")
    boards, metas = random_positions(48, 31)
    rng = np.random.RandomState(31)
    with filling():
        eng = ChessEngine(0)
        steps = sum(SE._replay(lambda **kw: ChessEnv(engine=eng, **kw), t) for t in (scripted, driven))
        assert steps > 20
        e = Engine(0)
        for i in range(48):
            b, m = boards[i:i + 1], metas[i:i + 1]
            for white in (0, 1):
                out, cnt = e.possible_moves(b, m, white)
                assert [int(x) for x in out[0, : cnt[0]]] == oracle.get_possible_moves(b[0], m[0], white, False), i
            occupied = np.nonzero(b[0])[0]
            a = 4096 + rng.randint(4) if rng.rand() < 0.2 else int(rng.choice(occupied)) * 64 + rng.randint(64)
            p = rng.randint(2)
            nb, nm, rw, st = e.next_state(b, m, p, a)
            rc, rb, rm, rr = oracle.next_state(b[0], m[0], p, a)
            assert st[0] == rc, i
            if rc in (0, 1):
                assert (nb[0] == rb).all() and list(nm[0, :7]) == list(rm[:7]) and rw[0] == rr, i
        out, cnt = e.possible_moves(boards, metas, metas[:, 0])
        for i in range(48):
            assert [int(x) for x in out[i, : cnt[i]]] == oracle.get_possible_moves(boards[i], metas[i], int(metas[i, 0]), False), i
        e.close()
