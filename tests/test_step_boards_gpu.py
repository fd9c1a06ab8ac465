"""GPU: one env.step() on the listed boards only (gc_env_step_boards / BatchedChessEnv.step_boards).

The reference is the dense device step (step_device) on a twin env, itself pinned to the oracle by
test_api_step.py / test_api_digest.py: two envs of the same size, seed, rules and opponent mode,
loaded from one checkpoint, take the same actions -- one through step_device, one through
step_boards.

Shapes: envs of 130 boards (not a multiple of 64: the wave-blocked window tables end in a partial
block), rows in {1, 67, 130} and the parts of a random three-way partition.  The boards come from
test_clone_gpu's three recipes (random plies, a knight shuffle one move short of the third
repetition, long quiet windows)."""
import ctypes

import numpy as np
import pytest

from test_clone_gpu import IDLE, SEED, SHUFFLE, play_recipes, recipe, slab, window
from test_policy_sample_gpu import Dev

pytestmark = pytest.mark.gpu

N = 130
BAD = 255
ROW_KEYS = ("reward", "done", "reason", "count", "obs")


def upload(env, ptr, host):
    from gym_chess_amd import _lib

    host = np.ascontiguousarray(host)
    _lib.check(env._L.gc_env_copy(env._h, ptr, _lib.ptr(host), ctypes.c_uint64(host.nbytes), 1))


def fill(env, ptr, nbytes, byte=0xAB):
    upload(env, ptr, np.full(nbytes, byte, dtype=np.uint8))


def fill_rows(env, rb, byte=0xAB):
    for k in rb.ptr:
        fill(env, rb.ptr[k], rb._shape(k)[1], byte)


class Twins:
    """a dense env and an indexed env in the same state, with their buffers.  fresh() builds both
    anew and loads one checkpoint into them: a load re-inserts the windows under generations that
    follow the env's earlier ones, so only envs with the same history end byte-identical."""

    def __init__(self, **kw):
        from gym_chess_amd.env import BatchedChessEnv

        self.kw = kw
        env = BatchedChessEnv(N, device=0, seed=SEED, **kw)
        play_recipes(env)
        self.blob = env.checkpoint()
        env.close()
        self.live = []

    def fresh(self):
        from gym_chess_amd.env import BatchedChessEnv

        self.close()
        self.dense = BatchedChessEnv(N, device=0, seed=SEED, **self.kw)
        self.rows = BatchedChessEnv(N, device=0, seed=SEED, **self.kw)
        self.dense.load(self.blob)
        self.rows.load(self.blob)
        assert self.dense.checkpoint() == self.rows.checkpoint()
        self.dio = self.dense.device_io(pick=False)  # (no pick: neither env's policy actions are refreshed)
        self.rio = self.rows.device_io(pick=False)
        self.dacts = Dev(self.dense, np.zeros(N, dtype=np.uint16))
        self.rb = self.rows.rows_buffer(N)
        self.live = [self.dio, self.rio, self.dacts, self.rb, self.dense, self.rows]
        return self.dense, self.rows

    def step_dense(self, acts, autoreset=False):
        upload(self.dense, self.dacts.ptr, np.asarray(acts, dtype=np.uint16))
        self.dense.step_device(self.dio, actions=self.dacts.ptr, autoreset=autoreset)
        return self.dio.fetch("reward", "done", "reason", "count", "obs", "mask")

    def close(self):
        for x in self.live:
            x.close()
        self.live = []


@pytest.fixture(scope="module")
def twins():
    t = Twins()
    yield t
    t.close()


def legal_actions(env, rng, done):
    """one seeded random legal action per board, IDLE on finished boards and boards without a move"""
    mv, cnt = env.legal_moves()
    acts = np.full(N, IDLE, dtype=np.uint16)
    for i in range(N):
        if not done[i] and cnt[i] > 0:
            acts[i] = sorted(int(a) for a in mv[i, : cnt[i]])[rng.randint(cnt[i])]
    return acts


def assert_rows_equal_dense(got, want, boards, what):
    for k in ROW_KEYS:
        bad = [j for j, b in enumerate(boards) if not (got[k][j] == want[k][b]).all()]
        assert not bad, (what, k, bad[:5], [(int(got[k][j].ravel()[0]), int(want[k][boards[j]].ravel()[0])) for j in bad[:5]])


# ----------------------------------------------------------------------------- 1. partition == dense
def run_partition(t, autoreset, plies=30, shuffle=True):
    """shuffle: the shuffle boards first complete their third repetition (plies 0 and 1), so some
    boards are done (IDLE from then on: reason 7) or, with auto-reset, start over"""
    dense, rows = t.fresh()
    rng = np.random.RandomState(11)
    sh = [i for i in range(N) if recipe(i) == "shuffle"]
    fill(rows, t.rio.ptr["mask"], 65 * t.rio.mask_stride * 8)
    done = dense.outputs()["done"] != 0
    seen_done = 0
    for ply in range(plies):
        acts = legal_actions(dense, rng, done)
        if shuffle and ply < 2:
            acts[sh] = SHUFFLE[(7 + ply) % 4]
        want = t.step_dense(acts, autoreset)
        perm = rng.permutation(N)
        cuts = np.sort(rng.choice(np.arange(1, N), size=2, replace=False))
        for part in np.split(perm, cuts):  # three parts, each in permuted order
            rb = rows.step_boards(t.rio, part, acts[part], out=t.rb, autoreset=autoreset)
            assert rb is t.rb
            got = rb.fetch()
            assert_rows_equal_dense(got, want, part, (ply, len(part)))
        assert (t.rio.fetch("mask")["mask"] == want["mask"]).all(), ply
        seen_done += int((want["done"] != 0).sum())
        done = (want["done"] != 0) & (not autoreset)
    assert dense.checkpoint() == rows.checkpoint()
    return seen_done


def test_partition_equals_dense(twins):
    assert run_partition(twins, autoreset=False) >= 10  # the shuffle boards' 3-fold verdicts


def test_partition_equals_dense_autoreset(twins):
    assert run_partition(twins, autoreset=True) >= 10  # the shuffle boards finish and start over


def test_all_boards_in_one_call(twins):
    """rows = 130: the whole env in one call, in reverse order, is the dense step"""
    dense, rows = twins.fresh()
    acts = legal_actions(dense, np.random.RandomState(12), dense.outputs()["done"] != 0)
    want = twins.step_dense(acts)
    order = np.arange(N - 1, -1, -1)
    got = rows.step_boards(twins.rio, order, acts[order], out=twins.rb).fetch()
    assert_rows_equal_dense(got, want, order, N)
    assert (twins.rio.fetch("mask")["mask"] == want["mask"]).all()
    assert dense.checkpoint() == rows.checkpoint()


@pytest.mark.parametrize("kw", [dict(rules="fide"), dict(opponent="random")], ids=["fide", "random_opponent"])
def test_partition_equals_dense_variants(kw):
    t = Twins(**kw)
    try:
        run_partition(t, autoreset=False, plies=30, shuffle="opponent" not in kw)
        if "opponent" in kw:  # the full partition keeps the twins' draw counters in step
            assert (slab(t.dense)["draw"] == slab(t.rows)["draw"]).all() and slab(t.rows)["draw"].max() > 0
    finally:
        t.close()


# ----------------------------------------------------------------------------- 2. 3-fold
def test_threefold_through_step_boards(twins):
    dense, rows = twins.fresh()
    sh = np.array([i for i in range(N) if recipe(i) == "shuffle"], dtype=np.int32)
    assert len(sh) >= 10
    verdict_d, verdict_r = {}, {}
    for t in range(3):
        a = SHUFFLE[(7 + t) % 4]
        acts = np.full(N, IDLE, dtype=np.uint16)
        acts[sh] = a
        want = twins.step_dense(acts)
        got = rows.step_boards(twins.rio, sh, np.full(len(sh), a), out=twins.rb).fetch()
        assert_rows_equal_dense(got, want, sh, t)
        for j, b in enumerate(sh):
            if want["reason"][b] == 2:
                verdict_d.setdefault(int(b), t)
            if got["reason"][j] == 2:
                verdict_r.setdefault(int(b), t)
    assert verdict_r == verdict_d and set(verdict_r) == set(sh.tolist())
    assert set(verdict_r.values()) == {1}  # Ng8, then Nf3 from the start position's third occurrence
    from gym_chess_amd import _lib

    with pytest.raises(_lib.GymChessError, match="policy actions stale"):  # no pick: act[] is stale
        rows.step_random(1)
    rows.select_random()
    rows.step_random(1)
    rows.synchronize()


# ----------------------------------------------------------------------------- 3. bystanders
def snapshot(env, io, boards):
    b, m = env.boards()
    o = env.outputs()
    sl = slab(env)
    snap = dict(board=b[boards], meta=m[boards], mask=io.fetch("mask")["mask"][boards])
    snap.update({k: v[boards] for k, v in o.items()})
    snap.update({k: v[boards] for k, v in sl.items()})
    return snap, [window(env, i) for i in boards]


@pytest.mark.parametrize("m", [1, 67])
def test_unlisted_boards_are_untouched(twins, m):
    dense, rows = twins.fresh()
    rng = np.random.RandomState(3)
    listed = rng.permutation(N)[:m].astype(np.int32)
    others = np.setdiff1d(np.arange(N), listed)
    acts = legal_actions(rows, rng, rows.outputs()["done"] != 0)
    fill(rows, twins.rio.ptr["mask"], 65 * twins.rio.mask_stride * 8)
    fill_rows(rows, twins.rb)
    before, win_before = snapshot(rows, twins.rio, others)
    assert (before["mask"] == np.uint64(0xABABABABABABABAB)).all()
    nsteps0 = rows.outputs()["nsteps"][listed]
    rows.step_boards(twins.rio, listed, acts[listed], out=twins.rb)
    after, win_after = snapshot(rows, twins.rio, others)
    for k in before:
        assert (before[k] == after[k]).all(), k
    assert win_before == win_after
    got = twins.rb.fetch()
    for k in ROW_KEYS:  # the row buffers beyond `rows` keep their prefill
        assert (got[k][m:].view(np.uint8) == 0xAB).all(), k
    want = twins.step_dense(acts)
    assert_rows_equal_dense({k: v[:m] for k, v in got.items()}, want, listed, m)
    assert (twins.rio.fetch("mask")["mask"][listed] == want["mask"][listed]).all()
    assert (rows.outputs()["nsteps"][listed] == nsteps0 + 1).all()
    b_r, _ = rows.boards()
    b_d, _ = dense.boards()
    assert (b_r[listed] == b_d[listed]).all()


# ----------------------------------------------------------------------------- 4. bad indices
def test_bad_indices(twins):
    dense, rows = twins.fresh()
    rng = np.random.RandomState(5)
    acts = legal_actions(rows, rng, rows.outputs()["done"] != 0)
    idx = np.array([3, -1, 7, N, 2 ** 31 - 1, 129, 64, -(2 ** 31)], dtype=np.int64)
    valid = np.array([0, 2, 5, 6])
    named = idx[valid]
    others = np.setdiff1d(np.arange(N), named)
    fill(rows, twins.rio.ptr["mask"], 65 * twins.rio.mask_stride * 8)
    fill_rows(rows, twins.rb)
    before, win_before = snapshot(rows, twins.rio, others)
    ra = np.full(len(idx), SHUFFLE[0], dtype=np.uint16)
    ra[valid] = acts[named]
    ip = Dev(rows, np.clip(idx, -(2 ** 31), 2 ** 31 - 1).astype(np.int32))  # the device-pointer form
    ap = Dev(rows, ra)
    rows.step_boards(twins.rio, ip.ptr, ap.ptr, rows=len(idx), out=twins.rb)
    got = twins.rb.fetch()
    bad = np.setdiff1d(np.arange(len(idx)), valid)
    assert (got["reason"][bad] == BAD).all() and (got["reward"][bad] == 0).all() and (got["done"][bad] == 0).all()
    assert (got["count"][bad] == -1).all() and (got["obs"][bad] == 0).all()
    want = twins.step_dense(acts)
    assert_rows_equal_dense({k: v[valid] for k, v in got.items()}, want, named, "valid rows")
    after, win_after = snapshot(rows, twins.rio, others)
    for k in before:
        assert (before[k] == after[k]).all(), k
    assert win_before == win_after
    assert (twins.rio.fetch("mask")["mask"][named] == want["mask"][named]).all()
    ip.close()
    ap.close()


# ----------------------------------------------------------------------------- 5. argument errors
def test_argument_errors(twins):
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    _, rows = twins.fresh()
    L, rb, io = rows._L, twins.rb, twins.rio
    idx = Dev(rows, np.arange(4, dtype=np.int32))
    act = Dev(rows, np.full(4, SHUFFLE[0], dtype=np.uint16))
    blob = rows.checkpoint()
    good = dict(e=rows._h, idx=idx.ptr, act=act.ptr, rows=4, rw=rb.ptr["reward"], dn=rb.ptr["done"], rs=rb.ptr["reason"],
                cnt=rb.ptr["count"], mask=io.ptr["mask"], stride=io.mask_stride, obs=rb.ptr["obs"], flags=0)

    def call(**kw):
        a = dict(good, **kw)
        return L.gc_env_step_boards(a["e"], a["idx"], a["act"], a["rows"], a["rw"], a["dn"], a["rs"], a["cnt"], a["mask"],
                                    a["stride"], a["obs"], a["flags"])

    for kw in (dict(e=None), dict(idx=None), dict(act=None), dict(rw=None), dict(dn=None), dict(rs=None), dict(rows=-1),
               dict(stride=N - 1), dict(stride=1), dict(flags=2), dict(flags=3), dict(flags=-1)):
        assert call(**kw) != 0, kw
        assert L.gc_last_error().decode(), kw
    assert call(rows=0) == 0 and call(rows=0, idx=None, act=None, rw=None, dn=None, rs=None) == 0
    rows.step_boards(io, [], [], out=rb)
    black = BatchedChessEnv(4, device=0, seed=1, opponent="random", player_color="BLACK")
    assert call(e=black._h, mask=None, stride=0) != 0
    msg = L.gc_last_error().decode()
    assert "BLACK" in msg and "clone" in msg
    with pytest.raises(_lib.GymChessError):
        black.step_boards(None, [0], [SHUFFLE[0]])
    with pytest.raises(ValueError):
        rows.step_boards(io, [0, 1], [SHUFFLE[0]], out=rb)
    with pytest.raises(ValueError):
        rows.step_boards(io, idx.ptr, act.ptr, out=rb)  # device pointers need rows
    with pytest.raises(ValueError):
        rows.step_boards(io, np.arange(N), np.full(N, IDLE), out=rows.rows_buffer(4))
    with pytest.raises(TypeError):
        rows.step_boards(io, [0], [IDLE], out=io)
    assert rows.checkpoint() == blob  # nothing was launched, nothing changed
    black.close()
    idx.close()
    act.close()


# ----------------------------------------------------------------------------- 6. the loop
def test_search_loop_equals_dense_calls():
    from gym_chess_amd.env import BatchedChessEnv

    G, SIMS = 10, 5
    tree = BatchedChessEnv(N, device=0, seed=9)
    twin = BatchedChessEnv(N, device=0, seed=9)
    tio, dio = tree.device_io(pick=False), twin.device_io(pick=False)
    dacts = Dev(twin, np.zeros(N, dtype=np.uint16))
    logits = Dev(tree, np.random.RandomState(2).standard_normal((G, 4100)).astype(np.float32))
    rb = tree.rows_buffer(G)
    planes_r = tree.planes_buffer(dtype="float16", rows=G)
    planes_d = twin.planes_buffer(dtype="float16")
    pri_r, pri_d = tree.priors_buffer(G, cap=64), twin.priors_buffer(G, cap=64)
    rng = np.random.RandomState(4)
    parent = np.arange(G, dtype=np.int32)
    for sim in range(SIMS):
        child = (G * (sim + 1) + rng.permutation(G)).astype(np.int32)
        mv, cnt = tree.legal_moves()
        move = np.array([mv[p, rng.randint(cnt[p])] if cnt[p] else IDLE for p in parent], dtype=np.uint16)
        # the indexed loop
        tree.clone_boards(tree, parent, child)
        tree.step_boards(tio, child, move, out=rb)
        tree.encode_planes_rows(planes_r, child, perspective=True)
        tree.policy_priors(tio, logits.ptr, pri_r, boards=child, relative=True)
        # the dense calls
        twin.clone_boards(twin, parent, child)
        acts = np.full(N, IDLE, dtype=np.uint16)
        acts[child] = move
        upload(twin, dacts.ptr, acts)
        twin.step_device(dio, actions=dacts.ptr)
        twin.encode_planes(planes_d, perspective=True)
        twin.policy_priors(dio, logits.ptr, pri_d, boards=child, relative=True)
        want = dio.fetch("reward", "done", "reason", "count", "obs")
        assert_rows_equal_dense(rb.fetch(), want, child, sim)
        assert (planes_r.raw() == planes_d.raw()[child]).all(), sim
        pr, pd = pri_r.fetch(), pri_d.fetch()
        for k in pr:
            assert (pr[k].view(np.uint8) == pd[k].view(np.uint8)).all(), (sim, k)
        assert (pr["count"] > 0).all()
        bt, mt = tree.boards()
        bd, md = twin.boards()
        assert (bt[child] == bd[child]).all() and (mt[child] == md[child]).all(), sim
        for c in child:
            assert window(tree, c) == window(twin, c), (sim, c)
        parent = child
    # the tree's earlier nodes kept their last outputs; the dense twin overwrote them (reason 6)
    ot, od = tree.outputs(), twin.outputs()
    early = np.arange(G, 2 * G)
    assert not (ot["reason"][early] == 6).any() and (od["reason"][early] == 6).all()
    assert (ot["nsteps"][early] == 1).all() and (od["nsteps"][early] == SIMS).all()
    for x in (tio, dio, dacts, logits, rb, planes_r, planes_d, pri_r, pri_d, tree, twin):
        x.close()
