"""GPU: the env's staging buffers for uploaded lists (gym_chess_amd.buffers._Staging) across their
first growth.  They start at 256 items, so a call with 2 rows, one with 257 and one with 2 again
runs on the first buffer, replaces it (synchronize, free, allocate 512) and runs on the new one;
step_boards' action list lives at offset 4 * cap of the same allocation and moves with it.  No
other GPU test uploads more than 256 rows from the host (they run on 70 to 200 boards, or pass
device pointers).

Each test: env A gets the three calls with host lists, env B -- same seed, same history -- the
same calls with the lists in device buffers of its own, which touch no staging buffer.  Before a
call that changes boards both are rewound from a saved copy by clone_boards with device pointers
(no staging either).  Everything is integer or the same kernel on the same inputs: outputs are
compared bit for bit."""
import numpy as np
import pytest

from test_clone_gpu import state
from test_policy_sample_gpu import Dev

pytestmark = pytest.mark.gpu

N, SEED, PLIES = 512, 23, 12
SIZES = (2, 257, 2)


class Side:
    """an env N boards wide, PLIES random plies and one step_device in, so io.mask / io.pick hold
    every board's legal mask and the random policy's action for it"""

    def __init__(self):
        from gym_chess_amd.env import BatchedChessEnv

        self.env = BatchedChessEnv(N, device=0, seed=SEED)
        self.env.step_random(PLIES)
        self.io = self.env.device_io()
        self.env.step_device(self.io)
        self.picks = self.io.fetch("pick")["pick"]
        self.live = [self.io]

    def dev(self, host):
        self.live.append(Dev(self.env, host))
        return self.live[-1].ptr

    def close(self):
        for x in self.live:
            x.close()
        self.env.close()


class Rig:
    """the two sides, a saved copy of their boards and rewind(side), which puts them back"""

    def __init__(self):
        from gym_chess_amd.env import BatchedChessEnv

        self.a, self.b = Side(), Side()
        assert (self.a.picks == self.b.picks).all() and self.a.env.checkpoint() == self.b.env.checkpoint()
        self.save = BatchedChessEnv(N, device=0, seed=SEED + 1)
        self.every = Dev(self.save, np.arange(N, dtype=np.int32))
        self.save.clone_boards(self.a.env, self.every.ptr, self.every.ptr, count=N)
        self.saved = state(self.save)
        assert (self.saved["done"] == 0).sum() >= N // 2

    def rewind(self, side):
        side.env.clone_boards(self.save, self.every.ptr, self.every.ptr, count=N)

    def close(self):
        errors = [e.clone_errors() for e in (self.a.env, self.b.env, self.save)]
        for x in (self.a, self.b, self.every, self.save):
            x.close()
        assert errors == [0, 0, 0]


@pytest.fixture
def rig():
    r = Rig()
    yield r
    r.close()


def boards_of(call, m):
    """m distinct boards in no order, another set per call, the first and the last board among them"""
    p = 1 + np.random.RandomState(40 + call).permutation(N - 2)[: m - 2]
    return np.concatenate([[N - 1], p, [0]]).astype(np.int32)


def same(got_a, got_b, what):
    assert set(got_a) == set(got_b)
    for k in got_a:
        assert got_a[k].dtype == got_b[k].dtype and got_a[k].tobytes() == got_b[k].tobytes(), (what, k)


def first(got, m):
    return {k: v[:m] for k, v in got.items()}


def test_step_boards(rig):
    a, b = rig.a, rig.b
    for call, m in enumerate(SIZES):
        idx = boards_of(call, m)
        acts = a.picks[idx]
        rig.rewind(a)
        rig.rewind(b)
        ra = a.env.step_boards(a.io, idx, acts)  # (out=None: the env's own rows buffer grows as well)
        rb = b.env.step_boards(b.io, b.dev(idx), b.dev(acts), rows=m)
        ga, gb = ra.fetch(), rb.fetch()
        assert ra.rows >= m and (ga["reason"][:m] != a.env.BAD_INDEX).all() and (ga["count"][:m] >= 0).all()
        same(first(ga, m), first(gb, m), (call, m))
        same(a.io.fetch("mask"), b.io.fetch("mask"), (call, m, "mask"))
        sa = state(a.env)
        same(sa, state(b.env), (call, m, "state"))
        moved = (sa["board"] != rig.saved["board"]).any(axis=1)
        assert moved[idx].sum() >= m // 2 and moved.sum() == moved[idx].sum(), (call, m)  # these boards, no other
    assert a.env._staging["rows"].cap == 512 and b.env._staging["rows"].cap == 0


def test_policy_priors(rig):
    a, b = rig.a, rig.b
    logits = np.random.RandomState(7).standard_normal((SIZES[1], 4100)).astype(np.float32)
    la, lb = a.dev(logits), b.dev(logits)
    pa = a.env.priors_buffer(SIZES[1], cap=48, logit_index=True)
    pb = b.env.priors_buffer(SIZES[1], cap=48, logit_index=True)
    a.live.append(pa)
    b.live.append(pb)
    for call, m in enumerate(SIZES):
        idx = boards_of(call, m)
        a.env.policy_priors(a.io, la, pa, boards=idx.tolist() if call else idx)
        b.env.policy_priors(b.io, lb, pb, boards=b.dev(idx), rows=m)
        ga, gb = pa.fetch(), pb.fetch()
        assert (ga["count"][:m] > 0).sum() >= m // 2 and (ga["priors"][:m, 0] > 0).sum() >= m // 2
        same(first(ga, m), first(gb, m), (call, m))
    assert a.env._staging["priors"].cap == 512 and b.env._staging["priors"].cap == 0


def test_encode_planes_rows(rig):
    a, b = rig.a, rig.b
    pa, pb = a.env.planes_buffer(dtype="float16", rows=SIZES[1]), b.env.planes_buffer(dtype="float16", rows=SIZES[1])
    dense = a.env.planes_buffer(dtype="float16")
    a.live += [pa, dense]
    b.live.append(pb)
    a.env.encode_planes(dense)
    want = dense.raw()
    assert want.any(axis=1).all()
    for call, m in enumerate(SIZES):
        idx = boards_of(call, m)
        a.env.encode_planes_rows(pa, idx)
        b.env.encode_planes_rows(pb, b.dev(idx), rows=m)
        ga, gb = pa.raw()[:m], pb.raw()[:m]
        assert ga.tobytes() == gb.tobytes() and ga.tobytes() == want[idx].tobytes(), (call, m)
    assert a.env._staging["rows"].cap == 512 and b.env._staging["rows"].cap == 0


def test_clone_boards(rig):
    a, b, saved = rig.a, rig.b, rig.saved
    for call, m in enumerate(SIZES):
        src, dst = boards_of(call, m), np.roll(boards_of(call + 3, m), 1)  # (m = 2: boards 511, 0 into 0, 511)
        rig.rewind(a)
        rig.rewind(b)
        a.env.clone_boards(rig.save, src, dst)
        b.env.clone_boards(rig.save, b.dev(src), b.dev(dst), count=m)
        sa = state(a.env)
        same(sa, state(b.env), (call, m))
        for k in sa:
            assert (sa[k][dst] == saved[k][src]).all(), (call, m, k)
        rest = np.setdiff1d(np.arange(N), dst)
        assert (sa["board"][rest] == saved["board"][rest]).all() and (sa["board"] != saved["board"]).any()
    assert a.env._staging["clone"].cap == 512 and b.env._staging["clone"].cap == 0
