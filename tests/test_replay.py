"""CPU: RefStore, the numpy restatement of the device sample store's contract (gc_replay_* in
include/gymchess.h) that tests/test_replay_gpu.py compares the kernels with, and hand-worked cases
that pin the restatement itself.

A sample = the packed position (seven bitboards and word 7 = meta word | count in the 3-fold
window, saturated at 2, << 32 | n << 40), n <= cap pairs (action u16, visits i32) and z.  record()
appends a pending sample per game, commit() stamps z on a finished game's samples (sign
alternating back from the last one on an opponent "none" env) and copies them to ring slots (total
+ off[g] + p) mod capacity, sample() decodes ring slots into planes, the policy target in the
network's view and z."""
import os
import re

import numpy as np

import test_planes as PL
import test_policy_sample as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = 4100
NONE = 0xFFFF
R_MATE, R_REPETITION, R_MOVE_CAP, R_MATED = 1, 2, 3, 8
# the bits of word 7 the host API can restate: side, rights, check flags, move_count, the FIDE
# en-passant flag and file, the 3-fold count and n (not: the done flag and the window's length)
W7_KNOWN = 0x7F | (0xFF << 8) | (0xF << 25) | (0xFF << 32) | (0x1FF << 40)


# ----------------------------------------------------------------------------- the packed position
def pack_pos(board, meta8, rep=0, ep_file=-1, n=0):
    """host arrays -> uint64[8]: bitboards K Q R B N P (both colours), WHITE's pieces (bit sq =
    row * 8 + col, row 0 = rank 8), word 7"""
    b = np.asarray(board, dtype=np.int64).reshape(64)
    w = [0] * 8
    for sq in range(64):
        if b[sq]:
            w[abs(int(b[sq])) - 1] |= 1 << sq
            if b[sq] > 0:
                w[6] |= 1 << sq
    m = [int(x) for x in meta8]
    meta = m[0] | m[1] << 1 | m[2] << 2 | m[3] << 3 | m[4] << 4 | m[5] << 5 | m[6] << 6 | m[7] << 8
    if ep_file >= 0:
        meta |= 1 << 25 | int(ep_file) << 26
    w[7] = meta | min(int(rep), 2) << 32 | int(n) << 40
    return np.array(w, dtype=np.uint64)


def unpack_pos(words):
    """uint64[8] -> (board int8[64], meta8 uint8[8], rep, ep_file, n)"""
    w = [int(x) for x in words]
    board = np.zeros(64, dtype=np.int8)
    for k in range(6):
        for sq in range(64):
            if w[k] >> sq & 1:
                board[sq] = (k + 1) if w[6] >> sq & 1 else -(k + 1)
    meta = w[7] & 0xFFFFFFFF
    meta8 = np.array([meta & 1, meta >> 1 & 1, meta >> 2 & 1, meta >> 3 & 1, meta >> 4 & 1, meta >> 5 & 1,
                      meta >> 6 & 1, meta >> 8 & 0xFF], dtype=np.uint8)
    ep = (meta >> 26 & 7) if meta >> 25 & 1 else -1
    return board, meta8, w[7] >> 32 & 0xFF, ep, w[7] >> 40 & 0x1FF


def mirror(a):
    """the logits-row element of action a on a BLACK-to-move position in the side-to-move view"""
    a = int(a)
    return a ^ 0xE38 if a < 4096 else 4096 + ((a - 4096) ^ 2)


def drawn_slots(rows, seed, draw, live):
    """slot of row j = (uint64(philox_x0(seed, j, draw)) * live) >> 32"""
    x = P.philox_x0(seed, np.arange(rows), draw).astype(np.uint64)
    return ((x * np.uint64(live)) >> np.uint64(32)).astype(np.int64)


# ----------------------------------------------------------------------------- the restatement
class RefStore:
    def __init__(self, games, cap, max_plies, capacity, alternate=True, fill=0):
        assert 1 <= cap <= 256 and max_plies >= 1 and capacity >= games * max_plies
        self.G, self.cap, self.P, self.R, self.alternate = games, cap, max_plies, capacity, alternate

        def arr(shape, dt):
            return np.frombuffer(bytes([fill]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dtype=dt).reshape(shape).copy()

        self.pend_pos, self.pend_act, self.pend_vis = arr((games, max_plies, 8), np.uint64), \
            arr((games, max_plies, cap), np.uint16), arr((games, max_plies, cap), np.int32)
        self.ring_pos, self.ring_act, self.ring_vis = arr((capacity, 8), np.uint64), arr((capacity, cap), np.uint16), \
            arr((capacity, cap), np.int32)
        self.ring_z = arr((capacity,), np.float32)
        self.off = arr((games,), np.int32)
        self.base = arr((1,), np.uint64)
        self.plies = np.zeros(games, dtype=np.int32)
        self.dropped = np.zeros(games, dtype=np.int32)
        self.total = 0

    @property
    def live(self):
        return min(self.total, self.R)

    def record(self, actions, visits, pos):
        """actions u16 / visits i32 [G][row_cap], pos uint64[G][8] (pack_pos; its n field is set here)"""
        actions, visits = np.asarray(actions), np.asarray(visits)
        assert actions.shape == visits.shape and actions.shape[0] == self.G and actions.shape[1] <= self.cap
        for g in range(self.G):
            if int(visits[g].astype(np.int64).sum()) == 0:
                continue
            p = int(self.plies[g])
            self.plies[g] = p + 1
            if p >= self.P:
                self.dropped[g] += 1
                continue
            on = actions[g] != NONE
            n = int(on.sum())
            self.pend_act[g, p] = NONE
            self.pend_vis[g, p] = 0
            self.pend_act[g, p, :n] = actions[g][on]
            self.pend_vis[g, p, :n] = visits[g][on]
            w = np.array(pos[g], dtype=np.uint64)
            w[7] = np.uint64((int(w[7]) & ~(0x1FF << 40)) | n << 40)
            self.pend_pos[g, p] = w

    def commit(self, done, reason, outcome=None):
        count = [min(int(self.plies[g]), self.P) if done[g] else 0 for g in range(self.G)]
        self.base[0] = self.total
        run = 0
        for g in range(self.G):
            self.off[g] = run
            run += count[g]
        for g in range(self.G):
            if not done[g]:
                continue
            Pn = int(self.plies[g])
            if outcome is not None:
                zl = np.float32(outcome[g])
            else:
                zl = np.float32(1.0 if reason[g] == R_MATE else -1.0 if reason[g] == R_MATED else 0.0)
            for p in range(count[g]):
                slot = (self.total + int(self.off[g]) + p) % self.R
                self.ring_pos[slot], self.ring_act[slot], self.ring_vis[slot] = \
                    self.pend_pos[g, p], self.pend_act[g, p], self.pend_vis[g, p]
                flip = self.alternate and ((Pn - 1 - p) & 1)
                self.ring_z[slot] = np.float32(0.0) if zl == 0 else (-zl if flip else zl)
            self.plies[g] = 0
        self.total += run

    def clear(self):
        self.__init__(self.G, self.cap, self.P, self.R, self.alternate)

    def target(self, slot, perspective):
        """(pi_index int32[cap], pi float32[cap], dense float32[4100]) of a ring slot"""
        idx = np.full(self.cap, -1, dtype=np.int32)
        pi = np.zeros(self.cap, dtype=np.float32)
        dense = np.zeros(ROW, dtype=np.float32)
        if slot < 0:
            return idx, pi, dense
        _, meta8, _, _, n = unpack_pos(self.ring_pos[slot])
        n = min(n, self.cap)
        vis = self.ring_vis[slot, :n].astype(np.int64)
        s = int(vis.sum())
        for k in range(n):
            a = int(self.ring_act[slot, k])
            if a >= ROW:
                continue
            idx[k] = mirror(a) if perspective and not meta8[0] else a
            pi[k] = np.float32(vis[k]) / np.float32(s) if s > 0 else np.float32(0)
            dense[idx[k]] = pi[k]
        return idx, pi, dense

    def sample(self, rows, index=None, seed=0, draw=0, perspective=True, layout="nchw", fide=False):
        """float32 planes [rows,...], pi_index, pi, pi_dense, z, slot, and the float64 quotients"""
        want = drawn_slots(rows, seed, draw, self.live) if index is None else np.asarray(index, dtype=np.int64)
        slot = np.where((want >= 0) & (want < self.live), want, -1).astype(np.int32)
        out = {"slot": slot, "z": np.zeros(rows, dtype=np.float32),
               "pi_index": np.zeros((rows, self.cap), dtype=np.int32), "pi": np.zeros((rows, self.cap), dtype=np.float32),
               "pi_dense": np.zeros((rows, ROW), dtype=np.float32)}
        shape = (PL.PLANES, 8, 8) if layout == "nchw" else (8, 8, PL.PLANES)
        out["planes"] = np.zeros((rows,) + shape, dtype=np.float32)
        for j in range(rows):
            s = int(slot[j])
            out["pi_index"][j], out["pi"][j], out["pi_dense"][j] = self.target(s, perspective)
            if s < 0:
                continue
            out["z"][j] = self.ring_z[s]
            board, meta8, rep, ep, _ = unpack_pos(self.ring_pos[s])
            out["planes"][j] = PL.ref_planes(board[None], meta8[None], [rep], [ep if fide else -1], perspective, layout)[0]
        return out

    def same_as(self, got, pos_mask=None):
        """every array of a device fetch (SampleStore.fetch()) equals the restatement's"""
        for k in ("pend_act", "pend_vis", "ring_act", "ring_vis", "plies", "dropped", "off"):
            assert (got[k] == getattr(self, k)).all(), k
        assert got["ring_z"].tobytes() == self.ring_z.tobytes(), "ring_z"
        assert int(got["total"][0]) == self.total and int(got["base"][0]) == int(self.base[0])
        for k in ("pend_pos", "ring_pos"):
            a, b = got[k].copy(), getattr(self, k).copy()
            if pos_mask is not None:
                a[..., 7] &= np.uint64(pos_mask)
                b[..., 7] &= np.uint64(pos_mask)
            assert (a == b).all(), k


# ----------------------------------------------------------------------------- hand-worked cases
START = PL.START
META = np.array([1, 1, 1, 1, 1, 0, 0, 0], dtype=np.uint8)


def _rows(games, cap, plies, seed=0):
    """per ply a [games][cap] block of distinct actions and positive visits, and positions that
    differ per ply (the move_count)"""
    rng = np.random.RandomState(seed)
    out = []
    for t in range(plies):
        a = np.stack([rng.choice(4100, size=cap, replace=False) for _ in range(games)]).astype(np.uint16)
        v = rng.randint(1, 50, size=(games, cap)).astype(np.int32)
        m = META.copy()
        m[7] = t
        m[0] = (t + 1) & 1
        out.append((a, v, np.stack([pack_pos(START, m)] * games)))
    return out


def _episode(st, plies, reason=0, outcome=None, seed=0):
    for a, v, pos in _rows(st.G, st.cap, plies, seed):
        st.record(a, v, pos)
    st.commit(np.ones(st.G, dtype=np.uint8), np.full(st.G, reason, dtype=np.uint8),
              None if outcome is None else np.full(st.G, outcome, dtype=np.float32))


def test_z_signs_by_hand():
    for plies, want in ((3, [1, -1, 1]), (4, [-1, 1, -1, 1])):
        st = RefStore(1, 4, 8, 8)
        _episode(st, plies, R_MATE)
        assert st.ring_z[:plies].tolist() == want and st.total == plies and st.plies[0] == 0
        # the stored order is the recorded order: move_count t at slot t
        assert [unpack_pos(st.ring_pos[t])[1][7] for t in range(plies)] == list(range(plies))
        st = RefStore(1, 4, 8, 8)
        _episode(st, plies, R_REPETITION)
        assert (st.ring_z[:plies] == 0).all() and not np.signbit(st.ring_z[:plies]).any()
        st = RefStore(1, 4, 8, 8)
        _episode(st, plies, R_MOVE_CAP, outcome=-0.0)
        assert not np.signbit(st.ring_z[:plies]).any()
    # an env with an opponent inside the step: every sample is the agent's
    st = RefStore(1, 4, 8, 8, alternate=False)
    _episode(st, 3, R_MATED)
    assert st.ring_z[:3].tolist() == [-1, -1, -1]
    st = RefStore(1, 4, 8, 8, alternate=False)
    _episode(st, 4, R_MATE)
    assert st.ring_z[:4].tolist() == [1, 1, 1, 1]
    # reason 8 on an alternating env still reads as -1 for the last mover
    st = RefStore(1, 4, 8, 8)
    _episode(st, 2, R_MATED)
    assert st.ring_z[:2].tolist() == [1, -1]


def test_outcome_override():
    st = RefStore(1, 4, 8, 8)
    _episode(st, 3, R_MATE, outcome=-0.5)  # the reason is not consulted
    assert st.ring_z[:3].tolist() == [-0.5, 0.5, -0.5]
    st = RefStore(1, 4, 8, 8, alternate=False)
    _episode(st, 3, 0, outcome=0.25)
    assert st.ring_z[:3].tolist() == [0.25, 0.25, 0.25]


def test_drop_at_max_plies_keeps_the_parity():
    st = RefStore(1, 4, 2, 4)
    _episode(st, 5, R_MATE)  # P = 5: samples 0 and 1 are stored, 2..4 dropped; the last mover is ply 4
    assert st.dropped[0] == 3 and st.total == 2
    assert st.ring_z[:2].tolist() == [1, -1]
    _episode(st, 4, R_MATE, seed=1)  # P = 4: ply 0 is the loser's
    assert st.dropped[0] == 5 and st.total == 4 and st.ring_z[2:4].tolist() == [-1, 1]


def test_ring_wraps():
    st = RefStore(1, 2, 3, 3)
    _episode(st, 2, R_MATE, seed=1)      # slots 0, 1
    first = st.ring_act.copy()
    _episode(st, 2, R_REPETITION, seed=2)  # slots 2, 0
    assert st.total == 4 and st.live == 3 and int(st.base[0]) == 2
    assert (st.ring_act[1] == first[1]).all() and not (st.ring_act[0] == first[0]).all()
    assert st.ring_z.tolist() == [0, 1, 0]
    _episode(st, 3, R_MATE, seed=3)      # slots 1, 2, 0
    assert st.total == 7 and st.ring_z.tolist() == [1, 1, -1]


def test_two_games_commit_in_prefix_order():
    st = RefStore(3, 2, 4, 12)
    rows = _rows(3, 2, 3, seed=4)
    for t, (a, v, pos) in enumerate(rows):
        v = v.copy()
        if t >= 1:
            v[2] = 0  # game 2 records one ply only
        if t >= 2:
            v[1] = 0  # game 1 two
        st.record(a, v, pos)
    assert st.plies.tolist() == [3, 2, 1]
    st.commit(np.array([1, 0, 1], dtype=np.uint8), np.array([R_MATE, 0, R_REPETITION], dtype=np.uint8))
    assert st.off.tolist() == [0, 3, 3] and st.total == 4 and st.plies.tolist() == [0, 2, 0]
    assert st.ring_z[:4].tolist() == [1, -1, 1, 0]
    assert (st.ring_act[3] == rows[0][0][2]).all() and (st.ring_act[2] == rows[2][0][0]).all()
    st.commit(np.array([1, 1, 0], dtype=np.uint8), np.array([0, R_MATE, 0], dtype=np.uint8))  # game 0 has nothing
    assert st.off.tolist() == [0, 0, 2] and st.total == 6 and st.ring_z[4:6].tolist() == [-1, 1]


def test_record_compacts_and_skips():
    st = RefStore(2, 4, 2, 4, fill=0xAB)
    a = np.array([[7, NONE, 9, NONE], [1, 2, 3, 4]], dtype=np.uint16)
    v = np.array([[5, 0, 6, 0], [0, 0, 0, 0]], dtype=np.int32)
    st.record(a, v, np.stack([pack_pos(START, META, rep=3)] * 2))
    assert st.plies.tolist() == [1, 0]
    assert st.pend_act[0, 0].tolist() == [7, 9, NONE, NONE] and st.pend_vis[0, 0].tolist() == [5, 6, 0, 0]
    board, meta8, rep, ep, n = unpack_pos(st.pend_pos[0, 0])
    assert (board == START).all() and (meta8 == META).all() and rep == 2 and ep == -1 and n == 2
    assert (st.pend_act[1] == 0xABAB).all()  # untouched
    st.record(a[:, :3], v[:, :3], np.stack([pack_pos(START, META)] * 2))  # row_cap < cap
    assert st.pend_act[0, 1].tolist() == [7, 9, NONE, NONE]


def test_pack_roundtrip():
    from conftest import random_positions

    boards, metas = random_positions(50, 11)
    rng = np.random.RandomState(1)
    for b, m in zip(boards, metas):
        m[5:7] = rng.randint(2, size=2)
        m[7] = rng.randint(256)
        rep, ep, n = int(rng.randint(3)), int(rng.randint(-1, 8)), int(rng.randint(257))
        w = pack_pos(b, m, rep, ep, n)
        gb, gm, grep, gep, gn = unpack_pos(w)
        assert (gb == b).all() and (gm == m).all() and (grep, gep, gn) == (rep, ep, n)
        assert int(w[7]) & ~W7_KNOWN == 0


def test_mirror_is_test_planes_mirror_action():
    a = np.arange(ROW)
    assert [mirror(x) for x in a] == PL.mirror_action(a).tolist()


def test_target_by_hand():
    st = RefStore(2, 4, 1, 2)
    black = META.copy()
    black[0] = 0
    a = np.array([[52 * 64 + 36, 4096, 4100, NONE], [12 * 64 + 28, 4099, NONE, NONE]], dtype=np.uint16)
    v = np.array([[1, 2, 1, 0], [3, 1, 0, 0]], dtype=np.int32)
    st.record(a, v, np.stack([pack_pos(START, META), pack_pos(START, black)]))
    st.commit([1, 1], [R_MATE, R_MATE])
    idx, pi, dense = st.target(0, True)  # WHITE to move: no mirror; action 4100 has no element
    assert idx.tolist() == [52 * 64 + 36, 4096, -1, -1] and pi.tolist() == [0.25, 0.5, 0, 0]
    assert dense[52 * 64 + 36] == 0.25 and dense[4096] == 0.5 and np.count_nonzero(dense) == 2
    idx, pi, dense = st.target(1, True)  # BLACK to move: e7e5 -> e2e4, 4099 -> 4097
    assert idx.tolist() == [52 * 64 + 36, 4097, -1, -1] and pi.tolist() == [0.75, 0.25, 0, 0]
    idx, _, _ = st.target(1, False)
    assert idx.tolist() == [12 * 64 + 28, 4099, -1, -1]
    out = st.sample(4, index=[1, 0, 2, -1], perspective=True)
    assert out["slot"].tolist() == [1, 0, -1, -1] and out["z"].tolist() == [1, 1, 0, 0]
    assert (out["planes"][2:] == 0).all() and (out["pi_index"][2:] == -1).all() and (out["pi_dense"][2:] == 0).all()
    assert (out["planes"][0] == PL.ref_planes(START[None], black[None], [0], [-1], True, "nchw")[0]).all()
    assert out["planes"][1, 12].all() and not out["planes"][0, 12].any()
    for j in range(2):  # dense = the sparse row scattered into zeros
        d = np.zeros(ROW, dtype=np.float32)
        on = out["pi_index"][j] >= 0
        d[out["pi_index"][j][on]] = out["pi"][j][on]
        assert (d == out["pi_dense"][j]).all()


def test_drawn_slot_is_the_formula():
    for seed, draw, live in ((5, 0, 1), (5, 1, 7), (2 ** 40 + 3, 9, 1000), (1, 2, 2 ** 31 - 1)):
        got = drawn_slots(300, seed, draw, live)
        x = P.philox_x0(seed, np.arange(300), draw)
        assert got.tolist() == [(int(v) * live) >> 32 for v in x]
        assert got.min() >= 0 and got.max() < live
    assert len(set(drawn_slots(300, 5, 1, 1000).tolist())) > 200
    assert (drawn_slots(300, 5, 1, 1000) != drawn_slots(300, 5, 2, 1000)).any()
    st = RefStore(1, 2, 1, 4)
    assert st.sample(5, seed=3)["slot"].tolist() == [-1] * 5  # live == 0
    _episode(st, 1, R_MATE)
    assert st.sample(5, seed=3)["slot"].tolist() == [0] * 5


# ----------------------------------------------------------------------------- the boundary
SYMBOLS = ("gc_replay_create", "gc_replay_destroy", "gc_replay_clear", "gc_replay_record", "gc_replay_commit",
           "gc_replay_sample", "gc_replay_counters", "gc_replay_pointers", "gc_replay_device_bytes")


def test_header_declares_and_binding_covers_the_store():
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv, SampleStore

    src = open(os.path.join(ROOT, "include", "gymchess.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), s
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    assert re.search(r"#define\s+GC_REPLAY_ARRAYS\s+12\b", src)
    assert len(SampleStore.ARRAYS) == 12
    assert len(_lib.SIGNATURES["gc_replay_sample"][1]) == 15
    assert callable(BatchedChessEnv.sample_store)
    for name in ("record", "commit", "sample", "counters", "clear", "device_bytes", "close", "fetch"):
        assert callable(getattr(SampleStore, name)), name
