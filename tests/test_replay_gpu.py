"""GPU: the device sample store (gc_replay_* / BatchedChessEnv.sample_store) against RefStore of
tests/test_replay.py: synthetic record / commit sequences compared field by field after every
call, the decoded planes against encode_planes' bytes captured at record time, the policy target,
drawn sampling, whole games of chess, and the argument errors.  Buffers come from gc_device_alloc /
gc_env_copy; no torch."""
import ctypes

import numpy as np
import pytest

import test_planes as PL
import test_policy_sample as P
import test_replay as R
from test_planes_gpu import FENS, ITEM, as_bytes, make_env, rep_counts
from test_policy_priors_gpu import Dev
from test_tree_search_gpu import fill

pytestmark = pytest.mark.gpu

NONE = R.NONE
ELEMS = PL.PLANES * 64
GUARD = 4096


# ----------------------------------------------------------------------------- helpers
def fill_store(env, store):
    """0xAB into every sample array and the commit scratch (not the counters), so a skipped store shows"""
    for k in ("pend_pos", "pend_act", "pend_vis", "ring_pos", "ring_act", "ring_vis", "ring_z", "off", "base"):
        fill(env, store.ptr[k], int(np.prod(store._shape(k))) * np.dtype(store._DTYPES.get(k, np.int32)).itemsize)


def host_positions(env, games):
    """pack_pos of the env's first `games` boards from the host readback"""
    b, m = env.boards()
    rep = rep_counts(env, b, ids=range(games))[0]
    ep = env.en_passant()
    return np.stack([R.pack_pos(b[g], m[g], rep[g], int(ep[g])) for g in range(games)])


def record(env, store, ref, actions, visits, pos):
    a, v = Dev(env, actions), Dev(env, visits)
    store.record((a.ptr, v.ptr, actions.shape[1]))
    ref.record(actions, visits, pos)
    env.synchronize()
    a.close()
    v.close()


def commit(env, store, ref, done, reason, outcome=None):
    bufs = [Dev(env, done), Dev(env, reason)] + ([Dev(env, outcome)] if outcome is not None else [])
    store.commit(bufs[0].ptr, reason=bufs[1].ptr, outcome=bufs[2].ptr if outcome is not None else None)
    ref.commit(done, reason, outcome)
    env.synchronize()
    for b in bufs:
        b.close()


def guarded(env, nbytes, byte=0xAB):
    return Dev(env, np.full(nbytes + GUARD, byte, dtype=np.uint8))


def back(env, dev, nbytes):
    from gym_chess_amd import _lib

    out = np.zeros(nbytes + GUARD, dtype=np.uint8)
    _lib.check(env._L.gc_env_copy(env._h, _lib.ptr(out), dev.ptr, ctypes.c_uint64(out.nbytes), 2))
    return out[:nbytes], out[nbytes:]


def raw_sample(env, store, rows, index=None, seed=0, draw=0, planes=None, dtype=1, row_stride=0, flags=1,
               dense=None, pi_stride=R.ROW, pi_index=None, pi=None, z=None, slot=None):
    from gym_chess_amd import _lib

    _lib.check(env._L.gc_replay_sample(store._h, rows, index, ctypes.c_uint64(seed), draw, planes, dtype,
                                       ctypes.c_int64(row_stride), flags, dense, ctypes.c_int64(pi_stride), pi_index,
                                       pi, z, slot))


# ----------------------------------------------------------------------------- 1. synthetic sequences
@pytest.fixture(scope="module")
def env8():
    env = make_env(8, 3)
    yield env
    env.close()


@pytest.mark.parametrize("games,cap,row_cap", [(5, 3, 3), (7, 64, 40), (5, 200, 200), (7, 200, 130)])
def test_synthetic_sequences(env8, games, cap, row_cap):
    """max_plies 4, capacity games * 4 (the ring wraps several times), episodes of 1-9 records with
    zero-visit rows and padding inside the rows, random done / reason / outcome: after every call
    every array of the store equals RefStore's"""
    env, MAXP = env8, 4
    rng = np.random.RandomState(games * 1000 + cap)
    store = env.sample_store(games=games, cap=cap, max_plies=MAXP, capacity=games * MAXP)
    ref = R.RefStore(games, cap, MAXP, games * MAXP, alternate=True, fill=0xAB)
    fill_store(env, store)
    pos = host_positions(env, games)
    target = rng.randint(1, 10, size=games)
    for call in range(36):
        actions = np.stack([rng.choice(4100, size=row_cap, replace=False) for _ in range(games)]).astype(np.uint16)
        visits = rng.randint(0, 1 << 20, size=(games, row_cap)).astype(np.int32)
        hole = rng.rand(games, row_cap) < 0.3  # padding anywhere in the row
        actions[hole], visits[hole] = NONE, 0
        visits[rng.rand(games) < 0.2] = 0  # roots without visits
        record(env, store, ref, actions, visits, pos)
        ref.same_as(store.fetch(), pos_mask=R.W7_KNOWN)
        done = ((ref.plies >= target) | (rng.rand(games) < 0.1)).astype(np.uint8)
        reason = rng.choice([0, 1, 2, 3, 8], size=games).astype(np.uint8)
        outcome = rng.choice([-1.0, -0.0, 0.0, 0.5, 1.0], size=games).astype(np.float32) if call % 3 == 2 else None
        target[done != 0] = rng.randint(1, 10, size=int(done.sum()))
        commit(env, store, ref, done, reason, outcome)
        ref.same_as(store.fetch(), pos_mask=R.W7_KNOWN)
    c = store.counters()
    assert c == {"total": ref.total, "live": ref.live, "plies": int(ref.plies.sum()), "dropped": int(ref.dropped.sum())}
    assert ref.total > 3 * ref.R and ref.dropped.sum() > 0 and (ref.ring_z != 0).any()
    assert store.device_bytes() >= ref.R * (68 + 6 * cap)
    store.clear()
    got = store.fetch()
    assert all(not a.any() for a in got.values())
    assert store.counters() == {"total": 0, "live": 0, "plies": 0, "dropped": 0}
    store.close()


# ----------------------------------------------------------------------------- 2. planes
COMBOS = [(d, lay, p) for d in PL.DTYPES for lay in PL.LAYOUTS for p in (False, True)]


def _capture(env, n):
    """encode_planes' raw bytes [n][1536 * item] per (dtype, layout, view), now"""
    out = {}
    for d, lay, p in COMBOS:
        buf = env.planes_buffer(dtype=d, layout=lay)
        env.encode_planes(buf, perspective=p)
        out[(d, lay, p)] = as_bytes(buf.raw())[:n].copy()
        buf.close()
    return out


def _want(env, n):
    b, m = env.boards()
    rep = rep_counts(env, b)[0]
    return {(lay, p): PL.ref_planes(b, m, rep, env.en_passant(), p, lay)[:n] for lay in PL.LAYOUTS for p in (False, True)}


def _one(env, store, n, caps, wants):
    """one record of every game with a dummy root, its planes captured"""
    a = Dev(env, np.full((n, 1), 7, dtype=np.uint16))
    v = Dev(env, np.ones((n, 1), dtype=np.int32))
    caps.append(_capture(env, n))
    wants.append(_want(env, n))
    store.record((a.ptr, v.ptr, 1))
    env.synchronize()
    a.close()
    v.close()


@pytest.fixture(scope="module")
def recorded():
    """three stores whose ring holds known positions, with encode_planes' bytes and ref_planes at
    record time; the envs are changed afterwards, so a sample cannot come from the env:
      weird   130 weird random boards, both colours to move, spread move counts
      shuffle 8 boards stepped through knight shuffles, recorded at plies 3..8 (3-fold counts 0, 1, 2)
      fide    a FIDE env with en-passant targets"""
    from gym_chess_amd import codec as C
    from gym_chess_amd.env import BatchedChessEnv

    out = {}

    def finish(name, env, store, n, caps, wants, fide=False):
        done = Dev(env, np.ones(n, dtype=np.uint8))
        store.commit(done.ptr, reason=done.ptr)
        env.reset(states=False)  # the env moves on
        plies = len(caps)  # slot g * plies + p holds record p of game g
        cap = {k: np.stack([c[k] for c in caps], axis=1).reshape(n * plies, -1) for k in caps[0]}
        want = {k: np.stack([w[k] for w in wants], axis=1).reshape((n * plies,) + wants[0][k].shape[1:]) for k in wants[0]}
        out[name] = dict(env=env, store=store, live=n * plies, cap=cap, want=want, done=done)

    env = make_env(130, 3)
    b, m = env.boards()
    assert 30 <= int(m[:, 0].sum()) <= 100 and len(set(m[:, 7].tolist())) > 40
    store = env.sample_store(cap=3, max_plies=1, capacity=130)
    caps, wants = [], []
    _one(env, store, 130, caps, wants)
    finish("weird", env, store, 130, caps, wants)

    env = BatchedChessEnv(8, device=0, seed=1)
    store = env.sample_store(cap=3, max_plies=6, capacity=48)
    cyc = [C.str_to_action(s) for s in ("g1f3", "g8f6", "f3g1", "f6g8")]
    caps, wants = [], []
    for ply in range(8):
        rw, dn, why = env.step(np.full(8, cyc[ply % 4]))
        assert not dn.any()
        if ply >= 2:
            _one(env, store, 8, caps, wants)
    seen = {(bool(w[("nchw", False)][0, 20, 0, 0]), bool(w[("nchw", False)][0, 21, 0, 0])) for w in wants}
    assert seen == {(False, False), (True, False), (True, True)}
    finish("shuffle", env, store, 8, caps, wants)

    env = BatchedChessEnv(3, device=0, seed=2, rules="fide")
    env.set_fens(FENS)
    assert env.en_passant().tolist() == [4, 3, -1]
    store = env.sample_store(cap=3, max_plies=1, capacity=3)
    caps, wants = [], []
    _one(env, store, 3, caps, wants)
    assert wants[0][("nchw", False)][:2, 22].sum() == 2
    finish("fide", env, store, 3, caps, wants)

    yield out
    for s in out.values():
        s["done"].close()
        s["store"].close()
        s["env"].close()


@pytest.mark.parametrize("dtype", PL.DTYPES)
@pytest.mark.parametrize("name", ["weird", "shuffle", "fide"])
def test_planes_equal_encode_planes_at_record_time(recorded, name, dtype):
    """explicit index (a permutation, duplicates and two slots out of range), both layouts and
    views, row_stride 1544: every row equals encode_planes' bytes captured at record time and
    ref_planes; the stride's padding and a 4 KiB guard keep their 0xA5"""
    s = recorded[name]
    env, store, live = s["env"], s["store"], s["live"]
    rng = np.random.RandomState(5)
    index = np.concatenate([rng.permutation(live), rng.randint(live, size=7), [live, -1]]).astype(np.int32)
    rows, stride, item = index.size, 1544, ITEM[dtype]
    ok = (index >= 0) & (index < live)
    idx = Dev(env, index)
    for layout in PL.LAYOUTS:
        for persp in (False, True):
            buf = guarded(env, rows * stride * item, 0xA5)
            raw_sample(env, store, rows, index=idx.ptr, planes=buf.ptr, dtype=env.POLICY_DTYPES[dtype],
                       row_stride=stride, flags=env.PLANES_LAYOUTS[layout] | int(persp))
            got, guard = back(env, buf, rows * stride * item)
            got = got.reshape(rows, stride * item)
            used = ELEMS * item
            key = (dtype, layout, persp)
            assert (got[ok, :used] == s["cap"][key][index[ok]]).all(), key
            exp = as_bytes(PL.encode_raw(s["want"][(layout, persp)].reshape(live, ELEMS), dtype))
            assert (got[ok, :used] == exp[index[ok]]).all(), key
            assert not got[~ok, :used].any(), "a slot out of range gives a zero row"
            assert (got[:, used:] == 0xA5).all(), "the padding between rows was written"
            assert (guard == 0xA5).all(), "the guard behind the buffer was written"
            buf.close()
    idx.close()


def test_wrapper_sample_fetch(recorded):
    """SampleStore.sample(): its own buffers, a planes_buffer and an uploaded index"""
    s = recorded["weird"]
    env, store = s["env"], s["store"]
    index = np.arange(129, -1, -1)
    b = store.sample(130, index=index, dtype="float32", layout="nhwc", perspective=True)
    got = b.fetch()
    assert (got["slot"] == index).all()
    assert (got["planes"][:, :ELEMS].reshape(130, 8, 8, 24) == s["want"][("nhwc", True)][index]).all()
    assert got["pi_dense"].shape == (130, 4100) and (got["pi_dense"].sum(axis=1) == 1).all()
    pb = env.planes_buffer(dtype="bfloat16", rows=130)
    b = store.sample(130, index=index, planes=pb, perspective=False, dense=False)
    assert "pi_dense" not in b.ptr
    assert (pb.fetch() == s["want"][("nchw", False)][index]).all()
    pb.close()
    with pytest.raises(ValueError):
        store.sample(4, index=[0, 1])


# ----------------------------------------------------------------------------- 3. targets
@pytest.fixture(scope="module")
def targets(env8):
    """a store of 8 games x 3 plies at cap 200 (four lane chunks) over both colours to move, with an
    action that has no logits-row element; RefStore alongside"""
    env, G, CAP, PLIES = env8, 8, 200, 3
    rng = np.random.RandomState(17)
    store = env.sample_store(games=G, cap=CAP, max_plies=PLIES, capacity=G * PLIES + 5)
    ref = R.RefStore(G, CAP, PLIES, G * PLIES + 5)
    pos = host_positions(env, G)
    assert 2 <= sum(int(w[7]) & 1 for w in pos) <= 6  # both colours
    for t in range(PLIES):
        n = rng.choice([1, 63, 64, 65, 130, 200], size=G)
        actions = np.full((G, CAP), NONE, dtype=np.uint16)
        visits = np.zeros((G, CAP), dtype=np.int32)
        for g in range(G):
            actions[g, : n[g]] = rng.choice(4100, size=n[g], replace=False)
            visits[g, : n[g]] = rng.randint(0, 1 << 22, size=n[g])
            visits[g, 0] += 1
        actions[0, 0] = 4100  # RESIGN: no element of a logits row
        actions[1, :4] = [4096, 4097, 4098, 4099]
        record(env, store, ref, actions, visits, pos)
    commit(env, store, ref, np.ones(G, dtype=np.uint8), rng.choice([1, 2], size=G).astype(np.uint8))
    yield env, store, ref
    store.close()


@pytest.mark.parametrize("persp", [False, True])
def test_targets(targets, persp):
    env, store, ref = targets
    CAP, live = ref.cap, ref.live
    index = np.concatenate([np.arange(live), [live, ref.R, -5, 2 ** 31 - 1]]).astype(np.int32)
    rows, stride = index.size, 4104
    idx = Dev(env, index)
    dense, pidx, pi = guarded(env, rows * stride * 4), guarded(env, rows * CAP * 4), guarded(env, rows * CAP * 4)
    z, slot = guarded(env, rows * 4), guarded(env, rows * 4)
    raw_sample(env, store, rows, index=idx.ptr, flags=int(persp), dense=dense.ptr, pi_stride=stride,
               pi_index=pidx.ptr, pi=pi.ptr, z=z.ptr, slot=slot.ptr)
    got = {}
    for k, (buf, dt, shape) in {"pi_dense": (dense, np.float32, (rows, stride)), "pi_index": (pidx, np.int32, (rows, CAP)),
                                "pi": (pi, np.float32, (rows, CAP)), "z": (z, np.float32, (rows,)),
                                "slot": (slot, np.int32, (rows,))}.items():
        data, guard = back(env, buf, int(np.prod(shape)) * 4)
        assert (guard == 0xAB).all(), k
        got[k] = data.view(dt).reshape(shape)
        buf.close()
    idx.close()
    want = ref.sample(rows, index=index, perspective=persp)
    assert (got["slot"] == want["slot"]).all() and (want["slot"][-4:] == -1).all()
    assert got["z"].tobytes() == want["z"].tobytes()
    assert (got["pi_index"] == want["pi_index"]).all()
    mirrored = 0
    for j in range(rows):
        s = int(want["slot"][j])
        if s < 0:
            assert (got["pi_index"][j] == -1).all() and not got["pi"][j].any() and not got["pi_dense"][j, :R.ROW].any()
            continue
        _, meta8, _, _, n = R.unpack_pos(ref.ring_pos[s])
        vis = ref.ring_vis[s, :n].astype(np.float64)
        on = got["pi_index"][j] >= 0
        q = np.where(on[:n], vis / vis.sum(), 0.0)
        assert (np.abs(got["pi"][j, :n] - q) <= 2.0 ** -22 * q).all(), j
        assert not got["pi"][j, n:].any() and (got["pi_index"][j, n:] == -1).all()
        a = ref.ring_act[s, :n].astype(np.int64)
        plain = np.where(a < R.ROW, a, -1)
        if persp and not meta8[0]:
            assert (got["pi_index"][j, :n] == np.where(a < R.ROW, PL.mirror_action(a), -1)).all()
            mirrored += 1
        else:
            assert (got["pi_index"][j, :n] == plain).all()
        d = np.zeros(R.ROW, dtype=np.float32)  # the dense row = the sparse row scattered into zeros
        d[got["pi_index"][j][on]] = got["pi"][j][on]
        assert got["pi_dense"][j, :R.ROW].tobytes() == d.tobytes(), j
    assert (got["pi_dense"][:, R.ROW:].view(np.uint32) == 0xABABABAB).all(), "the stride's padding was written"
    assert (got["pi"] == want["pi"]).all()  # and the fp32 quotient bit for bit
    assert (mirrored > 0) == persp
    assert (got["pi_index"][want["slot"] == 0][0][0] == -1) and got["pi"][want["slot"] == 0][0][0] == 0  # action 4100


# ----------------------------------------------------------------------------- 4. drawn sampling
def test_drawn_sampling(targets):
    env, store, ref = targets
    rows = 300
    first = None
    for draw in (0, 1, 1):
        b = store.sample(rows, seed=99, draw=draw, dtype="float16", perspective=True)
        got = b.fetch()
        want = R.drawn_slots(rows, 99, draw, ref.live)
        assert (got["slot"] == want).all(), draw
        exp = ref.sample(rows, index=want, perspective=True)
        assert got["z"].tobytes() == exp["z"].tobytes() and (got["pi_dense"] == exp["pi_dense"]).all()
        if draw == 1 and first is not None:
            assert all(first[k].tobytes() == got[k].tobytes() for k in got), "a drawn batch is repeatable"
        first = got if draw == 1 else None
    assert len(set(R.drawn_slots(rows, 99, 0, ref.live).tolist())) == ref.live  # every slot is drawn
    assert (R.drawn_slots(rows, 99, 0, ref.live) != R.drawn_slots(rows, 99, 1, ref.live)).any()
    b = store.sample(5, draw=3)  # seed None = the env's
    assert (b.fetch("slot")["slot"] == R.drawn_slots(5, env.seed, 3, ref.live)).all()


def test_empty_store_gives_zero_rows(env8):
    env = env8
    store = env.sample_store(games=4, cap=5, max_plies=2, capacity=8)
    a, v = Dev(env, np.full((4, 5), 9, dtype=np.uint16)), Dev(env, np.ones((4, 5), dtype=np.int32))
    store.record((a.ptr, v.ptr, 5))  # pending samples are not live
    for index in (None, [0, 1, 7, -1, 8, 100]):
        b = store.sample(6, index=index, seed=4, dtype="float32")
        for k in b.ptr:
            dt, shape = b._spec[k]
            fill(env, b.ptr[k], int(np.prod(shape)) * np.dtype(dt).itemsize)
        b = store.sample(6, index=index, seed=4, dtype="float32")
        got = b.fetch()
        assert (got["slot"] == -1).all() and not got["z"].any() and not got["planes"].any()
        assert (got["pi_index"] == -1).all() and not got["pi"].any() and not got["pi_dense"].any()
    assert store.counters() == {"total": 0, "live": 0, "plies": 4, "dropped": 0}
    store.close()
    a.close()
    v.close()


# ----------------------------------------------------------------------------- 5. end to end
MATE_IN_1 = {"none": ("rnbqkbnr/pppp1ppp/8/4p3/6P1/5P2/PPPPP2P/RNBQKBNR b KQkq - 0 2", "d8h4"),
             "random": ("r1bqkb1r/pppp1ppp/2n2n2/4p2Q/2B1P3/8/PPPP1PPP/RNB1K1NR w KQkq - 0 4", "h5f7")}


@pytest.mark.parametrize("opponent", ["none", "random"])
def test_end_to_end_with_chess(opponent):
    """6 games, uniform "visits" over the legal moves, the picks played by step_device(autoreset),
    record before and commit after every ply.  Game 0 starts one move before a mate (reason 1).
    opponent "none": game 1 shuffles its knights into a 3-fold repetition (reason 2); "random": the
    games start late, so some reach the move cap (reason 3).  Every committed sample's z is the
    alternating (none) or constant (random) sign of its game's result and its position the one
    played, by host readbacks; RefStore follows the whole run."""
    from gym_chess_amd import codec as C
    from gym_chess_amd.env import BatchedChessEnv
    from gym_chess_amd.fen import fen_to_arrays

    G, CAP, MAXP, PLIES = 6, 64, 12, 16
    rng = np.random.RandomState(3)
    env = BatchedChessEnv(G, device=0, seed=8, opponent=opponent)
    fen, mate = MATE_IN_1[opponent]
    if opponent == "random":
        env.step_random(146)  # late games: the move cap (150 moves) falls inside the run
    b, m = env.boards()
    b[0], m[0] = fen_to_arrays(fen)
    env.set_states(b, m)
    io = env.device_io(mask=False, obs=False, count=False, pick=False)
    store = env.sample_store(cap=CAP, max_plies=MAXP, capacity=G * MAXP)
    ref = R.RefStore(G, CAP, MAXP, G * MAXP, alternate=opponent == "none")
    cyc = [C.str_to_action(s) for s in ("g1f3", "g8f6", "f3g1", "f6g8")]
    episodes = [[] for _ in range(G)]  # per game the boards of the running episode
    finished = []  # (boards, reason, first ring slot)
    for ply in range(PLIES):
        lm = env.legal_mask()
        bd, mt = env.boards()
        pos = host_positions(env, G)
        actions = np.full((G, CAP), NONE, dtype=np.uint16)
        visits = np.zeros((G, CAP), dtype=np.int32)
        picks = np.zeros(G, dtype=np.uint16)
        for g in range(G):
            legal = np.flatnonzero(lm[g, :4100])[:CAP]
            assert legal.size > 0
            actions[g, : legal.size], visits[g, : legal.size] = legal, 1
            picks[g] = rng.choice(legal)
            episodes[g].append((bd[g].copy(), mt[g].copy()))
        if ply == 0:
            picks[0] = C.str_to_action(mate)
        if opponent == "none" and ply < 9:
            picks[1] = cyc[ply % 4]
        assert all(picks[g] in actions[g] for g in range(G))
        pk = Dev(env, picks)
        record(env, store, ref, actions, visits, pos)
        env.step_device(io, actions=pk.ptr, autoreset=True)
        store.commit(io)
        out = io.fetch("done", "reason")
        before = ref.total
        ref.commit(out["done"], out["reason"])
        pk.close()
        assert not np.isin(out["reason"], (5, 6, 7)).any(), out["reason"]
        for g in range(G):
            if out["done"][g]:
                finished.append((episodes[g], int(out["reason"][g]), before + int(ref.off[g])))
                episodes[g] = []
        ref.same_as(store.fetch(), pos_mask=R.W7_KNOWN)
    reasons = [f[1] for f in finished]
    assert 1 in reasons and any(r != 1 for r in reasons), reasons
    assert ref.total <= ref.R  # nothing was overwritten: every finished episode is still in the ring
    got = store.fetch("ring_pos", "ring_z")
    for boards, reason, first in finished:
        result = {1: 1.0, 8: -1.0}.get(reason, 0.0)
        n = len(boards)
        assert n <= MAXP
        for p, (bd, mt) in enumerate(boards):
            flip = opponent == "none" and ((n - 1 - p) & 1)
            z = got["ring_z"][first + p]
            assert z == (-result if flip else result) and not (result == 0 and np.signbit(z)), (reason, p)
            gb, gm, _, _, _ = R.unpack_pos(got["ring_pos"][first + p])
            assert (gb == bd).all() and (gm == mt).all(), (reason, p)
    if opponent == "random":
        assert all(mt[0] == 1 for boards, _, _ in finished for _, mt in boards)  # every sample is the agent's
    store.close()
    io.close()
    env.close()


# ----------------------------------------------------------------------------- 6. argument errors
def test_argument_errors(env8):
    from gym_chess_amd import _lib

    env, L = env8, env8._L
    G, CAP = 4, 8
    store = env.sample_store(games=G, cap=CAP, max_plies=2, capacity=8)
    r = store._h
    a, v = Dev(env, np.full((G, CAP), 5, dtype=np.uint16)), Dev(env, np.ones((G, CAP), dtype=np.int32))
    done = Dev(env, np.ones(G, dtype=np.uint8))
    buf = Dev(env, np.zeros(16 * 4200 * 4 + 64, dtype=np.uint8))
    assert buf.ptr % 16 == 0

    def refused(fn, *args):
        with pytest.raises(_lib.GymChessError) as ei:
            _lib.check(fn(*args))
        assert str(ei.value), args

    h = ctypes.c_void_p()
    c64 = ctypes.c_int64
    for args in ((None, G, CAP, 2, c64(8), ctypes.byref(h)), (env._h, G, CAP, 2, c64(8), None),
                 (env._h, 0, CAP, 2, c64(8), ctypes.byref(h)), (env._h, env.num_boards + 1, CAP, 2, c64(64), ctypes.byref(h)),
                 (env._h, G, 0, 2, c64(8), ctypes.byref(h)), (env._h, G, 257, 2, c64(8), ctypes.byref(h)),
                 (env._h, G, CAP, 0, c64(8), ctypes.byref(h)), (env._h, G, CAP, 2, c64(7), ctypes.byref(h)),
                 (env._h, G, CAP, 2, c64(2 ** 31), ctypes.byref(h))):
        refused(L.gc_replay_create, *args)
    assert not h.value
    with pytest.raises(_lib.GymChessError):
        env.sample_store(games=env.num_boards + 1)

    store.record((a.ptr, v.ptr, CAP))
    before = store.fetch()

    def untouched():
        now = store.fetch()
        assert all(before[k].tobytes() == now[k].tobytes() for k in before)

    for args in ((None, a.ptr, v.ptr, CAP), (r, None, v.ptr, CAP), (r, a.ptr, None, CAP), (r, a.ptr, v.ptr, CAP + 1),
                 (r, a.ptr, v.ptr, 0)):
        refused(L.gc_replay_record, *args)
    for args in ((None, done.ptr, done.ptr, None), (r, None, done.ptr, None), (r, done.ptr, None, None)):
        refused(L.gc_replay_commit, *args)
    ok = dict(rows=4, index=None, seed=1, draw=0, planes=buf.ptr, dtype=1, row_stride=0, flags=0, dense=buf.ptr,
              pi_stride=4100, pi_index=None, pi=None, z=None, slot=None)
    for bad in (dict(rows=-1), dict(dtype=3), dict(dtype=-1), dict(flags=4), dict(flags=-1), dict(row_stride=1535),
                dict(row_stride=1540), dict(planes=buf.ptr + 8), dict(pi_stride=4099), dict(pi_stride=4102),
                dict(dense=buf.ptr + 4)):
        with pytest.raises(_lib.GymChessError):
            raw_sample(env, store, **{**ok, **bad})
    with pytest.raises(_lib.GymChessError):
        _lib.check(L.gc_replay_sample(None, 4, None, ctypes.c_uint64(1), 0, None, 1, c64(0), 0, None, c64(4100), None,
                                      None, None, None))
    raw_sample(env, store, **{**ok, "rows": 0})
    raw_sample(env, store, **{**ok, "planes": None, "row_stride": 3, "dense": None, "pi_stride": 0})  # unused rules
    out = (ctypes.c_void_p * 12)()
    refused(L.gc_replay_pointers, r, out, 0)
    refused(L.gc_replay_pointers, r, None, 12)
    refused(L.gc_replay_pointers, None, out, 12)
    refused(L.gc_replay_counters, None, None, None, None, None)
    refused(L.gc_replay_clear, None)
    refused(L.gc_replay_destroy, None)
    assert L.gc_replay_device_bytes(None) == 0
    untouched()
    _lib.check(L.gc_replay_commit(r, done.ptr, None, v.ptr))  # an outcome needs no reason
    assert store.counters()["total"] == G
    store.close()
    for b in (a, v, done, buf):
        b.close()
