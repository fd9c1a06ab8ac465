"""GPU: the FIDE kernels against the independent reference (tests/fide_ref.py), never against the
host build of gc_fide.h.

  * Engine (k_flist, k_fnext_state, k_fupdate_state) on the depth-2 trees of the perft positions;
  * env.step (k_fenv_step<false>), step_device (k_fenv_step_api<false>) and step_boards (the FIDE
    body of gc_step_rows.h) on the scripted games of tests/fide_cases.py, one case per board, 130
    boards (a partial last block) cycling the table: reward, done, reason, every state byte, the
    en-passant file, the 4101-column mask (k_fmask's castle word included) and the lists;
  * the paired driver and the fused rollout (k_env_step2<FIDE>, k_env_rollout2<FIDE>, whose picks
    come from the set-wise generator fsw_*), followed ply by ply from reset and from set states;
  * the random opponent, both colours (fenv_step_vs, fenv_open_vs), through step and step_device:
    the agent's move, then the ONE legal reply that gives the device's board.
"""
import copy
import random
from collections import Counter

import numpy as np
import pytest

import fide_cases as FC
import fide_ref as F
from test_fide_ref import START, follow, walk_nodes

pytestmark = pytest.mark.gpu

N = 130  # two full blocks of 64 and a partial one
START_ENV = F.to_env(START, 0)


def mask_bits(raw):
    n = raw.shape[0]
    bits = np.unpackbits(raw[:, :64].view(np.uint8).reshape(n, 64, 8), axis=2, bitorder="little")
    out = np.zeros((n, 4101), dtype=bool)
    out[:, :4096] = bits.reshape(n, 4096).astype(bool)
    for c in range(5):
        out[:, 4096 + c] = (raw[:, 64] >> np.uint64(c)) & np.uint64(1) != 0
    assert (raw[:, 64] >> np.uint64(5) == 0).all()
    return out


def legal_matrix(lists):
    out = np.zeros((len(lists), 4101), dtype=bool)
    for i, l in enumerate(lists):
        out[i, l] = True
    return out


def assert_list_form(lst, legal, where):
    """a device list: the legal set, each id once, moves in ascending id, castles last"""
    assert len(lst) == len(legal) and set(lst) == set(legal), (where, lst, legal)
    moves = [a for a in lst if a < 4096]
    assert moves == sorted(moves) and lst[:len(moves)] == moves, (where, lst)


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def walk():
    """the tree-walk nodes as engine inputs, their legal lists, and every (node, move) pair of
    depths 0 and 1 with the reference's next state -- computed once"""
    nodes = walk_nodes()
    states = [F.to_engine(st) for st, _ in nodes]
    legal = [F.legal_actions(st) for st, _ in nodes]
    pairs = [(i, a) for i, (st, d) in enumerate(nodes) if d < 2 for a in legal[i]]
    nxt = [F.apply(nodes[i][0], a) for i, a in pairs]
    return dict(nodes=nodes, b=np.stack([s[0] for s in states]), m=np.stack([s[1] for s in states]), legal=legal,
                pairs=pairs, nb=np.stack([F.to_engine(s)[0] for s, _ in nxt]),
                nm=np.stack([F.to_engine(s)[1] for s, _ in nxt]), rw=np.array([r for _, r in nxt], dtype=np.int32))


@pytest.fixture(scope="module")
def engine():
    from gym_chess_amd.engine import Engine

    eng = Engine(0, rules="fide")
    yield eng
    eng.close()


def test_engine_lists_on_the_tree_walk(engine, walk):
    moves, cnt = engine.possible_moves(walk["b"], walk["m"], walk["m"][:, 0])
    assert len(cnt) == 10557
    for i, legal in enumerate(walk["legal"]):
        assert cnt[i] == len(legal), i
        assert_list_form([int(x) for x in moves[i, :cnt[i]]], legal, i)


def test_engine_next_state_on_the_tree_walk(engine, walk):
    idx = np.array([i for i, _ in walk["pairs"]])
    acts = np.array([a for _, a in walk["pairs"]], dtype=np.uint16)
    ob, om, rw, st = engine.next_state(walk["b"][idx], walk["m"][idx], walk["m"][idx, 0], acts)
    assert (st == 0).all()
    for name, got, exp in (("board", ob, walk["nb"]), ("meta8", om, walk["nm"]), ("reward", rw, walk["rw"])):
        bad = np.nonzero((got != exp).reshape(len(idx), -1).any(axis=1))[0]
        assert not len(bad), (name, [(walk["b"][idx[k]].tolist(), walk["m"][idx[k]].tolist(), int(acts[k]),
                                      got[k].tolist(), exp[k].tolist()) for k in bad[:3]])


def test_engine_next_state_status(engine):
    """status -1 for an empty from-square and for an enemy piece's; an id that is no move
    (4100) never reaches the kernel's -2: the C-ABI refuses the call"""
    from gym_chess_amd import _lib

    b, m = F.to_engine(START)
    acts = np.array([20 * 64 + 28, 8 * 64 + 16, 52 * 64 + 36], dtype=np.uint16)  # empty, enemy's, e2e4
    _, _, _, st = engine.next_state(np.stack([b] * 3), np.stack([m] * 3), 1, acts)
    assert st.tolist() == [-1, -1, 0]
    with pytest.raises(_lib.GymChessError):
        engine.next_state(b[None], m[None], 1, np.array([4100], dtype=np.uint16))


def test_engine_update_state_flags(engine, walk):
    cleared = walk["m"].copy()
    cleared[:, 5:7] = 0
    ob, om = engine.update_state(walk["b"], cleared)
    assert (ob == walk["b"]).all() and (om == walk["m"]).all()
    assert walk["m"][:, 5].sum() > 50 and walk["m"][:, 6].sum() > 50  # checked kings of both colours


# ------------------------------------------------------------------ scripted games on the env
def scripted(probes):
    tls = FC.timelines(probes)
    cols = [tls[i % len(tls)] for i in range(N)]
    return cols, FC.padded(cols)


def new_env(cols, **kw):
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(len(cols), device=0, seed=3, rules="fide", **kw)
    env.set_states(np.stack([t.start[0] for t in cols]), np.stack([t.start[1] for t in cols]),
                   en_passant=np.array([t.start[2] for t in cols], dtype=np.int8))
    return env


def assert_state(env, P, p, cols):
    b, m = env.boards()
    for name, got, exp in (("board", b, P["board"][p]), ("meta8", m, P["meta8"][p]), ("ep", env.en_passant(), P["ep"][p])):
        bad = np.nonzero((got != exp).reshape(len(cols), -1).any(axis=1))[0]
        assert not len(bad), (p, name, [(cols[i].name, got[i].tolist(), exp[i].tolist()) for i in bad[:3]])


def assert_outputs(rw, dn, why, P, p, cols):
    for name, got, exp in (("reward", rw, P["reward"][p]), ("done", np.asarray(dn) != 0, P["done"][p]),
                           ("reason", why, P["reason"][p])):
        bad = np.nonzero(np.asarray(got) != exp)[0]
        assert not len(bad), (p, name, [(cols[i].name, int(P["action"][p][i]), int(got[i]), int(exp[i])) for i in bad[:5]])


def test_env_step_scripted_games():
    cols, P = scripted(False)
    env = new_env(cols)
    for p in range(len(P["action"])):
        rw, dn, why = env.step(P["action"][p])
        assert_outputs(rw, dn, why, P, p, cols)
        assert_state(env, P, p, cols)
        legal = legal_matrix(P["legal"][p])
        got = env.legal_mask()
        assert (got == legal).all(), (p, [cols[i].name for i in np.nonzero((got != legal).any(axis=1))[0][:5]])
        for i, lst in enumerate(env.possible_actions()):
            assert_list_form(lst, P["legal"][p][i], (p, cols[i].name))
    env.close()


def test_env_step_device_scripted_games_with_invalid_actions():
    """the scripts with an invalid action in front of every move, through step_device: outputs,
    states, and the mask / obs / count / pick of the new state; then one auto-reset step: every
    board that reports done lands on the start position"""
    cols, P = scripted(True)
    env = new_env(cols)
    io = env.device_io(select=False)
    acts = env.device_io(mask=False, obs=False, count=False, pick=True, select=False)
    for p in range(len(P["action"])):
        acts.upload_actions(P["action"][p])
        env.step_device(io, actions=acts.ptr["pick"])
        o = io.fetch()
        assert_outputs(o["reward"], o["done"], o["reason"], P, p, cols)
        assert_state(env, P, p, cols)
        legal = legal_matrix(P["legal"][p])
        assert (mask_bits(o["mask"]) == legal).all(), p
        assert (o["obs"] == P["board"][p]).all() and (o["count"] == legal.sum(axis=1)).all(), p
        has = legal.any(axis=1)
        assert legal[np.nonzero(has)[0], o["pick"][has].astype(np.int64)].all(), p
        assert (o["pick"][~has] == 0xFFFF).all(), p
    # auto-reset: a legal action where one exists (reason 7 on a done board, 3 at the cap), else resign
    envs = [copy.deepcopy(t.env) for t in cols]
    last = [F.legal_actions(e.s) for e in envs]
    a = np.array([l[0] if l else F.A_RESIGN for l in last], dtype=np.uint16)
    exp = [e.step(int(x)) for e, x in zip(envs, a)]
    acts.upload_actions(a)
    env.step_device(io, actions=acts.ptr["pick"], autoreset=True)
    o = io.fetch()
    assert (o["reward"] == [x[0] for x in exp]).all() and (o["reason"] == [x[2] for x in exp]).all()
    assert ((o["done"] != 0) == [x[1] for x in exp]).all()
    assert sum(x[1] for x in exp) >= 20  # by the reference: the mated, repeated and capped games
    b, m = env.boards()
    ep = env.en_passant()
    start_legal = F.legal_actions(START)
    for i, e in enumerate(envs):
        wb, wm, wep = START_ENV if exp[i][1] else F.to_env(e.s, e.mc)
        assert (b[i] == wb).all() and (m[i] == wm).all() and ep[i] == wep, (i, cols[i].name)
        assert (o["obs"][i] == wb).all(), i
        want = start_legal if exp[i][1] else F.legal_actions(e.s)
        assert np.nonzero(mask_bits(o["mask"][i:i + 1])[0])[0].tolist() == want and o["count"][i] == len(want), i
    for x in (io, acts, env):
        x.close()


def test_step_boards_scripted_games():
    """the same scripts through step_boards: each ply the boards are stepped in two calls over a
    permuted, duplicate-free index list; the row-compact verdicts, counts and observations are the
    reference's, and a board not listed is untouched"""
    cols, P = scripted(False)
    env = new_env(cols)
    io = env.device_io(pick=False)
    rb = env.rows_buffer(N)
    rng = np.random.RandomState(17)
    prev_b = np.stack([t.start[0] for t in cols])
    for p in range(len(P["action"])):
        perm = rng.permutation(N)
        cut = int(rng.randint(1, N))
        for k, part in enumerate((perm[:cut], perm[cut:])):
            env.step_boards(io, part, P["action"][p][part], out=rb)
            o = rb.fetch()
            m = len(part)
            assert (o["reward"][:m] == P["reward"][p][part]).all(), (p, k)
            assert ((o["done"][:m] != 0) == P["done"][p][part]).all() and (o["reason"][:m] == P["reason"][p][part]).all(), (p, k)
            assert (o["obs"][:m] == P["board"][p][part]).all(), (p, k)
            assert (o["count"][:m] == [len(P["legal"][p][i]) for i in part]).all(), (p, k)
            if k == 0:  # the second part has not moved yet
                assert (env.boards()[0][perm[cut:]] == prev_b[perm[cut:]]).all(), p
        assert_state(env, P, p, cols)
        assert (mask_bits(io.fetch("mask")["mask"]) == legal_matrix(P["legal"][p])).all(), p
        prev_b = P["board"][p]
    for x in (rb, io, env):
        x.close()


# ------------------------------------------------------------------ the self-play drivers
def follow_all(trace, plies, firsts=None):
    """the reference follows every board's trace; -> the final reference envs and the counts"""
    envs, tot = [], Counter()
    for i in range(trace["action"].shape[1]):
        tr = {k: v[:, i] for k, v in trace.items()}
        env, seen = follow(tr, START, plies, first=firsts[i] if firsts else None)
        envs.append(env)
        tot += seen
    return envs, tot


def step_random_trace(env, plies):
    """one launch per ply of the paired one-ply step; the trace as rollout_device's"""
    n = env.num_boards
    tr = dict(action=np.zeros((plies, n), np.int32), reward=np.zeros((plies, n), np.int32),
              done=np.zeros((plies, n), np.uint8), reason=np.zeros((plies, n), np.uint8))
    for p in range(plies):
        played = env.outputs()["next_action"].astype(np.int32)
        env.step_random(1)
        o = env.outputs()
        tr["action"][p] = np.where(played == 0xFFFF, -1, played)
        for k in ("reward", "done", "reason"):
            tr[k][p] = o[k]
    return tr


def assert_final_states(env, refs):
    b, m = env.boards()
    ep = env.en_passant()
    for i, r in enumerate(refs):
        wb, wm, wep = F.to_env(r.s, r.mc)
        assert (b[i] == wb).all() and (m[i] == wm).all() and ep[i] == wep, i


def test_paired_step_random_followed_from_reset():
    """k_env_step2<FIDE>, 65 boards x 160 plies from reset, one launch per ply: every played
    action legal in the reference, reward / done / reason equal, no-move plies where the
    reference has no move; the final boards, meta and en-passant files are the reference's"""
    from gym_chess_amd.env import BatchedChessEnv

    n, plies = 65, 160
    env = BatchedChessEnv(n, device=0, seed=0xF1DE, rules="fide")
    tr = step_random_trace(env, plies)
    refs, tot = follow_all(tr, plies)
    assert tot[6] == 0 and tot[0] > n * plies * 0.9, tot
    assert_final_states(env, refs)
    env.close()


def test_fused_rollout_trace_followed_from_reset():
    """k_env_rollout2<FIDE> (rollout_device with a trace), 65 boards x 160 plies from reset"""
    from gym_chess_amd.env import BatchedChessEnv

    n, plies = 65, 160
    env = BatchedChessEnv(n, device=0, seed=0xBEEF, rules="fide")
    tb = env.trace_buffer(plies)
    env.rollout_device(plies, tb)
    env.synchronize()
    refs, tot = follow_all(tb.fetch(), plies)
    assert tot[6] == 0 and tot[0] > n * plies * 0.9, tot
    assert_final_states(env, refs)
    tb.close()
    env.close()


@pytest.mark.parametrize("fused", [False, True])
def test_drivers_followed_from_set_states(fused):
    """both drivers can start from set states (set_states, then select_random): one board per
    scripted case and mirror at its start position -- en-passant files, partial rights, move
    counts 148-150 -- for 40 plies; a finished episode goes on from the start position"""
    cols = FC.timelines()
    plies = 40
    env = new_env(cols)
    env.select_random()
    if fused:
        tb = env.trace_buffer(plies)
        env.rollout_device(plies, tb)
        env.synchronize()
        tr = tb.fetch()
        tb.close()
    else:
        tr = step_random_trace(env, plies)
    refs, tot = follow_all(tr, plies, firsts=[F.from_env(*t.start) for t in cols])
    assert tot[6] == 0 and tot[3] >= 6, tot  # no illegal move played; the six cap cases reach the cap
    assert_final_states(env, refs)
    env.close()


# ------------------------------------------------------------------ the random opponent
# (name, FEN with the agent to move, the agent's scripted moves); mirrored for a BLACK agent
OPP_CASES = [
    ("agent_mates", "6k1/5ppp/8/8/8/8/8/R5K1 w - - 0 1", ["a1a8"]),                        # reason 1
    ("only_reply_mates", "3r4/8/8/8/2N5/8/p2R2PP/k6K w - - 0 1", ["d2d1"]),                # reason 8: Rd1+ Rxd1#
    ("opponent_stalemated", "7k/5K2/8/6Q1/8/8/8/8 w - - 0 1", ["g5g6"]),                   # reason 9
    ("forced_shuffle", "k7/3P4/2K5/8/8/4B3/8/8 w - - 0 1", ["e3d4", "d4e3"] * 2 + ["e3d4"]),  # reason 2
    ("ep_and_castles", "r3k2r/1p1p1p1p/8/P1P1P1P1/p1p1p1p1/8/1P1P1P1P/R3K2R w KQkq - 0 1", []),
    ("start", F.STARTPOS, []),
]


def find_reply(board_after):
    """the opponent's reply = the one legal move whose result is the device's board"""
    def reply(env):
        hits = [a for a in F.legal_actions(env.s) if F.apply(env.s, a)[0].board == board_after]
        assert len(hits) == 1, hits
        return hits[0]
    return reply


@pytest.mark.parametrize("api", ["step", "step_device"])
@pytest.mark.parametrize("black", [False, True])
def test_random_opponent_against_the_reference(black, api):
    from gym_chess_amd.env import BatchedChessEnv

    n, plies = 70, 24
    env = BatchedChessEnv(n, device=0, seed=23, opponent="random", player_color="BLACK" if black else "WHITE",
                          rules="fide")
    start_board = list(START.board)
    refs = [F.RefEnv(START, opponent=True) for _ in range(n)]

    def opened(i, board):  # a BLACK agent's reset leaves one legal white opening played
        if black:
            refs[i].reset(opening=find_reply(np.asarray(board).tolist())(F.RefEnv(START)))
        else:
            refs[i].reset()

    b, m = env.boards()
    ep = env.en_passant()
    for i in range(n):
        opened(i, b[i])
    scripts = [[] for _ in range(n)]
    for i in range(n):  # the chosen positions on the first boards of every block, the rest from reset
        name, fen, script = OPP_CASES[i % 16] if i % 16 < len(OPP_CASES) else OPP_CASES[-1]
        if name == "start":
            continue
        st = F.from_fen(fen)
        refs[i].set(FC.mirror_state(st) if black else st, 0)
        scripts[i] = [FC.token_action(FC.mirror_token(t) if black else t) for t in script]
        b[i], m[i], ep[i] = F.to_env(refs[i].s, 0)
    env.set_states(b, m, en_passant=ep)
    if api == "step_device":
        io = env.device_io(pick=False, select=False)
        buf = env.device_io(mask=False, obs=False, count=False, pick=True, select=False)
    rng = random.Random(5)
    seen = Counter()
    for ply in range(plies):
        acts = np.zeros(n, dtype=np.uint16)
        for i, r in enumerate(refs):
            legal = F.legal_actions(r.s)
            acts[i] = scripts[i].pop(0) if scripts[i] else legal[rng.randrange(len(legal))] if legal else F.A_RESIGN
        if api == "step":
            rw, dn, why = env.step(acts)
        else:
            buf.upload_actions(acts)
            env.step_device(io, actions=buf.ptr["pick"])
            o = io.fetch()
            rw, dn, why = o["reward"], o["done"] != 0, o["reason"]
        b, m = env.boards()
        ep = env.en_passant()
        for i, r in enumerate(refs):
            exp = r.step(int(acts[i]), find_reply(b[i].tolist()))
            assert (int(rw[i]), bool(dn[i]), int(why[i])) == exp, (ply, i, int(acts[i]), exp)
            wb, wm, wep = F.to_env(r.s, r.mc)
            assert (b[i] == wb).all() and (m[i] == wm).all() and ep[i] == wep, (ply, i, m[i].tolist(), wm.tolist())
            seen[exp[2]] += 1
        if api == "step_device":
            assert (o["obs"] == b).all(), ply
            assert (mask_bits(o["mask"]) == legal_matrix([F.legal_actions(r.s) for r in refs])).all(), ply
        if dn.any():
            env.reset(dn.astype(np.uint8), states=False)
            b, m = env.boards()
            for i in np.nonzero(dn)[0]:
                opened(i, b[i])
                wb, wm, wep = F.to_env(refs[i].s, refs[i].mc)
                assert (b[i] == wb).all() and (m[i] == wm).all() and env.en_passant()[i] == wep, (ply, i)
    assert all(seen[r] >= 4 for r in (1, 8, 9, 2)) and seen[0] > n * plies * 0.8, seen
    env.close()
