"""GPU: the HIP kernels against the reference's own v1 engine on fuzzed boards
(tests/golden/v1_fuzz.json.gz; tests/test_v1_fuzz.py describes it and pins the oracle and the host
build of the core to it).  Everything here is compared with the FIXTURE, never with the oracle:
a misreading shared by the oracle and the kernels cannot pass.

About 1 000 positions and 16 000 (position, move) pairs: one engine call (or one env of one
board per position) per test, so each takes seconds."""
import numpy as np
import pytest

from test_api_step import _mask_bits
from test_v1_fuzz import load_fuzz

pytestmark = pytest.mark.gpu


def build_fx():
    """the fixture as arrays: positions, and one row per (position, move) pair"""
    from gym_chess_amd import codec as C

    pos = load_fuzz()
    d = dict(pos=pos, boards=np.stack([b for _, b, _ in pos]), metas=np.stack([m for _, _, m in pos]))
    owner, acts, nxt, rew, flags = [], [], [], [], []
    for i, (e, _, _) in enumerate(pos):
        for a, t, r, fl in zip(e["moves"], e["next_boards"], e["rewards"], e["flags"]):
            owner.append(i)
            acts.append(a)
            nxt.append(C.text_to_board(t))
            rew.append(r)
            flags.append([-1, -1] if fl is None else fl)
    d.update(owner=np.array(owner), acts=np.array(acts, dtype=np.uint16), next=np.stack(nxt),
             rewards=np.array(rew), flags=np.array(flags))
    # capture value by piece type, read off the fixture's own (captured piece, reward) pairs
    value = {0: 0}
    for k in range(len(acts)):
        if acts[k] < 4096:
            value.setdefault(abs(int(d["boards"][owner[k]][acts[k] & 63])), rew[k])
    assert value == {0: 0, 2: 10, 3: 5, 4: 3, 5: 3, 6: 1}, value
    d["value"] = value
    return d


@pytest.fixture(scope="module")
def fx():
    return build_fx()


def _lists(out, cnt):
    return [[int(x) for x in out[i, : cnt[i]]] for i in range(len(cnt))]


# ------------------------------------------------------------------ engine
@pytest.mark.parametrize("chunk", [0, 1, 2, 257])
def test_possible_moves_ordered(engine, fx, chunk):
    """ordered lists, all positions in one call (a partial last block) and in calls of 1 (the
    engine server), 2 and 257 positions: every staging path sees fixture data"""
    b, m = fx["boards"], fx["metas"]
    n = len(b)
    step = chunk or n
    got = []
    for lo in range(0, n, step):
        out, cnt = engine.possible_moves(b[lo:lo + step], m[lo:lo + step], m[lo:lo + step, 0])
        got += _lists(out, cnt)
    for i, (e, _, _) in enumerate(fx["pos"]):
        assert got[i] == e["moves"], (chunk, i)


def test_next_state_every_listed_move(engine, fx):
    """every (position, move) pair in one call: boards, rewards and the status (0; 1 where v1 says
    both kings are checked afterwards, the reference's one error: D9)"""
    o = fx["owner"]
    nb, nm, rw, st = engine.next_state(fx["boards"][o], fx["metas"][o], fx["metas"][o, 0], fx["acts"])
    bad = np.nonzero((nb != fx["next"]).any(axis=1) | (rw != fx["rewards"]))[0]
    assert bad.size == 0, [(int(o[k]), int(fx["acts"][k])) for k in bad[:4]]
    known = fx["flags"][:, 0] >= 0
    both = (fx["flags"] == 1).all(axis=1)
    assert (st[known] == both[known]).all() and np.isin(st, (0, 1)).all()
    assert both.sum() < 0.01 * len(both)  # status 0 nearly everywhere
    # the new states' flags, where the status is 0 (the raise carries no state)
    ok = known & ~both
    assert (nm[ok, 5:7] == fx["flags"][ok]).all()
    assert (nm[:, 0] != fx["metas"][o, 0]).all()


def test_update_state_flags_of_next_boards(engine, fx):
    o = fx["owner"]
    m = fx["metas"][o].copy()
    m[:, 0] ^= 1
    ob, om = engine.update_state(fx["next"], m)
    known = fx["flags"][:, 0] >= 0
    assert known.sum() > 13000
    assert (ob == fx["next"]).all() and (om[known, 5:7] == fx["flags"][known]).all()


def test_perft_where_v1_equals_v2(engine, fx):
    """depths 1-3, all roots of a depth in one call"""
    for d in ("1", "2", "3"):
        idx = [i for i, (e, _, _) in enumerate(fx["pos"]) if e.get("v1_equals_v2") and d in e["v1_perft"]]
        assert len(idx) >= (40 if d == "3" else 250)
        got = engine.perft(fx["boards"][idx], fx["metas"][idx], int(d))
        want = np.array([fx["pos"][i][0]["v1_perft"][d] for i in idx], dtype=np.uint64)
        assert (got == want).all(), (d, [idx[k] for k in np.nonzero(got != want)[0][:4]])


def test_perft_divergences_are_king_captures(engine, fx):
    """where v1 != v2 (D1): every v2-only move of the fixture's walk is in the device's list and
    lands on the enemy king"""
    from gym_chess_amd import codec as C

    divs = [dv for e, _, _ in fx["pos"] if e.get("v1_equals_v2") is False for dv in e["d1_divergences"]]
    assert len(divs) >= 50
    b = np.stack([C.text_to_board(dv["board"]) for dv in divs])
    m = np.zeros((len(divs), 8), dtype=np.uint8)
    m[:, 0] = [dv["white"] for dv in divs]
    out, cnt = engine.possible_moves(b, m, m[:, 0])
    for k, (dv, lst) in enumerate(zip(divs, _lists(out, cnt))):
        assert dv["v2_only"] and set(dv["v2_only"]) <= set(lst), k
        assert all(b[k][a & 63] == (-1 if dv["white"] else 1) for a in dv["v2_only"]), k


# ------------------------------------------------------------------ env
def _played(fx):
    """per board: the index of the move to play, cycling through the first move, the last move and
    a castle where there is one (-1: an empty list, nothing to play); the few boards with a mating
    move play that one, so that the WIN reward is seen too"""
    idx = []
    for i, (e, _, _) in enumerate(fx["pos"]):
        mv = e["moves"]
        castles = [k for k, a in enumerate(mv) if a >= 4096]
        mates = [k for k, (c, fl) in enumerate(zip(e["next_n"], e["flags"]))
                 if c == 0 and fl is not None and fl[1 if e["white"] else 0]]
        idx.append(-1 if not mv else castles[0] if castles and i % 3 == 2 else mates[0] if mates
                   else len(mv) - 1 if i % 3 else 0)
    return idx


def build_plan(fx):
    """the actions to play and what the fixture says must come out (opponent "none"): the
    reference's reward rule (chess_v2.py:260-272) over the recorded capture value"""
    from gym_chess_amd import codec as C

    n = len(fx["pos"])
    p = dict(acts=np.full(n, C.A_RESIGN, dtype=np.uint16), obs=fx["boards"].copy(), reward=np.zeros(n, dtype=np.int64),
             reason=np.full(n, 6), flags=np.full((n, 2), -1), count=np.full(n, -1), sure=np.ones(n, dtype=bool),
             both=np.zeros(n, dtype=bool), cap=np.zeros(n, dtype=np.int64), idx=_played(fx))
    p["reward"][:] = C.INVALID_ACTION_REWARD  # an empty list: RESIGN is an invalid action, the state stays
    for i, (e, b, m) in enumerate(fx["pos"]):
        j = p["idx"][i]
        if j < 0:
            p["count"][i] = 0
            continue
        fl, cnt = e["flags"][j], e["next_n"][j]
        p["acts"][i] = e["moves"][j]
        p["obs"][i] = C.text_to_board(e["next_boards"][j])
        p["cap"][i] = e["rewards"][j]
        if fl is None or cnt is None:  # v1 could not say whether the other side is mated
            p["sure"][i] = False
            continue
        p["flags"][i] = fl
        p["both"][i] = fl[0] and fl[1]
        p["count"][i] = cnt
        mate = cnt == 0 and fl[1 if e["white"] else 0]
        p["reward"][i] = C.INVALID_ACTION_REWARD + e["rewards"][j] + (C.WIN_REWARD if mate else 0)
        p["reason"][i] = 1 if mate else 0
    assert p["sure"].sum() > 0.9 * n and (p["reason"] == 1).sum() >= 5 and (p["acts"] >= 4096).sum() >= 20
    return p


@pytest.fixture(scope="module")
def plan(fx):
    return build_plan(fx)


def _check_none(p, reward, done, reason, obs, count=None, flags=None):
    ok = p["sure"] & ~p["both"]
    assert (obs == p["obs"])[~p["both"]].all(), np.nonzero((obs != p["obs"]).any(axis=1) & ~p["both"])[0][:4]
    assert (reason[p["both"]] == 5).all()  # the engine's error ends the episode
    assert (reward[ok] == p["reward"][ok]).all(), np.nonzero((reward != p["reward"]) & ok)[0][:4]
    assert (reason[ok] == p["reason"][ok]).all() and (done[ok].astype(bool) == (p["reason"][ok] == 1)).all()
    if count is not None:
        assert (count[ok] == p["count"][ok]).all(), np.nonzero((count != p["count"]) & ok)[0][:4]
    if flags is not None:
        played = ok & (p["reason"] != 6)
        assert (flags[played] == p["flags"][played]).all()


def test_env_mask_and_lists(fx):
    """set_states with the fixture boards: legal_mask() (k_mask and the castle word) is the list
    as a set, possible_actions() the list in order"""
    from gym_chess_amd.env import BatchedChessEnv

    env = BatchedChessEnv(len(fx["pos"]), device=0, seed=3)
    env.set_states(fx["boards"], fx["metas"])
    mask, lists = env.legal_mask(), env.possible_actions()
    for i, (e, _, _) in enumerate(fx["pos"]):
        assert lists[i] == e["moves"], i
        assert np.nonzero(mask[i])[0].tolist() == sorted(e["moves"]), i
    env.close()


def test_env_one_step_per_board(fx, plan):
    """one step per board through step, step_device and step_boards (opponent "none"): the
    observation is v1's next board, the reward its capture value under the env's rule, the new
    state's check flags and move count v1's"""
    from gym_chess_amd.env import BatchedChessEnv

    n = len(fx["pos"])
    env = BatchedChessEnv(n, device=0, seed=3)
    env.set_states(fx["boards"], fx["metas"])
    rw, dn, why = env.step(plan["acts"])
    b, m = env.boards()
    _check_none(plan, rw, dn, why, b, flags=m[:, 5:7])
    played = plan["sure"] & ~plan["both"] & (plan["reason"] != 6)
    assert (m[played, 0] != fx["metas"][played, 0]).all()

    env.set_states(fx["boards"], fx["metas"])
    io = env.device_io(pick=False)
    act = env.device_io(mask=False, obs=False, count=False, pick=True, select=False)
    act.upload_actions(plan["acts"])
    env.step_device(io, actions=act.ptr["pick"])
    o = io.fetch()
    _check_none(plan, o["reward"], o["done"], o["reason"], o["obs"], count=o["count"])
    bits = _mask_bits(o["mask"])
    assert (bits.sum(axis=1) == o["count"]).all()

    env.set_states(fx["boards"], fx["metas"])
    rows = env.step_boards(io, np.arange(n), plan["acts"]).fetch()
    _check_none(plan, rows["reward"][:n], rows["done"][:n], rows["reason"][:n], rows["obs"][:n], count=rows["count"][:n])
    assert (_mask_bits(io.fetch("mask")["mask"]) == bits).all()
    for x in (io, act, env):
        x.close()


def test_env_agent_half_with_random_opponent(fx, plan):
    """opponent "random": the agent's half of the step is v1's -- the observation is the recorded
    next board with exactly one reply of the other side played on it, and the reward the recorded
    capture value under the env's rule less the reply's capture (chess_v2.py:276-288); a mate by
    the agent's move ends the step before any reply"""
    from gym_chess_amd import codec as C
    from gym_chess_amd.env import BatchedChessEnv

    n = len(fx["pos"])
    env = BatchedChessEnv(n, device=0, seed=3, opponent="random")
    env.set_states(fx["boards"], fx["metas"])
    rw, dn, why = env.step(plan["acts"])
    obs, _ = env.boards()
    replies = 0
    for i, (e, _, _) in enumerate(fx["pos"]):
        if plan["both"][i] or not plan["sure"][i]:
            continue
        if plan["reason"][i] in (1, 6) or plan["count"][i] == 0:  # no reply: mate, nothing played, no move to reply with
            assert (obs[i] == plan["obs"][i]).all(), i
            if plan["reason"][i] != 0:
                assert (rw[i], why[i]) == (plan["reward"][i], plan["reason"][i]), i
            continue
        nb, opp = plan["obs"][i], -1 if e["white"] else 1
        diff = np.nonzero(obs[i] != nb)[0]
        base = C.INVALID_ACTION_REWARD + plan["cap"][i] + (C.LOSS_REWARD if why[i] == 8 else 0)
        if why[i] == 5:  # the reply left both kings checked: the engine's error, no state
            continue
        assert why[i] in (0, 8) and bool(dn[i]) == (why[i] == 8), (i, why[i])
        if len(diff) == 2:
            f, t = (diff[0], diff[1]) if obs[i][diff[0]] == 0 else (diff[1], diff[0])
            assert np.sign(nb[f]) == opp and obs[i][f] == 0 and obs[i][t] == nb[f] and np.sign(nb[t]) != opp, i
            if abs(nb[t]) != 1:  # (a reply that takes the king after a Q6 retreat pays what lib.rs pays)
                assert rw[i] == base - fx["value"][abs(int(nb[t]))], i
        else:  # a castle by the replying side (White only: Q4)
            assert opp == 1 and len(diff) == 4 and (diff >= 56).all() and rw[i] == base, (i, diff)
        replies += 1
    assert replies > 0.8 * n
    env.close()
