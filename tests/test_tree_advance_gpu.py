"""GPU: gc_tree_advance / SearchTree.advance (the played move's subtree kept across moves) against
AdvTree of test_tree_advance.py: synthetic trees at every cap that takes another path, trees of
several 64-node chunks (alone and side by side in one workgroup), the node bound, placement and
repeatability, the boards of the kept nodes in the documented chess loop under both rule sets
(the in-place board move's ordering), and the state and argument errors.  Buffers come from
gc_device_alloc / gc_env_copy; no torch."""
import ctypes

import numpy as np
import pytest

import test_clone_gpu as CG
import test_policy_sample as P
import test_tree_advance as A
import test_tree_search as R
import test_tree_search_gpu as T
from test_policy_priors_gpu import Dev

pytestmark = pytest.mark.gpu

NONE = R.NONE


@pytest.fixture(scope="module")
def env():
    from gym_chess_amd.env import BatchedChessEnv

    e = BatchedChessEnv(160, device=0, seed=3)
    yield e
    e.close()


def upload(env, ptr, a):
    from gym_chess_amd import _lib

    a = np.ascontiguousarray(a)
    _lib.check(env._L.gc_env_copy(env._h, ptr, _lib.ptr(a), ctypes.c_uint64(a.nbytes), 1))


def put_block(env, pri, block):
    """a host priors block into a priors_buffer() of the same cap"""
    for k, a in zip(("actions", "priors", "count"), block[:3]):
        upload(env, pri.ptr[k], a)


# --------------------------------------------------------------------------- 1. synthetic trees
def run_sequence(env, case, G, inp, blocks, check=True, shots=None, first_greedy=False, g0=0):
    """junk-filled arrays -> `nodes` simulations -> advance -> nodes / 2 more -> advance -> the
    rest, the reference following every selection under the acceptance rule.  The moves reach the
    device as root_policy's pick buffer (the greedy picks stay as the kernel wrote them; the other
    rules' moves are written over theirs).  shots: a list that takes the device's arrays after
    each advance and at the end.  first_greedy, g0: A.moves_for's (the large runs' move rule; a
    game taken out of a larger run)."""
    _, nodes, cap, rule, seed, c_puct, fpu = case
    r = T.Run(env, G, nodes, cap, inp, c_puct, fpu)
    r.ref = A.AdvTree(G, nodes, cap)
    tree = r.tree
    r.reset(check)
    pri = env.priors_buffer(G, cap=inp["pri_cap"])
    for turn, (a, b) in enumerate(A.stages(nodes)):
        for s in range(a, b):
            r.simulate(s, check)
        if turn == 2:
            break
        T.fill_arrays(env, tree._root)
        rp = tree.root_policy(greedy=True)
        picks = rp.fetch("pick")["pick"]
        mv = A.moves_for(r.ref, picks, turn, first_greedy, g0) if check else None
        if check:
            assert (picks == r.ref.root_policy(0, 0, True)["pick"]).all()
        else:  # (placement runs: the reference is not driven, the rules come from the device's tree)
            d = tree.fetch("child", "action", "n_children")
            shadow = A.AdvTree(G, nodes, cap)
            shadow.child, shadow.action, shadow.n_children = d["child"], d["action"], d["n_children"]
            mv = A.moves_for(shadow, picks, turn, first_greedy, g0)
        for g in np.flatnonzero(mv != picks):
            upload(env, rp.pick + 2 * int(g), mv[g: g + 1])
        act, prs, cnt, val = blocks[turn]
        put_block(env, pri, (act, prs, cnt))
        dval = Dev(env, val)
        T.fill_arrays(env, tree._adv)
        adv = tree.advance(rp.pick, pri, value=dval.ptr)
        assert adv is tree._adv
        o = adv.fetch()
        if check:
            kept, remap = r.ref.advance(mv, act, prs, cnt, value=val)
            assert (o["kept"] == kept).all(), (turn, o["kept"], kept)
            assert (o["remap"] == remap).all(), (turn, np.argwhere(o["remap"] != remap)[:4])
            r.ref.same_as(tree.fetch())
        if shots is not None:
            shots.append(dict(tree.fetch(), kept=o["kept"], remap=o["remap"]))
        env.synchronize()
        dval.close()
    if shots is not None:
        shots.append(tree.fetch())
    ref = r.ref
    env.synchronize()
    pri.close()
    r.close()
    return ref


@pytest.mark.parametrize("case", A.ADV_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_synthetic_trees(env, case):
    """after each advance the tree equals the reference's bit for bit below n_nodes, kept and remap
    are exact and (written over junk) fully defined; the search that follows is followed too"""
    G = case[0]
    ref = run_sequence(env, case, G, R.synth_run(*case[:5]), A.advance_blocks(case))
    assert ref.near_ties < 0.01 * ref.decisions, (ref.near_ties, ref.decisions)


@pytest.fixture(scope="module")
def large_env():
    """boards for the trees of R.LARGE_CASES (5 x 200 nodes)"""
    from gym_chess_amd.env import BatchedChessEnv

    e = BatchedChessEnv(1000, device=0, seed=3)
    yield e
    e.close()


@pytest.mark.parametrize("case", R.LARGE_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_large_synthetic_trees(large_env, case):
    """test_synthetic_trees on trees of 130 and 200 nodes (R.open_run's inputs; every game plays its
    greedy pick at the first advance, so games 0 to 2 keep subtrees of several 64-node chunks inside
    one workgroup -- A.test_large_runs_cross_the_chunks has what the runs reach): the keep bitmap
    read back across chunks, the ranks carried on, the rows and boards moved from later chunks into
    earlier ones"""
    G = case[0]
    ref = run_sequence(large_env, case, G, R.open_run(*case[:5]), A.advance_blocks(case), first_greedy=True)
    assert ref.near_ties < 0.01 * ref.decisions, (ref.near_ties, ref.decisions)


# --------------------------------------------------------------------------- 2. placement
def test_large_placement(large_env):
    """game 1 of R.LARGE_CASES[0] through the whole sequence: the same bits alone (G = 1: the
    workgroup's first wave, its keep bitmap at the start of the LDS block) and as one of five (the
    second wave, its bitmap one tree's words further on, between those of games 0 and 2, which
    keep subtrees too)"""
    case = R.LARGE_CASES[0]
    inp, blocks = R.open_run(*case[:5]), A.advance_blocks(case)
    one_blocks = [tuple(np.ascontiguousarray(x[1:2]) for x in b) for b in blocks]
    same = lambda x, y: np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
    five, one = [], []
    run_sequence(large_env, case, 5, inp, blocks, check=False, shots=five, first_greedy=True)
    run_sequence(large_env, case, 1, T._game0(inp, 1), one_blocks, check=False, shots=one, first_greedy=True, g0=1)
    assert (five[0]["kept"][:3] > 64).all(), five[0]["kept"]  # games 0 to 2 keep more than a chunk
    for turn, (a, c) in enumerate(zip(five[:2], one[:2])):
        n = int(a["n_nodes"][1])
        assert n == c["n_nodes"][0] and a["kept"][1] == c["kept"][0] and a["kept"][1] > 1, (turn, a["kept"], c["kept"])
        assert same(a["remap"][1], c["remap"][0]), turn
        for key in R.NODE_KEYS:
            assert same(a[key][1][:n], c[key][0][:n]), (turn, key)
    n = int(five[2]["n_nodes"][1])  # the end of the run
    assert n == one[2]["n_nodes"][0]
    for key in R.NODE_KEYS:
        assert same(five[2][key][1][:n], one[2][key][0][:n]), key


def test_placement_and_repeatability(env):
    """game 0 through the whole sequence: the same bits alone (G = 1) and as one of five, and in a
    second run (all five games, junk included)"""
    case = A.ADV_CASES[0]
    inp, blocks = R.synth_run(*case[:5]), A.advance_blocks(case)
    one_blocks = [tuple(np.ascontiguousarray(x[:1]) for x in b) for b in blocks]
    got = []
    for G, data, bl in ((5, inp, blocks), (5, inp, blocks), (1, T._game0(inp), one_blocks)):
        shots = []
        run_sequence(env, case, G, data, bl, check=False, shots=shots)
        got.append(shots)
    assert got[0][0]["kept"][0] > 1  # game 0 keeps a subtree at the first advance
    for a, b, c in zip(*got):
        n = int(a["n_nodes"][0])
        assert n == c["n_nodes"][0]
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), key
            if key in R.NODE_KEYS:
                x, y = a[key][0][:n], c[key][0][:n]
            elif key == "path":
                continue  # (the pending path's leftovers lie past depth)
            else:
                x, y = a[key][0], c[key][0]
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), key


# --------------------------------------------------------------------------- 3. the boards
def pair_states(env_a, ia, env_b, ib, what):
    """boards ia of env_a against boards ib of env_b: state, windows, planes in both views"""
    CG.assert_same_state(CG.state(env_a), ia, CG.state(env_b), ib, what)
    for x, y in zip(ia, ib):
        assert CG.window(env_a, x) == CG.window(env_b, y), (what, x, y)
    pa, pb = env_a.planes_buffer(dtype="float16"), env_b.planes_buffer(dtype="float16")
    for persp in (False, True):
        env_a.encode_planes(pa, perspective=persp)
        env_b.encode_planes(pb, perspective=persp)
        assert (pa.raw()[ia] == pb.raw()[ib]).all(), (what, persp)
    pa.close()
    pb.close()


def continue_pairs(a, aio, ia, b, bio, ib, steps):
    """boards ia of env a and ib of env b under one action sequence -- a knight shuffle move where
    one is legal (so repetitions complete), else a seeded quiet move of a's position --: every
    output equal on every step -> the (step, pair) list of 3-fold verdicts"""
    rng = np.random.RandomState(77)
    done = np.zeros(len(ia), dtype=bool)
    verdicts = []
    for t in range(steps):
        bd, _ = a.boards()
        mv, cnt = a.legal_moves()
        xa = np.full(a.num_boards, CG.IDLE, dtype=np.uint16)
        xb = np.full(b.num_boards, CG.IDLE, dtype=np.uint16)
        for j, (x, y) in enumerate(zip(ia, ib)):
            legal = sorted(int(m) for m in mv[x, : cnt[x]])
            back = [m for m in CG.SHUFFLE if m in legal]
            act = back[0] if back and not done[j] else CG.recipe_action("quiet", t, rng, bd[x], legal, done[j])
            xa[x] = xb[y] = act
        oa, ob = CG.step_both(a, aio, xa, b, bio, xb)
        for k in CG.OUTS:
            bad = [j for j in range(len(ia)) if not (oa[k][ia[j]] == ob[k][ib[j]]).all()]
            assert not bad, (t, k, bad[:5])
        done = oa["done"][ia] != 0
        verdicts += [(t, j) for j in np.flatnonzero(oa["reason"][ia] == 2)]
    return verdicts


# (G, NODES, SIMS, MORE): the second one's trees span two 64-node chunks of k_move_boards and
# k_tree_advance_compact.  The shuffling games 0..3 do not get there at any size: their most
# visited move leads to the draw by repetition, which takes the visits without growing (they keep 3
# to 7 nodes of 72 or 128); the games on random moves keep up to 90 of 96
BOARD_GEOMETRIES = [(8, 17, 16, 8), (8, 96, 95, 8)]


@pytest.mark.parametrize("geo", BOARD_GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("rules", ["reference", "fide"])
def test_boards_follow_their_nodes(rules, geo):
    """The documented loop with chess: G games 6 plies in (games 0..3 on test_clone_gpu's knight
    shuffle, the others on seeded random moves), trees of NODES nodes, SIMS simulations with fpu -1
    (deep trees) on seeded pseudo-logits that favour the shuffle's four moves -- so the shuffling
    games tend to play Ng1 and keep a subtree whose boards carry the shuffle's live window and, two
    plies down, the draw by repetition --, then root_policy -> the game env's step -> policy_priors
    on the game env -> advance -> the roots cloned, and MORE more simulations.
    Before the advance the whole tree env is cloned into a shadow env at the same indices; after it
    board g * NODES + new[k] must be the shadow's board g * NODES + k in every way a clone is
    compared, and every board at or past kept[g] must be as it was.  With more than 64 nodes a
    board also moves from node 64 or later to an earlier index, and a game's kept set lies in both
    chunks."""
    from gym_chess_amd.env import BatchedChessEnv

    G, NODES, SIMS, MORE = geo
    CAP = 64
    C_PUCT, FPU = 1.25, -1.0
    rng = np.random.RandomState(41)
    game = BatchedChessEnv(G, device=0, seed=5, rules=rules)
    gio = game.device_io(select=False)
    for ply in range(6):
        mv, cnt = game.legal_moves()
        acts = [CG.SHUFFLE[ply % 4] if g < 4 else int(sorted(mv[g, : cnt[g]])[rng.randint(cnt[g])]) for g in range(G)]
        gio.upload_actions(acts)
        game.step_device(gio, actions=gio.ptr["pick"], autoreset=False)
    assert not gio.fetch("done")["done"].any()
    counts = sorted(c for _, c in CG.window(game, 0))
    assert len(counts) == 4 and counts[-1] == 2, counts  # live entries, some seen twice
    tenv = BatchedChessEnv(G * NODES, device=0, seed=6, rules=rules)
    shadow = BatchedChessEnv(G * NODES, device=0, seed=8, rules=rules)
    shadow.step_random(40)  # (dirty tables, other generations)
    shadow.synchronize()
    tio, sio = tenv.device_io(select=False), shadow.device_io(select=False)
    raw = rng.uniform(-3, 3, size=(SIMS + MORE + 2, G, 4100)).astype(np.float32)
    raw[:, :, list(CG.SHUFFLE)] += 6.0
    raw, _ = P.quantise(raw, "bfloat16")
    values = rng.uniform(-1, 1, size=(SIMS + MORE + 2, G)).astype(np.float32)
    logits, vals = Dev(tenv, raw), Dev(tenv, values)
    row_bytes = G * 4100 * 2
    LAST = SIMS + MORE  # the blocks of the two roots: LAST, LAST + 1

    gpri = game.priors_buffer(G, cap=CAP)
    game.policy_priors(gio, logits.ptr + LAST * row_bytes, gpri, dtype="bfloat16")
    game.synchronize()
    tree = tenv.search_tree(G, NODES, cap=CAP)
    ref = A.AdvTree(G, NODES, CAP)
    tree.reset(gpri, value=vals.ptr + 4 * G * LAST)
    h = gpri.fetch()
    ref.reset(h["actions"], h["priors"], h["count"], value=values[LAST])
    all_roots = np.arange(G) * NODES
    tenv.clone_boards(game, np.arange(G), all_roots)
    pri, rows = tenv.priors_buffer(G, cap=CAP), tenv.rows_buffer(G)

    def simulate(s):
        T.fill_arrays(tenv, tree._sel)
        sel = tree.select(C_PUCT, FPU)
        tenv.clone_boards(tenv, sel.parent, sel.child, count=G)
        tenv.step_boards(tio, sel.child, sel.action, rows=G, out=rows)
        tenv.policy_priors(tio, logits.ptr + s * row_bytes, pri, boards=sel.child, rows=G, dtype="bfloat16")
        tree.backup(vals.ptr + 4 * G * s, rows, pri)
        d = tree.fetch("path", "depth")
        wp, wc, wa = ref.select(C_PUCT, FPU, follow=(d["path"], d["depth"]))
        o, st, pr = sel.fetch(), rows.fetch("done", "reason"), pri.fetch()
        assert (o["parent"] == wp).all() and (o["child"] == wc).all() and (o["action"] == wa).all()
        ref.backup(values[s], st["done"], st["reason"], pr["actions"], pr["priors"], pr["count"])
        ref.same_as(tree.fetch())

    for s in range(SIMS):
        simulate(s)

    # the move: root_policy -> the game env's step (a game that ends is reset and marked 0xFFFF)
    picks = tree.root_policy(greedy=True).fetch("pick")["pick"]
    assert (picks == ref.root_policy(0, 0, True)["pick"]).all() and (picks != NONE).all()
    gio.upload_actions(picks)
    game.step_device(gio, actions=gio.ptr["pick"], autoreset=True)
    ended = gio.fetch("done")["done"] != 0
    moves = np.where(ended, NONE, picks).astype(np.uint16)
    game.policy_priors(gio, logits.ptr + (LAST + 1) * row_bytes, gpri, dtype="bfloat16")
    game.synchronize()

    everything = np.arange(G * NODES)
    shadow.clone_boards(tenv, everything, everything)
    slab0 = CG.slab(tenv)
    adv = tree.advance(moves, gpri, value=vals.ptr + 4 * G * (LAST + 1))
    o, h = adv.fetch(), gpri.fetch()
    kept, remap = ref.advance(moves, h["actions"], h["priors"], h["count"], value=values[LAST + 1])
    assert (o["kept"] == kept).all() and (o["remap"] == remap).all()
    ref.same_as(tree.fetch())
    assert ((kept == 0) == ended).all() and (kept[~ended] > 1).all(), (kept, ended)

    src = np.array([g * NODES + k for g in range(G) for k in np.flatnonzero(remap[g] >= 0)], dtype=np.int64)
    dst = np.array([g * NODES + remap[g, k] for g in range(G) for k in np.flatnonzero(remap[g] >= 0)], dtype=np.int64)
    # the hazard: destinations that are the source of an earlier pair of their game
    hazards = sum(int(remap[g, k] >= 0 and remap[g, remap[g, k]] >= 0) for g in range(G) for k in range(NODES))
    print(f"{rules}: kept {kept.tolist()}, {src.size} boards moved, {hazards} onto the source of an earlier pair")
    assert src.size >= G and hazards >= 1, (kept, hazards)
    if NODES > 64:
        moved = [np.flatnonzero((remap[g] >= 0) & (remap[g] < np.arange(NODES))) for g in range(G)]
        spans = [np.unique(np.flatnonzero(remap[g] >= 0) >> 6).size for g in range(G)]
        print(f"{rules}: moved from node 64 or later {[int((m >= 64).sum()) for m in moved]}, chunks kept {spans}")
        assert any((m >= 64).any() for m in moved), kept  # a source in the second chunk
        assert any(((m >= 64) & (remap[g, m] < 64)).any() for g, m in enumerate(moved)), kept  # ... into the first
        assert max(spans) >= 2, spans  # a kept set in both chunks
    rest = np.setdiff1d(everything, dst)
    assert (rest % NODES >= kept[rest // NODES]).all()
    lens = [len(CG.window(shadow, int(i))) for i in src]
    assert sum(n > 0 for n in lens) >= src.size // 4 and max(lens) >= 4, lens  # live windows travel
    pair_states(shadow, src, tenv, dst, "moved")
    pair_states(shadow, rest, tenv, rest, "untouched")
    slab1 = CG.slab(tenv)
    assert (slab1["draw"] == slab0["draw"]).all() and (slab1["nsteps"] == slab0["nsteps"]).all()
    assert (slab1["hgen"][dst] == slab0["hgen"][dst] + 1).all() and (slab1["hgen"][rest] == slab0["hgen"][rest]).all()
    # a kept root is the game env's board: the game played that action from that state
    live = np.flatnonzero(~ended)
    pair_states(game, live, tenv, live * NODES, "root")

    # the moved boards continue as the shadow's (then the tree env is put back)
    blob = tenv.checkpoint()
    verdicts = continue_pairs(shadow, sio, src, tenv, tio, dst, 6)
    print(f"{rules}: 3-fold verdicts at {sorted(set(t for t, _ in verdicts))} on {len({j for _, j in verdicts})} pairs")
    assert verdicts
    tenv.load(blob)

    # the documented recipe: every root cloned from the game env, and the search goes on
    tenv.clone_boards(game, np.arange(G), all_roots)
    for s in range(SIMS, SIMS + MORE):
        simulate(s)
    assert ref.near_ties < 0.01 * ref.decisions
    lm = tenv.legal_mask()
    for g in range(G):
        for k in range(int(ref.n_nodes[g])):
            if ref.terminal[g, k]:
                assert ref.n_children[g, k] == 0
                continue
            legal = np.flatnonzero(lm[g * NODES + k, :4100])[:CAP]
            assert ref.n_children[g, k] == legal.size and (ref.action[g, k, : legal.size] == legal).all(), (g, k)
    tenv.synchronize()
    tree.close()
    for b in (logits, vals, pri, rows, gpri, tio, gio, sio):
        b.close()
    for e in (tenv, shadow, game):
        e.close()


# --------------------------------------------------------------------------- 4. state and argument errors
def test_state_and_argument_errors(env):
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    L, G, NODES, CAP = env._L, 4, 8, 16
    inp = R.synth_run(G, NODES, CAP, "wide", 12)
    a, p, c = (Dev(env, x) for x in inp["root"])
    v = Dev(env, inp["root_value"])
    done = Dev(env, np.zeros(G, dtype=np.uint8))
    mv = Dev(env, np.full(G, NONE, dtype=np.uint16))
    pc = inp["pri_cap"]
    tree = env.search_tree(G, NODES, cap=CAP)
    t, sel, adv = tree._h, tree._sel.ptr, tree._adv.ptr
    kept, remap = adv["kept"], adv["remap"]

    def refused(fn, *args):
        with pytest.raises(_lib.GymChessError) as ei:
            _lib.check(fn(*args))
        assert str(ei.value), args
        return str(ei.value)

    T.fill_tree(env, tree)
    _lib.check(L.gc_tree_reset(t, a.ptr, p.ptr, c.ptr, pc, v.ptr))
    back = (v.ptr, done.ptr, done.ptr, a.ptr, p.ptr, c.ptr, pc)
    for _ in range(3):
        _lib.check(L.gc_tree_select(t, 1.25, 0.0, sel["parent"], sel["child"], sel["action"]))
        _lib.check(L.gc_tree_backup(t, *back))
    T.fill_arrays(env, tree._adv)
    before = dict(tree.fetch(), **tree._adv.fetch())

    def untouched():
        now = dict(tree.fetch(), **tree._adv.fetch())
        assert all(before[k].tobytes() == now[k].tobytes() for k in before)

    good = (t, mv.ptr, a.ptr, p.ptr, c.ptr, pc, v.ptr, kept, remap)
    for k in (0, 1, 2, 3, 4, 7):  # the handle, the moves, the priors block, kept
        bad = list(good)
        bad[k] = None
        refused(L.gc_tree_advance, *bad)
    for bad_cap in (0, -3):
        refused(L.gc_tree_advance, *(good[:5] + (bad_cap,) + good[6:]))
    untouched()
    # the pending bit, both ways
    _lib.check(L.gc_tree_select(t, 1.25, 0.0, sel["parent"], sel["child"], sel["action"]))
    before = dict(tree.fetch(), **tree._adv.fetch())
    assert "pending" in refused(L.gc_tree_advance, *good)
    untouched()
    _lib.check(L.gc_tree_backup(t, *back))
    bytes0 = tree.device_bytes()
    _lib.check(L.gc_tree_advance(*(good[:6] + (None, kept, None))))  # the value and the remap are optional
    assert tree.device_bytes() == bytes0 + G * NODES * 4  # the remap scratch is the handle's, and counted
    assert (tree.fetch("n_nodes")["n_nodes"] == 1).all() and not tree._adv.fetch("kept")["kept"].any()
    refused(L.gc_tree_backup, t, *back)  # an advance leaves no selection pending
    _lib.check(L.gc_tree_select(t, 1.25, 0.0, sel["parent"], sel["child"], sel["action"]))
    _lib.check(L.gc_tree_backup(t, *back))
    _lib.check(L.gc_tree_advance(*good))
    _lib.check(L.gc_tree_advance(*(good[:8] + (None,))))
    assert tree.device_bytes() == bytes0 + G * NODES * 4

    # the wrapper's own checks
    small = env.priors_buffer(G - 1, cap=CAP)
    full = env.priors_buffer(G, cap=CAP)
    with pytest.raises(ValueError):
        tree.advance(mv.ptr, small)
    with pytest.raises(TypeError):
        tree.advance(mv.ptr, a.ptr)
    with pytest.raises(ValueError):
        tree.advance([1, 2, 3], full)
    with pytest.raises(ValueError):
        tree.advance([1, 2, 3, 70000], full)
    env.synchronize()
    tree.close()

    # a player_color BLACK tree env: refused as gc_env_clone_boards(e, e, ...) refuses it
    black = BatchedChessEnv(G * NODES, device=0, seed=1, opponent="random", player_color="BLACK")
    bt = black.search_tree(G, NODES, cap=CAP)
    _lib.check(L.gc_tree_reset(bt._h, a.ptr, p.ptr, c.ptr, pc, v.ptr))
    T.fill_arrays(black, bt._adv)
    before = dict(bt.fetch(), **bt._adv.fetch())
    assert "BLACK" in refused(L.gc_tree_advance, bt._h, mv.ptr, a.ptr, p.ptr, c.ptr, pc, v.ptr, bt._adv.ptr["kept"],
                              bt._adv.ptr["remap"])
    now = dict(bt.fetch(), **bt._adv.fetch())
    assert all(before[k].tobytes() == now[k].tobytes() for k in before)
    black.synchronize()
    bt.close()
    black.close()
    for b in (a, p, c, v, done, mv, small, full):
        b.close()


# --------------------------------------------------------------------------- 5. the node bound
def test_the_node_bound():
    """TREE_ADV_MAX_NODES = 65 536 (the keep bitmap's 32 KiB of LDS per workgroup), on one env of
    65 537 boards.  A tree of 65 537 nodes: advance is refused with a message that names the bound,
    and neither the tree nor kept / remap change.  A tree of 65 536 nodes over junk-filled arrays:
    a one-move root, three simulations with one-move lists (a chain of four nodes), advance on the
    greedy pick -> kept = 3, remap = the reference's over all 65 536 entries (1 024 ballot words,
    the largest launch the bound allows), the tree = the reference's below n_nodes."""
    from gym_chess_amd import _lib
    from gym_chess_amd.env import BatchedChessEnv

    BOUND = 65536
    e = BatchedChessEnv(BOUND + 1, device=0, seed=3)
    L = e._L
    blocks = [R._block([[(100 + s, 1.0)]], 1) for s in range(5)]  # the root, three leaves, the advance's
    dev = [[Dev(e, x) for x in b] for b in blocks]
    zero, val = Dev(e, np.zeros(1, dtype=np.uint8)), Dev(e, np.array([0.375], dtype=np.float32))
    mv = Dev(e, np.array([100], dtype=np.uint16))

    # above the bound
    tree = e.search_tree(1, BOUND + 1, cap=1)
    T.fill_tree(e, tree)
    _lib.check(L.gc_tree_reset(tree._h, *(b.ptr for b in dev[0]), 1, val.ptr))
    T.fill_arrays(e, tree._adv)
    before = dict(tree.fetch(), **tree._adv.fetch())
    with pytest.raises(_lib.GymChessError) as ei:
        _lib.check(L.gc_tree_advance(tree._h, mv.ptr, *(b.ptr for b in dev[4]), 1, val.ptr, tree._adv.ptr["kept"],
                                     tree._adv.ptr["remap"]))
    assert str(BOUND) in str(ei.value), str(ei.value)
    now = dict(tree.fetch(), **tree._adv.fetch())
    assert all(before[k].tobytes() == now[k].tobytes() for k in before)
    e.synchronize()
    tree.close()

    # at the bound
    tree = e.search_tree(1, BOUND, cap=1)
    ref = A.AdvTree(1, BOUND, 1)
    T.fill_tree(e, tree)
    _lib.check(L.gc_tree_reset(tree._h, *(b.ptr for b in dev[0]), 1, val.ptr))
    ref.reset(*blocks[0], value=np.array([0.375], dtype=np.float32))
    values = np.array([[0.5], [-0.25], [0.125]], dtype=np.float32)
    dvals = Dev(e, values)
    none = np.zeros(1, dtype=np.uint8)
    for s in range(3):
        tree.select(1.25, 0.0)
        d = tree.fetch("path", "depth")
        ref.select(1.25, 0.0, follow=(d["path"], d["depth"]))
        _lib.check(L.gc_tree_backup(tree._h, dvals.ptr + 4 * s, zero.ptr, zero.ptr, *(b.ptr for b in dev[1 + s]), 1))
        ref.backup(values[s], none, none, *blocks[1 + s])
        ref.same_as(tree.fetch())
    assert ref.n_nodes[0] == 4
    T.fill_arrays(e, tree._root)
    rp = tree.root_policy(greedy=True)
    picks = rp.fetch("pick")["pick"]
    assert picks.tolist() == [100]
    pri = e.priors_buffer(1, cap=1)
    put_block(e, pri, blocks[4])
    T.fill_arrays(e, tree._adv)
    o = tree.advance(rp.pick, pri, value=val.ptr).fetch()
    kept, remap = ref.advance(picks, *blocks[4], value=np.array([0.375], dtype=np.float32))
    assert kept.tolist() == [3] and o["kept"].tolist() == [3]
    assert remap[0, :5].tolist() == [-1, 0, 1, 2, -1] and (o["remap"] == remap).all()
    ref.same_as(tree.fetch())
    e.synchronize()
    tree.close()
    pri.close()
    for b in [x for row in dev for x in row] + [zero, val, mv, dvals]:
        b.close()
    e.close()
