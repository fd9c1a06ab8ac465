"""TEST INFRASTRUCTURE ONLY -- ctypes view of the CPU parity oracle (gc_oracle.c).

The oracle restates /root/reference/src/lib.rs (engine) and
/root/reference/gym_chess/envs/chess_v2.py (env bookkeeping) on the CPU.  Only
tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this
module; the product package (gym-chess_amd/gym_chess_amd) never does.

State convention (shared with the product C-ABI):
  board : int8[64], sq = row*8+col, row 0 = rank 8 (lib.rs:1235-1238),
          piece ids +-1..6 = K,Q,R,B,N,P, positive = white (lib.rs:11-17)
  meta  : uint8[8] = {white_to_move, wkc, wqc, bkc, bqc, white_checked,
                      black_checked, move_count}
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libgcoracle.so")

DEFAULT_BOARD = np.array(
    [
        [-3, -5, -4, -2, -1, -4, -5, -3],
        [-6] * 8,
        [0] * 8,
        [0] * 8,
        [0] * 8,
        [0] * 8,
        [6] * 8,
        [3, 5, 4, 2, 1, 4, 5, 3],
    ],
    dtype=np.int8,
).reshape(64)

_lib = None


def build():
    subprocess.run(["make", "-s", "-C", _HERE], check=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            build()
        L = ctypes.CDLL(_SO)
        P = ctypes.c_void_p
        i32, u32, u64 = ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
        L.oracle_get_possible_moves.argtypes = [P, P, i32, i32, P, i32]
        L.oracle_get_possible_moves.restype = i32
        L.oracle_get_castle_moves.argtypes = [P, P, i32, P]
        L.oracle_get_castle_moves.restype = i32
        L.oracle_next_state.argtypes = [P, P, i32, i32, P, P, P]
        L.oracle_next_state.restype = i32
        L.oracle_update_state.argtypes = [P, P, P, P]
        L.oracle_update_state.restype = None
        L.oracle_perft.argtypes = [P, P, i32]
        L.oracle_perft.restype = u64
        L.oracle_policy_index.argtypes = [u64, u32, u32, u32]
        L.oracle_policy_index.restype = u32
        L.oracle_rollout_trace.argtypes = [P, u64, u32, i32, P, P, P, P, P, P, P]
        L.oracle_rollout_trace.restype = None
        L.oracle_rollout_batch.argtypes = [P, u64, u32, u32, i32, i32, P]
        L.oracle_rollout_batch.restype = None
        L.oracle_perft_batch.argtypes = [P, P, u32, i32, i32, P]
        L.oracle_perft_batch.restype = None
        L.oracle_env_new.argtypes = [P]
        L.oracle_env_new.restype = P
        L.oracle_env_new2.argtypes = [P, i32, i32, u64, u32]
        L.oracle_env_new2.restype = P
        L.oracle_env_pick.argtypes = [P]
        L.oracle_env_pick.restype = i32
        L.oracle_env_draw.argtypes = [P]
        L.oracle_env_draw.restype = u32
        L.oracle_rollout_trace2.argtypes = [P, u64, u32, i32, i32, i32, P, P, P, P, P, P, P]
        L.oracle_rollout_trace2.restype = None
        L.oracle_rollout_trace3.argtypes = [P, u64, u32, i32, i32, i32, i32, P, P, P, P, P, P, P]
        L.oracle_rollout_trace3.restype = None
        L.oracle_rollout_batch2.argtypes = [P, u64, u32, u32, i32, i32, i32, i32, P]
        L.oracle_rollout_batch2.restype = None
        L.oracle_env_free.argtypes = [P]
        L.oracle_env_reset.argtypes = [P]
        L.oracle_env_step.argtypes = [P, i32, P, P, P]
        L.oracle_env_step.restype = i32
        L.oracle_env_moves.argtypes = [P, P, i32]
        L.oracle_env_moves.restype = i32
        L.oracle_env_state.argtypes = [P, P, P]
        L.oracle_env_done.argtypes = [P]
        L.oracle_env_done.restype = i32
        L.oracle_rollout_max_window.argtypes = [P, u64, u32, i32, i32, i32]
        L.oracle_rollout_max_window.restype = i32
        L.oracle_single_op.argtypes = [P, i32, i32, i32, P]
        L.oracle_single_op.restype = i32
        L.oracle_env_window.argtypes = [P]
        L.oracle_env_window.restype = i32
        L.oracle_env_set_board.argtypes = [P, P, P]
        L.oracle_env_set_board.restype = None
        L.oracle_rollout_digests.argtypes = [P, u64, u32, u32, i32, i32, i32, i32, P]
        L.oracle_rollout_digests.restype = None
        L.oracle_trace_word.argtypes = [i32, i32, i32, i32]
        L.oracle_trace_word.restype = u64
        L.oracle_api_digests.argtypes = [P, u64, u32, u32, i32, i32, i32, i32, i32, i32, P, P, P]
        L.oracle_api_digests.restype = None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def make_meta(white_to_move=True, wkc=True, wqc=True, bkc=True, bqc=True):
    return np.array([white_to_move, wkc, wqc, bkc, bqc, 0, 0, 0], dtype=np.uint8)


def get_possible_moves(board, meta, white, attack=False):
    """ChessEngine.get_possible_moves (lib.rs:1454-1480) -> ordered action list."""
    b = np.ascontiguousarray(board, dtype=np.int8).reshape(64)
    m = np.ascontiguousarray(meta, dtype=np.uint8)
    out = np.zeros(1024, dtype=np.uint16)
    n = lib().oracle_get_possible_moves(_p(b), _p(m), int(bool(white)), int(bool(attack)), _p(out), 1024)
    return [int(x) for x in out[:n]]


def get_castle_moves(board, meta, white):
    b = np.ascontiguousarray(board, dtype=np.int8).reshape(64)
    m = np.ascontiguousarray(meta, dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint16)
    n = lib().oracle_get_castle_moves(_p(b), _p(m), int(bool(white)), _p(out))
    return [int(x) for x in out[:n]]


def next_state(board, meta, white, action):
    """ChessEngine.next_state (lib.rs:1422-1452) -> (rc, board, meta, reward).
    rc: 0 ok, 1 both kings checked (reference raises), -1 empty from-square (panic)."""
    b = np.ascontiguousarray(board, dtype=np.int8).reshape(64)
    m = np.ascontiguousarray(meta, dtype=np.uint8)
    ob = np.zeros(64, dtype=np.int8)
    om = np.zeros(8, dtype=np.uint8)
    rw = ctypes.c_int(0)
    rc = lib().oracle_next_state(_p(b), _p(m), int(bool(white)), int(action), _p(ob), _p(om), ctypes.byref(rw))
    return rc, ob, om, rw.value


def update_state(board, meta):
    b = np.ascontiguousarray(board, dtype=np.int8).reshape(64)
    m = np.ascontiguousarray(meta, dtype=np.uint8)
    ob = np.zeros(64, dtype=np.int8)
    om = np.zeros(8, dtype=np.uint8)
    lib().oracle_update_state(_p(b), _p(m), _p(ob), _p(om))
    return ob, om


def perft(board, meta, depth):
    b = np.ascontiguousarray(board, dtype=np.int8).reshape(64)
    m = np.ascontiguousarray(meta, dtype=np.uint8)
    return int(lib().oracle_perft(_p(b), _p(m), int(depth)))


def perft_batch(boards, metas, depth, threads=1):
    b = np.ascontiguousarray(boards, dtype=np.int8).reshape(-1, 64)
    m = np.ascontiguousarray(metas, dtype=np.uint8).reshape(-1, 8)
    out = np.zeros(b.shape[0], dtype=np.uint64)
    lib().oracle_perft_batch(_p(b), _p(m), b.shape[0], int(depth), int(threads), _p(out))
    return out


def perft_by_children(boards, metas, depth, threads=1):
    """perft(depth) per root as the sum of perft(depth - 1) over its children (the definition,
    SURVEY.md §3.4), so the threads share the work of a few large roots evenly."""
    b = np.ascontiguousarray(boards, dtype=np.int8).reshape(-1, 64)
    m = np.ascontiguousarray(metas, dtype=np.uint8).reshape(-1, 8)
    if depth <= 1:
        return perft_batch(b, m, depth, threads)
    kb, km, owner = [], [], []
    for i in range(b.shape[0]):
        for a in get_possible_moves(b[i], m[i], int(m[i, 0])):
            _, nb, nm, _ = next_state(b[i], m[i], int(m[i, 0]), a)
            kb.append(nb)
            km.append(nm)
            owner.append(i)
    out = np.zeros(b.shape[0], dtype=np.uint64)
    if kb:
        sub = perft_batch(np.stack(kb), np.stack(km), depth - 1, threads)
        np.add.at(out, np.array(owner), sub)
    return out


def policy_index(seed, board, draw, n):
    return int(lib().oracle_policy_index(seed, board, draw, n))


def rollout_trace(seed, board_id, plies, init=DEFAULT_BOARD, opponent=0, agent_white=True, order=None):
    """Single-board random self-play (test_benchmark.py driver shape, auto-reset); with
    opponent=1 the env answers every step with the random opponent (chess_v2.py:275-288).
    The policy (agent and opponent) ranks the legal moves in move-set order; order="action"
    ranks them in action-id order instead (the API step's `pick` output: the order of its
    legal-action mask).
    Returns dict of per-ply arrays + final state + stats."""
    init = np.ascontiguousarray(init, dtype=np.int8).reshape(64)
    a = np.zeros(plies, dtype=np.int16)
    r = np.zeros(plies, dtype=np.int16)
    d = np.zeros(plies, dtype=np.uint8)
    why = np.zeros(plies, dtype=np.uint8)
    fb = np.zeros(64, dtype=np.int8)
    fm = np.zeros(8, dtype=np.uint8)
    st = np.zeros(8, dtype=np.uint64)
    o = {None: -1, "action": 0, "set": 1}[order]
    lib().oracle_rollout_trace3(_p(init), seed, board_id, plies, int(opponent), int(bool(agent_white)), o, _p(a),
                                _p(r), _p(d), _p(why), _p(fb), _p(fm), _p(st))
    return dict(action=a, reward=r, done=d, reason=why, final_board=fb, final_meta=fm, stats=st)


def rollout_max_window(seed, board_id, plies, init=DEFAULT_BOARD, opponent=0, agent_white=True):
    """the longest 3-fold window along rollout_trace's trajectory (the device spills a BLACK
    agent's windows past 511 boards)"""
    init = np.ascontiguousarray(init, dtype=np.int8).reshape(64)
    return int(lib().oracle_rollout_max_window(_p(init), seed, board_id, plies, int(opponent), int(bool(agent_white))))


def rollout_batch(seed, b_begin, n_boards, plies, threads=1, init=DEFAULT_BOARD, opponent=0, agent_white=True):
    init = np.ascontiguousarray(init, dtype=np.int8).reshape(64)
    st = np.zeros(8, dtype=np.uint64)
    lib().oracle_rollout_batch2(_p(init), seed, b_begin, n_boards, plies, int(opponent), int(bool(agent_white)), threads,
                                _p(st))
    return st


DIGEST_PRIME = 0x100000001B3


def rollout_digests(seed, n_boards, plies, opponent=0, agent_white=True, threads=1, init=DEFAULT_BOARD, b_begin=0):
    """Per board b_begin + k, a 64-bit digest of rollout_trace's whole trajectory: every ply's
    outputs packed as the device's trace word, folded d = (d ^ w) * DIGEST_PRIME in ply order, then
    the final board (eight little-endian words) and meta (one word) -- gc_oracle.c
    oracle_rollout_digests; the device side is tests/test_full_width_digest.py's trace_digest."""
    init = np.ascontiguousarray(init, dtype=np.int8).reshape(64)
    out = np.zeros(n_boards, dtype=np.uint64)
    lib().oracle_rollout_digests(_p(init), seed, b_begin, n_boards, plies, int(opponent), int(bool(agent_white)),
                                 threads, _p(out))
    return out


API_ACTION_STREAM = 0x5EEDAC7105  # seed ^ this: the Philox key of api_digests' action schedule
API_STAT_NAMES = ("stuck_resets", "arbitrary", "arbitrary_accepted", "near_miss", "near_miss_accepted",
                  "stuck_steps", "max_count", "episode_ends", "near_miss_changed_accepted")


def api_digests(seed, n_boards, steps, opponent=0, agent_white=True, threads=1, init=DEFAULT_BOARD, b_begin=0,
                mask_every=100, snap_every=500):
    """Per board b_begin + k, digests of the device API step's loop (gc_oracle.c api_board: the
    previous pick, arbitrary actions and near misses fed to the auto-reset step; a board without a
    legal move reset as the host reset does): every step's trace word and pick | count << 16
    folded d = (d ^ w) * DIGEST_PRIME, the 65 mask words and the observation every mask_every
    steps, then the final board and meta.  -> (snap uint64[steps // snap_every][n], final
    uint64[n], stats dict: "reasons" int64[16] steps by reason code + API_STAT_NAMES)."""
    init = np.ascontiguousarray(init, dtype=np.int8).reshape(64)
    snap = np.zeros((steps // snap_every, n_boards), dtype=np.uint64)
    final = np.zeros(n_boards, dtype=np.uint64)
    st = np.zeros(32, dtype=np.uint64)
    lib().oracle_api_digests(_p(init), seed, b_begin, n_boards, steps, int(opponent), int(bool(agent_white)),
                             int(mask_every), int(snap_every), threads, _p(snap), _p(final), _p(st))
    stats = {"reasons": st[:16].astype(np.int64)}
    stats.update({k: int(v) for k, v in zip(API_STAT_NAMES, st[16:])})
    return snap, final, stats


class OracleEnv:
    """Step-by-step chess_v2.ChessEnvV2 restatement: opponent 0 = "none", 1 = the random
    opponent drawing from the Philox stream (seed, board, draw++)."""

    def __init__(self, init=DEFAULT_BOARD, opponent=0, agent_white=True, seed=0, board=0):
        self._init = np.ascontiguousarray(init, dtype=np.int8).reshape(64)
        self.h = lib().oracle_env_new2(_p(self._init), int(opponent), int(bool(agent_white)), int(seed), int(board))

    def pick(self):
        """the random policy's action for the side to move (advances the Philox counter)"""
        return int(lib().oracle_env_pick(self.h))

    @property
    def draw(self):
        return int(lib().oracle_env_draw(self.h))

    def __del__(self):
        if getattr(self, "h", None):
            lib().oracle_env_free(self.h)
            self.h = None

    def reset(self):
        lib().oracle_env_reset(self.h)

    def step(self, action):
        rw, dn, why = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = lib().oracle_env_step(self.h, int(action), ctypes.byref(rw), ctypes.byref(dn), ctypes.byref(why))
        return rc, rw.value, dn.value, why.value

    def moves(self):
        out = np.zeros(1024, dtype=np.uint16)
        n = lib().oracle_env_moves(self.h, _p(out), 1024)
        return [int(x) for x in out[:n]]

    def state(self):
        b = np.zeros(64, dtype=np.int8)
        m = np.zeros(8, dtype=np.uint8)
        lib().oracle_env_state(self.h, _p(b), _p(m))
        return b, m

    @property
    def done(self):
        return bool(lib().oracle_env_done(self.h))

    def single_op(self, op, action=0, flags=0):
        """the device's gc_env_single_call ops (the single-board env's split step) ->
        (status, reward, done, reason)"""
        out = np.zeros(4, dtype=np.int32)
        lib().oracle_single_op(self.h, int(op), int(action), int(flags), _p(out))
        return tuple(int(x) for x in out)

    def set_board(self, board, flags6):
        """the env's state setter (chess_v2.py:315-323): board + rights + checks"""
        b = np.ascontiguousarray(board, dtype=np.int8).reshape(64)
        f = np.ascontiguousarray(flags6, dtype=np.uint8).reshape(6)
        lib().oracle_env_set_board(self.h, _p(b), _p(f))

    @property
    def window(self):
        """distinct pre-move boards since the last pawn move / capture"""
        return int(lib().oracle_env_window(self.h))
