// gc_step_rows.h -- one env.step() on the LISTED boards only (gc_env_step_boards,
// include/gymchess.h): the expansion step of a batched search that keeps one env state per tree
// node, where G boards of G * NODES change per simulation.
//
// k_env_step_rows<OPP> / k_fenv_step_rows<OPP> are the one-lane API steps (k_env_step_api,
// k_fenv_step_api) with the board gathered through an index: lane = row j, board i = idx[j].
// Everything that belongs to the BOARD is addressed by i -- state, window table and generation,
// draw counter, step counter, the env's last reward / done / reason, the mask column, and the
// Philox stream (PolicyCtx{seed, i, draw}), so an indexed step of board i is the dense step of
// board i, bit for bit.  Everything that belongs to the CALL is addressed by j: the action in,
// reward / done / reason / count / obs out.  An index outside [0, n) writes its row's sentinel
// (reward 0, done 0, reason GC_REASON_BAD_INDEX, count -1, a zero obs row) and touches nothing
// else.  No pick: act[] is left as it is (the host marks the policy actions stale).
//
// The bodies restate the dense kernels' instead of sharing a function with them: those kernels'
// schedules hang on where their loads are pinned (pin(), DevHist's deferred stores), and their
// code must not move.  tests/test_step_boards_gpu.py holds the two forms together.
//
// Launch-bound at the row counts a search uses (256-4096 rows are 4-64 waves on 256 CUs).  The
// loads gather (a row's seven bitboards sit n words apart anyway; the index only loses the
// coalescing across lanes) and the mask stores scatter: 65 words of 8 bytes per lane,
// mask_stride apart, one board's column each -- inherent to the board-indexed layout, which is
// what lets the buffer accumulate the masks of all tree nodes.  Measured on an env of 65 536 boards
// after 40 random plies, mask / count / obs on (tools/expand_bench.py, profiles/step_boards.json):
// about 18.6 us per launch at 256 rows, 19.1 at 1024, 19.9 at 4096 -- the time of ONE lane's step,
// not of the rows: the launch is latency-bound, and the scattered stores do not show at these
// counts.  (The dense quad kernel steps all 65 536 boards in 16 us by splitting a board over four
// waves; what a search gains is the encode and the framework glue it no longer pays)
// Included by gymchess.hip after k_fenv_step_api.
#pragma once

// Threads per workgroup of the rows kernels: 64 gives every wave of rows a workgroup of its own,
// BLOCK packs four waves to a workgroup.  Measured at rows = 1024 (GC_ROWS_BLOCK, read per call,
// switches for the A/B in tools/expand_bench.py): 19.0 us per launch with 64, 27.3 with 256
// (four of these long one-lane waves on one CU instead of four CUs; not profiled further); 64 kept.
#ifndef STEP_ROWS_BLOCK
#define STEP_ROWS_BLOCK 64
#endif

struct RowsOut {
    int32_t* rw;    // [rows]
    uint8_t* dn;    // [rows]
    uint8_t* rs;    // [rows]
    int32_t* cnt;   // [rows] or null
    u64* mask;      // [65][ms], by BOARD, or null
    int8_t* obs;    // [rows][64] or null
    size_t ms;      // the mask's row stride in words
};

// the row of an index outside [0, n)
__device__ __forceinline__ void rows_bad_index(const RowsOut& o, int j) {
    o.rw[j] = 0;
    o.dn[j] = 0;
    o.rs[j] = (uint8_t)GC_REASON_BAD_INDEX;
    if (o.cnt) o.cnt[j] = -1;
    if (o.obs) {
        u64* z = reinterpret_cast<u64*>(o.obs + 64 * (size_t)j);
#pragma unroll
        for (int r = 0; r < 8; r++) z[r] = 0;
    }
}

template <bool OPP>
__global__ void __launch_bounds__(BLOCK) k_env_step_rows(EnvDev e, const int32_t* __restrict__ idx,
                                                         const uint16_t* __restrict__ acts, int rows, RowsOut out,
                                                         int autoreset) {
    LDS_SCRATCH_DECL;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= rows) return;
    const int i = idx[j];
    if ((u32)i >= (u32)e.n) {
        rows_bad_index(out, j);
        return;
    }
    Pos s = e.st.load(i);
    u32 g0 = e.hgen[i], d = e.draw[i], nst = e.nsteps[i];
    int a = (int)acts[j];
    pin(s); pin(g0); pin(d); pin(nst);
    DevHist h = e.hist(i, g0);
    PolicyCtx pc = {e.seed, (u32)i, d};
    Gen gv, g;
    MoveSet ms;
    gen_init(s, gv);
    StepOut o = OPP ? env_step_vs<true>(s, h, a, &gv, g, ms, scr, pc) : env_step<true>(s, h, a, &gv, g, ms, scr);
    bool have = o.moved;
    nst += 1;
    if (autoreset && o.done) {
        reset_board(e, s, h);
        after_reset<OPP>(e, s, h, g, ms, scr, pc);
        have = true;
    }
    if (!have) {  // state unchanged (invalid action, done, move cap, both kings checked)
        gen_init(s, g);
        gen_moves(s, g, ms, scr);
    }
    out.rw[j] = o.reward;
    out.dn[j] = (uint8_t)o.done;
    out.rs[j] = (uint8_t)o.reason;
    if (out.cnt) out.cnt[j] = ms.total;
    if (out.mask) write_mask(s, g, ms, scr, out.mask + i, out.ms);
    if (out.obs) write_obs(s, out.obs + 64 * (size_t)j);
    h.commit();
    e.st.store(i, s);
    h.flush(g0);
    e.draw[i] = pc.draw;
    e.nsteps[i] = nst;
    e.reward[i] = o.reward;
    e.done[i] = (uint8_t)o.done;
    e.reason[i] = (uint8_t)o.reason;
}

// the same under the FIDE rules (k_fenv_step_api's body)
template <bool OPP>
__global__ void __launch_bounds__(BLOCK) k_fenv_step_rows(EnvDev e, const int32_t* __restrict__ idx,
                                                          const uint16_t* __restrict__ acts, int rows, RowsOut out,
                                                          int autoreset) {
    LDS_SCRATCH_DECL;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= rows) return;
    const int i = idx[j];
    if ((u32)i >= (u32)e.n) {
        rows_bad_index(out, j);
        return;
    }
    Pos s = e.st.load(i);
    u32 g0 = e.hgen[i], d = e.draw[i], nst = e.nsteps[i];
    DevHist h = e.hist(i, g0);
    gcf::FGen f;
    const StepOut o = OPP ? gcf::fenv_step_vs<true>(s, h, (int)acts[j], f, scr, e.seed, (u32)i, d)
                          : gcf::fenv_step<true>(s, h, (int)acts[j], f);
    bool have = o.moved;
    nst += 1;
    if (autoreset && o.done) {  // (a WHITE agent: nobody opens for it)
        s = fide_reset_pos(e);
        h.bump_gen();
        gcf::fgen(s, f);
        have = true;
    }
    if (!have) gcf::fgen(s, f);
    const size_t N = out.ms;
    u64 cw = 0;  // bit c = action 4096 + c
    if (f.g.castles & 1) cw |= f.g.white ? (1ull << 1) : (1ull << 3);
    if (f.g.castles & 2) cw |= f.g.white ? (1ull << 0) : (1ull << 2);
    int total = popc(cw);
    for (int sq = 0; sq < 64; sq++) {
        const u64 tg = ((f.g.own >> sq) & 1) ? gcf::ftargets(s, f, sq, type_at(s, sq)) : 0ull;
        if (out.mask) out.mask[sq * N + i] = tg;
        total += popc(tg);
    }
    if (out.mask) out.mask[64 * N + i] = cw;
    out.rw[j] = o.reward;
    out.dn[j] = (uint8_t)o.done;
    out.rs[j] = (uint8_t)o.reason;
    if (out.cnt) out.cnt[j] = total;
    if (out.obs) write_obs(s, out.obs + 64 * (size_t)j);
    h.commit();
    e.st.store(i, s);
    h.flush(g0);
    e.draw[i] = d;
    e.nsteps[i] = nst;
    e.reward[i] = o.reward;
    e.done[i] = (uint8_t)o.done;
    e.reason[i] = (uint8_t)o.reason;
}
