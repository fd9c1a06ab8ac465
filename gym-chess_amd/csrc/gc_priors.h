// gc_priors.h -- legal-move priors on the device: logits [rows][row_stride] + a legal mask ->
// per row the compact child list of a search node: every legal action with its prior
// softmax(logit / T), in action-id order (gc_env_policy_priors, include/gymchess.h).
//
// The sampler's sparse mapping (gc_policy.h) with another last stage: k_policy_priors<DT, REL,
// IDX> gives a workgroup of 4 waves POL_TILE = 16 consecutive ROWS; row j describes board
// b = IDX ? board_idx[j] : j, and reads logits row j.
//   A  the tile's mask words into LDS, board-major, as the sampler does.  With IDX the column of
//      a row is its board, so a thread's 5 loads are strided 8-byte gathers (all in flight
//      together, behind the one load of the board index).  A board outside [0, n) makes the row
//      dead: its loads are clamped to column 0, its tile row is empty, count = -1.
//   B  the popcount scan to incl[] and
//   C  the k-th legal action per lane with its logit (at pol_mirror(a) when REL and board b has
//      BLACK to move) are the sampler's.
//   D  x = logit / T, max and NaN flag, e = expf(x - max) (x == max ? 0: an infinite max), S = sum
//      of e over ALL m legal actions, p_k = e_k * (1 / S): ONE reciprocal per board (an IEEE
//      division) and a multiply per lane -- at most 1.5 ulp from the quotient, far inside the
//      rule's 2e-5, and 64 divisions per chunk saved.  Boards with m <= 64 stay in registers;
//      longer lists walk their chunks twice (max, sum), a third walk writes.
//   Stores: lane k of a chunk writes slot k of the row (actions / priors / logit_idx at j * cap +
//      k), so a wave's store is contiguous; slots min(m, cap) .. cap - 1 get the padding (0xFFFF,
//      0.0f, 0xFFFF), so the whole [rows][cap] block is defined.  count[j] = m (may exceed cap).
// No scratch, no per-lane loop over the 4100-element row (the padding loop is cap / 64 stores).
#pragma once
#include "gc_policy.h"

namespace gc {

struct PriorsArgs {
    const void* logits;
    size_t row_stride;  // elements
    const u64* mask;
    size_t mask_stride;  // words, >= n
    float temperature;
    const u32* meta;           // the env's meta words (read by k_policy_priors<DT, true, IDX> only)
    const int32_t* board_idx;  // [rows] (read by k_policy_priors<DT, REL, true> only)
    int rows;
    int n;
    u32 cap;
    uint16_t* actions;    // [rows][cap]
    float* priors;        // [rows][cap]
    int32_t* count;       // [rows], may be NULL
    uint16_t* logit_idx;  // [rows][cap], may be NULL
};

// slot k of the row whose outputs start at element o
__device__ __forceinline__ void pri_store(const PriorsArgs& A, size_t o, u32 k, u32 a, float p, u32 li) {
    if (k < A.cap) {
        A.actions[o + k] = (uint16_t)a;
        A.priors[o + k] = p;
        if (A.logit_idx) A.logit_idx[o + k] = (uint16_t)li;
    }
}
// the padding of slots from .. cap - 1 (from a multiple of 64), 64 slots per step
__device__ __forceinline__ void pri_pad(const PriorsArgs& A, size_t o, u32 from, int lane) {
    for (u32 k = from + lane; k < A.cap; k += 64) pri_store(A, o, k, POL_NONE, 0.f, POL_NONE);
}

template <int DT, bool REL, bool IDX>
__global__ __launch_bounds__(64 * POL_WAVES) void k_policy_priors(const PriorsArgs A) {
    __shared__ u64 tile[POL_TILE * POL_ROWS];
    __shared__ uint16_t incl[POL_TILE * (POL_ROWS + 1)];
    __shared__ int brd[POL_TILE];  // the rows' boards, -1 = dead
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)blockIdx.x * POL_TILE;

    // A: the tile's mask words, row by row (rows past the end and dead rows: empty)
    {
        constexpr int RPP = 64 * POL_WAVES / POL_TILE;  // rows per pass
        constexpr int PASSES = (POL_ROWS + RPP - 1) / RPP;
        const int b = tid & (POL_TILE - 1);
        const size_t j = base + b;
        long long bd = -1;
        if (j < (size_t)A.rows) bd = IDX ? (long long)A.board_idx[j] : (long long)j;
        const bool live = bd >= 0 && bd < (long long)A.n;
        if (tid < POL_TILE) brd[b] = live ? (int)bd : -1;
        const size_t col = live ? (size_t)bd : (size_t)0;  // clamped: every load is in bounds,
        u64 w[PASSES];                                     // and all are in flight together
#pragma unroll
        for (int q = 0; q < PASSES; q++) {
            const int f = tid / POL_TILE + q * RPP;
            w[q] = A.mask[(size_t)(f < POL_ROWS ? f : POL_ROWS - 1) * A.mask_stride + col];
        }
#pragma unroll
        for (int q = 0; q < PASSES; q++) {
            const int f = tid / POL_TILE + q * RPP;
            if (f < POL_ROWS) tile[b * POL_ROWS + f] = !live ? 0 : f == 64 ? w[q] & 0xF : w[q];
        }
    }
    __syncthreads();
    // B: inclusive offsets per board
#pragma unroll
    for (int j = 0; j < POL_PER_WAVE; j++) {
        const int b = wave * POL_PER_WAVE + j;
        const u64* row = tile + b * POL_ROWS;
        const u32 c = pol_wave_scan((u32)__popcll(row[lane]));
        incl[b * (POL_ROWS + 1) + lane] = (uint16_t)c;
        if (lane == 63) incl[b * (POL_ROWS + 1) + 64] = (uint16_t)(c + __popcll(row[64]));
    }
    __syncthreads();

    // is the row of tile slot b read mirrored?
    auto mirrored = [&](int b) {
        if (!REL) return false;
        const int bd = brd[b];
        return bd >= 0 && !(A.meta[bd] & M_WHITE);
    };

    // C: the first 64 legal actions of the wave's rows and their logits (idle lanes read element
    // 0 of the buffer and drop it)
    u32 act0[POL_PER_WAVE], raw0[POL_PER_WAVE];
#pragma unroll
    for (int j = 0; j < POL_PER_WAVE; j++) {
        const int b = wave * POL_PER_WAVE + j;
        const u32 m = incl[b * (POL_ROWS + 1) + 64];
        const bool on = (u32)lane < m;
        const u32 a = pol_kth_action(tile + b * POL_ROWS, incl + b * (POL_ROWS + 1), on ? (u32)lane : 0u);
        act0[j] = a;
        const u32 at = mirrored(b) ? pol_mirror(a) : a;
        raw0[j] = pol_load<DT>(A.logits, on ? (base + b) * A.row_stride + at : (size_t)0);
    }

    // D1: the rows whose list fits one chunk (m <= 64), out of the registers loaded above
    const float ninf = -__builtin_inff();
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int j = 0; j < POL_PER_WAVE; j++) {
        const int b = wave * POL_PER_WAVE + j;
        const size_t r = base + b;
        const u32 m = incl[b * (POL_ROWS + 1) + 64];
        if (r >= (size_t)A.rows || m > 64) continue;
        const size_t o = r * A.cap;
        const bool on = (u32)lane < m;
        float p = 0.f;
        if (m) {
            // x = logit / T, -inf on idle lanes (they then drop out of every sum: exp(-inf) = 0)
            const float x = on ? pol_value<DT>(raw0[j]) / A.temperature : ninf;
            const bool bad = __ballot(x != x) != 0;
            const float mx = pol_wave_max(x);
            if (bad || mx == ninf) {
                p = nan;
            } else {
                const float e = expf(x == mx ? 0.f : x - mx);
                p = e * (1.0f / pol_wave_sum(e));
            }
        }
        const u32 a = act0[j];
        pri_store(A, o, (u32)lane, on ? a : POL_NONE, on ? p : 0.f, !on ? POL_NONE : mirrored(b) ? pol_mirror(a) : a);
        pri_pad(A, o, 64, lane);
        if (lane == 0 && A.count) A.count[r] = brd[b] < 0 ? -1 : (int32_t)m;
    }

    // D2: longer lists (rare in chess), 64 actions per step, gathered again in each of three
    // passes (the later ones hit L2): max and NaN; the sum; the priors
    for (int j = 0; j < POL_PER_WAVE; j++) {
        const int b = wave * POL_PER_WAVE + j;
        const size_t r = base + b;
        const u64* row = tile + b * POL_ROWS;
        const uint16_t* inc = incl + b * (POL_ROWS + 1);
        const u32 m = inc[64];
        if (r >= (size_t)A.rows || m <= 64) continue;
        const size_t o = r * A.cap;
        const u32 chunks = (m + 63) >> 6;
        const size_t rbase = r * A.row_stride;
        const bool mir = mirrored(b);
        // chunk c: the lane's action, where its logit sits and x = logit / T (-inf on idle lanes)
        auto fetch = [&](u32 c, u32& a, u32& at, float& x) {
            const u32 k = c * 64 + lane;
            const bool on = k < m;
            a = pol_kth_action(row, inc, on ? k : 0u);
            at = mir ? pol_mirror(a) : a;
            const u32 raw = pol_load<DT>(A.logits, on ? rbase + at : (size_t)0);
            x = on ? pol_value<DT>(raw) / A.temperature : ninf;
        };
        float mx = ninf;
        bool bad = false;
        for (u32 c = 0; c < chunks; c++) {
            u32 a, at;
            float x;
            fetch(c, a, at, x);
            bad |= __ballot(x != x) != 0;
            mx = fmaxf(mx, x);
        }
        mx = pol_wave_max(mx);
        const bool unusable = bad || mx == ninf;
        float inv = nan;
        if (!unusable) {
            float S = 0.f;
            for (u32 c = 0; c < chunks; c++) {
                u32 a, at;
                float x;
                fetch(c, a, at, x);
                S += expf(x == mx ? 0.f : x - mx);
            }
            inv = 1.0f / pol_wave_sum(S);
        }
        const u32 wchunks = ((m < A.cap ? m : A.cap) + 63) >> 6;  // the chunks with a slot to fill
        for (u32 c = 0; c < wchunks; c++) {
            u32 a, at;
            float x;
            fetch(c, a, at, x);
            const u32 k = c * 64 + lane;
            const bool on = k < m;
            const float p = unusable ? nan : expf(x == mx ? 0.f : x - mx) * inv;
            pri_store(A, o, k, on ? a : POL_NONE, on ? p : 0.f, on ? at : POL_NONE);
        }
        pri_pad(A, o, wchunks * 64, lane);
        if (lane == 0 && A.count) A.count[r] = (int32_t)m;
    }
}

}  // namespace gc
