// gc_policy.h -- policy head on the device: logits [N][row_stride] + the step's legal mask ->
// action, log-prob, entropy per board (gc_env_sample_policy, include/gymchess.h).
//
// The work is sparse: a position has ~30 legal actions of 4100, so the kernel walks the mask's
// bits and gathers only those logits (a few cache lines per board; a dense pass reads 16.4 KB).
//
// Mapping (k_sample_policy): a workgroup of 4 waves owns POL_TILE = 16 consecutive boards.
//   A  every thread copies mask words of the tile into LDS: the 65 rows are contiguous across
//      boards, so a row's 16 words are one 128-byte read, and a thread's 5 reads are all in
//      flight together; the tile lands board-major (tile[b][65], stride 65 words: the stores
//      and the later per-board row reads are conflict-free).  Row 64 keeps its four castle bits.
//      (32 boards per workgroup, 256-byte reads: 42 against 38 us per launch at N = 65 536 --
//      the smaller workgroups fill the CUs more evenly.)
//   B  one wave per board (4 boards per wave): lane f popcounts word f, a wave scan gives the
//      inclusive offsets incl[b][0..64] (incl[b][64] = m, the legal count).
//   C  the k-th legal action, k = 64 * chunk + lane: a 7-step search of incl for its word, a
//      6-step select of its bit -- 64 actions per step whatever their from-squares (a queen's 27
//      targets spread over 27 lanes).  The first chunk's logits of the wave's 4 boards are all
//      requested before any is used (4 gathers in flight per wave).
//   D  per board: max and NaN flag, sum of exp and of exp * (x - max), then (sampling) a wave
//      scan for the CDF.  Boards with m <= 64 never leave registers (D1); longer lists walk
//      their chunks in three passes, gathering each time (D2: rare, and L2-resident).
// In k_sample_policy<DT, true> (flags bit 1) the row is relative to the side to move: on a board
// with BLACK to move the logit of action a is read at pol_mirror(a); the actions themselves,
// their order and the outputs stay absolute.
// No per-lane loop over the row, no division but the logit's by the temperature, no scratch.
#pragma once
#include <hipcub/hipcub.hpp>

#include "gc_core.h"

namespace gc {

#define POL_TILE 16                      // boards per workgroup
#define POL_WAVES 4                      // waves per workgroup
#define POL_PER_WAVE (POL_TILE / POL_WAVES)
#define POL_ROWS 65                      // mask words per board
#define POL_NONE 0xFFFFu                 // "no legal move" / unusable logits

struct PolicyArgs {
    const void* logits;
    size_t row_stride;  // elements
    const u64* mask;
    size_t mask_stride;  // words, >= n
    float temperature;
    u64 seed;
    u32 draw;
    int greedy;
    const u32* meta;  // the env's meta words (read by k_sample_policy<DT, true> only)
    uint16_t* action;
    float* logprob;  // may be NULL
    float* entropy;  // may be NULL
    int n;
};

// DT 0 fp32, 1 fp16, 2 bf16: the raw element (the conversion waits for the load, so it is kept
// apart from it) and its exact fp32 value
template <int DT>
__device__ __forceinline__ u32 pol_load(const void* base, size_t idx) {
    if (DT == 0) return ((const u32*)base)[idx];
    return ((const uint16_t*)base)[idx];
}
template <int DT>
__device__ __forceinline__ float pol_value(u32 raw) {
    if (DT == 0) return __uint_as_float(raw);
    if (DT == 1) {
        union { uint16_t u; _Float16 h; } c;
        c.u = (uint16_t)raw;
        return (float)c.h;
    }
    return __uint_as_float(raw << 16);
}

// Where the logit of action a sits in a row that is relative to the side to move, on a board with
// BLACK to move: from and to mirrored (sq ^ 56), the castles' colours swapped.  An involution.
__device__ __forceinline__ u32 pol_mirror(u32 a) { return a < 4096u ? a ^ 0xE38u : 4096u + ((a - 4096u) ^ 2u); }
// is board i's row mirrored?  (REL = flags bit 1; without it the env's state is not read and the
// kernel is the absolute one, instruction for instruction)
template <bool REL>
__device__ __forceinline__ bool pol_mirrored(const PolicyArgs& A, int i) {
    if (!REL) return false;
    return i < A.n && !(A.meta[i] & M_WHITE);
}

// Wave-wide reductions and scans through rocPRIM's DPP forms (row shifts and broadcasts in the
// VALU; the ds_bpermute forms of __shfl cost an LDS round trip per step, and the six dependent
// steps of each were most of this kernel's time).  Their temporary storage is empty for wave64.
using PolReduce = hipcub::WarpReduce<float, 64>;
using PolScan = hipcub::WarpScan<float, 64>;
using PolScanU = hipcub::WarpScan<u32, 64>;
__device__ __forceinline__ float pol_first_lane(float v) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}
__device__ __forceinline__ float pol_wave_max(float v) {
    PolReduce::TempStorage ts;
    return pol_first_lane(PolReduce(ts).Reduce(v, hipcub::Max()));
}
__device__ __forceinline__ float pol_wave_sum(float v) {
    PolReduce::TempStorage ts;
    return pol_first_lane(PolReduce(ts).Sum(v));
}
__device__ __forceinline__ float pol_wave_scan(float v) {  // inclusive
    PolScan::TempStorage ts;
    float out;
    PolScan(ts).InclusiveSum(v, out);
    return out;
}
__device__ __forceinline__ u32 pol_wave_scan(u32 v) {  // inclusive
    PolScanU::TempStorage ts;
    u32 out;
    PolScanU(ts).InclusiveSum(v, out);
    return out;
}

// the k-th legal action (k < m) of a board from its LDS mask row and inclusive offsets
__device__ __forceinline__ u32 pol_kth_action(const u64* row, const uint16_t* incl, u32 k) {
    u32 f = 0;  // f = #{j < 64 : incl[j] <= k}: words 0..f-1 hold the first incl[f-1] <= k legal actions
#pragma unroll
    for (u32 s = 64; s; s >>= 1) {
        const u32 mid = f + s;
        if (mid <= 64 && incl[mid - 1] <= k) f = mid;
    }
    u32 r = k - (f ? incl[f - 1] : 0u);  // the r-th set bit of word f
    const u64 w = row[f];
    u32 v = (u32)w, pos = 0;
    u32 c = __popc(v);
    if (r >= c) { r -= c; pos = 32; v = (u32)(w >> 32); }
#pragma unroll
    for (u32 s = 16; s; s >>= 1) {
        c = __popc(v & ((1u << s) - 1u));
        if (r >= c) { r -= c; pos += s; v >>= s; }
    }
    return f * 64u + pos;
}

template <int DT, bool REL>
__global__ __launch_bounds__(64 * POL_WAVES) void k_sample_policy(const PolicyArgs A) {
    __shared__ u64 tile[POL_TILE * POL_ROWS];
    __shared__ uint16_t incl[POL_TILE * (POL_ROWS + 1)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = blockIdx.x * POL_TILE;

    // A: the tile's mask words, row by row (boards past n: empty)
    {
        constexpr int RPP = 64 * POL_WAVES / POL_TILE;         // rows per pass
        constexpr int PASSES = (POL_ROWS + RPP - 1) / RPP;
        const int b = tid & (POL_TILE - 1);
        const bool live = base + b < A.n;
        const size_t col = (size_t)(live ? base + b : A.n - 1);  // clamped: every load is in bounds,
        u64 w[PASSES];                                           // and all are in flight together
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

    // C: the first 64 legal actions of the wave's boards and their logits (idle lanes read
    // element 0 of the buffer and drop it)
    u32 act0[POL_PER_WAVE], raw0[POL_PER_WAVE];
#pragma unroll
    for (int j = 0; j < POL_PER_WAVE; j++) {
        const int b = wave * POL_PER_WAVE + j;
        const u32 m = incl[b * (POL_ROWS + 1) + 64];
        const bool on = (u32)lane < m;
        const u32 a = pol_kth_action(tile + b * POL_ROWS, incl + b * (POL_ROWS + 1), on ? (u32)lane : 0u);
        act0[j] = a;
        const u32 at = pol_mirrored<REL>(A, base + b) ? pol_mirror(a) : a;
        raw0[j] = pol_load<DT>(A.logits, on ? (size_t)(base + b) * A.row_stride + at : (size_t)0);
    }

    // D1: the boards whose list fits one chunk (m <= 64), out of the registers loaded above
    const float ninf = -__builtin_inff();
#pragma unroll
    for (int j = 0; j < POL_PER_WAVE; j++) {
        const int b = wave * POL_PER_WAVE + j;
        const int i = base + b;
        const u32 m = incl[b * (POL_ROWS + 1) + 64];
        if (i >= A.n || m > 64) continue;
        uint16_t out_a = (uint16_t)POL_NONE;
        float out_lp = 0.f, out_h = 0.f;
        if (m) {
            // x = logit / T, -inf on idle lanes (they then drop out of every sum: exp(-inf) = 0)
            const float x = (u32)lane < m ? pol_value<DT>(raw0[j]) / A.temperature : ninf;
            const bool bad = __ballot(x != x) != 0;
            const float mx = pol_wave_max(x);
            if (bad || mx == ninf) {
                out_lp = out_h = __builtin_nanf("");
            } else {
                const float d = x == mx ? 0.f : x - mx;
                const float e = expf(d);
                const float S = pol_wave_sum(e);
                const float W = pol_wave_sum(e > 0.f ? e * d : 0.f);
                const float logS = logf(S);
                int l;
                if (A.greedy) {  // the lowest action id at the maximum
                    l = __ffsll((long long)__ballot(x == mx)) - 1;
                } else {  // the first k with u * S < e_1 + ... + e_k (and e_k > 0: a rounded
                          // scan is not monotone); else the last k of positive probability
                    const float u = (float)(philox_x0(A.seed, (u32)i, A.draw) >> 8) * (1.0f / 16777216.0f);
                    const float sc = pol_wave_scan(e);
                    const u64 hit = __ballot(e > 0.f && u * S < sc);
                    l = hit ? __ffsll((long long)hit) - 1 : 63 - __clzll((long long)__ballot(e > 0.f));
                }
                out_a = (uint16_t)__shfl(act0[j], l, 64);
                out_lp = __shfl(d, l, 64) - logS;
                out_h = logS - W / S;
            }
        }
        if (lane == 0) {
            A.action[i] = out_a;
            if (A.logprob) A.logprob[i] = out_lp;
            if (A.entropy) A.entropy[i] = out_h;
        }
    }

    // D2: longer lists (rare in chess), 64 actions per step, gathered again in each of three
    // passes (the later ones hit L2): max and NaN; the sums; the CDF
    for (int j = 0; j < POL_PER_WAVE; j++) {
        const int b = wave * POL_PER_WAVE + j;
        const int i = base + b;
        const u64* row = tile + b * POL_ROWS;
        const uint16_t* inc = incl + b * (POL_ROWS + 1);
        const u32 m = inc[64];
        if (i >= A.n || m <= 64) continue;
        const u32 chunks = (m + 63) >> 6;
        const size_t rbase = (size_t)i * A.row_stride;
        const bool mir = pol_mirrored<REL>(A, i);
        // chunk c: the lane's action and x = logit / T (-inf on idle lanes)
        auto fetch = [&](u32 c, u32& a, float& x) {
            const u32 k = c * 64 + lane;
            const bool on = k < m;
            a = pol_kth_action(row, inc, on ? k : 0u);
            const u32 raw = pol_load<DT>(A.logits, on ? rbase + (mir ? pol_mirror(a) : a) : (size_t)0);
            x = on ? pol_value<DT>(raw) / A.temperature : ninf;
        };
        uint16_t out_a = (uint16_t)POL_NONE;
        float out_lp, out_h;
        float mx = ninf;
        bool bad = false;
        for (u32 c = 0; c < chunks; c++) {
            u32 a;
            float x;
            fetch(c, a, x);
            bad |= __ballot(x != x) != 0;
            mx = fmaxf(mx, x);
        }
        mx = pol_wave_max(mx);
        if (bad || mx == ninf) {
            out_lp = out_h = __builtin_nanf("");
        } else {
            float S = 0.f, W = 0.f;
            u32 pick = POL_NONE;
            for (u32 c = 0; c < chunks; c++) {
                u32 a;
                float x;
                fetch(c, a, x);
                const float d = x == mx ? 0.f : x - mx;
                const float e = expf(d);
                S += e;
                W += e > 0.f ? e * d : 0.f;
                if (A.greedy && pick == POL_NONE) {
                    const u64 bal = __ballot(x == mx);
                    if (bal) pick = __shfl(a, __ffsll((long long)bal) - 1, 64);
                }
            }
            S = pol_wave_sum(S);
            W = pol_wave_sum(W);
            const float logS = logf(S);
            float dsel = 0.f;
            if (!A.greedy) {
                const float u = (float)(philox_x0(A.seed, (u32)i, A.draw) >> 8) * (1.0f / 16777216.0f);
                const float thr = u * S;
                float run = 0.f;
                u32 last_a = POL_NONE;
                float last_d = 0.f;
                for (u32 c = 0; c < chunks && pick == POL_NONE; c++) {
                    u32 a;
                    float x;
                    fetch(c, a, x);
                    const float d = x == mx ? 0.f : x - mx;
                    const float e = expf(d);
                    const float sc = pol_wave_scan(e);
                    const u64 hit = __ballot(e > 0.f && thr < run + sc);
                    const u64 pos = __ballot(e > 0.f);
                    if (hit) {
                        const int l = __ffsll((long long)hit) - 1;
                        pick = __shfl(a, l, 64);
                        dsel = __shfl(d, l, 64);
                    } else if (pos) {
                        const int l = 63 - __clzll((long long)pos);
                        last_a = __shfl(a, l, 64);
                        last_d = __shfl(d, l, 64);
                    }
                    run += __shfl(sc, 63, 64);
                }
                if (pick == POL_NONE) {
                    pick = last_a;
                    dsel = last_d;
                }
            }
            out_a = (uint16_t)pick;
            out_lp = dsel - logS;
            out_h = logS - W / S;
        }
        if (lane == 0) {
            A.action[i] = out_a;
            if (A.logprob) A.logprob[i] = out_lp;
            if (A.entropy) A.entropy[i] = out_h;
        }
    }
}

}  // namespace gc
