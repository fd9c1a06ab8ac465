// gc_stamps.h -- diagnostic builds only (-DGC_STAMPS, -DGC_PSTAMPS): per-wave clock stamps of the
// kernels' segments, kept in LDS, and the empty PST* macros of every other build.  Included by
// gymchess.hip first of all, before gc_core.h (it needs the HIP runtime alone).
#pragma once

#ifdef GC_STAMPS
// diagnostic build only: per-wave s_memtime stamps (MI355X guide, "In-kernel stamps")
__shared__ unsigned long long gc_stamp_lds[4][8];
__device__ __forceinline__ void gc_stamp(int k) {
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t;
#ifdef GC_STAMPS_REAL  // the 100 MHz constant clock, comparable across CUs (launch ramp / tail)
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    if (k == 0) {  // placement of the wave in bits 44+ of its first stamp: cu | sh | se | simd | xcc
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)"
                     : "=s"(hw), "=s"(xcc));
        unsigned long long where = ((hw >> 8) & 0xF) | (((hw >> 12) & 1) << 4) | (((hw >> 13) & 3) << 5) |
                                   (((hw >> 4) & 3) << 7) | ((unsigned long long)(xcc & 0xF) << 9);
        t = (t & ((1ull << 44) - 1)) | (where << 44);
    }
#else
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
#endif
    __builtin_amdgcn_sched_barrier(0);
    if ((threadIdx.x & 63) == 0) gc_stamp_lds[threadIdx.x >> 6][k] = t;
}
#define GC_STAMP(k) gc_stamp(k)
#endif
#ifdef GC_PSTAMPS
// diagnostic build only: per wave, the cycles of each segment of the fused ply (phase work
// and barrier waits), summed over the launch's plies (tools/pstamp_probe.py)
__shared__ unsigned long long gc_pst[8][9];  // [wave][segment 0..7, last stamp]
__device__ unsigned long long* g_pst_out;
__device__ __forceinline__ void gc_pst_mark(int k) {
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        gc_pst[w][k] += t - gc_pst[w][8];
        gc_pst[w][8] = t;
    }
    __builtin_amdgcn_sched_barrier(0);
}
#define PST(k) gc_pst_mark(k)
// the quad rollout's Q1, phase 2, split by whether any lane of the wave loaded a window slot
// beyond its home slot in this ply (rep_commit's in-loop load): per wave, the plies that did
// and the cycles of their phase 2
__shared__ unsigned long long gc_pst_run[8][2];
__device__ unsigned long long* g_pst_run_out;
__device__ __forceinline__ void gc_pst_mark_run(int k, bool loaded) {
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    const bool any = __any(loaded);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        gc_pst[w][k] += t - gc_pst[w][8];
        if (any) {
            gc_pst_run[w][0] += 1;
            gc_pst_run[w][1] += t - gc_pst[w][8];
        }
        gc_pst[w][8] = t;
    }
    __builtin_amdgcn_sched_barrier(0);
}
#define PST_LOADED(x) do { if (x) pst_loaded = true; } while (0)
// the quad rollout, one quad per workgroup: which role arrives last at each of the ply's four
// barriers (A, B, C, D) and by how much.  A wave leaves its arrival stamp (the segment stamp just
// taken) before the barrier; after it each wave reads the four and the last one counts itself, in
// bins of PST_BIN_CYCLES of its margin over the next to last (the last bin: all above), and adds
// the margin up.  A slot is written again three barriers later, which every reader has to reach
// first.
#define PST_BINS 16
#define PST_BIN_CYCLES 128
__shared__ unsigned long long gc_pst_arr[4][4];      // [barrier][wave]
__shared__ unsigned gc_pst_last[4][4][PST_BINS + 1];  // [wave][barrier][bin .. , the margins' sum]
__device__ unsigned* g_pst_last_out;
__device__ __forceinline__ void gc_pst_arrive(int b) {
    __builtin_amdgcn_sched_barrier(0);
    if ((threadIdx.x & 63) == 0) gc_pst_arr[b][(threadIdx.x >> 6) & 3] = gc_pst[threadIdx.x >> 6][8];
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void gc_pst_count_last(int b) {
    __builtin_amdgcn_sched_barrier(0);
    if ((threadIdx.x & 63) == 0) {
        const int w = (threadIdx.x >> 6) & 3;
        const unsigned long long mine = gc_pst_arr[b][w];
        unsigned long long next = 0;  // the latest of the others
        bool last = true;
        for (int o = 0; o < 4; o++) {
            if (o == w) continue;
            const unsigned long long t = gc_pst_arr[b][o];
            last = last && (t < mine || (t == mine && o > w));
            next = t > next ? t : next;
        }
        if (last) {
            const unsigned long long m = mine - next;
            const unsigned bin = (unsigned)(m / PST_BIN_CYCLES);
            gc_pst_last[w][b][bin < PST_BINS - 1 ? bin : PST_BINS - 1] += 1u;
            gc_pst_last[w][b][PST_BINS] += (unsigned)m;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}
#define PST_ARRIVE(b) gc_pst_arrive(b)
#define PST_LAST(b) gc_pst_count_last(b)
#else
#define PST(k)
#define PST_LOADED(x)
#define PST_ARRIVE(b) ((void)0)
#define PST_LAST(b) ((void)0)
#endif
