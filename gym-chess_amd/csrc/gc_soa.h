// gc_soa.h -- how the kernels reach a board in HBM: the structure-of-arrays state (SoA), the env's
// spill table (SpillTab), a board's 3-fold window (DevHist) and the per-lane LDS scratch.
// Included by gymchess.hip after gc_core.h / gc_env.h, NBB and BLOCK, before every kernel.
#pragma once

// ----------------------------------------------------------------------------- SoA access
struct SoA {
    u64* bb;   // [7][N]
    u32* meta; // [N]
    int n;
    __device__ Pos load(int i) const {
        Pos s;
        s.k = bb[0 * (size_t)n + i]; s.q = bb[1 * (size_t)n + i]; s.r = bb[2 * (size_t)n + i];
        s.b = bb[3 * (size_t)n + i]; s.n = bb[4 * (size_t)n + i]; s.p = bb[5 * (size_t)n + i];
        s.w = bb[6 * (size_t)n + i];
        s.meta = meta[i];
        return s;
    }
    __device__ void store(int i, const Pos& s) const {
        bb[0 * (size_t)n + i] = s.k; bb[1 * (size_t)n + i] = s.q; bb[2 * (size_t)n + i] = s.r;
        bb[3 * (size_t)n + i] = s.b; bb[4 * (size_t)n + i] = s.n; bb[5 * (size_t)n + i] = s.p;
        bb[6 * (size_t)n + i] = s.w;
        meta[i] = s.meta;
    }
};

// The env's spill table (gc_env.h spill_find / spill_insert): 64-B entries shared by the
// boards of a BLACK-agent env whose windows outgrow their per-board tables; ctr[0] = slots
// ever claimed, ctr[1] = sticky "no free slot" flag (both read by the host, gc_env_*).
struct SpillTab {
    u64* ent;  // [mask + 1][8]
    u32* ctr;
    u32 mask;  // 0: no spill table (every env but a BLACK agent's)
};

// repetition window of board i (gc_env.h rep_prefetch / rep_commit): HTAB 64-byte entries
// per board (entry() below), one cache line each (4 x 16-B loads); generation [N]
struct DevHist {
    u64* htab;
    u32* hgen;
    u32 g;
    int i;
    int nb = HTAB_BITS;  // log2 entries per board (gc_env.h: 9, or 10 for a BLACK agent)
    // Wave-blocked layout: entry pos of board i at ((i/64)*HTAB + pos)*64 + i%64, i.e. the 64
    // boards of a wave share one 4 MiB block and a wave's 64 probes land on 64 random 4 KiB
    // rows of it.  Board-major tables (64 KiB per board) put a wave's probes 64 KiB apart, on
    // the same HBM channels: tools/lat_probe.hip measures 9.6 vs 5.5 us per launch for one
    // random 64-B read + write per board at 65 536 boards.
    __device__ size_t entry(int pos) const { return ((((size_t)(i >> 6)) << nb) + pos) * 64 + (i & 63); }
    __device__ int bits() const { return nb; }
    __device__ u32 gen() const { return g; }
    __device__ void bump_gen() { g++; }                // written back by flush()
    __device__ void flush(u32 g0) const { if (g != g0) hgen[i] = g; }
    __device__ RepEntry load(int pos) const {
        const ulonglong2* p = reinterpret_cast<const ulonglong2*>(htab + entry(pos) * 8);
        ulonglong2 a = p[0], b = p[1], c = p[2], d = p[3];
        RepEntry e = {a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
        return e;
    }
    // Table writes are recorded and issued by commit() at the end of the step: a store
    // issued mid-kernel makes the compiler wait (vmcnt) before reusing its data registers.
    int wkind = 0, wpos = 0;  // 0 none, 1 header only, 2 whole entry
    RepEntry we;
    __device__ void store_hdr(int pos, u64 h) { wkind = 1; wpos = pos; we.hdr = h; }
    __device__ void store(int pos, const RepEntry& e) { wkind = 2; wpos = pos; we = e; }
    __device__ void commit() {
        u64* base = htab + entry(wpos) * 8;
        if (wkind == 1) {
            base[0] = we.hdr;
        } else if (wkind == 2) {
            ulonglong2* p = reinterpret_cast<ulonglong2*>(base);
            p[0] = make_ulonglong2(we.hdr, we.k);
            p[1] = make_ulonglong2(we.q, we.r);
            p[2] = make_ulonglong2(we.b, we.n);
            p[3] = make_ulonglong2(we.p, we.w);
        }
        wkind = 0;
    }
    // the spill table (gc_env.h): headers through device-coherent atomics -- other boards'
    // lanes, on any XCD, claim slots concurrently; a board's own entry bodies are written and
    // read only by its own lane (or by later launches)
    SpillTab sp = {nullptr, nullptr, 0};
    __device__ u32 spill_mask() const { return sp.mask; }
    __device__ u32 owner() const { return (u32)i; }
    __device__ u64 sp_hdr(u32 slot) const {
        return __hip_atomic_load(sp.ent + (size_t)slot * 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ bool sp_cas(u32 slot, u64& expect, u64 desired) const {
        return __hip_atomic_compare_exchange_strong(sp.ent + (size_t)slot * 8, &expect, desired, __ATOMIC_RELAXED,
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ void sp_set_hdr(u32 slot, u64 v) const {
        __hip_atomic_store(sp.ent + (size_t)slot * 8, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ void sp_put(u32 slot, const Pos& s) const {
        u64* d = sp.ent + (size_t)slot * 8;
        d[1] = s.k; d[2] = s.q; d[3] = s.r; d[4] = s.b; d[5] = s.n; d[6] = s.p; d[7] = s.w;
    }
    __device__ bool sp_same(u32 slot, const Pos& s) const {
        const u64* d = sp.ent + (size_t)slot * 8;
        return d[1] == s.k && d[2] == s.q && d[3] == s.r && d[4] == s.b && d[5] == s.n && d[6] == s.p && d[7] == s.w;
    }
    __device__ u32 sp_owner_gen(u32 o) const { return __hip_atomic_load(hgen + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ void sp_claimed() const { __hip_atomic_fetch_add(sp.ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ void sp_fail() const { __hip_atomic_fetch_or(sp.ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// per-lane move-target scratch in LDS: slot j of lane t at lds[j*BLOCK + t] (each wave's
// ds_read_b64/ds_write_b64 touches 512 contiguous bytes: conflict-free)
struct LdsScratch {
    static constexpr bool kPark = true;
    u64* base;
    __device__ void put(int j, u64 v) { base[j * BLOCK] = v; }
    __device__ u64 get(int j) const { return base[j * BLOCK]; }
};
#define LDS_SCRATCH_DECL __shared__ u64 lds_scr[SCRATCH_SLOTS * BLOCK]; LdsScratch scr{lds_scr + threadIdx.x}
