// gc_host_spill.h -- the env's spill table: kernels and host policy.
#pragma once

// ----------------------------------------------------------------------------- spill table
// A BLACK agent's games have no move cap (chess_v2.py:291-292), so its 3-fold window is
// unbounded (saved_boards, chess_v2.py:192, 404-407).  Boards of a window past its per-board
// table's hist_cap go to the env's spill table (gc_env.h spill_find / spill_insert).  The
// host keeps the table's load under 1/4: after each stepping call the slot counters are
// copied to pinned memory; before the next call (or, when the copy has not landed, after at
// most SPILL_CHECK_LAG calls, synchronously) they are read, and a table past 1/4 is rehashed
// -- dead entries dropped, doubled when the live ones pass 1/8.  A failed insert (no free
// slot within SPILL_PROBES) sets a sticky flag: the next call reports it as an error, and so
// does every stepping call after it until every window is cleared (gc_env_reset of all
// boards, gc_env_set_states, gc_env_load), which starts a fresh table.
// Multi-step calls (gc_env_step_random, the fused rollouts) cannot wait for the next call:
// a launch's window generations are published only when it ends, so no entry it makes dead
// is reclaimed within it.  They run in chunks (spill_chunk): before each, the counters and a
// census of the windows within SPILL_PER_STEP x SPILL_CHUNK boards of the per-board cap are
// read, and the chunk is sized so that even if every such window spilled at every step the
// slots in use stay under half the table (rehashed / doubled first when that leaves fewer
// than SPILL_CHUNK_MIN steps).
#define SPILL_CHECK_LAG 4
#define SPILL_CHUNK 128      // steps per launch of a spill-enabled multi-step call, at most
#define SPILL_CHUNK_MIN 16   // below this many steps of room the table is rehashed / doubled first
#define SPILL_PER_STEP 2     // window boards one step adds: the agent's and the opponent's pre-move boards
#define SPILL_BITS_MAX 30    // 2^30 entries = 64 GiB

// boards whose window is within SPILL_PER_STEP x SPILL_CHUNK boards of the per-board cap
__global__ void k_spill_census(const u32* __restrict__ meta, int n, u32 thresh, u32* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool near = i < n && hl_of(meta[i]) >= thresh;
    const unsigned long long b = __ballot(near);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(out, (u32)__popcll(b));
}

__global__ void k_spill_rehash(const u64* __restrict__ old, u32 old_mask, SpillTab nt, const u32* __restrict__ hgen) {
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot > old_mask) return;
    const u64* e = old + slot * 8;
    const u64 hdr = e[0];
    const u32 o1 = sp_owner1(hdr);
    if (o1 == 0 || sp_gen(hdr) != hgen[o1 - 1]) return;  // empty or dead
    Pos b = {e[1], e[2], e[3], e[4], e[5], e[6], e[7], 0};
    DevHist h{nullptr, const_cast<u32*>(hgen), sp_gen(hdr), (int)(o1 - 1), HTAB_BITS_UNCAPPED};
    h.sp = nt;
    u32 t = sp_home(board_key(b), o1 - 1, nt.mask);
    for (int probe = 0; probe < SPILL_PROBES; probe++, t = (t + 1) & nt.mask) {
        u64 z = 0;
        if (h.sp_cas(t, z, hdr)) {
            h.sp_put(t, b);
            h.sp_claimed();
            return;
        }
    }
    h.sp_fail();
}

static int spill_bits_max() {
    const char* v = getenv("GC_SPILL_BITS_MAX");  // tests: cap the growth to force a failed insert
    return v && atoi(v) >= 6 && atoi(v) < SPILL_BITS_MAX ? atoi(v) : SPILL_BITS_MAX;
}

static int spill_bits_for(int n) {
    int b = 14;
    while (b < 22 && (1 << (b - 4)) < n) b++;  // 2^20 entries (64 MiB) at 65 536 boards
    const char* v = getenv("GC_SPILL_BITS");   // tests: start small to drive the rehash / growth path
    if (v && atoi(v) >= 6 && atoi(v) <= 30) b = atoi(v);
    return b;
}

// publish e->d.ic.spill to the device copy the paired kernels read
static int spill_publish(gc_env* e) {
    HIPCHK(hipMemcpyAsync(&e->icd->spill, &e->d.ic.spill, sizeof(SpillTab), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

static int spill_alloc(gc_env* e, int bits) {
    Temps tmps;  // the new table, until the env takes it
    SpillTab t = {nullptr, nullptr, (1u << bits) - 1};
    if (tmps.alloc(&t.ent, (size_t)8 << bits) || tmps.alloc(&t.ctr, 4)) return -1;
    hipError_t he = hipMemsetAsync(t.ent, 0, (size_t)64 << bits, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(t.ctr, 0, 16, e->stream);
    if (he == hipSuccess && !e->sp_ctr_h) {
        he = hipHostMalloc(&e->sp_ctr_h, 16, hipHostMallocDefault);
        if (he == hipSuccess) host_fill(e->sp_ctr_h, 16);
    }
    if (he == hipSuccess && !e->sp_ev) he = hipEventCreateWithFlags(&e->sp_ev, hipEventDisableTiming);
    if (he != hipSuccess) return fail(std::string("spill table: ") + hipGetErrorString(he));
    if (e->d.ic.spill.ent) (void)hipFree(e->d.ic.spill.ent);
    if (e->d.ic.spill.ctr) (void)hipFree(e->d.ic.spill.ctr);
    tmps.keep(t.ent); tmps.keep(t.ctr);
    e->d.ic.spill = t;
    e->sp_bits = bits;
    e->sp_pending = 0;
    e->sp_failed = false;
    e->sp_ctr_h[0] = e->sp_ctr_h[1] = e->sp_ctr_h[2] = 0;
    return spill_publish(e);
}

static void spill_drop(gc_env* e) {
    if (e->d.ic.spill.ent) (void)hipFree(e->d.ic.spill.ent);
    if (e->d.ic.spill.ctr) (void)hipFree(e->d.ic.spill.ctr);
    e->d.ic.spill = SpillTab{nullptr, nullptr, 0};
    e->sp_bits = 0;
    e->sp_pending = 0;
}

// rehash the live entries into a table of 2^bits slots (the stream is idle)
static int spill_rehash(gc_env* e, int bits) {
    const SpillTab old = e->d.ic.spill;
    Temps tmps;  // the new table, until the env takes it
    SpillTab t = {nullptr, nullptr, (1u << bits) - 1};
    if (tmps.alloc(&t.ent, (size_t)8 << bits) || tmps.alloc(&t.ctr, 4)) return -1;
    u32 c[2] = {0, 0};
    hipError_t he = hipMemsetAsync(t.ent, 0, (size_t)64 << bits, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(t.ctr, 0, 16, e->stream);
    if (he == hipSuccess) {
        const size_t slots = (size_t)old.mask + 1;
        k_spill_rehash<<<grid_for_slots(slots), BLOCK, 0, e->stream>>>(old.ent, old.mask, t, e->d.hgen);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(c, t.ctr, 8, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess || c[1])
        return fail(he != hipSuccess ? std::string("spill rehash: ") + hipGetErrorString(he)
                                     : std::string("spill rehash: no free slot (table of 2^") + std::to_string(bits) + ")");
    (void)hipFree(old.ent);
    (void)hipFree(old.ctr);
    tmps.keep(t.ent); tmps.keep(t.ctr);
    e->d.ic.spill = t;
    e->sp_bits = bits;
    e->sp_pending = 0;
    e->sp_ctr_h[0] = c[0];
    e->sp_ctr_h[1] = 0;
    return spill_publish(e);
}

static int spill_failed(gc_env* e) {
    e->sp_failed = true;
    return fail("repetition spill table: an insert found no free slot (a window outgrew 2^" + std::to_string(e->sp_bits) +
                " shared entries); results since then are invalid until every window is cleared (gc_env_reset of all "
                "boards, gc_env_set_states or gc_env_load)");
}

// every window was cleared (the stream is idle): a failed table starts afresh
static int spill_windows_cleared(gc_env* e) {
    if (!e->d.ic.spill.ent || !e->sp_failed) return 0;
    return spill_alloc(e, e->sp_bits);
}

// before a stepping call: the counters of the last copy that landed
static int spill_before(gc_env* e) {
    if (!e->d.ic.spill.ent) return 0;
    if (e->sp_failed) return spill_failed(e);
    if (!e->sp_pending) return 0;
    if (e->sp_pending >= SPILL_CHECK_LAG) HIPCHK(hipEventSynchronize(e->sp_ev));
    else if (hipEventQuery(e->sp_ev) != hipSuccess) return 0;  // not landed yet: check next call
    e->sp_pending = 0;
    const u32 used = e->sp_ctr_h[0], failed = e->sp_ctr_h[1];
    if (failed) return spill_failed(e);
    const u32 cap = 1u << e->sp_bits;
    if (used > cap / 4) {
        HIPCHK(hipStreamSynchronize(e->stream));
        if (spill_rehash(e, e->sp_bits)) return -1;  // drops the dead entries
        if (e->sp_ctr_h[0] > cap / 8 && e->sp_bits < spill_bits_max() && spill_rehash(e, e->sp_bits + 1)) return -1;
    }
    return 0;
}

// the steps the next launch of a multi-step call may take (<= want; synchronous): see above
static int spill_chunk(gc_env* e, int want) {
    if (!e->d.ic.spill.ent || want <= 0) return want;
    if (e->sp_failed) return spill_failed(e);
    const u32 thresh = (u32)(hist_cap(HTAB_BITS_UNCAPPED) - SPILL_PER_STEP * SPILL_CHUNK);
    bool rehashed = false;
    for (;;) {
        u32* ctr = e->d.ic.spill.ctr;
        HIPCHK(hipMemsetAsync(ctr + 2, 0, 4, e->stream));
        k_spill_census<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d.st.meta, e->n, thresh, ctr + 2);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(e->sp_ctr_h, ctr, 12, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        e->sp_pending = 0;
        const u32 used = e->sp_ctr_h[0], near = e->sp_ctr_h[2];
        if (e->sp_ctr_h[1]) return spill_failed(e);
        const uint64_t half = (uint64_t)1 << (e->sp_bits - 1);
        const uint64_t room = half > used ? half - used : 0;
        uint64_t steps = near ? room / ((uint64_t)SPILL_PER_STEP * near) : (uint64_t)SPILL_CHUNK;
        if (steps > SPILL_CHUNK) steps = SPILL_CHUNK;
        if (steps > (uint64_t)want) steps = (uint64_t)want;
        const uint64_t enough = want < SPILL_CHUNK_MIN ? (uint64_t)want : (uint64_t)SPILL_CHUNK_MIN;
        if (steps >= enough) return (int)steps;
        if (e->sp_bits >= spill_bits_max()) {
            if (steps >= 1 || rehashed) return steps >= 1 ? (int)steps : 1;  // (a failed insert would be reported)
            if (spill_rehash(e, e->sp_bits)) return -1;  // the dead entries, at least
            rehashed = true;
            continue;
        }
        // too little room: drop the dead entries first, then double
        if (spill_rehash(e, rehashed ? e->sp_bits + 1 : e->sp_bits)) return -1;
        rehashed = true;
    }
}

// after a stepping call: copy the counters (asynchronously) for the next check
static int spill_after(gc_env* e) {
    if (!e->d.ic.spill.ent) return 0;
    HIPCHK(hipMemcpyAsync(e->sp_ctr_h, e->d.ic.spill.ctr, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipEventRecord(e->sp_ev, e->stream));
    e->sp_pending++;
    return 0;
}

// the spill table's state (synchronous): log2 slots (0: none), slots in use (live + dead),
// live entries
__global__ void k_spill_live(const u64* __restrict__ ent, u32 mask, const u32* __restrict__ hgen,
                             unsigned long long* __restrict__ live) {
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot > mask) return;
    const u64 hdr = ent[slot * 8];
    const u32 o1 = sp_owner1(hdr);
    if (o1 != 0 && sp_gen(hdr) == hgen[o1 - 1]) atomicAdd(live, 1ull);
}
extern "C" int gc_env_spill_info(gc_env* e, int* bits, uint64_t* used, uint64_t* live) {
    if (!e || !bits || !used || !live) return fail("null argument");
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    *bits = e->sp_bits;
    *used = *live = 0;
    const SpillTab& sp = e->d.ic.spill;
    if (!sp.ent) return 0;
    Temps tmps;
    unsigned long long* d = nullptr;
    if (tmps.alloc(&d, 1)) return -1;
    u32 c[2] = {0, 0};
    unsigned long long lv = 0;
    hipError_t he = hipMemsetAsync(d, 0, 8, e->stream);
    if (he == hipSuccess) {
        const size_t slots = (size_t)sp.mask + 1;
        k_spill_live<<<grid_for_slots(slots), BLOCK, 0, e->stream>>>(sp.ent, sp.mask, e->d.hgen, d);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(&lv, d, 8, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(c, sp.ctr, 8, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess) return fail(std::string("spill info: ") + hipGetErrorString(he));
    *used = c[0];
    *live = lv;
    if (c[1]) return fail("repetition spill table: an insert found no free slot");
    return 0;
}
