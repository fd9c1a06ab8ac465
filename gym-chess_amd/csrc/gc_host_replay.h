// gc_host_replay.h -- gc_replay_*: the sample store's handle, its one device allocation and the
// launches of gc_replay.h's kernels, all asynchronous on the env's stream.
#pragma once

struct gc_replay {
    gc_env* e = nullptr;
    int device = 0;
    ReplayDev d{};
    uint8_t* slab = nullptr;  // every array of d, 256-byte aligned, in GC_REPLAY_ARRAYS order
    size_t bytes = 0;
};

// the arrays' sizes in bytes, in the header's order
static void replay_sizes(size_t G, size_t cap, size_t plies, size_t ring, size_t out[GC_REPLAY_ARRAYS]) {
    const size_t p = G * plies;
    const size_t s[GC_REPLAY_ARRAYS] = {64 * p, 2 * p * cap, 4 * p * cap, 64 * ring, 2 * ring * cap, 4 * ring * cap,
                                        4 * ring, 4 * G,       4 * G,       8,         4 * G,          8};
    for (int k = 0; k < GC_REPLAY_ARRAYS; k++) out[k] = s[k];
}
static inline dim3 replay_grid(const gc_replay* r) { return dim3((unsigned)((r->d.games + RPL_WAVES - 1) / RPL_WAVES)); }

extern "C" int gc_replay_create(gc_env* e, int games, int cap, int max_plies, int64_t capacity, gc_replay** out) {
    if (!e || !out) return fail("null argument");
    if (games < 1 || games > e->n) return fail("games must be in [1, the env's boards]");
    if (cap < 1 || cap > RPL_MAX_CAP) return fail("cap must be in [1, 256]");
    if (max_plies < 1) return fail("max_plies must be >= 1");
    if (capacity < (int64_t)games * max_plies) return fail("capacity must be >= games * max_plies");
    if (capacity > INT32_MAX) return fail("capacity must be below 2^31 (slots are int32)");
    HIPCHK(hipSetDevice(e->device));
    size_t sz[GC_REPLAY_ARRAYS], off[GC_REPLAY_ARRAYS], total = 0;
    replay_sizes((size_t)games, (size_t)cap, (size_t)max_plies, (size_t)capacity, sz);
    for (int k = 0; k < GC_REPLAY_ARRAYS; k++) {
        off[k] = total;
        total += (sz[k] + 255) & ~(size_t)255;
    }
    gc_replay* r = new gc_replay();
    if (dalloc(&r->slab, total)) {
        delete r;
        return -1;
    }
    hipError_t rc = hipMemsetAsync(r->slab, 0, total, e->stream);
    if (rc != hipSuccess) {
        (void)hipFree(r->slab);
        delete r;
        return fail(std::string("hipMemsetAsync: ") + hipGetErrorString(rc));
    }
    r->e = e;
    r->device = e->device;
    r->bytes = total;
    uint8_t* b = r->slab;
    ReplayDev& d = r->d;
    d.pend_pos = (u64*)(b + off[0]);
    d.pend_act = (uint16_t*)(b + off[1]);
    d.pend_vis = (int32_t*)(b + off[2]);
    d.ring_pos = (u64*)(b + off[3]);
    d.ring_act = (uint16_t*)(b + off[4]);
    d.ring_vis = (int32_t*)(b + off[5]);
    d.ring_z = (float*)(b + off[6]);
    d.plies = (int32_t*)(b + off[7]);
    d.dropped = (int32_t*)(b + off[8]);
    d.total = (u64*)(b + off[9]);
    d.off = (int32_t*)(b + off[10]);
    d.base = (u64*)(b + off[11]);
    d.games = games;
    d.cap = cap;
    d.max_plies = max_plies;
    d.capacity = (int)capacity;
    *out = r;
    return 0;
}

extern "C" int gc_replay_destroy(gc_replay* r) {
    if (!r) return fail("null store");
    (void)hipSetDevice(r->device);  // (not through e: the env may be gone already)
    if (r->slab) (void)hipFree(r->slab);  // (waits for the device: no launch still uses the arrays)
    delete r;
    return 0;
}

extern "C" int gc_replay_clear(gc_replay* r) {
    if (!r) return fail("null store");
    SRV_QUIESCE(r->e);
    HIPCHK(hipSetDevice(r->e->device));
    HIPCHK(hipMemsetAsync(r->slab, 0, r->bytes, r->e->stream));
    return 0;
}

extern "C" int gc_replay_record(gc_replay* r, const uint16_t* d_actions, const int32_t* d_visits, int row_cap) {
    if (!r) return fail("null store");
    if (!d_actions || !d_visits) return fail("null actions / visits block");
    if (row_cap < 1 || row_cap > r->d.cap) return fail("row_cap must be in [1, the store's cap]");
    gc_env* e = r->e;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    ReplayEnv v;
    v.bb = e->d.st.bb;
    v.meta = e->d.st.meta;
    v.hgen = e->d.hgen;
    v.htab = e->d.htab;
    v.sp = e->d.ic.spill;
    v.n = e->n;
    v.hbits = e->d.hbits;
    k_replay_record<<<replay_grid(r), dim3(64 * RPL_WAVES), 0, e->stream>>>(r->d, v, d_actions, d_visits, row_cap);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gc_replay_commit(gc_replay* r, const uint8_t* d_done, const uint8_t* d_reason, const float* d_outcome) {
    if (!r) return fail("null store");
    if (!d_done) return fail("null done array");
    if (!d_reason && !d_outcome) return fail("null reason array without an outcome array");
    gc_env* e = r->e;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    k_replay_scan<<<dim3(1), dim3(RPL_SCAN_THREADS), 0, e->stream>>>(r->d, d_done);
    HIPCHK(hipGetLastError());
    k_replay_commit<<<replay_grid(r), dim3(64 * RPL_WAVES), 0, e->stream>>>(r->d, d_done, d_reason, d_outcome,
                                                                          e->d.opp == 0);
    HIPCHK(hipGetLastError());
    return 0;
}

template <int DT, bool NHWC>
static void launch_replay_sample(gc_replay* r, const ReplaySampleArgs& a, bool nt) {
    const dim3 grid((a.rows + RPL_SAMPLE_WAVES - 1) / RPL_SAMPLE_WAVES), block(64 * RPL_SAMPLE_WAVES);
    if (nt) k_replay_sample<DT, NHWC, true><<<grid, block, 0, r->e->stream>>>(r->d, a);
    else k_replay_sample<DT, NHWC, false><<<grid, block, 0, r->e->stream>>>(r->d, a);
}

extern "C" int gc_replay_sample(gc_replay* r, int rows, const int32_t* d_index, uint64_t seed, uint32_t draw,
                                void* d_planes, int dtype, int64_t row_stride, int flags, float* d_pi_dense,
                                int64_t pi_stride, int32_t* d_pi_index, float* d_pi, float* d_z, int32_t* d_slot) {
    if (!r) return fail("null store");
    if (rows < 0) return fail("negative row count");
    if (dtype < 0 || dtype > 2) return fail("dtype: 0 float32, 1 float16, 2 bfloat16");
    if (flags & ~3) return fail("flags: bit 0 = side-to-move view, bit 1 = channels-last");
    if (d_planes) {
        if (row_stride != 0 && row_stride < PLN_ELEMS) return fail("row stride below the 1536 elements of a board");
        if (row_stride % 8) return fail("row stride must be a multiple of 8 elements");
        if ((uintptr_t)d_planes % 16) return fail("the planes buffer must be 16-byte aligned");
    }
    if (d_pi_dense) {
        if (pi_stride < RPL_ROW) return fail("pi_stride below the 4100 elements of a logits row");
        if (pi_stride % 4) return fail("pi_stride must be a multiple of 4 elements");
        if ((uintptr_t)d_pi_dense % 16) return fail("the dense target buffer must be 16-byte aligned");
    }
    if (rows == 0) return 0;
    gc_env* e = r->e;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    ReplaySampleArgs a;
    a.index = d_index;
    a.seed = seed;
    a.draw = draw;
    a.rows = rows;
    a.planes = d_planes;
    a.stride = row_stride ? (size_t)row_stride : (size_t)PLN_ELEMS;
    a.persp = flags & 1;
    a.fide = e->rules != 0;
    a.pi_dense = d_pi_dense;
    a.pi_stride = (size_t)pi_stride;
    a.pi_index = d_pi_index;
    a.pi = d_pi;
    a.z = d_z;
    a.slot = d_slot;
    const char* ntv = getenv("GC_REPLAY_NT");  // A/B (read per call): non-temporal stores
    const bool nt = ntv ? atoi(ntv) != 0 : RPL_NT_DEFAULT;
    const bool nhwc = (flags & 2) != 0;
    if (dtype == 0) { if (nhwc) launch_replay_sample<0, true>(r, a, nt); else launch_replay_sample<0, false>(r, a, nt); }
    else if (dtype == 1) { if (nhwc) launch_replay_sample<1, true>(r, a, nt); else launch_replay_sample<1, false>(r, a, nt); }
    else { if (nhwc) launch_replay_sample<2, true>(r, a, nt); else launch_replay_sample<2, false>(r, a, nt); }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gc_replay_counters(gc_replay* r, uint64_t* total, uint64_t* live, uint64_t* plies, uint64_t* dropped) {
    if (!r) return fail("null store");
    gc_env* e = r->e;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    const size_t G = (size_t)r->d.games;
    std::vector<int32_t> h(2 * G);
    uint64_t t = 0;
    HIPCHK(hipMemcpyAsync(h.data(), r->d.plies, 4 * G, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(h.data() + G, r->d.dropped, 4 * G, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(&t, r->d.total, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    uint64_t ps = 0, ds = 0;
    for (size_t g = 0; g < G; g++) {
        ps += (uint64_t)h[g];
        ds += (uint64_t)h[G + g];
    }
    if (total) *total = t;
    if (live) *live = t < (uint64_t)r->d.capacity ? t : (uint64_t)r->d.capacity;
    if (plies) *plies = ps;
    if (dropped) *dropped = ds;
    return 0;
}

extern "C" int gc_replay_pointers(gc_replay* r, void** out, int n) {
    if (!r || !out) return fail("null argument");
    if (n < 1) return fail("n must be >= 1");
    const ReplayDev& d = r->d;
    void* p[GC_REPLAY_ARRAYS] = {d.pend_pos, d.pend_act, d.pend_vis, d.ring_pos, d.ring_act, d.ring_vis,
                                 d.ring_z,   d.plies,    d.dropped,  d.total,    d.off,      d.base};
    for (int k = 0; k < n && k < GC_REPLAY_ARRAYS; k++) out[k] = p[k];
    return 0;
}

extern "C" uint64_t gc_replay_device_bytes(gc_replay* r) { return r ? (uint64_t)r->bytes : 0; }
