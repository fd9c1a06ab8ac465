// gc_host_playout.h -- gc_playout_*: the playout handle, its one device allocation (the lanes'
// private 3-fold windows, gc_playout.h) and the launch of k_playout, asynchronous on the env's
// stream.
#pragma once

struct gc_playout {
    gc_env* e = nullptr;
    int device = 0;
    int max_rows = 0, logp = 0, max_plies = 0;
    size_t lanes = 0;  // max_rows * P rounded up to whole waves
    u64* scratch = nullptr;
    size_t bytes = 0;
};

// the envs a playout runs on: reference rules, opponent "none"
static int playout_env_ok(const gc_env* e) {
    if (e->rules != 0) return fail("playouts: reference rules only (not a rules=\"fide\" env)");
    if (e->d.opp != 0) return fail("playouts: opponent \"none\" only (this env's opponent replies inside the step)");
    return 0;
}

extern "C" int gc_playout_create(gc_env* e, int max_rows, int playouts, int max_plies, gc_playout** out) {
    if (!e || !out) return fail("null argument");
    if (playout_env_ok(e)) return -1;
    if (max_rows < 1) return fail("max_rows must be >= 1");
    if (playouts < 1 || playouts > PLAYOUT_MAX_P || (playouts & (playouts - 1)))
        return fail("playouts must be one of 1, 2, 4, 8, 16, 32, 64");
    if (max_plies < 1 || max_plies > PLAYOUT_MAX_PLIES) return fail("max_plies must be in [1, 128]");
    if ((int64_t)max_rows * playouts > (int64_t)1 << 30) return fail("max_rows * playouts must be at most 2^30");
    HIPCHK(hipSetDevice(e->device));
    gc_playout* p = new gc_playout();
    p->lanes = ((size_t)max_rows * (size_t)playouts + 63) & ~(size_t)63;
    p->bytes = playout_scratch_bytes(p->lanes);
    if (dalloc(&p->scratch, p->bytes / 8)) {
        delete p;
        return -1;
    }
    const hipError_t rc = hipMemsetAsync(p->scratch, 0, p->bytes, e->stream);  // generation 0: every entry dead
    if (rc != hipSuccess) {
        (void)hipFree(p->scratch);
        delete p;
        return fail(std::string("hipMemsetAsync: ") + hipGetErrorString(rc));
    }
    p->e = e;
    p->device = e->device;
    p->max_rows = max_rows;
    p->max_plies = max_plies;
    while ((1 << p->logp) < playouts) p->logp++;
    *out = p;
    return 0;
}

extern "C" int gc_playout_destroy(gc_playout* p) {
    if (!p) return fail("null playout handle");
    (void)hipSetDevice(p->device);  // (not through e: the env may be gone already)
    if (p->scratch) (void)hipFree(p->scratch);  // (waits for the device: no launch still uses the windows)
    delete p;
    return 0;
}

extern "C" int gc_playout_run(gc_playout* p, const int32_t* d_board_idx, int rows, int n_plies, uint64_t seed,
                              uint32_t draw, float cut_weight, float* d_value, int32_t* d_tally) {
    if (!p) return fail("null playout handle");
    gc_env* e = p->e;
    if (playout_env_ok(e)) return -1;  // (gc_env_set_rules / gc_env_set_opponent since the handle was made)
    if (rows < 0 || rows > p->max_rows) return fail("rows must be in [0, the handle's max_rows]");
    if (n_plies < 1 || n_plies > p->max_plies) return fail("n_plies must be in [1, the handle's max_plies]");
    if (!(cut_weight >= 0.0f && cut_weight <= 1.0f)) return fail("cut_weight must be in [0, 1]");
    if (rows == 0) return 0;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    PlayArgs a;
    a.idx = d_board_idx;
    a.rows = rows;
    a.logp = p->logp;
    a.n_plies = n_plies;
    a.seed = seed;
    a.draw = draw;
    a.cut_weight = cut_weight;
    a.value = d_value;
    a.tally = d_tally;
    a.tab = p->scratch;
    a.gen = reinterpret_cast<u32*>(p->scratch + playout_tab_words(p->lanes));
    const size_t lanes = (size_t)rows << p->logp;
    k_playout<<<dim3((unsigned)((lanes + PLAYOUT_BLOCK - 1) / PLAYOUT_BLOCK)), dim3(PLAYOUT_BLOCK), 0, e->stream>>>(e->d.st, a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" uint64_t gc_playout_device_bytes(gc_playout* p) { return p ? (uint64_t)p->bytes : 0; }
