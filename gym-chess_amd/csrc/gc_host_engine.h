// gc_host_engine.h -- gc_engine and the gc_engine_* calls.
#pragma once

struct gc_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    int cap_n = 0, cap_list = 0;
    u64* bb = nullptr; u32* meta = nullptr;       // input states
    u64* bb2 = nullptr; u32* meta2 = nullptr;     // output states
    // The host-facing buffers of one call are views into ONE device block (dio), laid out for
    // the call's n by engine_layout, mirrored by a pinned host block (hio): a call stages its
    // inputs with one host-to-device copy and returns its outputs with one copy back (a
    // single-board call is latency-bound: every copy is a round trip)
    uint8_t* dio = nullptr; uint8_t* hio = nullptr; size_t io_cap = 0;
    int8_t* mbox = nullptr; uint8_t* m8 = nullptr; uint8_t* side = nullptr;
    uint16_t* acts = nullptr; int32_t* i32a = nullptr; int32_t* i32b = nullptr;
    uint16_t* list = nullptr; uint64_t* u64o = nullptr;
    int rules = 0;  // 0 reference (lib.rs), 1 FIDE (gc_fide.h)
    // small calls (a layout within ENGINE_ZC_BYTES) stage in host-mapped coherent memory that
    // the kernels read and write directly: one launch and no copy per call, where the
    // staged form paid a copy each way (two more dispatches) around it
    uint8_t* zc = nullptr; uint8_t* zcd = nullptr; bool zc_on = false;
    // one-position calls under the reference rules go to the engine server (k_engine_server)
    SrvClient<EngBox> srv{"engine server"};
    // one call at a time per engine: ctypes releases the GIL, and a call's staging buffers
    // and the server's mailbox are the engine's own
    std::mutex mu;
};
#define ENGINE_ZC_BYTES 65536
// byte offsets of the views for n boards and a list capacity lc (256-B aligned)
struct EngineLayout {
    size_t mbox, m8, side, acts, i32a, i32b, list, end;
};
static EngineLayout engine_offsets(size_t n, size_t lc) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    EngineLayout o;
    o.mbox = 0;
    o.m8 = up(o.mbox + 64 * n);
    o.side = up(o.m8 + 8 * n);
    o.acts = up(o.side + n);
    o.i32a = up(o.acts + 2 * n);
    o.i32b = up(o.i32a + 4 * n);
    o.list = up(o.i32b + 4 * n);
    o.end = up(o.list + 2 * lc * n);
    return o;
}
static EngineLayout engine_layout(gc_engine* e, int n, int lc, uint8_t* base) {
    EngineLayout o = engine_offsets((size_t)n, (size_t)lc);
    e->mbox = reinterpret_cast<int8_t*>(base + o.mbox);
    e->m8 = base + o.m8;
    e->side = base + o.side;
    e->acts = reinterpret_cast<uint16_t*>(base + o.acts);
    e->i32a = reinterpret_cast<int32_t*>(base + o.i32a);
    e->i32b = reinterpret_cast<int32_t*>(base + o.i32b);
    e->list = reinterpret_cast<uint16_t*>(base + o.list);
    return o;
}
static bool engine_zc_enabled() {
    static const bool off = getenv("GC_ENGINE_ZC") && atoi(getenv("GC_ENGINE_ZC")) == 0;  // A/B
    return !off;
}

static void engine_free_bufs(gc_engine* e) {
    void* ps[] = {e->bb, e->meta, e->bb2, e->meta2, e->dio, e->u64o};
    for (void* p : ps) if (p) (void)hipFree(p);
    if (e->hio) (void)hipHostFree(e->hio);
    if (e->zc) (void)hipHostFree(e->zc);
    e->zc = nullptr; e->zcd = nullptr; e->zc_on = false;
    e->bb = nullptr; e->meta = nullptr; e->bb2 = nullptr; e->meta2 = nullptr; e->dio = nullptr; e->hio = nullptr;
    e->mbox = nullptr; e->m8 = nullptr; e->side = nullptr; e->acts = nullptr; e->i32a = nullptr; e->i32b = nullptr;
    e->list = nullptr; e->u64o = nullptr;
    e->cap_n = 0; e->cap_list = 0; e->io_cap = 0;
}

static int engine_reserve(gc_engine* e, int n, int listcap) {
    if (n <= e->cap_n && listcap <= e->cap_list) return 0;
    int nn = n > e->cap_n ? n : e->cap_n, lc = listcap > e->cap_list ? listcap : e->cap_list;
    engine_free_bufs(e);
    const size_t io = engine_offsets((size_t)nn, (size_t)lc).end;
    if (dalloc(&e->bb, (size_t)NBB * nn) || dalloc(&e->meta, nn) || dalloc(&e->bb2, (size_t)NBB * nn) ||
        dalloc(&e->meta2, nn) || dalloc(&e->dio, io) || dalloc(&e->u64o, nn))
        return -1;
    hipError_t he = hipHostMalloc((void**)&e->hio, io, hipHostMallocDefault);
    if (he != hipSuccess) return fail(std::string("hipHostMalloc: ") + hipGetErrorString(he));
    host_fill(e->hio, io);
    e->io_cap = io;
    e->cap_n = nn;
    e->cap_list = lc;
    return 0;
}
// one call's staging: the inputs present (side / acts may be null) into the pinned block, one
// copy to the device; the views laid out for (n, lc)
static int engine_stage(gc_engine* e, int n, int lc, const int8_t* boards, const uint8_t* meta, const uint8_t* side,
                        const uint16_t* acts, EngineLayout& o) {
    e->zc_on = engine_zc_enabled() && engine_offsets((size_t)n, (size_t)lc).end <= ENGINE_ZC_BYTES;
    if (e->zc_on && !e->zc) {
        HIPCHK(hipHostMalloc((void**)&e->zc, ENGINE_ZC_BYTES, hipHostMallocMapped | hipHostMallocCoherent));
        host_fill(e->zc, ENGINE_ZC_BYTES);
        HIPCHK(hipHostGetDevicePointer((void**)&e->zcd, e->zc, 0));
    }
    uint8_t* h = e->zc_on ? e->zc : e->hio;
    o = engine_layout(e, n, lc, e->zc_on ? e->zcd : e->dio);
    std::memcpy(h + o.mbox, boards, (size_t)64 * n);
    std::memcpy(h + o.m8, meta, (size_t)8 * n);
    size_t end = o.m8 + (size_t)8 * n;
    if (side) { std::memcpy(h + o.side, side, (size_t)n); end = o.side + n; }
    if (acts) { std::memcpy(h + o.acts, acts, (size_t)2 * n); end = o.acts + (size_t)2 * n; }
    if (!e->zc_on) HIPCHK(hipMemcpyAsync(e->dio, e->hio, end, hipMemcpyHostToDevice, e->stream));
    return 0;
}
// the byte range [a, b) of the device block back into the pinned one, then wait (a small
// call's outputs are already in host memory: only the wait, and the range into hio)
static int engine_fetch(gc_engine* e, size_t a, size_t b) {
    if (!e->zc_on) HIPCHK(hipMemcpyAsync(e->hio + a, e->dio + a, b - a, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->zc_on) std::memcpy(e->hio + a, e->zc + a, b - a);
    return 0;
}

// The batched calls' prologue: n and the states checked, the call's inputs staged (side / acts
// when given) and the views laid out for (n, lc); then, unless the caller's kernel fuses it, the
// import into e->bb / e->meta (a side given is its side to move)
static int engine_begin(gc_engine* e, int n, const int8_t* boards, const uint8_t* meta, const uint8_t* side,
                        const uint16_t* acts, int lc, bool fused_import, EngineLayout& o) {
    if (n <= 0) return fail("n must be > 0");
    if (!boards || !meta) return fail("null boards/meta");
    if (check_boards(n, boards)) return -1;
    HIPCHK(hipSetDevice(e->device));
    if (engine_stage(e, n, lc, boards, meta, side, acts, o)) return -1;
    if (fused_import) return 0;
    const uint8_t* dside = side ? e->side : nullptr;
    SoA st{e->bb, e->meta, n};
    if (e->rules) k_fimport<<<grid_for(n), BLOCK, 0, e->stream>>>(e->mbox, e->m8, dside, st);
    else k_import<<<grid_for(n), BLOCK, 0, e->stream>>>(e->mbox, e->m8, dside, st);
    HIPCHK(hipGetLastError());
    return 0;
}

static void engine_export(gc_engine* e, SoA st) {
    if (e->rules) k_fexport<<<grid_for(st.n), BLOCK, 0, e->stream>>>(st, e->mbox, e->m8);
    else k_export<<<grid_for(st.n), BLOCK, 0, e->stream>>>(st, e->mbox, e->m8);
}

// rules 0: the reference's (default); 1: FIDE (gc_fide.h; meta8[7] = en-passant file + 1)
extern "C" int gc_engine_set_rules(gc_engine* e, int rules) {
    if (!e) return fail("null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    if (rules != 0 && rules != 1) return fail("rules must be 0 (reference) or 1 (fide)");
    e->rules = rules;
    return 0;
}

extern "C" int gc_engine_create(int device, gc_engine** out) {
    if (!out) return fail("null out pointer");
    int nd = 0;
    HIPCHK(hipGetDeviceCount(&nd));
    if (device < 0 || device >= nd) return fail("device index out of range");
    gc_engine* e = new gc_engine();
    e->device = device;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    if (engine_reserve(e, 256, 256)) { delete e; return -1; }
    *out = e;
    return 0;
}

// ---- the engine server's host side (SrvClient)
static bool eng_srv_enabled() {
    static const bool off = getenv("GC_ENGINE_SERVER") && atoi(getenv("GC_ENGINE_SERVER")) == 0;  // A/B
    return !off;
}
static bool eng_srv_use(const gc_engine* e, int n) { return n == 1 && !e->rules && eng_srv_enabled(); }
static int eng_srv_stop(void* p) {
    gc_engine* e = static_cast<gc_engine*>(p);
    return e->srv.stop(e->device, e);
}
// the one-position calls' prologue and request: one op on one position through the server;
// the response lands in e->srv.box
static int eng_srv_call(gc_engine* e, int op, const int8_t* board, const uint8_t* meta, bool white, int arg) {
    if (!board || !meta) return fail("null boards/meta");
    if (check_boards(1, board)) return -1;
    return e->srv.call(
        e->device, e, eng_srv_stop,
        [&](EngBox* b) {
            memcpy(b->board, board, 64);
            memcpy(b->meta, meta, 8);
            __atomic_store_n(&b->op, (u32)op, __ATOMIC_RELAXED);
            __atomic_store_n(&b->white, white ? 1u : 0u, __ATOMIC_RELAXED);
            __atomic_store_n(&b->arg, (u32)arg, __ATOMIC_RELAXED);
            return 0;
        },
        [] { return 0; },
        [&](EngBox* box_d, u32 seq, u32 launch) { k_engine_server<<<1, 64, 0, e->srv.stream>>>(box_d, seq, launch); });
}

extern "C" int gc_engine_destroy(gc_engine* e) {
    if (!e) return 0;
    (void)hipSetDevice(e->device);
    (void)eng_srv_stop(e);
    srv_unregister(e);
    e->srv.destroy();
    (void)hipStreamSynchronize(e->stream);
    engine_free_bufs(e);
    (void)hipStreamDestroy(e->stream);
    delete e;
    return 0;
}

extern "C" int gc_engine_get_possible_moves(gc_engine* e, int n, const int8_t* boards, const uint8_t* meta,
                                            const uint8_t* player_white, int attack, uint16_t* moves, int cap,
                                            int32_t* counts) {
    if (!e || !moves || !counts || !player_white) return fail("null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (cap <= 0) return fail("cap must be > 0");
    if (eng_srv_use(e, n) && cap <= ENG_SRV_CAP) {
        if (eng_srv_call(e, ENG_LIST, boards, meta, player_white[0] != 0, attack ? 1 : 0)) return -1;
        const int c = (int)e->srv.box->count;
        memcpy(moves, e->srv.box->moves, (size_t)2 * (c < cap ? c : cap));
        counts[0] = c;
        return 0;
    }
    if (devsrv_quiesce(e->device) || engine_reserve(e, n, cap)) return -1;
    EngineLayout o;
    if (engine_begin(e, n, boards, meta, player_white, nullptr, cap, !e->rules, o)) return -1;
    if (e->rules) k_flist<<<grid_for(n), BLOCK, 0, e->stream>>>(SoA{e->bb, e->meta, n}, attack ? 1 : 0, cap, e->list, e->i32a);
    else  // one launch: import + list
        k_list_mb<<<grid_for(n), BLOCK, 0, e->stream>>>(e->mbox, e->m8, e->side, n, attack ? 1 : 0, cap, e->list, e->i32a);
    HIPCHK(hipGetLastError());
    if (engine_fetch(e, o.i32a, o.list + (size_t)2 * cap * n)) return -1;
    std::memcpy(moves, e->hio + o.list, (size_t)2 * cap * n);
    std::memcpy(counts, e->hio + o.i32a, (size_t)4 * n);
    return 0;
}

// a castle word's moves in reference order (QS then KS, lib.rs:992,1011) into out[0..2); their number
static int castle_moves(u64 c, uint16_t* out) {
    int k = 0;
    if (c & (1ull << 1)) out[k++] = A_QSW;
    if (c & (1ull << 0)) out[k++] = A_KSW;
    if (c & (1ull << 3)) out[k++] = A_QSB;
    if (c & (1ull << 2)) out[k++] = A_KSB;
    return k;
}

extern "C" int gc_engine_get_castle_moves(gc_engine* e, int n, const int8_t* boards, const uint8_t* meta,
                                          const uint8_t* player_white, uint16_t* moves, int32_t* counts) {
    if (!e || !moves || !counts || !player_white) return fail("null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (eng_srv_use(e, n)) {
        if (eng_srv_call(e, ENG_CASTLE, boards, meta, player_white[0] != 0, 0)) return -1;
        counts[0] = castle_moves(e->srv.box->count, moves);
        return 0;
    }
    if (devsrv_quiesce(e->device) || engine_reserve(e, n, 2)) return -1;
    EngineLayout o;
    if (engine_begin(e, n, boards, meta, player_white, nullptr, 2, false, o)) return -1;
    std::vector<u64> mask(e->rules ? (size_t)65 * n : 0);
    if (e->rules) {
        Temps tmp;
        u64* dmask = nullptr;
        if (tmp.alloc(&dmask, (size_t)65 * n)) return -1;
        k_fmask<<<grid_for(n), BLOCK, 0, e->stream>>>(SoA{e->bb, e->meta, n}, dmask, nullptr);
        hipError_t le = hipGetLastError();
        hipError_t ce = hipMemcpyAsync(mask.data(), dmask, (size_t)8 * 65 * n, hipMemcpyDeviceToHost, e->stream);
        hipError_t se = hipStreamSynchronize(e->stream);
        if (le != hipSuccess || ce != hipSuccess || se != hipSuccess) return fail("castle mask kernel failed");
    } else {  // the castle word per board into the layout's int32 row
        k_castle_word<<<grid_for(n), BLOCK, 0, e->stream>>>(SoA{e->bb, e->meta, n}, e->i32a);
        HIPCHK(hipGetLastError());
        if (engine_fetch(e, o.i32a, o.i32a + (size_t)4 * n)) return -1;
    }
    for (int i = 0; i < n; i++) {
        const u64 c = e->rules ? mask[(size_t)65 * i + 64] : (u64)reinterpret_cast<const int32_t*>(e->hio + o.i32a)[i];
        counts[i] = castle_moves(c, moves + 2 * (size_t)i);
    }
    return 0;
}

extern "C" int gc_engine_next_state(gc_engine* e, int n, const int8_t* boards, const uint8_t* meta,
                                    const uint8_t* player_white, const uint16_t* actions, int8_t* out_boards,
                                    uint8_t* out_meta, int32_t* rewards, int32_t* status) {
    if (!e || !player_white || !actions || !out_boards || !out_meta || !rewards || !status) return fail("null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    for (int i = 0; i < n; i++)
        if (actions[i] > A_QSB) return fail("action out of range at index " + std::to_string(i));
    if (eng_srv_use(e, n)) {
        if (eng_srv_call(e, ENG_NEXT, boards, meta, player_white[0] != 0, actions[0])) return -1;
        memcpy(out_boards, e->srv.box->out_board, 64);
        memcpy(out_meta, e->srv.box->out_meta, 8);
        rewards[0] = e->srv.box->reward;
        status[0] = e->srv.box->status;
        return 0;
    }
    if (devsrv_quiesce(e->device) || engine_reserve(e, n, 1)) return -1;
    // FIDE: the player argument is the side to move; reference: it only steers next_state's
    // promotion colour and rights logic (lib.rs:679-784), the state keeps current_player
    EngineLayout o;
    if (engine_begin(e, n, boards, meta, player_white, actions, 1, !e->rules, o)) return -1;
    if (e->rules) {
        SoA in{e->bb, e->meta, n}, out{e->bb2, e->meta2, n};
        k_fnext_state<<<grid_for(n), BLOCK, 0, e->stream>>>(in, e->acts, out, e->i32a, e->i32b);
        HIPCHK(hipGetLastError());
        engine_export(e, out);
    } else {  // one launch: import + next_state + export, in place on the staged mailbox
        k_next_state_mb<<<grid_for(n), BLOCK, 0, e->stream>>>(e->mbox, e->m8, e->side, e->acts, n, e->i32a, e->i32b);
    }
    HIPCHK(hipGetLastError());
    if (engine_fetch(e, 0, o.i32b + (size_t)4 * n)) return -1;
    std::memcpy(out_boards, e->hio + o.mbox, (size_t)64 * n);
    std::memcpy(out_meta, e->hio + o.m8, (size_t)8 * n);
    std::memcpy(rewards, e->hio + o.i32a, (size_t)4 * n);
    std::memcpy(status, e->hio + o.i32b, (size_t)4 * n);
    return 0;
}

extern "C" int gc_engine_update_state(gc_engine* e, int n, const int8_t* boards, const uint8_t* meta,
                                      int8_t* out_boards, uint8_t* out_meta) {
    if (!e || !out_boards || !out_meta) return fail("null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (eng_srv_use(e, n)) {
        if (eng_srv_call(e, ENG_UPDATE, boards, meta, false, 0)) return -1;
        memcpy(out_boards, e->srv.box->out_board, 64);
        memcpy(out_meta, e->srv.box->out_meta, 8);
        return 0;
    }
    if (devsrv_quiesce(e->device) || engine_reserve(e, n, 1)) return -1;
    EngineLayout o;
    if (engine_begin(e, n, boards, meta, nullptr, nullptr, 1, false, o)) return -1;
    SoA st{e->bb, e->meta, n};
    if (e->rules) k_fupdate_state<<<grid_for(n), BLOCK, 0, e->stream>>>(st);
    else k_update_state<<<grid_for(n), BLOCK, 0, e->stream>>>(st);
    HIPCHK(hipGetLastError());
    engine_export(e, st);
    HIPCHK(hipGetLastError());
    if (engine_fetch(e, 0, o.m8 + (size_t)8 * n)) return -1;
    std::memcpy(out_boards, e->hio + o.mbox, (size_t)64 * n);
    std::memcpy(out_meta, e->hio + o.m8, (size_t)8 * n);
    return 0;
}
