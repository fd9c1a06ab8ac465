// gc_host_env.h -- the gc_env_* calls: create / destroy, step / rollout, legal moves, sync.
#pragma once

// ---- the single-board server's host side (SrvClient)
static bool srv_enabled() {
    static const bool off = getenv("GC_SINGLE_SERVER") && atoi(getenv("GC_SINGLE_SERVER")) == 0;
    return !off;
}
// stop the server (if one runs) and wait until it has drained: every other op on this env
// reads or writes the board's memory through other kernels
static int srv_stop(void* p) {
    gc_env* e = static_cast<gc_env*>(p);
    return e->srv.stop(e->device, e);
}
// one op through the server; the record lands in e->srec.  A server holds one board: a request
// for another stops it first.  It is (re)started after the env's own work.
static int srv_call(gc_env* e, int board, int op, int action, int flags) {
    return e->srv.call(
        e->device, e, srv_stop,
        [&](SrvBox* b) {
            if (e->srv.launch && e->srv_board != board && (srv_stop(e) || devsrv_claim(devsrv(e->device), e, srv_stop)))
                return -1;
            __atomic_store_n(&b->op, (u32)op, __ATOMIC_RELAXED);
            __atomic_store_n(&b->action, action, __ATOMIC_RELAXED);
            __atomic_store_n(&b->flags, (u32)flags, __ATOMIC_RELAXED);
            return 0;
        },
        [&]() -> int {
            HIPCHK(hipStreamSynchronize(e->stream));
            e->srv_board = board;
            return 0;
        },
        [&](SrvBox* box_d, u32 seq, u32 launch) {
            k_single_server<<<1, 64, 0, e->srv.stream>>>(e->d, board, box_d, e->srec_d, seq, launch);
        });
}

// The repetition tables for move-capped games (HTAB_BITS) or for a BLACK agent's uncapped
// ones (HTAB_BITS_UNCAPPED + the spill table); the stream is idle, the windows are cleared.
static int set_window_kind(gc_env* e, bool uncapped) {
    const int bits = uncapped ? HTAB_BITS_UNCAPPED : HTAB_BITS;
    if (bits != e->d.hbits) {
        size_t nb64 = ((size_t)e->n + 63) / 64 * 64;
        u64* t = nullptr;
        if (dalloc(&t, ((size_t)8 << bits) * nb64)) return -1;
        HIPCHK(hipMemsetAsync(t, 0, ((size_t)64 << bits) * nb64, e->stream));
        (void)hipFree(e->d.htab);
        e->d.htab = t;
        e->d.hbits = bits;
    }
    if (uncapped && !e->d.ic.spill.ent) {  // a BLACK agent's windows may outgrow the table
        if (spill_alloc(e, spill_bits_for(e->n))) return -1;
    } else if (!uncapped && e->d.ic.spill.ent) {
        HIPCHK(hipStreamSynchronize(e->stream));
        spill_drop(e);
        if (spill_publish(e)) return -1;
    }
    return 0;
}

// kernel dispatch on the env's opponent mode (a kernel-argument-uniform choice made once per
// launch on the host, so the opponent="none" kernels carry no opponent code)
static void launch_reset(gc_env* e, const uint8_t* mask, int select) {
    if (e->rules && e->d.opp) k_fenv_reset<true><<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d, mask, select);
    else if (e->rules) k_fenv_reset<false><<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d, mask, select);
    else if (e->d.opp) k_env_reset<true><<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d, mask, select);
    else k_env_reset<false><<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d, mask, select);
}
template <bool POLICY>
static void launch_step(gc_env* e) {
    if (e->rules && e->d.opp) k_fenv_step<POLICY, true><<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d);
    else if (e->rules) k_fenv_step<POLICY, false><<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d);
    else if (e->d.opp) k_env_step<POLICY, true><<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d);
    else k_env_step<POLICY, false><<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d);
}

// the reset position's cache of the env's rules (reference or FIDE) for the paired kernels
struct ResetInfo {
    const EnvDev::InitCache* icd;
    const uint16_t* racts;
    u32 rinfo;  // table << 16 | total
};
static ResetInfo reset_info(const gc_env* e) {
    const EnvDev::InitCache& ic = e->rules ? e->ic_f : e->d.ic;
    return ResetInfo{e->rules ? e->icd_f : e->icd, e->rules ? e->racts_f : e->d.reset_acts,
                     (ic.table ? 1u << 16 : 0u) | (u32)(ic.total & 0xFFFF)};
}

// The paired kernels serve opponent "none" (both rules) and the random opponent when the
// start position's picks come from its table and, for a BLACK agent, no opening can end in
// both kings checked (pair_step_vs); otherwise the one-wave kernels run.
// the reset picks of the self-play policy (reference rules): the move-set order table
static const uint16_t* sw_table(const ResetInfo& r) {
    return r.racts ? r.racts + RESET_ACTS_MAX : r.racts;
}
static bool pair_ok(const gc_env* e) {
    if (!e->d.opp) return true;
    if (e->rules) return false;  // FIDE with the random opponent: the one-wave kernels (k_fenv_*)
    const EnvDev::InitCache& ic = e->d.ic;
    return ic.usable && ic.table && (!e->d.agent_black || ic.open_safe);
}
static int pair_opp(const gc_env* e) { return e->d.opp ? (e->d.agent_black ? 2 : 1) : 0; }

// launch geometry of the paired (two waves per 64 boards) and quad (four) kernels over nb board
// blocks (64 boards each)
static_assert(PAIR_BOARDS == QUAD_BOARDS, "one board block size");
struct LaunchGeom {
    dim3 grid, block;
};
static int board_blocks(const gc_env* e) { return (e->n + PAIR_BOARDS - 1) / PAIR_BOARDS; }
static LaunchGeom pair_geom(int nb) { return {dim3((nb + PAIRS_WG - 1) / PAIRS_WG), dim3(2 * PAIR_BOARDS * PAIRS_WG)}; }
static LaunchGeom quad_geom(int nb) { return {dim3((nb + QUADS_WG - 1) / QUADS_WG), dim3(4 * QUAD_BOARDS * QUADS_WG)}; }
// the quad rollout's own (k_env_rollout4<OCC, qw>: qw quads per workgroup, roll_quads_wg)
static LaunchGeom roll_geom(int nb, int qw) { return {dim3((nb + qw - 1) / qw), dim3(4 * QUAD_BOARDS * qw)}; }

// the paired kernels' <FIDE, OPP> variant for the env's rules and opponent, and the reset picks'
// table it reads
template <class K>
static K pair_variant(const gc_env* e, K fide, K none, K vs_white, K vs_black) {
    if (e->rules) return fide;
    const int opp = pair_opp(e);
    return opp == 0 ? none : opp == 1 ? vs_white : vs_black;
}
static const uint16_t* pair_racts(const gc_env* e, const ResetInfo& r) { return e->rules ? r.racts : sw_table(r); }

// one ply (opponent: one two-ply step) of the paired step kernel over the board blocks
// [b0, b0 + nb) (64 boards each)
static void launch_step2(gc_env* e, hipStream_t st, int b0 = 0, int nb = -1) {
    const EnvDev& d = e->d;
    const ResetInfo r = reset_info(e);
    const LaunchGeom g = pair_geom(nb < 0 ? board_blocks(e) : nb);
    const auto kernel = pair_variant(e, k_env_step2<true>, k_env_step2<false>, k_env_step2<false, 1>, k_env_step2<false, 2>);
    kernel<<<g.grid, g.block, 0, st>>>(e->slab, d.n, b0, d.seed, d.htab, pair_racts(e, r), r.icd, r.rinfo);
}

extern "C" int gc_env_create(int device, int n_boards, uint64_t seed, const int8_t* initial_board, gc_env** out) {
    if (!out) return fail("null out pointer");
    if (n_boards <= 0) return fail("n_boards must be > 0");
    int nd = 0;
    HIPCHK(hipGetDeviceCount(&nd));
    if (device < 0 || device >= nd) return fail("device index out of range");
    static const int8_t DEF[64] = {-3, -5, -4, -2, -1, -4, -5, -3, -6, -6, -6, -6, -6, -6, -6, -6,
                                   0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,
                                   0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,
                                   6,  6,  6,  6,  6,  6,  6,  6,  3,  5,  4,  2,  1,  4,  5,  3};
    const int8_t* ib = initial_board ? initial_board : DEF;
    if (check_boards(1, ib)) return -1;
    gc_env* e = new gc_env();
    e->device = device;
    e->n = n_boards;
    e->seed = seed;
    int n = n_boards;
    size_t nb64 = ((size_t)n + 63) / 64 * 64;  // the window tables come in blocks of 64 boards
    hipError_t he = hipSetDevice(device);
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he != hipSuccess) { env_free(e); delete e; return fail(std::string("stream: ") + hipGetErrorString(he)); }
    if (dalloc(&e->slab, Slab::BYTES_PER_BOARD * (size_t)n) ||
        dalloc(&e->d.htab, (size_t)HTAB * 8 * nb64) || dalloc(&e->mbox, (size_t)64 * n) ||
        dalloc(&e->m8, (size_t)8 * n) || dalloc(&e->mask, n) || dalloc(&e->counts, n) || dalloc(&e->stats, (size_t)8 * n + 8) /* [n][8] + the 8 sums */) {
        std::string m = g_err;
        env_free(e); delete e;
        return fail(m);
    }
    {
        uint8_t* sl = e->slab;
        size_t nz = (size_t)n;
        e->bb = reinterpret_cast<u64*>(sl);
        e->meta = reinterpret_cast<u32*>(sl + Slab::meta(nz));
        e->d.hgen = reinterpret_cast<u32*>(sl + Slab::hgen(nz));
        e->d.draw = reinterpret_cast<u32*>(sl + Slab::draw(nz));
        e->d.nsteps = reinterpret_cast<u32*>(sl + Slab::nsteps(nz));
        e->d.reward = reinterpret_cast<int32_t*>(sl + Slab::reward(nz));
        e->d.act = reinterpret_cast<uint16_t*>(sl + Slab::act(nz));
        e->d.done = sl + Slab::done(nz);
        e->d.reason = sl + Slab::reason(nz);
    }
    // initial board bitboards (pure data conversion of the caller's input; no engine work)
    Pos ip = from_mailbox(ib, 0);
    u64 ibb[NBB] = {ip.k, ip.q, ip.r, ip.b, ip.n, ip.p, ip.w};
    for (int j = 0; j < NBB; j++) e->d.init[j] = ibb[j];
    he = hipSuccess;
    if (he == hipSuccess) he = hipMemsetAsync(e->d.draw, 0, (size_t)4 * n, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(e->d.htab, 0, (size_t)64 * HTAB * nb64, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(e->d.hgen, 0, (size_t)4 * n, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(e->d.nsteps, 0, (size_t)4 * n, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(e->d.reward, 0, (size_t)4 * n, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(e->d.done, 0, (size_t)n, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(e->d.reason, 0, (size_t)n, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(e->stats, 0, (size_t)64 * n, e->stream);
    for (auto& v : e->ev) if (he == hipSuccess) he = hipEventCreate(&v);
    if (he != hipSuccess) { env_free(e); delete e; return fail(std::string("env init: ") + hipGetErrorString(he)); }
    e->d.st = SoA{e->bb, e->meta, n};
    e->d.seed = seed;
    e->d.n = n;
    e->d.opp = 0;
    e->d.agent_black = 0;
    e->d.hbits = HTAB_BITS;
    {  // the start position's move set, shared by every reset (EnvDev::ic)
        EnvDev::InitCache* dic = nullptr;
        uint16_t* dacts = nullptr;
        if (dalloc(&dic, 1) || dalloc(&dacts, 2 * RESET_ACTS_MAX)) {
            std::string m = g_err; (void)hipFree(dic); env_free(e); delete e; return fail(m);
        }
        e->reset_acts = dacts;
        e->d.reset_acts = dacts;
        e->icd = dic;
        k_init_cache<<<1, BLOCK, 0, e->stream>>>(e->d, dic, dacts);
        he = hipGetLastError();
        if (he == hipSuccess) he = hipMemcpyAsync(&e->d.ic, dic, sizeof(EnvDev::InitCache), hipMemcpyDeviceToHost, e->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
        if (he != hipSuccess) { env_free(e); delete e; return fail(std::string("init cache: ") + hipGetErrorString(he)); }
        // the completion word of the quad rollout (host-mapped, fine-grained)
        u32* hw = nullptr;
        he = hipHostMalloc(&hw, 4, hipHostMallocMapped | hipHostMallocCoherent);
        if (he == hipSuccess) { e->done_host = hw; host_fill(hw, 4); *hw = 0; }
        if (he == hipSuccess && dalloc(&e->done_dev, 2)) {
            std::string m = g_err; env_free(e); delete e; return fail(m);
        }
        if (he == hipSuccess) he = hipMemsetAsync(e->done_dev, 0, 8, e->stream);
        u32* hwd = nullptr;
        if (he == hipSuccess) he = hipHostGetDevicePointer((void**)&hwd, hw, 0);
        if (he == hipSuccess) {
            e->d.ic.done = EnvDev::InitCache::DoneWord{e->done_dev, e->done_dev + 1, hwd};
            he = hipMemcpyAsync(&dic->done, &e->d.ic.done, sizeof(e->d.ic.done), hipMemcpyHostToDevice, e->stream);
        }
        if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
        if (he != hipSuccess) { env_free(e); delete e; return fail(std::string("completion word: ") + hipGetErrorString(he)); }
    }
    launch_reset(e, nullptr, 1);
    he = hipGetLastError();
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess) { env_free(e); delete e; return fail(std::string("reset: ") + hipGetErrorString(he)); }
    e->policy_ready = true;
    {
        const char* sv = getenv("GC_STREAMS");
        int k = sv ? atoi(sv) : GC_DEFAULT_STREAMS;
        if (k > 1 && gc_env_set_streams(e, k)) { std::string m = g_err; env_free(e); delete e; return fail(m); }
    }
    *out = e;
    return 0;
}

// opponent mode (chess_v2.py:133-181): opponent 0 "none", 1 "random" (the device policy
// answers inside every step); agent_white 0 = player_color BLACK (requires an opponent: the
// reference's reset calls the opponent policy to open).  Resets every board.
extern "C" int gc_env_set_opponent(gc_env* e, int opponent, int agent_white) {
    if (!e) return fail("null env");
    SRV_QUIESCE(e);
    if (opponent != 0 && opponent != 1) return fail("opponent must be 0 (none) or 1 (random)");
    if (!agent_white && !opponent) return fail("player_color BLACK needs an opponent (chess_v2.py:208-212)");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (set_window_kind(e, !agent_white)) return -1;
    e->d.opp = opponent;
    e->d.agent_black = agent_white ? 0 : 1;
    if (!agent_white && e->d.ic.table && !e->open_cache) {  // the openings of a BLACK agent's resets
        if (dalloc(&e->open_cache, RESET_ACTS_MAX) || dalloc(&e->open_acts, (size_t)RESET_ACTS_MAX * RESET_ACTS_MAX))
            return -1;
        k_init_open_cache<<<(RESET_ACTS_MAX + BLOCK - 1) / BLOCK, BLOCK, 0, e->stream>>>(
            e->d, e->icd, e->reset_acts + RESET_ACTS_MAX, e->open_cache, e->open_acts);
        HIPCHK(hipGetLastError());
        e->d.ic.open = e->open_cache;
        e->d.ic.open_acts = e->open_acts;
        HIPCHK(hipMemcpyAsync(&e->icd->open, &e->d.ic.open, sizeof(e->d.ic.open) + sizeof(e->d.ic.open_acts),
                              hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    HIPCHK(hipMemsetAsync(e->d.draw, 0, (size_t)4 * e->n, e->stream));  // fresh policy streams
    launch_reset(e, nullptr, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    e->policy_ready = true;
    return 0;
}

// rules 0: the reference's (default); 1: FIDE (gc_fide.h; with the random opponent on the
// one-wave kernels).  Resets every board and restarts the policy streams.
extern "C" int gc_env_set_rules(gc_env* e, int rules) {
    if (!e) return fail("null env");
    SRV_QUIESCE(e);
    if (rules != 0 && rules != 1) return fail("rules must be 0 (reference) or 1 (fide)");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (rules && !e->icd_f) {  // the FIDE reset position's move set (paired kernels)
        if (dalloc(&e->icd_f, 1) || dalloc(&e->racts_f, RESET_ACTS_MAX)) return -1;
        k_finit_cache<<<1, BLOCK, 0, e->stream>>>(e->d, e->icd_f, e->racts_f);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&e->ic_f, e->icd_f, sizeof(EnvDev::InitCache), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    e->rules = rules;
    HIPCHK(hipMemsetAsync(e->d.draw, 0, (size_t)4 * e->n, e->stream));
    launch_reset(e, nullptr, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    e->policy_ready = true;
    return 0;
}

extern "C" int gc_env_destroy(gc_env* e) {
    if (!e) return 0;
    (void)hipSetDevice(e->device);
    (void)srv_stop(e);
    srv_unregister(e);
    (void)hipStreamSynchronize(e->stream);
    env_free(e);
    delete e;
    return 0;
}

extern "C" int gc_env_num_boards(gc_env* e) { return e ? e->n : -1; }

extern "C" int gc_env_reset(gc_env* e, const uint8_t* mask) {
    if (!e) return fail("null env");
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    if (mask) HIPCHK(hipMemcpyAsync(e->mask, mask, e->n, hipMemcpyHostToDevice, e->stream));
    launch_reset(e, mask ? e->mask : nullptr, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    if (!mask && spill_windows_cleared(e)) return -1;
    e->policy_ready = true;
    return 0;
}

// ---- single-board env ops (k_single)
extern "C" int gc_env_single_setup(gc_env* e, int agent_white) {
    if (!e) return fail("null env");
    SRV_QUIESCE(e);
    if (e->rules) return fail("the single-board env ops follow the reference's rules");
    if (e->d.opp) return fail("the single-board env ops drive the opponent from the host (opponent 0)");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (set_window_kind(e, !agent_white)) return -1;
    if (!e->srec) {
        HIPCHK(hipHostMalloc(&e->srec, sizeof(gc_single_record), hipHostMallocMapped));
        host_fill(e->srec, sizeof(gc_single_record));
        HIPCHK(hipHostGetDevicePointer((void**)&e->srec_d, e->srec, 0));
    }
    return 0;
}

// diagnostic: the server's segments of its last op (10 ns ticks): op, list, record copy, idle
extern "C" int gc_env_single_stamps(gc_env* e, uint32_t* out6) {
    if (!e || !out6) return fail("null argument");
    for (int k = 0; k < 6; k++) out6[k] = e->srv.box ? __atomic_load_n(&e->srv.box->stamps[k], __ATOMIC_ACQUIRE) : 0u;
    return 0;
}

extern "C" int gc_env_single_call(gc_env* e, int board, int op, int action, int flags, const gc_single_record** rec) {
    if (!e || !rec) return fail("null argument");
    if (!e->srec) return fail("call gc_env_single_setup first");
    if (board < 0 || board >= e->n) return fail("board index out of range");
    if (op < SOP_RESET || op > SOP_SYNC) return fail("op: 0 reset, 1 agent, 2 reply, 3 open, 4 sync (5 set: gc_env_single_set)");
    if (op != SOP_RESET && op != SOP_SYNC && (action < 0 || action > A_RESIGN))
        return fail("action out of range [0, 4100]");
    HIPCHK(hipSetDevice(e->device));
    if (e->d.ic.spill.ent) {  // a BLACK agent: the spill table's host checks need the stream
        if (devsrv_quiesce(e->device) || spill_before(e)) return -1;
    }
    if (srv_enabled() && !e->d.ic.spill.ent) {
        if (srv_call(e, board, op, action, flags)) return -1;
    } else {
        if (devsrv_quiesce(e->device)) return -1;
        k_single<<<1, 64, 0, e->stream>>>(e->d, board, op, action, flags, e->srec_d);
        HIPCHK(hipGetLastError());
        if (spill_after(e) || gc_env_synchronize(e)) return -1;
    }
    e->policy_ready = false;
    *rec = e->srec;
    return 0;
}

// the state setter (chess_v2.py:315-323) of one board: its pieces and the six flags; the side
// to move, move_count, done and the 3-fold window stay (k_single's SET)
extern "C" int gc_env_single_set(gc_env* e, int board, const int8_t* board64, const uint8_t* flags6,
                                 const gc_single_record** rec) {
    if (!e || !board64 || !flags6 || !rec) return fail("null argument");
    if (!e->srec) return fail("call gc_env_single_setup first");
    if (board < 0 || board >= e->n) return fail("board index out of range");
    for (int k = 0; k < 64; k++)
        if (board64[k] < -6 || board64[k] > 6) return fail("board: piece ids are -6..6");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));  // the record is the launch's input here
    memcpy(e->srec->board, board64, 64);
    for (int k = 0; k < 4; k++) e->srec->rights[k] = flags6[k] ? 1 : 0;
    for (int k = 0; k < 2; k++) e->srec->checked[k] = flags6[4 + k] ? 1 : 0;
    if (srv_enabled() && !e->d.ic.spill.ent) {
        if (srv_call(e, board, SOP_SET, 0, 0)) return -1;
    } else {
        if (devsrv_quiesce(e->device)) return -1;
        k_single<<<1, 64, 0, e->stream>>>(e->d, board, SOP_SET, 0, 0, e->srec_d);
        HIPCHK(hipGetLastError());
        if (gc_env_synchronize(e)) return -1;
    }
    e->policy_ready = false;
    *rec = e->srec;
    return 0;
}

extern "C" int gc_env_window_boards(gc_env* e, int board, int8_t* boards, uint8_t* counts, int cap, int* n) {
    if (!e || !n || (cap > 0 && (!boards || !counts))) return fail("null argument");
    SRV_QUIESCE(e);
    if (board < 0 || board >= e->n) return fail("board index out of range");
    HIPCHK(hipSetDevice(e->device));
    Temps tmps;
    int8_t* db = nullptr;
    uint8_t* dc = nullptr;
    int* dn = nullptr;
    const int c = cap > 0 ? cap : 0;
    if (tmps.alloc(&db, (size_t)64 * (c ? c : 1)) || tmps.alloc(&dc, c ? c : 1) || tmps.alloc(&dn, 1)) return -1;
    k_window_boards<<<1, 64, 0, e->stream>>>(e->d, board, db, dc, c, dn);
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(n, dn, sizeof(int), hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    const int k = *n < c ? *n : c;
    if (he == hipSuccess && k) he = hipMemcpy(boards, db, (size_t)64 * k, hipMemcpyDeviceToHost);
    if (he == hipSuccess && k) he = hipMemcpy(counts, dc, (size_t)k, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return fail(std::string("window readout: ") + hipGetErrorString(he));
    return 0;
}

extern "C" int gc_env_step(gc_env* e, const uint16_t* actions, int32_t* reward, uint8_t* done, uint8_t* reason) {
    if (!e || !actions) return fail("null argument");
    SRV_QUIESCE(e);
    for (int i = 0; i < e->n; i++)
        if (actions[i] > A_RESIGN) return fail("action out of range [0, 4100] at index " + std::to_string(i));
    HIPCHK(hipSetDevice(e->device));
    if (spill_before(e)) return -1;
    HIPCHK(hipMemcpyAsync(e->d.act, actions, (size_t)2 * e->n, hipMemcpyHostToDevice, e->stream));
    launch_step<false>(e);
    HIPCHK(hipGetLastError());
    if (spill_after(e)) return -1;
    e->policy_ready = false;
    if (reward) HIPCHK(hipMemcpyAsync(reward, e->d.reward, (size_t)4 * e->n, hipMemcpyDeviceToHost, e->stream));
    if (done) HIPCHK(hipMemcpyAsync(done, e->d.done, e->n, hipMemcpyDeviceToHost, e->stream));
    if (reason) HIPCHK(hipMemcpyAsync(reason, e->d.reason, e->n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// the paired / quad API step's output pointers: the device copy follows the caller's buffers
static int api_publish(gc_env* e, const ApiOut& o) {
    if (!e->api_out) {
        if (dalloc(&e->api_out, 1)) return -1;
        e->api_host = {};
    }
    if (memcmp(&o, &e->api_host, sizeof o) != 0) {  // the caller's buffers changed
        e->api_host = o;
        HIPCHK(hipMemcpyAsync(e->api_out, &e->api_host, sizeof o, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));  // api_host may change again before a lazy copy ran
    }
    return 0;
}

// step() with device buffers (k_env_step_api4 and its siblings): asynchronous on the env's
// stream (gc_env_get_stream); every pointer is device memory of n entries (mask: 65 rows of
// mask_stride words, word f of board i at f * mask_stride + i; obs: n*64 bytes); mask / obs /
// count / pick may be NULL.  The stride travels with each call: with n a multiple
// of a large power of two, packed rows n words apart alias on the same HBM channels, so a caller
// may pad them (gym_chess_amd.env.DeviceIO does); gc_env_step_device is the packed form.
extern "C" int gc_env_step_device2(gc_env* e, const uint16_t* d_actions, int32_t* d_reward, uint8_t* d_done,
                                   uint8_t* d_reason, uint64_t* d_mask, int8_t* d_obs, int32_t* d_count,
                                   uint16_t* d_pick, int flags, int64_t mask_stride) {
    if (!e || !d_actions || !d_reward || !d_done || !d_reason) return fail("null argument");
    SRV_QUIESCE(e);
    if (flags & ~1) return fail("flags: bit 0 = auto-reset");
    if (mask_stride != 0 && mask_stride < (int64_t)e->n) return fail("mask stride below the board count");
    HIPCHK(hipSetDevice(e->device));
    if (spill_before(e)) return -1;
    const int ar = flags & 1;
    const size_t ms = mask_stride ? (size_t)mask_stride : (size_t)e->n;  // the mask rows' stride
    const EnvDev& d = e->d;
    const ResetInfo r = reset_info(e);
    const ApiOut o = {d_reward, d_done, d_reason, d_mask, d_obs, d_count, d_pick, ms};
    const LaunchGeom quad = quad_geom(board_blocks(e)), pair = pair_geom(board_blocks(e));
    auto lanes = [&](auto kernel) {  // one lane per board
        kernel<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d, d_actions, d_reward, d_done, d_reason, d_mask, d_obs, d_count,
                                                        d_pick, ar, ms);
    };
    auto waves = [&](auto kernel, const LaunchGeom& g) {  // two or four waves per 64 boards
        kernel<<<g.grid, g.block, 0, e->stream>>>(e->slab, d.seed, d.htab, r.racts, r.icd, d_actions, e->api_out, d.n,
                                                  r.rinfo | ((u32)ar << 17));
    };
    if (e->rules) {  // FIDE
        if (d.opp) lanes(k_fenv_step_api<true>);
        else lanes(k_fenv_step_api<false>);
    } else if (!d.opp && d.ic.usable && d.ic.table) {
        // (over two board-range streams, so a range's store tail could overlap the other's
        // generation: measured 47 vs 21 us per step with the paired kernel, round 3)
        if (api_publish(e, o)) return -1;
        waves(k_env_step_api4, quad);
    } else if (d.opp && pair_ok(e)) {  // the random opponent on the paired driver
        if (api_publish(e, o)) return -1;
        const char* nq = getenv("GC_NO_QUAD_API");  // A/B and tests (read per call): api2_vs
        const bool no_quad_vs = nq && atoi(nq) != 0;
        // (a BLACK agent's resets open with the opponent's move: the openings' positions and moves
        // are cached, k_init_open_cache -- 33.9 vs 41.1 us per launch for the paired kernel,
        // tools/api_color_probe.py; through the per-piece fallback instead: 46.9)
        if (!no_quad_vs && d.agent_black && d.ic.open) waves(k_env_step_api4_vs<true>, quad);
        else if (!no_quad_vs && !d.agent_black) waves(k_env_step_api4_vs<false>, quad);
        else if (d.agent_black) waves(k_env_step_api2_vs<true>, pair);
        else waves(k_env_step_api2_vs<false>, pair);
    } else if (d.opp) {
        lanes(k_env_step_api<true>);
    } else {
        lanes(k_env_step_api<false>);
    }
    HIPCHK(hipGetLastError());
    if (spill_after(e)) return -1;
    e->policy_ready = d_pick != nullptr;
    return 0;
}

extern "C" int gc_env_step_device(gc_env* e, const uint16_t* d_actions, int32_t* d_reward, uint8_t* d_done,
                                  uint8_t* d_reason, uint64_t* d_mask, int8_t* d_obs, int32_t* d_count,
                                  uint16_t* d_pick, int flags) {
    return gc_env_step_device2(e, d_actions, d_reward, d_done, d_reason, d_mask, d_obs, d_count, d_pick, flags, 0);
}

// step() of the listed boards only (gc_step_rows.h): row j steps board d_board_idx[j] under
// d_actions[j]; row-compact outputs, the mask by board.  One launch, asynchronous on the env's
// stream; every board not listed, and its mask column, stays as it is.
extern "C" int gc_env_step_boards(gc_env* e, const int32_t* d_board_idx, const uint16_t* d_actions, int rows,
                                  int32_t* d_reward, uint8_t* d_done, uint8_t* d_reason, int32_t* d_count,
                                  uint64_t* d_mask, int64_t mask_stride, int8_t* d_obs, int flags) {
    if (!e) return fail("null env");
    if (rows < 0) return fail("negative row count");
    if (rows > 0 && (!d_board_idx || !d_actions || !d_reward || !d_done || !d_reason)) return fail("null argument");
    if (flags & ~1) return fail("flags: bit 0 = auto-reset");
    if (mask_stride != 0 && mask_stride < (int64_t)e->n) return fail("mask stride below the board count");
    // gc_env_clone_boards' line: a player_color BLACK env's windows can spill into the env's shared
    // table, whose upkeep (gc_host_spill.h) counts on whole-env stepping calls
    if (e->d.agent_black || e->d.ic.spill.ent)
        return fail("step_boards: a player_color BLACK env (spill table) cannot be stepped by board index, as it "
                    "cannot be cloned; the search envs this serves are opponent \"none\"");
    if (rows == 0) return 0;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    const int ar = flags & 1;
    const RowsOut o = {d_reward, d_done, d_reason, d_count, d_mask, d_obs,
                       mask_stride ? (size_t)mask_stride : (size_t)e->n};
    const char* bv = getenv("GC_ROWS_BLOCK");  // A/B (read per call): 64-lane or BLOCK-lane workgroups
    const int block = bv ? (atoi(bv) == BLOCK ? BLOCK : 64) : STEP_ROWS_BLOCK;
    auto lanes = [&](auto kernel) {  // one lane per row
        kernel<<<dim3((rows + block - 1) / block), dim3(block), 0, e->stream>>>(e->d, d_board_idx, d_actions, rows, o, ar);
    };
    if (e->rules) {  // FIDE
        if (e->d.opp) lanes(k_fenv_step_rows<true>);
        else lanes(k_fenv_step_rows<false>);
    } else if (e->d.opp) {
        lanes(k_env_step_rows<true>);
    } else {
        lanes(k_env_step_rows<false>);
    }
    HIPCHK(hipGetLastError());
    e->policy_ready = false;  // act[] describes the listed boards' earlier positions
    return 0;
}

// Policy head on the device (gc_policy.h): per board an action sampled from softmax(logits / T)
// over the legal mask that gc_env_step_device2 wrote (or the greedy one), its log-prob and the
// entropy.  Reads only the mask and the logits at legal actions: either rule set, either
// opponent mode.  Asynchronous on the env's stream, so a following gc_env_step_device2 that
// takes d_action as its actions is ordered after it.
extern "C" int gc_env_sample_policy(gc_env* e, const void* d_logits, int dtype, int64_t row_stride,
                                    const uint64_t* d_mask, int64_t mask_stride, float temperature,
                                    uint64_t seed, uint32_t draw, int flags,
                                    uint16_t* d_action, float* d_logprob, float* d_entropy) {
    if (!e || !d_logits || !d_mask || !d_action) return fail("null argument");
    if (dtype < 0 || dtype > 2) return fail("dtype: 0 float32, 1 float16, 2 bfloat16");
    if (row_stride < 4100) return fail("row stride below the 4100 move actions");
    if (mask_stride != 0 && mask_stride < (int64_t)e->n) return fail("mask stride below the board count");
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail("temperature must be finite and > 0");
    if (flags & ~3) return fail("flags: bit 0 = greedy, bit 1 = logits relative to the side to move");
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    PolicyArgs a;
    a.meta = e->d.st.meta;
    a.logits = d_logits;
    a.row_stride = (size_t)row_stride;
    a.mask = d_mask;
    a.mask_stride = mask_stride ? (size_t)mask_stride : (size_t)e->n;
    a.temperature = temperature;
    a.seed = seed;
    a.draw = draw;
    a.greedy = flags & 1;
    a.action = d_action;
    a.logprob = d_logprob;
    a.entropy = d_entropy;
    a.n = e->n;
    const dim3 grid((e->n + POL_TILE - 1) / POL_TILE), block(64 * POL_WAVES);
    const bool rel = (flags & 2) != 0;  // logits relative to the side to move
    if (dtype == 0) { if (rel) k_sample_policy<0, true><<<grid, block, 0, e->stream>>>(a); else k_sample_policy<0, false><<<grid, block, 0, e->stream>>>(a); }
    else if (dtype == 1) { if (rel) k_sample_policy<1, true><<<grid, block, 0, e->stream>>>(a); else k_sample_policy<1, false><<<grid, block, 0, e->stream>>>(a); }
    else { if (rel) k_sample_policy<2, true><<<grid, block, 0, e->stream>>>(a); else k_sample_policy<2, false><<<grid, block, 0, e->stream>>>(a); }
    HIPCHK(hipGetLastError());
    return 0;
}

// Legal-move priors on the device (gc_priors.h): per row every legal action of its board with its
// prior softmax(logits / T), as a compact [rows][cap] child list for a batched search.  Row j
// reads logits row j and the mask column of board d_board_idx[j] (NULL: board j).  Reads only
// the mask, the logits at legal actions and (flags bit 1) the env's side to move; asynchronous on
// the env's stream.
template <int DT>
static void launch_priors(gc_env* e, const PriorsArgs& a, bool rel) {
    const dim3 grid((unsigned)(((int64_t)a.rows + POL_TILE - 1) / POL_TILE)), block(64 * POL_WAVES);
    const bool idx = a.board_idx != nullptr;
    if (rel) { if (idx) k_policy_priors<DT, true, true><<<grid, block, 0, e->stream>>>(a); else k_policy_priors<DT, true, false><<<grid, block, 0, e->stream>>>(a); }
    else { if (idx) k_policy_priors<DT, false, true><<<grid, block, 0, e->stream>>>(a); else k_policy_priors<DT, false, false><<<grid, block, 0, e->stream>>>(a); }
}

extern "C" int gc_env_policy_priors(gc_env* e, const void* d_logits, int dtype, int64_t row_stride,
                                    const uint64_t* d_mask, int64_t mask_stride,
                                    const int32_t* d_board_idx, int rows,
                                    float temperature, int flags, int cap,
                                    uint16_t* d_actions, float* d_priors, int32_t* d_count, uint16_t* d_logit_idx) {
    if (!e || !d_logits || !d_mask || !d_actions || !d_priors) return fail("null argument");
    if (dtype < 0 || dtype > 2) return fail("dtype: 0 float32, 1 float16, 2 bfloat16");
    if (row_stride < 4100) return fail("row stride below the 4100 move actions");
    if (mask_stride != 0 && mask_stride < (int64_t)e->n) return fail("mask stride below the board count");
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail("temperature must be finite and > 0");
    if (flags & ~2) return fail("flags: bit 1 = logits relative to the side to move; every other bit 0");
    if (cap < 1 || cap > 4100) return fail("cap must be in [1, 4100]");
    if (rows < 0) return fail("negative row count");
    if (!d_board_idx && rows > e->n) return fail("more rows than boards without a board index");
    if (rows == 0) return 0;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    PriorsArgs a;
    a.logits = d_logits;
    a.row_stride = (size_t)row_stride;
    a.mask = d_mask;
    a.mask_stride = mask_stride ? (size_t)mask_stride : (size_t)e->n;
    a.temperature = temperature;
    a.meta = e->d.st.meta;
    a.board_idx = d_board_idx;
    a.rows = rows;
    a.n = e->n;
    a.cap = (u32)cap;
    a.actions = d_actions;
    a.priors = d_priors;
    a.count = d_count;
    a.logit_idx = d_logit_idx;
    const bool rel = (flags & 2) != 0;  // logits relative to the side to move
    if (dtype == 0) launch_priors<0>(e, a, rel);
    else if (dtype == 1) launch_priors<1>(e, a, rel);
    else launch_priors<2>(e, a, rel);
    HIPCHK(hipGetLastError());
    return 0;
}

// The network's input planes of every board's current state (gc_planes.h), asynchronous on the
// env's stream: after a gc_env_step_device2 it describes what that call's mask / obs / pick do.
// Reads the slab and the 3-fold tables, writes nothing but d_planes.
template <int DT, bool NHWC>
static void launch_planes(gc_env* e, const PlanesArgs& a, bool nt) {
    const dim3 grid((e->n + PLN_WAVES - 1) / PLN_WAVES), block(64 * PLN_WAVES);
    if (nt) k_encode_planes<DT, NHWC, true><<<grid, block, 0, e->stream>>>(a);
    else k_encode_planes<DT, NHWC, false><<<grid, block, 0, e->stream>>>(a);
}

extern "C" int gc_env_encode_planes(gc_env* e, void* d_planes, int dtype, int64_t board_stride, int flags) {
    static_assert(GC_PLANES == PLN_C, "the header's plane count is the kernel's");
    if (!e || !d_planes) return fail("null argument");
    if (dtype < 0 || dtype > 2) return fail("dtype: 0 float32, 1 float16, 2 bfloat16");
    if (flags & ~3) return fail("flags: bit 0 = side-to-move view, bit 1 = channels-last");
    if (board_stride != 0 && board_stride < PLN_ELEMS) return fail("board stride below the 1536 elements of a board");
    if (board_stride % 8) return fail("board stride must be a multiple of 8 elements");
    if ((uintptr_t)d_planes % 16) return fail("the planes buffer must be 16-byte aligned");
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    PlanesArgs a;
    a.bb = e->d.st.bb;
    a.meta = e->d.st.meta;
    a.hgen = e->d.hgen;
    a.htab = e->d.htab;
    a.sp = e->d.ic.spill;
    a.out = d_planes;
    a.stride = board_stride ? (size_t)board_stride : (size_t)PLN_ELEMS;
    a.n = e->n;
    a.hbits = e->d.hbits;
    a.persp = flags & 1;
    a.fide = e->rules != 0;
    const char* ntv = getenv("GC_PLANES_NT");  // A/B (read per call): non-temporal stores
    const bool nt = ntv ? atoi(ntv) != 0 : PLN_NT_DEFAULT;
    const bool nhwc = (flags & 2) != 0;
    if (dtype == 0) { if (nhwc) launch_planes<0, true>(e, a, nt); else launch_planes<0, false>(e, a, nt); }
    else if (dtype == 1) { if (nhwc) launch_planes<1, true>(e, a, nt); else launch_planes<1, false>(e, a, nt); }
    else { if (nhwc) launch_planes<2, true>(e, a, nt); else launch_planes<2, false>(e, a, nt); }
    HIPCHK(hipGetLastError());
    return 0;
}

// The planes of the listed boards, row-compact (k_encode_planes_rows): row j = board
// d_board_idx[j].  Read-only like the dense call, so duplicates and any env are fine.
template <int DT, bool NHWC>
static void launch_planes_rows(gc_env* e, const PlanesRowsArgs& a, bool nt) {
    const dim3 grid((a.rows + PLN_WAVES - 1) / PLN_WAVES), block(64 * PLN_WAVES);
    if (nt) k_encode_planes_rows<DT, NHWC, true><<<grid, block, 0, e->stream>>>(a);
    else k_encode_planes_rows<DT, NHWC, false><<<grid, block, 0, e->stream>>>(a);
}

extern "C" int gc_env_encode_planes_rows(gc_env* e, const int32_t* d_board_idx, int rows, void* d_planes,
                                         int dtype, int64_t row_stride, int flags) {
    if (!e || !d_planes) return fail("null argument");
    if (rows < 0) return fail("negative row count");
    if (rows > 0 && !d_board_idx) return fail("null board index");
    if (dtype < 0 || dtype > 2) return fail("dtype: 0 float32, 1 float16, 2 bfloat16");
    if (flags & ~3) return fail("flags: bit 0 = side-to-move view, bit 1 = channels-last");
    if (row_stride != 0 && row_stride < PLN_ELEMS) return fail("row stride below the 1536 elements of a board");
    if (row_stride % 8) return fail("row stride must be a multiple of 8 elements");
    if ((uintptr_t)d_planes % 16) return fail("the planes buffer must be 16-byte aligned");
    if (rows == 0) return 0;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    PlanesRowsArgs a;
    a.p.bb = e->d.st.bb;
    a.p.meta = e->d.st.meta;
    a.p.hgen = e->d.hgen;
    a.p.htab = e->d.htab;
    a.p.sp = e->d.ic.spill;
    a.p.out = d_planes;
    a.p.stride = row_stride ? (size_t)row_stride : (size_t)PLN_ELEMS;
    a.p.n = e->n;
    a.p.hbits = e->d.hbits;
    a.p.persp = flags & 1;
    a.p.fide = e->rules != 0;
    a.board_idx = d_board_idx;
    a.rows = rows;
    const char* ntv = getenv("GC_PLANES_NT");  // A/B (read per call): non-temporal stores
    const bool nt = ntv ? atoi(ntv) != 0 : PLN_ROWS_NT_DEFAULT;
    const bool nhwc = (flags & 2) != 0;
    if (dtype == 0) { if (nhwc) launch_planes_rows<0, true>(e, a, nt); else launch_planes_rows<0, false>(e, a, nt); }
    else if (dtype == 1) { if (nhwc) launch_planes_rows<1, true>(e, a, nt); else launch_planes_rows<1, false>(e, a, nt); }
    else { if (nhwc) launch_planes_rows<2, true>(e, a, nt); else launch_planes_rows<2, false>(e, a, nt); }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gc_env_get_stream(gc_env* e, void** stream) {
    if (!e || !stream) return fail("null argument");
    *stream = (void*)e->stream;
    return 0;
}

// device buffers for callers without their own allocator (tests, bench): hipMalloc /
// hipFree on the env's device, and copies on its stream
extern "C" int gc_device_alloc(int device, uint64_t bytes, void** ptr) {
    if (!ptr) return fail("null argument");
    HIPCHK(hipSetDevice(device));
    return dalloc(reinterpret_cast<uint8_t**>(ptr), (size_t)bytes);
}
// GC_ALLOC_FILL's effect since load: the allocations filled and their bytes
extern "C" int gc_alloc_fill_stats(uint64_t* allocs, uint64_t* bytes) {
    if (!allocs || !bytes) return fail("null argument");
    *allocs = g_fill_allocs.load();
    *bytes = g_fill_bytes.load();
    return 0;
}
extern "C" int gc_device_free(int device, void* ptr) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipFree(ptr));
    return 0;
}
extern "C" int gc_env_copy(gc_env* e, void* dst, const void* src, uint64_t bytes, int kind) {
    if (!e || !dst || !src) return fail("null argument");
    if (kind < 0 || kind > 3) return fail("kind: 0 h2h, 1 h2d, 2 d2h, 3 d2d");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, (hipMemcpyKind)kind, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// n plies of the paired step kernel after the work already on the env's stream: on the
// env's stream, or over the board-range streams (forked from it and joined back into it)
static int issue_plies(gc_env* e, int n) {
    if (e->n_sub <= 1) {
        for (int p = 0; p < n; p++) launch_step2(e, e->stream);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const int blocks = board_blocks(e);
    const int k = e->n_sub < blocks ? e->n_sub : blocks;
    // a range is a whole number of workgroups (PAIRS_WG blocks each), so no workgroup reaches
    // into the next range; only the last range is partial, and beyond it every lane is dead
    const int per = ((blocks + k - 1) / k + PAIRS_WG - 1) / PAIRS_WG * PAIRS_WG;
    HIPCHK(hipEventRecord(e->fork_ev, e->stream));
    for (int j = 0; j < k; j++) HIPCHK(hipStreamWaitEvent(e->sub[j], e->fork_ev, 0));
    for (int p = 0; p < n; p++)
        for (int j = 0; j < k; j++) {
            int b0 = j * per, nb = blocks - b0 < per ? blocks - b0 : per;
            if (nb > 0) launch_step2(e, e->sub[j], b0, nb);
        }
    HIPCHK(hipGetLastError());
    for (int j = 0; j < k; j++) {
        HIPCHK(hipEventRecord(e->sub_ev[j], e->sub[j]));
        HIPCHK(hipStreamWaitEvent(e->stream, e->sub_ev[j], 0));
    }
    return 0;
}

// device-resident random self-play: n_plies launches of the one-ply step kernel (no host
// traffic, no sync).  Outputs of the LAST ply stay in device buffers (gc_env_get_outputs).
// (a hipGraph of the plies' launches was measured slower: 11.4 vs 9.8 us per ply, round 2)
static int step_random(gc_env* e, int n_plies) {
    if (pair_ok(e)) return n_plies > 0 ? issue_plies(e, n_plies) : 0;  // (all but rare opponent setups)
    for (int p = 0; p < n_plies; p++) {
        launch_step<true>(e);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
extern "C" int gc_env_step_random(gc_env* e, int n_plies) {
    if (!e) return fail("null env");
    SRV_QUIESCE(e);
    if (!e->policy_ready) return fail("policy actions stale: call gc_env_reset or gc_env_select_random first");
    HIPCHK(hipSetDevice(e->device));
    if (spill_before(e)) return -1;
    for (int p = 0; p < n_plies;) {  // one chunk unless the env spills (spill_chunk)
        const int k = spill_chunk(e, n_plies - p);
        if (k < 0 || step_random(e, k)) return -1;
        p += k;
    }
    return spill_after(e);
}

// board-range streams of gc_env_step_random (1 = the env's stream only)
extern "C" int gc_env_set_streams(gc_env* e, int k) {
    if (!e) return fail("null env");
    if (k < 1 || k > GC_MAX_SUBSTREAMS) return fail("streams must be in [1, 8]");
    HIPCHK(hipSetDevice(e->device));
    for (int j = 0; j < k; j++) {
        if (!e->sub[j]) HIPCHK(hipStreamCreateWithFlags(&e->sub[j], hipStreamNonBlocking));
        if (!e->sub_ev[j]) HIPCHK(hipEventCreateWithFlags(&e->sub_ev[j], hipEventDisableTiming));
    }
    if (!e->fork_ev) HIPCHK(hipEventCreateWithFlags(&e->fork_ev, hipEventDisableTiming));
    e->n_sub = k;
    return 0;
}

extern "C" int gc_env_paired(gc_env* e) {
    if (!e) return fail("null env");
    return pair_ok(e) ? 1 : 0;
}

// The quads take a reset board's pick from the start position's table only (Q1 reads it in
// phase 0, before the ply's outcome is known); a start position without one (> 16 own pieces,
// or more than RESET_ACTS_MAX moves) runs on the paired kernel, whose pair_ply regenerates the
// start position's move sets at a reset.
static bool use_quad(const gc_env* e) {
    static const bool no_quad = getenv("GC_NO_QUAD") != nullptr;  // A/B: the paired kernel
    return !no_quad && !e->rules && pair_opp(e) == 0 && e->d.ic.table;
}

// The occupancy filter (k_env_rollout4<true>, above) costs Q1 ~700 cycles of phase 1 and the
// ply ~3 % more cycles (tools/pstamp_probe.py); what it buys is half the ply's HBM bytes, and
// with them the clock a long launch holds under the power limit (r06h stamps: 2.27 vs 2.18 GHz
// over 1 000 plies).  Same box, always / never, the workgroups taking turns (profiles/r06_v1/
// ab_summary.txt, run_r06q): K = 20 12.86 / 13.27e9, 100 15.29 / 15.48, 300 15.73 / 15.90, 500
// 15.79 / 15.91, 700 15.91 / 15.43, 1 000 15.94 / 15.12, 2 000 16.26 / 15.62 -- so it runs for
// launches of GC_OCC_MIN_PLIES (600, the crossover) plies or more
static int occ_min_plies() {
    static const int v = getenv("GC_OCC_MIN_PLIES") ? atoi(getenv("GC_OCC_MIN_PLIES")) : 600;
    return v;
}

extern "C" int gc_env_rollout_occ_min_plies(void) { return occ_min_plies(); }

// One quad per workgroup (k_env_rollout4<OCC, ROLL_QUADS_WG>: four workgroups per CU, each
// waiting at its barriers for its own four waves only) runs the ply faster but starts twice
// the workgroups.  Same box, 5 interleaved repeats, one / two quads per workgroup, us per ply
// by events (profiles/r08_geometry/ab_ksweep.log): K = 20 4.66 / 4.41, 50 4.12 / 4.13, 100
// 3.95 / 4.01, 200 3.92 / 4.00, 400 3.87 / 3.93, 600 3.91 / 4.08, 1 000 3.83 / 3.98 -- so
// launches below ROLL_SPLIT_MIN_PLIES plies keep two quads per workgroup
#define ROLL_SPLIT_MIN_PLIES 50
static int roll_quads_wg(int plies) { return plies >= ROLL_SPLIT_MIN_PLIES ? ROLL_QUADS_WG : QUADS_WG; }

extern "C" int gc_env_rollout_waves(gc_env* e) {
    if (!e) return fail("null env");
    return pair_ok(e) ? (use_quad(e) ? 4 : 2) : 1;
}

extern "C" int gc_env_select_random(gc_env* e) {
    if (!e) return fail("null env");
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    if (e->rules) k_fenv_select<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d);
    else k_select<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d);
    HIPCHK(hipGetLastError());
    e->policy_ready = true;
    return 0;
}

// n_plies of fused random self-play after the work already on the env's stream (no host
// sync): ROLLOUT_MAX_PLIES per launch; the per-ply trace (device memory, [n_plies][N] words,
// trace_word) when d_trace is not NULL; with `stats`, per-board stats accumulate into e->stats.
static int issue_rollout(gc_env* e, int n_plies, uint64_t* d_trace, bool stats) {
    uint64_t* const st = stats ? e->stats : nullptr;
    const bool pair = pair_ok(e);
    const EnvDev& d = e->d;
    const ResetInfo r = reset_info(e);
    const LaunchGeom pg = pair_geom(board_blocks(e));
    for (int p0 = 0, k = 0; p0 < n_plies; p0 += k) {
        k = spill_chunk(e, n_plies - p0 < ROLLOUT_MAX_PLIES ? n_plies - p0 : ROLLOUT_MAX_PLIES);
        if (k < 0) return -1;
        u64* tr = d_trace ? reinterpret_cast<u64*>(d_trace) + (size_t)p0 * e->n : nullptr;
        const u32 ri = r.rinfo | ((u32)k << 18);
        e->done_expect = 0;
        if (pair && use_quad(e)) {
            const bool occ = k >= occ_min_plies(), split = roll_quads_wg(k) == ROLL_QUADS_WG;
            const LaunchGeom qg = roll_geom(board_blocks(e), roll_quads_wg(k));
            const auto kernel = split ? (occ ? k_env_rollout4<true, ROLL_QUADS_WG> : k_env_rollout4<false, ROLL_QUADS_WG>)
                                      : (occ ? k_env_rollout4<true, QUADS_WG> : k_env_rollout4<false, QUADS_WG>);
            kernel<<<qg.grid, qg.block, 0, e->stream>>>(e->slab, d.n, d.seed, d.htab, sw_table(r), r.icd, ri, st, tr);
            e->done_expect = ++e->done_issued;
        } else if (pair) {
            const auto kernel = pair_variant(e, k_env_rollout2<true>, k_env_rollout2<false>, k_env_rollout2<false, 1>,
                                             k_env_rollout2<false, 2>);
            kernel<<<pg.grid, pg.block, 0, e->stream>>>(e->slab, d.n, d.seed, d.htab, pair_racts(e, r), r.icd, ri, st, tr);
        } else if (e->rules) {  // FIDE with the random opponent
            k_fenv_rollout<true><<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d, k, tr, st);
        } else if (e->d.opp) {
            k_env_rollout<true><<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d, k, tr, st);
        } else {
            k_env_rollout<false><<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d, k, tr, st);
        }
        hipError_t le = hipGetLastError();
        if (le != hipSuccess) return fail(std::string("rollout launch: ") + hipGetErrorString(le));
    }
    return 0;
}

extern "C" int gc_env_rollout(gc_env* e, int n_plies, int16_t* tr_action, int16_t* tr_reward, uint8_t* tr_done,
                              uint8_t* tr_reason, uint64_t* stats8) {
    if (!e) return fail("null env");
    SRV_QUIESCE(e);
    if (n_plies < 0) return fail("n_plies must be >= 0");
    if (!e->policy_ready) return fail("policy actions stale: call gc_env_reset or gc_env_select_random first");
    HIPCHK(hipSetDevice(e->device));
    const bool trace = tr_action || tr_reward || tr_done || tr_reason;
    const size_t cnt = (size_t)n_plies * e->n;
    Temps tmps;
    u64* dt = nullptr;
    if (trace && cnt && tmps.alloc(&dt, cnt)) return -1;
    if (spill_before(e)) return -1;
    HIPCHK(hipMemsetAsync(e->stats, 0, (size_t)64 * e->n, e->stream));
    if (issue_rollout(e, n_plies, dt, true) || spill_after(e)) return -1;
    if (trace && cnt) {
        std::vector<u64> h(cnt);
        hipError_t ce = hipMemcpyAsync(h.data(), dt, cnt * 8, hipMemcpyDeviceToHost, e->stream);
        if (ce == hipSuccess) ce = hipStreamSynchronize(e->stream);
        if (ce != hipSuccess) return fail(std::string("rollout trace: ") + hipGetErrorString(ce));
        for (size_t t = 0; t < cnt; t++) {
            const u64 w = h[t];
            if (tr_action) tr_action[t] = (int16_t)(uint16_t)w;
            if (tr_reward) tr_reward[t] = (int16_t)(uint16_t)(w >> 16);
            if (tr_done) tr_done[t] = (uint8_t)(w >> 32);
            if (tr_reason) tr_reason[t] = (uint8_t)(w >> 40);
        }
    }
    if (stats8) {
        uint64_t* sums = e->stats + (size_t)8 * e->n;
        HIPCHK(hipMemsetAsync(sums, 0, 64, e->stream));
        k_sum_stats<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->stats, e->n, reinterpret_cast<unsigned long long*>(sums));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(stats8, sums, 64, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return 0;
}

// n_plies env.step() calls of every board under the random self-play policy in one launch
// (per ROLLOUT_MAX_PLIES), asynchronous on the env's stream; each ply's outputs land in the
// device trace [n_plies][N] (trace_word) when d_trace is not NULL.  State, windows, counters
// and the last ply's outputs afterwards are those of n_plies gc_env_step_random plies.
// ev_begin / ev_end: event slots (gc_env_record_event) recorded on the env's stream right
// before / after the launches, -1 = none (one C-ABI call brackets the timed work).
extern "C" int gc_env_rollout_device(gc_env* e, int n_plies, uint64_t* d_trace, int ev_begin, int ev_end) {
    if (!e) return fail("null env");
    SRV_QUIESCE(e);
    if (n_plies < 0) return fail("n_plies must be >= 0");
    if (ev_begin < -1 || ev_begin >= 8 || ev_end < -1 || ev_end >= 8) return fail("event slots: -1 or 0..7");
    if (!e->policy_ready) return fail("policy actions stale: call gc_env_reset or gc_env_select_random first");
    HIPCHK(hipSetDevice(e->device));
    if (spill_before(e)) return -1;
    // marker events around the launches (r03 probe: timing the launches by hipExtLaunchKernel's
    // own start / stop events cost ~8 us more host time per call at K = 20 -- tools/short_probe.py)
    if (ev_begin >= 0) HIPCHK(hipEventRecord(e->ev[ev_begin], e->stream));
    if (issue_rollout(e, n_plies, d_trace, false)) return -1;
    if (ev_end >= 0) HIPCHK(hipEventRecord(e->ev[ev_end], e->stream));
    return spill_after(e);
}

extern "C" int gc_env_get_outputs(gc_env* e, int32_t* reward, uint8_t* done, uint8_t* reason, uint16_t* next_action,
                                  uint32_t* nsteps) {
    if (!e) return fail("null env");
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    if (reward) HIPCHK(hipMemcpyAsync(reward, e->d.reward, (size_t)4 * e->n, hipMemcpyDeviceToHost, e->stream));
    if (done) HIPCHK(hipMemcpyAsync(done, e->d.done, e->n, hipMemcpyDeviceToHost, e->stream));
    if (reason) HIPCHK(hipMemcpyAsync(reason, e->d.reason, e->n, hipMemcpyDeviceToHost, e->stream));
    if (next_action) HIPCHK(hipMemcpyAsync(next_action, e->d.act, (size_t)2 * e->n, hipMemcpyDeviceToHost, e->stream));
    if (nsteps) HIPCHK(hipMemcpyAsync(nsteps, e->d.nsteps, (size_t)4 * e->n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int gc_env_get_states(gc_env* e, int8_t* boards, uint8_t* meta) {
    if (!e) return fail("null env");
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    k_export<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d.st, e->mbox, e->m8);
    HIPCHK(hipGetLastError());
    if (boards) HIPCHK(hipMemcpyAsync(boards, e->mbox, (size_t)64 * e->n, hipMemcpyDeviceToHost, e->stream));
    if (meta) HIPCHK(hipMemcpyAsync(meta, e->m8, (size_t)8 * e->n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// set states (FEN/dict ingest). meta8[7] = move_count; repetition windows are cleared.
extern "C" int gc_env_set_states(gc_env* e, const int8_t* boards, const uint8_t* meta) {
    if (!e || !boards || !meta) return fail("null argument");
    SRV_QUIESCE(e);
    if (check_boards(e->n, boards)) return -1;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->mbox, boards, (size_t)64 * e->n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->m8, meta, (size_t)8 * e->n, hipMemcpyHostToDevice, e->stream));
    if (e->rules) k_fenv_import<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->mbox, e->m8, nullptr, e->d);
    else k_env_import<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->mbox, e->m8, e->d, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    if (spill_windows_cleared(e)) return -1;
    e->policy_ready = false;
    return 0;
}

// FEN ingest for the whole env: boards[i] := fens[i], check flags from update_state,
// repetition windows cleared (like gc_env_set_states)
extern "C" int gc_env_set_fens(gc_env* e, const char* const* fens) {
    if (!e || !fens) return fail("null argument");
    SRV_QUIESCE(e);
    std::vector<int8_t> b((size_t)64 * e->n), ep(e->n, -1);
    std::vector<uint8_t> m((size_t)8 * e->n);
    for (int i = 0; i < e->n; i++) {
        uint8_t* mi = m.data() + 8 * (size_t)i;
        if (gc_fen_to_state_rules(fens[i], b.data() + 64 * (size_t)i, mi, e->rules))
            return fail("board " + std::to_string(i) + ": " + g_err);
        if (e->rules) {  // meta8[7] carried the en-passant file: the env keeps move_count 0
            ep[i] = (int8_t)(mi[7] ? mi[7] - 1 : -1);
            mi[7] = 0;
        }
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->mbox, b.data(), b.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->m8, m.data(), m.size(), hipMemcpyHostToDevice, e->stream));
    if (e->rules) {
        if (!e->ep && dalloc(&e->ep, e->n)) return -1;
        HIPCHK(hipMemcpyAsync(e->ep, ep.data(), e->n, hipMemcpyHostToDevice, e->stream));
        k_fenv_import<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->mbox, e->m8, e->ep, e->d);
    } else {
        k_env_import<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->mbox, e->m8, e->d, 1);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    e->policy_ready = false;
    return 0;
}

extern "C" int gc_env_legal_moves(gc_env* e, uint16_t* moves, int cap, int32_t* counts) {
    if (!e || !moves || !counts) return fail("null argument");
    SRV_QUIESCE(e);
    if (cap <= 0) return fail("cap must be > 0");
    HIPCHK(hipSetDevice(e->device));
    if (cap > e->list_cap) {
        if (e->list) (void)hipFree(e->list);
        e->list = nullptr;
        e->list_cap = 0;
        if (dalloc(&e->list, (size_t)cap * e->n)) return -1;
        e->list_cap = cap;
    }
    if (e->rules) k_flist<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d.st, 0, cap, e->list, e->counts);
    else k_list<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d.st, 0, cap, e->list, e->counts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(moves, e->list, (size_t)2 * cap * e->n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(counts, e->counts, (size_t)4 * e->n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int gc_env_legal_mask(gc_env* e, uint64_t* mask, int32_t* counts) {
    if (!e || !mask) return fail("null argument");
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    if (!e->lmask && dalloc(&e->lmask, (size_t)65 * e->n)) return -1;
    if (e->rules) k_fmask<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d.st, e->lmask, e->counts);
    else k_mask<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d.st, e->lmask, e->counts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(mask, e->lmask, (size_t)8 * 65 * e->n, hipMemcpyDeviceToHost, e->stream));
    if (counts) HIPCHK(hipMemcpyAsync(counts, e->counts, (size_t)4 * e->n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// Wait for the env's stream.  Spin on hipStreamQuery first (bounded): a blocking
// hipStreamSynchronize can sleep on the completion interrupt and pays its wake-up on every
// short wait; after GC_SPIN_US (default 20 000 us) of spinning it blocks.
extern "C" int gc_env_synchronize(gc_env* e) {
    if (!e) return fail("null env");
    HIPCHK(hipSetDevice(e->device));
    static const long spin_us = getenv("GC_SPIN_US") ? atol(getenv("GC_SPIN_US")) : 20000;
    if (spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t q = hipStreamQuery(e->stream);
            if (q == hipSuccess) return 0;
            if (q != hipErrorNotReady) return fail(std::string("stream: ") + hipGetErrorString(q));
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us)) break;
        }
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// Wait for the work of the last gc_env_rollout_device call: when it ended with a quad launch,
// until that launch's completion word reaches host memory (every workgroup's stores done),
// else until the stream is idle.  Work enqueued after the launch (an event record) may still
// be pending; reads through the env's stream stay ordered after it.  Spins with a stream
// query now and then, so a word that never comes cannot hang the caller.
extern "C" int gc_env_wait_rollout(gc_env* e) {
    if (!e) return fail("null env");
    if (!e->done_expect || !e->done_host) return gc_env_synchronize(e);
    const u32 want = e->done_expect;
    for (unsigned k = 0;; k++) {
        if ((int)(__atomic_load_n(e->done_host, __ATOMIC_ACQUIRE) - want) >= 0) return 0;
        if ((k & 255) == 255) {
            const hipError_t q = hipStreamQuery(e->stream);
            if (q == hipSuccess) return 0;
            if (q != hipErrorNotReady) return fail(std::string("stream: ") + hipGetErrorString(q));
        }
    }
}

extern "C" int gc_env_record_event(gc_env* e, int slot) {
    if (!e || slot < 0 || slot >= 8) return fail("bad env or event slot");
    HIPCHK(hipEventRecord(e->ev[slot], e->stream));
    return 0;
}

extern "C" int gc_env_elapsed_ms(gc_env* e, int a, int b, float* ms) {
    if (!e || !ms || a < 0 || a >= 8 || b < 0 || b >= 8) return fail("bad argument");
    HIPCHK(hipEventSynchronize(e->ev[b]));
    HIPCHK(hipEventElapsedTime(ms, e->ev[a], e->ev[b]));
    return 0;
}

// sum over boards of the repetition-window length (bytes accounting in bench.py)
__global__ void k_window_sum(SoA st, unsigned long long* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long v = i < st.n ? (unsigned long long)hl_of(st.meta[i]) : 0ull;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}

extern "C" int gc_env_window_sum(gc_env* e, uint64_t* sum) {
    if (!e || !sum) return fail("null argument");
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    Temps tmps;
    unsigned long long* d = nullptr;
    if (tmps.alloc(&d, 1)) return -1;
    HIPCHK(hipMemsetAsync(d, 0, 8, e->stream));
    k_window_sum<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d.st, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sum, d, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

#ifdef GC_PSTAMPS
// per wave (global wave index = block * waves per block + wave): the 8 segment cycle sums of
// one fused launch of n_plies (reference rules, opponent "none"), then 4 s_memrealtime stamps:
// wave start, entry loads done, first ply done, last ply done.  run (or NULL; the quad rollout):
// per wave, the plies in which the commit loaded a slot beyond the home slot and the cycles of
// their phase 2 (Q1's waves; 0 for the other roles).  last (or NULL; one quad per workgroup): per
// wave and barrier A, B, C, D, the plies in which the wave arrived last, in PST_BINS bins of
// PST_BIN_CYCLES of its margin over the next to last, then the margins' sum
extern "C" int gc_debug_pstamps2(gc_env* e, int n_plies, uint64_t* out /* waves * 12 */, uint64_t* run /* waves * 2 */,
                                 uint32_t* last /* waves * 4 * (PST_BINS + 1) */) {
    Temps tmps;
    unsigned long long *d = nullptr, *dr = nullptr;
    unsigned* dl = nullptr;
    // waves of the fused launch: pairs (2 per 64 boards) or quads (4 per 64 boards)
    const LaunchGeom g = use_quad(e) ? roll_geom(board_blocks(e), roll_quads_wg(n_plies)) : pair_geom(board_blocks(e));
    const size_t waves = (size_t)g.grid.x * (g.block.x / 64);
    const size_t nlast = waves * 4 * (PST_BINS + 1);
    if (tmps.alloc(&d, waves * 12)) return -1;
    HIPCHK(hipMemsetAsync(d, 0, waves * 96, e->stream));
    if (run) {
        if (tmps.alloc(&dr, waves * 2)) return -1;
        HIPCHK(hipMemsetAsync(dr, 0, waves * 16, e->stream));
    }
    if (last) {
        if (tmps.alloc(&dl, nlast)) return -1;
        HIPCHK(hipMemsetAsync(dl, 0, nlast * 4, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_pst_out), &d, sizeof(d)));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_pst_run_out), &dr, sizeof(dr)));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_pst_last_out), &dl, sizeof(dl)));
    if (issue_rollout(e, n_plies, nullptr, false)) return -1;
    HIPCHK(hipMemcpyAsync(out, d, waves * 96, hipMemcpyDeviceToHost, e->stream));
    if (run) HIPCHK(hipMemcpyAsync(run, dr, waves * 16, hipMemcpyDeviceToHost, e->stream));
    if (last) HIPCHK(hipMemcpyAsync(last, dl, nlast * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    unsigned long long* z = nullptr;
    unsigned* zl = nullptr;
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_pst_out), &z, sizeof(z)));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_pst_run_out), &z, sizeof(z)));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_pst_last_out), &zl, sizeof(zl)));
    return 0;
}
extern "C" int gc_debug_pstamps(gc_env* e, int n_plies, uint64_t* out, uint64_t* run) {
    return gc_debug_pstamps2(e, n_plies, out, run, nullptr);
}
#endif

#ifdef GC_PSTAMPS
// the quad API step's per-wave stamps (tools/api_pstamp_probe.py): buffer on (`on` != 0, sized
// for the env's k_env_step_api4 waves, zeroed) or copied out and off
static unsigned long long* g_api_pst = nullptr;
extern "C" int gc_debug_api_pstamps(gc_env* e, int on, uint64_t* out /* waves * 12 */) {
    const LaunchGeom g = quad_geom(board_blocks(e));
    const size_t waves = (size_t)g.grid.x * (g.block.x / 64);
    HIPCHK(hipStreamSynchronize(e->stream));
    if (on) {
        if (!g_api_pst && dalloc(&g_api_pst, waves * 12)) return -1;
        HIPCHK(hipMemset(g_api_pst, 0, waves * 96));
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_pst_out), &g_api_pst, sizeof(g_api_pst)));
        return 0;
    }
    if (g_api_pst && out) HIPCHK(hipMemcpy(out, g_api_pst, waves * 96, hipMemcpyDeviceToHost));
    unsigned long long* z = nullptr;
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_pst_out), &z, sizeof(z)));
    return 0;
}
#endif

#ifdef GC_STAMPS
extern "C" int gc_debug_stamps(gc_env* e, int n_plies, uint64_t* out /* (n/64)*8 */) {
    Temps tmps;
    unsigned long long* d = nullptr;
    size_t cnt = (size_t)((e->n + 63) / 64) * 16;  // per wave: 8 stamps (the paired kernel has 2 waves / 64 boards)
    if (tmps.alloc(&d, cnt)) return -1;
    HIPCHK(hipMemsetAsync(d, 0, cnt * 8, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_out), &d, sizeof(d)));
    for (int p = 0; p < n_plies; p++) {
        launch_step2(e, e->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d, cnt * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    unsigned long long* z = nullptr;
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_out), &z, sizeof(z)));
    return 0;
}
#endif

// en passant of the FIDE-rules env (gc_fide.h keeps it in meta bits 25..28; the env's
// meta8[7] is move_count, so it travels beside the state arrays)
__global__ void k_get_ep(SoA st, int8_t* __restrict__ files) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= st.n) return;
    u32 m = st.meta[i];
    files[i] = (m & gcf::M_EP) ? (int8_t)((m & gcf::M_EP_MASK) >> gcf::M_EP_SHIFT) : (int8_t)-1;
}
__global__ void k_set_ep(SoA st, const int8_t* __restrict__ files) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= st.n) return;
    st.meta[i] = gcf::with_ep(st.meta[i], files[i] < 0 ? -1 : (int)files[i]);
}

extern "C" int gc_env_get_en_passant(gc_env* e, int8_t* files) {
    if (!e || !files) return fail("null argument");
    HIPCHK(hipSetDevice(e->device));
    if (!e->ep && dalloc(&e->ep, e->n)) return -1;
    k_get_ep<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d.st, e->ep);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(files, e->ep, e->n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int gc_env_set_en_passant(gc_env* e, const int8_t* files) {
    if (!e || !files) return fail("null argument");
    for (int i = 0; i < e->n; i++) {
        if (files[i] > 7) return fail("en-passant file out of range at index " + std::to_string(i));
        if (files[i] >= 0 && !e->rules) return fail("en passant exists only under rules=fide (Q3: the reference has none)");
    }
    HIPCHK(hipSetDevice(e->device));
    if (!e->ep && dalloc(&e->ep, e->n)) return -1;
    HIPCHK(hipMemcpyAsync(e->ep, files, e->n, hipMemcpyHostToDevice, e->stream));
    k_set_ep<<<grid_for(e->n), BLOCK, 0, e->stream>>>(e->d.st, e->ep);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    e->policy_ready = false;
    return 0;
}

// bytes of device memory held by the env (for reports)
extern "C" uint64_t gc_env_device_bytes(gc_env* e) {
    if (!e) return 0;
    uint64_t n = (uint64_t)e->n;
    return n * (NBB * 8 + 4) + n * ((uint64_t)64 << e->d.hbits) + n * (4 + 4 + 2 + 4 + 1 + 1 + 4) +
           n * (64 + 8 + 1 + 4 + 64);
}
