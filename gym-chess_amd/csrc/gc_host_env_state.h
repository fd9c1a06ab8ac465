// gc_host_env_state.h -- struct gc_env and its teardown.
#pragma once

// ----------------------------------------------------------------------------- env API
#define GC_MAX_SUBSTREAMS 8
#ifndef GC_DEFAULT_STREAMS
#define GC_DEFAULT_STREAMS 2  // measured: 1 stream 10.2 us per ply, 2 streams 9.8, 3 10.6, 4 17 (graph-captured 11.4)
#endif
struct gc_env {
    int device = 0, n = 0;
    uint64_t seed = 0;
    hipStream_t stream = nullptr;
    EnvDev d{};
    u64* bb = nullptr; u32* meta = nullptr;
    int8_t* mbox = nullptr; uint8_t* m8 = nullptr; uint8_t* mask = nullptr;
    uint16_t* list = nullptr; int list_cap = 0; int32_t* counts = nullptr; u64* lmask = nullptr;
    uint64_t* stats = nullptr;
    hipEvent_t ev[8] = {};
    bool policy_ready = false;  // act[] holds policy picks for the current states
    int rules = 0;              // 0 reference, 1 FIDE (gc_fide.h)
    int8_t* ep = nullptr;       // FIDE ingest: en-passant files
    ApiOut* api_out = nullptr;  // the paired API step's output pointers (device copy of api_host)
    ApiOut api_host{};
    uint16_t* reset_acts = nullptr;
    EnvDev::InitCache* icd = nullptr;  // device copy of d.ic (the paired kernels read it from HBM)
    EnvDev::InitCache* icd_f = nullptr;  // the same for the FIDE reset position (gc_env_set_rules)
    uint16_t* racts_f = nullptr;
    OpenCache* open_cache = nullptr;     // a BLACK agent's openings (k_init_open_cache, gc_env_set_opponent)
    uint16_t* open_acts = nullptr;
    EnvDev::InitCache ic_f = {};
    uint8_t* slab = nullptr;  // per-board fields (Slab): bb, meta, hgen, draw, nsteps, reward, act, done, reason
    // Board-range streams of gc_env_step_random (gc_env_set_streams): ply p+1 of one range
    // depends only on ply p of the same range, so the ranges' launches interleave and the
    // launch ramp / tail of one range's ply overlaps another range's waves.
    int n_sub = 1;
    hipStream_t sub[GC_MAX_SUBSTREAMS] = {};
    hipEvent_t sub_ev[GC_MAX_SUBSTREAMS] = {};
    hipEvent_t fork_ev = nullptr;
    // gc_env_clone_boards: the event that orders a clone between this env's stream and the other
    // env's, and the count of pairs skipped for an index out of range (device, since creation)
    hipEvent_t clone_ev = nullptr;
    unsigned long long* clone_skipped = nullptr;
    // the spill table of a BLACK agent's windows (gc_env.h; SpillTab): its slot counters are
    // copied to pinned host memory after every stepping call and checked before the next one
    int sp_bits = 0;
    u32* sp_ctr_h = nullptr;  // pinned: {slots claimed, failed}
    hipEvent_t sp_ev = nullptr;
    int sp_pending = 0;       // stepping calls since the last counter copy was read
    bool sp_failed = false;   // an insert failed: every stepping call fails until the windows are cleared
    gc_single_record* srec = nullptr;  // gc_env_single_call's host-mapped record
    gc_single_record* srec_d = nullptr;  // its device address
    // the quad rollout's completion word (EnvDev::InitCache::DoneWord): its host-mapped copy,
    // the launches issued so far, and the count the last gc_env_rollout_device call waits for
    // (0: the last call's work was not a quad launch -- gc_env_wait_rollout syncs the stream)
    u32* done_host = nullptr;
    u32* done_dev = nullptr;  // {ctr, seq}
    u32 done_issued = 0;
    u32 done_expect = 0;
    // the single-board server (k_single_server) and the board it holds
    SrvClient<SrvBox> srv{"single-board server"};
    int srv_board = -1;
};

// before any launch on the env's device: no resident server (its own or another owner's) holds a queue
#define SRV_QUIESCE(e) do { if (devsrv_quiesce((e)->device)) return -1; } while (0)

static void env_free(gc_env* e) {
    void* ps[] = {e->api_out, e->reset_acts, e->icd, e->icd_f, e->racts_f, e->open_cache, e->open_acts, e->ep, e->slab, e->d.htab, e->mbox, e->m8, e->mask,
                  e->list, e->counts, e->lmask, e->stats, e->clone_skipped};
    for (void* p : ps) if (p) (void)hipFree(p);
    for (auto& v : e->ev) if (v) (void)hipEventDestroy(v);
    for (int j = 0; j < GC_MAX_SUBSTREAMS; j++) {
        if (e->sub_ev[j]) (void)hipEventDestroy(e->sub_ev[j]);
        if (e->sub[j]) (void)hipStreamDestroy(e->sub[j]);
    }
    if (e->fork_ev) (void)hipEventDestroy(e->fork_ev);
    if (e->clone_ev) (void)hipEventDestroy(e->clone_ev);
    if (e->d.ic.spill.ent) (void)hipFree(e->d.ic.spill.ent);
    if (e->d.ic.spill.ctr) (void)hipFree(e->d.ic.spill.ctr);
    if (e->sp_ctr_h) (void)hipHostFree(e->sp_ctr_h);
    if (e->sp_ev) (void)hipEventDestroy(e->sp_ev);
    if (e->srec) (void)hipHostFree(e->srec);
    if (e->done_host) (void)hipHostFree(e->done_host);
    e->srv.destroy();
    if (e->done_dev) (void)hipFree(e->done_dev);
    if (e->stream) (void)hipStreamDestroy(e->stream);
}
