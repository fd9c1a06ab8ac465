// gc_host_clone.h -- gc_env_clone_boards / gc_env_clone_errors: boards copied between envs (or
// within one) by k_clone_boards (gc_clone.h), asynchronous on the destination's stream.
#pragma once

extern "C" int gc_env_clone_boards(gc_env* dst, gc_env* src, const int32_t* d_src_idx, const int32_t* d_dst_idx, int m) {
    if (!dst || !src) return fail("null env");
    if (m < 0) return fail("m must be >= 0");
    if (m > 0 && (!d_src_idx || !d_dst_idx)) return fail("null index array");
    if (dst->device != src->device) return fail("clone: the envs live on different devices");
    if (dst->rules != src->rules) return fail("clone: the envs play under different rules");
    // a player_color BLACK env's windows can live partly in its shared spill table, which a
    // position-for-position copy does not cover
    if (dst->d.ic.spill.ent || src->d.ic.spill.ent)
        return fail("clone: a player_color BLACK env (spill table) cannot be cloned from or into; use the checkpoint");
    if (dst->d.hbits != src->d.hbits) return fail("clone: the envs' 3-fold tables differ in size");
    if (m == 0) return 0;
    SRV_QUIESCE(dst);
    SRV_QUIESCE(src);
    HIPCHK(hipSetDevice(dst->device));
    if (!dst->clone_skipped) {
        if (dalloc(&dst->clone_skipped, 1)) return -1;
        HIPCHK(hipMemsetAsync(dst->clone_skipped, 0, 8, dst->stream));
    }
    if (src != dst) {  // after the work already on the source's stream
        if (!src->clone_ev) HIPCHK(hipEventCreateWithFlags(&src->clone_ev, hipEventDisableTiming));
        if (!dst->clone_ev) HIPCHK(hipEventCreateWithFlags(&dst->clone_ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(src->clone_ev, src->stream));
        HIPCHK(hipStreamWaitEvent(dst->stream, src->clone_ev, 0));
    }
    CloneArgs a;
    a.sslab = src->slab;
    a.stab = src->d.htab;
    a.dslab = dst->slab;
    a.dtab = dst->d.htab;
    a.sidx = d_src_idx;
    a.didx = d_dst_idx;
    a.skipped = dst->clone_skipped;
    a.ns = src->n;
    a.nd = dst->n;
    a.m = m;
    a.hbits = dst->d.hbits;
    k_clone_boards<<<dim3((m + CLN_WAVES - 1) / CLN_WAVES), dim3(64 * CLN_WAVES), 0, dst->stream>>>(a);
    HIPCHK(hipGetLastError());
    if (src != dst) {  // and before the source's later work, which may change the boards read here
        HIPCHK(hipEventRecord(dst->clone_ev, dst->stream));
        HIPCHK(hipStreamWaitEvent(src->stream, dst->clone_ev, 0));
    }
    dst->policy_ready = false;  // act[] describes the boards' earlier positions
    return 0;
}

extern "C" int gc_env_clone_errors(gc_env* dst, uint64_t* skipped) {
    if (!dst || !skipped) return fail("null argument");
    HIPCHK(hipSetDevice(dst->device));
    *skipped = 0;
    if (dst->clone_skipped)
        HIPCHK(hipMemcpyAsync(skipped, dst->clone_skipped, 8, hipMemcpyDeviceToHost, dst->stream));
    HIPCHK(hipStreamSynchronize(dst->stream));
    return 0;
}
