// gc_host_minimax.h -- gc_env_minimax / gc_env_minimax_q: the one launch of k_minimax (gc_minimax.h),
// asynchronous on the env's stream.  No handle: the search allocates nothing on the device.
// quiesce == 0 launches the plain instantiations (k_minimax<NODES>), quiesce >= 1 the two with the
// quiescence nest below the leaves (k_minimax<NODES, true>).
#pragma once

extern "C" int gc_env_minimax_q(gc_env* e, const int32_t* d_board_idx, int rows, int depth, int quiesce, int tiebreak,
                                uint64_t seed, uint32_t draw, uint16_t* d_pick, int32_t* d_score, float* d_value,
                                int32_t* d_count, int cap, uint16_t* d_actions, int32_t* d_scores, uint32_t* d_nodes) {
    if (!e) return fail("null env");
    if (e->rules != 0) return fail("minimax: reference rules only (not a rules=\"fide\" env)");
    if (rows < 0) return fail("rows must be >= 0");
    if (depth < 1 || depth > MM_MAX_DEPTH) return fail("depth must be in [1, 4]");
    if (quiesce < 0 || quiesce > MM_MAX_QUIESCE) return fail("quiesce must be in [0, 4]");
    if (tiebreak != 0 && tiebreak != 1) return fail("tiebreak must be 0 (first) or 1 (random)");
    if (cap < 0) return fail("cap must be >= 0");
    if (cap == 0 && (d_actions || d_scores)) return fail("a list output needs cap >= 1");
    if (rows == 0) return 0;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    MinimaxArgs a;
    a.idx = d_board_idx;
    a.depth = depth;
    a.tiebreak = tiebreak;
    a.seed = seed;
    a.draw = draw;
    a.pick = d_pick;
    a.score = d_score;
    a.value = d_value;
    a.count = d_count;
    a.cap = (d_actions || d_scores) ? cap : 0;
    a.actions = d_actions;
    a.scores = d_scores;
    a.quiesce = quiesce;
    const dim3 grid((unsigned)rows), block(MINIMAX_BLOCK);
    if (quiesce) {
        if (d_nodes) k_minimax<true, true><<<grid, block, 0, e->stream>>>(e->d.st, a, d_nodes);
        else k_minimax<false, true><<<grid, block, 0, e->stream>>>(e->d.st, a, nullptr);
    } else {
        if (d_nodes) k_minimax<true><<<grid, block, 0, e->stream>>>(e->d.st, a, d_nodes);
        else k_minimax<false><<<grid, block, 0, e->stream>>>(e->d.st, a, nullptr);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gc_env_minimax(gc_env* e, const int32_t* d_board_idx, int rows, int depth, int tiebreak, uint64_t seed,
                              uint32_t draw, uint16_t* d_pick, int32_t* d_score, float* d_value, int32_t* d_count,
                              int cap, uint16_t* d_actions, int32_t* d_scores, uint32_t* d_nodes) {
    return gc_env_minimax_q(e, d_board_idx, rows, depth, 0, tiebreak, seed, draw, d_pick, d_score, d_value, d_count, cap,
                            d_actions, d_scores, d_nodes);
}
