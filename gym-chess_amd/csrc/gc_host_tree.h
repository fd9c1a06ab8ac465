// gc_host_tree.h -- gc_tree_*: the batched search tree's handle, its one device allocation (and
// advance's remap scratch, the batch scratch, the solver's and Gumbel root search's arrays, allocated when first needed) and the launches of gc_tree.h's kernels,
// all asynchronous on the tree env's stream.
#pragma once

struct gc_tree {
    gc_env* e = nullptr;
    int device = 0;
    TreeDev d{};
    uint8_t* slab = nullptr;  // every array of d, 256-byte aligned, in GC_TREE_ARRAYS order
    size_t bytes = 0;         // the slab, plus the remap scratch once it exists
    int32_t* remap = nullptr;  // [games][nodes]: gc_tree_advance's remap when the caller passes none
    bool pending = false;  // a selection waits for its backup
    // gc_tree_batch_reserve's scratch: one allocation, GC_TREE_BATCH_ARRAYS arrays in the header's order
    TreeBatchDev b{};
    uint8_t* bslab = nullptr;
    size_t bbytes = 0;
    int batch_pending = 0;  // leaves per game of the batch that waits for its backup, 0 = none
    // gc_tree_solver_enable's arrays: one allocation, GC_TREE_SOLVER_ARRAYS arrays in the header's order
    TreeSolverDev v{};
    uint8_t* vslab = nullptr;
    // gc_tree_gumbel_enable's arrays: one allocation, GC_TREE_GUMBEL_ARRAYS arrays in the header's order
    TreeGumbelDev u{};
    uint8_t* uslab = nullptr;
    size_t ubytes = 0;
    bool armed = false;  // gc_tree_gumbel_begin ran for this root: select takes the Gumbel rule at level 0
};

// the arrays' sizes in bytes, in the header's order
static void tree_sizes(size_t G, size_t nodes, size_t cap, size_t out[GC_TREE_ARRAYS]) {
    const size_t e = G * nodes * cap, n = G * nodes;
    const size_t s[GC_TREE_ARRAYS] = {2 * e, 4 * e, 4 * e, 4 * e, 4 * e, 4 * n, 4 * n, 4 * n,
                                      4 * n, n,     4 * G, 4 * G, 4 * G, 4 * G, 4 * G, 8 * n};
    for (int k = 0; k < GC_TREE_ARRAYS; k++) out[k] = s[k];
}
static void tree_addresses(const gc_tree* t, void* out[GC_TREE_ARRAYS]) {
    const TreeDev& d = t->d;
    void* p[GC_TREE_ARRAYS] = {d.action,  d.prior,    d.child,       d.edge_visits, d.edge_value, d.n_children,
                               d.parent,  d.parent_slot, d.leaf_value, d.terminal,    d.n_nodes,    d.overflow,
                               d.depth,   d.leaf,     d.leaf_new,    d.path};
    for (int k = 0; k < GC_TREE_ARRAYS; k++) out[k] = p[k];
}
// the batch scratch's sizes in bytes, in the header's order
static void tree_batch_sizes(size_t G, size_t nodes, size_t cap, size_t K, size_t out[GC_TREE_BATCH_ARRAYS]) {
    const size_t s[GC_TREE_BATCH_ARRAYS] = {G * nodes * cap, 8 * G * K * nodes, 4 * G * K, 4 * G * K, 4 * G * K, 4 * G};
    for (int k = 0; k < GC_TREE_BATCH_ARRAYS; k++) out[k] = s[k];
}
// the solver's arrays' sizes in bytes, in the header's order
static void tree_solver_sizes(size_t G, size_t nodes, size_t cap, size_t out[GC_TREE_SOLVER_ARRAYS]) {
    const size_t e = G * nodes * cap, n = G * nodes;
    const size_t s[GC_TREE_SOLVER_ARRAYS] = {e, 2 * e, n, 2 * n, n};
    for (int k = 0; k < GC_TREE_SOLVER_ARRAYS; k++) out[k] = s[k];
}
// Gumbel root search's arrays' sizes in bytes, in the header's order
static void tree_gumbel_sizes(size_t G, size_t cap, size_t considered, size_t sims, size_t out[GC_TREE_GUMBEL_ARRAYS]) {
    const size_t s[GC_TREE_GUMBEL_ARRAYS] = {4 * G * cap, 4 * G * cap, 4 * G * cap, 2 * (considered + 1) * sims};
    for (int k = 0; k < GC_TREE_GUMBEL_ARRAYS; k++) out[k] = s[k];
}
// The considered visit counts, [considered + 1][sims]: row k is the order in which sequential
// halving spends `sims` simulations on k considered moves (the header has the rule).
static std::vector<uint16_t> tree_gumbel_table(int considered, int sims) {
    std::vector<uint16_t> t((size_t)(considered + 1) * sims, 0);
    for (int k = 1; k <= considered; k++) {
        uint16_t* row = t.data() + (size_t)k * sims;
        if (k == 1) {
            for (int i = 0; i < sims; i++) row[i] = (uint16_t)i;
            continue;
        }
        int L = 0;
        while ((1 << L) < k) L++;
        std::vector<int> n((size_t)k, 0);
        int r = k, at = 0;
        while (at < sims) {
            int e = sims / (L * r);
            e = e > 1 ? e : 1;
            for (int i = 0; i < e && at < sims; i++)
                for (int m = 0; m < r; m++) {
                    if (at < sims) row[at++] = (uint16_t)n[m];
                    n[m]++;
                }
            r = r / 2 > 2 ? r / 2 : 2;
        }
    }
    return t;
}
static const char* const TREE_GUMBEL_NO_SOLVER =
    "a gumbel tree (gc_tree_gumbel_enable) takes no solver: the two together are not defined yet";
static const char* const TREE_GUMBEL_NO_BATCH =
    "a gumbel tree (gc_tree_gumbel_enable) takes one leaf per game per call: the batch calls are not defined for it yet";
static const char* const TREE_BATCH_PENDING = "a batch is pending: gc_tree_backup_batch first";
static const char* const TREE_SOLVER_NO_BATCH =
    "a solver tree takes one leaf per game per call: the batch calls are not defined for it yet";
static inline dim3 tree_grid(const gc_tree* t) { return dim3((unsigned)((t->d.games + TREE_WAVES - 1) / TREE_WAVES)); }

extern "C" int gc_tree_create(gc_env* e, int games, int nodes, int cap, gc_tree** out) {
    if (!e || !out) return fail("null argument");
    if (games < 1) return fail("games must be >= 1");
    if (nodes < 1) return fail("nodes must be >= 1");
    if (cap < 1 || cap > TREE_MAX_CAP) return fail("cap must be in [1, 256]");
    if ((int64_t)games * nodes > (int64_t)e->n) return fail("games * nodes exceeds the env's boards");
    HIPCHK(hipSetDevice(e->device));
    size_t sz[GC_TREE_ARRAYS], off[GC_TREE_ARRAYS], total = 0;
    tree_sizes((size_t)games, (size_t)nodes, (size_t)cap, sz);
    for (int k = 0; k < GC_TREE_ARRAYS; k++) {
        off[k] = total;
        total += (sz[k] + 255) & ~(size_t)255;
    }
    gc_tree* t = new gc_tree();
    if (dalloc(&t->slab, total)) {
        delete t;
        return -1;
    }
    hipError_t rc = hipMemsetAsync(t->slab, 0, total, e->stream);
    if (rc != hipSuccess) {
        (void)hipFree(t->slab);
        delete t;
        return fail(std::string("hipMemsetAsync: ") + hipGetErrorString(rc));
    }
    t->e = e;
    t->device = e->device;
    t->bytes = total;
    uint8_t* b = t->slab;
    TreeDev& d = t->d;
    d.action = (uint16_t*)(b + off[0]);
    d.prior = (float*)(b + off[1]);
    d.child = (int32_t*)(b + off[2]);
    d.edge_visits = (int32_t*)(b + off[3]);
    d.edge_value = (float*)(b + off[4]);
    d.n_children = (int32_t*)(b + off[5]);
    d.parent = (int32_t*)(b + off[6]);
    d.parent_slot = (int32_t*)(b + off[7]);
    d.leaf_value = (float*)(b + off[8]);
    d.terminal = (uint8_t*)(b + off[9]);
    d.n_nodes = (int32_t*)(b + off[10]);
    d.overflow = (int32_t*)(b + off[11]);
    d.depth = (int32_t*)(b + off[12]);
    d.leaf = (int32_t*)(b + off[13]);
    d.leaf_new = (int32_t*)(b + off[14]);
    d.path = (int32_t*)(b + off[15]);
    d.games = games;
    d.nodes = nodes;
    d.cap = cap;
    *out = t;
    return 0;
}

extern "C" int gc_tree_destroy(gc_tree* t) {
    if (!t) return fail("null tree");
    (void)hipSetDevice(t->device);  // (not through e: the env may be gone already)
    if (t->slab) (void)hipFree(t->slab);  // (waits for the device: no launch still uses the arrays)
    if (t->remap) (void)hipFree(t->remap);
    if (t->bslab) (void)hipFree(t->bslab);
    if (t->vslab) (void)hipFree(t->vslab);
    if (t->uslab) (void)hipFree(t->uslab);
    delete t;
    return 0;
}

extern "C" int gc_tree_reset(gc_tree* t, const uint16_t* d_actions, const float* d_priors, const int32_t* d_count,
                             int pri_cap, const float* d_value) {
    if (!t) return fail("null tree");
    if (!d_actions || !d_priors || !d_count) return fail("null priors block");
    if (pri_cap < 1) return fail("pri_cap must be >= 1");
    SRV_QUIESCE(t->e);
    HIPCHK(hipSetDevice(t->e->device));
    if (t->batch_pending) {  // the pending descents' marks: no batch pending means every in-flight byte is 0
        const TreeDev& d = t->d;
        HIPCHK(hipMemsetAsync(t->b.inflight, 0, (size_t)d.games * d.nodes * d.cap, t->e->stream));
    }
    const TreePriors p{d_actions, d_priors, d_count, pri_cap};
    if (t->vslab)
        k_tree_reset<true><<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, p, d_value, t->v);
    else
        k_tree_reset<false><<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, p, d_value, t->v);
    HIPCHK(hipGetLastError());
    t->pending = false;
    t->batch_pending = 0;
    t->armed = false;
    return 0;
}

extern "C" int gc_tree_select(gc_tree* t, float c_puct, float fpu, int32_t* d_parent, int32_t* d_child,
                              uint16_t* d_action) {
    if (!t) return fail("null tree");
    if (!d_parent || !d_child || !d_action) return fail("null output array");
    if (!std::isfinite(c_puct) || c_puct < 0.f) return fail("c_puct must be finite and >= 0");
    if (fpu != fpu) return fail("fpu is NaN");
    if (t->pending) return fail("a selection is pending: gc_tree_backup first");
    if (t->batch_pending) return fail(TREE_BATCH_PENDING);
    SRV_QUIESCE(t->e);
    HIPCHK(hipSetDevice(t->e->device));
    if (t->armed)
        k_tree_select<false, true><<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(
            t->d, c_puct, fpu, d_parent, d_child, d_action, t->v, t->u);
    else if (t->vslab)
        k_tree_select<true><<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, c_puct, fpu, d_parent,
                                                                                      d_child, d_action, t->v, t->u);
    else
        k_tree_select<false><<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, c_puct, fpu, d_parent,
                                                                                       d_child, d_action, t->v, t->u);
    HIPCHK(hipGetLastError());
    t->pending = true;
    return 0;
}

extern "C" int gc_tree_backup(gc_tree* t, const float* d_value, const uint8_t* d_done, const uint8_t* d_reason,
                              const uint16_t* d_actions, const float* d_priors, const int32_t* d_count, int pri_cap) {
    if (!t) return fail("null tree");
    if (!d_value || !d_done || !d_reason) return fail("null value / done / reason array");
    if (!d_actions || !d_priors || !d_count) return fail("null priors block");
    if (pri_cap < 1) return fail("pri_cap must be >= 1");
    if (t->batch_pending) return fail(TREE_BATCH_PENDING);
    if (!t->pending) return fail("no selection is pending: gc_tree_select first");
    SRV_QUIESCE(t->e);
    HIPCHK(hipSetDevice(t->e->device));
    const TreePriors p{d_actions, d_priors, d_count, pri_cap};
    if (t->vslab)
        k_tree_backup<true><<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, d_value, d_done, d_reason, p,
                                                                                      t->v);
    else
        k_tree_backup<false><<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, d_value, d_done, d_reason,
                                                                                       p, t->v);
    HIPCHK(hipGetLastError());
    t->pending = false;
    return 0;
}

extern "C" int gc_tree_advance(gc_tree* t, const uint16_t* d_move, const uint16_t* d_actions, const float* d_priors,
                               const int32_t* d_count, int pri_cap, const float* d_value, int32_t* d_kept,
                               int32_t* d_remap) {
    if (!t) return fail("null tree");
    if (!d_move || !d_kept) return fail("null move / kept array");
    if (!d_actions || !d_priors || !d_count) return fail("null priors block");
    if (pri_cap < 1) return fail("pri_cap must be >= 1");
    if (t->pending) return fail("a selection is pending: gc_tree_backup first");
    if (t->batch_pending) return fail(TREE_BATCH_PENDING);
    gc_env* e = t->e;
    // the board move is a clone within the tree env: refused where gc_env_clone_boards(e, e, ...) is
    if (e->d.ic.spill.ent)
        return fail("advance: a player_color BLACK tree env (spill table) cannot move boards; use the checkpoint");
    if (t->d.nodes > TREE_ADV_MAX_NODES) return fail("advance: nodes exceeds 65536 (the keep bitmap's LDS)");
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    if (!d_remap && !t->remap) {
        if (dalloc(&t->remap, (size_t)t->d.games * t->d.nodes)) return -1;
        t->bytes += (size_t)t->d.games * t->d.nodes * sizeof(int32_t);
    }
    int32_t* remap = d_remap ? d_remap : t->remap;
    const TreePriors p{d_actions, d_priors, d_count, pri_cap};
    const size_t lds = (size_t)TREE_WAVES * ((t->d.nodes + 63) / 64) * sizeof(unsigned long long);
    k_tree_advance_mark<<<tree_grid(t), dim3(64 * TREE_WAVES), lds, e->stream>>>(t->d, d_move, d_kept, remap);
    HIPCHK(hipGetLastError());
    if (t->vslab)
        k_tree_advance_compact<true><<<tree_grid(t), dim3(64 * TREE_WAVES), 0, e->stream>>>(t->d, p, d_value, d_kept,
                                                                                            remap, t->v);
    else
        k_tree_advance_compact<false><<<tree_grid(t), dim3(64 * TREE_WAVES), 0, e->stream>>>(t->d, p, d_value, d_kept,
                                                                                             remap, t->v);
    HIPCHK(hipGetLastError());
    CloneArgs a;
    a.sslab = e->slab;
    a.stab = e->d.htab;
    a.dslab = e->slab;
    a.dtab = e->d.htab;
    a.sidx = nullptr;
    a.didx = nullptr;
    a.skipped = nullptr;
    a.ns = e->n;
    a.nd = e->n;
    a.m = 0;
    a.hbits = e->d.hbits;
    k_move_boards<<<dim3((t->d.games + CLN_WAVES - 1) / CLN_WAVES), dim3(64 * CLN_WAVES), 0, e->stream>>>(
        a, remap, d_kept, t->d.games, t->d.nodes);
    HIPCHK(hipGetLastError());
    e->policy_ready = false;  // act[] describes the moved boards' earlier positions
    t->armed = false;  // the root changed: gc_tree_gumbel_begin draws for the new one
    return 0;
}

extern "C" int gc_tree_root_policy(gc_tree* t, uint64_t seed, uint32_t draw, int flags, uint16_t* d_actions,
                                   int32_t* d_visits, float* d_pi, uint16_t* d_pick, float* d_value) {
    if (!t) return fail("null tree");
    if (flags & ~3) return fail("flags: bit 0 = greedy, bit 1 = proofs (a solver tree); every other bit 0");
    if ((flags & 2) && !t->vslab) return fail("flags bit 1 (proofs) needs a solver tree: gc_tree_solver_enable first");
    if (t->pending) return fail("a selection is pending: gc_tree_backup first");
    if (t->batch_pending) return fail(TREE_BATCH_PENDING);
    SRV_QUIESCE(t->e);
    HIPCHK(hipSetDevice(t->e->device));
    TreeRootArgs a;
    a.seed = seed;
    a.draw = draw;
    a.greedy = flags & 1;
    a.actions = d_actions;
    a.visits = d_visits;
    a.pi = d_pi;
    a.pick = d_pick;
    a.value = d_value;
    a.proof = (flags >> 1) & 1;
    if (t->vslab)
        k_tree_root_policy<true><<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, a, t->v);
    else
        k_tree_root_policy<false><<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, a, t->v);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gc_tree_pointers(gc_tree* t, void** out, int n) {
    if (!t || !out) return fail("null argument");
    if (n < 1) return fail("n must be >= 1");
    void* p[GC_TREE_ARRAYS];
    tree_addresses(t, p);
    for (int k = 0; k < n && k < GC_TREE_ARRAYS; k++) out[k] = p[k];
    return 0;
}

extern "C" int gc_tree_batch_reserve(gc_tree* t, int max_leaves) {
    if (!t) return fail("null tree");
    if (t->vslab) return fail(TREE_SOLVER_NO_BATCH);
    if (t->uslab) return fail(TREE_GUMBEL_NO_BATCH);
    if (max_leaves < 1 || max_leaves > 64) return fail("max_leaves must be in [1, 64]");
    if (t->pending) return fail("a selection is pending: gc_tree_backup first");
    if (t->batch_pending) return fail(TREE_BATCH_PENDING);
    if (t->bslab && t->b.K == max_leaves) return 0;
    gc_env* e = t->e;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    const TreeDev& d = t->d;
    size_t sz[GC_TREE_BATCH_ARRAYS], off[GC_TREE_BATCH_ARRAYS], total = 0;
    tree_batch_sizes((size_t)d.games, (size_t)d.nodes, (size_t)d.cap, (size_t)max_leaves, sz);
    for (int k = 0; k < GC_TREE_BATCH_ARRAYS; k++) {
        off[k] = total;
        total += (sz[k] + 255) & ~(size_t)255;
    }
    uint8_t* slab = nullptr;
    if (dalloc(&slab, total)) return -1;
    hipError_t rc = hipMemsetAsync(slab, 0, total, e->stream);
    if (rc != hipSuccess) {
        (void)hipFree(slab);
        return fail(std::string("hipMemsetAsync: ") + hipGetErrorString(rc));
    }
    if (t->bslab) {
        (void)hipFree(t->bslab);  // (waits for the device: no launch still uses the old scratch)
        t->bytes -= t->bbytes;
    }
    t->bslab = slab;
    t->bbytes = total;
    t->bytes += total;
    TreeBatchDev& b = t->b;
    b.inflight = slab + off[0];
    b.path = (int32_t*)(slab + off[1]);
    b.depth = (int32_t*)(slab + off[2]);
    b.leaf = (int32_t*)(slab + off[3]);
    b.kind = (int32_t*)(slab + off[4]);
    b.collisions = (int32_t*)(slab + off[5]);
    b.K = max_leaves;
    return 0;
}

extern "C" int gc_tree_select_batch(gc_tree* t, int leaves, float c_puct, float fpu, float vloss, int32_t* d_parent,
                                    int32_t* d_child, uint16_t* d_action) {
    if (!t) return fail("null tree");
    if (t->vslab) return fail(TREE_SOLVER_NO_BATCH);
    if (!d_parent || !d_child || !d_action) return fail("null output array");
    if (!t->bslab) return fail("no batch scratch: gc_tree_batch_reserve first");
    if (leaves < 1 || leaves > t->b.K) return fail("leaves must be in [1, the reserved max_leaves]");
    if (!std::isfinite(c_puct) || c_puct < 0.f) return fail("c_puct must be finite and >= 0");
    if (fpu != fpu) return fail("fpu is NaN");
    if (!std::isfinite(vloss) || vloss < 0.f) return fail("vloss must be finite and >= 0");
    if (t->pending) return fail("a selection is pending: gc_tree_backup first");
    if (t->batch_pending) return fail(TREE_BATCH_PENDING);
    SRV_QUIESCE(t->e);
    HIPCHK(hipSetDevice(t->e->device));
    k_tree_select_batch<<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, t->b, leaves, c_puct, fpu, vloss,
                                                                                  d_parent, d_child, d_action);
    HIPCHK(hipGetLastError());
    t->batch_pending = leaves;
    return 0;
}

extern "C" int gc_tree_backup_batch(gc_tree* t, const float* d_value, const uint8_t* d_done, const uint8_t* d_reason,
                                    const uint16_t* d_actions, const float* d_priors, const int32_t* d_count,
                                    int pri_cap) {
    if (!t) return fail("null tree");
    if (t->vslab) return fail(TREE_SOLVER_NO_BATCH);
    if (!d_value || !d_done || !d_reason) return fail("null value / done / reason array");
    if (!d_actions || !d_priors || !d_count) return fail("null priors block");
    if (pri_cap < 1) return fail("pri_cap must be >= 1");
    if (t->pending) return fail("a selection is pending: gc_tree_backup first");
    if (!t->batch_pending) return fail("no batch is pending: gc_tree_select_batch first");
    SRV_QUIESCE(t->e);
    HIPCHK(hipSetDevice(t->e->device));
    const TreePriors p{d_actions, d_priors, d_count, pri_cap};
    k_tree_backup_batch<<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, t->b, t->batch_pending, d_value,
                                                                                  d_done, d_reason, p);
    HIPCHK(hipGetLastError());
    t->batch_pending = 0;
    return 0;
}

extern "C" int gc_tree_batch_pointers(gc_tree* t, void** out, int n) {
    if (!t || !out) return fail("null argument");
    if (n < 1) return fail("n must be >= 1");
    if (!t->bslab) return fail("no batch scratch: gc_tree_batch_reserve first");
    const TreeBatchDev& b = t->b;
    void* p[GC_TREE_BATCH_ARRAYS] = {b.inflight, b.path, b.depth, b.leaf, b.kind, b.collisions};
    for (int k = 0; k < n && k < GC_TREE_BATCH_ARRAYS; k++) out[k] = p[k];
    return 0;
}

extern "C" int gc_tree_solver_enable(gc_tree* t) {
    if (!t) return fail("null tree");
    if (t->vslab) return 0;
    if (t->pending) return fail("a selection is pending: gc_tree_backup first");
    if (t->batch_pending) return fail(TREE_BATCH_PENDING);
    if (t->bslab) return fail("a batch scratch is reserved: the batch calls are not defined for a solver tree yet");
    if (t->uslab) return fail(TREE_GUMBEL_NO_SOLVER);
    gc_env* e = t->e;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    const TreeDev& d = t->d;
    size_t sz[GC_TREE_SOLVER_ARRAYS], off[GC_TREE_SOLVER_ARRAYS], total = 0;
    tree_solver_sizes((size_t)d.games, (size_t)d.nodes, (size_t)d.cap, sz);
    for (int k = 0; k < GC_TREE_SOLVER_ARRAYS; k++) {
        off[k] = total;
        total += (sz[k] + 255) & ~(size_t)255;
    }
    uint8_t* slab = nullptr;
    if (dalloc(&slab, total)) return -1;
    hipError_t rc = hipMemsetAsync(slab, 0, total, e->stream);
    if (rc != hipSuccess) {
        (void)hipFree(slab);
        return fail(std::string("hipMemsetAsync: ") + hipGetErrorString(rc));
    }
    t->vslab = slab;
    t->bytes += total;
    TreeSolverDev& v = t->v;
    v.edge_proven = slab + off[0];
    v.edge_plies = (uint16_t*)(slab + off[1]);
    v.node_proven = slab + off[2];
    v.node_plies = (uint16_t*)(slab + off[3]);
    v.complete = slab + off[4];
    return 0;
}

extern "C" int gc_tree_solver_pointers(gc_tree* t, void** out, int n) {
    if (!t || !out) return fail("null argument");
    if (n < 1) return fail("n must be >= 1");
    if (!t->vslab) return fail("no solver: gc_tree_solver_enable first");
    const TreeSolverDev& v = t->v;
    void* p[GC_TREE_SOLVER_ARRAYS] = {v.edge_proven, v.edge_plies, v.node_proven, v.node_plies, v.complete};
    for (int k = 0; k < n && k < GC_TREE_SOLVER_ARRAYS; k++) out[k] = p[k];
    return 0;
}

extern "C" int gc_tree_root_proof(gc_tree* t, uint8_t* d_status, uint16_t* d_plies, uint16_t* d_move) {
    if (!t) return fail("null tree");
    if (!t->vslab) return fail("no solver: gc_tree_solver_enable first");
    if (t->pending) return fail("a selection is pending: gc_tree_backup first");
    SRV_QUIESCE(t->e);
    HIPCHK(hipSetDevice(t->e->device));
    k_tree_root_proof<<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, t->v, d_status, d_plies, d_move);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gc_tree_gumbel_enable(gc_tree* t, int considered, int sims, float c_visit, float c_scale) {
    if (!t) return fail("null tree");
    if (considered < 1 || considered > t->d.cap) return fail("gumbel: considered must be in [1, cap]");
    if (sims < 1 || sims > 65535) return fail("gumbel: sims must be in [1, 65535]");
    if (!std::isfinite(c_visit) || c_visit < 0.f) return fail("gumbel: c_visit must be finite and >= 0");
    if (!std::isfinite(c_scale) || !(c_scale > 0.f)) return fail("gumbel: c_scale must be finite and > 0");
    if (t->pending) return fail("gumbel: a selection is pending: gc_tree_backup first");
    if (t->batch_pending) return fail(TREE_BATCH_PENDING);
    if (t->vslab) return fail("gumbel: the tree has the solver enabled: the two together are not defined yet");
    if (t->bslab) return fail("gumbel: a batch scratch is reserved: the batch calls are not defined for a gumbel tree yet");
    TreeGumbelDev& u = t->u;
    if (t->uslab && u.considered == considered && u.sims == sims && u.c_visit == c_visit && u.c_scale == c_scale)
        return 0;
    gc_env* e = t->e;
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    const TreeDev& d = t->d;
    size_t sz[GC_TREE_GUMBEL_ARRAYS], off[GC_TREE_GUMBEL_ARRAYS], total = 0;
    tree_gumbel_sizes((size_t)d.games, (size_t)d.cap, (size_t)considered, (size_t)sims, sz);
    for (int k = 0; k < GC_TREE_GUMBEL_ARRAYS; k++) {
        off[k] = total;
        total += (sz[k] + 255) & ~(size_t)255;
    }
    uint8_t* slab = nullptr;
    if (dalloc(&slab, total)) return -1;
    const std::vector<uint16_t> table = tree_gumbel_table(considered, sims);
    hipError_t rc = hipMemsetAsync(slab, 0, total, e->stream);
    if (rc == hipSuccess) rc = hipMemcpyAsync(slab + off[3], table.data(), sz[3], hipMemcpyHostToDevice, e->stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(e->stream);  // (the host table lives until here)
    if (rc != hipSuccess) {
        (void)hipFree(slab);
        return fail(std::string("gumbel: the arrays' upload: ") + hipGetErrorString(rc));
    }
    if (t->uslab) {
        (void)hipFree(t->uslab);  // (waits for the device: no launch still uses the old arrays)
        t->bytes -= t->ubytes;
    }
    t->uslab = slab;
    t->ubytes = total;
    t->bytes += total;
    t->armed = false;
    u.gumbel = (float*)(slab + off[0]);
    u.logit = (float*)(slab + off[1]);
    u.base_visits = (int32_t*)(slab + off[2]);
    u.table = (const uint16_t*)(slab + off[3]);
    u.considered = considered;
    u.sims = sims;
    u.c_visit = c_visit;
    u.c_scale = c_scale;
    return 0;
}

extern "C" int gc_tree_gumbel_begin(gc_tree* t, uint64_t seed, uint32_t draw) {
    if (!t) return fail("null tree");
    if (!t->uslab) return fail("no gumbel search: gc_tree_gumbel_enable first");
    if (t->pending) return fail("a selection is pending: gc_tree_backup first");
    SRV_QUIESCE(t->e);
    HIPCHK(hipSetDevice(t->e->device));
    k_tree_gumbel_begin<<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, t->u, seed, draw);
    HIPCHK(hipGetLastError());
    t->armed = true;
    return 0;
}

extern "C" int gc_tree_gumbel_policy(gc_tree* t, uint16_t* d_actions, int32_t* d_visits, float* d_pi,
                                     int32_t* d_target, uint16_t* d_pick, float* d_value) {
    if (!t) return fail("null tree");
    if (!t->uslab) return fail("no gumbel search: gc_tree_gumbel_enable first");
    if (!t->armed) return fail("the gumbel search is not armed: gc_tree_gumbel_begin first (reset and advance disarm)");
    if (t->pending) return fail("a selection is pending: gc_tree_backup first");
    SRV_QUIESCE(t->e);
    HIPCHK(hipSetDevice(t->e->device));
    const TreeGumbelOut a{d_actions, d_visits, d_pi, d_target, d_pick, d_value};
    k_tree_gumbel_policy<<<tree_grid(t), dim3(64 * TREE_WAVES), 0, t->e->stream>>>(t->d, t->u, a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gc_tree_gumbel_pointers(gc_tree* t, void** out, int n) {
    if (!t || !out) return fail("null argument");
    if (n < 1) return fail("n must be >= 1");
    if (!t->uslab) return fail("no gumbel search: gc_tree_gumbel_enable first");
    const TreeGumbelDev& u = t->u;
    void* p[GC_TREE_GUMBEL_ARRAYS] = {u.gumbel, u.logit, u.base_visits, (void*)u.table};
    for (int k = 0; k < n && k < GC_TREE_GUMBEL_ARRAYS; k++) out[k] = p[k];
    return 0;
}

extern "C" uint64_t gc_tree_device_bytes(gc_tree* t) { return t ? (uint64_t)t->bytes : 0; }
