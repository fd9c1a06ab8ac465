// gc_host_perft.h -- the perft host driver and gc_engine_perft.
#pragma once

// depth-3 subtrees as depth-2 ones: the level below `leaf` is materialised chunk by chunk
// (it is ~30x larger) and its nodes run in order of their move counts, so the leaf kernel's
// one remaining loop has (nearly) equal trip counts across a wave -- with depth-3 subtrees
// the inner loop's trip count varied per lane (PMC: ~60 % lane utilisation).
// leaf-kernel time of the split pass (gc_perft_leaf_stats): HIP events around every
// leaf launch (k_perft2_val / k_perft2_rec), on the stream it runs on; summed once the pass has synchronised
static std::mutex g_leaf_mu;
static uint64_t g_leaf_launches = 0, g_leaf_subtrees = 0, g_leaf_records = 0;
static double g_leaf_ms = 0.0;

static int perft_split_leaves(hipStream_t st, SoA leaf, uint64_t* leaf_out) {
    // parents per chunk 2^21 and up to 2^27 children (7.5 GiB of boards); GC_PERFT_CHUNK=k
    // (A/B): 2^k parents, 2^(k+6) children (2^20 / 2^22 measured 1.92 / 1.83 vs 1.93e12)
    static const int chunk_log2 = getenv("GC_PERFT_CHUNK") ? atoi(getenv("GC_PERFT_CHUNK")) : 21;
    // (the lead word holds a sorted position in RUN_LEN_SHIFT bits)
    if (chunk_log2 < 10 || chunk_log2 + 6 > RUN_LEN_SHIFT)
        return fail("GC_PERFT_CHUNK must be in [10, 21] (2^k parents per chunk)");
    const int64_t cap = (int64_t)1 << (chunk_log2 + 6);
    int chunk = 1 << chunk_log2;
    Temps tmps;  // the buffers below, and event pairs around the leaf launches
    uint64_t subtrees = 0, records = 0;  // subtrees counted by the leaf kernel, of records made
    // GC_PERFT_DEDUP=0 (per call; tests): every record counted, transpositions too
    const char* dd = getenv("GC_PERFT_DEDUP");
    const bool dedup = !(dd && dd[0] == '0');
    int32_t *kc = nullptr, *offs = nullptr;
    uint8_t* bins = nullptr;
    u32 *hist = nullptr, *hbase = nullptr;
    const int max_blk = (chunk + BLOCK - 1) / BLOCK;
    const int max_dblk = (int)((cap + DEDUP_BLOCK * DEDUP_R - 1) / (DEDUP_BLOCK * DEDUP_R));  // the histograms' blocks
    const int hist_n = SPLIT_BINS * (dedup && max_dblk > max_blk ? max_dblk : max_blk);
    Node64* cr = nullptr;
    // the transposition pass: the records in expansion order; the sort's keys / values (16 B per
    // record), reused after it for the members' (leader, parent) pairs; the lead words; the
    // placed leaders' sorted positions
    Node64* cre = nullptr;
    u32* kv = nullptr;
    u32* leadw = nullptr;
    u32* spos = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    int rc = 0;
    std::string err;
    if (tmps.alloc(&kc, leaf.n) || tmps.alloc(&offs, chunk) || tmps.alloc(&cr, cap) || tmps.alloc(&bins, cap) ||
        tmps.alloc(&hist, (size_t)hist_n) || tmps.alloc(&hbase, (size_t)hist_n) ||
        (dedup && (tmps.alloc(&cre, cap) || tmps.alloc(&kv, 4 * cap) || tmps.alloc(&leadw, cap) || tmps.alloc(&spos, cap))))
        return -1;
    {  // scratch for the largest scan and sort of a chunk
        size_t b1 = 0, b2 = 0, b3 = 0;
        hipError_t he = hipcub::DeviceScan::ExclusiveSum(nullptr, b1, kc, offs, chunk, st);
        if (he == hipSuccess) he = hipcub::DeviceScan::ExclusiveSum(nullptr, b2, hist, hbase, hist_n, st);
        if (he == hipSuccess && dedup)
            he = hipcub::DeviceRadixSort::SortPairs(nullptr, b3, kv, kv + cap, kv + 2 * cap, kv + 3 * cap, (int)cap, 0, 32, st);
        tmp_bytes = b1 > b2 ? b1 : b2;
        tmp_bytes = tmp_bytes > b3 ? tmp_bytes : b3;
        if (he != hipSuccess) return fail(std::string("perft split: ") + hipGetErrorString(he));
        if (tmps.alloc((char**)&tmp, tmp_bytes)) return -1;
    }
    k_count_children<int32_t><<<grid_for(leaf.n), BLOCK, 0, st>>>(leaf, kc);
    for (int a = 0; a < leaf.n && rc == 0;) {
        int c = leaf.n - a < chunk ? leaf.n - a : chunk;
        size_t tb = tmp_bytes;
        hipError_t he = hipcub::DeviceScan::ExclusiveSum(tmp, tb, kc + a, offs, c, st);
        int32_t lo = 0, lc = 0;
        if (he == hipSuccess) he = hipMemcpyAsync(&lo, offs + c - 1, 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(&lc, kc + a + c - 1, 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) { err = std::string("perft split: ") + hipGetErrorString(he); rc = -1; break; }
        int64_t total = (int64_t)lo + lc;
        if (total > cap) { chunk /= 2; continue; }  // an unusually bushy chunk: halve and retry
        he = hipMemsetAsync(leaf_out + a, 0, (size_t)8 * c, st);  // the parents' sums
        if (he != hipSuccess) { err = std::string("perft split: ") + hipGetErrorString(he); rc = -1; break; }
        unsigned long long* psum = reinterpret_cast<unsigned long long*>(leaf_out + a);
        if (total > 0 && dedup) {  // transpositions merged, the leaders binned and placed in order
            const int n = (int)total;
            const int nbd = (n + DEDUP_BLOCK * DEDUP_R - 1) / (DEDUP_BLOCK * DEDUP_R);
            k_expand_range_rec<<<grid_for(c), BLOCK, 0, st>>>(leaf, a, c, offs, cre);
            u32* const keys = kv;
            u32* const vals = kv + cap;
            u32* const keys2 = kv + 2 * cap;
            u32* const vals2 = kv + 3 * cap;
            uint2* const fw = reinterpret_cast<uint2*>(kv);  // after the sort: over keys | vals
            k_dedup_keys<<<grid_for(n), BLOCK, 0, st>>>(cre, n, keys, vals, bins);
            tb = tmp_bytes;
            he = hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys, keys2, vals, vals2, n, 0, 32, st);
            if (he == hipSuccess) he = hipMemsetAsync(leadw, 0, (size_t)4 * n, st);
            if (he == hipSuccess) k_dedup_runs_f<<<grid_for(n), BLOCK, 0, st>>>(cre, n, keys2, vals2, leadw, fw);
            if (he == hipSuccess) k_leader_hist_f<<<nbd, DEDUP_BLOCK, 0, st>>>(n, leadw, bins, hist, nbd);
            tb = tmp_bytes;
            if (he == hipSuccess) he = hipcub::DeviceScan::ExclusiveSum(tmp, tb, hist, hbase, SPLIT_BINS * nbd, st);
            u32 hb = 0, hl = 0;  // the leaders: the last bin's base + its last block's count
            const size_t last = (size_t)SPLIT_BINS * nbd - 1;
            if (he == hipSuccess) he = hipMemcpyAsync(&hb, hbase + last, 4, hipMemcpyDeviceToHost, st);
            if (he == hipSuccess) he = hipMemcpyAsync(&hl, hist + last, 4, hipMemcpyDeviceToHost, st);
            if (he == hipSuccess) k_place_leaders_f<<<nbd, DEDUP_BLOCK, 0, st>>>(cre, n, bins, leadw, hbase, nbd, cr, spos);
            if (he == hipSuccess) he = hipStreamSynchronize(st);  // the leaf grid sized to the leaders
            if (he != hipSuccess) { err = std::string("perft split dedup: ") + hipGetErrorString(he); rc = -1; break; }
            const int lead_n = (int)(hb + hl);
            const hipEvent_t e0 = tmps.event(), e1 = tmps.event();
            if (e0 && e1) (void)hipEventRecord(e0, st);
            k_perft2_val<<<grid_for(lead_n), BLOCK, 0, st>>>(cr, lead_n, psum, n, keys2, fw, spos);
            if (e0 && e1) (void)hipEventRecord(e1, st);
            records += (uint64_t)total;
            subtrees += (uint64_t)lead_n;
        } else if (total > 0) {  // every record, in move-count order, then read in order
            const int nb = grid_for(c);
            k_expand_count<<<nb, BLOCK, 0, st>>>(leaf, a, c, bins, offs, hist, nb);
            tb = tmp_bytes;
            he = hipcub::DeviceScan::ExclusiveSum(tmp, tb, hist, hbase, SPLIT_BINS * nb, st);
            if (he != hipSuccess) { err = std::string("perft split scan: ") + hipGetErrorString(he); rc = -1; break; }
            k_expand_place<<<nb, BLOCK, 0, st>>>(leaf, a, c, bins, offs, hbase, nb, cr);
            const hipEvent_t e0 = tmps.event(), e1 = tmps.event();
            if (e0 && e1) (void)hipEventRecord(e0, st);
            k_perft2_rec<<<grid_for((int)total), BLOCK, 0, st>>>(cr, (int)total, psum);
            if (e0 && e1) (void)hipEventRecord(e1, st);
            records += (uint64_t)total;
            subtrees += (uint64_t)total;
        }
        he = hipGetLastError();
        if (he != hipSuccess) { err = std::string("perft split kernels: ") + hipGetErrorString(he); rc = -1; break; }
        a += c;
    }
    hipError_t he = hipStreamSynchronize(st);  // before the buffers are freed
    if (rc == 0 && he != hipSuccess) { err = std::string("perft split: ") + hipGetErrorString(he); rc = -1; }
    if (rc == 0) {
        const std::vector<hipEvent_t>& evs = tmps.events();
        double ms = 0.0;
        for (size_t k = 0; k + 1 < evs.size(); k += 2) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, evs[k], evs[k + 1]) == hipSuccess) ms += t;
        }
        std::lock_guard<std::mutex> lk(g_leaf_mu);
        g_leaf_launches += evs.size() / 2;
        g_leaf_subtrees += subtrees;
        g_leaf_records += records;
        g_leaf_ms += ms;
    }
    return rc ? fail(err) : 0;
}

// which leaf pass ran, per pass (gc_perft_path_counts): tests assert that a configuration
// takes the path it is meant to pin
static std::atomic<unsigned long long> g_perft_path[4];  // split, sorted, small, fide

// Leaf level: perft(node, rem) of every node of `leaf` (rem <= 3, or few nodes) into out.
static int perft_leaf(hipStream_t st, SoA ls, int rem, uint64_t* out, int fide) {
    if (ls.n == 0) return 0;
    const char* sp = getenv("GC_PERFT_SPLIT");  // per call: tests compare both paths
    if (!fide && rem == 3 && ls.n >= 65536 && !(sp && sp[0] == '0')) {
        g_perft_path[0]++;
        return perft_split_leaves(st, ls, out);
    }
    if (!fide && rem >= 2 && ls.n >= 65536) {  // subtrees by root move count
        Temps tmps;
        int32_t *kc = nullptr, *ks = nullptr, *ix = nullptr, *is = nullptr;
        void* tmp = nullptr;
        size_t tb = 0;
        hipError_t he = hipSuccess;
        if (tmps.alloc(&kc, ls.n) || tmps.alloc(&ks, ls.n) || tmps.alloc(&ix, ls.n) || tmps.alloc(&is, ls.n)) he = hipErrorOutOfMemory;
        if (he == hipSuccess) {
            k_count_children<int32_t><<<grid_for(ls.n), BLOCK, 0, st>>>(ls, kc);
            k_iota<<<grid_for(ls.n), BLOCK, 0, st>>>(ix, ls.n);
            he = hipcub::DeviceRadixSort::SortPairs(nullptr, tb, kc, ks, ix, is, ls.n, 0, 10, st);
        }
        if (he == hipSuccess && tmps.alloc((char**)&tmp, tb) == 0)
            he = hipcub::DeviceRadixSort::SortPairs(tmp, tb, kc, ks, ix, is, ls.n, 0, 10, st);
        bool ok = he == hipSuccess && tmp;
        if (ok) {
            k_perft_small_perm<<<grid_for(ls.n), BLOCK, 0, st>>>(ls, is, rem, out);
            he = hipStreamSynchronize(st);  // before the temporaries are freed
        }
        if (he != hipSuccess) return fail(std::string("perft sort: ") + hipGetErrorString(he));
        if (ok) { g_perft_path[1]++; return 0; }
    }
    g_perft_path[fide ? 3 : 2]++;
    if (fide) k_fperft_small<<<grid_for(ls.n), BLOCK, 0, st>>>(ls, rem, out);
    else k_perft_small<<<grid_for(ls.n), BLOCK, 0, st>>>(ls, rem, out);
    return 0;
}

// Children materialised per chunk of parents: <= PERFT_LEVEL_CAP nodes (60 B each plus
// 24 B of counts / offsets / values, ~11 GiB at 2^27) so any depth fits HBM; the split-leaf
// pass below holds its own <= 2^27-child chunk.  GC_PERFT_LEVEL_CAP (per call) lowers it so
// tests drive the chunked path at small sizes.
static const int64_t PERFT_LEVEL_CAP = (int64_t)1 << 27;

// out[i] = perft(nodes[i], rem).  While more than 3 plies remain, or while there are too few
// subtrees to fill the chip, the nodes are expanded into their children on the device
// (count, exclusive scan in 64 bits, write) and the children recursed on, one chunk of
// parents at a time when the level would not fit; the parents' values are the sums of their
// children's.  Sizes are 64-bit throughout: a level's child total may pass 2^31.
static int perft_nodes(hipStream_t st, SoA nodes, int rem, uint64_t* out, int fide) {
    if (nodes.n == 0) return 0;
    if (!(rem > 3 || (rem >= 2 && nodes.n < 131072))) return perft_leaf(st, nodes, rem, out, fide);
    int64_t cap = PERFT_LEVEL_CAP;
    if (const char* e = getenv("GC_PERFT_LEVEL_CAP")) cap = atoll(e) > 0 ? atoll(e) : cap;
    const int n = nodes.n;
    int64_t *cnt = nullptr, *offs = nullptr;
    u64* cb = nullptr;
    u32* cm = nullptr;
    uint64_t* cval = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    int64_t held = 0;  // children the buffers below can hold
    std::string err;
    Temps tmps(st);  // (drained first: nothing in flight may still use the buffers)
    if (tmps.alloc(&cnt, n) || tmps.alloc(&offs, n)) return -1;
    if (fide) k_fcount_children<<<grid_for(n), BLOCK, 0, st>>>(nodes, cnt);
    else k_count_children<int64_t><<<grid_for(n), BLOCK, 0, st>>>(nodes, cnt);
    hipError_t he = hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt, offs, n, st);
    if (he != hipSuccess) return fail(std::string("perft scan: ") + hipGetErrorString(he));
    if (tmps.alloc((char**)&tmp, tmp_bytes ? tmp_bytes : 1)) return -1;
    int chunk = n;
    for (int a = 0; a < n;) {
        const int c = n - a < chunk ? n - a : chunk;
        size_t tb = tmp_bytes;
        int64_t lo = 0, lc = 0;
        he = hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt + a, offs, c, st);
        if (he == hipSuccess) he = hipMemcpyAsync(&lo, offs + c - 1, 8, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(&lc, cnt + a + c - 1, 8, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) { err = std::string("perft scan: ") + hipGetErrorString(he); break; }
        const int64_t total = lo + lc;
        if (total > cap && c > 1) { chunk = (c + 1) / 2; continue; }  // halve the chunk and rescan
        if (total >= ((int64_t)1 << 31)) { err = "perft: one node has too many children"; break; }
        if (total > held) {  // (re)allocate the child buffers for this chunk
            (void)hipStreamSynchronize(st);
            tmps.drop(cb); tmps.drop(cm); tmps.drop(cval);
            held = 0;
            if (tmps.alloc(&cb, (size_t)NBB * total) || tmps.alloc(&cm, total) || tmps.alloc(&cval, total)) { err = g_err; break; }
            held = total;
        }
        if (total > 0) {
            SoA ch{cb, cm, (int)total};
            if (fide) k_fexpand_range<<<grid_for(c), BLOCK, 0, st>>>(nodes, a, c, offs, ch);
            else k_expand_range<int64_t><<<grid_for(c), BLOCK, 0, st>>>(nodes, a, c, offs, ch);
            he = hipGetLastError();
            if (he != hipSuccess) { err = std::string("perft expand: ") + hipGetErrorString(he); break; }
            if (perft_nodes(st, ch, rem - 1, cval, fide)) { err = g_err; break; }
        }
        k_sum_children<int64_t><<<grid_for(c), BLOCK, 0, st>>>(offs, cnt + a, cval, c, out + a);
        he = hipGetLastError();
        if (he != hipSuccess) { err = std::string("perft sum: ") + hipGetErrorString(he); break; }
        a += c;
    }
    return err.empty() ? 0 : fail(err);
}

// perft over n roots (side to move = meta[0])
static int perft_device(hipStream_t st, SoA roots, int depth, uint64_t* d_out, int fide) {
    if (perft_nodes(st, roots, depth, d_out, fide)) return -1;
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return fail(std::string("perft kernels: ") + hipGetErrorString(he));
    return 0;
}

extern "C" int gc_perft_path_counts(uint64_t* out4) {
    if (!out4) return fail("null argument");
    for (int k = 0; k < 4; k++) out4[k] = g_perft_path[k].load();
    return 0;
}

extern "C" int gc_perft_leaf_stats(uint64_t* launches, uint64_t* subtrees, double* kernel_ms) {
    if (!launches || !subtrees || !kernel_ms) return fail("null argument");
    std::lock_guard<std::mutex> lk(g_leaf_mu);
    *launches = g_leaf_launches;
    *subtrees = g_leaf_subtrees;
    *kernel_ms = g_leaf_ms;
    return 0;
}

extern "C" int gc_perft_dedup_stats(uint64_t* records, uint64_t* counted) {
    if (!records || !counted) return fail("null argument");
    std::lock_guard<std::mutex> lk(g_leaf_mu);
    *records = g_leaf_records;
    *counted = g_leaf_subtrees;
    return 0;
}

extern "C" int gc_engine_perft(gc_engine* e, int n, const int8_t* boards, const uint8_t* meta, int depth,
                               uint64_t* nodes) {
    if (!e || !nodes) return fail("null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (depth < 0 || depth > PERFT_MAXD) return fail("depth must be in [0, 8]");
    if (devsrv_quiesce(e->device) || engine_reserve(e, n, 1)) return -1;
    EngineLayout o;
    if (engine_begin(e, n, boards, meta, nullptr, nullptr, 1, false, o)) return -1;
    if (perft_device(e->stream, SoA{e->bb, e->meta, n}, depth, e->u64o, e->rules)) return -1;
    HIPCHK(hipMemcpyAsync(nodes, e->u64o, (size_t)8 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}
