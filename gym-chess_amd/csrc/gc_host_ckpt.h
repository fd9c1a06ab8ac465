// gc_host_ckpt.h -- env checkpoints: kernels and host code.
#pragma once

// ----------------------------------------------------------------------------- checkpoint
// Bit-exact save / restore of a whole env (SURVEY.md §5 "save/load = memcpy of state +
// repetition history"; the reference keeps its history in ChessEnvV2.saved_boards,
// chess_v2.py:192, 404-407, beside the state dict, 301-323).  Blob layout (version 2):
//   CkptHeader | slab (Slab::BYTES_PER_BOARD * n: bitboards, meta, window generation, Philox
//   draw counter, step counter, last outputs, next action) | spill counts u32[n] (live spill
//   entries per board, zero unless a BLACK agent's window spilled) | the live window-table
//   entries, board by board (hl_of(meta[i]) entries of 8 u64: header {tag | count << 56}, 7
//   bitboards) | the live spill entries, board by board (8 u64: count, 7 bitboards).
// Only live entries travel: restoring re-inserts them under a fresh generation, so a restored
// board answers every later probe exactly as before (same boards, same counts; slot positions
// may differ, which no result depends on).  The header pins the slab's field layout
// (CKPT_LAYOUT); a blob whose windows do not fit the env's tables is refused before anything
// of the env changes.
struct CkptHeader {
    char magic[8];  // "GCCKPT2"
    uint32_t version, n, rules, opp, agent_black, policy_ready;
    uint64_t seed;
    uint64_t init[NBB];  // the env's initial board (resets land on it)
    uint64_t entries;        // window-table entries
    uint64_t spill_entries;  // spill-table entries
    uint64_t layout;         // CKPT_LAYOUT of the writer
};
static const char CKPT_MAGIC[8] = {'G', 'C', 'C', 'K', 'P', 'T', '2', 0};
// the slab's size and field offsets per board (a writer with another layout is refused)
static constexpr uint64_t CKPT_LAYOUT = (uint64_t)Slab::BYTES_PER_BOARD | (56ull << 8) | (60ull << 16) | (64ull << 24) |
                                        (68ull << 32) | (72ull << 40) | (76ull << 48) | (78ull << 56);
static_assert(Slab::BYTES_PER_BOARD == 80, "update CKPT_LAYOUT with the slab");

__global__ void k_hl_of(const u32* __restrict__ meta, int n, uint32_t* __restrict__ hl) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hl[i] = hl_of(meta[i]);
}

// the live entries (generation == hgen[i]) of board i, in table order, at out[offs[i]..]
__global__ void k_ckpt_pack(const u64* __restrict__ htab, const u32* __restrict__ hgen, const u32* __restrict__ meta,
                            int n, int nb, const uint32_t* __restrict__ offs, u64* __restrict__ out,
                            uint32_t* __restrict__ bad) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DevHist h{const_cast<u64*>(htab), const_cast<u32*>(hgen), hgen[i], i, nb};
    const u32 g = h.gen(), hl = hl_of(meta[i]);
    u32 k = 0;
    u64* o = out + (size_t)offs[i] * 8;
    for (int pos = 0; pos < (1 << nb); pos++) {
        const u64* e = htab + h.entry(pos) * 8;
        u64 hdr = e[0];
        if ((u32)hdr != g) continue;
        if (k < hl) {
            u64* d = o + (size_t)k * 8;
            d[0] = hdr & ~0xFFFFFFFFull;  // tag | count; the generation is re-issued on restore
#pragma unroll
            for (int j = 1; j < 8; j++) d[j] = e[j];
        }
        k++;
    }
    if (k != hl) atomicOr(bad, 1u);
}

// live spill entries per board (cnt zeroed by the caller); with out: packed at
// out[offs[owner] + fill[owner]++] as {count, 7 bitboards}
__global__ void k_spill_collect(const u64* __restrict__ ent, u32 mask, const u32* __restrict__ hgen,
                                uint32_t* __restrict__ cnt, const uint32_t* __restrict__ offs, u64* __restrict__ out) {
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot > mask) return;
    const u64* e = ent + slot * 8;
    const u64 hdr = e[0];
    const u32 o1 = sp_owner1(hdr);
    if (o1 == 0 || sp_gen(hdr) != hgen[o1 - 1]) return;
    const u32 k = atomicAdd(cnt + (o1 - 1), 1u);
    if (!out) return;
    u64* d = out + ((size_t)offs[o1 - 1] + k) * 8;
    d[0] = sp_cnt(hdr);
#pragma unroll
    for (int j = 1; j < 8; j++) d[j] = e[j];
}

// fresh generation per board: above both the live table's and the saved one, so no entry of
// the live table can pass for a restored one
__global__ void k_ckpt_gen(const u32* __restrict__ live_hgen, const u32* __restrict__ saved_hgen, int n,
                           uint32_t* __restrict__ gnew) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) gnew[i] = (live_hgen[i] > saved_hgen[i] ? live_hgen[i] : saved_hgen[i]) + 1u;
}

// refuse a blob whose windows do not fit the env's tables (before the env changes): a window
// longer than hist_cap, or spill entries without a full table or without a spill table
__global__ void k_ckpt_check(const u32* __restrict__ meta, const uint32_t* __restrict__ scnt, int n, int nb, int spill,
                             uint32_t* __restrict__ bad) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int hl = (int)hl_of(meta[i]);
    if (hl > hist_cap(nb)) atomicOr(bad, 1u);
    if (scnt[i] && (!spill || hl < hist_cap(nb))) atomicOr(bad, 2u);
}

// board i takes generation gnew[i] and its saved entries are inserted by the probe rule of
// rep_commit (gc_env.h): home slot = key & (HTAB-1), linear probing; its spill entries by
// spill_insert's
__global__ void k_ckpt_unpack(u64* __restrict__ htab, u32* __restrict__ hgen, const u32* __restrict__ meta, int n,
                              int nb, const uint32_t* __restrict__ gnew, const uint32_t* __restrict__ offs,
                              const u64* __restrict__ in, SpillTab sp, const uint32_t* __restrict__ scnt,
                              const uint32_t* __restrict__ soffs, const u64* __restrict__ sin, uint32_t* __restrict__ bad) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 g = gnew[i];
    hgen[i] = g;
    DevHist h{htab, hgen, g, i, nb};
    h.sp = sp;
    const u32 hl = hl_of(meta[i]);
    const int size = 1 << nb;
    for (u32 k = 0; k < hl; k++) {
        const u64* e = in + ((size_t)offs[i] + k) * 8;
        Pos b = {e[1], e[2], e[3], e[4], e[5], e[6], e[7], 0};
        u32 key = board_key(b);
        u32 pos = key & (size - 1), tag = key >> nb;
        int probe = 0;
        while ((u32)htab[h.entry((int)pos) * 8] == g && probe < size) { pos = (pos + 1) & (size - 1); probe++; }
        if (probe == size) { atomicOr(bad, 2u); return; }
        u64* d = htab + h.entry((int)pos) * 8;
        d[0] = (u64)g | ((u64)tag << 32) | (e[0] & (0xFFull << 56));
#pragma unroll
        for (int j = 1; j < 8; j++) d[j] = e[j];
    }
    for (u32 k = 0; k < (scnt ? scnt[i] : 0u); k++) {
        const u64* e = sin + ((size_t)soffs[i] + k) * 8;
        Pos b = {e[1], e[2], e[3], e[4], e[5], e[6], e[7], 0};
        if (!spill_insert(h, b, board_key(b))) { atomicOr(bad, 4u); return; }
        u32 t = sp_home(board_key(b), (u32)i, sp.mask);  // the entry just inserted: set its count
        for (int probe = 0; probe < SPILL_PROBES; probe++, t = (t + 1) & sp.mask) {
            const u64 x = h.sp_hdr(t);
            if (sp_owner1(x) == (u32)i + 1 && sp_gen(x) == g && h.sp_same(t, b)) {
                h.sp_set_hdr(t, sp_make((u32)i, g, (u32)e[0]));
                break;
            }
        }
    }
}

// exclusive scan of v (n entries) -> offs; returns the total
static int scan_u32(gc_env* e, const uint32_t* v, uint32_t* offs, int n, uint64_t* total) {
    Temps tmps;
    size_t tb = 0;
    void* tmp = nullptr;
    hipError_t he = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, v, offs, n, e->stream);
    if (he == hipSuccess && tmps.alloc((char**)&tmp, tb ? tb : 1)) return -1;
    if (he == hipSuccess) he = hipcub::DeviceScan::ExclusiveSum(tmp, tb, v, offs, n, e->stream);
    uint32_t lo = 0, lc = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&lo, offs + n - 1, 4, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(&lc, v + n - 1, 4, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess) return fail(std::string("checkpoint scan: ") + hipGetErrorString(he));
    *total = (uint64_t)lo + lc;
    return 0;
}

// exclusive scan of the window lengths of `meta` (the saved or live slab's) -> offs; returns
// the total entry count
static int ckpt_offsets(gc_env* e, const u32* meta, uint32_t* hl, uint32_t* offs, uint64_t* total) {
    k_hl_of<<<grid_for(e->n), BLOCK, 0, e->stream>>>(meta, e->n, hl);
    return scan_u32(e, hl, offs, e->n, total);
}

// live spill entries per board (scnt) and their offsets (soffs); total
static int spill_offsets(gc_env* e, uint32_t* scnt, uint32_t* soffs, uint64_t* total) {
    HIPCHK(hipMemsetAsync(scnt, 0, (size_t)4 * e->n, e->stream));
    const SpillTab& sp = e->d.ic.spill;
    if (sp.ent) {
        const size_t slots = (size_t)sp.mask + 1;
        k_spill_collect<<<grid_for_slots(slots), BLOCK, 0, e->stream>>>(sp.ent, sp.mask, e->d.hgen, scnt,
                                                                                          nullptr, nullptr);
        HIPCHK(hipGetLastError());
    }
    return scan_u32(e, scnt, soffs, e->n, total);
}

static size_t ckpt_bytes(int n, uint64_t entries, uint64_t spill_entries) {
    return sizeof(CkptHeader) + (Slab::BYTES_PER_BOARD + 4) * (size_t)n + 64 * (size_t)(entries + spill_entries);
}

extern "C" int gc_env_checkpoint_bytes(gc_env* e, uint64_t* bytes) {
    if (!e || !bytes) return fail("null argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    Temps tmps;
    uint32_t *hl = nullptr, *offs = nullptr;
    if (tmps.alloc(&hl, e->n) || tmps.alloc(&offs, e->n)) return -1;
    uint64_t total = 0, stotal = 0;
    if (ckpt_offsets(e, e->meta, hl, offs, &total) || spill_offsets(e, hl, offs, &stotal)) return -1;
    *bytes = ckpt_bytes(e->n, total, stotal);
    return 0;
}

extern "C" int gc_env_save(gc_env* e, void* buf, uint64_t cap, uint64_t* written) {
    if (!e || !buf) return fail("null argument");
    SRV_QUIESCE(e);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int n = e->n;
    uint32_t *hl = nullptr, *offs = nullptr, *bad = nullptr, *scnt = nullptr, *soffs = nullptr, *fill = nullptr;
    u64 *ents = nullptr, *sents = nullptr;
    Temps tmps;
    if (tmps.alloc(&hl, n) || tmps.alloc(&offs, n) || tmps.alloc(&bad, 1) || tmps.alloc(&scnt, n) || tmps.alloc(&soffs, n) ||
        tmps.alloc(&fill, n))
        return -1;
    uint64_t total = 0, stotal = 0;
    if (ckpt_offsets(e, e->meta, hl, offs, &total) || spill_offsets(e, scnt, soffs, &stotal)) return -1;
    const size_t need = ckpt_bytes(n, total, stotal);
    if (written) *written = need;
    if (cap < need) return fail("checkpoint buffer too small: need " + std::to_string(need) + " bytes");
    if (tmps.alloc(&ents, 8 * (total ? total : 1)) || tmps.alloc(&sents, 8 * (stotal ? stotal : 1))) return -1;
    CkptHeader hd = {};
    memcpy(hd.magic, CKPT_MAGIC, 8);
    hd.version = 2; hd.n = (uint32_t)n; hd.rules = (uint32_t)e->rules; hd.opp = (uint32_t)e->d.opp;
    hd.agent_black = (uint32_t)e->d.agent_black; hd.policy_ready = e->policy_ready ? 1u : 0u;
    hd.seed = e->seed;
    for (int j = 0; j < NBB; j++) hd.init[j] = e->d.init[j];
    hd.entries = total;
    hd.spill_entries = stotal;
    hd.layout = CKPT_LAYOUT;
    uint8_t* out = static_cast<uint8_t*>(buf);
    memcpy(out, &hd, sizeof hd);
    const size_t o_slab = sizeof hd, o_scnt = o_slab + Slab::BYTES_PER_BOARD * (size_t)n, o_ent = o_scnt + 4 * (size_t)n,
                 o_sent = o_ent + 64 * (size_t)total;
    uint32_t flag = 0;
    hipError_t he = hipMemsetAsync(bad, 0, 4, e->stream);
    if (he == hipSuccess) {
        k_ckpt_pack<<<grid_for(n), BLOCK, 0, e->stream>>>(e->d.htab, e->d.hgen, e->meta, n, e->d.hbits, offs, ents, bad);
        he = hipGetLastError();
    }
    if (he == hipSuccess && stotal) {
        const SpillTab& sp = e->d.ic.spill;
        const size_t slots = (size_t)sp.mask + 1;
        he = hipMemsetAsync(fill, 0, (size_t)4 * n, e->stream);
        if (he == hipSuccess) {
            k_spill_collect<<<grid_for_slots(slots), BLOCK, 0, e->stream>>>(sp.ent, sp.mask, e->d.hgen,
                                                                                              fill, soffs, sents);
            he = hipGetLastError();
        }
    }
    if (he == hipSuccess) he = hipMemcpyAsync(out + o_slab, e->slab, Slab::BYTES_PER_BOARD * (size_t)n, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(out + o_scnt, scnt, 4 * (size_t)n, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess && total) he = hipMemcpyAsync(out + o_ent, ents, 64 * total, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess && stotal) he = hipMemcpyAsync(out + o_sent, sents, 64 * stotal, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(&flag, bad, 4, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess) return fail(std::string("checkpoint save: ") + hipGetErrorString(he));
    if (flag) return fail("checkpoint save: a repetition window does not match its recorded length");
    return 0;
}

extern "C" int gc_env_load(gc_env* e, const void* buf, uint64_t size) {
    if (!e || !buf) return fail("null argument");
    SRV_QUIESCE(e);
    if (size < sizeof(CkptHeader)) return fail("checkpoint: truncated header");
    CkptHeader hd;
    memcpy(&hd, buf, sizeof hd);
    if (memcmp(hd.magic, CKPT_MAGIC, 8) != 0 || hd.version != 2) return fail("checkpoint: not a gc_env checkpoint (v2)");
    if (hd.layout != CKPT_LAYOUT) return fail("checkpoint: written by a build with another slab layout");
    if ((int)hd.n != e->n) return fail("checkpoint: it holds " + std::to_string(hd.n) + " boards, the env " + std::to_string(e->n));
    if ((int)hd.rules != e->rules || (int)hd.opp != e->d.opp || (int)hd.agent_black != e->d.agent_black)
        return fail("checkpoint: rules / opponent / player colour differ from the env's");
    if (hd.seed != e->seed) return fail("checkpoint: the env's seed differs (the policy streams would not continue)");
    for (int j = 0; j < NBB; j++)
        if (hd.init[j] != e->d.init[j]) return fail("checkpoint: the env's initial board differs");
    if (size != ckpt_bytes(e->n, hd.entries, hd.spill_entries)) return fail("checkpoint: size does not match its header");
    if (hd.spill_entries && !e->d.ic.spill.ent) return fail("checkpoint: spill entries, but the env has no spill table");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int n = e->n;
    const uint8_t* in = static_cast<const uint8_t*>(buf);
    const size_t o_slab = sizeof hd, o_scnt = o_slab + Slab::BYTES_PER_BOARD * (size_t)n, o_ent = o_scnt + 4 * (size_t)n,
                 o_sent = o_ent + 64 * (size_t)hd.entries;
    uint8_t* slab = nullptr;
    u64 *ents = nullptr, *sents = nullptr;
    uint32_t *hl = nullptr, *offs = nullptr, *gnew = nullptr, *bad = nullptr, *scnt = nullptr, *soffs = nullptr;
    Temps tmps;
    if (tmps.alloc(&slab, Slab::BYTES_PER_BOARD * (size_t)n) || tmps.alloc(&ents, 8 * (hd.entries ? hd.entries : 1)) ||
        tmps.alloc(&sents, 8 * (hd.spill_entries ? hd.spill_entries : 1)) || tmps.alloc(&hl, n) || tmps.alloc(&offs, n) ||
        tmps.alloc(&gnew, n) || tmps.alloc(&bad, 1) || tmps.alloc(&scnt, n) || tmps.alloc(&soffs, n))
        return -1;
    // stage everything and validate it against the env's tables before touching the env
    hipError_t he = hipMemcpyAsync(slab, in + o_slab, Slab::BYTES_PER_BOARD * (size_t)n, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(scnt, in + o_scnt, 4 * (size_t)n, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess && hd.entries)
        he = hipMemcpyAsync(ents, in + o_ent, 64 * hd.entries, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess && hd.spill_entries)
        he = hipMemcpyAsync(sents, in + o_sent, 64 * hd.spill_entries, hipMemcpyHostToDevice, e->stream);
    if (he != hipSuccess) return fail(std::string("checkpoint load: ") + hipGetErrorString(he));
    uint64_t total = 0, stotal = 0;
    const u32* smeta = reinterpret_cast<const u32*>(slab + Slab::meta(n));
    if (ckpt_offsets(e, smeta, hl, offs, &total) || scan_u32(e, scnt, soffs, n, &stotal)) return -1;
    if (total != hd.entries || stotal != hd.spill_entries)
        return fail("checkpoint: window lengths do not match the entries it holds");
    uint32_t flag = 0;
    he = hipMemsetAsync(bad, 0, 4, e->stream);
    if (he == hipSuccess) {
        k_ckpt_check<<<grid_for(n), BLOCK, 0, e->stream>>>(smeta, scnt, n, e->d.hbits, e->d.ic.spill.ent != nullptr, bad);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(&flag, bad, 4, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess || flag)
        return fail(he != hipSuccess ? std::string("checkpoint load: ") + hipGetErrorString(he)
                                     : std::string("checkpoint: its repetition windows do not fit this env's tables"));
    // the spill table, emptied (every entry would be dead under the fresh generations) and
    // sized for the restored entries at a load <= 1/8
    if (e->d.ic.spill.ent) {
        int bits = e->sp_bits;
        while (((uint64_t)1 << bits) < 8 * stotal) bits++;
        if (spill_alloc(e, bits)) return -1;
    }
    // from here on the env changes; a failure resets every board (never a half-restored env)
    k_ckpt_gen<<<grid_for(n), BLOCK, 0, e->stream>>>(e->d.hgen, reinterpret_cast<const u32*>(slab + Slab::hgen(n)), n,
                                                     gnew);
    he = hipGetLastError();
    if (he == hipSuccess)
        he = hipMemcpyAsync(e->slab, slab, Slab::BYTES_PER_BOARD * (size_t)n, hipMemcpyDeviceToDevice, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(bad, 0, 4, e->stream);
    if (he == hipSuccess) {
        k_ckpt_unpack<<<grid_for(n), BLOCK, 0, e->stream>>>(e->d.htab, e->d.hgen, e->meta, n, e->d.hbits, gnew, offs,
                                                            ents, e->d.ic.spill, stotal ? scnt : nullptr, soffs, sents,
                                                            bad);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(&flag, bad, 4, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess || flag) {
        std::string m = he != hipSuccess ? std::string("checkpoint load: ") + hipGetErrorString(he)
                                         : std::string("checkpoint load: a repetition window did not fit the table");
        if (he == hipSuccess) {  // the env is half-restored: start every board afresh
            launch_reset(e, nullptr, 1);
            (void)hipStreamSynchronize(e->stream);
            e->policy_ready = true;
            m += " (every board was reset)";
        }
        return fail(m);
    }
    e->policy_ready = hd.policy_ready != 0;
    return 0;
}
