// gc_clone.h -- boards copied between envs on the device (gc_env_clone_boards, include/gymchess.h):
// per pair (source board, destination board) the seven bitboards, the meta word, the last step's
// reward / done / reason and the live 3-fold window; the destination keeps its policy stream
// (draw counter, board index) and its step counter.
//
// The window is the cost.  A board's table is 2^hbits 64-byte entries 4 KiB apart (the
// wave-blocked layout of DevHist::entry: the 64 boards of a block interleave entry by entry),
// so there is no contiguous 32 KiB to stream -- every entry is one cache line of its own.
// Mapping (k_clone_boards): one wave per pair, four pairs per workgroup.  Four lanes share an
// entry, 16 bytes each, so a wave-wide load covers 16 entries and CLN_UNROLL of them are in
// flight before the first is looked at.  The quad's first lane holds the header: whether it is
// live under the source's generation (rep_clone_hdr, gc_env.h) reaches the other three lanes
// through the wave's ballot, which also counts the live entries -- the scan ends once the
// window's length (the meta word's hl) has been copied, and a board with an empty window (fresh
// from a reset, a capture or a pawn move) touches no table at all.  Live entries are written
// to the same slot positions of the destination's table under its new generation (one bump,
// which kills whatever the table held).  No LDS, no atomics but the skipped-pair count.
// Included by gymchess.hip after DevHist.
#pragma once

#define CLN_WAVES 4    // pairs per workgroup
#define CLN_UNROLL 4   // 16-entry loads in flight per wave

struct CloneArgs {
    const uint8_t* sslab;  // the source env's per-board fields (Slab) and tables
    const u64* stab;
    uint8_t* dslab;        // the destination's (the same env's when src == dst)
    u64* dtab;
    const int32_t* sidx;   // [m] device memory
    const int32_t* didx;
    unsigned long long* skipped;  // pairs with an index out of range
    int ns, nd, m, hbits;
};

__global__ __launch_bounds__(64 * CLN_WAVES) void k_clone_boards(const CloneArgs A) {
    const int lane = threadIdx.x & 63;
    // the pair: uniform over the wave
    const int j = __builtin_amdgcn_readfirstlane(blockIdx.x * CLN_WAVES + (threadIdx.x >> 6));
    if (j >= A.m) return;
    const int si = __builtin_amdgcn_readfirstlane(A.sidx[j]), di = __builtin_amdgcn_readfirstlane(A.didx[j]);
    if ((unsigned)si >= (unsigned)A.ns || (unsigned)di >= (unsigned)A.nd) {
        if (lane == 0) atomicAdd(A.skipped, 1ull);
        return;
    }
    const size_t ns = (size_t)A.ns, nd = (size_t)A.nd;
    const u32* smeta = reinterpret_cast<const u32*>(A.sslab + Slab::meta(ns));
    const u32* shgen = reinterpret_cast<const u32*>(A.sslab + Slab::hgen(ns));
    u32* dhgen = reinterpret_cast<u32*>(A.dslab + Slab::hgen(nd));
    const u32 meta = smeta[si], sg = shgen[si], dg = dhgen[di] + 1u;

    // the slab's fields, one per lane
    if (lane < NBB) {
        reinterpret_cast<u64*>(A.dslab)[lane * nd + di] = reinterpret_cast<const u64*>(A.sslab)[lane * ns + si];
    } else if (lane == NBB) {
        reinterpret_cast<u32*>(A.dslab + Slab::meta(nd))[di] = meta;
        dhgen[di] = dg;
    } else if (lane == NBB + 1) {
        reinterpret_cast<int32_t*>(A.dslab + Slab::reward(nd))[di] =
            reinterpret_cast<const int32_t*>(A.sslab + Slab::reward(ns))[si];
    } else if (lane == NBB + 2) {
        (A.dslab + Slab::done(nd))[di] = (A.sslab + Slab::done(ns))[si];
    } else if (lane == NBB + 3) {
        (A.dslab + Slab::reason(nd))[di] = (A.sslab + Slab::reason(ns))[si];
    }

    int left = (int)hl_of(meta);  // live entries still to find
    if (left == 0) return;
    const DevHist hs{const_cast<u64*>(A.stab), nullptr, sg, si, A.hbits};
    const DevHist hd{A.dtab, nullptr, dg, di, A.hbits};
    const ulonglong2* sp = reinterpret_cast<const ulonglong2*>(A.stab);
    ulonglong2* dp = reinterpret_cast<ulonglong2*>(A.dtab);
    const int quad = lane >> 2, part = lane & 3, size = 1 << A.hbits;
    for (int base = 0; base < size && left > 0; base += 16 * CLN_UNROLL) {
        ulonglong2 v[CLN_UNROLL];
#pragma unroll
        for (int u = 0; u < CLN_UNROLL; u++) v[u] = sp[hs.entry(base + 16 * u + quad) * 4 + part];
#pragma unroll
        for (int u = 0; u < CLN_UNROLL; u++) {
            u64 hdr = v[u].x;
            const bool live = rep_clone_hdr(hdr, sg, dg, &hdr) && part == 0;
            const u64 lives = __ballot(live);  // bit 4q: entry q of these 16 is live
            if (live) v[u].x = hdr;
            if ((lives >> (lane & ~3)) & 1) dp[hd.entry(base + 16 * u + quad) * 4 + part] = v[u];
            left -= __popcll(lives);
        }
    }
}
