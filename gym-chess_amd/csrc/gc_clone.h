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
// The per-pair copy is clone_pair; k_move_boards (at the end) runs it pair after pair inside one
// wave for the boards gc_tree_advance moves within the tree env.
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

// one pair by one wave: board si of the source (in range, uniform over the wave) into board di of
// the destination (likewise).  Every load of the pair is consumed -- stored, or looked at by the
// wave's ballot -- before the function returns, so in a wave that copies pair after pair no store
// of a later pair can overtake a load of an earlier one.  The envs' addresses and sizes come as
// values, not as a reference to the kernel's CloneArgs: through a reference the compiler no longer
// proves k_clone_boards' three uniform loads (meta, the two generations) unclobbered and turns
// them from scalar into vector loads.
struct ClonePairArgs {
    const uint8_t* sslab;
    const u64* stab;
    uint8_t* dslab;
    u64* dtab;
    int ns, nd, hbits;
};
__device__ __forceinline__ void clone_pair(const uint8_t* sslab, const u64* stab, uint8_t* dslab, u64* dtab,
                                           int ns_, int nd_, int hbits, int si, int di, int lane) {
    const ClonePairArgs A{sslab, stab, dslab, dtab, ns_, nd_, hbits};
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
    clone_pair(A.sslab, A.stab, A.dslab, A.dtab, A.ns, A.nd, A.hbits, si, di, lane);
}

// Boards moved inside ONE env, game by game (gc_tree_advance): board g * nodes + k of a game with
// kept[g] > 0 goes to board g * nodes + remap[g][k] for every k with 0 <= remap[g][k] < k (a node
// that stays where it is needs no copy).  Within a game the pairs overlap: dst_i = base + i is
// never the source of a LATER pair (sources ascend and lie above their destinations) and no source
// was an earlier destination, but dst_i can be the source of an EARLIER pair (node 1 becomes the
// root, its child becomes node 1).  So one wave takes a whole game and copies its pairs one after
// the other in ascending order; clone_pair consumes every load of a pair before it returns, and
// the wave's program order puts the next pair's stores after that.  A wave per pair, as
// k_clone_boards has it, would be wrong here.  Games touch disjoint boards.
__global__ __launch_bounds__(64 * CLN_WAVES) void k_move_boards(const CloneArgs A, const int32_t* __restrict__ remap,
                                                                 const int32_t* __restrict__ kept, int games, int nodes) {
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(blockIdx.x * CLN_WAVES + (threadIdx.x >> 6));
    if (g >= games) return;
    if (__builtin_amdgcn_readfirstlane(kept[g]) <= 0) return;  // a fresh game: no board touched
    const size_t gb = (size_t)g * nodes;
    if (gb + nodes > (size_t)A.ns) return;  // (never: games * nodes <= the env's boards)
    for (int c0 = 0; c0 < nodes; c0 += 64) {
        const int k = c0 + lane;
        const int nw = k < nodes ? remap[gb + k] : -1;
        u64 todo = __ballot(nw >= 0 && nw < k);
        while (todo) {
            const int l = (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            const int d = __builtin_amdgcn_readfirstlane(__shfl(nw, l, 64));
            clone_pair(A.sslab, A.stab, A.dslab, A.dtab, A.ns, A.nd, A.hbits, (int)(gb + c0 + l), (int)(gb + d),
                       lane);
        }
    }
}
