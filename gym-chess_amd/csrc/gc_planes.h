// gc_planes.h -- a network's input on the device: the env's current state of every board as
// GC_PLANES = 24 planes of 8x8 (gc_env_encode_planes, include/gymchess.h), fp32 / fp16 / bf16,
// NCHW or channels-last, absolute or relative to the side to move.
//
// Store-bound: a board reads its seven bitboards, meta word and one entry of its 3-fold table
// (~130 B) and writes 1536 elements (3 KiB in fp16).  Mapping (k_encode_planes): one wave per
// board, four boards per workgroup.  Everything a board's values depend on is uniform over its
// wave (scalar loads and SALU), so a lane only expands bits: the block is NV = 1536 / EPV
// 16-byte vectors (EPV = 8 halves or 4 floats), lane l writes vectors l, l + 64, ..., and each
// store instruction of the wave covers 1 KiB contiguous.
//   NCHW  vector v = EPV squares of one row of plane c = v * EPV / 64: EPV bits of the plane's
//         bitboard, picked among the store's 8 (halves) or 4 (floats) planes by the lane's high
//         bits;
//   NHWC  vector v = EPV channels of square v * EPV / 24: lane l first gathers the 24 plane bits
//         of square l into one word, a store reads the word of its square from that lane.
// A set bit becomes the plane's value (1, or move_count / 256 on plane 19), a clear bit 0.
// No LDS, no scratch, no per-element store.  Included by gymchess.hip after DevHist / SpillTab.
#pragma once

#define PLN_C 24                        // planes (GC_PLANES)
#define PLN_ELEMS (PLN_C * 64)          // elements per board
#define PLN_WAVES 4                     // boards per workgroup
// Non-temporal stores: the tensor is written once and read by another kernel much later, and
// at N = 65 536 it is 201-403 MB, many times the L2.  Measured (tools/planes_bench.py, same
// process, GC_PLANES_NT read per call): fp16 49 us per launch against 67 with plain stores,
// fp32 73 against 173.
#ifndef PLN_NT_DEFAULT
#define PLN_NT_DEFAULT true
#endif
#define PLN_MC 19                       // the move_count plane (the only value that is not 0 / 1)

struct PlanesArgs {
    const u64* bb;    // [7][n]
    const u32* meta;  // [n]
    const u32* hgen;  // [n]
    u64* htab;        // the 3-fold tables (read only here)
    SpillTab sp;
    void* out;
    size_t stride;    // elements per board
    int n;
    int hbits;
    int persp;        // planes relative to the side to move
    int fide;         // plane 22 from the meta word's en-passant field
};

// How often board s already occurs in its live 3-fold window (0 = not there): the probe
// sequence of rep_commit and, for a spilled window, of spill_find -- without their writes.
template <class H>
GC_HD int rep_peek(const H& h, const Pos& s) {
    const int bits = h.bits();
    const u32 size_mask = (1u << bits) - 1, gen = h.gen(), key = board_key(s);
    const u32 tag = key >> bits;
    u32 pos = key & size_mask;
    for (int probe = 0; probe <= (int)size_mask; probe++) {
        const RepEntry e = h.load((int)pos);
        if ((u32)e.hdr != gen) break;  // free for this generation
        if ((u32)((e.hdr >> 32) & tag_mask(bits)) == tag && rep_same(e, s)) return (int)(e.hdr >> 56);
        pos = (pos + 1) & size_mask;
    }
    if (h.spill_mask() == 0 || (int)hl_of(s.meta) < hist_cap(bits)) return 0;
    const u32 mask = h.spill_mask(), me1 = h.owner() + 1;
    u32 slot = sp_home(key, h.owner(), mask);
    for (int probe = 0; probe < SPILL_PROBES; probe++, slot = (slot + 1) & mask) {
        const u64 e = h.sp_hdr(slot);
        if (sp_owner1(e) == 0) return 0;
        if (sp_owner1(e) == me1 && sp_gen(e) == gen && h.sp_same(slot, s)) return (int)sp_cnt(e);
    }
    return 0;
}

// the 24 planes of a position as bitboards (bit sq of pl[c] = element (c, sq) is non-zero);
// rep = its count in the 3-fold window, ep = the en-passant target square or -1
GC_HD void planes_bits(const Pos& s, int rep, int ep, bool persp, u64* pl) {
    const bool white = (s.meta & M_WHITE) != 0;
    const bool flip = persp && !white;
    const u64 first = flip ? ~s.w : s.w;
    const u64 t[6] = {s.k, s.q, s.r, s.b, s.n, s.p};
    for (int k = 0; k < 6; k++) {
        const u64 a = t[k] & first, b = t[k] & ~first;
        pl[k] = flip ? __builtin_bswap64(a) : a;
        pl[6 + k] = flip ? __builtin_bswap64(b) : b;
    }
    const u32 m = s.meta;
    auto all = [](bool on) { return on ? ~0ull : 0ull; };
    pl[12] = all(white);
    pl[13] = all(m & (flip ? M_BKC : M_WKC));
    pl[14] = all(m & (flip ? M_BQC : M_WQC));
    pl[15] = all(m & (flip ? M_WKC : M_BKC));
    pl[16] = all(m & (flip ? M_WQC : M_BQC));
    pl[17] = all(m & (flip ? M_BCHK : M_WCHK));
    pl[18] = all(m & (flip ? M_WCHK : M_BCHK));
    pl[PLN_MC] = ~0ull;
    pl[20] = all(rep >= 1);
    pl[21] = all(rep >= 2);
    pl[22] = ep < 0 ? 0ull : bit(flip ? ep ^ 56 : ep);
    pl[23] = ~0ull;
}

typedef u32 pln_vec __attribute__((ext_vector_type(4)));

// the raw element of k / 256 (k < 256; exact in all three types) and of 1
template <int DT>
__device__ __forceinline__ u32 pln_raw(u32 k, bool one) {
    const u32 f = __float_as_uint(one ? 1.0f : (float)k * (1.0f / 256.0f));
    if (DT == 0) return f;
    if (DT == 2) return f >> 16;  // at most 8 significant bits: the truncation is exact
    union { _Float16 h; uint16_t u; } c;
    c.h = (_Float16)__uint_as_float(f);
    return c.u;
}

// EPV bits -> one 16-byte vector: element j = (bits >> j) & 1 ? val[j] : 0.  mcpos = the element
// that holds the move_count plane (its value is vmc, every other 1), or -1.
template <int DT>
__device__ __forceinline__ pln_vec pln_expand(u32 bits, u32 vone, u32 vmc, int mcpos, bool all_mc) {
    pln_vec o;
    if (DT == 0) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u32 v = (all_mc || j == mcpos) ? vmc : vone;
            o[j] = (0u - ((bits >> j) & 1u)) & v;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u32 lo = (all_mc || 2 * j == mcpos) ? vmc : vone;
            const u32 hi = (all_mc || 2 * j + 1 == mcpos) ? vmc : vone;
            o[j] = ((0u - ((bits >> (2 * j)) & 1u)) & lo) | ((0u - ((bits >> (2 * j + 1)) & 1u)) & (hi << 16));
        }
    }
    return o;
}

template <bool NT>
__device__ __forceinline__ void pln_store(pln_vec* p, pln_vec v) {
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

template <int DT, bool NHWC, bool NT>
__global__ __launch_bounds__(64 * PLN_WAVES) void k_encode_planes(const PlanesArgs A) {
    constexpr int EPV = DT == 0 ? 4 : 8;         // elements per 16-byte vector
    constexpr int STORES = PLN_ELEMS / EPV / 64;  // per lane: 3 (halves) or 6 (floats)
    const int lane = threadIdx.x & 63;
    // the board: uniform over the wave, so its loads are scalar
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * PLN_WAVES + (threadIdx.x >> 6));
    if (i >= A.n) return;
    const size_t n = (size_t)A.n;
    Pos s;
    s.k = A.bb[0 * n + i]; s.q = A.bb[1 * n + i]; s.r = A.bb[2 * n + i]; s.b = A.bb[3 * n + i];
    s.n = A.bb[4 * n + i]; s.p = A.bb[5 * n + i]; s.w = A.bb[6 * n + i];
    s.meta = A.meta[i];
    DevHist h{A.htab, const_cast<u32*>(A.hgen), A.hgen[i], i, A.hbits};
    h.sp = A.sp;
    const int rep = rep_peek(h, s);
    u64 pl[PLN_C];
    planes_bits(s, rep, A.fide ? gcf::ep_square(s.meta) : -1, A.persp != 0, pl);
    const u32 vone = pln_raw<DT>(0, true), vmc = pln_raw<DT>(mc_of(s.meta) & 0xFFu, false);
    pln_vec* out = reinterpret_cast<pln_vec*>(reinterpret_cast<char*>(A.out) + (size_t)i * A.stride * (DT == 0 ? 4 : 2));

    if (!NHWC) {
        constexpr int VPP = 64 / EPV;       // vectors per plane: 8 or 16
        constexpr int PPS = 64 / VPP;       // planes per store instruction: 8 or 4
        const int sub = lane / VPP;         // the lane's plane within the store
        const int sq0 = (lane % VPP) * EPV; // its first square
#pragma unroll
        for (int st = 0; st < STORES; st++) {
            u64 w = pl[st * PPS];
#pragma unroll
            for (int k = 1; k < PPS; k++) w = sub == k ? pl[st * PPS + k] : w;
            const u32 bits = (u32)(w >> sq0) & ((1u << EPV) - 1u);
            const bool mc = st * PPS <= PLN_MC && PLN_MC < (st + 1) * PPS && sub == PLN_MC - st * PPS;
            pln_store<NT>(out + st * 64 + lane, pln_expand<DT>(bits, vone, vmc, -1, mc));
        }
    } else {
        // the 24 plane bits of square `lane`
        u32 ch = 0;
#pragma unroll
        for (int c = 0; c < PLN_C; c++) ch |= ((u32)(pl[c] >> lane) & 1u) << c;
#pragma unroll
        for (int st = 0; st < STORES; st++) {
            const int v = st * 64 + lane;
            const int e0 = v * EPV, sq = e0 / PLN_C, c0 = e0 - sq * PLN_C;
            const u32 bits = ((u32)__shfl((int)ch, sq, 64) >> c0) & ((1u << EPV) - 1u);
            pln_store<NT>(out + v, pln_expand<DT>(bits, vone, vmc, PLN_MC - c0, false));
        }
    }
}

// The indexed form (gc_env_encode_planes_rows): wave = row j of the output, its board read
// through the index (one scalar load); the network's batch for the nodes a search just expanded.
// An index outside [0, n) gives an all-zero row: all 1536 elements of every row are written, the
// stride's padding never.  The body restates k_encode_planes' instead of sharing a function with
// it: moving that kernel's body into one changed its register allocation, and the dense
// instantiations are to stay as they are.
// Stores: a [rows] block is a few MB (3 MiB at 1024 rows of fp16) and is read by the network right
// away, so plain stores that leave it in the L2 were the candidate.  Measured on an env of 65 536
// boards, fp16 NCHW side-to-move view (tools/expand_bench.py, GC_PLANES_NT read per call): 3.7-3.9
// us per launch with either form at 1024 rows, 5.3-5.5 plain against 5.2 non-temporal at 4096 (two
// runs) -- launch-bound, the forms differ by less than a leg's own spread; the non-temporal one was
// never the slower, so it is the default here too.  What the network's first read gains from
// either is not measured.
#ifndef PLN_ROWS_NT_DEFAULT
#define PLN_ROWS_NT_DEFAULT true
#endif

struct PlanesRowsArgs {
    PlanesArgs p;              // out / stride: the row block's
    const int32_t* board_idx;  // [rows]
    int rows;
};

template <int DT, bool NHWC, bool NT>
__global__ __launch_bounds__(64 * PLN_WAVES) void k_encode_planes_rows(const PlanesRowsArgs R) {
    constexpr int EPV = DT == 0 ? 4 : 8;         // elements per 16-byte vector
    constexpr int STORES = PLN_ELEMS / EPV / 64;  // per lane: 3 (halves) or 6 (floats)
    const PlanesArgs& A = R.p;
    const int lane = threadIdx.x & 63;
    // the row and its board: uniform over the wave, so their loads are scalar
    const int j = __builtin_amdgcn_readfirstlane(blockIdx.x * PLN_WAVES + (threadIdx.x >> 6));
    if (j >= R.rows) return;
    const int i = __builtin_amdgcn_readfirstlane(R.board_idx[j]);
    pln_vec* out = reinterpret_cast<pln_vec*>(reinterpret_cast<char*>(A.out) + (size_t)j * A.stride * (DT == 0 ? 4 : 2));
    if ((u32)i >= (u32)A.n) {
        const pln_vec z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int st = 0; st < STORES; st++) pln_store<NT>(out + st * 64 + lane, z);
        return;
    }
    const size_t n = (size_t)A.n;
    Pos s;
    s.k = A.bb[0 * n + i]; s.q = A.bb[1 * n + i]; s.r = A.bb[2 * n + i]; s.b = A.bb[3 * n + i];
    s.n = A.bb[4 * n + i]; s.p = A.bb[5 * n + i]; s.w = A.bb[6 * n + i];
    s.meta = A.meta[i];
    DevHist h{A.htab, const_cast<u32*>(A.hgen), A.hgen[i], i, A.hbits};
    h.sp = A.sp;
    const int rep = rep_peek(h, s);
    u64 pl[PLN_C];
    planes_bits(s, rep, A.fide ? gcf::ep_square(s.meta) : -1, A.persp != 0, pl);
    const u32 vone = pln_raw<DT>(0, true), vmc = pln_raw<DT>(mc_of(s.meta) & 0xFFu, false);

    if (!NHWC) {
        constexpr int VPP = 64 / EPV, PPS = 64 / VPP;  // vectors per plane, planes per store (k_encode_planes)
        const int sub = lane / VPP, sq0 = (lane % VPP) * EPV;
#pragma unroll
        for (int st = 0; st < STORES; st++) {
            u64 w = pl[st * PPS];
#pragma unroll
            for (int k = 1; k < PPS; k++) w = sub == k ? pl[st * PPS + k] : w;
            const u32 bits = (u32)(w >> sq0) & ((1u << EPV) - 1u);
            const bool mc = st * PPS <= PLN_MC && PLN_MC < (st + 1) * PPS && sub == PLN_MC - st * PPS;
            pln_store<NT>(out + st * 64 + lane, pln_expand<DT>(bits, vone, vmc, -1, mc));
        }
    } else {
        u32 ch = 0;  // the 24 plane bits of square `lane`
#pragma unroll
        for (int c = 0; c < PLN_C; c++) ch |= ((u32)(pl[c] >> lane) & 1u) << c;
#pragma unroll
        for (int st = 0; st < STORES; st++) {
            const int v = st * 64 + lane;
            const int e0 = v * EPV, sq = e0 / PLN_C, c0 = e0 - sq * PLN_C;
            const u32 bits = ((u32)__shfl((int)ch, sq, 64) >> c0) & ((1u << EPV) - 1u);
            pln_store<NT>(out + v, pln_expand<DT>(bits, vone, vmc, PLN_MC - c0, false));
        }
    }
}
