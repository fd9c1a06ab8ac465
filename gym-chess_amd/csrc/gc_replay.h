// gc_replay.h -- self-play training samples on the device (gc_replay_*, include/gymchess.h): every
// move a packed position and the root's visit counts are recorded per game (k_replay_record), a
// finished game's samples get their outcome and enter a ring (k_replay_scan, k_replay_commit), and
// a minibatch -- planes, policy target in the network's view, value target -- is decoded from
// ring slots in one launch (k_replay_sample).  Integer work, copies and one fp32 division per
// target entry; no atomics, so the ring is a function of the call sequence.
//
// A sample (pending area and ring alike) is a row of three arrays:
//   pos  u64[8]    k, q, r, b, n, p, w bitboards; word 7 = meta word (bits 0-31) | the position's
//                  count in its 3-fold window, saturated at 2 (32-39) | n entries (40-48)
//   act  u16[cap]  the n actions in row order, then 0xFFFF
//   vis  i32[cap]  their visit counts, then 0
// and, in the ring only, z f32.  64 + 6 * cap + 4 bytes against the 3 KiB of fp16 planes.
//
// Mapping: record and commit one wave per game (lanes over the cap entries), RPL_WAVES games per
// workgroup; a game is touched by its own wave only.  The scan is one workgroup.  Sample: one wave
// per row; the slot and the position are uniform over the wave (scalar loads), the planes leave by
// k_encode_planes_rows' vector stores (its body restated: gc_planes.h says why those kernels stay
// as they are) and the dense target is built in an LDS row of 4100 floats -- zeroed, the <= 256
// entries scattered in, then streamed out as 1025 16-byte stores that each carry their final
// contents, so no element of the output is stored twice.  Included by gymchess.hip after
// gc_planes.h and gc_policy.h.
#pragma once

#define RPL_WAVES 4          // games per workgroup (record, commit)
#define RPL_SAMPLE_WAVES 2   // rows per workgroup (sample): 2 x 16 400 B of LDS
#define RPL_MAX_CAP 256
#define RPL_ROW 4100         // elements of a logits row (actions 0..4099)
#define RPL_ROW_VECS (RPL_ROW / 4)
#define RPL_SCAN_THREADS 1024
#define RPL_NO_ACTION 0xFFFFu
// Non-temporal stores in k_replay_sample (planes and dense target; GC_REPLAY_NT read per call).
// A trainer reads the batch at once, and a batch fits the Infinity Cache.  Measured
// (tools/replay_bench.py, fp16 NCHW planes + dense target, windows alternating): 7.9 us per launch
// plain against 7.6 non-temporal at 1024 rows, 18.7 against 20.1 at 4096 -- plain is the default.
#ifndef RPL_NT_DEFAULT
#define RPL_NT_DEFAULT false
#endif

struct ReplayDev {
    // pending [games][max_plies] and ring [capacity] samples
    u64* pend_pos;
    uint16_t* pend_act;
    int32_t* pend_vis;
    u64* ring_pos;
    uint16_t* ring_act;
    int32_t* ring_vis;
    float* ring_z;
    int32_t* plies;    // [games] records of the running episode (dropped ones included)
    int32_t* dropped;  // [games] records past max_plies, since creation / clear
    u64* total;        // [1] samples ever committed
    int32_t* off;      // [games] the last commit's exclusive prefix of stored samples
    u64* base;         // [1] `total` before the last commit
    int games, cap, max_plies, capacity;
};

// what the store reads of its env
struct ReplayEnv {
    const u64* bb;    // [7][n]
    const u32* meta;  // [n]
    const u32* hgen;  // [n]
    u64* htab;        // the 3-fold tables (read only here)
    SpillTab sp;
    int n;
    int hbits;
};

using RplReduceI64 = hipcub::WarpReduce<long long, 64>;
__device__ __forceinline__ long long rpl_wave_sum(long long v) {
    RplReduceI64::TempStorage ts;
    return __shfl(RplReduceI64(ts).Sum(v), 0, 64);
}

// gc_replay_record: pending sample plies[g] of game g from board g and row g of the root's
// actions / visits ([games][row_cap], row_cap <= cap).  Every element of the sample's three rows
// is stored exactly once (entries, then padding).
__global__ __launch_bounds__(64 * RPL_WAVES) void k_replay_record(const ReplayDev R, const ReplayEnv E,
                                                                  const uint16_t* __restrict__ actions,
                                                                  const int32_t* __restrict__ visits, int row_cap) {
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(blockIdx.x * RPL_WAVES + (threadIdx.x >> 6));
    if (g >= R.games) return;
    const size_t row = (size_t)g * row_cap;
    const int chunks = (row_cap + 63) >> 6;
    long long sum = 0;
    for (int c = 0; c < chunks; c++) {
        const int s = c * 64 + lane;
        if (s < row_cap) sum += visits[row + s];
    }
    if (rpl_wave_sum(sum) == 0) return;  // no move is played from this root
    const int p = R.plies[g];
    if (lane == 0) R.plies[g] = p + 1;
    if (p < 0) return;  // (never written by this file)
    if (p >= R.max_plies) {
        if (lane == 0) R.dropped[g] += 1;
        return;
    }
    const size_t smp = (size_t)g * R.max_plies + p, o = smp * R.cap;
    int run = 0;  // entries so far
    for (int c = 0; c < chunks; c++) {
        const int s = c * 64 + lane;
        const bool in = s < row_cap;
        const u32 a = in ? actions[row + s] : RPL_NO_ACTION;
        const int v = in ? visits[row + s] : 0;
        const bool on = a != RPL_NO_ACTION;
        const unsigned long long bal = __ballot(on);
        if (on) {
            const int dst = run + __popcll(bal & ((1ull << lane) - 1ull));
            R.pend_act[o + dst] = (uint16_t)a;
            R.pend_vis[o + dst] = v;
        }
        run += __popcll(bal);
    }
    for (int s = run + lane; s < R.cap; s += 64) {
        R.pend_act[o + s] = (uint16_t)RPL_NO_ACTION;
        R.pend_vis[o + s] = 0;
    }
    // the position: board g is uniform over the wave, so its loads are scalar
    const size_t n = (size_t)E.n;
    Pos s;
    s.k = E.bb[0 * n + g]; s.q = E.bb[1 * n + g]; s.r = E.bb[2 * n + g]; s.b = E.bb[3 * n + g];
    s.n = E.bb[4 * n + g]; s.p = E.bb[5 * n + g]; s.w = E.bb[6 * n + g];
    s.meta = E.meta[g];
    DevHist h{E.htab, const_cast<u32*>(E.hgen), E.hgen[g], g, E.hbits};
    h.sp = E.sp;
    int rep = rep_peek(h, s);
    rep = rep < 2 ? rep : 2;
    const u64 w7 = (u64)s.meta | ((u64)(u32)rep << 32) | ((u64)(u32)run << 40);
    const u64 words[8] = {s.k, s.q, s.r, s.b, s.n, s.p, s.w, w7};
    u64 mine = words[0];
#pragma unroll
    for (int k = 1; k < 8; k++) mine = lane == k ? words[k] : mine;
    if (lane < 8) R.pend_pos[smp * 8 + lane] = mine;
}

// the samples game g stores at this commit
__device__ __forceinline__ int rpl_commit_count(const ReplayDev& R, const uint8_t* done, int g) {
    if (!done[g]) return 0;
    const int P = R.plies[g];
    return P <= 0 ? 0 : (P < R.max_plies ? P : R.max_plies);
}

// gc_replay_commit, first launch (ONE workgroup): off[g] = the exclusive prefix, over games in
// ascending order, of the samples each committing game stores; base = total; total += their sum.
// Thread t takes the games [t * per, (t + 1) * per).
__global__ __launch_bounds__(RPL_SCAN_THREADS) void k_replay_scan(const ReplayDev R, const uint8_t* __restrict__ done) {
    using Scan = hipcub::BlockScan<int, RPL_SCAN_THREADS>;
    __shared__ typename Scan::TempStorage ts;
    const int per = (R.games + RPL_SCAN_THREADS - 1) / RPL_SCAN_THREADS;
    const int lo = (int)threadIdx.x * per;
    int hi = lo + per;
    hi = hi < R.games ? hi : R.games;
    int mine = 0;
    for (int g = lo; g < hi; g++) mine += rpl_commit_count(R, done, g);
    int before = 0, all = 0;
    Scan(ts).ExclusiveSum(mine, before, all);
    for (int g = lo; g < hi; g++) {
        R.off[g] = before;
        before += rpl_commit_count(R, done, g);
    }
    if (threadIdx.x == 0) {
        const u64 t = R.total[0];
        R.base[0] = t;
        R.total[0] = t + (u64)all;
    }
}

// gc_replay_commit, second launch: a finished game's stored samples go to ring slots (base +
// off[g] + p) mod capacity with their z; plies[g] = 0.  alternate: the sides alternate between
// samples (an opponent "none" env).
__global__ __launch_bounds__(64 * RPL_WAVES) void k_replay_commit(const ReplayDev R, const uint8_t* __restrict__ done,
                                                                  const uint8_t* __restrict__ reason,
                                                                  const float* __restrict__ outcome, int alternate) {
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(blockIdx.x * RPL_WAVES + (threadIdx.x >> 6));
    if (g >= R.games) return;
    if (!done[g]) return;
    const int P = R.plies[g];
    const int cnt = rpl_commit_count(R, done, g);
    float zl;
    if (outcome) zl = outcome[g];
    else zl = reason[g] == R_MATE ? 1.f : reason[g] == R_MATED ? -1.f : 0.f;
    if (zl == 0.f) zl = 0.f;  // (-0.0 too) a zero stays +0.0 under the sign flips below
    const u64 cap64 = (u64)R.capacity;
    const u64 first = (R.base[0] + (u64)R.off[g]) % cap64;
    for (int p = 0; p < cnt; p++) {
        const size_t src = (size_t)g * R.max_plies + p;
        const size_t dst = (size_t)((first + (u64)p) % cap64);
        for (int s = lane; s < R.cap; s += 64) {
            R.ring_act[dst * R.cap + s] = R.pend_act[src * R.cap + s];
            R.ring_vis[dst * R.cap + s] = R.pend_vis[src * R.cap + s];
        }
        if (lane < 8) R.ring_pos[dst * 8 + lane] = R.pend_pos[src * 8 + lane];
        if (lane == 0) R.ring_z[dst] = (alternate && ((P - 1 - p) & 1) && zl != 0.f) ? -zl : zl;
    }
    if (lane == 0) R.plies[g] = 0;
}

struct ReplaySampleArgs {
    const int32_t* index;  // [rows] ring slots, or NULL: drawn from (seed, row, draw)
    uint64_t seed;
    u32 draw;
    int rows;
    void* planes;      // every output may be NULL
    size_t stride;     // elements per planes row
    int persp;         // planes and target in the side-to-move view
    int fide;          // plane 22 from the meta word's en-passant field
    float* pi_dense;   // [rows][pi_stride]
    size_t pi_stride;
    int32_t* pi_index;  // [rows][cap]
    float* pi;          // [rows][cap]
    float* z;           // [rows]
    int32_t* slot;      // [rows]
};

// gc_replay_sample: row j of every output from ring slot index[j] (or the drawn one); a slot
// outside [0, live) gives the zero row.  DT / NHWC: the planes' element type and layout.
template <int DT, bool NHWC, bool NT>
__global__ __launch_bounds__(64 * RPL_SAMPLE_WAVES) void k_replay_sample(const ReplayDev R, const ReplaySampleArgs A) {
    constexpr int EPV = DT == 0 ? 4 : 8;         // elements per 16-byte vector
    constexpr int STORES = PLN_ELEMS / EPV / 64;  // per lane: 3 (halves) or 6 (floats)
    __shared__ pln_vec dense[RPL_SAMPLE_WAVES][RPL_ROW_VECS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // the row and its slot: uniform over the wave, so their loads are scalar
    const int j = __builtin_amdgcn_readfirstlane(blockIdx.x * RPL_SAMPLE_WAVES + wv);
    if (j >= A.rows) return;
    const u64 total = R.total[0];
    const u64 live = total < (u64)R.capacity ? total : (u64)R.capacity;
    long long want;
    if (A.index) want = A.index[j];
    else want = (long long)(((u64)philox_x0(A.seed, (u32)j, A.draw) * live) >> 32);
    const bool valid = want >= 0 && (u64)want < live;
    const int slot = __builtin_amdgcn_readfirstlane(valid ? (int)want : 0);  // (slot 0 exists: capacity >= 1)
    u32 meta = 0;
    int n = 0;

    if (valid) {
        const u64* ps = R.ring_pos + (size_t)slot * 8;
        Pos s;
        s.k = ps[0]; s.q = ps[1]; s.r = ps[2]; s.b = ps[3]; s.n = ps[4]; s.p = ps[5]; s.w = ps[6];
        const u64 w7 = ps[7];
        s.meta = (u32)w7;
        meta = s.meta;
        n = (int)((w7 >> 40) & 0x1FFu);
        n = n < R.cap ? n : R.cap;
        if (A.planes) {
            pln_vec* out = reinterpret_cast<pln_vec*>(reinterpret_cast<char*>(A.planes) + (size_t)j * A.stride * (DT == 0 ? 4 : 2));
            const int rep = (int)((w7 >> 32) & 0xFFu);
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
    } else if (A.planes) {
        pln_vec* out = reinterpret_cast<pln_vec*>(reinterpret_cast<char*>(A.planes) + (size_t)j * A.stride * (DT == 0 ? 4 : 2));
        const pln_vec zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int st = 0; st < STORES; st++) pln_store<NT>(out + st * 64 + lane, zero);
    }
    if (lane == 0) {
        if (A.z) A.z[j] = valid ? R.ring_z[slot] : 0.f;
        if (A.slot) A.slot[j] = valid ? slot : -1;
    }
    if (!A.pi_dense && !A.pi_index && !A.pi) return;

    // the target: entry k < n at logits-row element a (mirrored on a BLACK-to-move position in the
    // side-to-move view) with value visits_k / sum visits
    const bool mir = A.persp && !(meta & M_WHITE);
    const size_t e = (size_t)slot * R.cap, o = (size_t)j * R.cap;
    const int chunks = (R.cap + 63) >> 6;
    long long sum = 0;
    for (int c = 0; c < chunks; c++) {
        const int s = c * 64 + lane;
        if (s < n) sum += R.ring_vis[e + s];
    }
    sum = rpl_wave_sum(sum);
    const float fsum = (float)sum;
    float* row = reinterpret_cast<float*>(dense[wv]);
    if (A.pi_dense) {
        const pln_vec zero = {0u, 0u, 0u, 0u};
        for (int v = lane; v < RPL_ROW_VECS; v += 64) dense[wv][v] = zero;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the zeros are in LDS before another lane's entry lands
    }
    for (int c = 0; c < chunks; c++) {
        const int s = c * 64 + lane;
        if (s >= R.cap) break;
        const bool on = s < n;
        const u32 a = on ? R.ring_act[e + s] : RPL_NO_ACTION;
        const int v = on ? R.ring_vis[e + s] : 0;
        const bool ok = a < (u32)RPL_ROW;  // (anything else has no element in a logits row)
        const int at = ok ? (int)(mir ? pol_mirror(a) : a) : -1;
        const float val = ok && sum > 0 ? (float)v / fsum : 0.f;
        if (A.pi_index) A.pi_index[o + s] = at;
        if (A.pi) A.pi[o + s] = val;
        if (A.pi_dense && ok) row[at] = val;
    }
    if (A.pi_dense) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the entries are in LDS before the row is read
        pln_vec* out = reinterpret_cast<pln_vec*>(A.pi_dense + (size_t)j * A.pi_stride);
        for (int v = lane; v < RPL_ROW_VECS; v += 64) pln_store<NT>(out + v, dense[wv][v]);
    }
}
