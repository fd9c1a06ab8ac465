// gc_playout.h -- random-playout leaf values (gc_playout_run, include/gymchess.h): for a device
// list of boards, P bounded random playouts per board from a private copy of its position, and
// the mean outcome -- the leaf evaluator of a search that runs without a network.
//
// The first half compiles for the host too (tests/core_host/playout_host.cpp): the playout of
// ONE lane (playout_lane), built on gc_env.h's env_step<false> and selfplay_pick and on nothing
// else, the material term of a cut-off and the value formula.  The second half is the device's:
// the private 3-fold window (PlayHist) and the kernel (k_playout).
//
// Mapping: one lane per playout, lane L = row * P + p, so the P lanes of a row are contiguous and
// a wave holds 64 / P rows.  A lane loads its board once (SoA::load, read-only), plays until its
// playout ends, and the wave leaves the ply loop when a ballot shows no lane alive; the six
// tallies of a row are then summed over its P lanes by lane shuffles (xor butterflies inside the
// row's group of lanes) and the row's first lane stores them.  No atomics, no LDS beyond the
// move-target scratch every step kernel uses.  At search sizes the launch is latency-bound
// (1 024 rows x 8 playouts are 128 waves on 1 024 SIMDs): its time is that of the longest
// playout of the slowest wave, one lane's ply after another.
//
// The pick.  After a step env_step leaves the new position's generation state in `g` (pins, check
// mask, castles), and the self-play policy ranks over the 28 move SETS built from it (gc_core.h
// sw_gen / sw_select): the next action is selfplay_pick_gen(s, g, pc) -- selfplay_pick without
// its own gen_init, the one place the move-set order is stated.  The step itself is asked for the
// move COUNT only (env_step<false, 1>: mate needs it), not for the per-piece move set nobody reads.
#pragma once

namespace gc {

// how a playout ended
enum { PO_WIN = 0, PO_LOSS = 1, PO_OTHER = 2, PO_CUT = 3 };
static constexpr int PLAYOUT_MAX_PLIES = 128;
static constexpr int PLAYOUT_MAX_P = 64;
static constexpr int PLAYOUT_TALLY = 6;  // wins, losses, other endings, cut-offs, sum of m, sum of plies

// The private window's table: 2^PLAY_BITS entries of 64 bytes per lane.  A playout adds at most
// one board per ply, so at the longest playout (PLAYOUT_MAX_PLIES) the load is 0.5 and the
// window length never reaches hist_cap.  Not smaller for shorter playouts: an entry's header
// keeps the key's bits above the slot index in 24 bits (bits 32..55, the count sits above
// them), so rep_commit's tag needs a table of at least 2^8 entries.
static constexpr int PLAY_BITS = 8;
static_assert((1 << PLAY_BITS) >= 2 * PLAYOUT_MAX_PLIES, "load <= 0.5 at the longest playout");
static_assert(32 - PLAY_BITS <= 24, "the tag fits below the count (RepEntry::hdr)");

struct PlayoutEnd {
    int kind;   // PO_*
    int plies;  // env steps taken
    int m;      // the material term of a cut-off, else 0
};

// the material term of a cut-off: clamp(sum of value * (own - enemy), -16, 16), in apply_move's
// capture values (Q 10, R 5, B 3, N 3, P 1); own = the side to move at the START of the playout
GC_HD int playout_material(const Pos& s, bool own_white) {
    const u64 occ = s.k | s.q | s.r | s.b | s.n | s.p;
    const u64 own = own_white ? s.w : occ & ~s.w, opp = occ & ~own;
    const int d = 10 * (popc(s.q & own) - popc(s.q & opp)) + 5 * (popc(s.r & own) - popc(s.r & opp)) +
                  3 * (popc((s.b | s.n) & own) - popc((s.b | s.n) & opp)) + (popc(s.p & own) - popc(s.p & opp));
    return d < -16 ? -16 : (d > 16 ? 16 : d);
}

// a row's value from its tally, each operation rounded on its own (no fused multiply-add: the
// host build and the device agree bit for bit)
GC_HD float playout_value(int wins, int losses, int msum, float cut_weight, int P) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float cut = cut_weight * ((float)msum * 0.0625f);
    return ((float)(wins - losses) + cut) / (float)P;
}

struct PlayoutNoTrace {
    GC_HDM void operator()(int, int, int) const {}
};
struct PlayoutOneLane {
    GC_HDM bool operator()(bool alive) const { return alive; }
};

// One playout: from position `s` (the caller emptied `hist` and set s's window length to 0) up
// to n_plies plies of the random self-play policy on the stream `pc`, each applied by
// env_step<false>.  Ends at the first of: R_MATE at ply t (a win for the side to move at the
// start if t is even, else a loss); any other done of the step, or no legal move (A_NONE picked,
// no draw taken): PO_OTHER; n_plies plies played: PO_CUT with the material term.
// `alive` false: the lane plays nothing (kind PO_OTHER, 0 plies; the caller ignores it) but keeps
// the loop's company.  any(alive): whether the loop goes on -- the lane itself on the host, a
// wave-wide ballot on the device.  trace(ply, action, reason) sees every step.
template <class H, class S, class ANY = PlayoutOneLane, class TR = PlayoutNoTrace>
GC_HD PlayoutEnd playout_lane(Pos s, H& hist, S& scr, PolicyCtx& pc, int n_plies, bool alive, ANY any = ANY{},
                              TR trace = TR{}) {
    PlayoutEnd r = {PO_OTHER, 0, 0};
    const bool own_white = s.meta & M_WHITE;
    int a = alive ? selfplay_pick(s, pc) : A_NONE;
    if (a == A_NONE) alive = false;  // no legal move: an other ending after 0 plies
    Gen g;
    MoveSet ms;
    while (any(alive)) {
        if (!alive) continue;
        const StepOut o = env_step<false, 1>(s, hist, a, nullptr, g, ms, scr);  // ms: the count only
        hist.commit();  // the ply's table write lands before the next ply probes the table
        trace(r.plies, a, o.reason);
        r.plies++;
        if (o.done) {
            r.kind = o.reason == R_MATE ? ((r.plies & 1) ? PO_WIN : PO_LOSS) : PO_OTHER;
            alive = false;
        } else if (r.plies >= n_plies) {
            r.kind = PO_CUT;
            r.m = playout_material(s, own_white);
            alive = false;
        } else {
            a = selfplay_pick_gen(s, g, pc);  // g: the new position's, from the step
            if (a == A_NONE) alive = false;   // r.kind is PO_OTHER
        }
    }
    return r;
}

}  // namespace gc

#if defined(__HIPCC__)
// ----------------------------------------------------------------------------- device side
// The private window of lane L: DevHist's table entry, deferred store_hdr / store / commit and
// generation word, on the handle's scratch instead of the env's tables -- wave-blocked the same
// way (entry pos of lane L at ((L / 64) * 2^PLAY_BITS + pos) * 64 + L % 64) -- and without a spill
// table, at compile time.  Every lane keeps its generation word in the scratch across calls; a
// run starts by bumping it, so the entries of earlier runs are dead and nothing is cleared.
struct PlayHist : DevHist {
    __device__ PlayHist(u64* tab, u32* gen, u32 g, int lane) : DevHist{tab, gen, g, lane, gc::PLAY_BITS} {}
    __device__ u32 spill_mask() const { return 0; }
};

// the scratch of a handle for `lanes` lanes (a multiple of 64): the tables, then the generations
static inline size_t playout_tab_words(size_t lanes) { return (lanes << gc::PLAY_BITS) * 8; }
static inline size_t playout_scratch_bytes(size_t lanes) { return playout_tab_words(lanes) * 8 + lanes * 4; }

struct PlayArgs {
    const int32_t* idx;  // [rows] or null (board j)
    int rows;
    int logp;            // P = 1 << logp
    int n_plies;
    uint64_t seed;
    u32 draw;
    float cut_weight;
    float* value;        // [rows] or null
    int32_t* tally;      // [rows][PLAYOUT_TALLY] or null
    u64* tab;            // the scratch: tables
    u32* gen;            //              generation per lane
};

#define PLAYOUT_BLOCK 64  // a wave per workgroup, as the rows kernels (gc_step_rows.h: measured there)

__global__ void __launch_bounds__(BLOCK) k_playout(SoA st, PlayArgs a) {
    LDS_SCRATCH_DECL;
    const int L = blockIdx.x * blockDim.x + threadIdx.x;
    const int P = 1 << a.logp, j = L >> a.logp;
    if (j >= a.rows) return;  // whole rows: the lanes of a row stay together
    const int b = a.idx ? a.idx[j] : j;
    bool alive = (u32)b < (u32)st.n;
    Pos s = st.load(alive ? b : 0);
    u32 g0 = a.gen[L];
    pin(s); pin(g0);
    alive = alive && !(s.meta & M_DONE);
    PlayHist h(a.tab, a.gen, g0, L);
    h.bump_gen();  // the window starts empty
    s.meta = with_hl(s.meta, 0);
    PolicyCtx pc = {a.seed, (u32)L, a.draw};
    const PlayoutEnd r = playout_lane(s, h, scr, pc, a.n_plies, alive, [](bool x) { return __ballot(x) != 0; });
    if (alive) h.flush(g0);
    // wins | losses << 8 | others << 16 | cut-offs << 24: each at most P <= 64
    u32 cnt = alive ? 1u << (8 * r.kind) : 0u;
    int msum = alive ? r.m : 0, plies = alive ? r.plies : 0;
    for (int off = P >> 1; off; off >>= 1) {
        cnt += (u32)__shfl_xor((int)cnt, off);
        msum += __shfl_xor(msum, off);
        plies += __shfl_xor(plies, off);
    }
    if (L & (P - 1)) return;
    const int wins = cnt & 0xFF, losses = (cnt >> 8) & 0xFF;
    if (a.tally) {
        int32_t* t = a.tally + (size_t)PLAYOUT_TALLY * j;
        t[0] = wins; t[1] = losses; t[2] = (cnt >> 16) & 0xFF; t[3] = cnt >> 24; t[4] = msum; t[5] = plies;
    }
    if (a.value) a.value[j] = playout_value(wins, losses, msum, a.cut_weight, P);
}
#endif
