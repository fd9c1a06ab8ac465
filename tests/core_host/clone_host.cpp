// TEST INFRASTRUCTURE ONLY: the window-clone rule of gc_env.h (rep_clone_hdr / rep_clone_table,
// what k_clone_boards of gc_clone.h applies four lanes per entry) on host tables with the
// HostHist contract of core_host.cpp, driven through rep_commit (tests/test_clone_host.py).
#include <cstdint>
#include <vector>

#include "../../gym-chess_amd/csrc/gc_core.h"
#include "../../gym-chess_amd/csrc/gc_env.h"

using namespace gc;

struct CloneHist {  // one board's table (no spill table: the move-capped envs)
    std::vector<RepEntry> tabv;
    u32 g = 0;
    CloneHist() : tabv(HTAB, RepEntry{0, 0, 0, 0, 0, 0, 0, 0}) {}
    int bits() const { return HTAB_BITS; }
    u32 gen() const { return g; }
    void bump_gen() { g++; }
    RepEntry load(int p) const { return tabv[p]; }
    void store_hdr(int p, u64 h) { tabv[p].hdr = h; }
    void store(int p, const RepEntry& e) { tabv[p] = e; }
    u32 spill_mask() const { return 0; }
    u32 owner() const { return 0; }
    u64 sp_hdr(u32) const { return 0; }
    bool sp_cas(u32, u64&, u64) { return false; }
    void sp_set_hdr(u32, u64) {}
    void sp_put(u32, const Pos&) {}
    bool sp_same(u32, const Pos&) const { return false; }
    u32 sp_owner_gen(u32) const { return g; }
    void sp_claimed() {}
    void sp_fail() {}
};

struct Rng {
    u64 s;
    u64 next() {  // splitmix64
        u64 z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    u32 below(u32 n) { return (u32)(next() >> 33) % n; }
};

static Pos random_board(Rng& r) {
    Pos s;
    s.k = r.next(); s.q = r.next(); s.r = r.next(); s.b = r.next(); s.n = r.next(); s.p = r.next(); s.w = r.next();
    s.meta = 0;
    return s;
}

// one reversible ply's bookkeeping: the count rep_commit returns for board s
static int visit(CloneHist& h, const Pos& s, u32& hl, bool irrev = false) {
    RepProbe pr;
    rep_prefetch(h, s, pr);
    return rep_commit(h, s, pr, hl, irrev);
}

// an earlier game of `plies` plies over `pool` boards of its own, ended by an irreversible
// move unless `open` (its entries then stay live)
static void other_game(CloneHist& h, Rng& r, int pool, int plies, bool open) {
    std::vector<Pos> p(pool);
    for (auto& s : p) s = random_board(r);
    u32 hl = 0;
    for (int t = 0; t < plies; t++) visit(h, p[r.below((u32)pool)], hl);
    if (!open) visit(h, p[0], hl, true);
}

// Source: two finished games, then `plies` reversible plies over `pool` boards (revisits) under
// generation src_gen.  Destination: finished games and one open game under generation dst_gen.
// The source's window is cloned into the destination; then both continue with `more` plies over
// the same pool plus as many new boards, one irreversible ply, and 40 plies more.
// out: 0 entries copied, 1 the source's window length, 2 entries the destination held before
// that are live afterwards without being the source's entry of that slot, 3 the first step at
// which the counts differ (-1 none), 4 live entries of the destination after the clone, 5 the
// largest count seen while continuing, 6 / 7 live / dead entries the destination held before,
// 8 the destination's generation after the clone.
extern "C" int ch_scenario(uint64_t seed, int pool, int plies, int more, uint32_t src_gen, uint32_t dst_gen,
                           int64_t* out) {
    if (src_gen < 3 || dst_gen < 4) return -1;  // generation 0 is the empty table's
    Rng r{seed};
    CloneHist src, dst;
    src.g = src_gen - 2;
    other_game(src, r, 40, 90, false);
    other_game(src, r, 60, 150, false);
    dst.g = dst_gen - 3;
    other_game(dst, r, 80, 200, false);
    other_game(dst, r, 30, 60, false);
    other_game(dst, r, 120, 280, false);
    other_game(dst, r, 100, 260, true);
    if (src.gen() != src_gen || dst.gen() != dst_gen) return -2;

    std::vector<Pos> p(pool);
    for (auto& s : p) s = random_board(r);
    u32 hl_s = 0;
    for (int t = 0; t < plies; t++)
        if (visit(src, p[r.below((u32)pool)], hl_s) == 0) return -3;  // (the window filled up)

    const std::vector<RepEntry> before = dst.tabv;
    const u32 dg0 = dst.gen();
    out[0] = rep_clone_table(src, dst);
    out[1] = hl_s;
    out[8] = dst.gen();
    int64_t resurrected = 0, live_after = 0, live_before = 0, dead_before = 0;
    for (int pos = 0; pos < HTAB; pos++) {
        const RepEntry& b = before[pos];
        const RepEntry a = dst.load(pos), s = src.load(pos);
        const bool a_live = (u32)a.hdr == dst.gen(), s_live = (u32)s.hdr == src.gen();
        live_after += a_live;
        const bool held = (u32)b.hdr != 0;
        live_before += held && (u32)b.hdr == dg0;
        dead_before += held && (u32)b.hdr != dg0;
        const bool is_sources = s_live && (a.hdr >> 32) == (s.hdr >> 32) && a.k == s.k && a.q == s.q && a.r == s.r &&
                                a.b == s.b && a.n == s.n && a.p == s.p && a.w == s.w;
        if (a_live && !is_sources) resurrected++;
    }
    out[2] = resurrected;
    out[4] = live_after;
    out[6] = live_before;
    out[7] = dead_before;

    std::vector<Pos> fresh(pool);
    for (auto& s : fresh) s = random_board(r);
    u32 hl_d = hl_s;
    out[3] = -1;
    out[5] = 0;
    for (int t = 0; t < more + 41; t++) {
        const u32 k = r.below((u32)(2 * pool));
        const Pos& s = k < (u32)pool ? p[k] : fresh[k - pool];
        const bool irrev = t == more;
        const int cs = visit(src, s, hl_s, irrev), cd = visit(dst, s, hl_d, irrev);
        if (cs > out[5]) out[5] = cs;
        if ((cs != cd || hl_s != hl_d) && out[3] < 0) out[3] = t;
    }
    return 0;
}
