// TEST INFRASTRUCTURE ONLY: the host minimax with quiescence (quiesce_host.cpp: gc_minimax.h's
// recursion, the quiescence nest and the row) as a stand-alone program for AddressSanitizer and
// UndefinedBehaviorSanitizer, over seeded fuzz positions (tests/test_quiesce.py builds and runs it):
//   g++ -O1 -g -std=c++17 -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o quiesce_sanitize tests/core_host/quiesce_sanitize_main.cpp && ./quiesce_sanitize 24
// Exit 0 = the pruned and the full-width search agree on every row and no sanitizer report.
#include "quiesce_host.cpp"

#include <cstdio>
#include <cstdlib>

struct Rng {
    u64 s;
    u64 next() {  // splitmix64
        u64 z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int below(int n) { return (int)((next() >> 33) % (u64)n); }
};

// sparse random placement (few men: the full-width twin runs four capture plies below depth 2),
// kings optional or doubled (boards the reference accepts)
static void fuzz_board(Rng& r, int8_t* b, uint8_t* m) {
    static const int8_t ids[] = {2, 3, 4, 5, 6, 6, 6, -2, -3, -4, -5, -6, -6, -6};
    for (int k = 0; k < 64; k++) b[k] = 0;
    const int n = 2 + r.below(9);
    for (int k = 0; k < n; k++) b[r.below(64)] = ids[r.below(14)];
    const int mode = r.below(10);
    if (mode != 1) b[r.below(64)] = 1;
    if (mode != 2) b[r.below(64)] = -1;
    if (mode == 3) b[r.below(64)] = r.below(2) ? 1 : -1;
    for (int k = 0; k < 8; k++) m[k] = 0;
    for (int k = 0; k < 5; k++) m[k] = (uint8_t)r.below(2);
}

int main(int argc, char** argv) {
    const int boards = argc > 1 ? atoi(argv[1]) : 24;
    Rng r{2026};
    int fails = 0;
    long long pruned = 0, full = 0;
    for (int i = 0; i < boards; i++) {
        int8_t b[64];
        uint8_t m[8];
        fuzz_board(r, b, m);
        for (int depth = 1; depth <= 2; depth++) {
            const int quiesce = depth == 2 ? 4 : 1 + r.below(4);  // depth 2 / quiesce 4 on every board
            const int cap = 1 + r.below(96);
            static uint16_t act[2][96];
            static int32_t sc[2][96];
            int32_t o[3][4];
            float v[3];
            const uint64_t seed = 5 + (uint64_t)i;
            const uint32_t draw = (uint32_t)r.next();
            const int tb = i & 1, done = i % 13 == 12;
            qh_row(b, m, done, depth, quiesce, tb, seed, (uint32_t)i, draw, 1, 0, nullptr, nullptr, o[0], &v[0]);
            qh_row(b, m, done, depth, quiesce, tb, seed, (uint32_t)i, draw, 1, cap, act[0], sc[0], o[1], &v[1]);
            qh_row(b, m, done, depth, quiesce, tb, seed, (uint32_t)i, draw, 0, cap, act[1], sc[1], o[2], &v[2]);
            bool ok = true;
            for (int w = 1; w < 3; w++) {
                for (int k = 0; k < 3; k++) ok = ok && o[w][k] == o[0][k];
                ok = ok && v[w] == v[0];
            }
            for (int k = 0; k < cap; k++) ok = ok && act[0][k] == act[1][k] && sc[0][k] == sc[1][k];
            ok = ok && o[0][3] <= o[1][3] && o[1][3] <= o[2][3] && v[0] >= -1.0f && v[0] <= 1.0f;
            if (done) ok = ok && o[0][0] == 0 && o[0][1] == A_NONE && o[0][3] == 0;
            pruned += o[0][3];
            full += o[2][3];
            if (!ok) {
                fails++;
                fprintf(stderr, "board %d depth %d quiesce %d: count %d pick %d score %d nodes %d | %d %d %d %d | %d %d %d %d\n",
                        i, depth, quiesce, o[0][0], o[0][1], o[0][2], o[0][3], o[1][0], o[1][1], o[1][2], o[1][3], o[2][0],
                        o[2][1], o[2][2], o[2][3]);
            }
        }
    }
    printf("sanitized quiescence run: %d boards, nodes pruned %lld full %lld, fails %d\n", boards, pruned, full, fails);
    return fails ? 1 : 0;
}
