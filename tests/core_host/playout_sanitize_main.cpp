// TEST INFRASTRUCTURE ONLY: the host playout body (playout_host.cpp: gc_playout.h's playout_lane
// on a plain-array window) as a stand-alone program for AddressSanitizer and
// UndefinedBehaviorSanitizer, over seeded fuzz positions (tests/test_playout.py builds and runs it):
//   g++ -O1 -g -std=c++17 -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o playout_sanitize tests/core_host/playout_sanitize_main.cpp && ./playout_sanitize 300
// Exit 0 = every row's tally is consistent and no sanitizer report.
#include "playout_host.cpp"

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

// sparse random placement, kings optional or doubled (boards the reference accepts)
static void fuzz_board(Rng& r, int8_t* b, uint8_t* m) {
    static const int8_t ids[] = {2, 3, 4, 5, 6, 6, 6, -2, -3, -4, -5, -6, -6, -6};
    for (int k = 0; k < 64; k++) b[k] = 0;
    const int n = 2 + r.below(24);
    for (int k = 0; k < n; k++) b[r.below(64)] = ids[r.below(14)];
    const int mode = r.below(10);
    if (mode != 1) b[r.below(64)] = 1;
    if (mode != 2) b[r.below(64)] = -1;
    if (mode == 3) b[r.below(64)] = r.below(2) ? 1 : -1;
    for (int k = 0; k < 8; k++) m[k] = 0;
    for (int k = 0; k < 5; k++) m[k] = (uint8_t)r.below(2);
    m[7] = (uint8_t)(r.below(4) ? 0 : 140 + r.below(12));  // some boards close to the move cap
}

int main(int argc, char** argv) {
    const int boards = argc > 1 ? atoi(argv[1]) : 300;
    Rng r{2024};
    int fails = 0;
    long long ends[4] = {0, 0, 0, 0};
    static int32_t act[64 * 128], fin[64 * 3];
    static uint8_t why[64 * 128];
    for (int i = 0; i < boards; i++) {
        int8_t b[64];
        uint8_t m[8];
        fuzz_board(r, b, m);
        static const int shapes[][2] = {{8, 48}, {1, 128}, {64, 5}, {4, 1}};
        for (const auto& sh : shapes) {
            const int P = sh[0], plies = sh[1];
            int32_t tally[6];
            float value;
            const int skipped = ph_row(b, m, i % 17 == 16, 77 + (uint64_t)i, (uint32_t)(i * P), P, (uint32_t)r.next(), plies,
                                       0.5f, act, why, fin, tally, &value);
            bool ok = value >= -1.0f && value <= 1.0f;
            if (skipped) {
                for (int k = 0; k < 6; k++) ok = ok && tally[k] == 0;
            } else {
                ok = ok && tally[0] + tally[1] + tally[2] + tally[3] == P && tally[5] >= 0 && tally[5] <= P * plies &&
                     tally[4] >= -16 * tally[3] && tally[4] <= 16 * tally[3];
                for (int p = 0; p < P; p++) {
                    const int kind = fin[3 * p], n = fin[3 * p + 1];
                    ok = ok && kind >= 0 && kind <= 3 && n >= 0 && n <= plies && (kind != PO_CUT || n == plies);
                    for (int k = 0; k < plies; k++) ok = ok && ((k < n) == (act[p * plies + k] >= 0));
                    if (kind >= 0 && kind <= 3) ends[kind]++;
                }
            }
            if (!ok) {
                fails++;
                fprintf(stderr, "board %d P %d plies %d: tally %d %d %d %d %d %d value %g\n", i, P, plies, tally[0], tally[1],
                        tally[2], tally[3], tally[4], tally[5], (double)value);
            }
        }
    }
    printf("sanitized playout run: %d boards, wins %lld losses %lld others %lld cuts %lld, fails %d\n", boards, ends[0],
           ends[1], ends[2], ends[3], fails);
    return fails ? 1 : 0;
}
