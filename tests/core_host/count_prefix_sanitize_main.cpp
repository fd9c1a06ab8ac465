// TEST INFRASTRUCTURE ONLY: the checks of count_prefix_host.cpp (the makers' prefix words,
// sw_locate_pre, the pick from fetched sets of gc_core.h) over seeded random sets, as a
// stand-alone program for AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_count_prefix.py builds and runs it):
//   g++ -O1 -g -std=c++17 -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o count_prefix_sanitize tests/core_host/count_prefix_sanitize_main.cpp && ./count_prefix_sanitize
// Exit 0 = every check agrees and no sanitizer report.
#include "count_prefix_host.cpp"

#include <cstdio>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// a set of about `bits` squares
static uint64_t some_set(int bits) {
    uint64_t x = 0;
    for (int i = 0; i < bits; i++) x |= 1ull << (rnd() & 63);
    return x;
}

int main() {
    int fails = 0;
    int64_t ranks[1] = {0}, first[2] = {0, 0};
    // below 256 moves: the words, the located set, the pick
    std::vector<uint64_t> cases;
    int n = 0;
    for (int rep = 0; rep < 400; rep++) {
        uint64_t t[SW_SETS];
        int total = 0;
        for (int j = 0; j < SW_SETS; j++) {
            t[j] = rep % 7 == 0 && j == rep % SW_SETS ? ~0ull : some_set((int)(rnd() % (rep % 4 == 0 ? 3 : 12)));
            if (rnd() % 5 == 0) t[j] = 0;
            total += popc(t[j]);
            if (total > 255) { total -= popc(t[j]); t[j] = 0; }
        }
        cases.insert(cases.end(), t, t + SW_SETS);
        n++;
        fails += cp_pick_sets(t, rnd(), rep & 1, rep & 3, ranks, first) != 0;
    }
    fails += cp_words(cases.data(), n, first) != 0;
    fails += cp_locate(cases.data(), n, ranks, first) != 0;
    // 256 moves and more: the scan
    for (int rep = 0; rep < 40; rep++) {
        uint64_t t[SW_SETS];
        for (int j = 0; j < SW_SETS; j++) t[j] = rep % 8 == 7 ? ~0ull : some_set(20 + rep);
        fails += cp_pick_sets(t, rnd(), rep & 1, rep & 3, ranks, first) != 0;
    }
    printf("sanitized count-prefix run: %lld ranks, fails %d\n", (long long)ranks[0], fails);
    return fails ? 1 : 0;
}
