// TEST INFRASTRUCTURE ONLY, run by hand (not part of the suite): the window-clone scenarios of
// clone_host.cpp (rep_clone_hdr / rep_clone_table of gc_env.h) as a stand-alone program for
// AddressSanitizer and UndefinedBehaviorSanitizer:
//   g++ -O1 -g -std=c++17 -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o clone_sanitize tests/core_host/clone_sanitize_main.cpp && ./clone_sanitize
// Exit 0 = every scenario agrees and no sanitizer report.
#include "clone_host.cpp"

#include <cstdio>

int main() {
    static const uint32_t gens[][2] = {{9, 4}, {9, 9}, {9, 40}, {1000, 5}, {5, 1000}, {0xFFFFFF00u, 7}, {7, 0xFFFFFFFEu}};
    static const int shapes[][3] = {{150, 400, 200}, {300, 600, 120}, {1, 5, 30}, {2, 1, 30}};
    int fails = 0, runs = 0;
    for (const auto& g : gens)
        for (const auto& s : shapes)
            for (uint64_t seed = 1; seed <= 8; seed++, runs++) {
                int64_t out[9];
                const int rc = ch_scenario(seed * 977 + (uint64_t)s[0], s[0], s[1], s[2], g[0], g[1], out);
                const bool ok = rc == 0 && out[0] == out[1] && out[4] == out[1] && out[2] == 0 && out[3] == -1 &&
                                (uint32_t)out[8] == g[1] + 1u;
                if (!ok) {
                    fails++;
                    fprintf(stderr, "gens %u %u shape %d %d %d seed %llu: rc %d copied %lld hl %lld resurrected %lld diff %lld\n",
                            g[0], g[1], s[0], s[1], s[2], (unsigned long long)seed, rc, (long long)out[0], (long long)out[1],
                            (long long)out[2], (long long)out[3]);
                }
            }
    printf("sanitized clone run: %d scenarios, fails %d\n", runs, fails);
    return fails ? 1 : 0;
}
