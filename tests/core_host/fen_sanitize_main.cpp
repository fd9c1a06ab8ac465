// TEST INFRASTRUCTURE ONLY: the product's FEN codec (gym-chess_amd/csrc/gc_fen.h, plain C++)
// under AddressSanitizer and UndefinedBehaviorSanitizer.  Valid input: the start position and
// seeded random states, state -> FEN -> state under both rule sets.  Malformed input: the
// strings tests/test_fen.py lists and over-long ranks (all must be refused with a message), and
// seeded mutations of valid FENs -- truncation at every length, one byte replaced by each of
// \x01..\xff -- which the codec may accept or refuse, but a refusal carries a message and what
// it accepts encodes again.  Exit 0 = no mismatch and no sanitizer report (sanitizers abort:
// -fno-sanitize-recover=all).
#include "../../gym-chess_amd/csrc/gc_fen.h"

#include <cstdio>
#include <vector>

static uint64_t rng_state = 0xFE2FE2ull;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}

static int fails = 0;
#define CHECK(c, ...)                        \
    do {                                     \
        if (!(c)) {                          \
            fprintf(stderr, __VA_ARGS__);    \
            fputc('\n', stderr);             \
            if (++fails > 20) exit(1);       \
        }                                    \
    } while (0)

// what FEN carries of a state: pieces, side, rights; meta[7] = move_count (reference) or the
// en-passant file + 1 (FIDE)
static void random_state(int8_t* b, uint8_t* m, int rules) {
    memset(b, 0, 64);
    const int k = (int)rnd(40);
    for (int j = 0; j < k; j++) b[rnd(64)] = (int8_t)((int)rnd(13) - 6);
    memset(m, 0, 8);
    for (int j = 0; j < 5; j++) m[j] = (uint8_t)rnd(2);
    m[7] = (uint8_t)(rules ? rnd(9) : rnd(256));
}

// a parse in a heap buffer of exactly the string's size (so ASan sees any read past its end)
static int parse(const std::string& fen, int8_t* b, uint8_t* m, int rules) {
    std::vector<char> z(fen.begin(), fen.end());
    z.push_back('\0');
    g_err.clear();
    return gc_fen_to_state_rules(z.data(), b, m, rules);
}

static void must_refuse(const std::string& fen, int rules) {
    int8_t b[64];
    uint8_t m[8];
    const int rc = parse(fen, b, m, rules);
    CHECK(rc != 0 && !g_err.empty(), "accepted (rules %d, rc %d, message '%s'): '%s'", rules, rc, g_err.c_str(), fen.c_str());
}

// accepted or refused; a refusal has a message, an accepted state encodes again
static void may_refuse(const std::string& fen, int rules) {
    int8_t b[64];
    uint8_t m[8];
    char out[128];
    const int rc = parse(fen, b, m, rules);
    if (rc != 0) CHECK(!g_err.empty(), "refused without a message (rules %d)", rules);
    else CHECK(gc_state_to_fen_rules(b, m, out, (int)sizeof out, rules) == 0, "accepted state does not encode: %s", g_err.c_str());
}

int main(int argc, char** argv) {
    const int states = argc > 1 ? atoi(argv[1]) : 3000;
    int8_t b[64], b2[64];
    uint8_t m[8], m2[8];
    char out[128];
    std::vector<std::string> valid;

    const char* START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1";
    for (int rules = 0; rules < 2; rules++) {
        CHECK(parse(START, b, m, rules) == 0, "start position refused: %s", g_err.c_str());
        CHECK(b[0] == -3 && b[4] == -1 && b[60] == 1 && b[63] == 3 && m[0] == 1 && m[1] && m[2] && m[3] && m[4] && m[7] == 0,
              "start position decoded wrongly");
        CHECK(gc_state_to_fen_rules(b, m, out, (int)sizeof out, rules) == 0 && std::string(out) == START,
              "start position encoded as '%s'", out);
    }
    for (int i = 0; i < states; i++) {
        const int rules = i & 1;
        random_state(b, m, rules);
        CHECK(gc_state_to_fen_rules(b, m, out, (int)sizeof out, rules) == 0, "encode failed: %s", g_err.c_str());
        const std::string fen(out);
        CHECK(parse(fen, b2, m2, rules) == 0, "own FEN refused: %s", g_err.c_str());
        CHECK(memcmp(b, b2, 64) == 0 && memcmp(m, m2, 8) == 0, "round trip differs (rules %d): %s", rules, fen.c_str());
        CHECK(gc_state_to_fen_rules(b, m, out, (int)fen.size(), rules) != 0 && !g_err.empty(), "short buffer accepted");
        if (valid.size() < 16) valid.push_back(fen);
    }
    b[rnd(64)] = 7;
    CHECK(gc_state_to_fen_rules(b, m, out, (int)sizeof out, 0) != 0 && !g_err.empty(), "piece id 7 encoded");

    // the malformed strings of tests/test_fen.py
    const char* BAD[] = {"", "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP", "rnbqkbnr/ppppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR",
                         "rnbqkbnr/pppppppp/9/8/8/8/PPPPPPPP/RNBQKBNR", "rnbqkbnr/pppxpppp/8/8/8/8/PPPPPPPP/RNBQKBNR",
                         "8/8/8/8/8/8/8/8 x - - 0 1", "8/8/8/8/8/8/8/8 w KZ - 0 1", "8/8/8/8/8/8/8/8 w - - 0 zz"};
    for (const char* bad : BAD)
        for (int rules = 0; rules < 2; rules++) must_refuse(bad, rules);

    long mutants = 0;
    for (size_t v = 0; v < valid.size(); v++) {
        const std::string& fen = valid[v];
        const int rules = (int)(v & 1);  // (the rule set it was written under)
        for (size_t len = 0; len < fen.size(); len++, mutants++) may_refuse(fen.substr(0, len), rules);
        for (size_t at = 0; at < fen.size(); at++)
            for (int c = 1; c < 256; c++, mutants++) {
                std::string x = fen;
                x[at] = (char)c;
                may_refuse(x, rules);
            }
        // over-long ranks: one more piece, or one more empty square, in a rank
        const size_t placement = fen.find(' ');
        for (int k = 0; k < 8; k++, mutants += 2) {
            size_t at = 0;  // the start of rank k
            for (int r = 0; r < k; r++) at = fen.find('/', at) + 1;
            must_refuse(std::string(fen).insert(at, "Q"), rules);
            must_refuse(std::string(fen).insert(at, "1"), rules);
            CHECK(at < placement, "rank %d not found in '%s'", k, fen.c_str());
        }
        must_refuse(std::string(fen).insert(0, "8/"), rules);  // a ninth rank
    }
    printf("states %d mutants %ld fails %d\n", states, mutants, fails);
    return fails ? 1 : 0;
}
