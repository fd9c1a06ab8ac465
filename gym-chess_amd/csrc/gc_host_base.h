// gc_host_base.h -- the C-ABI's error state and input checks (plain C++, no HIP).
#pragma once
#include <cstdint>
#include <string>

static thread_local std::string g_err;
static int fail(const std::string& m) {
    g_err = m;
    return -1;
}

static int check_boards(int n, const int8_t* boards) {
    for (size_t k = 0; k < (size_t)64 * n; k++)
        if (boards[k] < -6 || boards[k] > 6) return fail("piece id out of range [-6, 6] at index " + std::to_string(k));
    return 0;
}
