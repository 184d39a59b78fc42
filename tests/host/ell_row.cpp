// Host check of csrc/ell_row.hpp: the SELL-64 element index against the formula written out, and as
// a bijection from (row, column) onto the padded array, for row counts around the 64-row slice and
// the row widths 4, 8 and 32; the group base against the element index.
// tests/test_ell_row_host.py builds this with -fsanitize=address,undefined and runs it; exit
// status 0 and "ell_row: N checks, 0 failed".
#include <cstdio>
#include <vector>

#include "ell_row.hpp"

using namespace acs;

static_assert(ell_slot(uint64_t(65), 8, 5) == ((1 * 2 + 1) * 64 + 1) * 4 + 1, "usable in constant expressions");

static int g_checks = 0, g_failed = 0;

static void expect(bool ok, const char* what, uint64_t N, uint32_t dp, uint64_t i, uint32_t t) {
    ++g_checks;
    if (ok) return;
    ++g_failed;
    fprintf(stderr, "%s: N = %llu, dp = %u, i = %llu, t = %u\n", what, (unsigned long long)N, dp, (unsigned long long)i, t);
}

int main() {
    for (uint64_t N : {1ull, 63ull, 64ull, 65ull, 130ull})
        for (uint32_t dp : {4u, 8u, 32u}) {
            const uint64_t words = ((N + 63) / 64) * 64 * dp;   // what a handle allocates for the array
            std::vector<uint8_t> hit(words, 0);   // (indexing it past `words` is the sanitizer's to catch)
            for (uint64_t i = 0; i < N; ++i)
                for (uint32_t t = 0; t < dp; ++t) {
                    const uint64_t e = ell_slot(i, dp, t);
                    expect(e == (((i >> 6) * (dp >> 2) + (t >> 2)) * 64 + (i & 63)) * 4 + (t & 3), "ell_slot != the formula", N, dp, i, t);
                    expect(e == ell_slot((uint32_t)i, dp, t), "ell_slot of a 32-bit row differs", N, dp, i, t);
                    expect(e < words, "ell_slot outside the array", N, dp, i, t);
                    if (e < words) {
                        expect(!hit[e], "ell_slot hit twice", N, dp, i, t);
                        hit[e] = 1;
                    }
                    // group q = t / 4 of the row, element t % 4 of the group
                    expect(e == (ell_group0((uint32_t)i, (int)(dp / 4)) + (uint64_t)(t >> 2) * 64) * 4 + (t & 3),
                           "ell_group0 disagrees with ell_slot", N, dp, i, t);
                }
            // N * dp distinct indices below `words`; when N fills its slices they are all of them
            uint64_t n = 0;
            for (uint8_t h : hit) n += h;
            expect(n == N * dp, "not an injection", N, dp, 0, 0);
            if (N % 64 == 0) expect(n == words, "not onto", N, dp, 0, 0);
        }
    fprintf(stderr, "ell_row: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
