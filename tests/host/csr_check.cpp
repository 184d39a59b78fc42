// Host check of csrc/csr_check.hpp: every input acs_create_csr / acs_create_csr_weighted refuse
// before a handle exists, with the exact code and message, and the inputs on the edge of those
// checks that must pass.  tests/test_csr_check_host.py builds this with
// -fsanitize=address,undefined and runs it; exit status 0 and "csr_check: N checks, 0 failed".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "csr_check.hpp"

using namespace acs;

static int g_checks = 0, g_failed = 0;

struct Graph {
    std::vector<uint64_t> rowptr;
    std::vector<uint32_t> colidx;
    std::vector<double> wself, wedge;
};

static acs_config config(uint64_t n, uint32_t rule, uint32_t trim = 0, uint32_t dtype = ACS_F64) {
    acs_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.n_nodes = n;
    c.n_instances = 1;
    c.topology = ACS_TOPO_CSR;
    c.rule = rule;
    c.trim = trim;
    c.dtype = dtype;
    return c;
}

// arrays first, then (weighted rules) the weights: create_impl's order
static CsrCheck run(const acs_config& c, const Graph& g) {
    CsrCheck r;
    if (csr_check_arrays(r, c, g.rowptr.data(), g.colidx.data())) return r;
    if (c.rule == ACS_RULE_WEIGHTED || c.rule == ACS_RULE_PUSHSUM)
        csr_check_weights(r, c, g.rowptr.data(), g.colidx.data(), g.wself.data(), g.wedge.data());
    return r;
}

static void expect(const char* what, const CsrCheck& r, int code, const char* message) {
    ++g_checks;
    if (r.code == code && r.message == message) return;
    ++g_failed;
    fprintf(stderr, "%s: got (%d, \"%s\"), want (%d, \"%s\")\n", what, r.code, r.message.c_str(), code, message);
}

static void expect_ok(const char* what, const CsrCheck& r, uint64_t mmax, uint64_t nnz) {
    ++g_checks;
    if (r.code == ACS_OK && r.message.empty() && r.mmax == mmax && r.nnz == nnz) return;
    ++g_failed;
    fprintf(stderr, "%s: got (%d, \"%s\", mmax %llu, nnz %llu), want ok with mmax %llu, nnz %llu\n", what, r.code,
            r.message.c_str(), (unsigned long long)r.mmax, (unsigned long long)r.nnz, (unsigned long long)mmax,
            (unsigned long long)nnz);
}

// 3 nodes: row 0 <- {1, 2}, row 1 <- {0}, row 2 <- {0, 1}; every weight 0.25
static Graph small() {
    Graph g;
    g.rowptr = {0, 2, 3, 5};
    g.colidx = {1, 2, 0, 0, 1};
    g.wself = {0.25, 0.25, 0.25};
    g.wedge = {0.25, 0.25, 0.25, 0.25, 0.25};
    return g;
}

static void rejected_arrays() {
    Graph g = small();
    g.rowptr[0] = 1;
    expect("rowptr[0] != 0", run(config(3, ACS_RULE_AVERAGE), g), ACS_EINVAL, "rowptr[0] must be 0");
    g = small();
    g.rowptr = {0, 3, 2, 5};
    expect("decreasing rowptr", run(config(3, ACS_RULE_AVERAGE), g), ACS_EINVAL, "rowptr must be non-decreasing");
    g = small();   // row 1 has m = 2 entries: t = 1 needs m > 2
    expect("m <= 2t", run(config(3, ACS_RULE_TRIMMED_MEAN, 1), g), ACS_EINVAL, "receiver 1 has m = 2 <= 2t");
    expect_ok("AVERAGE ignores m <= 2t", run(config(3, ACS_RULE_AVERAGE, 0), g), 3, 5);
    g.colidx[3] = 3;
    expect("colidx out of range", run(config(3, ACS_RULE_AVERAGE), g), ACS_EINVAL, "colidx[3] out of range");
}

static void rejected_weights() {
    const acs_config w64 = config(3, ACS_RULE_WEIGHTED), w32 = config(3, ACS_RULE_WEIGHTED, 0, ACS_F32);
    Graph g = small();
    g.wself[2] = NAN;
    expect("NaN w_self", run(w64, g), ACS_EINVAL, "w_self[2] must be finite, in [0, 1]");
    g = small();
    g.wedge[4] = NAN;
    expect("NaN w_edge", run(w64, g), ACS_EINVAL, "w_edge[4] must be finite, in [0, 1]");
    g = small();
    g.wedge[1] = -0.5;
    expect("negative w_edge", run(w64, g), ACS_EINVAL, "w_edge[1] must be finite, in [0, 1]");
    g = small();
    g.wself[0] = -1e-300;
    expect("negative w_self", run(w64, g), ACS_EINVAL, "w_self[0] must be finite, in [0, 1]");
    g = small();
    g.wedge[2] = 1.0 + 0x1p-52;
    expect("w_edge > 1", run(w64, g), ACS_EINVAL, "w_edge[2] must be finite, in [0, 1]");
    g = small();
    g.wself[1] = INFINITY;
    expect("infinite w_self", run(w64, g), ACS_EINVAL, "w_self[1] must be finite, in [0, 1]");
    g = small();   // row 1: w_self and its only edge are 0
    g.wself[1] = 0.0;
    g.wedge[2] = -0.0;
    expect("zero row sum, fp64", run(w64, g), ACS_EINVAL, "receiver 1: the row's weights sum to 0");
    g.wself[1] = 1e-60;   // positive in fp64, 0 once rounded to binary32
    g.wedge[2] = 1e-50;
    expect_ok("tiny positive row, fp64", run(w64, g), 3, 5);
    expect("zero row sum after binary32 rounding", run(w32, g), ACS_EINVAL,
           "receiver 1: the row's weights sum to 0 after rounding to binary32");
}

static void pushsum_columns() {
    const acs_config p64 = config(3, ACS_RULE_PUSHSUM), p32 = config(3, ACS_RULE_PUSHSUM, 0, ACS_F32);
    // column 0 = w_self[0] + w_edge[2] + w_edge[3]
    Graph g = small();
    g.wself[0] = 0.5;
    g.wedge[2] = 0.25;
    g.wedge[3] = 0.25 + 0x1p-30;
    expect_ok("column sum of exactly 1 + 2^-30", run(p64, g), 3, 5);
    g.wedge[3] = 0.25 + 0x1p-29;
    char want[256];
    snprintf(want, sizeof want, "sender 0: column sum %.17g > 1 + 2^-30 (PUSHSUM must not create mass)", 1.0 + 0x1p-29);
    expect("column sum of 1 + 2^-29", run(p64, g), ACS_EINVAL, want);
    expect_ok("the same weights under WEIGHTED", run(config(3, ACS_RULE_WEIGHTED), g), 3, 5);
    // binary32: 0.25 + 2^-29 rounds to 0.25, and the column then sums to 1
    expect_ok("1 + 2^-29 before rounding, 1 after", run(p32, g), 3, 5);
    // The other way round: node 0 sends to nodes 1..3; its column is (1 - 3 * 2^-11) + e1 + e2 + e3 with
    // e = 2^-11 + {2^-31, 2^-32, 2^-32} + {5/8, -5/16, -5/16} u, u = 2^-34 the binary32 spacing there.
    // Every sum is exact in binary64: 1 + 2^-30 as given, and 1 + 2^-30 + u once e1 has rounded up.
    const double u = 0x1p-34;
    Graph h;
    h.rowptr = {0, 0, 1, 2, 3};
    h.colidx = {0, 0, 0};
    h.wself = {1.0 - 3 * 0x1p-11, 0.0, 0.0, 0.0};
    h.wedge = {0x1p-11 + 0x1p-31 + 0.625 * u, 0x1p-11 + 0x1p-32 - 0.3125 * u, 0x1p-11 + 0x1p-32 - 0.3125 * u};
    expect_ok("column sum of exactly 1 + 2^-30 from four terms", run(config(4, ACS_RULE_PUSHSUM), h), 2, 3);
    snprintf(want, sizeof want,
             "sender 0: column sum %.17g > 1 + 2^-30 after rounding to binary32 (PUSHSUM must not create mass)",
             1.0 + 0x1p-30 + u);
    expect("column sum above the bound only after binary32 rounding", run(config(4, ACS_RULE_PUSHSUM, 0, ACS_F32), h),
           ACS_EINVAL, want);
}

// one row of `deg` senders (all node 0), the other rows empty with w_self > 0
static Graph one_big_row(uint64_t n, uint64_t deg) {
    Graph g;
    g.rowptr.assign(n + 1, deg);
    g.rowptr[0] = 0;
    g.colidx.assign(deg, 0u);
    g.wself.assign(n, 0.5);
    g.wedge.assign(deg, 0.0);
    return g;
}

static void row_limits_and_accepted() {
    char want[256];
    // kGenericMaxM entries = kGenericMaxM - 1 senders and the receiver itself
    Graph g = one_big_row(4, kGenericMaxM - 1);
    expect_ok("a row of exactly kGenericMaxM entries", run(config(4, ACS_RULE_WEIGHTED), g), kGenericMaxM, kGenericMaxM - 1);
    g = one_big_row(4, kGenericMaxM);
    snprintf(want, sizeof want, "rule WEIGHTED serves rows of at most %u entries (largest row: %u)", kGenericMaxM,
             kGenericMaxM + 1);
    expect("a row above kGenericMaxM entries, WEIGHTED", run(config(4, ACS_RULE_WEIGHTED), g), ACS_EUNSUPPORTED, want);
    snprintf(want, sizeof want, "rule PUSHSUM serves rows of at most %u entries (largest row: %u)", kGenericMaxM,
             kGenericMaxM + 1);
    expect("a row above kGenericMaxM entries, PUSHSUM", run(config(4, ACS_RULE_PUSHSUM), g), ACS_EUNSUPPORTED, want);
    expect_ok("the same graph under AVERAGE (the big-m path serves it)", run(config(4, ACS_RULE_AVERAGE), g),
              kGenericMaxM + 1, kGenericMaxM);
    // an empty row with w_self > 0, and a graph with no edge at all
    g = small();
    g.rowptr = {0, 2, 2, 4};
    g.colidx = {1, 2, 0, 1};
    g.wedge = {0.25, 0.25, 0.25, 0.25};
    expect_ok("an empty row with w_self > 0", run(config(3, ACS_RULE_WEIGHTED), g), 3, 4);
    g.wself[1] = 0.0;
    expect("an empty row with w_self = 0", run(config(3, ACS_RULE_WEIGHTED), g), ACS_EINVAL,
           "receiver 1: the row's weights sum to 0");
    Graph e;
    e.rowptr = {0, 0, 0, 0};
    e.colidx = {};
    e.wself = {1.0, 0.5, 0x1p-1074};
    e.wedge = {};
    expect_ok("nnz = 0, WEIGHTED", run(config(3, ACS_RULE_WEIGHTED), e), 1, 0);
    expect_ok("nnz = 0, PUSHSUM", run(config(3, ACS_RULE_PUSHSUM), e), 1, 0);
    expect_ok("nnz = 0, TRIMMED t = 0", run(config(3, ACS_RULE_TRIMMED_MEAN, 0), e), 1, 0);
    // the held weights: rounded to the dtype, -0.0 stored as +0.0
    g = small();
    g.wself[0] = -0.0;
    g.wedge[0] = 0.1;
    CsrCheck r = run(config(3, ACS_RULE_WEIGHTED, 0, ACS_F32), g);
    ++g_checks;
    if (r.code != ACS_OK || std::signbit(r.wsv[0]) || r.wev[0] != (double)0.1f || r.wsv.size() != 3 || r.wev.size() != 5) {
        ++g_failed;
        fprintf(stderr, "held weights: code %d, wsv[0] %g, wev[0] %.17g\n", r.code, r.wsv[0], r.wev[0]);
    }
}

int main() {
    rejected_arrays();
    rejected_weights();
    pushsum_columns();
    row_limits_and_accepted();
    fprintf(stderr, "csr_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
