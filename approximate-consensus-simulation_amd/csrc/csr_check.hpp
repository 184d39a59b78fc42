// csr_check.hpp — host checks of a CSR handle's arrays, before any handle or device memory exists
// (create.hip, create_impl): the graph (§8(f) row 1) and, for rules WEIGHTED and PUSHSUM, the
// weights as the device will hold them.  Host-only, no HIP header, in the manner of
// binned_select.hpp: tests/host/csr_check.cpp feeds it every rejected input on the CPU.
#pragma once

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/acsim.h"

namespace acs {

// Generic kernel (round_generic.hip): one workgroup per receiver, LDS bitonic sort; receivers with
// more entries take the big-m path, which rules WEIGHTED and PUSHSUM do not have.
constexpr uint32_t kGenericMaxM = 8192;

// Rule PUSHSUM ("mass bound"): column sums at most 1 + 2^-30, chosen together with the
// admitted |s| and the fp32 round limit (handle.hpp) so that no sum of a run can overflow.
constexpr double kPushsumColMax = 1.0 + 0x1p-30;

struct CsrCheck {
    int code = ACS_OK;
    std::string message;         // acs_last_error's text when code != ACS_OK
    uint64_t mmax = 0, nnz = 0;  // largest m_i = deg(i) + 1 (at least 1), rowptr[N]
    std::vector<double> wsv, wev;   // the weights as held: rounded to the config dtype, -0.0 -> +0.0

    int fail(int c, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        message = buf;
        return code = c;
    }
};

// §8(f) row 1: rowptr starts at 0 and does not decrease, every receiver has m > 2t (but for
// AVERAGE), the slot count fits the counters, every sender id is a node.
inline int csr_check_arrays(CsrCheck& r, const acs_config& c, const uint64_t* rowptr, const uint32_t* colidx) {
    const uint64_t N = c.n_nodes;
    if (rowptr[0] != 0) return r.fail(ACS_EINVAL, "rowptr[0] must be 0");
    r.mmax = 1;
    for (uint64_t i = 0; i < N; ++i) {
        if (rowptr[i + 1] < rowptr[i]) return r.fail(ACS_EINVAL, "rowptr must be non-decreasing");
        const uint64_t m = rowptr[i + 1] - rowptr[i] + 1;
        if (c.rule != ACS_RULE_AVERAGE && m <= 2ull * c.trim)
            return r.fail(ACS_EINVAL, "receiver %llu has m = %llu <= 2t", (unsigned long long)i, (unsigned long long)m);
        if (m > r.mmax) r.mmax = m;
    }
    r.nnz = rowptr[N];
    if (r.nnz >= (1ull << 34)) return r.fail(ACS_EINVAL, "slot count must be < 2^34");
    if (c.fault_model == ACS_FAULT_BYZANTINE && c.byz_strategy == ACS_BYZ_RANDOM && r.nnz > (1ull << 33))
        return r.fail(ACS_EINVAL, "BYZ RANDOM needs slot count <= 2^33");
    for (uint64_t k = 0; k < r.nnz; ++k)
        if (colidx[k] >= N) return r.fail(ACS_EINVAL, "colidx[%llu] out of range", (unsigned long long)k);
    return ACS_OK;
}

// Rules WEIGHTED and PUSHSUM, after csr_check_arrays: the weights as the device will
// hold them (rounded to binary32 once in fp32 mode, -0.0 canonicalised), checked after rounding:
// finite, 0 <= w <= 1, and a positive weight sum in every row (all summands are >= 0, so the
// entry-order tree sum is positive exactly when some weight of the row is).
inline int csr_check_weights(CsrCheck& r, const acs_config& c, const uint64_t* rowptr, const uint32_t* colidx,
                             const double* wself, const double* wedge) {
    const uint64_t N = c.n_nodes;
    const bool f32 = c.dtype == ACS_F32, pushsum = c.rule == ACS_RULE_PUSHSUM;
    auto held = [f32](double w) { return (f32 ? (double)(float)w : w) + 0.0; };
    auto bad = [](double w) { return !(w >= 0.0 && w <= 1.0); };   // (NaN fails both comparisons)
    r.wsv.resize(N);
    r.wev.resize(r.nnz);
    for (uint64_t i = 0; i < N; ++i) {
        r.wsv[i] = held(wself[i]);
        if (bad(r.wsv[i])) return r.fail(ACS_EINVAL, "w_self[%llu] must be finite, in [0, 1]", (unsigned long long)i);
        bool pos = r.wsv[i] > 0.0;
        for (uint64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            r.wev[k] = held(wedge[k]);
            if (bad(r.wev[k])) return r.fail(ACS_EINVAL, "w_edge[%llu] must be finite, in [0, 1]", (unsigned long long)k);
            pos = pos || r.wev[k] > 0.0;
        }
        if (!pos)
            return r.fail(ACS_EINVAL, "receiver %llu: the row's weights sum to 0%s", (unsigned long long)i,
                          f32 ? " after rounding to binary32" : "");
    }
    if (pushsum) {
        // every column sum <= 1 + 2^-30 (the mass bound of DESIGN.md §9): w_self[j] plus every
        // w_edge[slot] with colidx[slot] == j, as a compensated (Kahan) double sum, whose error
        // (about 2 ulps) does not grow with the out-degree
        std::vector<double> cs(r.wsv), cc(N, 0.0);
        for (uint64_t k = 0; k < r.nnz; ++k) {
            const uint32_t j = colidx[k];
            const double y = r.wev[k] - cc[j];   // (no fast-math in this build: the compensation stays)
            const double tt = cs[j] + y;
            cc[j] = (tt - cs[j]) - y;
            cs[j] = tt;
        }
        for (uint64_t j = 0; j < N; ++j)
            if (!(cs[j] <= kPushsumColMax))
                return r.fail(ACS_EINVAL, "sender %llu: column sum %.17g > 1 + 2^-30%s (PUSHSUM must not create mass)",
                              (unsigned long long)j, cs[j], f32 ? " after rounding to binary32" : "");
    }
    if (r.mmax > kGenericMaxM)
        return r.fail(ACS_EUNSUPPORTED, "rule %s serves rows of at most %u entries (largest row: %llu)",
                      pushsum ? "PUSHSUM" : "WEIGHTED", kGenericMaxM, (unsigned long long)r.mmax);
    return ACS_OK;
}

}  // namespace acs
