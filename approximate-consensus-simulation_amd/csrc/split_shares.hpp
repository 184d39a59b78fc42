// split_shares.hpp — the share table of acs_create_csr_split ("Push-sum with
// per-round splitting"), computed once on the host before any device memory exists.
// Host-only, no HIP header, in the manner of sched_check.hpp.
#pragma once

#include <math.h>

#include "sched_check.hpp"

namespace acs {

// 1 / c rounded to the config dtype, stepped down while c * w exceeds 1 in exact arithmetic: the
// sign of fma(c, w, -1) in binary64 is that of the exact c * w - 1 (one rounding, and c < 2^34 is a
// binary64 value), for a binary32 w too.  The rule of acsim.graphs.pushsum_weights.
inline double split_share_of(uint64_t c, bool f32) {
    const double cd = (double)c;
    if (f32) {
        float w = 1.0f / (float)c;
        while (fma(cd, (double)w, -1.0) > 0.0) w = nextafterf(w, 0.0f);
        return (double)w;
    }
    double w = 1.0 / cd;
    while (fma(cd, w, -1.0) > 0.0) w = nextafter(w, 0.0);
    return w;
}

// out[p * N + j] = share_p(j) with c_p(j) = 1 + #{slots e : colidx[e] == j and bit p of avail[e] set},
// phase-major, as binary64 values that are exact in the config dtype.  The arrays have passed
// csr_check_arrays and sched_check.
inline void split_shares(std::vector<double>& out, bool f32, uint64_t N, uint64_t nnz, const uint32_t* colidx,
                         uint32_t period, const uint32_t* avail) {
    std::vector<uint64_t> cnt((size_t)period * N, 1);
    for (uint64_t e = 0; e < nnz; ++e)
        for (uint32_t m = avail[e], p = 0; m; m >>= 1, ++p)
            if (m & 1u) ++cnt[(size_t)p * N + colidx[e]];
    out.resize(cnt.size());
    double memo[64];   // small counts are nearly all of them
    for (uint64_t c = 1; c < 64; ++c) memo[c] = split_share_of(c, f32);
    for (size_t k = 0; k < cnt.size(); ++k) out[k] = cnt[k] < 64 ? memo[cnt[k]] : split_share_of(cnt[k], f32);
}

}  // namespace acs
