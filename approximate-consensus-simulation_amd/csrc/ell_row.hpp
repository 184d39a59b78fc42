// ell_row.hpp — the SELL-64 row layout of the register / binned paths (engine.hpp, "ell"), in one place.
//
// A padded row array of width dp (a multiple of 4) is stored as 64-row slices of 4-wide column
// groups, [ceil(N/64)][dp/4][64][4]: lane l of a wave reads the 4 elements of group q of its row
// with one 16-byte (ids, masks, fp32 weights) or 32-byte (fp64 weights) load, and the wave's 64
// loads are contiguous.  The ids (ell), the edge weights (well) and a link schedule's masks (avell)
// all use it.
// The index functions compile without HIP (tests/host/ell_row.cpp checks them on the CPU); the
// vector types below them need the HIP headers.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define ACS_ELL_HD __host__ __device__ __forceinline__
#else
#define ACS_ELL_HD inline
#endif

namespace acs {

// Element index of column t of row i in an array of row width dp.  Row = the caller's row type
// (uint32_t or uint64_t): a 32-bit row is split in 32 bits, as the kernels always did; the index
// itself is 64-bit either way.
template <typename Row>
ACS_ELL_HD constexpr uint64_t ell_slot(Row i, uint32_t dp, uint32_t t) {
    return (((uint64_t)(i >> 6) * (dp >> 2) + (t >> 2)) * 64 + (i & 63)) * 4 + (t & 3);
}

// Index of row i's group 0 in units of one 4-element group (uint4 / float4 / double4), nq = dp / 4
// groups per row; group q of the row is q * 64 further on: ell_slot(i, 4 * nq, 4 * q) / 4.
ACS_ELL_HD constexpr uint64_t ell_group0(uint32_t i, int nq) { return (uint64_t)(i >> 6) * (nq * 64) + (i & 63); }

#if defined(__HIPCC__)
// the vector types of a value type VT: w4 = one weight group, pair = a push-sum (s, z) or link (h, k) pair
template <typename VT>
struct EllVec;
template <>
struct EllVec<float> {
    using w4 = float4;
    using pair = float2;
};
template <>
struct EllVec<double> {
    using w4 = double4;
    using pair = double2;
};
#endif

}  // namespace acs
