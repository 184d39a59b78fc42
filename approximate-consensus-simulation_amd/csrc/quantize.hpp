// quantize.hpp — the quantizer of handles with quantized messages ("Quantized
// messages"; acs_create_csr_quantized).  The step is 2^-k, so every operation below is exact in the
// value type: scaling by a power of two, floor, rint, the fractional part and the scaling back.
#pragma once

#include "engine.hpp"

namespace acs {

constexpr uint32_t kStreamQuant = 8;   // ACS_STREAM_QUANT: the dither draw, one per node and round
constexpr uint32_t kQuantPartial = 0, kQuantTotal = 1, kQuantCompensated = 2;   // ACS_QUANT_*
constexpr uint32_t kQuantMaxLog2F64 = 52, kQuantMaxLog2F32 = 23;

__device__ __forceinline__ double scale2(double v, int e) { return __builtin_ldexp(v, e); }
__device__ __forceinline__ float scale2(float v, int e) { return __builtin_ldexpf(v, e); }
__device__ __forceinline__ double floor_t(double v) { return __builtin_floor(v); }
__device__ __forceinline__ float floor_t(float v) { return __builtin_floorf(v); }
__device__ __forceinline__ double rint_t(double v) { return __builtin_rint(v); }
__device__ __forceinline__ float rint_t(float v) { return __builtin_rintf(v); }

// Q(x; b, r, i): what node i of global instance b transmits in round r.
//   u = x * 2^k
//   deterministic: n = rint(u), half to even
//   dithered:      f = floor(u), g = u - f in [0, 1), thr = (uint32)(g * 2^32) by truncation,
//                  n = f + (draw(QUANT, b, r, i) < thr ? 1 : 0)      (E[n] = u up to 2^-32)
//   q = n * 2^-k + 0.0 (never -0.0)
// |u| >= 2^52 (2^23) is an integer already: g = 0 and no draw can raise it, so f + 1 is never inexact.
template <typename VT>
__device__ __forceinline__ VT quantize(VT x, uint32_t k, uint32_t dither, Key key, uint32_t b, uint32_t r,
                                       uint32_t i) {
    const VT u = scale2(x, (int)k);
    VT n;
    if (dither) {
        const VT f = floor_t(u);
        const uint32_t thr = (uint32_t)scale2(u - f, 32);
        n = f + (draw(key, kStreamQuant, b, r, i) < thr ? VT(1) : VT(0));
    } else {
        n = rint_t(u);
    }
    return scale2(n, -(int)k) + VT(0);
}

}  // namespace acs
