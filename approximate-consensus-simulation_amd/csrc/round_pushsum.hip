// round_pushsum.hip — rule PUSHSUM: push-sum / ratio consensus on a directed CSR graph.
//
// Node i holds a pair (s_i, z_i); x_i = s_i / z_i is the estimate the rest of the engine sees.
// One lane = one receiver i over the SELL-64 ELL of the CSR register path padded to a compile-time
// width D, with the edge weights in a second array in the same order (k_round_weighted's layout).
// Per lane and round:
//   - D/4 coalesced 16-byte loads of sender ids;
//   - one gather of the (s, z) pair of every present column (16 B in fp64, 8 B in fp32: one memory
//     sector, like a plain x gather), all issued before any arithmetic; absent columns load nothing;
//   - the weight groups are loaded after the gathers and multiplied in as they arrive, in place:
//     ps_e = (w_e * s_e) + 0.0 and pz_e = (w_e * z_e) + 0.0 (two roundings each, no FMA:
//     -ffp-contract=off), so ids, weights and pairs are never all live together;
//   - one DROP draw per present slot when loss_p > 0 (a dropped message adds +0.0 to both sums: its
//     mass is lost); no status array, no §A.6 resolve: the rule is not defined under faults;
//   - the two §A.7 tree sums over the m = D + 1 entries in entry order, in registers, no
//     normalisation; absent columns add +0.0;
//   - x_i' = s_i' / z_i' (IEEE divide) where z_i' > 0, else x_i is kept; one pair store, one x store;
//   - (min, max) of x^{r+1} reduced per block -> one partial (§A.8 epilogue).
// Hub rows (deg[i] = kDegHub) are left to k_round_generic's rule-6 branch.
#include "resolve.hpp"
#include "rules.hpp"

namespace acs {

template <typename VT>
struct PsVec;
template <>
struct PsVec<float> {
    using w4 = float4;
    using pair = float2;
};
template <>
struct PsVec<double> {
    using w4 = double4;
    using pair = double2;
};

// SCHED ("Link schedules"): with each weight group come the group's four
// availability masks (a.avell, the weights' order); a slot that is down in this round is gone like
// a dropped one.
template <int D, typename VT, bool SCHED>
__global__ __launch_bounds__(kRegularBlock) void k_round_pushsum(const RoundArgs a) {
    static_assert(D % 4 == 0, "compiled widths are multiples of 4");
    constexpr int M = D + 1;
    constexpr int NQ = D / 4;
    using W4 = typename PsVec<VT>::w4;
    using V2 = typename PsVec<VT>::pair;
    const uint32_t lb = blockIdx.y;
    InstState* S = a.st + lb;
    if (S->done) return;  // device-side early exit (uniform per block)

    const uint64_t N = a.N;
    const VT* __restrict__ x = reinterpret_cast<const VT*>(a.xin) + lb * N;
    VT* __restrict__ xo = reinterpret_cast<VT*>(a.xout) + lb * N;
    const V2* __restrict__ pin = reinterpret_cast<const V2*>(a.pin) + lb * N;
    V2* __restrict__ po = reinterpret_cast<V2*>(a.pout) + lb * N;
    const uint32_t i = blockIdx.x * kRegularBlock + threadIdx.x;   // receiver = ELL row

    double mn = kInf, mx = -kInf;   // exact for binary32 values too
    if (i < N && a.deg[i] != kDegHub) {
        const uint64_t g0 = (uint64_t)(i >> 6) * (NQ * 64) + (i & 63);
        const uint4* cp = reinterpret_cast<const uint4*>(a.ell) + g0;
        const W4* wp = reinterpret_cast<const W4*>(a.well) + g0;
        const uint32_t nqs = a.sw[i >> 6];   // uniform over the wave (one 64-row slice)
        const uint32_t dg = a.deg[i];
        const uint64_t rp = a.rowptr[i];
        VT ps[M], pz[M];
        {
            uint32_t col[D];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                uint4 c = make_uint4(kEllNone, kEllNone, kEllNone, kEllNone);
                if ((uint32_t)q < nqs) c = cp[q * 64];   // groups past the slice's width are not loaded
                col[4 * q + 0] = c.x;
                col[4 * q + 1] = c.y;
                col[4 * q + 2] = c.z;
                col[4 * q + 3] = c.w;
            }
            // all gathers first; absent columns load nothing
            const V2 own = pin[i];
            ps[0] = own.x;
            pz[0] = own.y;
#pragma unroll
            for (int t = 0; t < D; ++t) {
                V2 v;
                v.x = v.y = VT(0);
                if ((uint32_t)t < dg) v = pin[col[t]];
                ps[1 + t] = v.x;
                pz[1 + t] = v.y;
            }
        }
        const VT xi = x[i];
        const VT w0 = reinterpret_cast<const VT*>(a.wself)[i];
        ps[0] = w0 * ps[0] + VT(0);
        pz[0] = w0 * pz[0] + VT(0);
        const MsgParams& mp = a.mp;
        const uint32_t b = (uint32_t)(mp.inst_offset + lb);
        const uint32_t bG = b - b % mp.mask_group;
        const uint32_t r = a.r;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            W4 ww;
            ww.x = ww.y = ww.z = ww.w = VT(0);
            uint32_t down = 0;   // SCHED: bit k set = column 4q + k's slot is down in round r
            if ((uint32_t)q < nqs) {
                ww = wp[q * 64];
                if (SCHED) down = down_bits(reinterpret_cast<const uint4*>(a.avell)[g0 + q * 64], a.phase);
            }
            const VT wq[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = 4 * q + k;
                bool gone = (uint32_t)t >= dg;   // absent column: +0.0 in both sums
                if (!gone && mp.thr) gone = draw(mp.key, kStreamDrop, bG, r, rp + t) < mp.thr;
                if (SCHED) gone = gone || ((down >> k) & 1u);
                ps[1 + t] = gone ? VT(0) : wq[k] * ps[1 + t] + VT(0);
                pz[1 + t] = gone ? VT(0) : wq[k] * pz[1 + t] + VT(0);
            }
        }
        V2 o;
        o.x = tree_sum_const<M>(ps);
        o.y = tree_sum_const<M>(pz);
        const VT res = o.y > VT(0) ? o.x / o.y : xi;   // z' = 0 (all mass lost on the way here): keep x_i
        po[i] = o;
        xo[i] = res;
        mn = res;
        mx = res;
    }
    block_minmax_store<kRegularBlock>(mn, mx, a.partial + (uint64_t)lb * a.nblk + blockIdx.x);
}

// pairs[k] = (x[k], 1): round 0 of the rule, and acs_set_state
template <typename VT>
__global__ __launch_bounds__(256) void k_pushsum_fill(const VT* __restrict__ x,
                                                      typename PsVec<VT>::pair* __restrict__ pairs, uint64_t n) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    typename PsVec<VT>::pair v;
    v.x = x[k];
    v.y = VT(1);
    pairs[k] = v;
}

// x[k] = s / z where z > 0, else s (acs_set_pushsum_state: the round's keep rule with nothing to keep)
template <typename VT>
__global__ __launch_bounds__(256) void k_pushsum_estimate(const typename PsVec<VT>::pair* __restrict__ pairs,
                                                          VT* __restrict__ x, uint64_t n) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const typename PsVec<VT>::pair v = pairs[k];
    x[k] = v.y > VT(0) ? v.x / v.y : v.x;
}

hipError_t launch_pushsum_fill(const void* x, void* pairs, uint64_t n, bool f32, hipStream_t s) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (f32)
        hipLaunchKernelGGL(k_pushsum_fill<float>, grid, dim3(256), 0, s, static_cast<const float*>(x),
                           static_cast<float2*>(pairs), n);
    else
        hipLaunchKernelGGL(k_pushsum_fill<double>, grid, dim3(256), 0, s, static_cast<const double*>(x),
                           static_cast<double2*>(pairs), n);
    return hipGetLastError();
}

hipError_t launch_pushsum_estimate(const void* pairs, void* x, uint64_t n, bool f32, hipStream_t s) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (f32)
        hipLaunchKernelGGL(k_pushsum_estimate<float>, grid, dim3(256), 0, s, static_cast<const float2*>(pairs),
                           static_cast<float*>(x), n);
    else
        hipLaunchKernelGGL(k_pushsum_estimate<double>, grid, dim3(256), 0, s, static_cast<const double2*>(pairs),
                           static_cast<double*>(x), n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------- dispatch
#define ACS_PUSHSUM_WIDTHS(X) X(4) X(8) X(16) X(32)

bool pushsum_fast_supported(uint32_t d) {
#define X(DD) if (d == DD) return true;
    ACS_PUSHSUM_WIDTHS(X)
#undef X
    return false;
}

hipError_t launch_round_pushsum(const RoundArgs& a, uint64_t B, uint32_t nblk_fast, hipStream_t s) {
    if (!a.deg || !a.sw || !a.ell || !a.well || !a.wself || !a.rowptr || !a.pin || !a.pout)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblk_fast, (unsigned)B);
    const dim3 block(kRegularBlock);
#define X(DD)                                                                              \
    if (a.d == DD) {                                                                       \
        if (a.avell && a.f32)                                                              \
            hipLaunchKernelGGL((k_round_pushsum<DD, float, true>), grid, block, 0, s, a);   \
        else if (a.avell)                                                                  \
            hipLaunchKernelGGL((k_round_pushsum<DD, double, true>), grid, block, 0, s, a);  \
        else if (a.f32)                                                                    \
            hipLaunchKernelGGL((k_round_pushsum<DD, float, false>), grid, block, 0, s, a);  \
        else                                                                               \
            hipLaunchKernelGGL((k_round_pushsum<DD, double, false>), grid, block, 0, s, a); \
        return hipGetLastError();                                                          \
    }
    ACS_PUSHSUM_WIDTHS(X)
#undef X
    return hipErrorNotSupported;
}

}  // namespace acs
