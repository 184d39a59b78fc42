// round_pushsum_split.hip — rule PUSHSUM with per-round splitting ("Push-sum with
// per-round splitting"): push-sum on a periodic link schedule where, in every round, a sender divides
// its pair over itself and the links that are up in that round.
//
// Every node j holds, beside its pair (s_j, z_j), one offer o_j = (share_p(j) * s_j + 0.0,
// share_p(j) * z_j + 0.0) for the round's phase p = r mod P (two roundings each, no FMA:
// -ffp-contract=off): what it sends on every up link and keeps for itself.  The offers live in two
// buffers indexed by round parity, like the pairs: receivers gather from the one being read while
// the other is written.
// One lane = one receiver i over the SELL-64 ELL padded to a compile-time width D, in
// k_round_pushsum's order.  Per lane and round:
//   - D/4 coalesced 16-byte loads of sender ids;
//   - one gather of the offer of every present column (16 B in fp64, 8 B in fp32), all issued before
//     any arithmetic; absent columns load nothing;
//   - the mask groups (a.avell: one uint4 at the address a weight group would have), loaded after
//     the gathers; a slot that is down in this round adds +0.0 to both sums;
//   - one DROP draw per present slot when loss_p > 0 (a dropped message's mass is lost);
//   - the two §A.7 tree sums over the m = D + 1 entries in entry order, entry 0 = o_i;
//   - x_i' = s_i' / z_i' where z_i' > 0, else x_i is kept; one pair store, one x store;
//   - node i's offer of the next round, share_{(r+1) mod P}(i) * (s_i', z_i') + 0.0: one store, so no
//     separate pass over the nodes runs in the round loop;
//   - (min, max) of x^{r+1} reduced per block -> one partial (§A.8 epilogue).
// No weights and no links are streamed.  Hub rows (deg[i] = kDegHub) are left to k_round_generic's
// split sub-branch of rule 6.
#include "csr_lane.hpp"
#include "resolve.hpp"
#include "rules.hpp"

namespace acs {

template <int D, typename VT>
__global__ __launch_bounds__(kRegularBlock) void k_round_pushsum_split(const RoundArgs a) {
    static_assert(D % 4 == 0, "compiled widths are multiples of 4");
    constexpr int M = D + 1;
    constexpr int NQ = D / 4;
    using V2 = typename EllVec<VT>::pair;
    const uint32_t lb = blockIdx.y;
    InstState* S = a.st + lb;
    if (S->done) return;  // device-side early exit (uniform per block)

    const uint64_t N = a.N;
    const VT* __restrict__ x = reinterpret_cast<const VT*>(a.xin) + lb * N;
    VT* __restrict__ xo = reinterpret_cast<VT*>(a.xout) + lb * N;
    const V2* __restrict__ oin = reinterpret_cast<const V2*>(a.oin) + lb * N;
    V2* __restrict__ oo = reinterpret_cast<V2*>(a.oout) + lb * N;
    V2* __restrict__ po = reinterpret_cast<V2*>(a.pout) + lb * N;
    const uint32_t i = blockIdx.x * kRegularBlock + threadIdx.x;   // receiver = ELL row

    double mn = kInf, mx = -kInf;   // exact for binary32 values too
    if (i < N && a.deg[i] != kDegHub) {
        const uint64_t g0 = ell_group0(i, NQ);
        const uint4* cp = reinterpret_cast<const uint4*>(a.ell) + g0;
        const uint4* ap = reinterpret_cast<const uint4*>(a.avell) + g0;
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
            const V2 own = oin[i];
            ps[0] = own.x;
            pz[0] = own.y;
#pragma unroll
            for (int t = 0; t < D; ++t) {
                V2 v;
                v.x = v.y = VT(0);
                if ((uint32_t)t < dg) v = oin[col[t]];
                ps[1 + t] = v.x;
                pz[1 + t] = v.y;
            }
        }
        const VT xi = x[i];
        const VT shn = reinterpret_cast<const VT*>(a.share_next)[i];
        const MsgParams& mp = a.mp;
        const uint32_t b = (uint32_t)(mp.inst_offset + lb);
        const uint32_t bG = b - b % mp.mask_group;
        const uint32_t r = a.r;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            uint32_t down = 0;   // bit k set = column 4q + k's slot is down in round r
            if ((uint32_t)q < nqs) down = down_bits(ap[q * 64], a.phase);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = 4 * q + k;
                bool gone = (uint32_t)t >= dg;   // absent column: +0.0 in both sums
                if (!gone && mp.thr) gone = draw(mp.key, kStreamDrop, bG, r, rp + t) < mp.thr;
                gone = gone || ((down >> k) & 1u);
                ps[1 + t] = gone ? VT(0) : ps[1 + t];
                pz[1 + t] = gone ? VT(0) : pz[1 + t];
            }
        }
        V2 o;
        o.x = tree_sum_const<M>(ps);
        o.y = tree_sum_const<M>(pz);
        // z' = 0 (all mass lost on the way here): keep x_i
        const VT res = o.y > VT(0) ? o.x / o.y : xi;
        V2 nx;   // what node i offers in round r + 1
        nx.x = shn * o.x + VT(0);
        nx.y = shn * o.y + VT(0);
        po[i] = o;
        oo[i] = nx;
        xo[i] = res;
        mn = res;
        mx = res;
    }
    block_minmax_store<kRegularBlock>(mn, mx, a.partial + (uint64_t)lb * a.nblk + blockIdx.x);
}

// offers[b][i] = (share[i] * s + 0.0, share[i] * z + 0.0) of pairs[b][i]
template <typename VT>
__global__ __launch_bounds__(256) void k_pushsum_offer(const typename EllVec<VT>::pair* __restrict__ pairs,
                                                       const VT* __restrict__ share,
                                                       typename EllVec<VT>::pair* __restrict__ offers, uint64_t n,
                                                       uint64_t N) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const typename EllVec<VT>::pair v = pairs[k];
    const VT sh = share[k % N];
    typename EllVec<VT>::pair o;
    o.x = sh * v.x + VT(0);
    o.y = sh * v.y + VT(0);
    offers[k] = o;
}

hipError_t launch_pushsum_offer(const void* pairs, const void* share, void* offers, uint64_t B, uint64_t N, bool f32,
                                hipStream_t s) {
    const uint64_t n = B * N;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (f32)
        hipLaunchKernelGGL(k_pushsum_offer<float>, grid, dim3(256), 0, s, static_cast<const float2*>(pairs),
                           static_cast<const float*>(share), static_cast<float2*>(offers), n, N);
    else
        hipLaunchKernelGGL(k_pushsum_offer<double>, grid, dim3(256), 0, s, static_cast<const double2*>(pairs),
                           static_cast<const double*>(share), static_cast<double2*>(offers), n, N);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------- dispatch
hipError_t launch_round_pushsum_split(const RoundArgs& a, uint64_t B, uint32_t nblk_fast, hipStream_t s) {
    if (!a.deg || !a.sw || !a.ell || !a.avell || !a.rowptr || !a.oin || !a.oout || !a.share_next || !a.pout)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblk_fast, (unsigned)B);
    const dim3 block(kRegularBlock);
    const bool hit = csr_lane_width(a.d, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        if (a.f32)
            hipLaunchKernelGGL((k_round_pushsum_split<DD, float>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((k_round_pushsum_split<DD, double>), grid, block, 0, s, a);
    });
    return hit ? hipGetLastError() : hipErrorNotSupported;
}

}  // namespace acs
