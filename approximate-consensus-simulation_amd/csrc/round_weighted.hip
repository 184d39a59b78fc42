// round_weighted.hip — rule WEIGHTED: edge-weighted averaging x' = W x on a CSR graph.
//
// One lane = one receiver i of a CSR graph padded to a compile-time width D (the SELL-64 ELL of the
// CSR register path: column groups past the slice's widest row are not loaded, columns past deg(i)
// are absent entries).  Per lane and round:
//   - D/4 coalesced 16-byte loads of sender ids and, beside them, the same groups of the weight
//     array (same slice / group / lane order: 16 B per lane in fp32, 32 B in fp64, contiguous over
//     the wave);
//   - the x gathers (and status gathers) of every present column, issued together before any resolve;
//   - §A.6 resolution, one DROP draw per slot (CSR slots rowptr[i] + t are not 4-aligned);
//   - p_e = (w_e * v_e) + 0.0 (two roundings, no FMA: -ffp-contract=off) and the two §A.7 tree sums
//     over the m = D + 1 entries in entry order, in registers; absent columns and (OMIT) missing
//     entries add +0.0 to both;
//   - one IEEE divide (x_i is kept when the weight sum is 0, which only OMIT can produce), one store;
//   - honest (min, max) of x^{r+1} reduced per block -> one partial (§A.8 epilogue).
// Hub rows (deg[i] = kDegHub) are left to k_round_generic's rule-5 branch.
#include "csr_lane.hpp"
#include "quantize.hpp"
#include "resolve.hpp"
#include "rules.hpp"

namespace acs {

// SCHED ("Link schedules"): beside each weight group the lane loads the group's four
// availability masks (a.avell, the weights' order), 16 B per lane, predicated like the weight load.
// Once all groups are issued the masks are reduced to one bit per column, set when the slot is down
// in this round (so they are dead before the gathers); a down slot's message is missing exactly as
// a dropped one.
//
// QUANT ("Quantized messages"; no faults, no delays): the gathers read what the senders
// transmit (a.qin) and never x; entry 0, which a missing entry also takes under SELF, is x_i in mode
// PARTIAL and q_i = qin[i] otherwise; COMPENSATED adds the node's own quantization error x_i - q_i
// to the quotient.  The lane then stores what node i transmits in the next round beside
// x_i' (a.qout): one more load and store per lane, and one Philox call under dither.
template <int D, typename VT, bool SCHED, bool QUANT>
__global__ __launch_bounds__(kRegularBlock) void k_round_weighted(const RoundArgs a) {
    static_assert(D % 4 == 0, "compiled widths are multiples of 4");
    constexpr int M = D + 1;
    constexpr int NQ = D / 4;
    using W4 = typename EllVec<VT>::w4;
    const uint32_t lb = blockIdx.y;
    InstState* S = a.st + lb;
    if (S->done) return;  // device-side early exit (uniform per block)

    const uint64_t N = a.N;
    const VT* __restrict__ x = reinterpret_cast<const VT*>(a.xin) + lb * N;
    VT* __restrict__ xo = reinterpret_cast<VT*>(a.xout) + lb * N;
    const uint32_t i = blockIdx.x * kRegularBlock + threadIdx.x;   // receiver = ELL row

    double mn = kInf, mx = -kInf;   // exact for binary32 values too
    if (i < N && a.deg[i] != kDegHub) {
        const VT xi = x[i];
        VT res = xi;
        const VT* __restrict__ qin = nullptr;
        VT qi = xi, e0 = xi;   // e0: entry 0
        if constexpr (QUANT) {
            qin = reinterpret_cast<const VT*>(a.qin) + lb * N;
            qi = qin[i];
            e0 = a.qmode == kQuantPartial ? xi : qi;
        }
        bool honest = true, active = true;
        const uint32_t* stv = nullptr;   // null: no fault schedule
        if (a.status) {
            stv = a.status + lb * N;
            const uint32_t si = stv[i];
            honest = si == kHonest;
            active = is_active(si, a.r);
        }
        if (active) {
            const uint64_t g0 = ell_group0(i, NQ);
            const uint4* cp = reinterpret_cast<const uint4*>(a.ell) + g0;
            const W4* wp = reinterpret_cast<const W4*>(a.well) + g0;
            const uint32_t nqs = a.sw[i >> 6];   // uniform over the wave (one 64-row slice)
            const uint32_t dg = a.deg[i];
            const uint64_t rp = a.rowptr[i];
            uint32_t col[D];
            VT w[M], p[M];
            w[0] = reinterpret_cast<const VT*>(a.wself)[i];
            uint4 mk[SCHED ? NQ : 1];   // SCHED: the groups' masks, reduced to one bit per column below
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                uint4 c = make_uint4(kEllNone, kEllNone, kEllNone, kEllNone);
                W4 ww;
                ww.x = ww.y = ww.z = ww.w = VT(0);
                if constexpr (SCHED) mk[q] = make_uint4(0u, 0u, 0u, 0u);
                if ((uint32_t)q < nqs) {   // groups past the slice's width are not loaded
                    c = cp[q * 64];
                    ww = wp[q * 64];
                    if constexpr (SCHED) mk[q] = reinterpret_cast<const uint4*>(a.avell)[g0 + q * 64];
                }
                col[4 * q + 0] = c.x;
                col[4 * q + 1] = c.y;
                col[4 * q + 2] = c.z;
                col[4 * q + 3] = c.w;
                w[1 + 4 * q + 0] = ww.x;
                w[1 + 4 * q + 1] = ww.y;
                w[1 + 4 * q + 2] = ww.z;
                w[1 + 4 * q + 3] = ww.w;
            }
            // after the loads, not inside their loop: a reduction there would make every group's loads
            // wait for the group before it (bit t set = column t's slot is down in round r)
            uint32_t down = 0;
            if constexpr (SCHED) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) down |= down_bits(mk[q], a.phase) << (4 * q);
            }
            const MsgParams& mp = a.mp;
            const uint32_t b = (uint32_t)(mp.inst_offset + lb);
            const uint32_t bG = b - b % mp.mask_group;
            const VT lo = (VT)S->lo, hi = (VT)S->hi;
            const uint32_t r = a.r;
            VT xj[D];
            uint32_t sj[D];
            // all gathers first; absent columns load nothing
#pragma unroll
            for (int t = 0; t < D; ++t) {
                const bool ok = (uint32_t)t < dg;
                const uint32_t j = ok ? col[t] : i;
                if constexpr (QUANT) {
                    xj[t] = ok ? qin[j] : e0;
                    sj[t] = kHonest;
                    continue;
                }
                if (a.delay)
                    xj[t] = ok ? delayed_x<VT>(a, lb, r, draw(mp.key, kStreamDelay, b, r, rp + t), j) : xi;
                else
                    xj[t] = ok ? x[j] : xi;
                sj[t] = (ok && stv) ? stv[j] : kHonest;
            }
            p[0] = w[0] * e0 + VT(0);
#pragma unroll
            for (int t = 0; t < D; ++t) {
                bool gone = (uint32_t)t >= dg;   // absent column: +0.0 in both sums (w is +0.0 already)
                VT u = e0;
                if (!gone) {
                    const uint64_t s = rp + t;
                    bool dropped = mp.thr && draw(mp.key, kStreamDrop, bG, r, s) < mp.thr;
                    if (SCHED) dropped = dropped || ((down >> t) & 1u);
                    bool miss;
                    u = resolve_entry_m(mp, sj[t], xj[t], e0, dropped, b, r, i, s, lo, hi, miss);
                    gone = mp.omit && miss;   // SELF: the entry takes x_i and keeps its weight
                }
                const VT wt = gone ? VT(0) : w[1 + t];
                w[1 + t] = wt;
                p[1 + t] = gone ? VT(0) : wt * u + VT(0);
            }
            const VT num = tree_sum_const<M>(p), den = tree_sum_const<M>(w);
            if (den > VT(0)) res = num / den;   // den = 0: every present weight is 0 (OMIT) -> keep x_i
            if constexpr (QUANT) {
                if (den > VT(0) && a.qmode == kQuantCompensated) res = res + (xi - qi);
            }
        }
        xo[i] = res;
        if constexpr (QUANT)
            (reinterpret_cast<VT*>(a.qout) + lb * N)[i] =
                quantize<VT>(res, a.qk, a.qdither, a.mp.key, (uint32_t)(a.mp.inst_offset + lb), a.r + 1, i);
        if (honest) {
            mn = res;
            mx = res;
        }
    }
    block_minmax_store<kRegularBlock>(mn, mx, a.partial + (uint64_t)lb * a.nblk + blockIdx.x);
}

// ---------------------------------------------------------------------------- dispatch
hipError_t launch_round_weighted(const RoundArgs& a, uint64_t B, uint32_t nblk_fast, hipStream_t s) {
    if (!a.deg || !a.sw || !a.ell || !a.well || !a.wself || !a.rowptr) return hipErrorInvalidValue;
    if ((a.qin != nullptr) != (a.qout != nullptr) || (a.qin && (a.status || a.delay))) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblk_fast, (unsigned)B);
    const dim3 block(kRegularBlock);
    const bool hit = csr_lane_select(a, [&](auto d, auto vt, auto sched) {
        constexpr int DD = decltype(d)::value;
        constexpr bool SC = decltype(sched)::value;
        if (a.qin)
            hipLaunchKernelGGL((k_round_weighted<DD, decltype(vt), SC, true>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((k_round_weighted<DD, decltype(vt), SC, false>), grid, block, 0, s, a);
    });
    return hit ? hipGetLastError() : hipErrorNotSupported;
}

// q[b][i] = Q(x[b][i]; inst_offset + b, r, i)
template <typename VT>
__global__ __launch_bounds__(256) void k_quantize(const VT* __restrict__ x, VT* __restrict__ q, uint64_t N, uint32_t r,
                                                  Key key, uint64_t inst_offset, uint32_t k, uint32_t dither) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint64_t at = (uint64_t)blockIdx.y * N + i;
    q[at] = quantize<VT>(x[at], k, dither, key, (uint32_t)(inst_offset + blockIdx.y), r, (uint32_t)i);
}

hipError_t launch_quantize(const void* x, void* q, uint64_t B, uint64_t N, uint32_t r, const MsgParams& mp, uint32_t k,
                           uint32_t dither, bool f32, hipStream_t s) {
    const dim3 grid((unsigned)((N + 255) / 256), (unsigned)B);
    if (f32)
        hipLaunchKernelGGL(k_quantize<float>, grid, dim3(256), 0, s, static_cast<const float*>(x), static_cast<float*>(q), N,
                           r, mp.key, mp.inst_offset, k, dither);
    else
        hipLaunchKernelGGL(k_quantize<double>, grid, dim3(256), 0, s, static_cast<const double*>(x), static_cast<double*>(q),
                           N, r, mp.key, mp.inst_offset, k, dither);
    return hipGetLastError();
}

}  // namespace acs
