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
//
// LINK = kLinkHold is the rule under missing_policy = HOLD: robust ratio consensus by
// running sums.  Mass that fails to cross a link is not lost: it waits on the link and arrives with
// the next message that gets through.
// Besides the (s, z) pair of every node, every CSR slot e = rowptr[i] + t of every instance holds a
// pair (h_e, k_e) of the config dtype, [B][nnz] in slot order, +0.0 at round 0.  The lane's order
// stays: ids, all pair gathers, then the weight groups.  With each weight group come the up to four
// link pairs of its columns (loads predicated on t < deg(i): an absent column touches no link).
// Per sender entry:
//   a = (w_e * s_j) + 0.0, c = (w_e * z_j) + 0.0     as the plain rule: two roundings each, no FMA
//   hn = h_e + a, kn = k_e + c                        one rounding each
//   dropped = loss_p > 0 && draw(key, DROP, bG, r, e) < thr     the plain rule's draw
//   delivered: the entry contributes (hn, kn), the link stores (+0.0, +0.0)
//   dropped:   the entry contributes (+0.0, +0.0), the link stores (hn, kn)
// The link is consumed as it arrives (ps[1 + t] takes hn or +0.0 in place), so nothing D-wide is
// live beside ps and pz.  The update is in place: slot e is read and written by its receiver's lane
// alone, in this launch alone, and a finished instance's blocks return before touching it.  A store
// whose value equals, bit for bit, what was loaded is skipped (a delivered message on an empty
// link: every link of a lossless run).
// Hub rows take the same steps in k_round_generic's rule-6 branch when RoundArgs carries links.
//
// LINK = kLinkTransit is the rule with messages in transit ("Push-sum with messages in
// transit"; handles of acs_create_csr_transit): a message sent in round r on slot e arrives in round
// r + delta, delta = draw(DELAY, b, r, e) mod (transit_max + 1), and until then its mass waits in
// the ring a.trn: trn_np = transit_max + 1 planes [nnz] of (h, k) pairs per instance, the cell of
// arrival round q in plane q mod trn_np.  With each weight group come the group's cells of the
// plane this round delivers (a.trn_cur), as HOLD's links do.  Per sender entry that is not gone
// (dropped, or down under a schedule: a gone message never enters transit, its mass is lost):
//   a = (w_e * s_j) + 0.0, c = (w_e * z_j) + 0.0     the plain rule's products
//   delta = 0: the loaded cell takes (a, c) in registers     one rounding each
//   delta > 0: the cell of plane (r + delta) mod trn_np takes (a, c) in place (a load, a store)
// The entry contributes its cell of the current plane, which then stores (+0.0, +0.0); a store whose
// bits equal what was loaded is skipped.  A cell therefore folds its arrivals in ascending sending
// round, from +0.0 (or from what acs_set_pushsum_transit put there).  The delta > 0 cell is never
// the one being delivered (1 <= delta <= transit_max < trn_np), and every cell of slot e is touched
// by e's receiver lane alone.
#include "csr_lane.hpp"
#include "resolve.hpp"
#include "rules.hpp"

namespace acs {

__device__ __forceinline__ bool same_bits(double u, double v) { return __double_as_longlong(u) == __double_as_longlong(v); }
__device__ __forceinline__ bool same_bits(float u, float v) { return __float_as_uint(u) == __float_as_uint(v); }

// SCHED ("Link schedules"): with each weight group come the group's four
// availability masks (a.avell, the weights' order); a slot that is down in this round is gone like
// a dropped one (HOLD: it takes the dropped branch, so its mass waits on the link until the slot is
// up again).
enum : int { kLinkPlain = 0, kLinkHold = 1, kLinkTransit = 2 };   // what a message does on its link

template <int D, typename VT, bool SCHED, int LINK>
__global__ __launch_bounds__(kRegularBlock) void k_round_pushsum(const RoundArgs a) {
    static_assert(D % 4 == 0, "compiled widths are multiples of 4");
    constexpr bool HOLD = LINK == kLinkHold, TRANSIT = LINK == kLinkTransit;
    constexpr int M = D + 1;
    constexpr int NQ = D / 4;
    using W4 = typename EllVec<VT>::w4;
    using V2 = typename EllVec<VT>::pair;
    const uint32_t lb = blockIdx.y;
    InstState* S = a.st + lb;
    if (S->done) return;  // device-side early exit (uniform per block): a finished instance's links stay

    const uint64_t N = a.N;
    const VT* __restrict__ x = reinterpret_cast<const VT*>(a.xin) + lb * N;
    VT* __restrict__ xo = reinterpret_cast<VT*>(a.xout) + lb * N;
    const V2* __restrict__ pin = reinterpret_cast<const V2*>(a.pin) + lb * N;
    V2* __restrict__ po = reinterpret_cast<V2*>(a.pout) + lb * N;
    const uint32_t i = blockIdx.x * kRegularBlock + threadIdx.x;   // receiver = ELL row

    double mn = kInf, mx = -kInf;   // exact for binary32 values too
    if (i < N && a.deg[i] != kDegHub) {
        const uint64_t g0 = ell_group0(i, NQ);
        const uint4* cp = reinterpret_cast<const uint4*>(a.ell) + g0;
        const W4* wp = reinterpret_cast<const W4*>(a.well) + g0;
        const uint32_t nqs = a.sw[i >> 6];   // uniform over the wave (one 64-row slice)
        const uint32_t dg = a.deg[i];
        const uint64_t rp = a.rowptr[i];
        // HOLD: this row's links, slots rp .. rp + dg - 1 of instance lb (rp + dg <= nnz = a.lnk_stride).
        // Formed here, before the id loads: inside the group loop it compiles to other code.
        [[maybe_unused]] V2* lk = HOLD ? reinterpret_cast<V2*>(a.lnk) + (uint64_t)lb * a.lnk_stride + rp : nullptr;
        // TRANSIT: this row's cells of plane 0 of instance lb's ring; plane p is a.lnk_stride pairs on
        [[maybe_unused]] V2* tr =
            TRANSIT ? reinterpret_cast<V2*>(a.trn) + (uint64_t)lb * a.trn_np * a.lnk_stride + rp : nullptr;
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
        ps[0] = w0 * ps[0] + VT(0);   // entry 0 has no link
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
            if constexpr (HOLD) {
                V2 l[4];   // the group's links, taken with its weights
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    l[k].x = l[k].y = VT(0);
                    if ((uint32_t)(4 * q + k) < dg) l[k] = lk[4 * q + k];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int t = 4 * q + k;
                    const bool here = (uint32_t)t < dg;   // absent column: +0.0 in both sums, no link
                    const VT hn = l[k].x + (wq[k] * ps[1 + t] + VT(0));
                    const VT kn = l[k].y + (wq[k] * pz[1 + t] + VT(0));
                    bool dropped = false;
                    if (here && mp.thr) dropped = draw(mp.key, kStreamDrop, bG, r, rp + t) < mp.thr;
                    if (SCHED) dropped = dropped || (here && ((down >> k) & 1u));
                    ps[1 + t] = here && !dropped ? hn : VT(0);
                    pz[1 + t] = here && !dropped ? kn : VT(0);
                    V2 keep;
                    keep.x = dropped ? hn : VT(0);
                    keep.y = dropped ? kn : VT(0);
                    if (here && !(same_bits(keep.x, l[k].x) && same_bits(keep.y, l[k].y))) lk[t] = keep;
                }
            } else if constexpr (TRANSIT) {
                V2* tc = tr + (uint64_t)a.trn_cur * a.lnk_stride;   // the plane round r delivers
                V2 l[4], g[4];    // the group's cells of that plane, and of the planes its messages go to
                uint32_t dst[4];  // the plane a message goes to (a.trn_cur: delivered now), kEllNone: gone
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    l[k].x = l[k].y = VT(0);
                    if ((uint32_t)(4 * q + k) < dg) l[k] = tc[4 * q + k];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int t = 4 * q + k;
                    bool gone = (uint32_t)t >= dg;   // absent column: +0.0 in both sums, no cell
                    if (!gone && mp.thr) gone = draw(mp.key, kStreamDrop, bG, r, rp + t) < mp.thr;
                    if (SCHED) gone = gone || ((down >> k) & 1u);
                    uint32_t p = gone ? kEllNone : a.trn_cur;
                    if (!gone && a.trn_np > 1) {
                        p += draw(mp.key, kStreamDelay, b, r, rp + t) % a.trn_np;
                        if (p >= a.trn_np) p -= a.trn_np;
                    }
                    dst[k] = p;
                    g[k].x = g[k].y = VT(0);
                    if (p != kEllNone && p != a.trn_cur) g[k] = tr[(uint64_t)p * a.lnk_stride + t];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int t = 4 * q + k;
                    VT sv = ps[1 + t], zv = pz[1 + t];
                    // (binary32, D = 32: the SLP vectoriser pairs neighbouring elements of ps for packed
                    // multiplies and then leaves the whole array in scratch; the empty asm keeps them scalar)
                    if constexpr (sizeof(VT) == 4) asm("" : "+v"(sv), "+v"(zv));
                    const VT pa = wq[k] * sv + VT(0);
                    const VT pc = wq[k] * zv + VT(0);
                    const bool now = dst[k] == a.trn_cur;
                    ps[1 + t] = now ? l[k].x + pa : l[k].x;   // (absent column: the cell read as +0.0)
                    pz[1 + t] = now ? l[k].y + pc : l[k].y;
                    if (dst[k] != kEllNone && !now) {
                        V2 n;
                        n.x = g[k].x + pa;
                        n.y = g[k].y + pc;
                        if (!(same_bits(n.x, g[k].x) && same_bits(n.y, g[k].y))) tr[(uint64_t)dst[k] * a.lnk_stride + t] = n;
                    }
                    V2 zero;
                    zero.x = zero.y = VT(0);
                    // (an absent column's l is +0.0: no store)
                    if (!(same_bits(l[k].x, VT(0)) && same_bits(l[k].y, VT(0)))) tc[t] = zero;
                }
            } else {
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
        }
        V2 o;
        o.x = tree_sum_const<M>(ps);
        o.y = tree_sum_const<M>(pz);
        // z' = 0 (all mass lost on the way here, or under HOLD still on the links): keep x_i
        const VT res = o.y > VT(0) ? o.x / o.y : xi;
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
                                                      typename EllVec<VT>::pair* __restrict__ pairs, uint64_t n) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    typename EllVec<VT>::pair v;
    v.x = x[k];
    v.y = VT(1);
    pairs[k] = v;
}

// x[k] = s / z where z > 0, else s (acs_set_pushsum_state: the round's keep rule with nothing to keep)
template <typename VT>
__global__ __launch_bounds__(256) void k_pushsum_estimate(const typename EllVec<VT>::pair* __restrict__ pairs,
                                                          VT* __restrict__ x, uint64_t n) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const typename EllVec<VT>::pair v = pairs[k];
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
hipError_t launch_round_pushsum(const RoundArgs& a, bool hold, uint64_t B, uint32_t nblk_fast, hipStream_t s) {
    if (!a.deg || !a.sw || !a.ell || !a.well || !a.wself || !a.rowptr || !a.pin || !a.pout || hold != (a.lnk != nullptr))
        return hipErrorInvalidValue;
    if (a.trn && (hold || a.trn_np < 1 || a.trn_cur >= a.trn_np)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblk_fast, (unsigned)B);
    const dim3 block(kRegularBlock);
    const bool hit = csr_lane_select(a, [&](auto d, auto vt, auto sched) {
        constexpr int DD = decltype(d)::value;
        constexpr bool SCHED = decltype(sched)::value;
        using VT = decltype(vt);
        if (a.trn)
            hipLaunchKernelGGL((k_round_pushsum<DD, VT, SCHED, kLinkTransit>), grid, block, 0, s, a);
        else if (hold)
            hipLaunchKernelGGL((k_round_pushsum<DD, VT, SCHED, kLinkHold>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((k_round_pushsum<DD, VT, SCHED, kLinkPlain>), grid, block, 0, s, a);
    });
    return hit ? hipGetLastError() : hipErrorNotSupported;
}

}  // namespace acs
