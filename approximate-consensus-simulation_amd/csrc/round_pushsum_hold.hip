// round_pushsum_hold.hip — rule PUSHSUM under missing_policy = HOLD: robust ratio
// consensus by running sums.  Mass that fails to cross a link is not lost: it waits on the link and
// arrives with the next message that gets through.
//
// Besides the (s, z) pair of every node, every CSR slot e = rowptr[i] + t of every instance holds a
// pair (h_e, k_e) of the config dtype, [B][nnz] in slot order, +0.0 at round 0.  One lane = one
// receiver i over the same padded SELL-64 ELL and weight array as k_round_pushsum, in that
// kernel's order: ids, all pair gathers, then the weight groups.  With each weight group come the
// up to four link pairs of its columns (loads predicated on t < deg(i): an absent column touches
// no link).  Per sender entry:
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
// The rest is k_round_pushsum's: two §A.7 tree sums over the D + 1 entries, x_i' = s_i' / z_i' where
// z_i' > 0 and else x_i, one pair store, one x store, one (min, max) partial per block.
// Hub rows (deg[i] = kDegHub) are left to k_round_generic's rule-6 branch, which takes the same
// steps when RoundArgs carries links.
#include <type_traits>

#include "resolve.hpp"
#include "rules.hpp"

namespace acs {

__device__ __forceinline__ bool same_bits(double u, double v) { return __double_as_longlong(u) == __double_as_longlong(v); }
__device__ __forceinline__ bool same_bits(float u, float v) { return __float_as_uint(u) == __float_as_uint(v); }

// SCHED ("Link schedules"): with each weight group come the group's four
// availability masks (a.avell, the weights' order); a slot that is down in this round takes the
// dropped branch, so its mass waits on the link until the slot is up again.
template <int D, typename VT, bool SCHED>
__global__ __launch_bounds__(kRegularBlock) void k_round_pushsum_hold(const RoundArgs a) {
    static_assert(D % 4 == 0, "compiled widths are multiples of 4");
    constexpr int M = D + 1;
    constexpr int NQ = D / 4;
    using W4 = typename std::conditional<sizeof(VT) == 4, float4, double4>::type;
    using V2 = typename std::conditional<sizeof(VT) == 4, float2, double2>::type;
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
        const uint64_t g0 = (uint64_t)(i >> 6) * (NQ * 64) + (i & 63);
        const uint4* cp = reinterpret_cast<const uint4*>(a.ell) + g0;
        const W4* wp = reinterpret_cast<const W4*>(a.well) + g0;
        const uint32_t nqs = a.sw[i >> 6];   // uniform over the wave (one 64-row slice)
        const uint32_t dg = a.deg[i];
        const uint64_t rp = a.rowptr[i];
        // this row's links: slots rp .. rp + dg - 1 of instance lb (rp + dg <= nnz = a.lnk_stride)
        V2* lk = reinterpret_cast<V2*>(a.lnk) + (uint64_t)lb * a.lnk_stride + rp;
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
        }
        V2 o;
        o.x = tree_sum_const<M>(ps);
        o.y = tree_sum_const<M>(pz);
        const VT res = o.y > VT(0) ? o.x / o.y : xi;   // z' = 0 (all mass still on the links): keep x_i
        po[i] = o;
        xo[i] = res;
        mn = res;
        mx = res;
    }
    block_minmax_store<kRegularBlock>(mn, mx, a.partial + (uint64_t)lb * a.nblk + blockIdx.x);
}

// ---------------------------------------------------------------------------- dispatch
// (the widths of k_round_pushsum: pushsum_fast_supported decides for both)
#define ACS_PUSHSUM_HOLD_WIDTHS(X) X(4) X(8) X(16) X(32)

hipError_t launch_round_pushsum_hold(const RoundArgs& a, uint64_t B, uint32_t nblk_fast, hipStream_t s) {
    if (!a.deg || !a.sw || !a.ell || !a.well || !a.wself || !a.rowptr || !a.pin || !a.pout || !a.lnk)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblk_fast, (unsigned)B);
    const dim3 block(kRegularBlock);
#define X(DD)                                                                                   \
    if (a.d == DD) {                                                                            \
        if (a.avell && a.f32)                                                                   \
            hipLaunchKernelGGL((k_round_pushsum_hold<DD, float, true>), grid, block, 0, s, a);   \
        else if (a.avell)                                                                       \
            hipLaunchKernelGGL((k_round_pushsum_hold<DD, double, true>), grid, block, 0, s, a);  \
        else if (a.f32)                                                                         \
            hipLaunchKernelGGL((k_round_pushsum_hold<DD, float, false>), grid, block, 0, s, a);  \
        else                                                                                    \
            hipLaunchKernelGGL((k_round_pushsum_hold<DD, double, false>), grid, block, 0, s, a); \
        return hipGetLastError();                                                               \
    }
    ACS_PUSHSUM_HOLD_WIDTHS(X)
#undef X
    return hipErrorNotSupported;
}

}  // namespace acs
