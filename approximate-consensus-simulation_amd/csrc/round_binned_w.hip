// round_binned_w.hip — phase B of the binned exchange for rule WEIGHTED on a CSR plan (DESIGN.md §9;
// opt-in, ACSIM_BIN_WEIGHTED=1).  Phases A and M are round_binned.hip's, unchanged: the stage holds
// the senders' plain x.  Here one workgroup is one receiver block of kBinSB receivers, one lane each,
// exactly as in the VAR one-pass k_bin_gather (block order, done exit, qhi cut, neutral partials, hub
// rows, timestamps); instead of a sort the lane multiplies its D values by its D weights.
//
// The weights need no stream of their own.  invpos is indexed by ELL slot, so the lane sees its
// values in slot order, and acs_sim::well already holds the edge weights in SELL-64 order (slice of
// 64 rows, group of 4 columns, lane): with 256 receivers per block and lane = receiver, a wave's
// load of group q is the contiguous 2 KiB the per-lane kernel k_round_weighted<D> reads.  A lane
// loads group q only when 4q < deg(i): each lane's 32-byte group is a memory sector of its own, so a
// skipped group is 32 bytes not moved (the per-lane kernel cuts at the slice's widest row instead).
//
// Arithmetic is k_round_weighted's to the bit: p_e = (w_e * v_e) + 0.0 in two roundings, absent
// columns and (OMIT) dropped entries +0.0 in both sums, tree sums over the D + 1 entries in entry
// order, one IEEE divide, x_i kept when the weight sum is 0.  Loss: the lane draws its own §A.5 drop
// mask (one Philox call per 4 consecutive slots rowptr[i] + t) before the values arrive; under SELF
// a dropped entry takes x_i and keeps its weight.  No fault schedule reaches this kernel: no status
// array, no tags, no sender resolution.
#include "binned_dev.hpp"

namespace acs {

template <int D, bool LOSS>
__global__ __launch_bounds__(kBinSB, D == 32 ? 2 : 1) void k_bin_gather_w(const RoundArgs a,
                                                                           const double* __restrict__ stage,
                                                                           const uint16_t* __restrict__ invpos,
                                                                           const uint2* __restrict__ tiles, uint32_t nrun,
                                                                           uint32_t Q, uint32_t Qc, uint32_t pol) {
    static_assert(D % 8 == 0 && D <= 32, "invpos is read 8 slots at a time; one drop bit per slot");
    constexpr int SB = (int)kBinSB;
    constexpr int M = D + 1;
    constexpr int NQ = D / 4;
    // runs are padded to 16-byte multiples; nrun <= D*SB/16 (checked when the plan is built)
    __shared__ __attribute__((aligned(16))) double raw[D * SB + D * SB / 16];
    InstState* S = a.st;
    if (S->done) return;
    const uint64_t t0 = a.ts ? __builtin_amdgcn_s_memrealtime() : 0;
    uint64_t t1 = 0;
    // XCD-aware order, as in k_bin_gather
    const uint32_t b = a.qlo + (blockIdx.x & 7u) * Qc + (blockIdx.x >> 3);
    if (b >= a.qhi) return;   // past this launch's block range (hub rows' partial slots)
    if (b >= Q) {             // partial slots past the plan's blocks: neutral
        if (b < a.nblk && threadIdx.x == 0) a.partial[b] = make_double2(kInf, -kInf);
        return;
    }
    constexpr uint32_t NW = SB / 64;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t li = (uint64_t)b * SB + threadIdx.x;   // local row
    const uint64_t i = a.row0 + li;                        // global receiver
    bool live = li < a.nrows;
    uint32_t dg = 0;
    if (live) {
        dg = a.deg[i];
        if (dg == kDegHub) {   // a hub row: the generic kernel serves it
            live = false;
            dg = 0;
        }
    }
    const uint2* tb = tiles + (uint64_t)b * (nrun + 1);
    double v[M], wt[M];
    v[0] = live ? a.xin[i] : 0.0;
    wt[0] = live ? reinterpret_cast<const double*>(a.wself)[i] : 0.0;
    uint64_t rp = 0;
    if constexpr (LOSS) {
        if (live) rp = a.rowptr[i];
    }
    uint4 ip[D / 8];
    auto pos_of = [&](int t) -> uint32_t {   // position of slot t (compile-time t)
        const uint4& u = ip[t / 8];
        const uint32_t wd = (t & 6) == 0 ? u.x : (t & 6) == 2 ? u.y : (t & 6) == 4 ? u.z : u.w;
        return (t & 1) ? wd >> 16 : wd & 0xFFFFu;
    };
    {   // once-read stream: nontemporal 16-byte loads (padding lanes of a ragged last block read zeros)
        using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
        const u32x4* ipn = reinterpret_cast<const u32x4*>(invpos) + (uint64_t)b * (D / 8) * SB + threadIdx.x;
#pragma unroll
        for (int q = 0; q < D / 8; ++q) {
            const u32x4 t4 = __builtin_nontemporal_load(ipn + q * SB);
            ip[q] = make_uint4(t4.x, t4.y, t4.z, t4.w);
        }
    }
    // the block's runs -> LDS
    if (pol & kPolAsmDmaT)
        bin_dma_runs_asm_tb(tb, w * nrun / NW, (w + 1) * nrun / NW, stage, raw);
    else
        bin_dma_runs(tb, w * nrun / NW, (w + 1) * nrun / NW, stage, raw);
    // the weights, in flight beside the run copies: group q of the lane's row, only below deg(i)
    {
        // (+ ell_group0(i, NQ), ell_row.hpp, as two offsets: added as one the kernel compiles to other code)
        const double4* wp = reinterpret_cast<const double4*>(a.well) + (uint64_t)(i >> 6) * (NQ * 64) + (i & 63);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            double4 ww = make_double4(0.0, 0.0, 0.0, 0.0);
            if ((uint32_t)(4 * q) < dg) ww = wp[q * 64];
            wt[1 + 4 * q + 0] = ww.x;
            wt[1 + 4 * q + 1] = ww.y;
            wt[1 + 4 * q + 2] = ww.z;
            wt[1 + 4 * q + 3] = ww.w;
        }
    }
    // §A.5 drop decisions of the lane's slots as a bit mask, drawn while the copies are in flight (the
    // Philox state is dead before the D values are live): bit t = draw(key, DROP, bG, r, rp + t) < thr
    uint32_t dmask = 0;
    if constexpr (LOSS) {
        const MsgParams& mp = a.mp;
        if (dg) {
            const uint32_t bI = (uint32_t)mp.inst_offset, bG = bI - bI % mp.mask_group;
            const uint64_t c1 = (rp + dg + 3) >> 2;
            for (uint64_t c = rp >> 2; c < c1; ++c) {
                const U4 u = philox10((uint32_t)c, a.r, bG, kStreamDrop, mp.key);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint64_t t = 4 * c + e - rp;   // wraps past 2^64 below rp: out of range
                    if (t < dg) dmask |= (uint32_t)(u.v[e] < mp.thr) << t;
                }
            }
        }
    }
    if (pol & kPolAsmDmaT) bin_dma_wait();
    __syncthreads();
    if (a.ts) t1 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
    for (int t = 0; t < D; ++t) v[1 + t] = raw[pos_of(t)];

    double mn = kInf, mx = -kInf;
    if (live) {
        const double xi = v[0];
        const bool omit = LOSS && a.mp.omit;
        // products in place: v becomes p (values, weights and products are never all live)
        v[0] = wt[0] * xi + 0.0;
#pragma unroll
        for (int t = 0; t < D; ++t) {
            const bool dropped = LOSS && ((dmask >> t) & 1u);
            // absent column (its weight is +0.0 already) or an OMIT drop: +0.0 in both sums
            const bool gone = (uint32_t)t >= dg || (omit && dropped);
            const double u = dropped ? xi : v[1 + t];   // SELF: the entry takes x_i and keeps its weight
            const double we = gone ? 0.0 : wt[1 + t];
            wt[1 + t] = we;
            v[1 + t] = gone ? 0.0 : we * u + 0.0;
        }
        const double num = tree_sum_const<M>(v), den = tree_sum_const<M>(wt);
        const double res = den > 0.0 ? num / den : xi;   // den = 0: every present weight is 0 (OMIT)
        bin_store_x<SB>(a, i, res, pol);
        mn = res;
        mx = res;
    }
    block_minmax_store<SB>(mn, mx, a.partial + b, a.eacc);
    if (a.ts) bin_ts(a.ts, t0, t1);
}

// ---------------------------------------------------------------------------- dispatch
#define ACS_BINNED_W_WIDTHS(X) X(8) X(16) X(32)

bool binned_weighted_supported(uint32_t d) {
#define X(DD) if (d == DD) return true;
    ACS_BINNED_W_WIDTHS(X)
#undef X
    return false;
}

hipError_t launch_bin_gather_w(const BinnedPlan& p, const RoundArgs& a, const double* stage, uint32_t Qc,
                               hipStream_t s) {
    const dim3 grid(8 * Qc), block(kBinSB);
#define X(DD)                                                                                                        \
    if (p.D == DD) {                                                                                                 \
        if (a.mp.thr)                                                                                                \
            hipLaunchKernelGGL((k_bin_gather_w<DD, true>), grid, block, 0, s, a, stage, p.invpos, p.tiles, p.nrun,  \
                               p.Q, Qc, p.pol);                                                                      \
        else                                                                                                         \
            hipLaunchKernelGGL((k_bin_gather_w<DD, false>), grid, block, 0, s, a, stage, p.invpos, p.tiles, p.nrun, \
                               p.Q, Qc, p.pol);                                                                      \
        return hipGetLastError();                                                                                    \
    }
    ACS_BINNED_W_WIDTHS(X)
#undef X
    return hipErrorNotSupported;
}

}  // namespace acs
