// binned_plan.hip — construction of the binned exchange's plans (round_binned.hip runs them): the
// tile sort of the deliveries, the index streams of phases A / M / B and the fault fix-up list.  The
// knobs arrive as BinnedOptions (engine.hpp); nothing here reads the environment.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "binned_dev.hpp"

namespace acs {

// ------------------------------------------------------------------------------ plan build
// Geometry shared by the setup kernels.  Local receiver rows li in [0, NR) (a node partition's
// rows, or all N); global sender ids j in [0, N).
//   one level:  key1 = a*Q + b                         (phase B reads stage1)
//   two levels: key1 = a*R + r, key2 = (r*K + k)*QR + bl  with r = li / SR, k = a / PK,
//               bl = (li % SR) / SB                    (phase B reads stage2)
struct BinGeom {
    uint32_t D, dp, SA, P, Q, levels, SR, R, K, PK, QR;
    uint32_t SB;    // receivers per phase-B block (BinnedPlan::SB)
    uint32_t pad;   // tile lengths padded to 16 bytes: 2 (fp64) or 4 (fp32, narrow fp64) elements
    uint32_t npad_or;   // 1: tiles' starts carry the run's pad count in their low bits (not on narrow
                        // plans, whose 8-byte rounds address the starts in units of 2 entries)
    uint32_t none1, none2;   // tile count of level 1 / 2: the key of an absent CSR column (kEllNone),
                             // which sorts past every tile and is skipped by every fill kernel
};

__device__ __forceinline__ uint32_t ell_at(const uint32_t* ell, uint64_t i, uint32_t t, uint32_t dp) {
    return ell[ell_slot(i, dp, t)];
}

__global__ __launch_bounds__(256) void k_bin_keys(const uint32_t* __restrict__ ell, uint64_t E, BinGeom G, int level,
                                                  uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const uint64_t li = e / G.D;
    const uint32_t t = (uint32_t)(e % G.D);
    const uint32_t col = ell_at(ell, li, t, G.dp);
    const uint32_t a = col / G.SA;
    uint32_t key;
    if (col == kEllNone)
        key = level == 1 ? G.none1 : G.none2;
    else if (G.levels == 1)
        key = a * G.Q + (uint32_t)(li / G.SB);
    else if (level == 1)
        key = a * G.R + (uint32_t)(li / G.SR);
    else
        key = ((uint32_t)(li / G.SR) * G.K + a / G.PK) * G.QR + (uint32_t)((li % G.SR) / G.SB);
    keys[e] = key;
    vals[e] = (uint32_t)e;
}

// tile boundaries in the sorted keys: tl[key] = (first, last+1) unpadded sorted positions
__global__ __launch_bounds__(256) void k_bin_bounds(uint64_t E, const uint32_t* __restrict__ ks, uint2* __restrict__ tl,
                                                    uint64_t nt) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= E) return;
    const uint32_t key = ks[p];
    if (key >= nt) return;   // absent CSR columns
    if (p == 0 || ks[p - 1] != key) tl[key].x = (uint32_t)p;
    if (p == E - 1 || ks[p + 1] != key) tl[key].y = (uint32_t)(p + 1);
}

// padded tile lengths (even, so every run starts 16-byte aligned in the stage and in LDS)
__global__ __launch_bounds__(256) void k_bin_plen(const uint2* __restrict__ tl, uint64_t nt, uint32_t pad,
                                                  uint32_t* __restrict__ plen) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nt) return;
    const uint2 t = tl[k];
    plen[k] = t.y ? (t.y - t.x + pad - 1u) & ~(pad - 1u) : 0u;
}

// idxA[padded position] = sender index inside its source block (level-1 order)
__global__ __launch_bounds__(256) void k_bin_fill_a(const uint32_t* __restrict__ ell, uint64_t E, BinGeom G,
                                                    const uint32_t* __restrict__ ks, const uint32_t* __restrict__ vs,
                                                    const uint2* __restrict__ tl, const uint32_t* __restrict__ pstart,
                                                    uint16_t* __restrict__ idxA) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= E) return;
    const uint32_t e = vs[p], key = ks[p];
    if (key >= G.none1) return;
    idxA[pstart[key] + (p - tl[key].x)] = (uint16_t)(ell_at(ell, e / G.D, e % G.D, G.dp) % G.SA);
}

// idxA -> 14-bit packed blocks (binned_dev.hpp pk14): one thread per (512-position block m, lane l)
__global__ __launch_bounds__(256) void k_bin_pack14(const uint16_t* __restrict__ idx, uint64_t n, uint32_t* __restrict__ pk) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t m = t >> 6;
    const uint32_t l = (uint32_t)t & 63u;
    if (m * 512 >= n) return;
    uint64_t acc[2] = {0ull, 0ull};   // bits 0-63, 64-127
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint64_t pos = m * 512 + 2 * (64 * (uint64_t)(k >> 1) + l) + (k & 1);
        const uint64_t v = pos < n ? (uint64_t)(idx[pos] & 0x3FFFu) : 0ull;
        const int bit = 14 * k;
        if (bit < 64) {
            acc[0] |= v << bit;
            if (bit + 14 > 64) acc[1] |= v >> (64 - bit);
        } else {
            acc[1] |= v << (bit - 64);
        }
    }
    uint32_t* b = pk + m * kPk14Words + l;
    b[0] = (uint32_t)acc[0];
    b[64] = (uint32_t)(acc[0] >> 32);
    b[128] = (uint32_t)acc[1];
    reinterpret_cast<uint16_t*>(pk)[m * (2 * kPk14Words) + 384 + l] = (uint16_t)(acc[1] >> 32);
}


// phase-A ranges: aoff[a] = padded start of source block a's deliveries (aoff[P] = Ep)
__global__ __launch_bounds__(256) void k_bin_aoff(const uint32_t* __restrict__ pstart, uint32_t P, uint32_t G1,
                                                  uint64_t Ep, uint64_t* __restrict__ aoff) {
    const uint32_t a = blockIdx.x * 256 + threadIdx.x;
    if (a > P) return;
    aoff[a] = a < P ? pstart[(uint64_t)a * G1] : Ep;
}

// phase-M run tables: mt[g][j] for group g = r*K + k, run a = k*PK + j; total image size in cap[g]
__global__ __launch_bounds__(256) void k_bin_mtiles(const uint32_t* __restrict__ pstart1, const uint32_t* __restrict__ plen1,
                                                    BinGeom G, uint2* __restrict__ mt, uint32_t* __restrict__ cap) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G.R * G.K) return;
    const uint32_t r = g / G.K, k = g % G.K;
    uint32_t pre = 0;
    for (uint32_t j = 0; j < G.PK; ++j) {
        const uint32_t a = k * G.PK + j;
        if (a < G.P) {
            const uint64_t key = (uint64_t)a * G.R + r;
            mt[(uint64_t)g * (G.PK + 1) + j] = make_uint2(pstart1[key], pre);
            pre += plen1[key];
        } else {
            mt[(uint64_t)g * (G.PK + 1) + j] = make_uint2(0u, pre);
        }
    }
    mt[(uint64_t)g * (G.PK + 1) + G.PK] = make_uint2(0u, pre);
    cap[g] = pre;
}

// lpos[e] = position of delivery e inside its phase-M LDS image
__global__ __launch_bounds__(256) void k_bin_lpos(uint64_t E, BinGeom G, const uint32_t* __restrict__ ks1,
                                                  const uint32_t* __restrict__ vs1, const uint2* __restrict__ tl1,
                                                  const uint2* __restrict__ mt, uint16_t* __restrict__ lpos) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= E) return;
    const uint32_t key = ks1[p], a = key / G.R, r = key % G.R;
    if (key >= G.none1) return;
    const uint32_t g = r * G.K + a / G.PK;
    lpos[vs1[p]] = (uint16_t)(mt[(uint64_t)g * (G.PK + 1) + a % G.PK].y + (p - tl1[key].x));
}

// idxM[padded level-2 position] = lpos of that delivery
__global__ __launch_bounds__(256) void k_bin_fill_m(uint64_t E, const uint32_t* __restrict__ ks2,
                                                    const uint32_t* __restrict__ vs2, const uint2* __restrict__ tl2,
                                                    const uint32_t* __restrict__ pstart2, const uint16_t* __restrict__ lpos,
                                                    uint16_t* __restrict__ idxM, uint32_t none2) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= E) return;
    const uint32_t key = ks2[p];
    if (key >= none2) return;
    idxM[pstart2[key] + (p - tl2[key].x)] = lpos[vs2[p]];
}

// phase-M output ranges: moff[g] = padded level-2 start of group g (moff[R*K] = Ep2)
__global__ __launch_bounds__(256) void k_bin_moff(const uint32_t* __restrict__ pstart2, BinGeom G, uint64_t Ep2,
                                                  uint64_t* __restrict__ moff) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ng = G.R * G.K;
    if (g > ng) return;
    moff[g] = g < ng ? pstart2[(uint64_t)g * G.QR] : Ep2;
}

// Runs read by phase B for block b: one level: keys j*Q + b (j = source block, nrun = P); two
// levels: keys (r*K + j)*QR + bl (j = chunk, nrun = K).
__device__ __forceinline__ uint64_t bin_run_key(const BinGeom& G, uint32_t b, uint32_t j) {
    if (G.levels == 1) return (uint64_t)j * G.Q + b;
    return ((uint64_t)(b / G.QR) * G.K + j) * G.QR + b % G.QR;
}

// tiles[b][j] = (padded start | pad count, element offset inside block b's concatenated runs);
// tiles[b][nrun] = (0, total).  Starts are multiples of the pad unit, so the low bits carry the
// number of padding entries at the run's end.
__global__ __launch_bounds__(256) void k_bin_prefix(const uint32_t* __restrict__ pstart, const uint32_t* __restrict__ plen,
                                                    const uint2* __restrict__ tl, BinGeom G, uint32_t nrun,
                                                    uint2* __restrict__ tiles) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= G.Q) return;
    uint32_t pre = 0;
    for (uint32_t j = 0; j < nrun; ++j) {
        const uint64_t key = bin_run_key(G, b, j);
        const uint32_t npad = plen[key] - (tl[key].y - tl[key].x);
        tiles[(uint64_t)b * (nrun + 1) + j] = make_uint2(pstart[key] | (G.npad_or ? npad : 0u), pre);
        pre += plen[key];
    }
    tiles[(uint64_t)b * (nrun + 1) + nrun] = make_uint2(0u, pre);
}

// invpos[b][t/8][i_local][t%8] = element position of (receiver i_local, slot t) in block b's runs
__global__ __launch_bounds__(256) void k_bin_inv(uint64_t E, BinGeom G, uint32_t nrun, const uint32_t* __restrict__ ks,
                                                 const uint32_t* __restrict__ vs, const uint2* __restrict__ tl,
                                                 const uint2* __restrict__ tiles, uint16_t* __restrict__ invpos) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= E) return;
    const uint32_t e = vs[p], key = ks[p];
    if (key >= (G.levels == 1 ? G.none1 : G.none2)) return;
    const uint64_t li = e / G.D;
    const uint32_t t = e % G.D;
    const uint32_t b = (uint32_t)(li / G.SB);
    const uint32_t j = G.levels == 1 ? key / G.Q : (key / G.QR) % G.K;
    const uint32_t pos = tiles[(uint64_t)b * (nrun + 1) + j].y + (uint32_t)(p - tl[key].x);
    invpos[(((uint64_t)b * (G.D / 8) + t / 8) * G.SB + (li % G.SB)) * 8 + (t & 7)] = (uint16_t)pos;
}

// fix-up list: every sorted position p of the last level whose sender is not honest
__global__ __launch_bounds__(256) void k_bin_fixlist(const uint32_t* __restrict__ ell, uint64_t E, uint32_t D,
                                                     uint32_t dp, uint32_t none, const uint32_t* __restrict__ ks,
                                                     const uint32_t* __restrict__ vs, const uint2* __restrict__ tl,
                                                     const uint32_t* __restrict__ pstart,
                                                     const uint32_t* __restrict__ status,
                                                     uint4* __restrict__ fix, uint32_t cap, uint32_t* __restrict__ cnt) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= E) return;
    const uint32_t key = ks[p];
    if (key >= none) return;
    const uint32_t e = vs[p];
    const uint64_t li = e / D;
    const uint32_t t = e % D;
    const uint32_t j = ell_at(ell, li, t, dp);
    if (status[j] == kHonest) return;
    const uint32_t k = atomicAdd(cnt, 1u);
    if (k < cap) fix[k] = make_uint4(pstart[key] + (uint32_t)(p - tl[key].x), (uint32_t)li, t, j);
}

uint32_t binned_levels(uint64_t N, uint64_t NR, uint32_t d, uint32_t sa, uint32_t sb, uint32_t* sr_out) {
    if (d == 0 || sa == 0 || NR == 0 || sb == 0) return 0;
    const uint64_t P = (N + sa - 1) / sa;
    const uint64_t Q = (NR + sb - 1) / sb;
    // (the one- / two-level choice is the default block's, so a plan's level count and its
    // phase A / M do not change with the receiver block)
    const uint64_t Q0 = (NR + kBinSB - 1) / kBinSB;
    const double run1 = (double)NR * d / ((double)P * (double)Q0);
    if (run1 >= 64.0) {
        if (sr_out) *sr_out = sb;
        return (uint64_t)P <= (uint64_t)d * sb / 16 && Q >= 1 ? 1u : 0u;   // phase-B LDS bound
    }
    // level-1 runs (a, r) average NR*d / (P * R) with R = NR / SR: about 128 at SR = 128 * P / d
    // (SR a multiple of both the default block and sb: powers of two)
    const uint64_t unit = sb > kBinSB ? sb : kBinSB;
    uint64_t sr = (128ull * P / d + unit - 1) / unit * unit;
    if (sr < 4 * kBinSB) sr = 4 * kBinSB;
    if (sr % sb) return 0;
    if (sr > 65536) return 0;
    if (sr_out) *sr_out = (uint32_t)sr;
    return 2;
}

void binned_free(BinnedPlan& p) {
    if (p.ts) {   // diagnostic dump: phase,workgroup,t_entry,t_staged,t_end (100 MHz ticks)
        std::vector<uint64_t> h(3ull * (p.ts_a + p.ts_b + p.ts_m));
        if (hipMemcpy(h.data(), p.ts, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE* f = fopen(p.ts_file.c_str(), "w")) {
                for (uint64_t k = 0; k < p.ts_a + p.ts_b + p.ts_m; ++k)
                    fprintf(f, "%c,%llu,%llu,%llu,%llu\n", k < p.ts_a ? 'A' : k < p.ts_a + p.ts_b ? 'B' : 'M',
                            (unsigned long long)(k < p.ts_a ? k : k < p.ts_a + p.ts_b ? k - p.ts_a : k - p.ts_a - p.ts_b),
                            (unsigned long long)h[3 * k],
                            (unsigned long long)h[3 * k + 1], (unsigned long long)h[3 * k + 2]);
                fclose(f);
            }
        }
        (void)hipFree(p.ts);
    }
    (void)hipFree(p.idxA);
    (void)hipFree(p.pkA);
    (void)hipFree(p.idxM);
    (void)hipFree(p.invpos);
    (void)hipFree(p.tiles);
    (void)hipFree(p.mt);
    (void)hipFree(p.aoff);
    (void)hipFree(p.moff);
    (void)hipFree(p.stage1);
    (void)hipFree(p.stage2);
    (void)hipFree(p.xtag);
    (void)hipFree(p.fix);
    (void)hipFree(p.nhdr);
    p = BinnedPlan{};
}

namespace {

// Deliveries sorted by a tile key (stable LSD radix sort: ties stay in (row, slot) order) and the
// tiles padded to even lengths.  Owns its arrays.
struct TileSort {
    uint32_t *ks = nullptr, *vs = nullptr, *plen = nullptr, *pstart = nullptr;
    uint2* tl = nullptr;
    uint64_t nt = 0, Ep = 0;
    void release() {
        (void)hipFree(ks);
        (void)hipFree(vs);
        (void)hipFree(plen);
        (void)hipFree(pstart);
        (void)hipFree(tl);
        ks = vs = plen = pstart = nullptr;
        tl = nullptr;
    }
};

hipError_t tile_sort(const uint32_t* ell, uint64_t E, const BinGeom& G, int level, uint64_t nt, TileSort& T,
                     hipStream_t s) {
    hipError_t e;
    T.nt = nt;
    uint32_t *keys = nullptr, *vals = nullptr;
    void* temp = nullptr;
    size_t tb = 0, tb2 = 0;
    int bits = 1;
    while (bits < 32 && (1ull << bits) <= nt) ++bits;   // keys 0..nt (nt: absent CSR columns)
    const unsigned grid = (unsigned)((E + 255) / 256), gridt = (unsigned)((nt + 255) / 256);
    e = hipMalloc(&keys, E * 4);
    if (e == hipSuccess) e = hipMalloc(&vals, E * 4);
    if (e == hipSuccess) e = hipMalloc(&T.ks, E * 4);
    if (e == hipSuccess) e = hipMalloc(&T.vs, E * 4);
    if (e == hipSuccess) e = hipMalloc(&T.tl, nt * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc(&T.plen, nt * 4);
    if (e == hipSuccess) e = hipMalloc(&T.pstart, nt * 4);
    if (e == hipSuccess) e = hipMemsetAsync(T.tl, 0, nt * sizeof(uint2), s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bin_keys, dim3(grid), dim3(256), 0, s, ell, E, G, level, keys, vals);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys, T.ks, vals, T.vs, (int)E, 0, bits, s);
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, T.plen, T.pstart, (int)nt, s);
    if (tb2 > tb) tb = tb2;
    if (e == hipSuccess) e = hipMalloc(&temp, tb ? tb : 16);
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(temp, tb, keys, T.ks, vals, T.vs, (int)E, 0, bits, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bin_bounds, dim3(grid), dim3(256), 0, s, E, T.ks, T.tl, nt);
        hipLaunchKernelGGL(k_bin_plen, dim3(gridt), dim3(256), 0, s, T.tl, nt, G.pad, T.plen);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(temp, tb, T.plen, T.pstart, (int)nt, s);
    uint32_t last[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&last[0], T.pstart + nt - 1, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&last[1], T.plen + nt - 1, 4, hipMemcpyDeviceToHost, s);
    hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    T.Ep = (uint64_t)last[0] + last[1];
    (void)hipFree(temp);
    (void)hipFree(keys);
    (void)hipFree(vals);
    return e;
}

}  // namespace

hipError_t binned_build(BinnedPlan& p, const uint32_t* ell, const BinnedDesc& desc, const BinnedOptions& opt,
                        uint32_t sb, hipStream_t s) {
    const uint64_t N = desc.N, NR = desc.NR;
    const uint32_t d = desc.d, dp = desc.dp, sa = opt.sa;
    const bool tagged = desc.tagged, f32 = desc.f32, var = desc.var, clean = desc.clean;
    if (var && f32) return hipErrorNotSupported;   // CSR plans: fp64
    // receiver blocks other than kBinSB: clean plans of a compiled (d, sb) pair only
    if (sb != kBinSB && (var || tagged || !clean)) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    uint32_t sr = 0;
    const uint32_t levels = binned_levels(N, NR, d, sa, sb, &sr);
    if (!levels) return hipErrorNotSupported;
    const uint32_t pack = opt.pack;   // bit 0 (default 1; 0: u16 phase-A index stream), read below
    // narrow stage: clean one-level fp64 plans of d = 16 / 32 at the default
    // receiver block with the packed phase-A stream; confirmed at the end (phase-B LDS bound, passes)
    const bool nar_req = opt.narrow && desc.narrow && !f32 && !tagged && !var && clean && sb == kBinSB && levels == 1 &&
                         sa <= 16384 && (pack & 1u) && bin_narrow_degree(d);
    BinGeom G{};
    G.D = d;
    G.dp = dp;
    G.pad = f32 || nar_req ? 4u : 2u;
    G.npad_or = nar_req ? 0u : 1u;
    G.SA = sa;
    G.P = (uint32_t)((N + sa - 1) / sa);
    G.SB = sb;
    G.Q = (uint32_t)((NR + sb - 1) / sb);
    G.levels = levels;
    G.SR = sr;
    G.R = levels == 1 ? G.Q : (uint32_t)((NR + sr - 1) / sr);
    G.QR = sr / sb;
    G.PK = 1;
    if (levels == 2) {   // chunks of PK source blocks: an LDS image of about 16 Ki deliveries
        const double run1 = (double)NR * d / ((double)G.P * G.R);
        const uint32_t pk = (uint32_t)(opt.mimg / run1);   // target deliveries per phase-M image
        G.PK = pk < 1 ? 1 : pk > G.P ? G.P : pk;
    }
    G.K = (G.P + G.PK - 1) / G.PK;
    G.none1 = G.P * G.R;
    G.none2 = levels == 2 ? G.R * G.K * G.QR : 0;
    p.var = var;
    p.D = d;
    p.SA = sa;
    p.SB = sb;
    p.f32 = f32;
    p.P = G.P;
    p.Q = G.Q;
    p.levels = levels;
    p.E = NR * d;
    p.PK = G.PK;
    p.ngroups = levels == 2 ? G.R * G.K : 0;
    p.nrun = levels == 1 ? G.P : G.K;
    const uint64_t E = p.E;
    const uint64_t nt1 = (uint64_t)G.P * G.R;
    const uint64_t nt2 = levels == 2 ? (uint64_t)G.R * G.K * G.QR : 0;
    if (E >= (1ull << 32) || nt1 >= (1ull << 32) || nt2 >= (1ull << 32)) return hipErrorNotSupported;
    if ((uint64_t)p.nrun > (uint64_t)d * sb / 16) return hipErrorNotSupported;   // phase-B LDS bound
    const unsigned grid = (unsigned)((E + 255) / 256);

    // ---- level 1 (phase A): key (a, b) or (a, r)
    TileSort T1, T2;
    e = tile_sort(ell, E, G, 1, nt1, T1, s);
    p.Ep1 = T1.Ep;
    if (e == hipSuccess) e = hipMalloc(&p.idxA, p.Ep1 * 2);
    if (e == hipSuccess) e = hipMemsetAsync(p.idxA, 0, p.Ep1 * 2, s);
    if (e == hipSuccess) e = hipMalloc(&p.stage1, p.Ep1 * (f32 ? sizeof(float) : sizeof(double)));
    if (e == hipSuccess) e = hipMalloc(&p.aoff, ((uint64_t)G.P + 1) * sizeof(uint64_t));
    if (e == hipSuccess && tagged) e = hipMalloc(&p.xtag, (N + 2) * sizeof(double));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bin_fill_a, dim3(grid), dim3(256), 0, s, ell, E, G, T1.ks, T1.vs, T1.tl, T1.pstart, p.idxA);
        hipLaunchKernelGGL(k_bin_aoff, dim3((G.P + 256) / 256), dim3(256), 0, s, T1.pstart, G.P, G.R, p.Ep1, p.aoff);
        e = hipGetLastError();
    }
    // 14-bit packed phase-A indices (fp64 plans with source blocks of at most 2^14 senders).
    // ACSIM_BIN_PACK bit 0.  Measured per kernel (rocprofv3, cfg4,
    // profiles/r04_s8_pack_kernel_stats.csv): packed idxA 59.4 -> 53-54 us.  Packed phase-B
    // positions measured slower (62.5-63.0 against 61.7-61.8 us: the decode sits on phase B's
    // critical path) and were removed in round 5 (history: d8efbd1).
    if (e == hipSuccess && sa <= 16384) {   // fp64 and fp32 (bit 2 of ACSIM_BIN_PACK: no longer needed)
        if (pack & 1u) {
            const uint64_t nb = (p.Ep1 + 511) / 512;
            e = hipMalloc(&p.pkA, nb * kPk14Words * 4);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_bin_pack14, dim3((unsigned)((nb * 64 + 255) / 256)), dim3(256), 0, s, p.idxA, p.Ep1,
                                   p.pkA);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e == hipSuccess) {
                (void)hipFree(p.idxA);
                p.idxA = nullptr;
            }
        }
    }
    TileSort* last = &T1;
    if (e == hipSuccess && levels == 2) {
        // ---- level 2 (phase M): PK-run images per (r, k), regrouped by receiver block
        uint16_t* lpos = nullptr;
        uint32_t* cap = nullptr;
        const uint32_t ng = p.ngroups;
        e = hipMalloc(&p.mt, (uint64_t)ng * (G.PK + 1) * sizeof(uint2));
        if (e == hipSuccess) e = hipMalloc(&cap, (uint64_t)ng * 4);
        if (e == hipSuccess) e = hipMalloc(&lpos, E * 2);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_bin_mtiles, dim3((ng + 255) / 256), dim3(256), 0, s, T1.pstart, T1.plen, G, p.mt, cap);
            hipLaunchKernelGGL(k_bin_lpos, dim3(grid), dim3(256), 0, s, E, G, T1.ks, T1.vs, T1.tl, p.mt, lpos);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {   // every image must fit the phase-M LDS
            std::vector<uint32_t> h(ng);
            e = hipMemcpyAsync(h.data(), cap, (uint64_t)ng * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            uint32_t mx = 0;
            for (uint32_t v : h) mx = v > mx ? v : mx;
            p.mcap = mx;
            if (e == hipSuccess && mx > kBinMCap) e = hipErrorNotSupported;
        }
        if (e == hipSuccess) e = tile_sort(ell, E, G, 2, nt2, T2, s);
        p.Ep2 = T2.Ep;
        if (e == hipSuccess) e = hipMalloc(&p.idxM, p.Ep2 * 2);
        if (e == hipSuccess) e = hipMemsetAsync(p.idxM, 0, p.Ep2 * 2, s);
        if (e == hipSuccess) e = hipMalloc(&p.stage2, p.Ep2 * (f32 ? sizeof(float) : sizeof(double)));
        if (e == hipSuccess) e = hipMalloc(&p.moff, ((uint64_t)ng + 1) * sizeof(uint64_t));
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_bin_fill_m, dim3(grid), dim3(256), 0, s, E, T2.ks, T2.vs, T2.tl, T2.pstart, lpos, p.idxM,
                               G.none2);
            hipLaunchKernelGGL(k_bin_moff, dim3((ng + 256) / 256), dim3(256), 0, s, T2.pstart, G, p.Ep2, p.moff);
            e = hipGetLastError();
        }
        hipError_t e2 = hipStreamSynchronize(s);
        if (e == hipSuccess) e = e2;
        (void)hipFree(lpos);
        (void)hipFree(cap);
        last = &T2;
    }
    // ---- phase B tables over the last stage
    const uint64_t Qp = (uint64_t)G.Q * sb;   // receiver slots incl. the ragged last block's padding
    if (e == hipSuccess) e = hipMalloc(&p.tiles, ((uint64_t)p.nrun + 1) * G.Q * sizeof(uint2));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bin_prefix, dim3((G.Q + 255) / 256), dim3(256), 0, s, last->pstart, last->plen, last->tl, G,
                           p.nrun, p.tiles);
        e = hipGetLastError();
    }
    p.pol = opt.pol_set ? opt.pol & kPolMask : kPolDefault | (G.levels == 2 ? kPolTwoLevelStores : kPolOneLevelStores);
    if (e == hipSuccess) e = hipMalloc(&p.invpos, Qp * d * 2);
    if (e == hipSuccess) e = hipMemsetAsync(p.invpos, 0, Qp * d * 2, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bin_inv, dim3(grid), dim3(256), 0, s, E, G, p.nrun, last->ks, last->vs, last->tl,
                           p.tiles, p.invpos);
        e = hipGetLastError();
    }
    // fault fix-up list: when the faulty senders' deliveries are few (at most an
    // eighth of all), their resolutions are written into the stage instead of tagging every sender
    if (e == hipSuccess && tagged && desc.status && !opt.nofix) {
        // two passes: count (cap 0), then fill a list of exactly that size
        uint32_t* cnt = nullptr;
        uint32_t n = 0;
        e = hipMalloc(&cnt, sizeof(uint32_t));
        for (int pass = 0; pass < 2 && e == hipSuccess; ++pass) {
            if (pass == 1 && (n == 0 || (uint64_t)n > E / 8)) break;   // none, or too many to list
            if (pass == 1) e = hipMalloc(&p.fix, (uint64_t)n * sizeof(uint4));
            if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, sizeof(uint32_t), s);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_bin_fixlist, dim3(grid), dim3(256), 0, s, ell, E, G.D, G.dp,
                                   levels == 1 ? G.none1 : G.none2, last->ks, last->vs, last->tl, last->pstart,
                                   desc.status, p.fix, pass ? n : 0u, cnt);
                e = hipGetLastError();
            }
            uint32_t c = 0;
            if (e == hipSuccess) e = hipMemcpyAsync(&c, cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (pass == 0) n = c;
            else if (e == hipSuccess && c == n) p.nfix = n;
        }
        (void)hipFree(cnt);
        if (!p.nfix) {
            (void)hipFree(p.fix);
            p.fix = nullptr;
        }
    }
    hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    // NP-pass phase B: 2 passes by default where the whole image limits phase B to 2 workgroups
    // per CU (fp64, d = 32: 68 KiB of LDS; measured 72.7 -> 65.0 us on cfg4; fp32 images already
    // allow 4 and a second pass only costs: 39.3 -> 43.8 us), and only when every part of every
    // block's image fits.  ACSIM_BIN_SPLIT=1..4 overrides (1: one pass).
    p.split = 1;
    if (e == hipSuccess) {
        uint32_t np = opt.split ? opt.split : (!f32 && G.D == 32 ? 2u : 1u);
        // no more passes than the plan's phase B is compiled for: CSR plans one (the VAR kernels),
        // tagged fp32 one, tagged fp64 two, clean four
        np = std::min(np, bin_max_passes(f32, !tagged, var, kBinSB, false));
        if (np > 1) {
            const uint32_t D = G.D;
            const uint32_t cap = D * sb / np + D * sb / 16;   // kBinPartCap<D, np, sb>
            std::vector<uint2> h(((uint64_t)p.nrun + 1) * G.Q);
            e = hipMemcpy(h.data(), p.tiles, h.size() * sizeof(uint2), hipMemcpyDeviceToHost);
            bool fits = e == hipSuccess && p.nrun >= np;
            for (uint32_t b = 0; fits && b < G.Q; ++b) {
                const uint2* row = h.data() + (uint64_t)b * (p.nrun + 1);
                // the NP-pass kernel's skipped bound tests: part 0 starts at image offset 0, and the
                // image is non-empty (padding lanes read invpos 0, which must lie in the last part)
                fits = row[0].y == 0 && row[p.nrun].y > 0;
                for (uint32_t k = 0; fits && k < np; ++k)
                    fits = row[(k + 1) * p.nrun / np].y - row[k * p.nrun / np].y <= cap;
            }
            if (fits) p.split = np;
        }
    }
    // phase-A segmentation: for few source blocks one generation of workgroups per launch, a
    // multiple of the 4096-position super-step, covering the longest block.  A generation is 256
    // workgroups times the x images that fit a CU's 160 KiB of LDS together, at most 2: fp64
    // source blocks (128 KiB) take one per CU, each x block staged once per CU (measured 66-68 ->
    // 64 us against 512 workgroups on cfg4); fp32 ones (64 KiB) two, so that one stages its x block
    // while the other streams (round 6, profiles/r06_fp32_awg_ab.json: phase A 40.0 -> 33.7 us on
    // cfg4_f32 at 512 workgroups; 384 and 768 slower, as round 1 had measured 512 before the
    // packed stream)
    if (e == hipSuccess) {
        std::vector<uint64_t> h((uint64_t)G.P + 1);
        e = hipMemcpy(h.data(), p.aoff, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
        uint64_t mx = 0;
        for (uint32_t a = 0; a < G.P; ++a) mx = h[a + 1] - h[a] > mx ? h[a + 1] - h[a] : mx;
        // With more source blocks than CUs (cfg5-sized graphs: several generations anyway), shorter
        // workgroups of about 48 Ki deliveries measured faster: cfg5 phase A 2525 -> 2085 us at 6
        // segments per block (profiles/r01_s38_cfg5_awg.txt).
        const uint64_t fit = (160ull * 1024) / ((uint64_t)sa * (f32 ? 4 : 8) + 1024);
        const uint64_t gen = 256 * (fit >= 2 ? 2 : 1);
        uint64_t want = (gen + G.P - 1) / G.P;
        if (G.P > 256) want = (mx + 49151) / 49152;
        if (opt.awg) want = (opt.awg + G.P - 1) / G.P;   // phase-A workgroups per launch (sweeps)
        if (want == 0) want = 1;
        uint64_t ch = (mx + want - 1) / want;
        ch = ch < 8192 ? 8192 : ch;
        p.chunk = (uint32_t)((ch + 4095) / 4096 * 4096);
        p.segs = (uint32_t)((mx + p.chunk - 1) / p.chunk);
        if (p.segs == 0) p.segs = 1;
    }
    // narrow plans: every block's u32 image must fit the phase-B LDS of its instantiation (the
    // one- or two-pass kernel's buffer, in u32 entries), and the 8-byte rounds take one or two passes
    if (e == hipSuccess && nar_req && p.pkA && p.split <= 2) {
        const uint32_t raw_u32 = p.split == 2 ? 2u * (d * sb / 2 + d * sb / 16 + 2u) : 2u * (d * sb + d * sb / 16);
        std::vector<uint2> h(((uint64_t)p.nrun + 1) * G.Q);
        e = hipMemcpy(h.data(), p.tiles, h.size() * sizeof(uint2), hipMemcpyDeviceToHost);
        bool fits = e == hipSuccess;
        for (uint32_t b = 0; fits && b < G.Q; ++b) fits = h[(uint64_t)b * (p.nrun + 1) + p.nrun].y <= raw_u32;
        if (fits) e = hipMalloc(&p.nhdr, sizeof(uint4));
        if (fits && e == hipSuccess) e = hipMemset(p.nhdr, 0, sizeof(uint4));   // width 0: an 8-byte round
        p.narrow = fits && e == hipSuccess;
    }
    if (e == hipSuccess && opt.ts) {   // diagnostic workgroup timestamps
        p.ts_file = opt.ts_file;
        p.ts_a = (p.P + 7) / 8 * 8 * p.segs;
        p.ts_b = (p.Q + 7) / 8 * 8;
        p.ts_m = p.ngroups;
        e = hipMalloc(&p.ts, 3ull * (p.ts_a + p.ts_b + p.ts_m) * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMemset(p.ts, 0, 3ull * (p.ts_a + p.ts_b + p.ts_m) * sizeof(uint64_t));
    }
    T1.release();
    T2.release();
    return e;
}


}  // namespace acs
