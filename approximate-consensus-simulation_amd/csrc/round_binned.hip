// round_binned.hip — the sparse round (SURVEY §8(a) a5+a7+a8+a9: cfg4, cfg5) as a binned exchange.
//
// Why: the per-lane kernel (round_regular.hip) issues N·d random 8-byte gathers per round.  On
// MI355X each one moves a whole cache line into L1 (from L2 / MALL at cfg4, from HBM at cfg5), so
// the round is bound by line traffic, not by the algorithmic bytes per node.  Here
// every HBM access is a coalesced stream or a ≥ 1 KiB run, and the only random accesses are
// 8-byte LDS accesses.  A "delivery" is one (receiver i <- sender j, slot t) entry.
//
//   phase A  k_bin_scatter   workgroup = (source block a of SA senders, segment of its deliveries)
//            x[a·SA, (a+1)·SA) -> LDS by LDS-DMA, then a pure stream over the block's deliveries:
//            stage1[p] = lds[idxA[p]]                                  2 B read + 8 B write / delivery
//   phase M  k_bin_regroup   (two-level plans only: cfg5-sized graphs, where a (source block,
//            receiver block) tile would hold about one delivery)  workgroup = (receiver
//            super-block r, source-block chunk k): its PK runs of stage1 -> LDS by LDS-DMA, then
//            stage2[p] = lds[idxM[p]] grouped by receiver block         8 B + 2 B read + 8 B write
//   phase B  k_bin_gather    workgroup = receiver block b of kBinSB receivers (one lane each)
//            its runs of the last stage -> LDS by LDS-DMA, then per lane: own x_i, its d values at
//            invpos (LDS), the §A.7 rule in registers (rules.hpp), one store, block (min, max)
//            partial.                                                  8 B + 2 B read / delivery
//
// invpos is indexed by ELL slot t, so phase B sees receiver i's values in slot order: with the
// ELL in spec order (every config but the clean sort-based ones, whose rows are stored sorted)
// slot t is the spec slot s = i·d + t and the §A.5 drop draws, §A.4 crash draws and AVERAGE's
// entry-order sum all follow the spec exactly.
//
// Fault schedules (§A.4): phase B needs each delivered value's sender status.  Instead of a
// second exchange of status words, k_bin_tag rewrites x into xtag once per round: a sender that
// is Byzantine, crashing this round (partial) or crashed earlier (silent) is replaced by a quiet
// NaN whose payload holds that mode (x is never NaN, validated); phase A streams xtag instead of
// x, and phase B decodes the tag to the sender's §A.6 resolution.  A partial sender's message
// still delivers x_j when its per-slot draw passes, so its tag also carries j and phase B
// fetches x_j itself (n_faulty / crash_window senders per round at most).  +12 B read, +8 B
// written per node per round, against the 8·d B of random gathers the per-lane kernel spends.
#include <array>
#include <mutex>
#include <type_traits>
#include <utility>

// ACS_DIAG_B (variant builds only, tools/build_variant.sh; wrong values): the clean two-pass phase B
// without 1 its selection network, 2 its position-dependent pick-up, 3 its stage DMA, 4 its invpos
// stream (in-range synthetic positions)
#ifndef ACS_DIAG_B
#define ACS_DIAG_B 0
#endif

#include "binned_dev.hpp"

namespace acs {

// ------------------------------------------------------------------------------ phase A
template <typename VT = double>
__global__ __launch_bounds__(kBinA) void k_bin_scatter(const VT* __restrict__ x, const uint16_t* __restrict__ idxA,
                                                     const uint64_t* __restrict__ aoff, VT* __restrict__ stage,
                                                     const InstState* __restrict__ st, uint64_t N, uint32_t SA,
                                                     uint32_t segs, uint32_t chunk, uint32_t pol,
                                                     const FinalizeArgs fin, uint32_t fin_on, const SrcSel sel,
                                                     uint64_t* __restrict__ ts, unsigned long long* __restrict__ ereset,
                                                     const uint32_t* __restrict__ pkA, uint4* __restrict__ nhdr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lx_raw[];
    VT* lx = reinterpret_cast<VT*>(lx_raw);
    if (st->done) return;
    // this round's phase B publishes its verdict into ereset (the pair the previous phase B filled is
    // fin.eacc, read below; the next phase A reads this one)
    if (ereset && blockIdx.x == 0 && threadIdx.x < kEaccSlots) {
        unsigned long long* e = ereset + threadIdx.x * kEaccStride;
        __hip_atomic_store(e, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(e + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t t0 = ts ? __builtin_amdgcn_s_memrealtime() : 0;
    // XCD-aware order (dispatch deals blocks round-robin over the 8 XCDs): every segment of source
    // block a runs on the XCD of blockIdx % 8 = a % 8, so its x block is fetched into one L2 once
    // instead of once per XCD.  The grid is 8 * ceil(P / 8) * segs.
    const uint32_t slot = blockIdx.x >> 3;
    const uint32_t u = (slot / segs) * 8 + (blockIdx.x & 7u), sg = slot % segs;
    // selected source blocks (chunked partitioned rounds): launch-local block u -> global block a
    const uint32_t a = sel.n ? (u < sel.n ? (u / sel.bpc) * sel.bpr + sel.k0 + u % sel.bpc : 0xFFFFFFFFu) : u;
    // padding past the last source block, or a segment past its block's deliveries: idle (but
    // workgroup 0 still records a deferred finalize)
    const bool noblk = a == 0xFFFFFFFFu || (uint64_t)a * SA >= N;
    uint64_t p0 = 0, p1 = 0;
    if (!noblk) {
        const uint64_t s0 = aoff[a], s1 = aoff[a + 1];
        if (pkA) {
            // packed stream: the block's deliveries in `segs` equal parts cut at 512-position
            // boundaries (the stream's block grid), so no segment is short and no interior cut
            // needs the position-by-position head / tail decode
            auto cut = [&](uint32_t k) -> uint64_t {
                if (k == 0) return s0;
                if (k >= segs) return s1;
                const uint64_t c = (s0 + (s1 - s0) * k / segs + 256) & ~511ull;
                return c < s0 ? s0 : c > s1 ? s1 : c;
            };
            p0 = cut(sg);
            p1 = cut(sg + 1);
        } else {
            p0 = s0 + (uint64_t)sg * chunk;
            p1 = p0 + chunk < s1 ? p0 + chunk : s1;
        }
    }
    const bool idle = noblk || p0 >= p1;
    // (workgroup 0 always records the deferred finalize and, on narrow plans, the round's width)
    if (idle && !(blockIdx.x == 0 && (fin_on || nhdr))) return;
    const uint64_t base = (uint64_t)a * SA;
    const uint32_t n = idle ? 0u : (uint32_t)(N - base < SA ? N - base : SA);
    {   // x block -> LDS by LDS-DMA, 16 B per lane (x is allocated with spare elements, so the
        // last odd element's pair never reads past the buffer)
        constexpr uint32_t EPU = 16 / sizeof(VT);
        const uint32_t n16 = (n + EPU - 1) / EPU;
        const uint4* xs = reinterpret_cast<const uint4*>(x + base) + threadIdx.x;
        uint4* ld = reinterpret_cast<uint4*>(lx) + (threadIdx.x & ~63u);
        for (uint32_t o = 0; o < n16; o += kBinA)
            if (o + threadIdx.x < n16) __builtin_amdgcn_global_load_lds(xs + o, ld + o, 16, 0, 0);
    }
    // The (min, max) of x^r the previous phase B published (fin.eacc; plain loads: its atomics
    // completed before this launch began, and the kernel boundary makes them visible here as it
    // does x^r itself): the EPS verdict of workgroups other than 0, and on narrow plans (nhdr) the
    // round's stage entry width, which workgroup 0 records for phase B.  Every
    // workgroup reads the same pair, so all of them choose the same width.
    __shared__ uint32_t pub_done, nar_w;
    __shared__ unsigned long long nar_base;
    const bool pub_in = fin_on && fin.eacc;
    if (fin_on || nhdr) {
        if (threadIdx.x < 64) {
            unsigned long long lo = 0, hi = 0;
            if (pub_in && threadIdx.x < kEaccSlots) {
                lo = fin.eacc[threadIdx.x * kEaccStride];
                hi = fin.eacc[threadIdx.x * kEaccStride + 1];
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const unsigned long long l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
                lo = l2 > lo ? l2 : lo;
                hi = h2 > hi ? h2 : hi;
            }
            if (threadIdx.x == 0) {
                const double mn = ord_inv(~lo), mx = ord_inv(hi);
                const double spread = fin.f32 ? (double)(float)(mx - mn) : mx - mn;
                pub_done = pub_in && fin.term_eps && spread <= fin.eps ? 1u : 0u;
                uint32_t w = 8;
                unsigned long long base = 0;
                if (nhdr && pub_in) narrow_choose(~lo, hi, w, base);
                nar_w = w;
                nar_base = base;
                if (nhdr && blockIdx.x == 0) *nhdr = make_uint4((uint32_t)base, (uint32_t)(base >> 32), w, 0u);
            }
        }
    }
    if (fin_on) {
        // deferred finalize of the previous round.  Only workgroup 0 folds the
        // partials and records the verdict (the loads overlap the x staging above; the fold's
        // barrier drains both).  The other workgroups take the verdict the previous phase B
        // published (fin.eacc: the same exact min / max, so the same ε test), or without one stream
        // unconditionally unless the round cap is reached: if the EPS test has just ended the run,
        // their stage is never read, because phase B (the next launch) sees the done flag
        // workgroup 0 set and exits, and every later launch exits at its first line.  A finished
        // instance stops here.  (Every writer of the partials publishes: see the invariant where
        // rounds.hip enqueue_round chooses `pub`.)
        bool done;
        if (blockIdx.x == 0) {
            done = fold_partials<false, kBinA>(fin, 0, true);
        } else {
            __syncthreads();
            done = pub_done != 0u || fin.r_next >= fin.max_rounds;
        }
        if (done || idle) return;
    } else {
        __syncthreads();
    }
    // Uniform round (narrow plans, width 0: every x^r is one bit pattern): phase B
    // needs no stage, so nothing is streamed.  Workgroup 0 has recorded the header and the finalize
    // above.  Like the `done || idle` exit this one lies behind a barrier whose vmcnt(0) has landed
    // the x-block copies: no LDS-DMA write is in flight into LDS the CU's next workgroup will own.
    if (nhdr && nar_w == 0u) return;
    const uint64_t t1 = ts ? __builtin_amdgcn_s_memrealtime() : 0;
    const uint32_t smode = (pol & kPolSc1Store) ? 2u : (pol & kPolNtStore) ? 1u : 0u;
    if (pkA) {   // 14-bit packed indices
        if constexpr (sizeof(VT) == 8) {
            if (nhdr && nar_w == 4u) {   // narrow stage: u32 offsets from the round's base
                bin_stream_pk14_narrow(lx, pkA, reinterpret_cast<uint32_t*>(stage), p0, p1, smode, (uint32_t)nar_base);
                if (ts) bin_ts(ts, t0, t1);
                return;
            }
        }
        bin_stream_pk14(lx, pkA, stage, p0, p1, smode);
        if (ts) bin_ts(ts, t0, t1);
        return;
    }
    bin_stream(lx, idxA, stage, p0, p1, smode);
    if (ts) bin_ts(ts, t0, t1);
}

// ------------------------------------------------------------------------------ phase M
// mt[g][0..PK] (g = r*K + k): (stage1 start, image offset) of run (a = k*PK + j, r); entry PK holds
// the image size.  moff[g] .. moff[g+1]: the group's output range in stage2.
// VT = float for fp32 plans (runs padded to 4 elements, the image holds floats)
template <typename VT = double>
__global__ __launch_bounds__(kBinA) void k_bin_regroup(const VT* __restrict__ stage1, const uint2* __restrict__ mt,
                                                     const uint64_t* __restrict__ moff, const uint16_t* __restrict__ idxM,
                                                     VT* __restrict__ stage2, const InstState* __restrict__ st,
                                                     uint32_t PK, uint32_t pol, uint64_t* __restrict__ ts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lm_raw[];
    VT* lm = reinterpret_cast<VT*>(lm_raw);
    if (st->done) return;
    const uint64_t t0 = ts ? __builtin_amdgcn_s_memrealtime() : 0;
    const uint32_t g = blockIdx.x;
    constexpr uint32_t NW = kBinA / 64;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (pol & kPolAsmDmaT) {
        bin_dma_runs_asm_tb(mt + (uint64_t)g * (PK + 1), w * PK / NW, (w + 1) * PK / NW, stage1, lm);
        bin_dma_wait();
    } else {
        bin_dma_runs(mt + (uint64_t)g * (PK + 1), w * PK / NW, (w + 1) * PK / NW, stage1, lm);
    }
    __syncthreads();
    const uint64_t t1 = ts ? __builtin_amdgcn_s_memrealtime() : 0;
    bin_stream(lm, idxM, stage2, moff[g], moff[g + 1], (pol & kPolSc1StoreM) ? 2u : (pol & kPolNtStoreM) ? 1u : 0u);
    if (ts) bin_ts(ts, t0, t1);
}

// ------------------------------------------------------------------------------ phase B
// The runs of block b (run j of a table row of nrun + 1 descriptors) are copied into LDS,
// concatenated; lane i_local then reads its D values at invpos[b][t][i_local].
// quiet-NaN tag of a non-normal sender: payload bits 0-1 = 1 Byzantine, 2 crashing this round,
// 3 silent; bits 2-33 = the sender id (read back for mode 2; binned plans hold one instance, N < 2^32)
constexpr uint64_t kTagBase = 0x7FF8000000000000ull;

// fp32 plans use the binary32 quiet NaN 0x7FC00000 with the same payload layout in
// its 22 payload bits: bits 0-1 mode, bits 2-21 the sender id (N <= 2^20), or above 2^20 nodes the
// sender's rank among the round's crashing senders (RoundArgs::crank / clist; only mode 2 reads it)
constexpr uint32_t kTagBase32 = 0x7FC00000u;

__device__ __forceinline__ double bin_tag_value(uint64_t j, uint64_t mode, double) {
    return __longlong_as_double((long long)(kTagBase | j << 2 | mode));
}
__device__ __forceinline__ float bin_tag_value(uint64_t j, uint64_t mode, float) {   // 20-bit id field
    return __uint_as_float(kTagBase32 | (uint32_t)((j & 0xFFFFFu) << 2 | mode));
}

template <typename VT = double>
__global__ __launch_bounds__(256) void k_bin_tag(const VT* __restrict__ x, const uint32_t* __restrict__ status,
                                                 VT* __restrict__ xt, uint64_t N, uint32_t r,
                                                 const InstState* __restrict__ st, const uint32_t* __restrict__ crank) {
    if (st->done) return;
    const uint64_t j = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 2;
    if (j >= N) return;
    const uint32_t n = N - j >= 2 ? 2u : 1u;
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
        if (k >= n) break;
        const uint32_t sj = status[j + k];
        const uint64_t mode = sj == kHonest ? 0 : sj == kByz ? 1 : r < sj ? 0 : r == sj ? 2 : 3;
        // (crank: fp32 above 2^20 nodes, the id field holds the rank among round r's crashing senders)
        const uint64_t id = crank && mode == 2 ? crank[j + k] : j + k;
        xt[j + k] = mode ? bin_tag_value(id, mode, VT(0)) : x[j + k];
    }
}

// Fault fix-up: fix[k] = (stage position, local receiver row, slot t, sender j) for
// every delivery from a sender that is not honest.  Each round it writes the §A.4 / §A.6 resolution
// of that delivery into the last stage (Byzantine value, x_j, or a quiet NaN for a missing
// message); drops are phase B's.  The stream of phase A carried plain x there.
template <typename VT = double>
__global__ __launch_bounds__(256) void k_bin_fixup(const uint4* __restrict__ fix, uint32_t nfix, const RoundArgs a,
                                                   VT* __restrict__ stage, uint32_t D) {
    const InstState* S = a.st;
    if (S->done) return;
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nfix) return;
    const uint4 f = fix[k];
    const uint64_t i = a.row0 + f.y;
    const uint32_t stj = a.status[f.w];
    const uint64_t slot = a.rowptr ? a.rowptr[i] + f.z : i * D + f.z;
    const VT xj = reinterpret_cast<const VT*>(a.xin)[f.w];
    bool miss;
    const VT v = resolve_entry_m(a.mp, stj, xj, xj, false, (uint32_t)a.mp.inst_offset, a.r, (uint32_t)i, slot,
                                 (VT)S->lo, (VT)S->hi, miss);
    if constexpr (sizeof(VT) == 8)
        stage[f.x] = miss ? __longlong_as_double((long long)(kTagBase | 3u)) : v;
    else
        stage[f.x] = miss ? __uint_as_float(kTagBase32 | 3u) : v;
}


// VAR: a CSR graph padded to D (§8(f) row 1): slots t >= deg(i) are absent entries, slot numbers
// are rowptr[i] + t (one drop draw each); single pass only.
// Faulty NP > 1: the parts' LDS buffers admit 4 workgroups per CU, but the faulty bodies need more
// than the 128 VGPRs of 4 waves per SIMD (bounded to 4 they spilled 148-312 B/lane of scratch).
// The cfg4_byz shape (t = 5, not W-MSR) needs 163 with the drop mask drawn up front: 3 waves per
// SIMD (168 VGPRs), no scratch.  W-MSR and t = 0 (full 33-value sorts) need up to 203: 2.
// ACS_FAULTY_WPE overrides (variant builds).
#ifdef ACS_FAULTY_WPE
#define ACS_FAULTY_WPE_OF(T, W) ACS_FAULTY_WPE
#else
#define ACS_FAULTY_WPE_OF(T, W) ((T) == 5 && !(W) ? 3 : 2)
#endif
// FIX (fault fix-up plans): the stage already holds every faulty sender's resolved
// delivery (k_bin_fixup), a missing one as a quiet NaN; phase B draws the §A.5 drop mask, turns
// dropped and NaN entries into missing ones and applies the receiver's own status — no tag
// decoding, no Byzantine draws, clean-kernel registers.
// The narrow header as a scalar load (constant address space: phase A wrote it before this launch
// and nothing writes it during one, so the scalar cache may serve it; as a vector load the compiler
// made every workgroup wait for it alone before its first copies)
__device__ __forceinline__ uint4 bin_nhdr_load(const uint4* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) uint32_t* q = (const __attribute__((address_space(4))) uint32_t*)p;
    return make_uint4(q[0], q[1], q[2], q[3]);
#else
    return *p;
#endif
}

// NAR (narrow plans; clean fp64 only): each round reads the stage entry width
// phase A chose (a.nhdr); in a 4-byte round the whole image of u32 offsets is copied in one pass
// into the same LDS and every pick-up adds the round's base to recover the value's bits.
template <int D, int T, bool WMSR = false, bool FAULTY = false, typename VT = double, int NP = 1, bool VAR = false,
          bool FIX = false, int SB = (int)kBinSB, bool NAR = false>
__global__ __launch_bounds__(SB, FAULTY && NP > 1 ? ACS_FAULTY_WPE_OF(T, WMSR) : (FIX || NAR) && NP > 1 && (T || WMSR) ? 4 : 1) void k_bin_gather(const RoundArgs a, const VT* __restrict__ stage,
                                                       const uint16_t* __restrict__ invpos,
                                                       const uint2* __restrict__ tiles, uint32_t nrun, uint32_t Q,
                                                       uint32_t Qc, uint32_t pol) {
    static_assert(D % 8 == 0, "invpos is read 8 slots at a time");
    static_assert(!(FIX && FAULTY), "FIX replaces the tagged resolution");
    static_assert(!NAR || (sizeof(VT) == 8 && !FAULTY && !FIX && !VAR), "narrow stages: clean fp64 plans");
    constexpr bool FLT = FAULTY || FIX;   // a fault schedule or loss: receiver status and drop mask
    // runs are padded to 16-byte multiples; nrun <= D*SB/16 (checked when the plan is built)
    __shared__ __attribute__((aligned(16)))
    VT raw[NP > 1 ? kBinPartCap<D, NP, SB> + 16 / sizeof(VT) : D * SB + D * SB / 16 * (16 / sizeof(VT) - 1)];
    InstState* S = a.st;
    if (S->done) return;
    const uint64_t t0 = a.ts ? __builtin_amdgcn_s_memrealtime() : 0;
    uint64_t t1 = 0;
    // XCD-aware order: consecutive receiver blocks (which share the lines at their tile-run
    // seams) run on the same XCD (dispatch is round-robin over the 8 XCDs by blockIdx)
    const uint32_t b = a.qlo + (blockIdx.x & 7u) * Qc + (blockIdx.x >> 3);
    if (b >= a.qhi) return;   // past this launch's block range
    if (b >= Q) {   // partial slots past this partition's blocks: neutral (the finalize folds a.nblk)
        if (b < a.nblk && threadIdx.x == 0) a.partial[b] = make_double2(kInf, -kInf);
        return;
    }
    constexpr uint32_t NW = SB / 64;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t li = (uint64_t)b * SB + threadIdx.x;   // local row
    const uint64_t i = a.row0 + li;                              // global receiver
    bool live = li < a.nrows;
    if constexpr (VAR) {   // CSR hub rows (no deliveries in the plan): the generic kernel serves them
        if (live && a.deg[i] == kDegHub) live = false;
    }
    const uint2* tb = tiles + (uint64_t)b * (nrun + 1);
    // narrow plans: this round's stage entry width (4: u32 offsets from the base in .x/.y), read
    // after the first loads this workgroup needs anyway, so that one wait covers both (read first,
    // it was waited for alone ahead of them: phase B +4-5 us in 8-byte rounds)
    // Width 0 is a uniform round: every x^r is the bit pattern in .x/.y, so the D + 1 inputs of every
    // receiver are known from the header alone (no stage, no LDS image, no invpos).
    uint4 nh = make_uint4(0u, 0u, 8u, 0u);
    bool nar = false, uni = false;
    // NP-pass blocks of at most 64 runs: every wave fetches all descriptors first (one per lane)
    // and issues part 0's DMA before anything else is in flight, so the only wait ahead of the
    // first transfer is the descriptor load itself; later parts issue from registers.
    const bool pf = NP > 1 && nrun <= 64;
    // Clamped pick-up (kPolClampPick; two passes, prefetched descriptors, not the tagged kernels):
    // part 0 lies END-aligned in the buffer (image position p at raw[p + cap - hi0]) and part 1
    // start-aligned (p at raw[p - lo1]); raw[cap] holds zeros.  A slot's index, clamped to cap, then
    // reads its value in its own part and +0 bits in the other, and the two reads are OR-merged: no
    // compare or select per slot and part.
    uint2 pdsc = make_uint2(0u, 0u);
    uint32_t pnxt = 0;
    constexpr uint32_t cap = kBinPartCap<D, NP, SB>;
    const bool clampm = NP == 2 && sizeof(VT) == 8 && !FAULTY && pf && (pol & kPolClampPick);
    uint32_t hi0 = 0;
    const bool adma = clampm && (pol & kPolAsmDma);   // asm saddr LDS-DMA (binned_dev.hpp)
    uint32_t ppk = 0;                                   // this lane's run: image offset | 16-B units << 16
    if (pf) {
        const uint32_t lane = threadIdx.x & 63;
        if (lane < nrun) {
            pdsc = tb[lane];
            pnxt = tb[lane + 1].y;
        }
        if constexpr (NAR) {
            asm volatile("" ::: "memory");   // (issued after the descriptor loads)
            nh = bin_nhdr_load(a.nhdr);
            nar = nh.z == 4u;
            uni = nh.z == 0u;
        }
        const uint32_t j1 = nrun / NP;
        hi0 = __builtin_amdgcn_readlane(pdsc.y, j1);
        if (adma) ppk = pdsc.y | ((pnxt - pdsc.y) / (16 / sizeof(VT))) << 16;
        if (!nar && !uni) {   // (a narrow round copies its whole u32 image below, a uniform one nothing)
            if (adma)
                bin_dma_runs_asm(pdsc.x, ppk, w * j1 / NW, (w + 1) * j1 / NW, stage, raw, hi0 - cap);
            else
                bin_dma_runs_pf(pdsc, pnxt, w * j1 / NW, (w + 1) * j1 / NW, stage, raw, clampm ? hi0 - cap : 0u);
        }
    }
    if constexpr (NP > 1) {
        if (clampm && !nar && !uni && threadIdx.x < 16 / sizeof(VT)) raw[cap + threadIdx.x] = VT(0);   // +0 bits
    }
    // ordinary loads next (their wait is the barrier's vmcnt(0) anyway)
    // (x_i is the header's value in a uniform round and unused there since the rule runs once per
    // workgroup; with the rule in every lane, skipping the load had measured slower: DESIGN.md §5.15)
    const VT xi = live ? reinterpret_cast<const VT*>(a.xin)[i] : VT(0);
    uint32_t si = kHonest;
    if constexpr (FLT) {
        if (a.status && live) si = a.status[i];
    }
    uint32_t dg = D;
    uint64_t rp = 0;
    if constexpr (VAR) {
        if (live) {
            dg = a.deg[i];
            if constexpr (FLT) rp = a.rowptr[i];
        }
    }
    // §A.5 drop decisions of the lane's D slots as a bit mask, drawn before the values arrive: the
    // Philox state is then dead while the D + 1 values are live (drawn inside the resolution loop
    // below, the faulty two-pass kernels spilled 36-49 VGPRs at their 128-VGPR bound, and the CSR
    // slot loop — one draw per slot — was too large to unroll, so v[] went to scratch)
    uint32_t dmask = 0;
    if constexpr (FLT) {
        static_assert(D <= 32, "one drop bit per slot in a 32-bit mask");
        const MsgParams& mp = a.mp;
        if (mp.thr && live) {
            const uint32_t bI = (uint32_t)mp.inst_offset, bG = bI - bI % mp.mask_group;
            if constexpr (!VAR) {
#pragma unroll
                for (int q = 0; q < D / 4; ++q) {
                    const U4 w = philox10((uint32_t)i * (uint32_t)(D / 4) + q, a.r, bG, kStreamDrop, mp.key);
#pragma unroll
                    for (int e = 0; e < 4; ++e) dmask |= (uint32_t)(w.v[e] < mp.thr) << (4 * q + e);
                }
            } else if (dg) {   // slots rowptr[i] .. + deg(i) - 1: one call per 4 consecutive slots
                const uint64_t c1 = (rp + dg + 3) >> 2;
                for (uint64_t c = rp >> 2; c < c1; ++c) {
                    const U4 w = philox10((uint32_t)c, a.r, bG, kStreamDrop, mp.key);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint64_t t = 4 * c + e - rp;   // wraps past 2^64 below rp: out of range
                        if (t < dg) dmask |= (uint32_t)(w.v[e] < mp.thr) << t;
                    }
                }
            }
        }
    }
    uint4 ip[D / 8];
    // position of slot t (compile-time t)
    auto pos_of = [&](int t) -> uint32_t {
        const uint4& u = ip[t / 8];
        const uint32_t wd = (t & 6) == 0 ? u.x : (t & 6) == 2 ? u.y : (t & 6) == 4 ? u.z : u.w;
        return (t & 1) ? wd >> 16 : wd & 0xFFFFu;
    };
    const uint4* ipp = reinterpret_cast<const uint4*>(invpos) + (uint64_t)b * (D / 8) * SB + threadIdx.x;
#if ACS_DIAG_B == 4   // diagnostic: no invpos stream; in-range synthetic positions (wrong values)
    if (true) {
#pragma unroll
        for (int q = 0; q < D / 8; ++q) {
            uint32_t w4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                w4[e] = ((8 * q + 2 * e) * SB + threadIdx.x) | ((8 * q + 2 * e + 1) * SB + threadIdx.x) << 16;
            ip[q] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        }
    } else
#endif
    // (skipped in a uniform round the kernel already knows of: the prefetched kernels, which read the
    // header first; the one-pass kernels learn the width after these loads)
    if (!uni) {   // once-read stream: nontemporal loads (phase B 80 -> 71 us on cfg4)
        using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
        const u32x4* ipn = reinterpret_cast<const u32x4*>(ipp);
#pragma unroll
        for (int q = 0; q < D / 8; ++q) {
            const u32x4 t4 = __builtin_nontemporal_load(ipn + q * SB);
            ip[q] = make_uint4(t4.x, t4.y, t4.z, t4.w);
        }
    }
    if constexpr (NAR) {
        if (!pf) {   // (one-pass kernels: after the x_i and invpos loads)
            asm volatile("" ::: "memory");
            nh = bin_nhdr_load(a.nhdr);
            nar = nh.z == 4u;
            uni = nh.z == 0u;
        }
    }
    VT v[D + 1];
    VT x0 = xi;   // the receiver's own input to the rule
    bool picked = false;
    if constexpr (NAR) {
        if (uni) {   // uniform round: every delivered value is the header's bit pattern (and so is x_i)
            const VT u = __longlong_as_double((long long)((uint64_t)nh.x | (uint64_t)nh.y << 32));
#pragma unroll
            for (int t = 0; t < D; ++t) v[1 + t] = u;
            x0 = u;   // (x_i is not used in a uniform round: the compiler may drop its load on this path)
            if (a.ts) t1 = __builtin_amdgcn_s_memrealtime();
            picked = true;
        } else if (nar) {   // narrow round: the block's u32 image in one pass, values = base + offset
            uint32_t* r32 = reinterpret_cast<uint32_t*>(raw);
            const uint32_t* s32 = reinterpret_cast<const uint32_t*>(stage);
            if (pf) {
                const uint32_t pk32 = pdsc.y | ((pnxt - pdsc.y) / 4u) << 16;
                bin_dma_runs_asm(pdsc.x, pk32, w * nrun / NW, (w + 1) * nrun / NW, s32, r32, 0u);
            } else {
                bin_dma_runs_asm_tb(tb, w * nrun / NW, (w + 1) * nrun / NW, s32, r32);
            }
            bin_dma_wait();
            __syncthreads();
            if (a.ts) t1 = __builtin_amdgcn_s_memrealtime();
            const uint64_t base = (uint64_t)nh.x | (uint64_t)nh.y << 32;
#pragma unroll
            for (int t = 0; t < D; ++t) v[1 + t] = __longlong_as_double((long long)(base + r32[pos_of(t)]));
            picked = true;
            // (the rule, store and partial below are shared with the 8-byte path; a separate copy
            // here measured slower in both kinds of round: narrow 44.5 against 42.5 us)
        }
    }
    if (picked) {
    } else if constexpr (NP == 1) {
        if (pol & kPolAsmDmaT) {
            bin_dma_runs_asm_tb(tb, w * nrun / NW, (w + 1) * nrun / NW, stage, raw);
            bin_dma_wait();
        } else {
            bin_dma_runs(tb, w * nrun / NW, (w + 1) * nrun / NW, stage, raw);
        }
        __syncthreads();
        if (a.ts) t1 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
        for (int t = 0; t < D; ++t) v[1 + t] = raw[pos_of(t)];
    } else if (sizeof(VT) == 8 && clampm && !FLT && (pol & kPolBytePick)) {
        // Packed 16-bit pick-up (kPolBytePick, clean plans).  A u32 of invpos holds
        // two slots' positions: one v_pk_add_u16 shifts both into the part's buffer frame, one
        // v_pk_min_u16 clamps both to the zero slot at cap, and each becomes a byte offset by one
        // shift (the low half by an SDWA shift of its WORD_0; the high half by >> 13, exact because
        // both clamped halves are < cap < 2^13, so the low half's bits 13-15 are zero).  Part 1's
        // value is merged by one fp64 add: +0.0 is the identity for every value a clean round
        // carries (finite, never -0.0).  2 VALU per slot and part + 1 per slot for the merge,
        // against 3 + 3 + 2.  Positions p + (cap - hi0) stay below 2^16 (p < 2^14, cap < 2^13), and
        // p - lo1 for a part-0 slot wraps to at least 2^16 - 2^14 > cap.
        static_assert(cap < 8192, "two clamped positions per u32: each below 2^13");
        using us2 = unsigned short __attribute__((ext_vector_type(2)));
        const us2 cap2 = {(unsigned short)cap, (unsigned short)cap};
        const unsigned char* rb = reinterpret_cast<const unsigned char*>(raw);
        auto pick = [&](uint32_t word, const us2 sh, bool sub, VT& lo, VT& hi) {
            us2 q = __builtin_bit_cast(us2, word);
            q = sub ? q - sh : q + sh;
            q = __builtin_elementwise_min(q, cap2);
            const uint32_t qw = __builtin_bit_cast(uint32_t, q);
            uint32_t blo;
            asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
                : "=v"(blo) : "v"(qw));
            lo = *reinterpret_cast<const VT*>(rb + blo);
            hi = *reinterpret_cast<const VT*>(rb + (qw >> 13));
        };
        if (adma) bin_dma_wait();   // (the asm copies are not in the compiler's count)
        __syncthreads();
        if (a.ts) t1 = __builtin_amdgcn_s_memrealtime();
        uint32_t sh0 = cap - hi0;
        asm volatile("" : "+s"(sh0));   // (opaque: see the clamped branch below)
        const us2 s0 = {(unsigned short)sh0, (unsigned short)sh0};
#pragma unroll
        for (int q = 0; q < D / 8; ++q) {
            pick(ip[q].x, s0, false, v[1 + 8 * q], v[2 + 8 * q]);
            pick(ip[q].y, s0, false, v[3 + 8 * q], v[4 + 8 * q]);
            pick(ip[q].z, s0, false, v[5 + 8 * q], v[6 + 8 * q]);
            pick(ip[q].w, s0, false, v[7 + 8 * q], v[8 + 8 * q]);
        }
        __syncthreads();   // every lane has read part 0 before part 1 overwrites the buffer's front
        const uint32_t lo1 = hi0, j1 = nrun / NP;
        if (adma) {
            bin_dma_runs_asm(pdsc.x, ppk, j1 + w * (nrun - j1) / NW, j1 + (w + 1) * (nrun - j1) / NW, stage, raw, lo1);
            bin_dma_wait();
        } else {
            bin_dma_runs_pf(pdsc, pnxt, j1 + w * (nrun - j1) / NW, j1 + (w + 1) * (nrun - j1) / NW, stage, raw, lo1);
        }
        __syncthreads();
        uint32_t l1 = lo1;
        asm volatile("" : "+s"(l1));
        const us2 s1 = {(unsigned short)l1, (unsigned short)l1};
#pragma unroll
        for (int q = 0; q < D / 8; ++q) {
            const uint32_t wd[4] = {ip[q].x, ip[q].y, ip[q].z, ip[q].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                VT u0, u1;
                pick(wd[e], s1, true, u0, u1);
                v[1 + 8 * q + 2 * e] = v[1 + 8 * q + 2 * e] + u0;
                v[2 + 8 * q + 2 * e] = v[2 + 8 * q + 2 * e] + u1;
            }
        }
    } else if (sizeof(VT) == 8 && clampm) {
        const uint32_t lo1 = hi0;
        // part 0
        if (adma) bin_dma_wait();
        __syncthreads();
        if (a.ts) t1 = __builtin_amdgcn_s_memrealtime();
        uint32_t sh0 = cap - hi0;
        // opaque to the compiler: it otherwise computes (p - lo1) once for both parts, p - lo1 + cap
        // for part 0 (two VALU instead of one SDWA add) and keeps the 32 differences live across
        asm volatile("" : "+s"(sh0));
#pragma unroll
        for (int t = 0; t < D; ++t) {
#if ACS_DIAG_B == 2   // diagnostic: conflict-free reads that ignore the positions (kept live)
            asm volatile("" ::"v"(pos_of(t)));
            v[1 + t] = raw[(t * SB + threadIdx.x) % cap];
#else
            const uint32_t q = pos_of(t) + sh0;
            v[1 + t] = raw[q < cap ? q : cap];
#endif
        }
        __syncthreads();   // every lane has read part 0 before part 1 overwrites the buffer's front
        if (adma) {
            bin_dma_runs_asm(pdsc.x, ppk, nrun / NP + w * (nrun - nrun / NP) / NW,
                             nrun / NP + (w + 1) * (nrun - nrun / NP) / NW, stage, raw, lo1);
            bin_dma_wait();
        } else {
            bin_dma_runs_pf(pdsc, pnxt, nrun / NP + w * (nrun - nrun / NP) / NW,
                            nrun / NP + (w + 1) * (nrun - nrun / NP) / NW, stage, raw, lo1);
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < D; ++t) {
#if ACS_DIAG_B == 2
            const VT u = raw[(t * SB + threadIdx.x + 7) % cap];
#else
            const uint32_t q = pos_of(t) - lo1;   // wraps above cap below lo1
            const VT u = raw[q < cap ? q : cap];
#endif
            using UB = std::conditional_t<sizeof(VT) == 8, uint64_t, uint32_t>;
            v[1 + t] = __builtin_bit_cast(VT, (UB)(__builtin_bit_cast(UB, v[1 + t]) | __builtin_bit_cast(UB, u)));
        }
    } else {
#pragma unroll
        // Unrolled: the first part skips the p >= lo test and the last part the p < hi test.  This
        // relies on two invariants of the plan (binned_build checks both on the host): tb[0].y == 0
        // (lo of part 0), and every lane's invpos — live lanes and the zero-filled padding lanes of
        // a ragged last block alike — is below tb[nrun].y (hi of the last part).
        for (uint32_t k = 0; k < (uint32_t)NP; ++k) {
            const uint32_t j0 = k * nrun / NP, j1 = (k + 1) * nrun / NP;
            uint32_t lo, hi;   // image range of this part (pad-unit aligned)
            if (pf) {
                lo = __builtin_amdgcn_readlane(pdsc.y, j0);
                hi = j1 < nrun ? __builtin_amdgcn_readlane(pdsc.y, j1) : __builtin_amdgcn_readlane(pnxt, nrun - 1);
            } else {
                lo = tb[j0].y;
                hi = tb[j1].y;
            }
            if (k) __syncthreads();   // every lane has read the previous part before it is overwritten
            if (pf) {
                if (k) bin_dma_runs_pf(pdsc, pnxt, j0 + w * (j1 - j0) / NW, j0 + (w + 1) * (j1 - j0) / NW, stage, raw, lo);
            } else {
                bin_dma_runs(tb, j0 + w * (j1 - j0) / NW, j0 + (w + 1) * (j1 - j0) / NW, stage, raw, lo);
            }
            __syncthreads();
            if (k == 0 && a.ts) t1 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
            for (int q = 0; q < D / 8; ++q) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t p0 = pos_of(8 * q + 2 * e), p1 = pos_of(8 * q + 2 * e + 1);
                    const bool in0 = (k == 0 || p0 >= lo) && (k + 1 == (uint32_t)NP || p0 < hi);
                    const bool in1 = (k == 0 || p1 >= lo) && (k + 1 == (uint32_t)NP || p1 < hi);
                    // (faulty kernels: exec-masked reads straight into v; the clamped read + select
                    // holds the old and the new values together: 148-312 B/lane of scratch at their
                    // 128-VGPR bound)
                    if (!FAULTY && (pol & kPolBfPick)) {   // every lane reads (offset 0 when out of this part), then selects
                        const VT t0 = raw[in0 ? p0 - lo : 0u], t1 = raw[in1 ? p1 - lo : 0u];
                        v[1 + 8 * q + 2 * e] = in0 ? t0 : v[1 + 8 * q + 2 * e];
                        v[2 + 8 * q + 2 * e] = in1 ? t1 : v[2 + 8 * q + 2 * e];
                    } else {
                        if (in0) v[1 + 8 * q + 2 * e] = raw[p0 - lo];
                        if (in1) v[2 + 8 * q + 2 * e] = raw[p1 - lo];
                    }
                }
            }
        }
    }

    double mn = kInf, mx = -kInf;
    if constexpr (NAR) {
        // Narrow plans' tail (clean fp64: every lane honest and active).  In a uniform round the D + 1
        // inputs are the same for every receiver, so the rule's value is one number: wave 0 evaluates
        // it (every lane of it, live or not: the inputs do not depend on the lane) through the same
        // call site as the other rounds, and the workgroup takes it from LDS.  VALU time is paid per
        // wave, and 2^20 lanes evaluating it cost 16 384 evaluations of one value.
        VT res = VT(0);
        if (uni ? w == 0 : live) {
            v[0] = x0;
#if ACS_DIAG_B == 1
            if (NP == 2)
                res = tree_sum_const<D + 1>(v) / (VT)(D + 1);
            else
#endif
            res = apply_rule_reg<D, T, WMSR, true>(a.rule, v);
        }
        if (uni) {
            // (raw holds nothing in a uniform round: no part, no image and no zero slot was written.
            // The barrier is outside `live`: the dead waves of a ragged last block reach it too.)
            if (threadIdx.x == 0) raw[0] = res;
            __syncthreads();
            res = raw[0];
        }
        if (live) {
            bin_store_x<SB>(a, i, res, pol);
            mn = res;
            mx = res;
        }
        if (uni) {   // every live lane holds the same value R: the block's pair is (R, R)
            if (threadIdx.x == 0) {
                a.partial[b] = make_double2(res, res);
                if (a.eacc) publish_minmax(a.eacc, res, res);
            }
        } else {
            block_minmax_store<SB>(mn, mx, a.partial + b, a.eacc);
        }
        if (a.ts) bin_ts(a.ts, t0, t1);
        return;
    }
    if (live) {
        VT res = xi;
        if (!FLT || is_active(si, a.r)) {
            v[0] = xi;
            uint32_t nmiss = 0;   // entries left out under missing_policy = OMIT
            if constexpr (VAR && !FAULTY && !FIX) {   // absent CSR entries
#pragma unroll
                for (int t = 0; t < D; ++t)
                    if ((uint32_t)t >= dg) {
                        v[1 + t] = omit_fill<VT>(a.rule);
                        ++nmiss;
                    }
            }
            if constexpr (FAULTY) {   // §A.5 drops, §A.4 / §A.6 sender resolution (round_regular.hip order)
                const MsgParams& mp = a.mp;
                const uint32_t bI = (uint32_t)mp.inst_offset;
                const uint32_t r = a.r, iu = (uint32_t)i;
                const VT lo = (VT)S->lo, hi = (VT)S->hi;
#pragma unroll
                for (int q = 0; q < D / 4; ++q) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int t = 4 * q + e;
                        if (VAR && (uint32_t)t >= dg) {   // absent CSR entry
                            v[1 + t] = omit_fill<VT>(a.rule);
                            ++nmiss;
                            continue;
                        }
                        const uint64_t slot = VAR ? rp + t : (uint64_t)iu * D + t;
                        const bool dropped = (dmask >> t) & 1u;
                        VT u = v[1 + t];
                        uint32_t stj = kHonest;
                        if constexpr (sizeof(VT) == 8) {
                            const uint64_t bits = (uint64_t)__double_as_longlong(u);
                            if ((bits >> 51) == 0xFFFull) {
                                const uint32_t md = (uint32_t)(bits & 3u);
                                stj = md == 1 ? kByz : md == 2 ? r : r - 1;   // silent implies r >= 1
                                if (md == 2) u = reinterpret_cast<const VT*>(a.xin)[(bits >> 2) & 0xFFFFFFFFull];
                            }
                        } else {
                            const uint32_t bits = __float_as_uint(u);
                            if ((bits >> 22) == 0x1FFu) {
                                const uint32_t md = bits & 3u;
                                stj = md == 1 ? kByz : md == 2 ? r : r - 1;
                                if (md == 2) {
                                    const uint32_t f = (bits >> 2) & 0xFFFFFu;
                                    u = reinterpret_cast<const VT*>(a.xin)[a.clist ? a.clist[a.coff + f] : f];
                                }
                            }
                        }
                        bool miss;
                        const VT rv = resolve_entry_m(mp, stj, u, xi, dropped, bI, r, iu, slot, lo, hi, miss);
                        const bool out = mp.omit && miss;
                        v[1 + t] = out ? omit_fill<VT>(a.rule) : rv;
                        nmiss += out;
                    }
                }
            }
            if constexpr (FIX) {   // drops and the fix-up's missing entries (NaN) -> x_i (missing_policy
                                   // = SUBSTITUTE: OMIT configs keep the tagged path); absent CSR entries
#pragma unroll
                for (int t = 0; t < D; ++t) {
                    if (VAR && (uint32_t)t >= dg) {
                        v[1 + t] = omit_fill<VT>(a.rule);
                        ++nmiss;
                        continue;
                    }
                    const VT u = v[1 + t];
                    v[1 + t] = (((dmask >> t) & 1u) || u != u) ? xi : u;
                }
            }
            if (VAR || (FAULTY && a.mp.omit))
                res = apply_rule_reg_omit<D, T, WMSR>(a.rule, v, nmiss);
#if ACS_DIAG_B == 1   // diagnostic: the plain sum instead of the selection network (wrong values)
            else if (NP == 2 && !FLT)
                res = tree_sum_const<D + 1>(v) / (VT)(D + 1);
#endif
            else if constexpr (!FLT)   // padding adds skipped, exact for every input (sortnet.hpp)
                res = apply_rule_reg<D, T, WMSR, true>(a.rule, v);
            else
                res = apply_rule_reg<D, T, WMSR>(a.rule, v);
        }
        bin_store_x<SB>(a, i, res, pol);
        if (si == kHonest) {
            mn = res;
            mx = res;
        }
    }
    block_minmax_store<SB>(mn, mx, a.partial + b, a.eacc);
    if (a.ts) bin_ts(a.ts, t0, t1);
}

// ------------------------------------------------------------------------------ host side
bool binned_supported(uint32_t d, uint32_t t, uint32_t rule) {
    if (rule > 4) return false;
    if (rule == 0 && t != 0) return false;   // AVERAGE: entry order (the rows must be in spec order)
    if (rule == 3 && t < 1) return false;
    return bin_pair_compiled(d, t);
}

uint32_t binned_block_size(const BinnedOptions& opt, uint32_t d, uint32_t t, uint32_t rule, bool clean_fast) {
    return binned_sb_supported(d, t, rule, opt.sb, clean_fast) ? opt.sb : kBinSB;
}

// Source blocks above 8192 senders and phase-M images need more than 64 KiB of dynamic LDS.  The
// attribute belongs to the current device, so it is set once per device ordinal (a process may
// drive several devices from several threads).
static hipError_t binned_set_lds_attributes() {
    constexpr int kMaxDev = 64;
    static std::once_flag once[kMaxDev];
    static hipError_t status[kMaxDev];
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDev) return hipErrorInvalidDevice;
    std::call_once(once[dev], [dev] {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_bin_scatter<double>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 16384 * sizeof(double));
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_bin_scatter<float>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 16384 * sizeof(double));
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_bin_regroup<double>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (kBinMCap + 2) * sizeof(double));
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_bin_regroup<float>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (kBinMCap + 4) * sizeof(float));
        status[dev] = e;
    });
    return status[dev];
}

// ---- phase B: one typed launcher per row of kGatherTable (binned_select.hpp), the only place
// k_bin_gather is instantiated and launched
using GatherLaunch = void (*)(const BinnedPlan& p, const RoundArgs& a, const void* stage, uint32_t Qc, hipStream_t s);

template <size_t I>
static void launch_gather(const BinnedPlan& p, const RoundArgs& a, const void* stage, uint32_t Qc, hipStream_t s) {
    constexpr GatherKey k = kGatherTable.row[I];
    using VT = std::conditional_t<k.f32, float, double>;
    hipLaunchKernelGGL((k_bin_gather<(int)k.D, (int)k.T, k.wmsr, k.faulty, VT, (int)k.np, k.var, k.fix, (int)k.sb, k.nar>),
                       dim3(8 * Qc), dim3(k.sb), 0, s, a, static_cast<const VT*>(stage), p.invpos, p.tiles, p.nrun, p.Q,
                       Qc, p.pol);
}

template <size_t... I>
static constexpr std::array<GatherLaunch, sizeof...(I)> gather_launchers(std::index_sequence<I...>) {
    return {{&launch_gather<I>...}};
}
static constexpr auto kGatherLaunch = gather_launchers(std::make_index_sequence<kGatherVariants>{});

// One round's launches for a plan of value type VT.  tag: the senders are tagged first (slot-dependent
// rounds with a fault schedule and no fix-up); c: select_gather's choice of the phase-B kernel.
// wgt: rule WEIGHTED (fp64 CSR plans; round_binned_w.hip): k_bin_gather_w in the place of c's row.
template <typename VT>
static hipError_t round_binned(const BinnedPlan& p, const RoundArgs& a, bool tag, const GatherChoice& c, hipStream_t s,
                               const FinalizeArgs& fa, uint32_t fin_on, uint32_t phases, SrcSel sel, bool wgt = false) {
    constexpr bool kF32 = sizeof(VT) == 4;
    const uint32_t nsrc = sel.n ? sel.n : p.P;
    uint64_t* const ts_m = p.ts ? p.ts + 3ull * (p.ts_a + p.ts_b) : nullptr;
    const VT* src = reinterpret_cast<const VT*>(a.xin);
    if (tag) {
        // fp32: the 20-bit id field holds a sender id up to 2^20 nodes, beyond that a crash rank
        if (!p.xtag || (kF32 && a.N > (1ull << 20) && a.mp.fault == 1 && !a.crank)) return hipErrorInvalidValue;
        VT* xt = reinterpret_cast<VT*>(p.xtag);
        if (phases & 1)
            hipLaunchKernelGGL(k_bin_tag<VT>, dim3((unsigned)((a.N + 511) / 512)), dim3(256), 0, s, src, a.status, xt, a.N,
                               a.r, a.st, kF32 ? a.crank : nullptr);
        src = xt;
    }
    VT* last = reinterpret_cast<VT*>(p.stage1);
    if (phases & 1)   // (fp32 plans are never narrow: no nhdr)
        hipLaunchKernelGGL(k_bin_scatter<VT>, dim3((nsrc + 7) / 8 * 8 * p.segs), dim3(kBinA), p.SA * sizeof(VT), s, src,
                           p.idxA, p.aoff, last, a.st, a.N, p.SA, p.segs, p.chunk, p.pol, fa, fin_on, sel, p.ts, a.eacc,
                           p.pkA, kF32 || !c.nar ? nullptr : p.nhdr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (p.levels == 2) {   // phase B reads the regrouped stage (LDS: the image and one 16-byte unit)
        VT* st2 = reinterpret_cast<VT*>(p.stage2);
        if (phases & 2)
            hipLaunchKernelGGL(k_bin_regroup<VT>, dim3(p.ngroups), dim3(kBinA), (p.mcap + 16 / sizeof(VT)) * sizeof(VT), s,
                               last, p.mt, p.moff, p.idxM, st2, a.st, p.PK, p.pol, ts_m);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        last = st2;
    }
    if (c.fixp)
        hipLaunchKernelGGL(k_bin_fixup<VT>, dim3((p.nfix + 255) / 256), dim3(256), 0, s, p.fix, p.nfix, a, last, p.D);
    if constexpr (!kF32) {
        if (wgt) return (phases & 4) ? launch_bin_gather_w(p, a, last, (a.qhi - a.qlo + 7) / 8, s) : hipGetLastError();
    }
    if (phases & 4) kGatherLaunch[c.row](p, a, last, (a.qhi - a.qlo + 7) / 8, s);
    return hipGetLastError();
}

hipError_t launch_round_binned(const BinnedPlan& p, const RoundArgs& a0, bool clean, hipStream_t s,
                               const FinalizeArgs* fin, uint32_t phases, SrcSel sel) {
    if (hipError_t e = binned_set_lds_attributes(); e != hipSuccess) return e;
    RoundArgs a = a0;
    a.ts = p.ts ? p.ts + 3ull * p.ts_a : nullptr;
    // phase B writes a.partial[b] for each of its receiver blocks b < p.Q (and neutral pairs up to
    // a.nblk): partials sized for fewer blocks would be written past their slice
    if (((phases & 4u) && a.nblk < p.Q) || (p.narrow && !p.nhdr)) return hipErrorInvalidValue;
    // phase B block range: every partial slot by default (blocks past the plan's Q write neutral
    // partials), or the caller's [qlo, qhi)
    const uint32_t nslot_all = a.nblk > p.Q ? a.nblk : p.Q;
    if (a.qhi > nslot_all) a.qhi = nslot_all;
    if (a.qlo >= a.qhi) phases &= ~4u;
    const FinalizeArgs fa = fin ? *fin : FinalizeArgs{};
    if (a.rule == 5) {
        // Rule WEIGHTED: its phase B is no row of kGatherTable (GatherFacts::rule has no
        // meaning for it).  Whole rounds of an untagged fp64 CSR plan only, refused before any launch;
        // the phases then run exactly as for a clean or lossy VAR plan.
        if (!p.var || p.f32 || a.status || sel.n || p.narrow || !binned_weighted_supported(p.D) || !a.well ||
            !a.wself || !a.deg || (a.mp.thr && !a.rowptr))
            return hipErrorInvalidValue;
        a.nhdr = nullptr;
        return round_binned<double>(p, a, false, GatherChoice{GatherErr::kNone, 0, false, false}, s, fa, fin ? 1u : 0u,
                                    phases, sel, true);
    }
    const GatherChoice c = select_gather({p.D, a.trim, a.rule, p.f32, clean, a.status != nullptr, p.var, p.split, p.SB,
                                          p.narrow, p.fix != nullptr, phases, sel.n, a.mp.omit != 0});
    if (c.err == GatherErr::kInvalidValue) return hipErrorInvalidValue;
    a.nhdr = c.nar ? p.nhdr : nullptr;
    // a plan state without a compiled phase B: refused before anything is launched
    if ((phases & 4u) && c.err != GatherErr::kNone) return hipErrorNotSupported;
    const bool tag = !clean && a.status && !c.fixp;
    return p.f32 ? round_binned<float>(p, a, tag, c, s, fa, fin ? 1u : 0u, phases, sel)
                 : round_binned<double>(p, a, tag, c, s, fa, fin ? 1u : 0u, phases, sel);
}

}  // namespace acs
