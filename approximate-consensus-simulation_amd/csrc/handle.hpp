// handle.hpp — the handle behind the C ABI (struct acs_sim) and what its three translation units
// share: create.hip (validation, the creation stages, release), rounds.hip (the round-chunk loop
// with device-side early exit, node partitions, kernel event timing) and api.hip (extern "C").
#pragma once

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/acsim.h"
#include "engine.hpp"

// Sets the calling thread's acs_last_error text and returns `code` (api.hip).
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(ACS_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                              \
    } while (0)

#define NCCL_TRY(expr)                                                                    \
    do {                                                                                  \
        ncclResult_t r_ = (expr);                                                         \
        if (r_ != ncclSuccess)                                                            \
            return fail(ACS_ECOMM, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), \
                        __FILE__, __LINE__);                                              \
    } while (0)

// Inside a creation stage (create.hip): out of memory is ACS_ENOMEM, anything else ACS_EDEVICE.
// The stage returns the code; create_impl releases the handle.
#define STAGE_TRY(expr)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail((e_ == hipErrorOutOfMemory || e_ == hipErrorMemoryAllocation) ? ACS_ENOMEM : ACS_EDEVICE, \
                        "%s failed: %s", #expr, hipGetErrorString(e_));                   \
    } while (0)

enum Path { PATH_REGULAR = 0, PATH_GENERIC = 1, PATH_BATCHED = 2, PATH_DENSE = 3 };

// CSR plans (and hub rows beside them) share one partial-slot numbering between the binned phase B
// and the per-lane / generic kernels: their receiver blocks must agree.
static_assert(acs::kBinSB == acs::kRegularBlock, "CSR binned plans index partials by kRegularBlock-row blocks");

struct Part {              // one node partition's private copy (virtual partitions only)
    double* x[2] = {nullptr, nullptr};
    uint32_t* ell = nullptr;
    acs::BinnedPlan bin{};
};

struct acs_sim {
    acs_config c{};
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t N = 0, B = 0, m = 0;
    uint32_t d = 0, dp = 0;
    Path path = PATH_GENERIC;
    bool clean = true;
    bool ell_sorted = false;       // rows stored ascending (clean + order-independent rule)
    bool binned = false;           // PATH_REGULAR served by the binned exchange (round_binned.hip)
    bool defer_fin = false;        // binned, one instance, unpartitioned: a round's finalize runs inside
                                   // the next round's phase A (the last round of a chunk launches it)
    bool fin_pending = false;
    acs::FinalizeArgs fin_args{};
    bool mfma = false;             // PATH_BATCHED served by the MFMA group kernel (batched_mfma.hip)
    bool dense_persist = false;    // PATH_DENSE served by the persistent LDS-resident kernel
    acs::BinnedPlan bin{};
    acs::GenericBig big{};         // PATH_GENERIC receivers above kGenericMaxM entries (round_generic.hip)
    bool generic_small = true;     // PATH_GENERIC: some receiver has at most kGenericMaxM entries
    acs::MsgParams mp{};
    double* x[2] = {nullptr, nullptr};   // x[k] = xb(k): the synchronous double buffer
    double* xall = nullptr;        // H value buffers of B*Npad (+2) doubles, x^q in buffer q % H
    uint64_t xstride = 0;          // elements per buffer
    uint32_t es = 8;               // value bytes: 8 (ACS_F64) or 4 (ACS_F32)
    bool f32 = false;
    uint32_t H = 2;                // delay_max + 2: x^{r-D} .. x^r read, x^{r+1} written
    uint32_t* ell = nullptr;       // rows [row0, row0 + rows_per) of this rank
    uint32_t* status = nullptr;
    acs::InstState* st = nullptr;
    double2* partial = nullptr;
    uint32_t nblk = 0, nblk_init = 0;
    uint32_t* n_done = nullptr;
    double* trace = nullptr;
    uint32_t* h_ndone = nullptr;   // pinned [2]
    acs::RunSummary* h_sum = nullptr;   // pinned, host-mapped: the one-launch summary writes it directly
    acs::RunSummary* h_sum_dev = nullptr;   // h_sum's device address
    void* sum_scratch = nullptr;       // launch_run_summary_mapped's partials and arrival counter
    unsigned long long* eacc = nullptr;   // [2][kEaccWords] published EPS verdicts (RoundArgs::eacc), by round parity
    bool want_summary = false;     // acs_run on a one-launch path: enqueue the summary before the sync
    bool summary_ready = false;    // h_sum holds the summary of the current state
    unsigned long long sum_seq = 0;    // sequence number of the last summary launch (h_sum->seq)
    acs::MappedStates* h_ms = nullptr;      // pinned, host-mapped instance states (B <= kMappedStates), or null
    acs::MappedStates* h_ms_dev = nullptr;  // its device address
    unsigned long long ms_seq = 0;     // sequence number of the last launch_states_mapped
    bool ms_fresh = false;             // h_ms holds the states advance() ended with (acs_round reuses them)
    uint32_t round = 0;            // round of every unfinished instance
    bool all_done = false;
    // node partitioning: rank owns rows [rank*rows_per, (rank+1)*rows_per) ∩ [0, N)
    int nranks = 1, rank = 0;
    bool partitioned = false;      // node partition mode (virtual, or RCCL with >= 1 rank)
    bool virt = false;             // all nranks partitions simulated on this device
    uint64_t rows_per = 0, Npad = 0;
    ncclComm_t comm = nullptr;
    double2* gpart = nullptr;      // (-min, max) exchanged by all-reduce
    // chunked exchange (binned partitions): the round's rows in xchunks row chunks;
    // chunk k is sent on cstream as soon as its phase B finishes, and the next round's phase A for
    // the source blocks of chunk k starts as soon as chunk k has arrived from every rank
    uint32_t xchunks = 0;          // 0: the unchunked sequence (all-gather after the round)
    uint32_t bin_sa = 0;           // source-block size of the binned plans (chunks align to it)
    uint32_t bin_sb = 0;           // their phase-B receiver block, as decided for rows_per rows (an empty
                                   // last rank builds no plan of its own)
    hipStream_t cstream = nullptr;
    static constexpr uint32_t kMaxX = 8;
    hipEvent_t ev_b[kMaxX] = {}, ev_x[kMaxX] = {};
    hipEvent_t ev_fin = nullptr;
    uint64_t* rowptr = nullptr;    // CSR topology (device copies)
    uint32_t* colidx = nullptr;
    bool csr_var = false;          // CSR on the register / binned paths: padded ELL of a compiled degree
    uint8_t* deg = nullptr;        // [N] deg(i) (csr_var)
    uint8_t* sw = nullptr;         // [ceil(N/64)] SELL-64 slice widths in 4-wide groups (csr_var)
    // CSR hub rows (deg > d beside a fast path): the generic kernel over hub_ids (rows with at most
    // kGenericMaxM entries) and the big-m path (the rest); their partial slots follow the fast
    // path's nblk_fast block partials
    // CSR rows on the generic kernel go by size class (LDS per workgroup sized to the class):
    // gen_ids = the listed rows, class k = gen_ids[gcls[k].off, +n) with every m_i <= gcls[k].P;
    // row gen_ids[q]'s partial slot is gen_base + q
    struct GenClass {
        uint64_t off, n;
        uint32_t P;
    };
    uint32_t* crank = nullptr;     // fp32 tagged binned plans above 2^20 nodes with crash faults (RoundArgs::crank)
    uint32_t* clist = nullptr;
    std::vector<uint32_t> coff;    // [crash_window + 1] start of round r's crashing senders in clist
    uint32_t* gen_ids = nullptr;
    std::vector<GenClass> gcls;
    uint32_t gen_base = 0;
    uint64_t n_hub = 0;
    uint32_t nblk_fast = 0;
    // rule WEIGHTED: weights of the config dtype, shared by all instances
    bool weighted = false;
    uint64_t nnz = 0;              // rowptr[N] (CSR handles)
    void* wself = nullptr;         // [N]
    void* wedge = nullptr;         // [nnz] slot order (generic kernel, acs_get_weights)
    void* well = nullptr;          // the ELL's order (csr_var; RoundArgs::well)
    // rule PUSHSUM (a weighted handle too): (s, z) pairs of the config dtype beside x,
    // two buffers [B][N]; instance b at round r lives in buffer r & 1
    bool pushsum = false;
    void* pairs = nullptr;
    // ... under missing_policy = HOLD: the held (h, k) pair of every slot, one buffer [B][nnz] in CSR
    // slot order (the public order, and the one k_round_generic indexes), zeroed at create; the round
    // kernels update it in place.  Null for every other handle.
    bool hold = false;
    void* links = nullptr;
    // ... with messages in transit (handles of acs_create_csr_transit, never HOLD): a
    // message arrives up to tmax rounds after it is sent, and waits in a ring of tmax + 1 planes
    // [B][tmax + 1][nnz] of (h, k) pairs in slot order, zeroed at create; the cell of arrival round q
    // is in plane q mod (tmax + 1).  Null for every other handle.
    bool transit = false;
    uint32_t tmax = 0;
    void* ring = nullptr;
    // link schedule ("Link schedules"; handles of acs_create_csr_scheduled): the slots'
    // availability masks, shared by all instances, held twice: in slot order (the public view, and
    // the one k_round_generic indexes) and, on the per-lane path, in well's order (0 in absent columns)
    bool sched = false;
    uint32_t period = 0;
    uint32_t* avail = nullptr;     // [nnz]
    uint32_t* avell = nullptr;     // (csr_var; RoundArgs::avell)
    // rule PUSHSUM with per-round splitting (handles of acs_create_csr_split, which are
    // scheduled handles with no weights: wself, wedge, well and links stay null): the share table
    // [period][N] of the config dtype, and every node's offer beside its pair, two buffers [B][N] of
    // pairs by round parity
    bool split = false;
    void* share = nullptr;
    void* offers = nullptr;
    // rule WEIGHTED with quantized messages (handles of acs_create_csr_quantized): what
    // every node transmits, two buffers [B][N] of the config dtype by round parity, beside x
    bool quant = false;
    uint32_t qk = 0, qmode = 0, qdither = 0;   // step 2^-qk, ACS_QUANT_*, 0 / 1
    void* qbuf = nullptr;
    double* dsorted = nullptr;    // dense path: sorted base multiset [N]
    uint32_t* dcounts = nullptr;   // dense path: |B|, #Byzantine, #crash-silent
    std::vector<Part> parts;       // virtual partitions 1..P-1 (partition 0 uses x / ell)
    // kernel timing (bench)
    uint32_t timing = 0;           // 0 off, else bracket every timing-th round (sampling)
    bool timing_runs = false;      // bracket runs of `timing` consecutive rounds instead (one pair each)
    hipEvent_t run_end = nullptr;  // the open run's end event (recorded after its last round)
    uint32_t run_rounds = 0;       // rounds in the open run
    std::vector<uint32_t> ev_w;    // rounds covered by each event pair
    uint64_t timing_ctr = 0;
    std::vector<hipEvent_t> ev;    // pairs (start, stop)
    size_t ev_used = 0;
    double timed_ms = 0.0;
    uint64_t timed_launches = 0;
    std::string kname;             // kernel_name_of(this), assigned once when creation ends
};

// Rule PUSHSUM ("mass bound"): admitted |s| and the fp32 round limit, chosen together
// with the column-sum bound (csr_check.hpp kPushsumColMax) so that no sum of a run can overflow.
static constexpr double kPushsumMaxAbs64 = 1e290;
static constexpr float kPushsumMaxAbs32 = 1e26f;
static constexpr uint32_t kPushsumF32MaxRounds = 1u << 22;
// ... with messages in transit: a pending value passes through up to transit_max further additions,
// so the fp32 round limit is 2^26 / (16 + transit_max) (2^22 at transit_max = 0)
static constexpr uint32_t kTransitMax = 64;
static inline uint32_t transit_f32_max_rounds(uint32_t tmax) { return (1u << 26) / (16u + tmax); }

// Host memory the device writes and the host polls (run summary, instance states): mapped into the
// device's address space and explicitly COHERENT, so the device's system-scope release of the
// sequence number (and the fields stored before it) reaches host memory without a cache flush at
// the end of the kernel; the polling protocol (rounds.hip) depends on that and must not rest on the
// runtime's default or on HIP_HOST_COHERENT.  acs_runtime_info reports it.
static constexpr unsigned kPolledHostFlags = hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent;

// roctx range for the rocprofv3 --marker-trace timeline: host-side enqueue spans of
// handle creation, round chunks and the one-launch batched / dense paths.
struct RoctxRange {
    explicit RoctxRange(const char* m) { roctxRangePushA(m); }
    ~RoctxRange() { roctxRangePop(); }
};

// value buffer q % H holding x^q (typed double* for the kernels' argument structs; f32 kernels reinterpret)
static inline double* xb(const acs_sim* s, uint32_t q) {
    return reinterpret_cast<double*>(reinterpret_cast<char*>(s->xall) + (uint64_t)(q % s->H) * s->xstride * s->es);
}
// element k of a value buffer (byte arithmetic on the config's value size)
static inline void* xat(const acs_sim* s, const void* base, uint64_t k) {
    return const_cast<char*>(static_cast<const char*>(base)) + k * s->es;
}
// rule PUSHSUM: the pair buffer of round q (parity q & 1; synchronous rounds only)
static inline void* pairs_at(const acs_sim* s, uint32_t q) {
    return static_cast<char*>(s->pairs) + (uint64_t)(q & 1u) * s->B * s->N * 2 * s->es;
}
// ... with per-round splitting: the offer buffer of round q, and the shares of the phase round q runs in
static inline void* offers_at(const acs_sim* s, uint32_t q) {
    return static_cast<char*>(s->offers) + (uint64_t)(q & 1u) * s->B * s->N * 2 * s->es;
}
static inline void* share_at(const acs_sim* s, uint32_t q) {
    return static_cast<char*>(s->share) + (uint64_t)(q % s->period) * s->N * s->es;
}
// quantized messages: the buffer of what the nodes transmit in round q
static inline void* quant_at(const acs_sim* s, uint32_t q) {
    return static_cast<char*>(s->qbuf) + (uint64_t)(q & 1u) * s->B * s->N * s->es;
}
// rule PUSHSUM under HOLD: bytes of the link buffer (at least one pair, so the pointer is never null)
static inline uint64_t links_bytes(const acs_sim* s) { return (s->B * s->nnz ? s->B * s->nnz : 1) * 2 * s->es; }
// ... with messages in transit: bytes of one plane of one instance, and of the whole ring (at least
// one pair, so the pointer is never null)
static inline uint64_t plane_bytes(const acs_sim* s) { return s->nnz * 2 * s->es; }
static inline uint64_t ring_bytes(const acs_sim* s) {
    const uint64_t b = s->B * (s->tmax + 1) * plane_bytes(s);
    return b ? b : 2 * s->es;
}
static inline uint64_t part_row0(const acs_sim* s, int p) { return (uint64_t)p * s->rows_per; }
static inline uint64_t part_rows(const acs_sim* s, int p) {
    const uint64_t r0 = part_row0(s, p);
    if (r0 >= s->N) return 0;
    return s->N - r0 < s->rows_per ? s->N - r0 : s->rows_per;
}

// ---- create.hip
struct LinkSchedule {   // acs_create_csr_scheduled's arguments as given (sched_check.hpp checks them)
    uint32_t period;
    const uint32_t* avail;
    bool split = false;   // acs_create_csr_split: no weights, shares from the schedule (split_shares.hpp)
};
struct QuantSpec {      // acs_create_csr_quantized's arguments (api.hip checks them)
    uint32_t k, mode, dither;
};
int validate(const acs_config* c);   // §A.8 constraints
// A handle for a validated config (the callers in api.hip validate); *out is null on any failure.
int create_impl(const acs_config* cfg, int device, int nranks, int rank, const void* comm_id, uint64_t id_len,
                acs_sim** out, const uint64_t* h_rowptr = nullptr, const uint32_t* h_colidx = nullptr,
                const double* h_wself = nullptr, const double* h_wedge = nullptr,
                const LinkSchedule* h_sched = nullptr, int transit_max = -1,   // >= 0: acs_create_csr_transit
                const QuantSpec* h_quant = nullptr);                           // acs_create_csr_quantized
void release(acs_sim* s);

// ---- rounds.hip
// (Re)initialise the per-instance state from x[round & 1] (create and set_state).
int init_state(acs_sim* s, uint32_t round);
int advance(acs_sim* s, uint32_t k);   // every unfinished instance by at most k rounds
int read_states(acs_sim* s, std::vector<acs::InstState>& out, bool reuse_fresh = false);
int summary_and_wait(acs_sim* s);
int harvest_timing(acs_sim* s);
