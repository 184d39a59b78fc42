// create.hip — handle lifecycle: config validation, the environment's switches, kernel-path
// selection, HBM buffer ownership, graph / plan construction and release.  create_impl runs the
// creation stages in order; each returns an ACS code (message through fail) and create_impl
// releases the handle when one fails.  SURVEY §8(b), §8(e).
#include "csr_lane.hpp"
#include "handle.hpp"
#include "sched_check.hpp"
#include "split_shares.hpp"

using namespace acs;

// ------------------------------------------------------------------------- validation
// §A.8 constraints (restated here independently of the oracle's copy).
int validate(const acs_config* c) {
    if (!c) return fail(ACS_EINVAL, "null config");
    if (c->struct_size != sizeof(acs_config))
        return fail(ACS_EINVAL, "struct_size %u != %zu", c->struct_size, sizeof(acs_config));
    if (c->n_nodes < 1 || c->n_nodes > 0x7FFFFFFFull) return fail(ACS_EINVAL, "n_nodes out of range");
    if (c->n_instances < 1) return fail(ACS_EINVAL, "n_instances must be >= 1");
    if (c->instance_offset + c->n_instances > 0x100000000ull)
        return fail(ACS_EINVAL, "global instance ids must fit in u32");
    uint64_t m, slots;
    if (c->topology == ACS_TOPO_COMPLETE) {
        m = c->n_nodes;
        slots = c->n_nodes * c->n_nodes;
    } else if (c->topology == ACS_TOPO_RANDOM_REGULAR) {
        if (c->degree < 2 || (c->degree & 1u) || c->degree > 4096)
            return fail(ACS_EINVAL, "degree must be even, in [2, 4096]");
        m = (uint64_t)c->degree + 1;
        slots = c->n_nodes * (uint64_t)c->degree;
    } else if (c->topology == ACS_TOPO_CSR) {
        m = 0;       // per receiver: checked against the arrays in acs_create_csr
        slots = 0;
    } else {
        return fail(ACS_EINVAL, "unknown topology %u", c->topology);
    }
    if (slots >= (1ull << 34)) return fail(ACS_EINVAL, "slot count must be < 2^34");
    if (c->topology == ACS_TOPO_CSR) {
        if (c->rule > ACS_RULE_PUSHSUM) return fail(ACS_EINVAL, "unknown rule %u", c->rule);
        if (c->rule == ACS_RULE_AVERAGE && c->trim != 0) return fail(ACS_EINVAL, "AVERAGE requires trim == 0");
        if (c->rule == ACS_RULE_WEIGHTED && c->trim != 0) return fail(ACS_EINVAL, "WEIGHTED requires trim == 0");
        if (c->rule == ACS_RULE_PUSHSUM && c->trim != 0) return fail(ACS_EINVAL, "PUSHSUM requires trim == 0");
        if (c->rule == ACS_RULE_DLPSW_SELECT && c->trim < 1) return fail(ACS_EINVAL, "DLPSW needs t >= 1");
    } else
    switch (c->rule) {
        case ACS_RULE_AVERAGE:
            if (c->trim != 0) return fail(ACS_EINVAL, "AVERAGE requires trim == 0");
            break;
        case ACS_RULE_TRIMMED_MEAN:
        case ACS_RULE_MIDPOINT:
        case ACS_RULE_WMSR:
            if (m <= 2ull * c->trim) return fail(ACS_EINVAL, "need m > 2t");
            break;
        case ACS_RULE_DLPSW_SELECT:
            if (c->trim < 1 || m <= 2ull * c->trim) return fail(ACS_EINVAL, "DLPSW needs t >= 1, m > 2t");
            break;
        case ACS_RULE_WEIGHTED:
            return fail(ACS_EINVAL, "WEIGHTED needs a CSR graph with weights: use acs_create_csr_weighted");
        case ACS_RULE_PUSHSUM:
            return fail(ACS_EINVAL, "PUSHSUM needs a CSR graph with weights: use acs_create_csr_weighted");
        default:
            return fail(ACS_EINVAL, "unknown rule %u", c->rule);
    }
    if (c->fault_model == ACS_FAULT_NONE) {
        if (c->n_faulty != 0) return fail(ACS_EINVAL, "n_faulty must be 0 without a fault model");
    } else if (c->fault_model == ACS_FAULT_CRASH || c->fault_model == ACS_FAULT_BYZANTINE) {
        if ((uint64_t)c->n_faulty >= c->n_nodes) return fail(ACS_EINVAL, "n_faulty must be < n_nodes");
    } else {
        return fail(ACS_EINVAL, "unknown fault model %u", c->fault_model);
    }
    if (c->fault_model == ACS_FAULT_CRASH && (c->crash_window < 1 || c->crash_window > (1u << 30)))
        return fail(ACS_EINVAL, "crash_window must be in [1, 2^30]");
    if (c->fault_model == ACS_FAULT_BYZANTINE) {
        if (c->byz_strategy > ACS_BYZ_CONSTANT) return fail(ACS_EINVAL, "unknown byz strategy");
        if (!(fabs(c->byz_delta) <= 1e100) || !(fabs(c->byz_const) <= 1e100))
            return fail(ACS_EINVAL, "byz_delta / byz_const must be finite, |.| <= 1e100");
        if (c->byz_strategy == ACS_BYZ_RANDOM && slots > (1ull << 33))
            return fail(ACS_EINVAL, "BYZ RANDOM needs slot count <= 2^33");
    }
    if (!(c->loss_p >= 0.0 && c->loss_p < 1.0)) return fail(ACS_EINVAL, "loss_p must be in [0,1)");
    if (c->mask_group < 1) return fail(ACS_EINVAL, "mask_group must be >= 1");
    if (!(c->eps >= 0.0 && c->eps <= 1e300)) return fail(ACS_EINVAL, "eps must be finite, >= 0");
    if (c->termination > ACS_TERM_FIXED) return fail(ACS_EINVAL, "unknown termination");
    if (c->dtype != ACS_F64 && c->dtype != ACS_F32) return fail(ACS_EINVAL, "unknown dtype %u", c->dtype);
    if (c->dtype == ACS_F32 && c->fault_model == ACS_FAULT_BYZANTINE &&
        !(fabs(c->byz_delta) <= 1e30 && fabs(c->byz_const) <= 1e30))
        return fail(ACS_EINVAL, "fp32: byz_delta / byz_const must satisfy |.| <= 1e30");
    if (c->delay_max > 64) return fail(ACS_EINVAL, "delay_max must be <= 64");
    if (c->missing_policy > ACS_MISSING_HOLD) return fail(ACS_EINVAL, "unknown missing_policy %u", c->missing_policy);
    if (c->missing_policy == ACS_MISSING_HOLD && c->rule != ACS_RULE_PUSHSUM)
        return fail(ACS_EINVAL, "missing_policy = HOLD is defined for rule PUSHSUM only (got rule %u): held mass "
                                "needs (s, z) pairs", c->rule);
    if (c->trace_spread && c->n_instances * ((uint64_t)c->max_rounds + 1) > (1ull << 28))
        return fail(ACS_EINVAL, "spread trace too large (B*(max_rounds+1) > 2^28)");
    if (c->rule == ACS_RULE_PUSHSUM) {
        if (c->fault_model != ACS_FAULT_NONE)
            return fail(ACS_EINVAL, "PUSHSUM is not defined under faults: Byzantine and crash values are "
                                    "defined on x, not on (s, z) pairs");
        if (c->loss_p > 0.0 && c->missing_policy == ACS_MISSING_SELF)
            return fail(ACS_EINVAL, "PUSHSUM with loss_p > 0 needs missing_policy = OMIT: SELF would put the "
                                    "receiver's own pair in place of a lost message and create mass");
        if (c->delay_max > 0)
            return fail(ACS_EUNSUPPORTED, "PUSHSUM does not serve delay_max > 0: a stale read of (s, z) pairs creates and "
                                          "destroys mass; acs_create_csr_transit delays messages with their mass in transit");
        if (c->dtype == ACS_F32 && c->max_rounds > kPushsumF32MaxRounds)
            return fail(ACS_EINVAL, "PUSHSUM in fp32 needs max_rounds <= 2^22 (binary32 sums stay finite, DESIGN.md §9)");
    }
    return ACS_OK;
}

// ------------------------------------------------------------------------- the environment
// The binned exchange's knobs (engine.hpp BinnedOptions), read once per acs_create: tests change them
// between handles of one process.
BinnedOptions acs::binned_options_from_env(bool f32) {
    BinnedOptions o;
    const char* v;
    if ((v = getenv("ACSIM_BINNED"))) o.enabled = v[0] != '0';
    // 128 KiB of LDS per phase-A source block: 16 Ki fp64 or 32 Ki fp32 senders (anything else: the default)
    if ((v = getenv("ACSIM_BIN_SA"))) {
        const uint32_t sa = (uint32_t)strtoul(v, nullptr, 10);
        if (sa >= 64 && sa <= (f32 ? 32768u : 16384u) && !(sa & (sa - 1))) o.sa = sa;
    }
    if ((v = getenv("ACSIM_BIN_SB"))) o.sb = (uint32_t)strtoul(v, nullptr, 10);
    if ((v = getenv("ACSIM_BIN_SPLIT"))) {   // (anything but 1..4: one pass)
        o.split = (uint32_t)strtoul(v, nullptr, 10);
        if (o.split < 1 || o.split > 4) o.split = 1;
    }
    if ((v = getenv("ACSIM_BIN_PACK"))) o.pack = (uint32_t)strtoul(v, nullptr, 10);
    if ((v = getenv("ACSIM_BIN_POL"))) {
        o.pol_set = true;
        o.pol = (uint32_t)strtoul(v, nullptr, 0);
    }
    if ((v = getenv("ACSIM_BIN_MIMG")) && strtod(v, nullptr) > 0) o.mimg = strtod(v, nullptr);
    if ((v = getenv("ACSIM_BIN_AWG"))) o.awg = strtoull(v, nullptr, 10);
    o.nofix = getenv("ACSIM_BIN_NOFIX") != nullptr;
    if ((v = getenv("ACSIM_BIN_NARROW"))) o.narrow = v[0] != '0';   // (on by default)
    if ((v = getenv("ACSIM_BIN_WEIGHTED"))) o.weighted = v[0] != '0';   // (off by default)
    if ((v = getenv("ACSIM_BIN_TS"))) {
        o.ts = true;
        o.ts_file = v;
    }
    return o;
}

// Tuning / cross-check switches: ACSIM_<NAME>=0 turns an optional fast path off.
static bool env_off(const char* name) {
    const char* v = getenv(name);
    return v && v[0] == '0';
}

// Everything handle creation takes from the environment, read once at the top of create_impl
// (ACSIM_BATCH_SPLIT alone stays with its kernel, in batched_split_factor).
struct CreateOptions {
    bool mfma = true;            // ACSIM_MFMA=0: the VALU batched kernels for every N <= 64 batch
    bool defer_fin = true;       // ACSIM_DEFER_FIN=0: a k_finalize launch per binned round
    bool eps_pub = true;         // ACSIM_EPS_PUB=0: no verdict slots (phase B publishes nothing)
    bool dense_persist = true;   // ACSIM_DENSE_PERSIST=0: the two-kernel dense path at every size
    bool csr_fast = true;        // ACSIM_CSR_FAST=0: CSR graphs on the generic kernels only
    bool xchunks_set = false;    // ACSIM_XCHUNKS: chunks of the chunked exchange (unset: 4 for virtual
    uint32_t xchunks = 0;        // partitions, 0 for a multi-rank communicator)
    BinnedOptions bin;
};

static CreateOptions options_from_env(bool f32) {
    CreateOptions o;
    o.mfma = !env_off("ACSIM_MFMA");
    o.defer_fin = !env_off("ACSIM_DEFER_FIN");
    o.eps_pub = !env_off("ACSIM_EPS_PUB");
    o.dense_persist = !env_off("ACSIM_DENSE_PERSIST");
    o.csr_fast = !env_off("ACSIM_CSR_FAST");
    if (const char* v = getenv("ACSIM_XCHUNKS")) {
        o.xchunks_set = true;
        o.xchunks = (uint32_t)strtoul(v, nullptr, 10);
    }
    o.bin = binned_options_from_env(f32);
    return o;
}

static uint32_t drop_threshold(double p) {
    const double t = floor(p * 4294967296.0);   // §A.5, in fp64
    if (t <= 0.0) return 0u;
    if (t >= 4294967295.0) return 0xFFFFFFFFu;
    return (uint32_t)t;
}

// ------------------------------------------------------------------------- release
void release(acs_sim* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->cstream) (void)hipStreamSynchronize(s->cstream);
    if (s->comm) (void)ncclCommDestroy(s->comm);
    for (uint32_t k = 0; k < acs_sim::kMaxX; ++k) {
        if (s->ev_b[k]) (void)hipEventDestroy(s->ev_b[k]);
        if (s->ev_x[k]) (void)hipEventDestroy(s->ev_x[k]);
    }
    if (s->ev_fin) (void)hipEventDestroy(s->ev_fin);
    if (s->cstream) (void)hipStreamDestroy(s->cstream);
    for (hipEvent_t e : s->ev) (void)hipEventDestroy(e);
    for (Part& p : s->parts) {
        (void)hipFree(p.x[0]);
        (void)hipFree(p.x[1]);
        (void)hipFree(p.ell);
        binned_free(p.bin);
    }
    (void)hipFree(s->xall);
    (void)hipFree(s->ell);
    binned_free(s->bin);
    generic_big_free(s->big);
    (void)hipFree(s->status);
    (void)hipFree(s->st);
    (void)hipFree(s->partial);
    (void)hipFree(s->gpart);
    (void)hipFree(s->rowptr);
    (void)hipFree(s->colidx);
    (void)hipFree(s->deg);
    (void)hipFree(s->sw);
    (void)hipFree(s->wself);
    (void)hipFree(s->wedge);
    (void)hipFree(s->well);
    (void)hipFree(s->pairs);
    (void)hipFree(s->links);
    (void)hipFree(s->ring);
    (void)hipFree(s->avail);
    (void)hipFree(s->avell);
    (void)hipFree(s->share);
    (void)hipFree(s->offers);
    (void)hipFree(s->qbuf);
    (void)hipFree(s->gen_ids);
    (void)hipFree(s->crank);
    (void)hipFree(s->clist);
    (void)hipFree(s->dsorted);
    (void)hipFree(s->dcounts);
    (void)hipFree(s->n_done);
    (void)hipFree(s->trace);
    if (s->h_ndone) (void)hipHostFree(s->h_ndone);
    (void)hipFree(s->sum_scratch);
    if (s->h_sum) (void)hipHostFree(s->h_sum);
    if (s->h_ms) (void)hipHostFree(s->h_ms);
    if (s->eacc) (void)hipFree(s->eacc);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

// ------------------------------------------------------------------------- stage 2: path choice
// CSR on the register / binned paths (§8(f) row 1): the smallest compiled degree D >= the
// largest row with the config's (t, rule), 0 if none (the generic kernel then runs).
// (rules WEIGHTED and PUSHSUM have their own per-lane kernels, k_round_weighted<D> and
// k_round_pushsum<D> (under HOLD its HOLD instantiation), over the same padded rows and so of the
// same widths, csr_lane.hpp; WEIGHTED also a binned phase B, decide_binned)
static bool csr_width_compiled(uint32_t d, uint32_t t, uint32_t rule) {
    if (rule == ACS_RULE_WEIGHTED || rule == ACS_RULE_PUSHSUM) return t == 0 && csr_lane_fast_supported(d);
    return regular_fast_supported(d, t, rule);
}

static uint32_t csr_fast_degree(uint64_t maxdeg, uint32_t t, uint32_t rule) {
    for (uint32_t d : {4u, 8u, 16u, 32u})
        if (d >= maxdeg && csr_width_compiled(d, t, rule)) return d;
    return 0;
}

// CSR graphs whose largest degree is above every compiled degree: the largest compiled degree d
// (for this t and rule) whose hub rows (deg > d) are at most a quarter of the rows; 0 if none.
// The hub rows go to the generic kernel, the rest to the register / binned path padded to d.
static uint32_t csr_hub_degree(const uint64_t* rowptr, uint64_t N, uint32_t t, uint32_t rule, uint64_t* nhub) {
    for (uint32_t d : {32u, 16u, 8u, 4u}) {
        if (!csr_width_compiled(d, t, rule)) continue;
        uint64_t h = 0;
        for (uint64_t i = 0; i < N; ++i) h += rowptr[i + 1] - rowptr[i] > d;
        if (h * 4 <= N) {
            *nhub = h;
            return d;
        }
        return 0;   // smaller compiled degrees would only leave more hubs
    }
    return 0;
}

struct PathChoice {
    Path path = PATH_GENERIC;
    uint64_t m = 0;                // entries per receiver (CSR: the largest row's)
    uint32_t d = 0, dp = 0;        // degree (CSR: the compiled degree the rows are padded to, or 0), ELL row width
    bool csr_var = false;
    uint64_t n_hub = 0;
    bool mfma = false, dense_persist = false, generic_small = true;
};

// Which kernel family serves the config; csr_mmax: the largest CSR row's entries.
// Before any allocation: a config no path serves costs nothing to refuse.
// fp32 runs on the register, generic, batched (N <= 64), dense (persistent up to
// 4096 nodes, the two-kernel path up to 8192 since round 6) and binned kernels; the MFMA group
// kernel is fp64-only (its hardware-ordered sums would not keep fp32 rounds-to-convergence)
static int choose_path(const acs_config& c, const CreateOptions& o, bool partitioned, uint64_t csr_mmax,
                       const uint64_t* h_rowptr, PathChoice& pc) {
    const uint64_t N = c.n_nodes, B = c.n_instances;
    const uint64_t m = pc.m = c.topology == ACS_TOPO_COMPLETE ? N
                              : c.topology == ACS_TOPO_CSR    ? csr_mmax
                                                              : (uint64_t)c.degree + 1;
    const bool faults = c.fault_model != ACS_FAULT_NONE, f32 = c.dtype == ACS_F32;
    pc.d = c.topology == ACS_TOPO_CSR ? 0 : c.degree;
    pc.dp = (c.degree + 3u) & ~3u;
    if (c.topology == ACS_TOPO_COMPLETE && N <= kBatchedMaxN && c.delay_max == 0) {
        pc.path = PATH_BATCHED;
        pc.mfma = o.mfma && !f32 && batched_mfma_supported((uint32_t)N, c.rule, faults, c.mask_group, c.instance_offset);
    } else if (c.topology == ACS_TOPO_COMPLETE && !partitioned && c.delay_max == 0 &&
               (B == 1 || (N <= kDensePersistMaxN && o.dense_persist)) &&
               dense_supported(c.fault_model, c.byz_strategy, c.rule, drop_threshold(c.loss_p), N)) {
        pc.path = PATH_DENSE;
        pc.dense_persist = N <= kDensePersistMaxN && o.dense_persist;
    } else if (c.topology == ACS_TOPO_RANDOM_REGULAR && regular_fast_supported(pc.d, c.trim, c.rule)) {
        pc.path = PATH_REGULAR;
    } else if (c.topology == ACS_TOPO_CSR && o.csr_fast &&
               ((pc.d = csr_fast_degree(m - 1, c.trim, c.rule)) != 0 ||
                (pc.d = csr_hub_degree(h_rowptr, N, c.trim, c.rule, &pc.n_hub)) != 0)) {
        // §8(f) row 1: rows padded to the smallest compiled degree >= max deg(i) with the same t, or
        // (power-law graphs) to the largest compiled degree with the rows above it as hub rows
        pc.path = PATH_REGULAR;
        pc.csr_var = true;
        pc.dp = pc.d;
    } else if (m <= kGenericBigMaxM) {
        pc.path = PATH_GENERIC;
        pc.generic_small = !(c.topology == ACS_TOPO_COMPLETE && m > kGenericMaxM);
    } else {
        return fail(ACS_EUNSUPPORTED, "m = %llu entries per receiver exceeds the big-m generic path's %llu",
                    (unsigned long long)m, (unsigned long long)kGenericBigMaxM);
    }
    if (faults && N >= (1ull << 31))   // (any B: setup.hip batches instances)
        return fail(ACS_EUNSUPPORTED, "fault schedules need N < 2^31");
    return ACS_OK;
}

// ------------------------------------------------------------------------- stage 3: binned decision, partials
static uint64_t rows_local(const acs_sim* s) { return s->partitioned ? s->rows_per : s->N; }
// the per-lane kernel's receiver blocks (kRegularBlock rows each)
static uint32_t nblk_lane(const acs_sim* s) { return (uint32_t)((rows_local(s) + kRegularBlock - 1) / kRegularBlock); }

// Decides whether the binned exchange serves the handle (binned, defer_fin, bin_sa, bin_sb) and
// counts the block partials (nblk, nblk_fast, nblk_init).  Returns the partial buffer's capacity in
// slots per instance.
static uint64_t decide_binned(acs_sim* s, const CreateOptions& o) {
    const acs_config& c = s->c;
    const uint64_t nrows = rows_local(s);
    // binned exchange (round_binned.hip): one instance, synchronous rounds, and a graph shape with
    // one or two exchange levels (faults and loss are resolved in phase B from tagged values and
    // slot-order draws); ACSIM_BINNED=0 forces the per-lane kernel and ACSIM_BIN_SA sets the
    // source block size (tests use small blocks on small graphs).  Default 16 Ki for
    // fp32 too: 14-bit packed phase-A indices, and measured faster (cfg4_f32 82.2 -> 80.9 us per round,
    // cfg5_f32 4.69 -> 4.51 ms; profiles/r04_f32_sa_ab.jsonl); ACSIM_BIN_SA up to 32 Ki
    // (the order-free phase B of rounds 1-5, ACSIM_BIN_OF=1, measured slower than the invpos phase
    // B and was removed in round 6: DESIGN.md §5.1, §5.13)
    s->bin_sa = o.bin.sa;
    // phase-B receiver block (BinnedPlan::SB): the default, or ACSIM_BIN_SB where the clean (d, t)
    // pair has that instantiation; block partials follow it (one per receiver block)
    s->bin_sb = binned_block_size(o.bin, s->d, c.trim, c.rule, s->clean && !s->csr_var && s->path == PATH_REGULAR);
    const uint32_t lv =
        s->path == PATH_REGULAR && s->d ? binned_levels(s->N, nrows, s->d, s->bin_sa, s->bin_sb, nullptr) : 0;
    // fp32 tags carry a 20-bit sender field: above 2^20 nodes a crash schedule stores crash ranks
    // there (at most 2^20 senders may crash in one round: n_faulty <= 2^20)
    const bool f32_tags_ok = !s->f32 || s->clean || s->N <= (1ull << 20) || c.fault_model != ACS_FAULT_CRASH ||
                             c.n_faulty <= (1u << 20);
    // Rule WEIGHTED takes the exchange only where ACSIM_BIN_WEIGHTED asks for it: fp64
    // CSR rows padded to a degree with a weighted phase B and no fault schedule (loss is served: phase
    // B draws its own drop mask); every other weighted handle, and every PUSHSUM handle (16-byte
    // pairs), keeps its per-lane kernel; so does every handle with a link schedule (phase B has no
    // availability test) and every handle with quantized messages (phase A stages x, not what the nodes transmit).
    const bool rule_binned = s->weighted ? o.bin.weighted && c.rule == ACS_RULE_WEIGHTED && !s->f32 && s->csr_var && !s->sched &&
                                               !s->quant && c.fault_model == ACS_FAULT_NONE && binned_weighted_supported(s->d)
                                         : binned_supported(s->d, c.trim, c.rule);
    s->binned = o.bin.enabled && f32_tags_ok && s->path == PATH_REGULAR && c.delay_max == 0 &&
                !(s->csr_var && s->f32) &&
                // (CSR hub rows own the partial slots after the fast path's blocks; CSR plans
                // always take kBinSB = kRegularBlock receivers per block, so both paths agree:
                // static_assert in handle.hpp)
                s->B == 1 && lv != 0 && rule_binned && nrows * s->d < (1ull << 32);
    s->defer_fin = s->binned && !s->partitioned && s->B == 1 && o.defer_fin;
    // Block partials: one per receiver block of the round kernel.  The binned path's phase B writes
    // slot b of its bin_sb-row block b, the per-lane kernel slot b of its kRegularBlock-row block b;
    // a binned plan refused later falls back to the per-lane kernel (drop_binned), so the buffer
    // holds the larger count and nblk is reset to the per-lane count on that fallback
    // (launch_round_binned refuses a plan whose block count exceeds nblk).
    const uint32_t nblk_bin = (uint32_t)((nrows + s->bin_sb - 1) / s->bin_sb);
    s->nblk = s->path == PATH_REGULAR ? (s->binned ? nblk_bin : nblk_lane(s))
            : s->path == PATH_GENERIC ? (uint32_t)s->N
            : s->path == PATH_DENSE   ? dense_nblk(s->N)
                                      : 0u;
    s->nblk_fast = s->nblk;
    s->nblk += (uint32_t)s->n_hub;   // hub rows: one partial slot each, after the fast path's
    s->nblk_init = (uint32_t)((s->N + 255) / 256);
    if (s->nblk_init > 1024) s->nblk_init = 1024;
    const uint32_t nblk_max = s->path == PATH_REGULAR
                                  ? (nblk_bin > nblk_lane(s) ? nblk_bin : nblk_lane(s)) + (uint32_t)s->n_hub
                                  : s->nblk;
    // (virtual partitions: partition p's slice starts at p * nblk, with nblk the count in use)
    const uint64_t nround = (uint64_t)nblk_max * (s->virt ? s->nranks : 1);
    return nround > s->nblk_init ? nround : s->nblk_init;
}

// A binned plan that was refused once laid out (binned_build: hipErrorNotSupported): the per-lane
// kernel serves the rows, with its own block partials; hub rows keep the slots after them (n_hub
// is 0 on RANDOM_REGULAR graphs, and on CSR graphs nblk_lane equals the plan's count: kBinSB =
// kRegularBlock).
static void drop_binned(acs_sim* s) {
    binned_free(s->bin);
    for (Part& q : s->parts) binned_free(q.bin);
    s->binned = false;
    s->defer_fin = false;
    s->nblk_fast = nblk_lane(s);
    s->nblk = nblk_lane(s) + (uint32_t)s->n_hub;
}

// ------------------------------------------------------------------------- stage 4: state buffers
static int alloc_state(acs_sim* s, const CreateOptions& o, uint64_t ncap) {
    STAGE_TRY(hipSetDevice(s->device));
    STAGE_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    s->H = s->c.delay_max + 2;
    s->xstride = s->B * s->Npad + 4;   // +4 elements: 16-byte tail reads (binned phase A staging)
    STAGE_TRY(hipMalloc(&s->xall, s->H * s->xstride * s->es));
    s->x[0] = xb(s, 0);
    s->x[1] = xb(s, 1);
    STAGE_TRY(hipMalloc(&s->st, s->B * sizeof(InstState)));
    STAGE_TRY(hipMemsetAsync(s->st, 0, s->B * sizeof(InstState), s->stream));
    STAGE_TRY(hipMalloc(&s->partial, s->B * ncap * sizeof(double2)));
    STAGE_TRY(hipMalloc(&s->gpart, sizeof(double2)));
    if (s->path == PATH_DENSE) {
        STAGE_TRY(hipMalloc(&s->dsorted, s->N * sizeof(double)));
        STAGE_TRY(hipMalloc(&s->dcounts, 4 * sizeof(uint32_t)));
    }
    STAGE_TRY(hipMalloc(&s->n_done, sizeof(uint32_t)));
    STAGE_TRY(hipHostMalloc(&s->h_ndone, 2 * sizeof(uint32_t), hipHostMallocDefault));
    STAGE_TRY(hipHostMalloc(&s->h_sum, sizeof(RunSummary), kPolledHostFlags));
    STAGE_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&s->h_sum_dev), s->h_sum, 0));
    memset(s->h_sum, 0, sizeof(RunSummary));
    if (s->B <= kMappedStates) {
        STAGE_TRY(hipHostMalloc(&s->h_ms, sizeof(MappedStates), kPolledHostFlags));
        STAGE_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&s->h_ms_dev), s->h_ms, 0));
        memset(s->h_ms, 0, sizeof(MappedStates));
    }
    STAGE_TRY(hipMalloc(&s->sum_scratch, kSummaryScratch));
    if (o.eps_pub) {   // (before any binned_build: bin_desc reads it)
        STAGE_TRY(hipMalloc(&s->eacc, 2 * kEaccWords * sizeof(unsigned long long)));
        STAGE_TRY(hipMemsetAsync(s->eacc, 0, 2 * kEaccWords * sizeof(unsigned long long), s->stream));
    }
    STAGE_TRY(hipMemsetAsync(s->sum_scratch, 0, kSummaryScratch, s->stream));
    if (s->c.trace_spread) {
        const uint64_t nt = s->B * ((uint64_t)s->c.max_rounds + 1);
        STAGE_TRY(hipMalloc(&s->trace, nt * sizeof(double)));
        STAGE_TRY(hipMemsetAsync(s->trace, 0xFF, nt * sizeof(double), s->stream));   // NaN
    }
    return ACS_OK;
}

// The fault schedule (before the plans: the fix-up list of a binned plan reads it) and, once
// `binned` is decided, the crash ranks of the fp32 tags.
static int build_fault_schedule(acs_sim* s) {
    const acs_config& c = s->c;
    if (c.fault_model == ACS_FAULT_NONE) return ACS_OK;
    STAGE_TRY(hipMalloc(&s->status, s->B * s->N * sizeof(uint32_t)));
    STAGE_TRY(build_fault_status(s->status, s->B, s->N, c.n_faulty, c.fault_model, c.crash_window, s->mp.key,
                                 c.instance_offset, s->stream));
    if (!(s->binned && s->f32 && c.fault_model == ACS_FAULT_CRASH && s->N > (1ull << 20))) return ACS_OK;
    // crash ranks for the fp32 tags (RoundArgs::crank): faulty nodes grouped by crash round
    std::vector<uint32_t> st(s->N), rank(s->N, 0u), list;
    STAGE_TRY(hipMemcpy(st.data(), s->status, s->N * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint32_t W = c.crash_window;
    s->coff.assign(W + 1, 0u);
    for (uint64_t i = 0; i < s->N; ++i)
        if (st[i] < W) ++s->coff[st[i] + 1];
    for (uint32_t w = 0; w < W; ++w) s->coff[w + 1] += s->coff[w];
    list.resize(s->coff[W] ? s->coff[W] : 1);
    std::vector<uint32_t> fill(s->coff.begin(), s->coff.end() - 1);
    for (uint64_t i = 0; i < s->N; ++i)
        if (st[i] < W) {
            rank[i] = fill[st[i]] - s->coff[st[i]];
            list[fill[st[i]]++] = (uint32_t)i;
        }
    STAGE_TRY(hipMalloc(&s->crank, s->N * sizeof(uint32_t)));
    STAGE_TRY(hipMalloc(&s->clist, list.size() * sizeof(uint32_t)));
    STAGE_TRY(hipMemcpy(s->crank, rank.data(), s->N * sizeof(uint32_t), hipMemcpyHostToDevice));
    STAGE_TRY(hipMemcpy(s->clist, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return ACS_OK;
}

// ------------------------------------------------------------------------- stage 5: graph and plans
// What a binned plan of nr local rows is built for.  Narrow stage (the default where a plan
// qualifies): whole unpartitioned rounds with the deferred finalize, whose
// phase B publishes each round's (min, max) for the next phase A
static BinnedDesc bin_desc(const acs_sim* s, uint64_t nr) {
    return BinnedDesc{s->N, nr, s->d, s->dp, s->c.fault_model != ACS_FAULT_NONE, s->f32, s->csr_var, s->clean,
                      s->status, !s->partitioned && s->defer_fin && s->eacc != nullptr};
}

// Build the adjacency rows of partition p into `ell` (sorted when the config allows it).
static hipError_t build_rows(acs_sim* s, uint32_t* ell, int p) {
    const uint64_t gseed = s->c.graph_seed ? s->c.graph_seed : s->c.seed;
    const uint64_t nr = !s->partitioned ? s->N : part_rows(s, p);
    if (nr == 0) return hipSuccess;
    hipError_t e = launch_build_ell(ell, s->N, !s->partitioned ? 0 : part_row0(s, p), nr, s->d, s->dp,
                                    make_feistel(s->N, gseed), s->stream);
    if (e == hipSuccess && s->ell_sorted) e = launch_sort_ell_rows(ell, nr, s->d, s->stream);
    return e;
}

// RANDOM_REGULAR: the ELL of this rank's rows (and of every other virtual partition, each with its
// private x copies), then the binned plans, which replace the ELLs in the round loop.  A plan can
// still be refused after it is laid out (a two-level plan whose phase-M image outgrows the LDS,
// too many runs per receiver block): then every partition keeps its ELL and runs the per-lane
// kernel, which serves the same configs (binned_supported implies a compiled register variant).
static int build_regular(acs_sim* s, const CreateOptions& o) {
    const uint64_t words = ((rows_local(s) + 63) / 64) * 64ull * s->dp;
    bool refused = false;
    auto rows_and_plan = [&](uint32_t** ell, BinnedPlan& plan, int p) -> int {
        STAGE_TRY(hipMalloc(ell, words * sizeof(uint32_t)));
        STAGE_TRY(hipMemsetAsync(*ell, 0, words * sizeof(uint32_t), s->stream));
        STAGE_TRY(build_rows(s, *ell, p));
        const uint64_t nr = s->partitioned ? part_rows(s, p) : s->N;
        if (!s->binned || refused || !nr) return ACS_OK;
        const hipError_t e = binned_build(plan, *ell, bin_desc(s, nr), o.bin, s->bin_sb, s->stream);
        refused = e == hipErrorNotSupported;
        if (!refused) STAGE_TRY(e);
        return ACS_OK;
    };
    if (int rc = rows_and_plan(&s->ell, s->bin, s->partitioned ? s->rank : 0)) return rc;
    if (s->virt) {
        s->parts.resize(s->nranks - 1);
        for (int p = 1; p < s->nranks; ++p) {
            Part& q = s->parts[p - 1];
            STAGE_TRY(hipMalloc(&q.x[0], s->xstride * s->es));
            STAGE_TRY(hipMalloc(&q.x[1], s->xstride * s->es));
            if (int rc = rows_and_plan(&q.ell, q.bin, p)) return rc;
        }
    }
    if (s->binned && refused) drop_binned(s);
    if (s->binned) {
        (void)hipFree(s->ell);
        s->ell = nullptr;
        for (Part& q : s->parts) {
            (void)hipFree(q.ell);
            q.ell = nullptr;
        }
    }
    return ACS_OK;
}

// CSR: the device copies of the graph and the weights (as csr_check.hpp rounded them), and on the
// register / binned paths the padded ELL (SELL-64 slice widths), sorted rows when
// order-independent, the weights in the ELL's order and the binned plan.
static int build_csr(acs_sim* s, const CreateOptions& o, const CsrCheck& chk, const uint64_t* h_rowptr,
                     const uint32_t* h_colidx, const LinkSchedule* h_sched) {
    const uint64_t nnz = s->nnz;
    STAGE_TRY(hipMalloc(&s->rowptr, (s->N + 1) * sizeof(uint64_t)));
    STAGE_TRY(hipMalloc(&s->colidx, (nnz ? nnz : 1) * sizeof(uint32_t)));
    STAGE_TRY(hipMemcpy(s->rowptr, h_rowptr, (s->N + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (nnz) STAGE_TRY(hipMemcpy(s->colidx, h_colidx, nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (s->weighted && !s->split) {
        STAGE_TRY(hipMalloc(&s->wself, s->N * s->es));
        STAGE_TRY(hipMalloc(&s->wedge, (nnz ? nnz : 1) * s->es));
        if (s->f32) {   // (exact: the values were rounded to binary32 by the check)
            std::vector<float> fs(chk.wsv.begin(), chk.wsv.end()), fe(chk.wev.begin(), chk.wev.end());
            STAGE_TRY(hipMemcpy(s->wself, fs.data(), s->N * sizeof(float), hipMemcpyHostToDevice));
            if (nnz) STAGE_TRY(hipMemcpy(s->wedge, fe.data(), nnz * sizeof(float), hipMemcpyHostToDevice));
        } else {
            STAGE_TRY(hipMemcpy(s->wself, chk.wsv.data(), s->N * sizeof(double), hipMemcpyHostToDevice));
            if (nnz) STAGE_TRY(hipMemcpy(s->wedge, chk.wev.data(), nnz * sizeof(double), hipMemcpyHostToDevice));
        }
    }
    if (s->sched) {   // the masks in slot order (k_round_generic, acs_get_link_schedule)
        STAGE_TRY(hipMalloc(&s->avail, (nnz ? nnz : 1) * sizeof(uint32_t)));
        if (nnz) STAGE_TRY(hipMemcpy(s->avail, h_sched->avail, nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (s->split) {   // the share table [period][N], in the config dtype (exact: the values were rounded to it)
        std::vector<double> sh;
        split_shares(sh, s->f32, s->N, nnz, h_colidx, s->period, h_sched->avail);
        STAGE_TRY(hipMalloc(&s->share, sh.size() * s->es));
        if (s->f32) {
            std::vector<float> fs(sh.begin(), sh.end());
            STAGE_TRY(hipMemcpy(s->share, fs.data(), fs.size() * sizeof(float), hipMemcpyHostToDevice));
        } else {
            STAGE_TRY(hipMemcpy(s->share, sh.data(), sh.size() * sizeof(double), hipMemcpyHostToDevice));
        }
    }
    if (!s->csr_var) return ACS_OK;
    const uint64_t words = ((s->N + 63) / 64) * 64ull * s->dp;
    STAGE_TRY(hipMalloc(&s->ell, words * sizeof(uint32_t)));
    STAGE_TRY(hipMalloc(&s->deg, s->N));
    STAGE_TRY(hipMalloc(&s->sw, (s->N + 63) / 64));
    STAGE_TRY(hipMemsetAsync(s->ell, 0xFF, words * sizeof(uint32_t), s->stream));
    STAGE_TRY(launch_csr_to_ell(s->rowptr, s->colidx, s->N, s->d, s->ell, s->deg, s->sw, s->stream));
    if (s->ell_sorted) STAGE_TRY(launch_sort_ell_rows(s->ell, s->N, s->d, s->stream));
    if (s->weighted && !s->split) {
        STAGE_TRY(hipMalloc(&s->well, words * s->es));
        STAGE_TRY(launch_weights_to_ell(s->rowptr, s->wedge, s->deg, s->N, s->d, s->f32, s->well, s->stream));
    }
    if (s->sched) {   // ... and in the weights' order
        STAGE_TRY(hipMalloc(&s->avell, words * sizeof(uint32_t)));
        STAGE_TRY(launch_avail_to_ell(s->rowptr, s->avail, s->deg, s->N, s->d, s->avell, s->stream));
    }
    if (!s->binned) return ACS_OK;
    const hipError_t be = binned_build(s->bin, s->ell, bin_desc(s, s->N), o.bin, kBinSB, s->stream);
    if (be == hipErrorNotSupported) {   // the plan does not fit: the per-lane kernel serves the rows
        drop_binned(s);
        return ACS_OK;
    }
    STAGE_TRY(be);
    (void)hipFree(s->ell);
    s->ell = nullptr;
    return ACS_OK;
}

// ------------------------------------------------------------------------- stage 6: generic receiver lists
// CSR rows for the generic kernels: the hub rows beside a fast path, or every row on the
// generic path.  Rows up to kGenericMaxM entries by size class, the rest on the big-m path.
static int build_csr_generic_lists(acs_sim* s, const uint64_t* h_rowptr) {
    constexpr uint32_t kCls[] = {64, 256, 1024, 4096, kGenericMaxM};
    std::vector<uint32_t> lists[5], big;
    std::vector<uint64_t> mv;
    for (uint64_t i = 0; i < s->N; ++i) {
        const uint64_t mi = h_rowptr[i + 1] - h_rowptr[i] + 1;
        if (s->n_hub && mi - 1 <= s->d) continue;   // a fast-path row
        if (mi > kGenericMaxM) {
            big.push_back((uint32_t)i);
            mv.push_back(mi);
            continue;
        }
        int k = 0;
        while (mi > kCls[k]) ++k;
        lists[k].push_back((uint32_t)i);
    }
    std::vector<uint32_t> all;
    for (int k = 0; k < 5; ++k) {
        if (lists[k].empty()) continue;
        s->gcls.push_back({all.size(), lists[k].size(), kCls[k]});
        all.insert(all.end(), lists[k].begin(), lists[k].end());
    }
    s->gen_base = s->n_hub ? s->nblk_fast : 0;
    if (!all.empty()) {
        STAGE_TRY(hipMalloc(&s->gen_ids, all.size() * sizeof(uint32_t)));
        STAGE_TRY(hipMemcpy(s->gen_ids, all.data(), all.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    STAGE_TRY(generic_big_build(s->big, big, mv, s->f32, s->stream));
    s->big.pbase = s->gen_base + all.size();
    return ACS_OK;
}

static int build_generic_lists(acs_sim* s, const uint64_t* h_rowptr) {
    if (s->n_hub || (s->path == PATH_GENERIC && s->c.topology == ACS_TOPO_CSR)) return build_csr_generic_lists(s, h_rowptr);
    if (!(s->path == PATH_GENERIC && s->m > kGenericMaxM)) return ACS_OK;
    // complete / regular graphs above kGenericMaxM entries: every receiver on the big-m path
    std::vector<uint32_t> ids(s->N);
    for (uint64_t i = 0; i < s->N; ++i) ids[i] = (uint32_t)i;
    STAGE_TRY(generic_big_build(s->big, ids, std::vector<uint64_t>(s->N, s->m), s->f32, s->stream));
    return ACS_OK;
}

// ------------------------------------------------------------------------- the kernel name
// kernel_name() of a finished handle: the one place the name is written.  The strings are pinned
// by tests/golden/kernel_names.json and by the tests' own assertions.
static std::string kernel_name_of(const acs_sim* s) {
    const acs_config& c = s->c;
    const bool faults = c.fault_model != ACS_FAULT_NONE;
    const bool regular_plan = s->binned && !s->csr_var;   // (CSR plans' names say neither passes, packing nor fix-up)
    std::string nm;
    if (s->path == PATH_BATCHED) {
        const uint32_t F = batched_split_factor((uint32_t)s->N, c.rule, faults);
        nm = s->mfma ? "k_batched_mfma<v_mfma_f64_16x16x4>"
             : F > 1 ? "k_batched_split<" + std::to_string(F) + ">"
                     : batched_small_name((uint32_t)s->N, c.rule, faults);
    } else if (s->path == PATH_DENSE) {
        nm = s->dense_persist ? "k_dense_persist" : "k_dense_sort+k_dense_recv";
    } else if (s->path == PATH_GENERIC) {
        nm = s->m <= kGenericMaxM ? "k_round_generic"
             : s->generic_small   ? "k_round_generic+k_big_resolve+sort+k_big_rule"
                                  : "k_big_resolve+sort+k_big_rule";
    } else if (s->binned) {
        // (levels and receiver block as decided for rows_per rows: a ragged or empty last rank's own
        // plan need not share them)
        const bool two = binned_levels(s->N, rows_local(s), s->d, s->bin_sa, s->bin_sb, nullptr) == 2;
        nm = std::string("k_bin_scatter+") + (two ? "k_bin_regroup+" : "");
        if (s->weighted)   // named after what runs: the lossy instantiation is no ",faulty" kernel
            nm += "k_bin_gather_w<" + std::to_string(s->d) + ",csr>";
        else
            nm += "k_bin_gather<" + std::to_string(s->d) + "," + std::to_string(c.trim) + (s->clean ? "" : ",faulty") +
                  (s->csr_var ? ",csr" : "") + ">";
        // fault fix-up list instead of tagged senders
        if (faults) nm += regular_plan && s->bin.fix ? "+k_bin_fixup" : "+k_bin_tag";
        if (s->bin_sb != kBinSB) nm += " sb" + std::to_string(s->bin_sb);
    } else if (s->csr_var) {
        // (SCHED instantiations; k_round_weighted's QUANT ones)
        const std::string w = "<" + std::to_string(s->d) + (s->sched ? ",csr,sched" : ",csr") + (s->quant ? ",quant>" : ">");
        // (k_round_pushsum_hold, k_round_pushsum_transit: the reported names of k_round_pushsum's kLinkHold and
        // kLinkTransit instantiations)
        nm = s->split    ? "k_round_pushsum_split<" + std::to_string(s->d) + ",csr>"
           : s->hold     ? "k_round_pushsum_hold" + w
           : s->transit  ? "k_round_pushsum_transit" + w
           : s->pushsum  ? "k_round_pushsum" + w
           : s->weighted ? "k_round_weighted" + w
                         : "k_round_regular<" + std::to_string(s->d) + "," + std::to_string(c.trim) + ",csr>";
    } else {
        nm = regular_fast_name(s->d, c.trim, s->clean);
    }
    if (s->n_hub) nm += "+k_round_generic(hubs)";
    if (s->f32) nm += " [f32]";
    if (regular_plan) {
        // NP-pass phase B (slot-dependent configs: fp64, two passes only; see launch_round_binned)
        if (s->bin.split > 1 && (s->clean || (!s->f32 && s->bin.split == 2))) nm += " split" + std::to_string(s->bin.split);
        if (s->bin.pkA) nm += " pk14A";     // 14-bit packed phase-A index stream
        if (s->bin.narrow) nm += " narrow";   // narrow stage
    }
    if (s->xchunks) nm += " xchunks" + std::to_string(s->xchunks);
    return nm;
}

// ------------------------------------------------------------------------- stage 7: values, exchange, communicator
static int finish_handle(acs_sim* s, const CreateOptions& o, const void* comm_id) {
    const acs_config& c = s->c;
    STAGE_TRY(launch_init_values(s->x[0], s->B, s->N, s->mp.key, c.instance_offset, s->f32, s->stream));
    if (s->pushsum) {   // round 0: s = x^0, z = 1 (Npad == N: CSR handles are not partitioned)
        STAGE_TRY(hipMalloc(&s->pairs, 2 * s->B * s->N * 2 * s->es));
        STAGE_TRY(launch_pushsum_fill(s->x[0], pairs_at(s, 0), s->B * s->N, s->f32, s->stream));
    }
    if (s->split) {   // round 0's offers: phase 0's shares of (x^0, 1)
        STAGE_TRY(hipMalloc(&s->offers, 2 * s->B * s->N * 2 * s->es));
        STAGE_TRY(launch_pushsum_offer(pairs_at(s, 0), share_at(s, 0), offers_at(s, 0), s->B, s->N, s->f32, s->stream));
    }
    if (s->quant) {   // what the nodes transmit in round 0: Q(x^0; b, 0, i)
        STAGE_TRY(hipMalloc(&s->qbuf, 2 * s->B * s->N * s->es));
        STAGE_TRY(launch_quantize(s->x[0], quant_at(s, 0), s->B, s->N, 0, s->mp, s->qk, s->qdither, s->f32, s->stream));
    }
    if (s->hold) {   // every link starts empty: (+0.0, +0.0)
        STAGE_TRY(hipMalloc(&s->links, links_bytes(s)));
        STAGE_TRY(hipMemsetAsync(s->links, 0, links_bytes(s), s->stream));
    }
    if (s->transit) {   // nothing is in transit at round 0
        STAGE_TRY(hipMalloc(&s->ring, ring_bytes(s)));
        STAGE_TRY(hipMemsetAsync(s->ring, 0, ring_bytes(s), s->stream));
    }
    for (Part& q : s->parts)
        STAGE_TRY(launch_init_values(q.x[0], s->B, s->N, s->mp.key, c.instance_offset, s->f32, s->stream));
    // chunked exchange: clean binned partitions whose row blocks split into
    // ACSIM_XCHUNKS chunks of whole source blocks AND of whole phase-B receiver blocks (chunk k's
    // exchange is recorded after phase B's blocks [k*qpc, (k+1)*qpc), which must cover exactly the
    // chunk's rows); 0 or 1 keeps the unchunked sequence.  Default: 4 for virtual partitions (GPU-
    // tested bit-exact), and the per-round all-gather for a real multi-rank communicator until a
    // multi-GPU run has matched the golden hash (the grouped send / receive path is opt-in there).
    if (s->partitioned && s->binned && s->clean) {
        const uint32_t K = o.xchunks_set ? o.xchunks : (comm_id && s->nranks > 1) ? 0u : 4u;
        if (K >= 2 && K <= acs_sim::kMaxX && s->rows_per % ((uint64_t)K * s->bin_sa) == 0 &&
            (s->rows_per / K) % s->bin.SB == 0)
            s->xchunks = K;
    }
    if (s->xchunks) {
        hipError_t e = hipStreamCreateWithFlags(&s->cstream, hipStreamNonBlocking);
        for (uint32_t k = 0; e == hipSuccess && k < s->xchunks; ++k) {
            e = hipEventCreateWithFlags(&s->ev_b[k], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_x[k], hipEventDisableTiming);
        }
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_fin, hipEventDisableTiming);
        if (e != hipSuccess) return fail(ACS_EDEVICE, "comm stream / events: %s", hipGetErrorString(e));
    }
    s->kname = kernel_name_of(s);
    if (comm_id) {
        ncclUniqueId id;
        memcpy(&id, comm_id, sizeof id);
        ncclResult_t nr = ncclCommInitRank(&s->comm, s->nranks, id, s->rank);
        if (nr != ncclSuccess)
            return fail(ACS_ECOMM, "ncclCommInitRank(%d ranks, rank %d) failed: %s", s->nranks, s->rank,
                        ncclGetErrorString(nr));
    }
    return init_state(s, 0);
}

// ------------------------------------------------------------------------- create
// Checks that need no handle: the CSR arrays and weights, the partition arguments, the device.
static int check_arguments(const acs_config* cfg, int device, int nranks, int rank, const void* comm_id,
                           uint64_t id_len, const uint64_t* h_rowptr, const uint32_t* h_colidx, const double* h_wself,
                           const double* h_wedge, const LinkSchedule* h_sched, CsrCheck& chk) {
    if (cfg->topology == ACS_TOPO_CSR) {   // §8(f) row 1: check the arrays on the host
        if (!h_rowptr || !h_colidx) return fail(ACS_EINVAL, "CSR topology needs acs_create_csr(rowptr, colidx)");
        if (nranks != 1) return fail(ACS_EUNSUPPORTED, "node partitioning needs RANDOM_REGULAR");
        if (csr_check_arrays(chk, *cfg, h_rowptr, h_colidx)) return fail(chk.code, "%s", chk.message.c_str());
    }
    const bool split = h_sched && h_sched->split;
    if (split) {   // (no weights: the shares follow from the schedule; the generic kernel's row limit stays)
        if (chk.mmax > kGenericMaxM)
            return fail(ACS_EUNSUPPORTED, "rule PUSHSUM serves rows of at most %u entries (largest row: %llu)", kGenericMaxM,
                        (unsigned long long)chk.mmax);
    } else if (cfg->rule == ACS_RULE_WEIGHTED || cfg->rule == ACS_RULE_PUSHSUM) {
        if (!h_wself || !h_wedge) return fail(ACS_EINVAL, "rule WEIGHTED needs acs_create_csr_weighted(w_self, w_edge)");
        if (csr_check_weights(chk, *cfg, h_rowptr, h_colidx, h_wself, h_wedge))
            return fail(chk.code, "%s", chk.message.c_str());
    }
    if (h_sched && sched_check(chk, *cfg, chk.nnz, h_sched->period, h_sched->avail, split))
        return fail(chk.code, "%s", chk.message.c_str());
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(ACS_EINVAL, "bad rank / n_ranks");
    const bool partitioned = nranks > 1 || comm_id != nullptr;
    if (partitioned && !comm_id && rank != 0) return fail(ACS_EINVAL, "virtual partitions live on one handle (rank 0)");
    if (comm_id && id_len != sizeof(ncclUniqueId))
        return fail(ACS_EINVAL, "comm id must be %zu bytes", sizeof(ncclUniqueId));
    if (partitioned && cfg->delay_max)
        return fail(ACS_EUNSUPPORTED, "node partitioning runs synchronous rounds only (delay_max = 0)");
    if (partitioned) {
        if (cfg->topology != ACS_TOPO_RANDOM_REGULAR || cfg->n_instances != 1 ||
            !regular_fast_supported(cfg->degree, cfg->trim, cfg->rule))
            return fail(ACS_EUNSUPPORTED, "node partitioning needs one RANDOM_REGULAR instance with a "
                                          "compiled (degree, trim) variant");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(ACS_EDEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return fail(ACS_EINVAL, "device %d out of range", device);
    return ACS_OK;
}

// The handle's fields that follow from the config, the partition arguments and the path alone.
static acs_sim* new_handle(const acs_config& c, int device, int nranks, int rank, bool partitioned, bool virt,
                           const PathChoice& pc, const CsrCheck& chk, const LinkSchedule* h_sched, int transit_max,
                           const QuantSpec* h_quant) {
    acs_sim* s = new acs_sim();
    s->c = c;
    s->device = device;
    s->N = c.n_nodes;
    s->B = c.n_instances;
    s->m = pc.m;
    s->path = pc.path;
    s->d = pc.d;
    s->dp = pc.dp;
    s->csr_var = pc.csr_var;
    s->n_hub = pc.n_hub;
    s->mfma = pc.mfma;
    s->dense_persist = pc.dense_persist;
    s->generic_small = pc.generic_small;
    s->pushsum = c.rule == ACS_RULE_PUSHSUM;   // (weights as for WEIGHTED, one more rule)
    s->weighted = c.rule == ACS_RULE_WEIGHTED || s->pushsum;
    s->hold = s->pushsum && c.missing_policy == ACS_MISSING_HOLD;   // (validate: HOLD only with PUSHSUM)
    s->transit = transit_max >= 0;   // (acs_create_csr_transit: rule PUSHSUM, never HOLD)
    s->tmax = s->transit ? (uint32_t)transit_max : 0u;
    s->nnz = chk.nnz;
    s->sched = h_sched != nullptr;
    s->period = h_sched ? h_sched->period : 0;
    s->split = h_sched && h_sched->split;
    s->quant = h_quant != nullptr;   // (acs_create_csr_quantized: rule WEIGHTED, no faults, no delays)
    if (h_quant) s->qk = h_quant->k, s->qmode = h_quant->mode, s->qdither = h_quant->dither;
    // "clean": no slot-dependent decision at all (no faults, no loss, no delays, no link schedule)
    s->clean = c.fault_model == ACS_FAULT_NONE && drop_threshold(c.loss_p) == 0 && c.delay_max == 0 && !s->sched;
    s->mp.key = key_of(c.seed);
    s->mp.thr = drop_threshold(c.loss_p);
    s->mp.fault = c.fault_model;
    s->mp.byz = c.byz_strategy;
    s->mp.mask_group = c.mask_group;
    s->mp.inst_offset = c.instance_offset;
    s->mp.delta = c.byz_delta;
    s->mp.bconst = c.byz_const + 0.0;   // canonicalise -0.0 (no -0 ever enters a sort)
    s->mp.omit = c.missing_policy == ACS_MISSING_OMIT ? 1u : 0u;
    s->nranks = nranks;
    s->rank = rank;
    s->partitioned = partitioned;
    s->virt = virt;
    s->rows_per = partitioned ? ((s->N + nranks - 1) / nranks + 63) / 64 * 64 : s->N;
    s->Npad = partitioned ? s->rows_per * nranks : s->N;
    s->f32 = c.dtype == ACS_F32;
    s->es = s->f32 ? 4u : 8u;
    s->ell_sorted = s->path == PATH_REGULAR && s->clean && c.rule != ACS_RULE_AVERAGE &&
                    !s->weighted;   // (WEIGHTED is entry-ordered like AVERAGE, and its weights go by slot)
    return s;
}

int create_impl(const acs_config* cfg, int device, int nranks, int rank, const void* comm_id, uint64_t id_len,
                acs_sim** out, const uint64_t* h_rowptr, const uint32_t* h_colidx, const double* h_wself,
                const double* h_wedge, const LinkSchedule* h_sched, int transit_max, const QuantSpec* h_quant) {
    *out = nullptr;
    // 1. host checks and 2. path choice, before any handle exists
    CsrCheck chk;
    if (int rc = check_arguments(cfg, device, nranks, rank, comm_id, id_len, h_rowptr, h_colidx, h_wself, h_wedge, h_sched, chk))
        return rc;
    const CreateOptions opt = options_from_env(cfg->dtype == ACS_F32);
    const bool partitioned = nranks > 1 || comm_id != nullptr;
    PathChoice pc;
    if (int rc = choose_path(*cfg, opt, partitioned, chk.mmax, h_rowptr, pc)) return rc;

    RoctxRange range("acs: create (graph, plan, fault schedule, x0)");
    acs_sim* s = new_handle(*cfg, device, nranks, rank, partitioned, partitioned && !comm_id, pc, chk, h_sched, transit_max,
                            h_quant);
    // 3. - 7.: the order matters in three places.  eacc (alloc_state) exists before any
    // binned_build, whose bin_desc reads it; the fault status is built before the plans, whose fix-up
    // list reads it; and `binned` is decided (decide_binned) before the fp32 crash-rank table.
    const uint64_t ncap = decide_binned(s, opt);
    int rc = alloc_state(s, opt, ncap);
    if (!rc) rc = build_fault_schedule(s);
    if (!rc && cfg->topology == ACS_TOPO_RANDOM_REGULAR) rc = build_regular(s, opt);
    if (!rc && cfg->topology == ACS_TOPO_CSR) rc = build_csr(s, opt, chk, h_rowptr, h_colidx, h_sched);
    if (!rc) rc = build_generic_lists(s, h_rowptr);
    if (!rc) rc = finish_handle(s, opt, comm_id);
    if (rc) {
        release(s);
        return rc;
    }
    *out = s;
    return ACS_OK;
}
