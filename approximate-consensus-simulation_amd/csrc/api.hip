// api.hip — the C ABI (include/acsim.h) over the handle: every extern "C" entry point, argument
// checks, and the thread's last error text.  Handles are made in create.hip and stepped in rounds.hip.
#include <stdarg.h>

#include <chrono>

#include "handle.hpp"
#include "quantize.hpp"

using namespace acs;

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// A handle for a config not validated yet (every entry point but acs_create, which has checks of
// its own between the two steps).
static int validate_and_create(const acs_config* cfg, int device, int nranks, int rank, const void* comm_id,
                               uint64_t id_len, acs_sim** out, const uint64_t* rowptr = nullptr,
                               const uint32_t* colidx = nullptr, const double* w_self = nullptr,
                               const double* w_edge = nullptr, const LinkSchedule* sched = nullptr) {
    if (!out) return fail(ACS_EINVAL, "null out");
    *out = nullptr;
    if (int rc = validate(cfg)) return rc;
    return create_impl(cfg, device, nranks, rank, comm_id, id_len, out, rowptr, colidx, w_self, w_edge, sched);
}

// ------------------------------------------------------------------------- C ABI
extern "C" {

int acs_abi_version(void) { return ACS_ABI_VERSION; }

const char* acs_last_error(void) { return g_err.c_str(); }

int acs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return fail(ACS_EDEVICE, "hipGetDeviceCount failed");
    return n;
}

int acs_runtime_info(char* out, uint64_t cap) {
    if (!out || cap == 0) return fail(ACS_EINVAL, "acs_runtime_info: empty buffer");
    int hv = 0, nv = 0;
    if (hipRuntimeGetVersion(&hv) != hipSuccess) return fail(ACS_EDEVICE, "hipRuntimeGetVersion failed");
    if (ncclGetVersion(&nv) != ncclSuccess) return fail(ACS_ECOMM, "ncclGetVersion failed");
    snprintf(out, cap, "hip %d rccl %d polled-host-flags 0x%x", hv, nv, kPolledHostFlags);
    return ACS_OK;
}

int acs_create(const acs_config* cfg, int backend, const int* devices, int n_devices, acs_sim** out) {
    if (out) *out = nullptr;
    int rc = validate(cfg);
    if (rc) return rc;
    if (backend != ACS_HIP)
        return fail(ACS_EUNSUPPORTED, "libacsim implements ACS_HIP only (the CPU spec reference is the "
                                      "test oracle in oracle/, not a product backend)");
    if (n_devices != 1 || !devices)
        return fail(ACS_EINVAL, "exactly one device per handle (shard across processes, one rank per GPU)");
    if (cfg->topology == ACS_TOPO_CSR) return fail(ACS_EINVAL, "CSR topology: use acs_create_csr");
    if (!out) return fail(ACS_EINVAL, "null out");
    return create_impl(cfg, devices[0], 1, 0, nullptr, 0, out);
}

int acs_create_csr(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx, int device,
                   acs_sim** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->topology != ACS_TOPO_CSR) return fail(ACS_EINVAL, "config topology must be ACS_TOPO_CSR");
    if (!rowptr || !colidx) return fail(ACS_EINVAL, "null CSR arrays");
    if (cfg->rule == ACS_RULE_WEIGHTED || cfg->rule == ACS_RULE_PUSHSUM)
        return fail(ACS_EINVAL, "rules WEIGHTED and PUSHSUM need weights: use acs_create_csr_weighted");
    return validate_and_create(cfg, device, 1, 0, nullptr, 0, out, rowptr, colidx);
}

int acs_create_csr_weighted(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx,
                            const double* w_self, const double* w_edge, int device, acs_sim** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->topology != ACS_TOPO_CSR) return fail(ACS_EINVAL, "config topology must be ACS_TOPO_CSR");
    if (cfg->rule != ACS_RULE_WEIGHTED && cfg->rule != ACS_RULE_PUSHSUM)
        return fail(ACS_EINVAL, "acs_create_csr_weighted takes rules ACS_RULE_WEIGHTED and ACS_RULE_PUSHSUM only (got rule %u)",
                    cfg->rule);
    if (!rowptr || !colidx) return fail(ACS_EINVAL, "null CSR arrays");
    if (!w_self || !w_edge) return fail(ACS_EINVAL, "null weight arrays");
    return validate_and_create(cfg, device, 1, 0, nullptr, 0, out, rowptr, colidx, w_self, w_edge);
}

int acs_create_csr_scheduled(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx, const double* w_self,
                             const double* w_edge, uint32_t period, const uint32_t* avail, int device, acs_sim** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->topology != ACS_TOPO_CSR) return fail(ACS_EINVAL, "config topology must be ACS_TOPO_CSR");
    if (cfg->rule != ACS_RULE_WEIGHTED && cfg->rule != ACS_RULE_PUSHSUM)
        return fail(ACS_EUNSUPPORTED, "link schedules are served for rules WEIGHTED and PUSHSUM (got rule %u)", cfg->rule);
    if (!rowptr || !colidx) return fail(ACS_EINVAL, "null CSR arrays");
    if (!w_self || !w_edge) return fail(ACS_EINVAL, "null weight arrays");
    const LinkSchedule sched{period, avail};   // (checked with the arrays: sched_check.hpp)
    return validate_and_create(cfg, device, 1, 0, nullptr, 0, out, rowptr, colidx, w_self, w_edge, &sched);
}

int acs_create_csr_split(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx, uint32_t period,
                         const uint32_t* avail, int device, acs_sim** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->topology != ACS_TOPO_CSR) return fail(ACS_EINVAL, "config topology must be ACS_TOPO_CSR");
    if (cfg->rule != ACS_RULE_PUSHSUM)
        return fail(ACS_EINVAL, "acs_create_csr_split takes rule ACS_RULE_PUSHSUM only (got rule %u)", cfg->rule);
    if (!rowptr || !colidx) return fail(ACS_EINVAL, "null CSR arrays");
    if (!out) return fail(ACS_EINVAL, "null out");
    if (int rc = validate(cfg)) return rc;   // (before the HOLD check: an invalid config is ACS_EINVAL first)
    if (cfg->missing_policy == ACS_MISSING_HOLD)
        return fail(ACS_EUNSUPPORTED, "push-sum with per-round splitting does not serve missing_policy = HOLD: a lost "
                                      "message's mass is lost, as under OMIT");
    LinkSchedule sched{period, avail};   // (checked with the arrays: sched_check.hpp)
    sched.split = true;
    return create_impl(cfg, device, 1, 0, nullptr, 0, out, rowptr, colidx, nullptr, nullptr, &sched);
}

int acs_create_csr_transit(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx, const double* w_self,
                           const double* w_edge, uint32_t period, const uint32_t* avail, uint32_t transit_max, int device,
                           acs_sim** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->topology != ACS_TOPO_CSR) return fail(ACS_EINVAL, "config topology must be ACS_TOPO_CSR");
    if (cfg->rule != ACS_RULE_PUSHSUM)
        return fail(ACS_EUNSUPPORTED, "messages in transit are served for rule PUSHSUM (got rule %u): rule WEIGHTED "
                                      "delays values with delay_max", cfg->rule);
    if (!rowptr || !colidx) return fail(ACS_EINVAL, "null CSR arrays");
    if (!w_self || !w_edge) return fail(ACS_EINVAL, "null weight arrays");
    if (!out) return fail(ACS_EINVAL, "null out");
    if (transit_max > kTransitMax) return fail(ACS_EINVAL, "transit_max must be <= %u (got %u)", kTransitMax, transit_max);
    if (period == 0 && avail) return fail(ACS_EINVAL, "a link schedule needs period >= 1 (no schedule: 0, NULL)");
    if (int rc = validate(cfg)) return rc;   // (delay_max > 0 is refused there: the two delay models do not mix)
    if (cfg->missing_policy == ACS_MISSING_HOLD)
        return fail(ACS_EUNSUPPORTED, "push-sum with messages in transit does not serve missing_policy = HOLD yet: a gone "
                                      "message's mass is lost, as under OMIT");
    if (cfg->dtype == ACS_F32 && cfg->max_rounds > transit_f32_max_rounds(transit_max))
        return fail(ACS_EINVAL, "PUSHSUM in fp32 with transit_max = %u needs max_rounds <= 2^26 / (16 + transit_max) = %u "
                                "(binary32 sums stay finite, DESIGN.md §9)", transit_max, transit_f32_max_rounds(transit_max));
    const LinkSchedule sched{period, avail};   // (checked with the arrays: sched_check.hpp)
    return create_impl(cfg, device, 1, 0, nullptr, 0, out, rowptr, colidx, w_self, w_edge, period ? &sched : nullptr,
                       (int)transit_max);
}

int acs_create_csr_quantized(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx, const double* w_self,
                             const double* w_edge, uint32_t period, const uint32_t* avail, uint32_t step_log2, uint32_t mode,
                             uint32_t dither, int device, acs_sim** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->topology != ACS_TOPO_CSR) return fail(ACS_EINVAL, "config topology must be ACS_TOPO_CSR");
    if (cfg->rule != ACS_RULE_WEIGHTED)
        return fail(ACS_EUNSUPPORTED, "quantized messages are served for rule WEIGHTED (got rule %u): quantizing "
                                      "push-sum's pairs loses mass", cfg->rule);
    if (!rowptr || !colidx) return fail(ACS_EINVAL, "null CSR arrays");
    if (!w_self || !w_edge) return fail(ACS_EINVAL, "null weight arrays");
    if (!out) return fail(ACS_EINVAL, "null out");
    if (period == 0 && avail) return fail(ACS_EINVAL, "a link schedule needs period >= 1 (no schedule: 0, NULL)");
    if (int rc = validate(cfg)) return rc;   // (before the refusals: an invalid config is ACS_EINVAL first)
    const uint32_t kmax = cfg->dtype == ACS_F32 ? kQuantMaxLog2F32 : kQuantMaxLog2F64;
    if (step_log2 > kmax)
        return fail(ACS_EINVAL, "quantized messages: step_log2 must be <= %u%s (got %u): the step 2^-step_log2 keeps "
                                "every operation exact", kmax, cfg->dtype == ACS_F32 ? " in fp32" : "", step_log2);
    if (mode > ACS_QUANT_COMPENSATED)
        return fail(ACS_EINVAL, "quantized messages: mode must be ACS_QUANT_PARTIAL, _TOTAL or _COMPENSATED (got %u)", mode);
    if (dither > 1) return fail(ACS_EINVAL, "quantized messages: dither must be 0 or 1 (got %u)", dither);
    if (cfg->fault_model != ACS_FAULT_NONE)
        return fail(ACS_EUNSUPPORTED, "quantized messages are not served with a fault model (fault_model = %u)",
                    cfg->fault_model);
    if (cfg->delay_max > 0)
        return fail(ACS_EUNSUPPORTED, "quantized messages are not served with delay_max > 0 (got %u): a delayed read "
                                      "would need every past round's quantized values", cfg->delay_max);
    const LinkSchedule sched{period, avail};   // (checked with the arrays: sched_check.hpp)
    const QuantSpec quant{step_log2, mode, dither};
    return create_impl(cfg, device, 1, 0, nullptr, 0, out, rowptr, colidx, w_self, w_edge, period ? &sched : nullptr, -1,
                       &quant);
}

int acs_get_quantized(acs_sim* s, uint64_t b, void* out, uint64_t n) {
    if (!s || !out) return fail(ACS_EINVAL, "null argument");
    if (!s->quant) return fail(ACS_EINVAL, "acs_get_quantized: not a handle of acs_create_csr_quantized");
    if (b >= s->B || n < s->N) return fail(ACS_EINVAL, "bad get_quantized arguments (instance < B, n >= N)");
    HIP_TRY(hipSetDevice(s->device));
    InstState e;
    HIP_TRY(hipMemcpyAsync(&e, s->st + b, sizeof e, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpyAsync(out, static_cast<char*>(quant_at(s, e.rounds)) + b * s->N * s->es, s->N * s->es,
                           hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ACS_OK;
}

// The instance's relative plane d = 0 .. tmax - 1 (what round R + d delivers, R its executed rounds)
// is ring plane (R + d) mod (tmax + 1): two runs of whole planes, [c, first) and [0, tmax - first)
// with c = R mod (tmax + 1).  The plane left out, (R + tmax) mod (tmax + 1), is the one round R - 1
// delivered and emptied.
struct TransitRuns {
    uint32_t c, first;   // ring plane of relative plane 0; relative planes in the first run
};
static TransitRuns transit_runs(const acs_sim* s, uint32_t rounds) {
    const uint32_t np = s->tmax + 1, c = rounds % np;
    return TransitRuns{c, np - c < s->tmax ? np - c : s->tmax};
}

int acs_get_pushsum_transit(acs_sim* s, uint64_t b, void* h_out, void* k_out, uint64_t n) {
    if (!s) return fail(ACS_EINVAL, "null handle");
    if (!s->transit) return fail(ACS_EINVAL, "acs_get_pushsum_transit: not a handle of acs_create_csr_transit");
    const uint64_t need = (uint64_t)s->tmax * s->nnz;
    if (b >= s->B || n < need || ((!h_out || !k_out) && need) || (s->tmax == 0 && n != 0))
        return fail(ACS_EINVAL, "bad get_pushsum_transit arguments (instance < B, n >= transit_max * nnz = %llu; "
                                "n = 0 on a transit_max = 0 handle)", (unsigned long long)need);
    if (!need) return ACS_OK;
    HIP_TRY(hipSetDevice(s->device));
    InstState e;
    HIP_TRY(hipMemcpyAsync(&e, s->st + b, sizeof e, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const TransitRuns t = transit_runs(s, e.rounds);
    const uint64_t pb = plane_bytes(s);
    const char* ring = static_cast<const char*>(s->ring) + b * (s->tmax + 1) * pb;
    std::vector<unsigned char> h(need * 2 * s->es);
    HIP_TRY(hipMemcpyAsync(h.data(), ring + t.c * pb, t.first * pb, hipMemcpyDeviceToHost, s->stream));
    if (t.first < s->tmax)
        HIP_TRY(hipMemcpyAsync(h.data() + t.first * pb, ring, (s->tmax - t.first) * pb, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->f32) {
        const float* p = reinterpret_cast<const float*>(h.data());
        for (uint64_t q = 0; q < need; ++q) {
            static_cast<float*>(h_out)[q] = p[2 * q];
            static_cast<float*>(k_out)[q] = p[2 * q + 1];
        }
    } else {
        const double* p = reinterpret_cast<const double*>(h.data());
        for (uint64_t q = 0; q < need; ++q) {
            static_cast<double*>(h_out)[q] = p[2 * q];
            static_cast<double*>(k_out)[q] = p[2 * q + 1];
        }
    }
    return ACS_OK;
}

int acs_set_pushsum_transit(acs_sim* s, const void* hv, const void* kv, uint64_t n) {
    if (!s) return fail(ACS_EINVAL, "null handle");
    if (!s->transit) return fail(ACS_EINVAL, "acs_set_pushsum_transit: not a handle of acs_create_csr_transit");
    const uint64_t per = (uint64_t)s->tmax * s->nnz;
    if (n != s->B * per)
        return fail(ACS_EINVAL, "set_pushsum_transit needs B * transit_max * nnz = %llu values in h and in k (got %llu)",
                    (unsigned long long)(s->B * per), (unsigned long long)n);
    if ((!hv || !kv) && n) return fail(ACS_EINVAL, "null argument");
    if (!n) return ACS_OK;
    // mass in transit takes the caps of s and z ("mass bound"); -0.0 is stored as +0.0
    std::vector<unsigned char> h(n * 2 * s->es);
    if (s->f32) {
        float* p = reinterpret_cast<float*>(h.data());
        for (uint64_t e = 0; e < n; ++e) {
            const float a = static_cast<const float*>(hv)[e], k = static_cast<const float*>(kv)[e];
            if (!(fabsf(a) <= kPushsumMaxAbs32))
                return fail(ACS_EINVAL, "set_pushsum_transit: h[%llu] is not finite or |h| > 1e26", (unsigned long long)e);
            if (!(k >= 0.0f && k <= kPushsumMaxAbs32))
                return fail(ACS_EINVAL, "set_pushsum_transit: k[%llu] must be finite, in [0, 1e26]", (unsigned long long)e);
            p[2 * e] = a + 0.0f;
            p[2 * e + 1] = k + 0.0f;
        }
    } else {
        double* p = reinterpret_cast<double*>(h.data());
        for (uint64_t e = 0; e < n; ++e) {
            const double a = static_cast<const double*>(hv)[e], k = static_cast<const double*>(kv)[e];
            if (!(fabs(a) <= kPushsumMaxAbs64))
                return fail(ACS_EINVAL, "set_pushsum_transit: h[%llu] is not finite or |h| > 1e290", (unsigned long long)e);
            if (!(k >= 0.0 && k <= kPushsumMaxAbs64))
                return fail(ACS_EINVAL, "set_pushsum_transit: k[%llu] must be finite, in [0, 1e290]", (unsigned long long)e);
            p[2 * e] = a + 0.0;
            p[2 * e + 1] = k + 0.0;
        }
    }
    HIP_TRY(hipSetDevice(s->device));
    std::vector<InstState> v;
    if (int rc = read_states(s, v)) return rc;
    const uint64_t pb = plane_bytes(s);
    HIP_TRY(hipMemsetAsync(s->ring, 0, ring_bytes(s), s->stream));   // (the plane no relative plane maps to stays empty)
    for (uint64_t b = 0; b < s->B; ++b) {
        const TransitRuns t = transit_runs(s, v[b].rounds);
        char* ring = static_cast<char*>(s->ring) + b * (s->tmax + 1) * pb;
        const unsigned char* src = h.data() + b * s->tmax * pb;
        HIP_TRY(hipMemcpyAsync(ring + t.c * pb, src, t.first * pb, hipMemcpyHostToDevice, s->stream));
        if (t.first < s->tmax)
            HIP_TRY(hipMemcpyAsync(ring, src + t.first * pb, (s->tmax - t.first) * pb, hipMemcpyHostToDevice, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));   // h outlives the copies
    return ACS_OK;
}

int acs_get_split_shares(acs_sim* s, double* out, uint64_t n) {
    if (!s || !out) return fail(ACS_EINVAL, "null argument");
    if (!s->split) return fail(ACS_EINVAL, "acs_get_split_shares: not a handle of acs_create_csr_split");
    if (n != (uint64_t)s->period * s->N)
        return fail(ACS_EINVAL, "acs_get_split_shares: expected n = period * N = %llu", (unsigned long long)(s->period * s->N));
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->f32) {
        std::vector<float> f(n);
        HIP_TRY(hipMemcpy(f.data(), s->share, n * sizeof(float), hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < n; ++k) out[k] = f[k];
    } else {
        HIP_TRY(hipMemcpy(out, s->share, n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return ACS_OK;
}

int acs_get_link_schedule(acs_sim* s, uint32_t* period_out, uint32_t* avail_out, uint64_t nnz) {
    if (!s || !period_out || (!avail_out && nnz)) return fail(ACS_EINVAL, "null argument");
    if (!s->sched) return fail(ACS_EINVAL, "acs_get_link_schedule: not a handle of acs_create_csr_scheduled");
    if (nnz != s->nnz) return fail(ACS_EINVAL, "acs_get_link_schedule: expected nnz = %llu", (unsigned long long)s->nnz);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    *period_out = s->period;
    if (nnz) HIP_TRY(hipMemcpy(avail_out, s->avail, nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return ACS_OK;
}

int acs_get_weights(acs_sim* s, double* w_self_out, uint64_t n, double* w_edge_out, uint64_t nnz) {
    if (!s || !w_self_out || (!w_edge_out && nnz)) return fail(ACS_EINVAL, "null argument");
    if (!s->weighted) return fail(ACS_EINVAL, "acs_get_weights: not a handle of acs_create_csr_weighted");
    if (n != s->N || nnz != s->nnz)
        return fail(ACS_EINVAL, "acs_get_weights: expected n = %llu, nnz = %llu", (unsigned long long)s->N,
                    (unsigned long long)s->nnz);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->split) {   // phase 0's effective weights: the sender's share on an up slot, +0.0 on a down one
        std::vector<uint32_t> ci(nnz), av(nnz);
        if (s->f32) {
            std::vector<float> f(n);
            HIP_TRY(hipMemcpy(f.data(), s->share, n * sizeof(float), hipMemcpyDeviceToHost));
            for (uint64_t k = 0; k < n; ++k) w_self_out[k] = f[k];
        } else {
            HIP_TRY(hipMemcpy(w_self_out, s->share, n * sizeof(double), hipMemcpyDeviceToHost));
        }
        if (nnz) HIP_TRY(hipMemcpy(ci.data(), s->colidx, nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (nnz) HIP_TRY(hipMemcpy(av.data(), s->avail, nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint64_t e = 0; e < nnz; ++e) w_edge_out[e] = (av[e] & 1u) ? w_self_out[ci[e]] : 0.0;
        return ACS_OK;
    }
    if (s->f32) {
        std::vector<float> fs(n), fe(nnz);
        HIP_TRY(hipMemcpy(fs.data(), s->wself, n * sizeof(float), hipMemcpyDeviceToHost));
        if (nnz) HIP_TRY(hipMemcpy(fe.data(), s->wedge, nnz * sizeof(float), hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < n; ++k) w_self_out[k] = fs[k];
        for (uint64_t k = 0; k < nnz; ++k) w_edge_out[k] = fe[k];
    } else {
        HIP_TRY(hipMemcpy(w_self_out, s->wself, n * sizeof(double), hipMemcpyDeviceToHost));
        if (nnz) HIP_TRY(hipMemcpy(w_edge_out, s->wedge, nnz * sizeof(double), hipMemcpyDeviceToHost));
    }
    return ACS_OK;
}

int acs_comm_id_size(void) { return (int)sizeof(ncclUniqueId); }

int acs_get_comm_id(void* out, uint64_t n) {
    if (!out || n < sizeof(ncclUniqueId)) return fail(ACS_EINVAL, "buffer must hold %zu bytes", sizeof(ncclUniqueId));
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    memcpy(out, &id, sizeof id);
    return ACS_OK;
}

int acs_create_partitioned(const acs_config* cfg, int device, int n_ranks, int rank, const void* comm_id,
                           uint64_t id_len, acs_sim** out) {
    return validate_and_create(cfg, device, n_ranks, rank, comm_id, id_len, out);
}

void acs_destroy(acs_sim* s) { release(s); }

static void fill_info(acs_sim* s, const std::vector<InstState>& v, acs_round_info* out) {
    (void)s;
    if (!out) return;
    memset(out, 0, sizeof *out);
    uint64_t nd = 0;
    double sp = -INFINITY;
    uint32_t rmax = 0;
    for (const InstState& e : v) {
        nd += e.done;
        if (e.spread > sp) sp = e.spread;
        if (e.rounds > rmax) rmax = e.rounds;
    }
    out->round = rmax;
    out->done = nd == v.size();
    out->spread = sp;
    out->lo = v[0].lo;
    out->hi = v[0].hi;
    out->instances_done = nd;
}

int acs_round(acs_sim* s, uint32_t k, acs_round_info* out) {
    if (!s) return fail(ACS_EINVAL, "null sim");
    HIP_TRY(hipSetDevice(s->device));
    int rc = advance(s, k);
    if (rc) return rc;
    std::vector<InstState> v;
    rc = read_states(s, v, true);   // (EPS calls end with the states already fetched)
    if (rc) return rc;
    fill_info(s, v, out);
    return ACS_OK;
}

int acs_run(acs_sim* s, acs_result* out) {
    if (!s) return fail(ACS_EINVAL, "null sim");
    HIP_TRY(hipSetDevice(s->device));
    const auto t0 = std::chrono::steady_clock::now();
    s->want_summary = out != nullptr;
    s->summary_ready = false;
    int rc = advance(s, s->c.max_rounds);
    s->want_summary = false;
    if (rc) return rc;
    if (!s->summary_ready) HIP_TRY(hipStreamSynchronize(s->stream));
    const auto t1 = std::chrono::steady_clock::now();
    if (out) {   // the summary is folded on the device: 32 bytes back instead of B states
        if (!s->summary_ready)
            if (int rc2 = summary_and_wait(s)) return rc2;
        s->summary_ready = false;
        const RunSummary& r = *s->h_sum;
        memset(out, 0, sizeof *out);
        out->n_instances = s->B;
        out->rounds_max = r.rounds_max;
        out->n_converged = (uint32_t)r.n_converged;
        out->node_rounds = s->N * r.rounds_sum;
        double sp;
        memcpy(&sp, &r.spread_max_bits, sizeof sp);
        out->final_spread_max = s->B ? sp : -INFINITY;
        out->wall_seconds = std::chrono::duration<double>(t1 - t0).count();
    }
    return ACS_OK;
}

int acs_sync(acs_sim* s) {
    if (!s) return fail(ACS_EINVAL, "null sim");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ACS_OK;
}

int acs_get_values(acs_sim* s, uint64_t b, void* out, uint64_t n) {
    if (!s || !out || b >= s->B || n < s->N) return fail(ACS_EINVAL, "bad get_values arguments");
    HIP_TRY(hipSetDevice(s->device));
    InstState e;
    HIP_TRY(hipMemcpyAsync(&e, s->st + b, sizeof e, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpyAsync(out, xat(s, xb(s, e.rounds), b * s->Npad), s->N * s->es, hipMemcpyDeviceToHost,
                           s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ACS_OK;
}

int acs_get_all_values(acs_sim* s, void* out, uint64_t n) {
    if (!s || !out || n < s->B * s->N) return fail(ACS_EINVAL, "bad get_all_values arguments");
    HIP_TRY(hipSetDevice(s->device));
    std::vector<InstState> v;
    int rc = read_states(s, v);
    if (rc) return rc;
    // instances stop at different rounds: x_b lives in buffer rounds_b % H.  Copy the buffers
    // holding any instance whole (one transfer each), then pick every instance's row on the host.
    std::vector<unsigned char> used(s->H, 0);
    for (const InstState& e : v) used[e.rounds % s->H] = 1;
    const uint64_t row = s->N * s->es, buf = s->B * s->Npad * s->es;
    uint32_t only = s->H;
    for (uint32_t q = 0; q < s->H; ++q)
        if (used[q]) only = only == s->H ? q : s->H + 1;
    if (only < s->H && s->Npad == s->N) {   // every instance in one buffer: straight into `out`
        HIP_TRY(hipMemcpyAsync(out, xb(s, only), s->B * row, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        return ACS_OK;
    }
    std::vector<unsigned char> h((size_t)buf);
    for (uint32_t q = 0; q < s->H; ++q) {
        if (!used[q]) continue;
        HIP_TRY(hipMemcpyAsync(h.data(), xb(s, q), buf, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        for (uint64_t b = 0; b < s->B; ++b)
            if (v[b].rounds % s->H == q)
                memcpy(static_cast<unsigned char*>(out) + b * row, h.data() + b * s->Npad * s->es, row);
    }
    return ACS_OK;
}

int acs_get_partition_values(acs_sim* s, int partition, void* out, uint64_t n) {
    if (!s || !out || n < s->N) return fail(ACS_EINVAL, "bad arguments");
    if (partition < 0 || partition >= (s->virt ? s->nranks : 1)) return fail(ACS_EINVAL, "no such partition copy");
    HIP_TRY(hipSetDevice(s->device));
    InstState e;
    HIP_TRY(hipMemcpyAsync(&e, s->st, sizeof e, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const double* src = partition == 0 ? s->x[e.rounds & 1u] : s->parts[partition - 1].x[e.rounds & 1u];
    HIP_TRY(hipMemcpyAsync(out, src, s->N * s->es, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ACS_OK;
}

int acs_get_instance_rounds(acs_sim* s, uint32_t* out, uint64_t n) {
    if (!s || !out || n < s->B) return fail(ACS_EINVAL, "bad arguments");
    std::vector<InstState> v;
    int rc = read_states(s, v);
    if (rc) return rc;
    for (uint64_t b = 0; b < s->B; ++b) out[b] = v[b].rounds;
    return ACS_OK;
}

int acs_get_instance_converged(acs_sim* s, uint8_t* out, uint64_t n) {
    if (!s || !out || n < s->B) return fail(ACS_EINVAL, "bad arguments");
    std::vector<InstState> v;
    int rc = read_states(s, v);
    if (rc) return rc;
    for (uint64_t b = 0; b < s->B; ++b) out[b] = (uint8_t)v[b].converged;
    return ACS_OK;
}

int acs_get_instance_spread(acs_sim* s, double* out, uint64_t n) {
    if (!s || !out || n < s->B) return fail(ACS_EINVAL, "bad arguments");
    std::vector<InstState> v;
    int rc = read_states(s, v);
    if (rc) return rc;
    for (uint64_t b = 0; b < s->B; ++b) out[b] = v[b].spread;
    return ACS_OK;
}

int acs_get_spread_trace(acs_sim* s, uint64_t b, double* out, uint64_t n, uint64_t* n_out) {
    if (!s || !out || b >= s->B) return fail(ACS_EINVAL, "bad arguments");
    if (!s->trace) return fail(ACS_EINVAL, "trace_spread was not enabled");
    InstState e;
    HIP_TRY(hipMemcpyAsync(&e, s->st + b, sizeof e, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    uint64_t cnt = (uint64_t)e.rounds + 1;
    if (cnt > n) cnt = n;
    HIP_TRY(hipMemcpyAsync(out, s->trace + b * ((uint64_t)s->c.max_rounds + 1), cnt * sizeof(double),
                           hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (n_out) *n_out = cnt;
    return ACS_OK;
}

int acs_set_state(acs_sim* s, uint32_t round, const void* x, uint64_t n) {
    if (!s || !x || n != s->B * s->N) return fail(ACS_EINVAL, "set_state needs B*N values");
    if (round > s->c.max_rounds) return fail(ACS_EINVAL, "round > max_rounds");
    // Values must be finite and bounded (sums of up to kGenericBigMaxM = 2^27 of them stay finite, so no
    // NaN can ever appear in x: the tagged binned phase B reads every quiet NaN as a sender tag),
    // and -0.0 is canonicalised to +0.0 (sorted value sequences stay unique).
    std::vector<unsigned char> canon(n * s->es);
    if (s->f32) {
        const float* xf = static_cast<const float*>(x);
        float* cf = reinterpret_cast<float*>(canon.data());
        for (uint64_t k = 0; k < n; ++k) {
            if (!(fabsf(xf[k]) <= 1e30f)) return fail(ACS_EINVAL, "set_state: value %llu is not finite or |x| > 1e30", (unsigned long long)k);
            if (s->pushsum && !(fabsf(xf[k]) <= kPushsumMaxAbs32))
                return fail(ACS_EINVAL, "set_state: value %llu has |x| > 1e26 (PUSHSUM, fp32)", (unsigned long long)k);
            if (s->quant && !(fabsf(xf[k]) <= kPushsumMaxAbs32))   // (|x| * 2^k stays finite)
                return fail(ACS_EINVAL, "set_state: value %llu has |x| > 1e26 (quantized messages, fp32)", (unsigned long long)k);
            cf[k] = xf[k] + 0.0f;
        }
    } else {
        const double* xd = static_cast<const double*>(x);
        double* cd = reinterpret_cast<double*>(canon.data());
        for (uint64_t k = 0; k < n; ++k) {
            if (!(fabs(xd[k]) <= 1e300)) return fail(ACS_EINVAL, "set_state: value %llu is not finite or |x| > 1e300", (unsigned long long)k);
            if (s->pushsum && !(fabs(xd[k]) <= kPushsumMaxAbs64))
                return fail(ACS_EINVAL, "set_state: value %llu has |x| > 1e290 (PUSHSUM)", (unsigned long long)k);
            if (s->quant && !(fabs(xd[k]) <= kPushsumMaxAbs64))   // (|x| * 2^k stays finite)
                return fail(ACS_EINVAL, "set_state: value %llu has |x| > 1e290 (quantized messages)", (unsigned long long)k);
            cd[k] = xd[k] + 0.0;
        }
    }
    x = canon.data();
    HIP_TRY(hipSetDevice(s->device));
    for (uint64_t b = 0; b < s->B; ++b) {
        const void* hb = xat(s, x, b * s->N);
        // every delay-history buffer restarts from x; one buffer when synchronous
        for (uint32_t q = 0; q < (s->c.delay_max ? s->H : 1u); ++q)
            HIP_TRY(hipMemcpyAsync(xat(s, s->c.delay_max ? xb(s, q) : xb(s, round), b * s->Npad), hb, s->N * s->es,
                                   hipMemcpyHostToDevice, s->stream));
        for (Part& q : s->parts)
            HIP_TRY(hipMemcpyAsync(xat(s, q.x[round & 1u], b * s->Npad), hb, s->N * s->es, hipMemcpyHostToDevice,
                                   s->stream));
    }
    if (s->pushsum)   // s = x, z = 1
        HIP_TRY(launch_pushsum_fill(xb(s, round), pairs_at(s, round), s->B * s->N, s->f32, s->stream));
    if (s->split)     // the offers of round `round`: its phase's shares of the new pairs
        HIP_TRY(launch_pushsum_offer(pairs_at(s, round), share_at(s, round), offers_at(s, round), s->B, s->N, s->f32,
                                     s->stream));
    if (s->quant)     // what the nodes transmit in round `round`: a pure function of (x, b, round, i)
        HIP_TRY(launch_quantize(xb(s, round), quant_at(s, round), s->B, s->N, round, s->mp, s->qk, s->qdither, s->f32,
                                s->stream));
    if (s->hold)      // and every link empty (a resume with held mass calls acs_set_pushsum_links next)
        HIP_TRY(hipMemsetAsync(s->links, 0, links_bytes(s), s->stream));
    if (s->transit)   // and nothing in transit (a resume with mass in flight calls acs_set_pushsum_transit next)
        HIP_TRY(hipMemsetAsync(s->ring, 0, ring_bytes(s), s->stream));
    return init_state(s, round);
}

int acs_get_pushsum_state(acs_sim* s, uint64_t b, void* s_out, void* z_out, uint64_t n) {
    if (!s || !s_out || !z_out || b >= s->B || n < s->N) return fail(ACS_EINVAL, "bad get_pushsum_state arguments");
    if (!s->pushsum) return fail(ACS_EINVAL, "acs_get_pushsum_state: not a rule-PUSHSUM handle");
    HIP_TRY(hipSetDevice(s->device));
    InstState e;
    HIP_TRY(hipMemcpyAsync(&e, s->st + b, sizeof e, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    std::vector<unsigned char> h(s->N * 2 * s->es);
    HIP_TRY(hipMemcpyAsync(h.data(), static_cast<char*>(pairs_at(s, e.rounds)) + b * s->N * 2 * s->es, h.size(),
                           hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->f32) {
        const float* p = reinterpret_cast<const float*>(h.data());
        for (uint64_t k = 0; k < s->N; ++k) {
            static_cast<float*>(s_out)[k] = p[2 * k];
            static_cast<float*>(z_out)[k] = p[2 * k + 1];
        }
    } else {
        const double* p = reinterpret_cast<const double*>(h.data());
        for (uint64_t k = 0; k < s->N; ++k) {
            static_cast<double*>(s_out)[k] = p[2 * k];
            static_cast<double*>(z_out)[k] = p[2 * k + 1];
        }
    }
    return ACS_OK;
}

int acs_set_pushsum_state(acs_sim* s, uint32_t round, const void* sv, const void* zv, uint64_t n) {
    if (!s || !sv || !zv) return fail(ACS_EINVAL, "null argument");
    if (!s->pushsum) return fail(ACS_EINVAL, "acs_set_pushsum_state: not a rule-PUSHSUM handle");
    if (n != s->B * s->N) return fail(ACS_EINVAL, "set_pushsum_state needs B*N values in s and in z");
    if (round > s->c.max_rounds) return fail(ACS_EINVAL, "round > max_rounds");
    // the mass bound of DESIGN.md §9 admits |s| <= 1e290 (fp32: 1e26); z finite, >= 0 (z <= the same
    // bound); -0.0 is stored as +0.0
    std::vector<unsigned char> h(n * 2 * s->es);
    if (s->f32) {
        float* p = reinterpret_cast<float*>(h.data());
        for (uint64_t k = 0; k < n; ++k) {
            const float a = static_cast<const float*>(sv)[k], z = static_cast<const float*>(zv)[k];
            if (!(fabsf(a) <= kPushsumMaxAbs32))
                return fail(ACS_EINVAL, "set_pushsum_state: s[%llu] is not finite or |s| > 1e26", (unsigned long long)k);
            if (!(z >= 0.0f && z <= kPushsumMaxAbs32))
                return fail(ACS_EINVAL, "set_pushsum_state: z[%llu] must be finite, in [0, 1e26]", (unsigned long long)k);
            p[2 * k] = a + 0.0f;
            p[2 * k + 1] = z + 0.0f;
        }
    } else {
        double* p = reinterpret_cast<double*>(h.data());
        for (uint64_t k = 0; k < n; ++k) {
            const double a = static_cast<const double*>(sv)[k], z = static_cast<const double*>(zv)[k];
            if (!(fabs(a) <= kPushsumMaxAbs64))
                return fail(ACS_EINVAL, "set_pushsum_state: s[%llu] is not finite or |s| > 1e290", (unsigned long long)k);
            if (!(z >= 0.0 && z <= kPushsumMaxAbs64))
                return fail(ACS_EINVAL, "set_pushsum_state: z[%llu] must be finite, in [0, 1e290]", (unsigned long long)k);
            p[2 * k] = a + 0.0;
            p[2 * k + 1] = z + 0.0;
        }
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpyAsync(pairs_at(s, round), h.data(), h.size(), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(launch_pushsum_estimate(pairs_at(s, round), xb(s, round), n, s->f32, s->stream));
    if (s->split)   // as acs_set_state: the offers are rebuilt with the shares of phase round mod period
        HIP_TRY(launch_pushsum_offer(pairs_at(s, round), share_at(s, round), offers_at(s, round), s->B, s->N, s->f32,
                                     s->stream));
    if (s->hold) HIP_TRY(hipMemsetAsync(s->links, 0, links_bytes(s), s->stream));   // as acs_set_state
    if (s->transit) HIP_TRY(hipMemsetAsync(s->ring, 0, ring_bytes(s), s->stream));
    return init_state(s, round);   // (synchronises: h outlives the copy)
}

int acs_get_pushsum_links(acs_sim* s, uint64_t b, void* h_out, void* k_out, uint64_t n) {
    if (!s) return fail(ACS_EINVAL, "null handle");
    if (!s->hold) return fail(ACS_EINVAL, "acs_get_pushsum_links: not a rule-PUSHSUM handle with missing_policy = HOLD");
    if (b >= s->B || n < s->nnz || ((!h_out || !k_out) && s->nnz))
        return fail(ACS_EINVAL, "bad get_pushsum_links arguments (instance < B, n >= nnz = %llu)",
                    (unsigned long long)s->nnz);
    HIP_TRY(hipSetDevice(s->device));
    std::vector<unsigned char> h(s->nnz * 2 * s->es);
    if (s->nnz)
        HIP_TRY(hipMemcpyAsync(h.data(), static_cast<char*>(s->links) + b * s->nnz * 2 * s->es, h.size(),
                               hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->f32) {
        const float* p = reinterpret_cast<const float*>(h.data());
        for (uint64_t e = 0; e < s->nnz; ++e) {
            static_cast<float*>(h_out)[e] = p[2 * e];
            static_cast<float*>(k_out)[e] = p[2 * e + 1];
        }
    } else {
        const double* p = reinterpret_cast<const double*>(h.data());
        for (uint64_t e = 0; e < s->nnz; ++e) {
            static_cast<double*>(h_out)[e] = p[2 * e];
            static_cast<double*>(k_out)[e] = p[2 * e + 1];
        }
    }
    return ACS_OK;
}

int acs_set_pushsum_links(acs_sim* s, const void* hv, const void* kv, uint64_t n) {
    if (!s) return fail(ACS_EINVAL, "null handle");
    if (!s->hold) return fail(ACS_EINVAL, "acs_set_pushsum_links: not a rule-PUSHSUM handle with missing_policy = HOLD");
    if (n != s->B * s->nnz)
        return fail(ACS_EINVAL, "set_pushsum_links needs B*nnz = %llu values in h and in k (got %llu)",
                    (unsigned long long)(s->B * s->nnz), (unsigned long long)n);
    if ((!hv || !kv) && n) return fail(ACS_EINVAL, "null argument");
    // held mass takes the caps of s and z ("mass bound" under HOLD); -0.0 is stored as +0.0
    std::vector<unsigned char> h(n * 2 * s->es);
    if (s->f32) {
        float* p = reinterpret_cast<float*>(h.data());
        for (uint64_t e = 0; e < n; ++e) {
            const float a = static_cast<const float*>(hv)[e], k = static_cast<const float*>(kv)[e];
            if (!(fabsf(a) <= kPushsumMaxAbs32))
                return fail(ACS_EINVAL, "set_pushsum_links: h[%llu] is not finite or |h| > 1e26", (unsigned long long)e);
            if (!(k >= 0.0f && k <= kPushsumMaxAbs32))
                return fail(ACS_EINVAL, "set_pushsum_links: k[%llu] must be finite, in [0, 1e26]", (unsigned long long)e);
            p[2 * e] = a + 0.0f;
            p[2 * e + 1] = k + 0.0f;
        }
    } else {
        double* p = reinterpret_cast<double*>(h.data());
        for (uint64_t e = 0; e < n; ++e) {
            const double a = static_cast<const double*>(hv)[e], k = static_cast<const double*>(kv)[e];
            if (!(fabs(a) <= kPushsumMaxAbs64))
                return fail(ACS_EINVAL, "set_pushsum_links: h[%llu] is not finite or |h| > 1e290", (unsigned long long)e);
            if (!(k >= 0.0 && k <= kPushsumMaxAbs64))
                return fail(ACS_EINVAL, "set_pushsum_links: k[%llu] must be finite, in [0, 1e290]", (unsigned long long)e);
            p[2 * e] = a + 0.0;
            p[2 * e + 1] = k + 0.0;
        }
    }
    HIP_TRY(hipSetDevice(s->device));
    if (n) HIP_TRY(hipMemcpyAsync(s->links, h.data(), h.size(), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));   // h outlives the copy
    return ACS_OK;
}

int acs_get_fault_status(acs_sim* s, uint32_t* out, uint64_t n) {
    if (!s || !out || n < s->B * s->N) return fail(ACS_EINVAL, "bad arguments");
    HIP_TRY(hipSetDevice(s->device));
    if (!s->status) {
        for (uint64_t k = 0; k < s->B * s->N; ++k) out[k] = kHonest;
        return ACS_OK;
    }
    HIP_TRY(hipMemcpyAsync(out, s->status, s->B * s->N * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ACS_OK;
}

int acs_get_neighbors(acs_sim* s, uint32_t* out, uint64_t n) {
    if (!s || !out) return fail(ACS_EINVAL, "bad arguments");
    if (s->c.topology != ACS_TOPO_RANDOM_REGULAR) return fail(ACS_EINVAL, "not a RANDOM_REGULAR topology");
    if (n < s->N * s->d) return fail(ACS_EINVAL, "buffer too small");
    HIP_TRY(hipSetDevice(s->device));
    // always rebuild the full graph in spec (slot) order on the side: the handle's own ELL may be
    // sorted and may hold only this rank's rows
    const uint64_t words = ((s->N + 63) / 64) * 64ull * s->dp;
    std::vector<uint32_t> h(words);
    uint32_t* tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, words * sizeof(uint32_t)));
    const uint64_t gseed = s->c.graph_seed ? s->c.graph_seed : s->c.seed;
    hipError_t e = launch_build_ell(tmp, s->N, 0, s->N, s->d, s->dp, make_feistel(s->N, gseed), s->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), tmp, words * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    (void)hipFree(tmp);
    HIP_TRY(e);
    for (uint64_t i = 0; i < s->N; ++i)
        for (uint32_t t = 0; t < s->d; ++t)
            out[i * s->d + t] = h[ell_slot(i, s->dp, t)];
    return ACS_OK;
}

int acs_set_kernel_timing(acs_sim* s, int enable) {
    if (!s) return fail(ACS_EINVAL, "null sim");
    HIP_TRY(hipSetDevice(s->device));
    int rc = harvest_timing(s);
    if (rc) return rc;
    s->timing = enable > 0 ? (uint32_t)enable : enable < 0 ? (uint32_t)(-(int64_t)enable) : 0u;
    s->timing_runs = enable < 0;
    s->run_end = nullptr;
    s->timing_ctr = 0;
    s->timed_ms = 0.0;
    s->timed_launches = 0;
    return ACS_OK;
}

int acs_get_kernel_timing(acs_sim* s, double* total_ms, uint64_t* launches, char* kernel_name,
                          uint64_t name_cap) {
    if (!s) return fail(ACS_EINVAL, "null sim");
    HIP_TRY(hipSetDevice(s->device));
    int rc = harvest_timing(s);
    if (rc) return rc;
    if (total_ms) *total_ms = s->timed_ms;
    if (launches) *launches = s->timed_launches;
    if (kernel_name && name_cap) {
        strncpy(kernel_name, s->kname.c_str(), name_cap - 1);
        kernel_name[name_cap - 1] = 0;
    }
    return ACS_OK;
}

}  // extern "C"

