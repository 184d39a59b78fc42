/*
 * acsim.h — C ABI of the MI355X-native approximate-consensus round engine.
 *
 * Provenance.  The upstream reference (Dariusrussellkish/approximate-consensus-simulation,
 * mounted at /root/reference) holds exactly one file, README.md:1 ("# eventual-consensus-simulation"),
 * and no code.  There is therefore no upstream function this ABI can replace line for line; every
 * entry point below replaces the spec-level operation named in SURVEY.md §8(a)/(b), and the
 * semantics are those of SURVEY.md Appendix A (the frozen spec that stands in for the missing
 * reference).  Each declaration cites the §8 row / §A section it implements.
 *
 * Conventions.
 *  - Plain C, no C++ or torch types: pointers, sizes and POD structs only.
 *  - Every function returns 0 (ACS_OK) or a negative ACS_E* status; no exceptions cross the ABI.
 *    acs_last_error() returns a thread-local message for the last non-zero status.
 *  - The handle owns every device buffer.  Callers own the host buffers they pass in; the library
 *    copies into / out of them and retains no pointer after return.
 *  - A handle is not thread-safe; distinct handles may be used from distinct threads.
 */
#ifndef ACSIM_H
#define ACSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACS_ABI_VERSION 4   /* 2: acs_config.delay_max (bounded-delay rounds);
                               3: acs_config.missing_policy (was reserved0), acs_get_all_values;
                               4: ACS_RULE_WEIGHTED, acs_create_csr_weighted, acs_get_weights
                                  (still 4: ACS_RULE_PUSHSUM and acs_get / acs_set_pushsum_state are
                                  additions; acs_config and every older symbol are unchanged;
                                  likewise ACS_MISSING_HOLD and acs_get / acs_set_pushsum_links;
                                  likewise ACS_SCHEDULE_MAX_PERIOD, acs_create_csr_scheduled and
                                  acs_get_link_schedule; likewise acs_create_csr_split and
                                  acs_get_split_shares; likewise acs_create_csr_transit and
                                  acs_get / acs_set_pushsum_transit; likewise ACS_STREAM_QUANT,
                                  ACS_QUANT_*, acs_create_csr_quantized and acs_get_quantized) */

/* status codes */
#define ACS_OK            0
#define ACS_EINVAL       (-1)
#define ACS_ENOMEM       (-2)
#define ACS_EDEVICE      (-3)
#define ACS_ECOMM        (-4)
#define ACS_EUNSUPPORTED (-5)

/* backends.  The product library implements ACS_HIP only; the CPU spec reference lives in
 * oracle/ as test infrastructure and is not reachable through this library (ACS_CPU returns
 * ACS_EUNSUPPORTED here). */
#define ACS_CPU 0
#define ACS_HIP 1

/* topology (§A.3) */
#define ACS_TOPO_COMPLETE        0
#define ACS_TOPO_RANDOM_REGULAR  1
#define ACS_TOPO_CSR             2   /* user-supplied adjacency, see acs_create_csr (§8(f) row 1) */

/* update rule (§A.7) */
#define ACS_RULE_AVERAGE       0
#define ACS_RULE_TRIMMED_MEAN  1
#define ACS_RULE_MIDPOINT      2
#define ACS_RULE_DLPSW_SELECT  3
/* W-MSR (LeBlanc et al. 2013): drop up to t entries strictly below the receiver's
 * own value (the smallest ones) and up to t strictly above it (the largest), average the rest */
#define ACS_RULE_WMSR          4
/* Edge-weighted averaging x' = W x on a CSR graph: entry e of receiver i carries a
 * weight (w_self[i], then w_edge[slot]); x_i' = tree_sum(w_e * v_e) / tree_sum(w_e).  CSR topology
 * and trim == 0 only; handles come from acs_create_csr_weighted */
#define ACS_RULE_WEIGHTED      5
/* Push-sum / ratio consensus on a directed CSR graph (Kempe, Dobra, Gehrke 2003):
 * node i holds a pair (s_i, z_i), s_i = x_i^0 and z_i = 1 at round 0; a round sets
 * s_i' = tree_sum(w_e * s_e), z_i' = tree_sum(w_e * z_e) over the receiver's entries with the
 * weights of rule WEIGHTED (no normalisation) and x_i' = s_i' / z_i' (x_i is kept while z_i' = 0).
 * With column sums of the weights equal to 1 the mass sum(s) / sum(z) is the mean of x^0, which
 * every x_i approaches.  CSR topology, trim == 0, no faults, no delays; loss needs
 * missing_policy = OMIT (a dropped message loses its mass) or HOLD (it waits on the link, see
 * ACS_MISSING_HOLD).  Handles come from acs_create_csr_weighted */
#define ACS_RULE_PUSHSUM       6

/* fault model (§A.4) */
#define ACS_FAULT_NONE       0
#define ACS_FAULT_CRASH      1
#define ACS_FAULT_BYZANTINE  2

/* Byzantine strategy (§A.4) */
#define ACS_BYZ_SPLIT     0
#define ACS_BYZ_RANDOM    1
#define ACS_BYZ_CONSTANT  2

/* termination (§A.8) */
#define ACS_TERM_EPS    0
#define ACS_TERM_FIXED  1

/* missing-message policy (§A.6): a crashed-silent or dropped message is replaced
 * by the receiver's own value (SELF, the §A.6 default), or removed from S_i (OMIT: m_i shrinks;
 * the trimming rules keep x_i when m_i <= 2t) */
#define ACS_MISSING_SELF 0
#define ACS_MISSING_OMIT 1
/* HOLD (rule ACS_RULE_PUSHSUM only, ACS_EINVAL with any other rule): robust ratio
 * consensus by running sums.  A dropped message's mass is not lost: it waits on the link and arrives
 * with the next message that gets through.  Besides (s_i, z_i), every slot e = rowptr[i] + t of
 * every instance holds a pair (h_e, k_e) of the config dtype, +0.0 at round 0.  Per sender entry e
 * of receiver i, sender j = colidx[e]:
 *   a = (w_e * s_j) + 0.0, c = (w_e * z_j) + 0.0    (as without HOLD: two roundings each, no FMA)
 *   hn = h_e + a, kn = k_e + c                       (one rounding each)
 *   dropped = loss_p > 0 && draw(key, DROP, bG, r, e) < thr     (the draw OMIT makes)
 *   delivered: the entry contributes (hn, kn) to the two sums and the link stores (+0.0, +0.0)
 *   dropped:   the entry contributes (+0.0, +0.0) and the link stores (hn, kn)
 * Entry 0 (the receiver itself) has no link; sums, x and the stored pair are as without HOLD.  With
 * column sums of 1, sum(z) + sum(k) stays N and every x_i approaches the mean of x^0 under loss,
 * where OMIT ends away from it.  With loss_p = 0 a HOLD run equals the plain run bit for bit. */
#define ACS_MISSING_HOLD 2

/* value type (§A.0): fp64, or binary32 throughout */
#define ACS_F64 0
#define ACS_F32 1

/* Philox streams (§A.1) */
#define ACS_STREAM_INIT          0u
#define ACS_STREAM_DROP          1u
#define ACS_STREAM_FAULTSET      2u
#define ACS_STREAM_CRASH_ROUND   3u
#define ACS_STREAM_CRASH_PARTIAL 4u
#define ACS_STREAM_BYZ           5u
#define ACS_STREAM_GRAPH         6u
#define ACS_STREAM_DELAY         7u   /* bounded-delay rounds */
#define ACS_STREAM_QUANT         8u   /* dither of quantized messages */

/* quantized messages ("Quantized messages"; acs_create_csr_quantized): what entry 0
 * of a receiver's row is, and whether the quantization error is added back */
#define ACS_QUANT_PARTIAL     0   /* entry 0 is x_i; x_i' = y */
#define ACS_QUANT_TOTAL       1   /* entry 0 is q_i; x_i' = y */
#define ACS_QUANT_COMPENSATED 2   /* entry 0 is q_i; x_i' = y + (x_i - q_i): the mean is kept */

/* Opaque simulation handle. */
typedef struct acs_sim acs_sim;

/* One simulation configuration.  POD; struct_size must equal sizeof(acs_config). */
typedef struct acs_config {
    uint32_t struct_size;
    uint64_t n_nodes;          /* N */
    uint64_t n_instances;      /* B: independent instances held by this handle */
    uint32_t topology;         /* ACS_TOPO_* */
    uint32_t degree;           /* d (even, >= 2) for RANDOM_REGULAR */
    uint32_t rule;             /* ACS_RULE_* */
    uint32_t trim;             /* t */
    uint32_t fault_model;      /* ACS_FAULT_* */
    uint32_t n_faulty;         /* f */
    uint32_t byz_strategy;     /* ACS_BYZ_* */
    double   byz_delta;        /* Δ */
    double   byz_const;        /* c */
    uint32_t crash_window;     /* W >= 1 */
    double   loss_p;           /* message-loss probability in [0,1) */
    uint32_t mask_group;       /* G >= 1: instances b with equal b - b%G share drop masks */
    double   eps;              /* ε */
    uint32_t max_rounds;       /* round cap (EPS) or exact round count (FIXED) */
    uint32_t termination;      /* ACS_TERM_* */
    uint32_t dtype;            /* ACS_F64 | ACS_F32 */
    uint64_t seed;             /* Philox key for every stream except GRAPH */
    uint64_t graph_seed;       /* Philox key for GRAPH; 0 means "use seed" */
    uint32_t trace_spread;     /* 1: keep spread^r for every round (per instance) */
    uint32_t omp_threads;      /* CPU oracle only; ignored by the HIP library */
    uint64_t instance_offset;  /* global id of local instance 0 (multi-GPU instance sharding, §8e) */
    uint32_t delay_max;        /* D: bounded-delay rounds; 0 = synchronous (§A.6) */
    uint32_t missing_policy;   /* ACS_MISSING_*: what a missing message becomes */
} acs_config;

/* Result of acs_round. For B > 1: round = max rounds over instances,
 * spread = max current spread over instances, lo/hi = instance 0's honest min/max. */
typedef struct acs_round_info {
    uint32_t round;            /* rounds executed so far (max over instances) */
    uint32_t done;             /* 1 when every instance has terminated */
    double   spread;
    double   lo;
    double   hi;
    uint64_t instances_done;
} acs_round_info;

/* Result of acs_run. */
typedef struct acs_result {
    uint32_t rounds_max;       /* max over instances of rounds executed */
    uint32_t n_converged;      /* instances with final spread <= eps */
    uint64_t node_rounds;      /* Σ_b N · rounds_executed(b) */
    double   wall_seconds;     /* host wall time of this call */
    double   final_spread_max; /* max over instances of final spread */
    uint64_t n_instances;
} acs_result;

/* §8b: create a simulation (validates the §A.8 constraints, allocates HBM, builds the graph,
 * the fault schedule and x^0 on the device).  devices/n_devices: exactly one device id. */
int acs_create(const acs_config* cfg, int backend, const int* devices, int n_devices,
               struct acs_sim** out);

/* §8(f) row 1: a simulation on a user-supplied graph in CSR form (cfg->topology = ACS_TOPO_CSR;
 * cfg->degree is ignored).  Receiver i's entries are itself (entry 0, no slot) followed by the
 * senders colidx[rowptr[i] + t], t < deg(i) = rowptr[i+1] - rowptr[i], on slot s = rowptr[i] + t;
 * m_i = deg(i) + 1 varies per receiver (trim rules need m_i > 2t for every i).  rowptr has N+1
 * entries (rowptr[0] = 0, non-decreasing, rowptr[N] < 2^34), colidx rowptr[N] entries < N.
 * Both arrays are copied to the device. */
int acs_create_csr(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx, int device,
                   struct acs_sim** out);

/* DESIGN.md §9 (rule "weighted"): acs_create_csr with one weight per entry, shared by all
 * instances: w_self[N] for entry 0 and w_edge[rowptr[N]] indexed by slot.  cfg->rule must be
 * ACS_RULE_WEIGHTED or ACS_RULE_PUSHSUM (and only this entry point takes those rules) with
 * cfg->trim == 0.  Every weight
 * must be finite with 0 <= w <= 1 and every row's weight sum positive; with cfg->dtype = ACS_F32
 * the weights are rounded to binary32 once, here, and checked after rounding.  All of this is
 * checked on the host before any device call (ACS_EINVAL).  Rows above 8192 entries are not
 * served yet (ACS_EUNSUPPORTED).
 * ACS_RULE_PUSHSUM adds: every column sum (w_self[j] plus every w_edge[slot] with colidx[slot] == j,
 * a compensated double sum of the weights as held) must be at most 1 + 2^-30, so the total mass
 * cannot grow without bound; fault_model must be NONE and loss_p > 0 needs missing_policy = OMIT
 * or HOLD (ACS_EINVAL); delay_max > 0 is not served (ACS_EUNSUPPORTED); with ACS_F32, max_rounds <= 2^22
 * (ACS_EINVAL; the bound that keeps every binary32 sum finite). */
int acs_create_csr_weighted(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx,
                            const double* w_self, const double* w_edge, int device, struct acs_sim** out);

/* The weights the device holds (fp32 handles: the rounded weights, widened back to double):
 * n = N values into w_self_out, nnz = rowptr[N] values into w_edge_out.  Handles of
 * acs_create_csr_weighted only (rules WEIGHTED and PUSHSUM). */
int acs_get_weights(struct acs_sim* sim, double* w_self_out, uint64_t n, double* w_edge_out, uint64_t nnz);

/* DESIGN.md §9 ("Link schedules"): acs_create_csr_weighted on a time-varying graph.  A link
 * schedule is a period P, 1 <= P <= ACS_SCHEDULE_MAX_PERIOD, and one mask per CSR slot, shared by all
 * instances: bit p (p < P) of avail[slot] is set when the link on that slot is up in every round r
 * with r mod P == p (r: the instance's own round index, which continues across acs_set_state and
 * acs_set_pushsum_state).  Bits at positions >= P must be zero; avail[slot] == 0 is a dead link.
 * A message on a slot that is down in round r is missing exactly as a dropped one: WEIGHTED / SELF
 * takes x_i and keeps the weight, WEIGHTED / OMIT leaves the entry out, PUSHSUM / OMIT loses the
 * mass, PUSHSUM / HOLD keeps it on the link until the slot is up again (the mean-preserving choice).
 * With delay_max > 0 (WEIGHTED) the availability tested is that of the delivery round.
 * Checked on the host before any device call: period outside 1..32, a null avail or a bit at a
 * position >= period (ACS_EINVAL, naming the first offending slot); a rule other than WEIGHTED or
 * PUSHSUM (ACS_EUNSUPPORTED); PUSHSUM with missing_policy = SELF and a slot that is not up in every
 * phase (ACS_EINVAL); and every check of acs_create_csr_weighted. */
#define ACS_SCHEDULE_MAX_PERIOD 32
int acs_create_csr_scheduled(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx,
                             const double* w_self, const double* w_edge,
                             uint32_t period, const uint32_t* avail, int device, struct acs_sim** out);
/* period into *period_out, nnz masks in slot order into avail_out; ACS_EINVAL on an unscheduled handle */
int acs_get_link_schedule(struct acs_sim* sim, uint32_t* period_out, uint32_t* avail_out, uint64_t nnz);

/* DESIGN.md §9 ("Push-sum with per-round splitting"): rule PUSHSUM on a link schedule with no weights.
 * In round r, phase p = r mod P, sender j divides its pair by c_p(j) = 1 + (its slots that are up in
 * phase p): share_p(j) = 1 / c_p(j) rounded to the config dtype, one ulp lower where c_p(j) * share
 * would exceed 1 exactly.  Every round's matrix is column-stochastic, so the mean is kept on any
 * schedule with no per-link state; a message lost to loss_p loses its mass, as under OMIT.
 * The schedule is acs_create_csr_scheduled's and is checked the same way, except that slots that are
 * down in some phase are allowed under missing_policy = SELF when loss_p == 0 (nothing is sent on a
 * down link, so nothing is missing).  Checked on the host before any device call: a rule other than
 * PUSHSUM, trim != 0, a fault model, loss_p > 0 with SELF (ACS_EINVAL); missing_policy = HOLD,
 * delay_max > 0, a row above 8192 entries (ACS_EUNSUPPORTED).
 * acs_get_link_schedule, acs_get / acs_set_pushsum_state and acs_set_state serve the handle;
 * acs_get_weights returns phase 0's effective weights (0 on a slot that is down in phase 0). */
int acs_create_csr_split(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx,
                         uint32_t period, const uint32_t* avail, int device, struct acs_sim** out);
/* The share table as the device holds it, phase-major: out[p * N + j] = share_p(j), n = P * N values
 * (fp32 handles: widened to double).  ACS_EINVAL on any handle not made by acs_create_csr_split. */
int acs_get_split_shares(struct acs_sim* sim, double* out, uint64_t n);

/* DESIGN.md §9 ("Push-sum with messages in transit"): rule PUSHSUM under bounded delays.  A message
 * sent in round r on slot e arrives in round r + delta, delta = draw(DELAY, b, r, e) mod
 * (transit_max + 1) with b the global instance id; until then its mass is in transit on the link, so
 * node mass plus transit mass is conserved and the run converges to the mean.  (acs_config.delay_max
 * is another model, a stale read of values, and stays refused for PUSHSUM.)  A message that is
 * dropped, or down under the schedule, in the round it is sent never enters transit: its mass is
 * lost, as under OMIT.  The EPS test looks at x alone: a run may stop with mass in transit.
 * period, avail: a link schedule as for acs_create_csr_scheduled, or 0, NULL for none.
 * transit_max = 0 computes what acs_create_csr_weighted / _scheduled computes, bit for bit.
 * Checked on the host before any device call: a rule other than PUSHSUM, missing_policy = HOLD,
 * delay_max > 0 (ACS_EUNSUPPORTED); transit_max > 64, ACS_F32 with max_rounds above
 * floor(2^26 / (16 + transit_max)) (ACS_EINVAL); and every check of acs_create_csr_weighted /
 * acs_create_csr_scheduled.  The ring of pending pairs takes B * (transit_max + 1) * nnz pairs of
 * device memory (ACS_ENOMEM when that fails). */
int acs_create_csr_transit(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx,
                           const double* w_self, const double* w_edge,
                           uint32_t period, const uint32_t* avail,   /* 0, NULL: no schedule */
                           uint32_t transit_max, int device, struct acs_sim** out);
/* The mass in transit, ACS_EINVAL on any handle not made by acs_create_csr_transit (and on a
 * transit_max = 0 handle with n != 0).  Planes are relative to the instance's own executed rounds R:
 * acs_get_pushsum_transit: out[d * nnz + e], d = 0 .. transit_max - 1, is what round R + d will
 * deliver on slot e from messages already sent; n >= transit_max * nnz values of the config dtype
 * into each of h_out and k_out.
 * acs_set_pushsum_transit: n = B * transit_max * nnz values in each array, instance-major, each
 * instance plane-major as above.  |h| <= 1e290 (ACS_F32: 1e26), k finite, >= 0 and within the same
 * cap; -0.0 is stored as +0.0.  acs_set_state and acs_set_pushsum_state empty the planes, so a resume
 * with mass in flight calls acs_set_pushsum_transit after them. */
int acs_get_pushsum_transit(struct acs_sim* sim, uint64_t instance, void* h_out, void* k_out, uint64_t n);
int acs_set_pushsum_transit(struct acs_sim* sim, const void* h, const void* k, uint64_t n);

/* DESIGN.md §9 ("Quantized messages"): rule WEIGHTED on links that carry a finite number of bits.
 * Every node transmits q = Q(x), its state on the grid of step 2^-step_log2, and the rule's arithmetic
 * runs on those values unchanged.  Q(x; b, r, i) for node i of global instance b in round r:
 * u = x * 2^k; dither = 0: n = rint(u) (half to even); dither = 1: f = floor(u), g = u - f,
 * n = f + (draw(QUANT, b, r, i) < (uint32)(g * 2^32)); q = n * 2^-k + 0.0.  Every step is exact in the
 * config dtype.  Sender entries are q_j; entry 0, which a missing entry also takes under SELF, is x_i
 * (ACS_QUANT_PARTIAL) or q_i (ACS_QUANT_TOTAL, ACS_QUANT_COMPENSATED); y = num / den; x_i' = y, or
 * y + (x_i - q_i) under ACS_QUANT_COMPENSATED; a zero weight sum keeps x_i.
 * period, avail: a link schedule as for acs_create_csr_scheduled, or 0, NULL for none.
 * Checked on the host before any device call: a rule other than WEIGHTED, a fault model, delay_max > 0
 * (ACS_EUNSUPPORTED); step_log2 > 52 (ACS_F32: 23), mode > 2, dither > 1 (ACS_EINVAL); and every check
 * of acs_create_csr_weighted / acs_create_csr_scheduled.  acs_set_state on such a handle admits
 * |x| <= 1e290 (ACS_F32: 1e26) and recomputes q. */
int acs_create_csr_quantized(const acs_config* cfg, const uint64_t* rowptr, const uint32_t* colidx,
                             const double* w_self, const double* w_edge,
                             uint32_t period, const uint32_t* avail,   /* 0, NULL: no schedule */
                             uint32_t step_log2, uint32_t mode, uint32_t dither, int device,
                             struct acs_sim** out);
/* What the instance's nodes transmit in its next round R (its executed rounds): q^R = Q(x^R; b, R, .),
 * n >= N values of the config dtype.  ACS_EINVAL on any handle not made by acs_create_csr_quantized. */
int acs_get_quantized(struct acs_sim* sim, uint64_t instance, void* out, uint64_t n);

/* §8(e) node partitioning of ONE RANDOM_REGULAR instance over n_ranks GPUs (cfg5), one process
 * (or thread) per GPU.  Rank r owns the 64-aligned row block [r*R, (r+1)*R) ∩ [0, N),
 * R = ceil(ceil(N/n_ranks)/64)*64, keeps the full x on its GPU, and after every round exchanges
 * x^{r+1} with an in-place RCCL all-gather over xGMI plus an all-reduce of the honest
 * (-min, max) for the ε test, so every rank holds identical state.
 *   acs_get_comm_id: rank 0 creates the RCCL unique id (acs_comm_id_size() bytes) that every
 *   rank passes to acs_create_partitioned (any out-of-band channel, e.g. torch.distributed).
 *   comm_id == NULL with n_ranks > 1 simulates all n_ranks partitions on `device` with private
 *   x copies and a device-memcpy all-gather (validation of the partitioned data flow on one GPU;
 *   rank must be 0).  n_ranks == 1 behaves like acs_create. */
int acs_comm_id_size(void);
int acs_get_comm_id(void* out, uint64_t n);
int acs_create_partitioned(const acs_config* cfg, int device, int n_ranks, int rank,
                           const void* comm_id, uint64_t id_len, struct acs_sim** out);
/* Virtual partitions only: the private x copy of one partition (all copies are identical after
 * every round's all-gather; partition 0's copy is what acs_get_values returns). */
int acs_get_partition_values(struct acs_sim* sim, int partition, void* out, uint64_t n);

/* §8(a) a10/a9: advance every unfinished instance by at most k rounds; stops at convergence. */
int acs_round(struct acs_sim* sim, uint32_t k, acs_round_info* out);

/* §8(a) a11: run to convergence (EPS) or exactly max_rounds (FIXED). */
int acs_run(struct acs_sim* sim, acs_result* out);

/* Copy instance's current node values (N values of the config dtype) into a caller buffer. */
int acs_get_values(struct acs_sim* sim, uint64_t instance, void* out, uint64_t n);

/* Every instance's current values (B*N values, instance-major) in one call; instances that
 * terminated at different rounds are each read from their own round's buffer. */
int acs_get_all_values(struct acs_sim* sim, void* out, uint64_t n);

/* Per-instance rounds executed / converged flag / current spread. */
int acs_get_instance_rounds(struct acs_sim* sim, uint32_t* out, uint64_t n_instances);
int acs_get_instance_converged(struct acs_sim* sim, uint8_t* out, uint64_t n_instances);
int acs_get_instance_spread(struct acs_sim* sim, double* out, uint64_t n_instances);

/* Spread trace spread^0..spread^rounds of one instance (needs trace_spread = 1).
 * *n_out receives the number of values written (rounds + 1, capped at n). */
int acs_get_spread_trace(struct acs_sim* sim, uint64_t instance, double* out, uint64_t n,
                         uint64_t* n_out);

/* Resume (§A.9): set every instance to round `round` with values x (B*N values, instance-major).
 * Instances become unfinished unless the EPS test already holds at `round`. */
int acs_set_state(struct acs_sim* sim, uint32_t round, const void* x, uint64_t n);

/* Rule PUSHSUM, ACS_EINVAL on any other handle.
 * acs_get_pushsum_state: the pairs of one instance, n >= N values of the config dtype into each of
 * s_out and z_out, read from the buffer of the instance's own round (as acs_get_values reads x).
 * acs_set_pushsum_state: resume with pairs, n = B*N values of the config dtype in each array,
 * instance-major.  |s| <= 1e290 (ACS_F32: 1e26), z finite and >= 0; -0.0 is stored as +0.0.  x is
 * recomputed on the device: s / z where z > 0, and s where z = 0.  Spread and done flags restart as
 * for acs_set_state.  On a push-sum handle acs_set_state(round, x) sets s = x and z = 1, with the
 * same bound on |x|. */
int acs_get_pushsum_state(struct acs_sim* sim, uint64_t instance, void* s_out, void* z_out, uint64_t n);
int acs_set_pushsum_state(struct acs_sim* sim, uint32_t round, const void* s, const void* z, uint64_t n);

/* Rule PUSHSUM with missing_policy = ACS_MISSING_HOLD, ACS_EINVAL on any other handle: the held
 * (h, k) pair of every link, in slot order (slot rowptr[i] + t carries colidx[slot] -> i).
 * acs_get_pushsum_links: one instance's links, n >= nnz = rowptr[N] values of the config dtype
 * into each of h_out and k_out.
 * acs_set_pushsum_links: n = B*nnz values of the config dtype in each array, instance-major.
 * |h| <= 1e290 (ACS_F32: 1e26), k finite, >= 0 and within the same cap; -0.0 is stored as +0.0.
 * acs_set_state and acs_set_pushsum_state empty every link, so a resume with held mass calls
 * acs_set_pushsum_links after them. */
int acs_get_pushsum_links(struct acs_sim* sim, uint64_t instance, void* h_out, void* k_out, uint64_t n);
int acs_set_pushsum_links(struct acs_sim* sim, const void* h, const void* k, uint64_t n);

/* Device-side fault schedule (§A.4): per node u32 status, 0xFFFFFFFF honest, 0xFFFFFFFE
 * Byzantine, otherwise the crash round r_v.  out holds B*N words. */
int acs_get_fault_status(struct acs_sim* sim, uint32_t* out, uint64_t n);

/* Adjacency (§A.3) of a RANDOM_REGULAR graph: out[i*d + t] = nbr(i, t). */
int acs_get_neighbors(struct acs_sim* sim, uint32_t* out, uint64_t n);

/* Kernel timing (bench measurement, §8d): while enabled, HIP events bracket the launches of the
 * round kernel on the handle's stream — every round for enable == 1, every enable-th round for
 * enable > 1 (each event pair idles the stream for a few µs, so the bench samples); enable < 0
 * brackets runs of -enable consecutive rounds with one pair each (a run ends at the end of an
 * acs_round / acs_run call at the latest) and counts every round of a run as one launch; 0 disables.
 * A run's pair brackets EVERYTHING the handle enqueues between its first and last round, not only
 * the round kernels: on node-partitioned handles the RCCL exchange, the (-min, max) all-reduce and
 * the finalize; on EPS runs of long rounds, which wait for each 16-round chunk's verdict before
 * enqueuing the next, the host round trip at a chunk boundary inside the run.  Use enable >= 1
 * for a kernel-only figure there (bench.py uses run mode on the one-instance cfg4 legs only).
 * acs_get_kernel_timing returns the summed device time and bracketed launch count since the
 * last reset, plus the name of the round kernel in use. */
int acs_set_kernel_timing(struct acs_sim* sim, int enable);
int acs_get_kernel_timing(struct acs_sim* sim, double* total_ms, uint64_t* launches,
                          char* kernel_name, uint64_t name_cap);

/* Wait for all device work of this handle. */
int acs_sync(struct acs_sim* sim);

/* Process-level facts for multi-GPU launchers (bench.py, acsim.rendezvous): the number of HIP
 * devices visible (hipGetDeviceCount), and the HIP runtime and RCCL versions this library is
 * running on, as "hip <hipRuntimeGetVersion> rccl <ncclGetVersion>" (NUL-terminated, cut to cap). */
int acs_device_count(void);
int acs_runtime_info(char* out, uint64_t cap);

void acs_destroy(struct acs_sim* sim);
const char* acs_last_error(void);
int acs_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ACSIM_H */
