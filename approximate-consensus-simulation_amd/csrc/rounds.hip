// rounds.hip — the round loop of a handle: one round's launches on every kernel path (with node
// partitions over virtual copies or RCCL), the round-chunk loop with device-side
// early exit, the host-mapped state and summary polling, and the bench-time kernel event timing.
// enqueue_round and advance share this translation unit: on the headline the host's enqueue cost
// is within a microsecond of the device time per round, and the inlining here is part of it.
#include <chrono>
#include <thread>

#include "handle.hpp"

using namespace acs;

static FinalizeArgs make_finalize(acs_sim* s, uint32_t r_next, const double2* partial, uint32_t nblk,
                                  bool init) {
    FinalizeArgs f{};
    f.st = s->st;
    f.partial = partial;
    f.nblk = nblk;
    f.r_next = r_next;
    f.max_rounds = s->c.max_rounds;
    f.term_eps = s->c.termination == ACS_TERM_EPS;
    f.eps = s->c.eps;
    f.trace = s->trace;
    f.trace_stride = (uint64_t)s->c.max_rounds + 1;
    f.n_done = s->n_done;
    f.init_mode = init ? 1u : 0u;
    f.f32 = s->f32 ? 1u : 0u;
    return f;
}

// (Re)initialise the per-instance state from x[round & 1] (create and set_state).  Every rank
// holds the full x, so the initial honest min/max needs no exchange.
int init_state(acs_sim* s, uint32_t round) {
    HIP_TRY(hipMemsetAsync(s->n_done, 0, sizeof(uint32_t), s->stream));
    HIP_TRY(launch_partials_from_x(xb(s, round), s->status, s->B, s->N, s->partial, s->nblk_init, s->f32, s->stream));
    const FinalizeArgs f = make_finalize(s, round, s->partial, s->nblk_init, true);
    HIP_TRY(launch_finalize(f, s->B, s->stream));
    HIP_TRY(hipMemcpyAsync(s->h_ndone, s->n_done, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->round = round;
    s->all_done = s->h_ndone[0] == s->B;
    return ACS_OK;
}

static hipEvent_t next_event(acs_sim* s) {
    if (s->ev_used == s->ev.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        s->ev.push_back(e);
    }
    return s->ev[s->ev_used++];
}

int harvest_timing(acs_sim* s) {
    if (s->ev_used == 0) return ACS_OK;
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (size_t k = 0; k + 1 < s->ev_used; k += 2) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev[k], s->ev[k + 1]));
        s->timed_ms += ms;
        s->timed_launches += k / 2 < s->ev_w.size() ? s->ev_w[k / 2] : 1u;
    }
    s->ev_used = 0;
    return ACS_OK;
}

// one bracketed launch (the binned pair of a round, one partition round, or one batched / dense
// launch covering a whole round(k) call: acs_get_kernel_timing counts launches, not rounds)
static int timing_begin(acs_sim* s, hipEvent_t* e1) {
    *e1 = nullptr;
    if (s->timing && s->timing_runs) {   // runs of `timing` consecutive rounds, one pair per run
        const uint64_t pos = s->timing_ctr++ % s->timing;
        if (pos == 0 && !s->run_end) {
            if (s->ev_used + 2 > 4096) {
                int rc = harvest_timing(s);
                if (rc) return rc;
            }
            if (s->ev_w.size() < s->ev_used / 2 + 1) s->ev_w.resize(s->ev_used / 2 + 1);
            s->ev_w[s->ev_used / 2] = 0;
            hipEvent_t e0 = next_event(s);
            s->run_end = next_event(s);
            if (!e0 || !s->run_end) return fail(ACS_EDEVICE, "hipEventCreate failed");
            HIP_TRY(hipEventRecord(e0, s->stream));
            s->run_rounds = 0;
        }
        s->run_rounds++;
        if (pos + 1 == s->timing) {   // the run's last round: the caller records the end event
            *e1 = s->run_end;
            s->ev_w[s->ev_used / 2 - 1] = s->run_rounds;
            s->run_end = nullptr;
        }
        return ACS_OK;
    }
    if (!s->timing || s->timing_ctr++ % s->timing != 0) return ACS_OK;
    if (s->ev_used + 2 > 4096) {
        int rc = harvest_timing(s);
        if (rc) return rc;
    }
    if (s->ev_w.size() < s->ev_used / 2 + 1) s->ev_w.resize(s->ev_used / 2 + 1);
    s->ev_w[s->ev_used / 2] = 1;
    hipEvent_t e0 = next_event(s);
    *e1 = next_event(s);
    if (!e0 || !*e1) return fail(ACS_EDEVICE, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(e0, s->stream));
    return ACS_OK;
}

// Close a timing run still open at the end of an advance() call (run mode: a run never spans
// two calls, so host time between calls is never bracketed).
static int timing_close(acs_sim* s) {
    if (!s->run_end) return ACS_OK;
    HIP_TRY(hipEventRecord(s->run_end, s->stream));
    s->ev_w[s->ev_used / 2 - 1] = s->run_rounds;
    s->run_end = nullptr;
    s->timing_ctr = 0;
    return ACS_OK;
}

static RoundArgs round_args(acs_sim* s, uint32_t r) {
    RoundArgs a{};
    a.xin = xb(s, r);
    a.xout = xb(s, r + 1);
    a.xh = s->xall;
    a.xstride = s->xstride;
    a.H = s->H;
    a.delay = s->c.delay_max;
    a.ell = s->ell;
    a.status = s->status;
    a.st = s->st;
    a.partial = s->partial;
    a.N = s->N;
    a.row0 = 0;
    a.nrows = s->N;
    a.rowptr = s->rowptr;
    a.colidx = s->colidx;
    a.m = (uint32_t)s->m;
    a.d = s->d;
    a.dp = s->dp;
    a.topology = s->c.topology;
    a.rule = s->c.rule;
    a.trim = s->c.trim;
    a.r = r;
    a.nblk = s->nblk;
    a.mp = s->mp;
    a.f32 = s->f32 ? 1u : 0u;
    a.deg = s->deg;
    a.sw = s->sw;
    a.qlo = 0;
    a.qhi = 0xFFFFFFFFu;
    a.crank = s->crank;
    a.clist = s->clist;
    a.coff = s->clist && r < s->coff.size() ? s->coff[r] : 0u;
    a.wself = s->wself;
    a.wedge = s->wedge;
    a.well = s->well;
    if (s->sched) {   // (the phase follows the round index, also after acs_set_state(round, ...))
        a.avail = s->avail;
        a.avell = s->avell;
        a.phase = 1u << (r % s->period);
    }
    if (s->pushsum) {
        a.pin = pairs_at(s, r);
        a.pout = pairs_at(s, r + 1);
        a.lnk = s->links;   // (HOLD handles only: null selects the plain rule in k_round_generic)
        a.lnk_stride = s->nnz;
    }
    if (s->transit) {   // (the plane follows the round index, like the schedule's phase)
        a.trn = s->ring;
        a.trn_np = s->tmax + 1;
        a.trn_cur = r % a.trn_np;
    }
    if (s->split) {   // (this round's shares are in the offers already)
        a.oin = offers_at(s, r);
        a.oout = offers_at(s, r + 1);
        a.share_next = share_at(s, r + 1);
    }
    if (s->quant) {   // (what the nodes transmit in this round was stored with x^r)
        a.qin = quant_at(s, r);
        a.qout = quant_at(s, r + 1);
        a.qk = s->qk;
        a.qmode = s->qmode;
        a.qdither = s->qdither;
    }
    return a;
}

static uint64_t chunk_rows(const acs_sim* s, int p, uint32_t k) {
    const uint64_t cs = s->rows_per / s->xchunks, n = part_rows(s, p), lo = (uint64_t)k * cs;
    return n > lo ? (n - lo < cs ? n - lo : cs) : 0;
}

// ---- pieces the two partitioned round sequences share
// RoundArgs of partition g's rows: a virtual partition reads and writes its private copies (its
// partials land at partial[g * nblk]); an RCCL rank (g = its rank) its own rows of the one copy.
static RoundArgs part_args(const acs_sim* s, const RoundArgs& a, int g, uint32_t r) {
    RoundArgs ap = a;
    if (s->virt && g > 0) {
        ap.xin = s->parts[g - 1].x[r & 1u];
        ap.xout = s->parts[g - 1].x[(r + 1) & 1u];
        ap.ell = s->parts[g - 1].ell;   // (null like s->ell where the binned plans replaced the ELLs)
    }
    ap.row0 = part_row0(s, g);
    ap.nrows = part_rows(s, g);
    if (s->virt) ap.partial = s->partial + (uint64_t)g * s->nblk;
    return ap;
}

// Virtual partitions: rows [off, off + n) of partition p's copy of x^{r+1} into every other copy, on stream q.
static int copy_rows_to_other_parts(acs_sim* s, uint32_t r, int p, uint64_t off, uint64_t n, hipStream_t q) {
    const uint32_t o = (r + 1) & 1u;
    const double* src = p == 0 ? s->x[o] : s->parts[p - 1].x[o];
    for (int t = 0; t < s->nranks; ++t) {
        if (t == p) continue;
        double* dst = t == 0 ? s->x[o] : s->parts[t - 1].x[o];
        HIP_TRY(hipMemcpyAsync(xat(s, dst, off), xat(s, src, off), n * s->es, hipMemcpyDeviceToDevice, q));
    }
    return ACS_OK;
}

// Virtual partitions: the partial slots up to the last partition that has rows (an empty tail
// partition's partials are not folded).
static uint32_t nblk_live(const acs_sim* s) {
    uint32_t n = 0;
    for (int p = 0; p < s->nranks; ++p)
        if (part_rows(s, p)) n = (uint32_t)((p + 1) * s->nblk);
    return n;
}

// A real partition's verdict of round r on stream q: fold this rank's partials into (-min, max),
// all-reduce the pair (reduce: the communicator has peers, or the sequence always reduces), verdict.
static int fold_allreduce_verdict(acs_sim* s, uint32_t r, bool reduce, hipStream_t q) {
    FinalizeArgs fold = make_finalize(s, r + 1, s->partial, part_rows(s, s->rank) ? s->nblk : 0, false);
    fold.fold_out = s->gpart;
    HIP_TRY(launch_finalize(fold, s->B, q));
    if (reduce) NCCL_TRY(ncclAllReduce(s->gpart, s->gpart, 2, ncclFloat64, ncclMax, s->comm, q));
    FinalizeArgs fin = make_finalize(s, r + 1, s->gpart, 1, false);
    fin.negmin = 1;
    HIP_TRY(launch_finalize(fin, s->B, q));
    return ACS_OK;
}

// Chunked node-partitioned round on the binned path.  Compute stream: phase A by
// source-block chunk (chunk k of every rank, after round r-1's exchange of chunk k), phase M, then
// phase B by receiver-block chunk (after round r-1's verdict, so a finished run's phase B exits).
// Comm stream: each chunk's exchange as soon as its phase B is done (RCCL grouped send / recv to
// every peer over xGMI, or device copies between virtual partitions), then the spread fold,
// all-reduce and verdict.  Phase A / M of round r+1 may run before round r's verdict: they only
// write the stage, and phase B (the only writer of x) waits for the verdict.
static int enqueue_round_xchunked(acs_sim* s, uint32_t r) {
    const RoundArgs a = round_args(s, r);
    const uint32_t K = s->xchunks;
    const uint64_t cs = s->rows_per / K;
    const uint32_t SA = s->bin_sa;
    const uint32_t bpr = (uint32_t)(s->rows_per / SA), bpc = (uint32_t)(cs / SA);
    const uint32_t qpc = (uint32_t)(cs / s->bin.SB);   // phase-B receiver blocks per chunk
    const int nparts = s->virt ? s->nranks : 1;
    auto pargs = [&](int p) { return part_args(s, a, s->virt ? p : s->rank, r); };
    auto plan = [&](int p) -> const BinnedPlan& { return (s->virt && p > 0) ? s->parts[p - 1].bin : s->bin; };
    hipEvent_t e1;
    int rc = timing_begin(s, &e1);
    if (rc) return rc;
    for (uint32_t k = 0; k < K; ++k) {
        HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_x[k], 0));
        for (int p = 0; p < nparts; ++p)
            if (pargs(p).nrows)
                HIP_TRY(launch_round_binned(plan(p), pargs(p), s->clean, s->stream, nullptr, 1u,
                                            SrcSel{(uint32_t)s->nranks * bpc, bpr, bpc, k * bpc}));
    }
    for (int p = 0; p < nparts; ++p)
        if (pargs(p).nrows) HIP_TRY(launch_round_binned(plan(p), pargs(p), s->clean, s->stream, nullptr, 2u));
    HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_fin, 0));
    const ncclDataType_t dt = s->f32 ? ncclFloat32 : ncclFloat64;
    for (uint32_t k = 0; k < K; ++k) {
        for (int p = 0; p < nparts; ++p) {
            RoundArgs ap = pargs(p);
            if (!ap.nrows) continue;
            ap.qlo = k * qpc;
            ap.qhi = k + 1 == K ? 0xFFFFFFFFu : (k + 1) * qpc;
            HIP_TRY(launch_round_binned(plan(p), ap, s->clean, s->stream, nullptr, 4u));
        }
        HIP_TRY(hipEventRecord(s->ev_b[k], s->stream));
        HIP_TRY(hipStreamWaitEvent(s->cstream, s->ev_b[k], 0));
        if (s->virt) {   // chunk k of every partition into every other partition's copy
            for (int p = 0; p < s->nranks; ++p)
                if (const uint64_t n = chunk_rows(s, p, k))
                    if (int rc2 = copy_rows_to_other_parts(s, r, p, part_row0(s, p) + (uint64_t)k * cs, n, s->cstream))
                        return rc2;
        } else if (s->nranks > 1) {
            double* xo = s->x[(r + 1) & 1u];
            NCCL_TRY(ncclGroupStart());
            for (int q = 0; q < s->nranks; ++q) {
                if (q == s->rank) continue;
                const uint64_t mine = chunk_rows(s, s->rank, k), theirs = chunk_rows(s, q, k);
                if (mine)
                    NCCL_TRY(ncclSend(xat(s, xo, part_row0(s, s->rank) + (uint64_t)k * cs), mine, dt, q, s->comm,
                                      s->cstream));
                if (theirs)
                    NCCL_TRY(ncclRecv(xat(s, xo, part_row0(s, q) + (uint64_t)k * cs), theirs, dt, q, s->comm,
                                      s->cstream));
            }
            NCCL_TRY(ncclGroupEnd());
        }
        HIP_TRY(hipEventRecord(s->ev_x[k], s->cstream));
    }
    if (e1) HIP_TRY(hipEventRecord(e1, s->stream));
    // verdict of round r on the comm stream (it has waited for every phase-B chunk)
    if (s->virt)
        HIP_TRY(launch_finalize(make_finalize(s, r + 1, s->partial, nblk_live(s), false), s->B, s->cstream));
    else if (int rc2 = fold_allreduce_verdict(s, r, s->nranks > 1, s->cstream))
        return rc2;
    HIP_TRY(hipEventRecord(s->ev_fin, s->cstream));
    return ACS_OK;
}

// One round x^r -> x^{r+1}: round kernel(s), [exchange], spread finalize.
static int enqueue_round(acs_sim* s, uint32_t r) {
    if (s->xchunks) return enqueue_round_xchunked(s, r);
    RoundArgs a = round_args(s, r);
    hipEvent_t e1;
    int rc = timing_begin(s, &e1);
    if (rc) return rc;
    // EPS verdict publication: phase B of round r folds its exact (min, max) into
    // eacc[(r + 1) & 1], so every workgroup of round r + 1's phase A can stop on convergence
    // (without it only workgroup 0 folds the partials and the others stream one last round).
    // Invariant: EVERY kernel that writes a.partial in such a round must also publish into ab.eacc
    // (block_minmax_store(..., a.eacc)): k_bin_gather in all its forms (NP = 1 .. 4, VAR, FIX,
    // FAULTY, the narrow NAR kernels and the 128- / 512-receiver blocks: every row of kGatherTable,
    // binned_select.hpp) and rule WEIGHTED's k_bin_gather_w (round_binned_w.hip).  A writer that
    // skipped it would not crash: phase A's other
    // workgroups would stop on a stale verdict while workgroup 0 streams.  Hub rows (generic
    // kernel partials) and partitioned rounds are therefore excluded here;
    // tests/test_gpu_binned.py::test_eps_publication_in_every_gather_variant covers each form.
    // Narrow plans publish in every round, whatever the termination: the next phase A chooses its
    // stage width and base from the pair, so there publication is needed for correct values, not
    // only for the early stop.
    unsigned long long* pub = s->eacc && s->binned && s->defer_fin && !s->n_hub && !s->partitioned &&
                                      (s->c.termination == ACS_TERM_EPS || s->bin.narrow)
                                  ? s->eacc + kEaccWords * ((r + 1) & 1u)
                                  : nullptr;
    if (!s->partitioned) {
        if (s->binned) {
            RoundArgs ab = a;
            ab.eacc = pub;
            if (s->n_hub) ab.qhi = s->nblk_fast;   // the hub rows' partial slots are the generic kernel's
            HIP_TRY(launch_round_binned(s->bin, ab, s->clean, s->stream, s->fin_pending ? &s->fin_args : nullptr));
            s->fin_pending = false;
        } else if (s->path == PATH_REGULAR && s->split) {
            HIP_TRY(launch_round_pushsum_split(a, s->B, s->nblk_fast, s->stream));
        } else if (s->path == PATH_REGULAR && s->pushsum) {
            HIP_TRY(launch_round_pushsum(a, s->hold, s->B, s->nblk_fast, s->stream));
        } else if (s->path == PATH_REGULAR && s->weighted) {
            HIP_TRY(launch_round_weighted(a, s->B, s->nblk_fast, s->stream));
        } else if (s->path == PATH_REGULAR) {
            HIP_TRY(launch_round_regular(a, s->B, s->clean, s->stream));
        } else if (s->path == PATH_DENSE) {
            DenseArgs d{};
            d.x = a.xin;
            d.xo = a.xout;
            d.status = s->status;
            d.st = s->st;
            d.partial = s->partial;
            d.sorted = s->dsorted;
            d.counts = s->dcounts;
            d.N = (uint32_t)s->N;
            uint32_t P = 1;
            while (P < s->N) P <<= 1;
            d.P = P;
            d.r = r;
            d.rule = s->c.rule;
            d.trim = s->c.trim;
            d.byz = s->c.byz_strategy;
            d.delta = s->mp.delta;
            d.bconst = s->mp.bconst;
            d.f32 = s->f32 ? 1u : 0u;
            HIP_TRY(launch_round_dense(d, s->stream));
        } else if (s->c.topology != ACS_TOPO_CSR) {   // complete / regular graphs: one size for all
            if (s->generic_small) HIP_TRY(launch_round_generic(a, s->B, s->stream));
            HIP_TRY(launch_round_generic_big(s->big, a, s->B, s->stream));
        }
        if (s->c.topology == ACS_TOPO_CSR && (s->path == PATH_GENERIC || s->n_hub)) {
            // CSR rows on the generic kernels (every row, or the hub rows after the fast path):
            // by size class, then the rows above kGenericMaxM on the big-m path
            for (const auto& c : s->gcls) {
                RoundArgs ah = a;
                ah.rid = s->gen_ids + c.off;
                ah.pbase = s->gen_base + (uint32_t)c.off;
                HIP_TRY(launch_round_generic(ah, s->B, s->stream, c.n, c.P));
            }
            HIP_TRY(launch_round_generic_big(s->big, a, s->B, s->stream));
        }
        if (e1) HIP_TRY(hipEventRecord(e1, s->stream));
        const FinalizeArgs fin = make_finalize(s, r + 1, s->partial, s->nblk, false);
        if (s->defer_fin) {   // folded by the next round's phase A, or by flush_finalize
            s->fin_args = fin;
            s->fin_args.eacc = pub;
            s->fin_pending = true;
            return ACS_OK;
        }
        HIP_TRY(launch_finalize(fin, s->B, s->stream));
        return ACS_OK;
    }
    if (s->virt) {
        // every partition p reads its own full copy, writes its own rows; block partials of
        // partition p land at partial[p * nblk]
        for (int p = 0; p < s->nranks; ++p) {
            const RoundArgs ap = part_args(s, a, p, r);
            if (ap.nrows == 0) continue;   // empty tail partition (its partials are not folded)
            if (s->binned)
                HIP_TRY(launch_round_binned(p == 0 ? s->bin : s->parts[p - 1].bin, ap, s->clean, s->stream));
            else
                HIP_TRY(launch_round_regular(ap, s->B, s->clean, s->stream));
        }
        if (e1) HIP_TRY(hipEventRecord(e1, s->stream));
        // all-gather emulation: copy each partition's fresh rows into every other copy
        for (int p = 0; p < s->nranks; ++p)
            if (const uint64_t nr = part_rows(s, p))
                if (int rc2 = copy_rows_to_other_parts(s, r, p, part_row0(s, p), nr, s->stream)) return rc2;
        HIP_TRY(launch_finalize(make_finalize(s, r + 1, s->partial, nblk_live(s), false), s->B, s->stream));
        return ACS_OK;
    }
    // RCCL partition: own rows, then in-place all-gather of x^{r+1} and all-reduce of the spread
    a = part_args(s, a, s->rank, r);
    if (a.nrows) {
        if (s->binned)
            HIP_TRY(launch_round_binned(s->bin, a, s->clean, s->stream));
        else
            HIP_TRY(launch_round_regular(a, s->B, s->clean, s->stream));
    }
    if (e1) HIP_TRY(hipEventRecord(e1, s->stream));
    double* xo = s->x[(r + 1) & 1u];
    NCCL_TRY(ncclAllGather(xat(s, xo, a.row0), xo, s->rows_per, s->f32 ? ncclFloat32 : ncclFloat64, s->comm,
                           s->stream));
    return fold_allreduce_verdict(s, r, true, s->stream);
}

// Poll a host-mapped sequence number a launch on s->stream releases at system scope.  The stream is
// queried every 256 spins, so a failed launch returns its error rather than spinning forever.
// patient: the wait may span a whole chunk of long rounds (EPS chunk verdicts of large graphs,
// milliseconds each): after 100 us of spinning the host yields the core between polls
// (sched_yield), so ranks and threads sharing the box's cores run meanwhile, without adding the
// wake-up latency of a sleep (a 20 us sleep_for, with the kernel's default timer slack, added
// ≈ 60 us to every cfg4 EPS run: profiles/r06_eps_yield_configs.jsonl).  The short call-end reads
// spin throughout (their wait is a few microseconds).
static int wait_mapped_seq(acs_sim* s, const unsigned long long* p, unsigned long long seq, const char* what,
                           bool patient = false) {
    const auto t0 = std::chrono::steady_clock::now();
    bool yielding = false;
    for (uint32_t it = 1;; ++it) {
        if (__atomic_load_n(p, __ATOMIC_ACQUIRE) == seq) return ACS_OK;
        if ((it & 255u) == 0) {
            const hipError_t q = hipStreamQuery(s->stream);
            if (q == hipSuccess) {
                if (__atomic_load_n(p, __ATOMIC_ACQUIRE) == seq) return ACS_OK;
                return fail(ACS_EDEVICE, "%s: stream idle without the sequence number", what);
            }
            if (q != hipErrorNotReady) return fail(ACS_EDEVICE, "%s: %s", what, hipGetErrorString(q));
            if (patient && !yielding && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(100))
                yielding = true;
        }
        if (yielding)
            std::this_thread::yield();
        else
            __builtin_ia32_pause();
    }
}

// The B instance states after everything enqueued so far.  Handles of at most kMappedStates
// instances take them through host-mapped memory (launch_states_mapped: no device-to-host copy,
// no wait on the stream's completion signal); the stream may still be retiring that small launch
// on return, and later work stays ordered behind it.
static int fetch_mapped_states(acs_sim* s, bool patient = false) {
    const unsigned long long seq = ++s->ms_seq;
    HIP_TRY(launch_states_mapped(s->st, s->n_done, (uint32_t)s->B, s->h_ms_dev, seq, s->stream));
    return wait_mapped_seq(s, &s->h_ms->seq, seq, "instance states", patient);
}

// The done count after everything enqueued so far (EPS chunks and call ends): through the mapped
// states where the handle has them (which then hold the states of that moment too).  patient: a
// chunk verdict behind a chunk of long rounds (wait_mapped_seq).
static int fetch_done_count(acs_sim* s, uint32_t& nd, bool patient = false) {
    if (s->h_ms) {
        if (int rc = fetch_mapped_states(s, patient)) return rc;
        nd = s->h_ms->n_done;
        return ACS_OK;
    }
    HIP_TRY(hipMemcpyAsync(s->h_ndone, s->n_done, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    nd = s->h_ndone[0];
    return ACS_OK;
}

int read_states(acs_sim* s, std::vector<InstState>& out, bool reuse_fresh) {
    out.resize(s->B);
    if (s->h_ms) {
        if (!(reuse_fresh && s->ms_fresh))
            if (int rc = fetch_mapped_states(s)) return rc;
        s->ms_fresh = false;
        memcpy(out.data(), s->h_ms->st, s->B * sizeof(InstState));
        return ACS_OK;
    }
    HIP_TRY(hipMemcpyAsync(out.data(), s->st, s->B * sizeof(InstState), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ACS_OK;
}

static constexpr uint32_t kChunk = 16;

// Enqueue the one-launch run summary and wait for it by polling its host-mapped sequence number
// instead of the stream's completion signal (the wake-up after that signal cost ≈ 6 µs per run on
// a 12 500-instance cfg3 shard).  The stream is queried every 256 spins, so a failed
// launch returns its error rather than spinning forever.  On return the summary's fields are
// valid; later stream work stays ordered behind the (finishing) summary kernel.
int summary_and_wait(acs_sim* s) {
    const unsigned long long seq = ++s->sum_seq;
    HIP_TRY(launch_run_summary_mapped(s->st, s->B, s->sum_scratch, s->h_sum_dev, seq, s->stream));
    return wait_mapped_seq(s, &s->h_sum->seq, seq, "run summary");
}

// Launch a finalize still deferred (the last round enqueued has no next phase A to fold it).
static int flush_finalize(acs_sim* s) {
    if (!s->fin_pending) return ACS_OK;
    s->fin_pending = false;
    HIP_TRY(launch_finalize(s->fin_args, s->B, s->stream));
    return ACS_OK;
}

// Advance every unfinished instance by at most k rounds.
int advance(acs_sim* s, uint32_t k) {
    s->ms_fresh = false;
    if (s->all_done || k == 0) return ACS_OK;
    const uint32_t cap = s->c.max_rounds > s->round ? s->c.max_rounds - s->round : 0;
    if (k > cap) k = cap;
    if (k == 0) return ACS_OK;
    if (s->path == PATH_BATCHED || s->dense_persist) {
        BatchArgs a{};
        a.x0 = s->x[0];
        a.x1 = s->x[1];
        a.status = s->status;
        a.st = s->st;
        a.trace = s->trace;
        a.trace_stride = (uint64_t)s->c.max_rounds + 1;
        a.n_done = s->n_done;
        a.N = (uint32_t)s->N;
        a.rule = s->c.rule;
        a.trim = s->c.trim;
        a.max_rounds = s->c.max_rounds;
        a.term_eps = s->c.termination == ACS_TERM_EPS;
        a.eps = s->c.eps;
        a.mp = s->mp;
        a.f32 = s->f32 ? 1u : 0u;
        hipEvent_t e1;
        int rc = timing_begin(s, &e1);
        if (rc) return rc;
        RoctxRange range(s->dense_persist ? "acs: persistent dense rounds" : "acs: batched rounds");
        if (s->dense_persist)
            HIP_TRY(launch_dense_persist(a, s->B, k, s->stream));
        else if (s->mfma)
            HIP_TRY(launch_batched_mfma(a, s->B, k, s->stream));
        else
            HIP_TRY(launch_batched_small(a, s->B, k, s->stream));
        if (e1) HIP_TRY(hipEventRecord(e1, s->stream));
        if (int rc2 = timing_close(s)) return rc2;   // (run mode: one launch per call)
        // The done count (and, for acs_run, the result summary) ride on the same synchronisation,
        // folded from the instances' done flags in one launch that writes host memory: no copies
        // (each costs a DMA round trip) and no per-instance atomic on one counter (the batched
        // kernels' last generation finished together and serialised on it), DESIGN.md §6
        if (int rc2 = summary_and_wait(s)) return rc2;
        s->summary_ready = s->want_summary;
        s->round += k;
        s->h_ndone[0] = s->h_sum->n_done;
        s->all_done = s->h_ndone[0] == s->B;
        return ACS_OK;
    }
    const bool eps_mode = s->c.termination == ACS_TERM_EPS;
    // FIXED runs need no verdict between chunks: the deferred finalize of a chunk's last round is
    // folded by the next chunk's first phase A like any other, and one standalone finalize closes
    // the call (round 5: one 4.7 µs k_finalize per 16 rounds fewer)
    const bool chunk_flush = eps_mode || s->partitioned;
    // Long rounds (a chunk of them takes milliseconds): wait for each chunk's verdict before
    // enqueuing the next, so no chunk of no-op launches follows convergence (the host wake-up is
    // < 1 % of a chunk).  Short rounds keep one chunk in flight and poll the previous one.
    const bool sync_poll = eps_mode && s->N * (uint64_t)(s->d ? s->d : s->m) * s->B >= (1ull << 22);
    int slot = 0, prev = -1;
    hipEvent_t poll[2] = {nullptr, nullptr};
    while (k > 0 && !s->all_done) {
        const uint32_t chunk = k < kChunk ? k : kChunk;
        RoctxRange range("acs: round chunk (enqueue)");
        for (uint32_t q = 0; q < chunk; ++q) {
            int rc = enqueue_round(s, s->round + q);
            if (rc) return rc;
        }
        if (chunk_flush)
            if (int rc = flush_finalize(s)) return rc;
        if (s->xchunks) HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_fin, 0));   // verdicts land on cstream
        s->round += chunk;
        k -= chunk;
        if (s->round >= s->c.max_rounds) break;
        if (sync_poll && k > 0) {
            uint32_t nd = 0;
            if (int rc = fetch_done_count(s, nd, true)) return rc;
            if (nd == s->B) s->all_done = true;
        } else if (eps_mode && !sync_poll) {
            // keep one chunk in flight: poll the previous chunk's done counter
            HIP_TRY(hipMemcpyAsync(s->h_ndone + slot, s->n_done, sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   s->stream));
            if (!poll[slot]) HIP_TRY(hipEventCreateWithFlags(&poll[slot], hipEventDisableTiming));
            HIP_TRY(hipEventRecord(poll[slot], s->stream));
            if (prev >= 0) {
                HIP_TRY(hipEventSynchronize(poll[prev]));
                if (s->h_ndone[prev] == s->B) s->all_done = true;
            }
            prev = slot;
            slot ^= 1;
        }
    }
    for (hipEvent_t e : poll)
        if (e) (void)hipEventDestroy(e);
    if (int rc = flush_finalize(s)) return rc;   // (FIXED: the call's last round)
    if (s->run_end)   // a timing run cut short by the end of this call
        if (int rc = timing_close(s)) return rc;
    if (!eps_mode) {
        // FIXED: every instance is done exactly at max_rounds, so no device round trip is needed
        // here (acs_round's state read and acs_run's summary synchronise the stream anyway)
        s->all_done = s->round >= s->c.max_rounds;
        return ACS_OK;
    }
    if (s->want_summary) {   // acs_run: the summary carries the done count (one round trip, not two)
        if (int rc = summary_and_wait(s)) return rc;
        s->summary_ready = true;
        s->all_done = s->h_sum->n_done == s->B;
        return ACS_OK;
    }
    uint32_t nd = 0;
    if (int rc = fetch_done_count(s, nd)) return rc;
    s->ms_fresh = s->h_ms != nullptr;   // nothing is enqueued after it: acs_round reuses these states
    s->all_done = nd == s->B;
    return ACS_OK;
}
