"""Synthetic user graphs in CSR form for the ACS_TOPO_CSR topology:
``(rowptr uint64[N+1], colidx uint32[nnz])`` as ``acsim.Simulator(cfg, csr=...)`` takes them,
and the edge weights of rules "weighted" and "pushsum" (``weights=(w_self, w_edge)``).
Used by the CSR benchmarks and tests; any CSR the caller builds works the same way."""
from __future__ import annotations

import numpy as np


def random_csr(n: int, dmin: int, dmax: int, seed: int):
    """Uniform degrees in [dmin, dmax], uniformly random senders."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(dmin, dmax + 1, size=n)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    colidx = rng.integers(0, n, size=int(rowptr[-1])).astype(np.uint32)
    return rowptr, colidx


def skewed_csr(n: int, dmin: int, dmax: int, seed: int, alpha: float = 2.0):
    """Power-law degrees in [dmin, dmax] (most rows near dmin, a tail up to dmax); senders half
    uniform, half from a hub set of n/100 nodes (skewed in-degree too)."""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    deg = np.floor(dmin * (1 - u * (1 - (dmin / (dmax + 1)) ** (alpha - 1))) ** (-1 / (alpha - 1))).astype(np.int64)
    deg = np.clip(deg, dmin, dmax)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    nnz = int(rowptr[-1])
    hubs = rng.integers(0, n, size=max(1, n // 100))
    col = np.where(rng.random(nnz) < 0.5, rng.integers(0, n, size=nnz), hubs[rng.integers(0, hubs.size, size=nnz)])
    return rowptr, col.astype(np.uint32)


# ---------------------------------------------------------------------------- .npz graph files
# user graphs arrive as `.npz` files.  Two layouts are read:
#   acsim's own      rowptr (uint64 [N+1]), colidx (uint32 [nnz])   (save_csr writes this)
#   scipy.sparse     indptr, indices, shape, format = "csr"          (scipy.sparse.save_npz of a CSR
#                    matrix whose row i lists receiver i's senders; `data` holds the edge
#                    weights, read only when weights are asked for)
# Weights (rule "weighted") are optional: acsim's layout adds w_self (float64 [N]) and
# w_edge (float64 [nnz], by slot); in the scipy layout w_edge = data and w_self = 0 (a diagonal
# entry is an ordinary self-loop message on its slot, with its own weight).
# A link schedule is optional too, in acsim's layout only: sched_period (uint32 scalar)
# and sched_avail (uint32 [nnz], by slot).
# Receiver i's senders are colidx[rowptr[i] : rowptr[i+1]] in slot order (slot = rowptr[i] + t,
# SURVEY §A.3).  Files are loaded with allow_pickle=False: a graph file executes nothing.

def save_csr(path: str, rowptr, colidx, weights=None, schedule=None) -> None:
    """Write a CSR graph in acsim's `.npz` layout (validated first); weights = (w_self, w_edge)
    are stored beside it for rule "weighted", and schedule = (period, avail) as sched_period and
    sched_avail (a link schedule, checked by check_schedule)."""
    rp, ci = check_csr(rowptr, colidx)
    extra = {}
    if weights is not None:
        ws, we = check_weights(rp, weights[0], weights[1])
        extra = {"w_self": ws, "w_edge": we}
    if schedule is not None:
        period, av = check_schedule(rp, schedule[0], schedule[1])
        extra.update(sched_period=np.array(period, dtype=np.uint32), sched_avail=av)
    np.savez(path, rowptr=rp, colidx=ci, format=np.array("acsim-csr-v1"), **extra)


def load_csr(path: str, weights: bool = False, schedule: bool = False):
    """Read a CSR graph file (acsim or scipy.sparse layout) -> (rowptr uint64[N+1], colidx uint32[nnz]).
    weights=True also returns the file's weights, (rowptr, colidx, w_self, w_edge): the arrays
    w_self / w_edge of acsim's layout, or w_edge = data and w_self = 0 for a scipy.sparse matrix;
    a file without weights is a ValueError.  schedule=True appends the file's link schedule
    (period, avail) to the result; a file without one (sched_period / sched_avail of acsim's layout)
    is a ValueError."""
    ws = we = sched = None
    with np.load(path, allow_pickle=False) as z:
        keys = set(z.files)
        if {"rowptr", "colidx"} <= keys:
            rp, ci = z["rowptr"], z["colidx"]
            if weights:
                if not {"w_self", "w_edge"} <= keys:
                    raise ValueError(f"{path}: no weights (w_self / w_edge) in {sorted(keys)}")
                ws, we = z["w_self"], z["w_edge"]
            if schedule and {"sched_period", "sched_avail"} <= keys:
                sched = (int(z["sched_period"]), z["sched_avail"])
        elif {"indptr", "indices"} <= keys:
            if "format" in keys and str(z["format"].astype(str)) != "csr":
                raise ValueError(f"{path}: scipy.sparse matrix in {z['format']!s} format; CSR expected")
            rp, ci = z["indptr"], z["indices"]
            if "shape" in keys:
                shape = tuple(int(v) for v in z["shape"])
                if shape[0] != shape[1] or shape[0] != rp.size - 1:
                    raise ValueError(f"{path}: adjacency must be N x N with N = len(indptr) - 1, got {shape}")
            if weights:
                if "data" not in keys:
                    raise ValueError(f"{path}: no weights (data) in {sorted(keys)}")
                we = z["data"]
                ws = np.zeros(rp.size - 1)
        else:
            raise ValueError(f"{path}: no CSR arrays (rowptr/colidx or indptr/indices) in {sorted(keys)}")
    rp, ci = check_csr(rp, ci)
    if schedule and sched is None:
        raise ValueError(f"{path}: no link schedule (sched_period / sched_avail) in {sorted(keys)}")
    out = (rp, ci) + (check_weights(rp, ws, we) if weights else ())
    return out + check_schedule(rp, *sched) if schedule else out


def check_weights(rowptr, w_self, w_edge):
    """Shapes and type of a weight pair for the graph `rowptr` -> (float64 [N], float64 [nnz]).  The
    value rules (finite, in [0, 1], positive row sums) belong to acs_create_csr_weighted."""
    rp = np.asarray(rowptr)
    ws = np.asarray(w_self)
    we = np.asarray(w_edge)
    for w in (ws, we):
        if not (np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer)):
            raise ValueError("weights must be real numbers")
    if ws.shape != (rp.size - 1,) or we.shape != (int(rp[-1]),):
        raise ValueError("weights must be (w_self[N], w_edge[nnz])")
    return ws.astype(np.float64), we.astype(np.float64)


# ---------------------------------------------------------------------------- link schedules
# DESIGN.md §9, "Link schedules": a period P in 1..32 and one uint32 mask per CSR slot; bit p < P of
# avail[slot] is set when the link on that slot is up in every round r with r % P == p.

SCHEDULE_MAX_PERIOD = 32


def check_schedule(rowptr, period, avail, values: bool = True):
    """Shape and type of a link schedule for the graph `rowptr` -> (int period, uint32 [nnz]).
    values=True also applies the value rules of acs_create_csr_scheduled: 1 <= period <= 32 and no
    bit of any mask at a position >= period (the first offending slot is named)."""
    rp = np.asarray(rowptr)
    av = np.asarray(avail)
    if isinstance(period, (bool, np.bool_)) or not isinstance(period, (int, np.integer)):
        raise ValueError("schedule period must be an integer")
    period = int(period)
    if not np.issubdtype(av.dtype, np.integer) or av.dtype == np.bool_:
        raise ValueError("schedule masks must be an integer array")
    if av.shape != (int(rp[-1]),):
        raise ValueError("schedule masks must be avail[nnz], one per CSR slot")
    if not 0 <= period < 1 << 32 or (av.size and (int(av.min()) < 0 or int(av.max()) >= 1 << 32)):
        raise ValueError("schedule period and masks must fit in uint32")
    av = np.ascontiguousarray(av, dtype=np.uint32)
    if values:
        if not 1 <= period <= SCHEDULE_MAX_PERIOD:
            raise ValueError(f"schedule period {period} outside 1..{SCHEDULE_MAX_PERIOD}")
        stray = np.flatnonzero(av >> np.uint32(period)) if period < 32 else np.empty(0, dtype=np.int64)
        if stray.size:
            e = int(stray[0])
            raise ValueError(f"avail[{e}] = {int(av[e]):#010x} has a bit at a position >= period {period}")
    return period, av


def full_schedule(nnz: int, period: int):
    """The schedule on which every link is up in every phase: (period, avail[nnz]) with every mask
    (1 << period) - 1.  A handle made with it equals the unscheduled handle bit for bit."""
    if not 1 <= int(period) <= SCHEDULE_MAX_PERIOD:
        raise ValueError(f"schedule period {period} outside 1..{SCHEDULE_MAX_PERIOD}")
    return int(period), np.full(int(nnz), (1 << int(period)) - 1, dtype=np.uint32)


def _mix64(v):
    """The finaliser of splitmix64 on a uint64 array (arithmetic modulo 2^64)."""
    v = np.asarray(v, dtype=np.uint64).copy()
    v ^= v >> np.uint64(30)
    v *= np.uint64(0xBF58476D1CE4E5B9)
    v ^= v >> np.uint64(27)
    v *= np.uint64(0x94D049BB133111EB)
    v ^= v >> np.uint64(31)
    return v


def phase_schedule(rowptr, colidx, period: int, seed: int = 0, symmetric: bool = False):
    """Exactly one phase per slot (TDMA-style link activation): slot e is up in the rounds r with
    r % period == phase(e) and down in all others, so its longest down streak is period - 1 rounds.
    With mix = the splitmix64 finaliser and all arithmetic modulo 2^64,
        phase(e) = mix(mix(seed + 0x9E3779B97F4A7C15) + e) % period,
    and with symmetric=True, for slot e of receiver i with sender j = colidx[e],
        phase(e) = mix(mix(mix(seed + 0x9E3779B97F4A7C15) + min(i, j)) + max(i, j)) % period,
    so both directions of an edge (and parallel edges) share a phase.  Returns (period, avail[nnz])."""
    rp, ci = check_csr(rowptr, colidx)
    if not 1 <= int(period) <= SCHEDULE_MAX_PERIOD:
        raise ValueError(f"schedule period {period} outside 1..{SCHEDULE_MAX_PERIOD}")
    period = int(period)
    s0 = _mix64(np.array([(int(seed) + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))
    if symmetric:
        rows = np.repeat(np.arange(rp.size - 1, dtype=np.uint64), np.diff(rp.astype(np.int64)))
        cols = ci.astype(np.uint64)
        h = _mix64(_mix64(s0 + np.minimum(rows, cols)) + np.maximum(rows, cols))
    else:
        h = _mix64(s0 + np.arange(ci.size, dtype=np.uint64))
    return period, (np.uint32(1) << (h % np.uint64(period)).astype(np.uint32)).astype(np.uint32)


def metropolis_weights(rowptr, colidx):
    """Metropolis-Hastings weights of a symmetric graph: w_ij = 1 / (1 + max(deg_i, deg_j)) on the
    slot of every edge and w_ii = 1 - sum_j w_ij, so W is doubly stochastic and x' = W x keeps the
    mean.  deg = entries per row.  Returns (w_self, w_edge)."""
    rp, ci = check_csr(rowptr, colidx)
    deg = np.diff(rp.astype(np.int64))
    rows = np.repeat(np.arange(deg.size), deg)
    we = 1.0 / (1.0 + np.maximum(deg[rows], deg[ci.astype(np.int64)]).astype(np.float64))
    ws = 1.0 - np.bincount(rows, weights=we, minlength=deg.size)
    return ws, we


def pushsum_weights(rowptr, colidx, dtype="f64"):
    """Push-sum weights of a directed graph (rule "pushsum"): sender j gives
    1 / (outdeg(j) + 1) to itself and to each slot it appears on (outdeg(j) = its slots in colidx), so
    every column of W sums to 1 and the mass sum(s) / sum(z) is the mean of x^0.  Where
    (outdeg + 1) times the rounded weight exceeds 1 exactly, the weight is taken one ulp lower, so
    every exact column sum is at most 1.  dtype="f32" (a Config's dtype) rounds and steps in
    binary32, for a handle that holds binary32 weights: rounding float64 weights there would push
    half the columns above 1.  Returns (w_self, w_edge) as float64."""
    rp, ci = check_csr(rowptr, colidx)
    ft, p = (np.float32, 24) if str(dtype) in ("f32", "float32") else (np.float64, 53)
    k = np.bincount(ci.astype(np.int64), minlength=rp.size - 1).astype(np.int64) + 1
    w = (ft(1) / k.astype(ft)).astype(ft)
    # k * w > 1, decided exactly in integers: w = mi * 2^(e - p) with mi = the p-bit significand
    m, e = np.frexp(w.astype(np.float64))
    mi = np.ldexp(m, p).astype(np.int64).astype(object) * k.astype(object)   # exact integers
    over = np.array([int(a) > (1 << int(p - b)) for a, b in zip(mi, e)], dtype=bool)
    w = np.where(over, np.nextafter(w, ft(0)), w).astype(np.float64)
    return w.copy(), w[ci.astype(np.int64)]


def _floor_recip(k, dtype):
    """1 / k rounded to `dtype`, one ulp lower where k times the rounded value exceeds 1 exactly
    (decided in integers), for an int64 array k >= 1; float64 values."""
    ft, p = (np.float32, 24) if str(dtype) in ("f32", "float32") else (np.float64, 53)
    uk, inv = np.unique(np.asarray(k, dtype=np.int64), return_inverse=True)
    w = (ft(1) / uk.astype(ft)).astype(ft)
    m, e = np.frexp(w.astype(np.float64))   # w = mi * 2^(e - p) with mi = the p-bit significand
    mi = np.ldexp(m, p).astype(np.int64)
    for q in range(uk.size):
        while int(mi[q]) * int(uk[q]) > 1 << int(p - e[q]):
            w[q] = np.nextafter(w[q], ft(0))
            m1, e1 = np.frexp(np.float64(w[q]))
            mi[q], e[q] = int(np.ldexp(m1, p)), e1
    return w.astype(np.float64)[inv].reshape(np.shape(k))


def split_shares(rowptr, colidx, period, avail, dtype="f64"):
    """The share table of push-sum with per-round splitting (Simulator(..., split=True)):
    share[p, j] = 1 / c_p(j) with c_p(j) = 1 + the slots of sender j that are up in phase p, rounded
    to `dtype` and taken one ulp lower where c_p(j) times the rounded share exceeds 1 exactly (the
    rule of pushsum_weights), so every round's column sums are at most 1.  Returns float64 [period, N]."""
    rp, ci = check_csr(rowptr, colidx)
    period, av = check_schedule(rp, period, avail)
    n = rp.size - 1
    c = np.ones((period, n), dtype=np.int64)
    for p in range(period):
        up = (av >> np.uint32(p)) & np.uint32(1)
        c[p] += np.bincount(ci.astype(np.int64), weights=up, minlength=n).astype(np.int64)
    return _floor_recip(c, dtype)


def quant_args(quant, dtype="f64"):
    """(k, mode, dither) of Simulator(..., quant=...) as the three integers acs_create_csr_quantized
    takes: the step is 2**-k, mode is "partial", "total" or "compensated", dither a bool."""
    from . import _abi
    try:
        k, mode, dither = quant
    except (TypeError, ValueError):
        raise ValueError("quant must be (k, mode, dither)") from None
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise ValueError("quant: k must be an integer")
    kmax = _abi.QUANT_MAX_LOG2["f32" if str(dtype) in ("f32", "float32") else "f64"]
    if not 0 <= int(k) <= kmax:
        raise ValueError(f"quant: k must be in [0, {kmax}] (dtype {dtype}): the step is 2**-k")
    if not isinstance(mode, str) or mode not in _abi.QUANT_MODES:
        raise ValueError(f"quant: mode must be one of {sorted(_abi.QUANT_MODES)}")
    if not isinstance(dither, (bool, np.bool_)):
        raise ValueError("quant: dither must be a bool")
    return int(k), _abi.QUANT_MODES[mode], int(bool(dither))


def quantize(x, k, dither=False, seed=0, instance=0, round=0, dtype=None):
    """What the nodes transmit under Simulator(..., quant=(k, mode, dither)): Q(x) on
    the grid of step 2**-k.  x[N] holds node i's state at index i; seed is the config's, instance the
    global instance id (instance_offset + local index) and round the round in which the values are
    sent.  dither False: rint(x * 2**k) * 2**-k, half to even.  dither True: floor(x * 2**k) plus one
    where draw(QUANT, instance, round, i) < uint32(frac * 2**32).  Every step is exact in x's dtype
    (float32 stays float32, everything else is float64, unless dtype says otherwise); -0.0 never
    comes out."""
    from . import _abi
    x = np.asarray(x)
    ft = np.float32 if (str(dtype) in ("f32", "float32") if dtype is not None else x.dtype == np.float32) else np.float64
    if isinstance(k, (bool, np.bool_)) or int(k) != k or not 0 <= int(k) <= _abi.QUANT_MAX_LOG2["f32" if ft is np.float32 else "f64"]:
        raise ValueError("quantize: k must be an integer in [0, 52] (float32: [0, 23])")
    x = x.astype(ft)
    if x.ndim != 1:
        raise ValueError("quantize: x must be one instance's values, x[N]")
    u = np.ldexp(x, int(k)).astype(ft)
    if dither:
        f = np.floor(u)
        thr = np.ldexp(u - f, 32).astype(np.uint64)
        w = _draw(int(seed), _abi.STREAM_QUANT, int(instance), int(round), np.arange(x.size, dtype=np.uint64))
        n = f + (w.astype(np.uint64) < thr).astype(ft)
    else:
        n = np.rint(u)
    return (np.ldexp(n, -int(k)).astype(ft) + ft(0)).astype(ft)


def _draw(seed, stream, b, r, s):
    """draw(stream, b, r, s) = philox4x32-10((s >> 2, r, b, stream), key(seed))[s & 3]
    for a uint64 array s; uint32 values."""
    m32 = np.uint64(0xFFFFFFFF)
    s = np.asarray(s, dtype=np.uint64)
    c = [s >> np.uint64(2), np.full(s.shape, r & 0xFFFFFFFF, np.uint64), np.full(s.shape, b & 0xFFFFFFFF, np.uint64),
         np.full(s.shape, stream, np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for rnd in range(10):
        if rnd:
            k0 = (k0 + np.uint64(0x9E3779B9)) & m32
            k1 = (k1 + np.uint64(0xBB67AE85)) & m32
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
    sel = (s & np.uint64(3)).astype(np.intp)
    return np.choose(sel, c).astype(np.uint32)


def column_sums(rowptr, colidx, w_self, w_edge):
    """Column sums of the weight matrix: w_self[j] plus every w_edge[slot] with colidx[slot] == j,
    each as a correctly rounded sum (math.fsum).  Rule "pushsum" needs every one <= 1 + 2^-30."""
    import math
    rp, ci = check_csr(rowptr, colidx)
    ws, we = check_weights(rp, w_self, w_edge)
    order = np.argsort(ci, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(ci.astype(np.int64), minlength=ws.size))])
    wo = we[order]
    return np.array([math.fsum([ws[j]] + wo[start[j]:start[j + 1]].tolist()) for j in range(ws.size)])


def scale_weights(w_self, w_edge):
    """Scale every weight by one power of two: 1 if the largest weight is already at most 1, else
    1 / 2^e with the smallest e that brings it to at most 1 (the library admits weights in [0, 1]).  The simulation's result does not change: a power-of-two
    factor is exact on every product and on both tree sums, and cancels in the divide (short of
    underflow, i.e. for weights above about 1e-290 after scaling).  Returns (w_self, w_edge)."""
    ws = np.asarray(w_self, dtype=np.float64)
    we = np.asarray(w_edge, dtype=np.float64)
    top = max(float(ws.max(initial=0.0)), float(we.max(initial=0.0)))
    if not np.isfinite(top) or top <= 1.0:
        return ws.copy(), we.copy()
    e = int(np.ceil(np.log2(top)))
    while np.ldexp(top, -e) > 1.0:
        e += 1
    while e > 0 and np.ldexp(top, -(e - 1)) <= 1.0:
        e -= 1
    return np.ldexp(ws, -e), np.ldexp(we, -e)


def check_csr(rowptr, colidx):
    """The ACS_TOPO_CSR admission rules that need no config (acs_create_csr re-checks them and the
    per-config m_i > 2t rule): rowptr[0] = 0, non-decreasing, rowptr[N] = nnz, sender ids < N."""
    rp = np.asarray(rowptr)
    ci = np.asarray(colidx)
    if rp.ndim != 1 or rp.size < 2 or ci.ndim != 1:
        raise ValueError("rowptr must be 1-D with N + 1 >= 2 entries, colidx 1-D")
    if not (np.issubdtype(rp.dtype, np.integer) and np.issubdtype(ci.dtype, np.integer)):
        raise ValueError("rowptr and colidx must be integer arrays")
    if rp[0] != 0 or np.any(np.diff(rp.astype(np.int64)) < 0) or int(rp[-1]) != ci.size:
        raise ValueError("rowptr must start at 0, be non-decreasing and end at len(colidx)")
    n = rp.size - 1
    if ci.size and (int(ci.min()) < 0 or int(ci.max()) >= n):
        raise ValueError(f"sender ids must lie in [0, {n})")
    if n >= 1 << 31:
        raise ValueError("at most 2^31 - 1 nodes")
    return rp.astype(np.uint64), ci.astype(np.uint32)
