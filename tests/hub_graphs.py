"""CSR graphs with hub rows in every size class of k_round_generic, and an exact one-round reference
for rules "weighted" and "pushsum".  TEST INFRASTRUCTURE (tests/test_hub_classes.py,
tests/test_gpu_hub_classes.py, tests/test_properties_csr_rules.py).

A handle of rule "weighted" or "pushsum" sends every row above 32 senders to k_round_generic, which
launches the rows by size class: m = deg + 1 entries in (32, 64], (64, 256], (256, 1024],
(1024, 4096] and (4096, 8192], on blocks of 64 (classes 64 and 256), 256 (class 1024) and 1024
threads (classes 4096 and 8192).  hub_class_graph has a hub row at both ends of every class.

exact_round recomputes one lossless, fault-free round of every row in fractions.Fraction arithmetic
from stored binary values, and check_exact_round holds a computed round against it within a bound
that follows from the operation count alone.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

SLICE = 64          # rows per SELL slice of the lane kernels
FAST_D = 32         # the lane width beside hub rows
CLASSES = (64, 256, 1024, 4096, 8192)   # k_round_generic's size classes, in entries
# sender counts on both sides of every class boundary in entries (m = deg + 1)
HUB_DEGREES = (33, 62, 63, 64, 254, 255, 256, 1022, 1023, 1024, 4094, 4095, 4096, 8190, 8191)
N_HUB_GRAPH = 650   # ten full slices and a partial one


def block_size(P):
    """The block k_round_generic runs a class of P entries on."""
    return 64 if P <= 512 else 256 if P <= 2048 else 1024


def slice_widths(rp):
    """ceil(max non-hub degree / 4) of every 64-row slice."""
    deg = np.diff(np.asarray(rp, dtype=np.int64))
    low = np.where(deg > FAST_D, 0, deg)
    return [int(-(-low[a:a + SLICE].max() // 4)) for a in range(0, deg.size, SLICE)]


def hub_rows(rp):
    return np.nonzero(np.diff(np.asarray(rp, dtype=np.int64)) > FAST_D)[0]


def hub_slots(rp):
    """A mask over the CSR slots: those of hub rows."""
    deg = np.diff(np.asarray(rp, dtype=np.int64))
    return np.repeat(deg > FAST_D, deg)


def _csr(deg, rng):
    n = deg.size
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    return rp, rng.integers(0, n, int(rp[-1])).astype(np.uint32)   # uniform senders, repeats allowed


def hub_class_graph(seed=0):
    """650 rows, nnz about 43 000.  Slice 0 holds the 15 hub rows of HUB_DEGREES among rows with no
    sender (slice width 0); slice 1 has degrees 0 .. 12 (width 3); slices 2 .. 9 have degrees 0 .. 32
    with rows of exactly 0 and 32 (width 8); the last slice has 10 rows of degrees 0 .. 20 (width 5)."""
    rng = np.random.default_rng([seed, 650])
    n = N_HUB_GRAPH
    deg = rng.integers(0, FAST_D + 1, n)
    deg[:SLICE] = 0
    deg[1 + 4 * np.arange(len(HUB_DEGREES))] = rng.permutation(HUB_DEGREES)
    deg[SLICE:2 * SLICE] = rng.integers(0, 13, SLICE)
    deg[SLICE + 5] = 12
    for a in range(2 * SLICE, 10 * SLICE, SLICE):
        deg[a + 3], deg[a + 40] = FAST_D, 0
    deg[10 * SLICE:] = rng.integers(0, 21, n - 10 * SLICE)
    deg[n - 2] = 20
    rp, ci = _csr(deg, rng)
    check_hub_class_graph(rp, ci)
    return rp, ci


def check_hub_class_graph(rp, ci):
    """The conditions hub_class_graph is built for; returns {class: block size} of the classes reached."""
    deg = np.diff(rp.astype(np.int64))
    n = deg.size
    hubs = deg[deg > FAST_D]
    assert 600 <= n <= 680 and n % SLICE != 0                     # about 640 nodes, a partial last slice
    assert 0 < hubs.size * 4 <= n                                 # the handle keeps its fast path
    assert set(HUB_DEGREES) <= set(hubs.tolist())
    low = deg[deg <= FAST_D]
    assert low.min() == 0 and low.max() == FAST_D                 # non-hub rows of exactly 0 and 32 senders
    m = hubs + 1
    assert m.max() == CLASSES[-1]                                 # m = 8192 is present, nothing above it
    reached = {}
    for below, P in zip((FAST_D + 1,) + CLASSES[:-1], CLASSES):
        assert below + 1 in m and P in m, (below, P)              # just above the boundary, and at the next
        reached[P] = block_size(P)
    assert set(reached.values()) == {64, 256, 1024}               # every block size
    w = slice_widths(rp)
    assert 0 in w and 8 in w and any(1 <= v <= 7 for v in w) and max(w) == 8, w
    assert ci.size == int(rp[-1]) and ci.max() < n
    return reached


def heard_hub_graph(seed=0):
    """hub_class_graph with one sender given to every row that had none: with positive weights every
    x_i then moves and the spread can fall to eps."""
    rp, ci = hub_class_graph(seed)
    n = rp.size - 1
    deg = np.diff(rp.astype(np.int64))
    rng = np.random.default_rng([seed, 651])
    rows = [ci[int(rp[i]):int(rp[i + 1])] if deg[i] else rng.integers(0, n, 1).astype(np.uint32) for i in range(n)]
    rp2 = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.uint64)
    assert np.diff(rp2.astype(np.int64)).min() == 1
    return rp2, np.concatenate(rows).astype(np.uint32)


def admission_graph(n_hubs, n=256, seed=3):
    """n rows of degrees 0 .. 32 with n_hubs hub rows of 33 .. 300 senders (classes 64, 256 and 1024):
    n_hubs * 4 <= n keeps the lane kernel beside k_round_generic, one more hub row does not."""
    rng = np.random.default_rng([seed, n])
    deg = rng.integers(0, FAST_D + 1, n)
    at = rng.permutation(n)[:n_hubs]
    deg[at] = rng.integers(FAST_D + 1, 71, n_hubs)
    deg[at[:3]] = [FAST_D + 1, 255, 300]
    rp, ci = _csr(deg, rng)
    assert hub_rows(rp).size == n_hubs
    return rp, ci


def positive_weights(rp, seed):
    """Rule "weighted": every weight in [0.25, 1), so every row moves towards its senders."""
    rng = np.random.default_rng(seed)
    return 0.25 + 0.75 * rng.random(rp.size - 1), 0.25 + 0.75 * rng.random(int(rp[-1]))


# ----------------------------------------------------------------------------- one exact round
UNIT = {"f64": Fraction(1, 2 ** 53), "f32": Fraction(1, 2 ** 24)}


def _fr(a):
    return [Fraction(v) for v in np.asarray(a, dtype=np.float64).tolist()]


def sim_state(n, lb=0):
    """The state of instance lb of a restatement, as exact_round and check_exact_round take it."""
    st = dict(x=n.x[lb].copy())
    for key in ("s", "z"):
        if hasattr(n, key):
            st[key] = getattr(n, key)[lb].copy()
    for key in ("h", "k"):
        if hasattr(n, key):
            st[key] = getattr(n, key)[lb, n.N:].copy()
    return st


def handle_state(got, lb=0):
    """The same from test_link_schedule.read_all of a handle."""
    return {key: got[key][lb].copy() for key in ("x", "s", "z", "h", "k") if key in got}


def exact_round(rule, policy, csr, weights, schedule, r, state, dtype):
    """Round index r of a lossless, fault-free, undelayed run from `state`, every row in Fractions.

    Inputs are the stored binary values of the state and the weights rounded to the config dtype,
    each taken exactly.  A slot is down in round r when its schedule mask lacks bit r % period.
      weighted  x_i' = sum_e w_e v_e / sum_e w_e over entry 0 (w_self[i], x_i) and the slots of row i;
                a down slot's entry takes x_i and keeps its weight (SELF) or leaves both sums (OMIT);
                a zero weight sum keeps x_i
      pushsum   s_i' = w_self[i] s_i + sum over up slots of (h_e + w_e s_j), z_i' likewise, x_i' =
                s_i' / z_i' or x_i where z_i' = 0; h = k = 0 under OMIT; under HOLD an up slot's link
                becomes 0 and a down slot's link becomes (h_e + w_e s_j, k_e + w_e z_j)
    -> dict of lists of Fractions (x, and s, z, h, k for pushsum); `keep` marks rows that keep x_i."""
    ft = np.float32 if dtype == "f32" else np.float64
    rp = np.asarray(csr[0], dtype=np.int64).tolist()
    ci = np.asarray(csr[1], dtype=np.int64).tolist()
    n, nnz = len(rp) - 1, len(ci)
    ws = _fr(np.asarray(weights[0], dtype=np.float64).astype(ft))
    we = _fr(np.asarray(weights[1], dtype=np.float64).astype(ft))
    if schedule is None:
        up = [True] * nnz
    else:
        up = ((np.asarray(schedule[1], dtype=np.uint32) >> np.uint32(r % int(schedule[0]))) & np.uint32(1)).astype(bool).tolist()
    x = _fr(state["x"])
    out = dict(x=[None] * n, keep=[False] * n)
    if rule == "weighted":
        assert policy in ("self", "omit")
        for i in range(n):
            num, den = ws[i] * x[i], ws[i]
            for e in range(rp[i], rp[i + 1]):
                if up[e]:
                    num += we[e] * x[ci[e]]
                    den += we[e]
                elif policy == "self":
                    num += we[e] * x[i]
                    den += we[e]
            out["keep"][i] = den == 0
            out["x"][i] = x[i] if den == 0 else num / den
        return out
    assert rule == "pushsum" and policy in ("omit", "hold")
    hold = policy == "hold"
    s, z = _fr(state["s"]), _fr(state["z"])
    h = _fr(state["h"]) if hold else [Fraction(0)] * nnz
    k = _fr(state["k"]) if hold else [Fraction(0)] * nnz
    out.update(s=[None] * n, z=[None] * n, h=[Fraction(0)] * nnz, k=[Fraction(0)] * nnz)
    for i in range(n):
        sn, zn = ws[i] * s[i], ws[i] * z[i]
        for e in range(rp[i], rp[i + 1]):
            j = ci[e]
            hn, kn = h[e] + we[e] * s[j], k[e] + we[e] * z[j]
            if up[e]:
                sn += hn
                zn += kn
            elif hold:
                out["h"][e], out["k"][e] = hn, kn
        out["s"][i], out["z"][i] = sn, zn
        out["keep"][i] = zn == 0
        out["x"][i] = x[i] if zn == 0 else sn / zn
    return out


def check_exact_round(rule, policy, csr, weights, schedule, r, before, after, dtype):
    """A computed round (state `before` -> state `after`, round index r) against exact_round.

    The bound, from the operation count alone.  Every summand is non-negative (x^0 >= 0, weights >= 0:
    asserted), so every rounding error is relative to the exact sum of the terms below it.  With
    u = 2^-53 (f64) or 2^-24 (f32), L = log2(P_i), P_i the power of two >= deg(i) + 1, to first order
    in u:
      a product is rounded once and a stride-halving tree over P_i leaves adds L levels of one
      rounding each: a tree sum of rounded products is within (L + 1) u of the exact sum;
      weighted   num within (L + 1) u, den (weights, no product) within L u, one divide:
                 x' within (2 L + 3) u, which allows one u more than the count;
      pushsum    s' and z' within (L + 2) u each (one u above the count), one more u under HOLD for
                 h + a; x' = s' / z' within the sum of the two plus one u for the divide;
      links      a down slot's h + a is a rounded product and one add: within 2 u + u^2, exactly; an
                 up slot's link is +0.0.
    A row that keeps x_i (zero weight sum, z' = 0) must hold x_i's bits, and an exact 0 must be 0: a
    sum of non-negative floating-point terms is 0 exactly when every term is.  Nothing here is
    subnormal (asserted on the inputs: non-zero values and weights are at least 2^-60, so binary32
    products stay above 2^-120).
    -> {quantity: worst error / bound}; asserts every ratio <= 1."""
    u = UNIT[dtype]
    deg = np.diff(np.asarray(csr[0], dtype=np.int64)).tolist()
    n = len(deg)
    for key, a in list(before.items()) + [("w_self", weights[0]), ("w_edge", weights[1])]:
        a = np.asarray(a, dtype=np.float64)
        assert np.all(a >= 0), key
        assert not a[a > 0].size or a[a > 0].min() >= 2.0 ** -60, key
    want = exact_round(rule, policy, csr, weights, schedule, r, before, dtype)
    hold = policy == "hold"
    worst = {}

    def hold_to(key, got, exact, bound):
        if bound == 0 or exact == 0:
            assert got == exact, (key, got, exact)
            return
        ratio = abs(got - exact) / (bound * exact)
        worst[key] = max(worst.get(key, Fraction(0)), ratio)

    ax, bx = _fr(after["x"]), _fr(before["x"])
    if rule == "pushsum":
        as_, az = _fr(after["s"]), _fr(after["z"])
    for i in range(n):
        L = deg[i].bit_length()   # 2^L is the power of two >= deg + 1
        if rule == "weighted":
            bound = (2 * L + 3) * u
        else:
            part = (L + 2 + hold) * u
            hold_to("s", as_[i], want["s"][i], part)
            hold_to("z", az[i], want["z"][i], part)
            bound = 2 * part + u
        if want["keep"][i]:
            assert ax[i] == bx[i], ("kept", i)
        else:
            hold_to("x", ax[i], want["x"][i], bound)
    if hold:
        for key in ("h", "k"):
            for got, exact in zip(_fr(after[key]), want[key]):
                hold_to(key, got, exact, 2 * u + u * u)
    out = {key: float(v) for key, v in worst.items()}
    assert all(v <= 1 for v in worst.values()), out
    return out
