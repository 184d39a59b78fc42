"""numpy restatement of quantized messages ("Quantized messages").  TEST INFRASTRUCTURE.

A subclass of spec_weighted_np.NpWeightedSim (and, with a link schedule, of spec_sched_np's mixin):
the weights, the entry list, the drops and the schedule's down test are the parents'; the quantizer
and the row update are restated here, from the spec:

    Q(x; b, r, i):  u = x * 2^k
                    deterministic   n = rint(u)                        half to even
                    dithered        f = floor(u), g = u - f, thr = uint32(g * 2^32) by truncation
                                    n = f + (draw(QUANT, b, r, i) < thr ? 1 : 0)
                    q = n * 2^-k + 0.0
    q^r_j = Q(x^r_j; b, r, j) is what node j transmits in round r; b is the global instance id (the
    draw is per instance, not per mask group)
    sender entries are q^r_j; entry 0 is e0 = x_i (partial) or q^r_i (total, compensated)
    a missing entry takes e0 and keeps its weight (SELF) or adds +0.0 to both sums (OMIT)
    y = tree_sum(p) / tree_sum(w) with p_e = (w_e * v_e) + 0.0, as rule "weighted"
    x_i' = y (partial, total) or y + (x_i - q^r_i) (compensated); a zero weight sum keeps x_i

Every quantizer step is exact in the value type, so numpy's float arithmetic restates it bit for
bit.  The parents' `_values` is called with q in place of x: it returns q[j] for a delivered entry
and marks the missing ones, which (with the self entries) are then set to e0.
"""
from __future__ import annotations

import numpy as np

import spec_np as S
from spec_sched_np import ScheduleMixin
from spec_weighted_np import NpWeightedSim

QUANT = 8   # ACS_STREAM_QUANT
MODES = ("partial", "total", "compensated")


def quantize_np(x, k, dither, seed, b, r):
    """Q(x; b, r, i) for every node i of one instance (x[N] of float32 or float64)."""
    ft = x.dtype.type
    u = x * ft(2.0 ** k)
    if dither:
        f = np.floor(u)
        g = u - f
        thr = (g * ft(2.0 ** 32)).astype(np.uint64)   # g < 1: below 2^32, truncated
        w = S.draw(seed, QUANT, b, r, np.arange(x.size, dtype=np.uint64)).astype(np.uint64)
        n = f + np.where(w < thr, ft(1), ft(0))
    else:
        n = np.rint(u)
    return (n * ft(2.0 ** -k) + ft(0)).astype(x.dtype)


class NpQuantWeightedSim(NpWeightedSim):
    def __init__(self, cfg, csr, weights, quant=None):
        super().__init__(cfg, csr, weights)
        quant = quant if quant is not None else self._quant_arg   # (set by the scheduled subclass)
        self.k, self.mode, self.dither = int(quant[0]), MODES.index(quant[1]), bool(quant[2])
        assert self.fault == 0 and self.D == 0
        self.q = np.empty_like(self.x)
        for lb in range(self.B):
            self._requantize(lb)

    def _requantize(self, lb):
        self.q[lb] = quantize_np(self.x[lb], self.k, self.dither, self.seed, self.gb[lb], int(self.rounds[lb]))

    def set_state(self, rnd, x):
        """acs_set_state: every instance restarts at round rnd from x[B, N]."""
        self.x[:] = np.asarray(x, dtype=self.ft).reshape(self.B, self.N) + self.ft(0)
        self.rounds[:] = rnd
        self.trace = [[] for _ in range(self.B)]
        for lb in range(self.B):
            self.hist[lb] = [self.x[lb].copy()]
            self._requantize(lb)
            self._after(lb)

    def _step(self, lb):
        cfg = self.cfg
        b = self.gb[lb]
        bG = b - b % int(cfg.mask_group)
        r = int(self.rounds[lb])
        x, q = self.x[lb], self.q[lb]
        ft = self.ft
        e0 = x if self.mode == 0 else q
        rows = self.e_row
        V, miss = self._values(rows, self.e_j[:, None], self.e_slot[:, None], self.e_self[:, None], r, b, bG, q,
                               self.status[lb], self.lo[lb], self.hi[lb])
        V, miss = V[:, 0], miss[:, 0]
        V = np.where(miss | self.e_self, e0[rows], V)
        gone = miss if self.omit else np.zeros_like(miss)
        w = np.where(gone, ft(0), self.e_w).astype(ft)
        p = np.where(gone, ft(0), (w * V).astype(ft) + ft(0)).astype(ft)
        num, den = self.row_sums(rows, self.e_pos, p), self.row_sums(rows, self.e_pos, w)
        with np.errstate(divide="ignore", invalid="ignore"):
            y = (num / den).astype(ft)
            if self.mode == 2:
                y = (y + (x - q)).astype(ft)
        self.zero_den += int(np.count_nonzero(den == 0))
        xn = np.where(den > 0, y, x)
        self.x[lb] = xn
        self.hist[lb].append(xn.copy())
        self.rounds[lb] = r + 1
        self._requantize(lb)
        self._after(lb)


class NpSchedQuantWeightedSim(ScheduleMixin, NpQuantWeightedSim):
    def __init__(self, cfg, csr, weights, quant, schedule):
        # (ScheduleMixin.__init__ passes cfg, csr and weights on: the quantizer's arguments wait here)
        self._quant_arg = quant
        ScheduleMixin.__init__(self, cfg, csr, weights, schedule)


def quant_sim(cfg, csr, weights, quant, schedule=None):
    """The restatement of Simulator(cfg, csr=csr, weights=weights, schedule=schedule, quant=quant)."""
    if schedule is None:
        return NpQuantWeightedSim(cfg, csr, weights, quant)
    return NpSchedQuantWeightedSim(cfg, csr, weights, quant, schedule)
