"""numpy restatement of link schedules ("Link schedules").  TEST INFRASTRUCTURE.

A mixin over the restatements of rules "weighted" and "pushsum" (spec_weighted_np, spec_pushsum_np,
spec_pushsum_hold_np).  A schedule is a period P and one uint32 mask per CSR slot; bit p of
avail[e] is set when slot e is up in every round r with r % P == p.  The spec, restated:

    a message on a slot that is down in round r is missing, exactly as a dropped one

Only the resolution of missing entries (spec_np.NpSim._values) is overridden: after the parent has
resolved crashes, drops, delays and Byzantine values for round r, every non-self entry whose slot
lacks bit r % P takes x_i and is reported missing.  What a missing entry then becomes (SELF keeps
its weight, OMIT adds +0.0, HOLD leaves the mass on the link) is the parents' code, untouched.
With delay_max > 0 the round tested is the delivery round r, like the parents' DROP draw; the round
index is the instance's own, so a restart at round r0 continues at phase r0 % P.
"""
from __future__ import annotations

import numpy as np

from spec_pushsum_hold_np import NpPushSumHoldSim
from spec_pushsum_np import NpPushSumSim
from spec_weighted_np import NpWeightedSim


class ScheduleMixin:
    def __init__(self, cfg, csr, weights, schedule):
        super().__init__(cfg, csr, weights)
        self.period = int(schedule[0])
        av = np.asarray(schedule[1], dtype=np.uint32)
        assert 1 <= self.period <= 32 and av.shape == (self.e_row.size - self.N,)
        assert not np.any(av.astype(np.uint64) >> np.uint64(self.period))
        self.avail = np.concatenate([av, np.zeros(1, np.uint32)])   # (a self entry's slot 0 exists when nnz = 0)

    def _values(self, A, J, slots, selfm, r, b, bG, x, st, lo, hi):
        V, miss = super()._values(A, J, slots, selfm, r, b, bG, x, st, lo, hi)
        bit = np.uint32(1 << (r % self.period))
        down = ~selfm & ((self.avail[slots.astype(np.int64)] & bit) == 0)
        V = np.where(down, np.broadcast_to(x[A][:, None], V.shape), V)
        return V, miss | down


class NpSchedWeightedSim(ScheduleMixin, NpWeightedSim):
    pass


class NpSchedPushSumSim(ScheduleMixin, NpPushSumSim):
    pass


class NpSchedPushSumHoldSim(ScheduleMixin, NpPushSumHoldSim):
    pass


def sched_sim(cfg, csr, weights, schedule):
    """The scheduled restatement the config asks for."""
    if cfg.rule == "weighted":
        return NpSchedWeightedSim(cfg, csr, weights, schedule)
    cls = NpSchedPushSumHoldSim if cfg.missing_policy == "hold" else NpSchedPushSumSim
    return cls(cfg, csr, weights, schedule)


def plain_sim(cfg, csr, weights):
    """The unscheduled restatement of the same config."""
    if cfg.rule == "weighted":
        return NpWeightedSim(cfg, csr, weights)
    return (NpPushSumHoldSim if cfg.missing_policy == "hold" else NpPushSumSim)(cfg, csr, weights)
