"""numpy restatement of rule "pushsum" with messages in transit.  TEST INFRASTRUCTURE.

A subclass of spec_pushsum_np.NpPushSumSim (with a link schedule: of spec_sched_np.ScheduleMixin over
it): the flat entry list, the weights, the missing test (drop draws, down slots) and the row sums are
the parents'; only what happens to a message between its sender and its receiver is restated here,
from the spec.  A handle has a transit bound D.  Per sender entry e and round q:

    a^q, c^q    (w_e * s_j^q) + 0.0 and (w_e * z_j^q) + 0.0      the plain rule's products
    gone^q      the plain rule's missing test of round q          a gone message never enters transit
    delta^q     draw(DELAY = 7, b, q, e) mod (D + 1)              b the global instance id, no clipping
    the message is delivered in round q + delta^q

The restatement is written in HISTORY FORM: it keeps, per instance, the products, delays and gone
flags of the last D + 1 sending rounds and nothing else.  The arrival on slot e in round r is then
computed from the definition,

    base_r(e) + sum over q = r - D .. r, ascending, of a^q(e) where delta^q(e) = r - q and not gone^q(e)

one rounding per addition in the config dtype, where base_r is +0.0 or the plane set_transit put
down for round r.  There is no ring and no cell that is updated as messages are sent: that is the
device's formulation, and this one is independent of it.  (A cell of the device's ring takes its
summands in the same ascending order, one rounding each, so the two agree bit for bit.)

transit(lb) returns the D planes acs_get_pushsum_transit returns: plane d is what round R + d would
deliver from the messages already sent, the same fold cut off at sending round R - 1.

Entry 0 (the receiver itself) has no link: it is never gone, its delay is 0, and it is delivered in
the round it is computed.  Arrays are per flat entry ([N + nnz]: the N self entries, then the slots).
"""
from __future__ import annotations

import math

import numpy as np

import spec_np as S
from spec_pushsum_np import NpPushSumSim
from spec_sched_np import ScheduleMixin

DELAY = 7


class NpPushSumTransitSim(NpPushSumSim):
    def __init__(self, cfg, csr, weights, transit=0):
        super().__init__(cfg, csr, weights)
        self._init_transit(transit)

    def _init_transit(self, transit):
        self.T = int(transit)
        assert 0 <= self.T <= 64
        self.nnz = self.e_row.size - self.N
        # per instance: {sending round q: (a, c, delta, gone)} of the last D + 1 rounds, and the planes a
        # resume put down, {arrival round: (h, k)} per flat entry
        self.sent = [dict() for _ in range(self.B)]
        self.base = [dict() for _ in range(self.B)]

    # ------------------------------------------------------------------ the definition of an arrival
    def _arrival(self, lb, rho, upto):
        """What round rho delivers from the messages sent in rounds <= upto: (h, k) per flat entry."""
        ft = self.ft
        n = self.e_row.size
        h, k = self.base[lb].get(rho, (np.zeros(n, ft), np.zeros(n, ft)))
        h, k = h.copy(), k.copy()
        for q in range(rho - self.T, min(rho, upto) + 1):
            if q not in self.sent[lb]:
                continue
            a, c, dl, gone = self.sent[lb][q]
            hit = ~gone & (dl == rho - q)
            h = np.where(hit, (h + a).astype(ft), h)
            k = np.where(hit, (k + c).astype(ft), k)
        return h, k

    def transit(self, lb=0):
        """(h[D, nnz], k[D, nnz]) of one instance in slot order (acs_get_pushsum_transit)."""
        R = int(self.rounds[lb])
        planes = [self._arrival(lb, R + d, R - 1) for d in range(self.T)]
        h = np.stack([p[0][self.N:] for p in planes]) if self.T else np.zeros((0, self.nnz), self.ft)
        k = np.stack([p[1][self.N:] for p in planes]) if self.T else np.zeros((0, self.nnz), self.ft)
        return h, k

    def restart(self, rnd, s, z=None):
        """acs_set_pushsum_state / acs_set_state: nothing is in transit afterwards."""
        for lb in range(self.B):
            self.sent[lb].clear()
            self.base[lb].clear()
        super().restart(rnd, s, z)

    def set_transit(self, h, k):
        """acs_set_pushsum_transit(h, k): B * D * nnz values each, instance-major, each instance's D
        planes relative to its own round; -0.0 becomes +0.0.  Whatever was in transit is replaced."""
        ft = self.ft
        h = np.asarray(h, dtype=ft).reshape(self.B, self.T, self.nnz) + ft(0)
        k = np.asarray(k, dtype=ft).reshape(self.B, self.T, self.nnz) + ft(0)
        pad = np.zeros(self.N, ft)
        for lb in range(self.B):
            R = int(self.rounds[lb])
            self.sent[lb].clear()
            self.base[lb] = {R + d: (np.concatenate([pad, h[lb, d]]), np.concatenate([pad, k[lb, d]]))
                             for d in range(self.T)}

    def mass(self, lb=0):
        """(fsum(s) + fsum(h), fsum(z) + fsum(k)) as Python floats (Simulator.pushsum_mass)."""
        h, k = self.transit(lb)
        return (math.fsum(self.s[lb].tolist()) + math.fsum(h.reshape(-1).tolist()),
                math.fsum(self.z[lb].tolist()) + math.fsum(k.reshape(-1).tolist()))

    # ------------------------------------------------------------------------------------ one round
    def _step(self, lb):
        cfg = self.cfg
        b = self.gb[lb]
        bG = b - b % int(cfg.mask_group)
        r = int(self.rounds[lb])
        x, s, z = self.x[lb], self.s[lb], self.z[lb]
        ft = self.ft
        _, miss = self._values(self.e_row, self.e_j[:, None], self.e_slot[:, None], self.e_self[:, None],
                               r, b, bG, x, self.status[lb], self.lo[lb], self.hi[lb])
        gone = miss[:, 0]   # (never an entry 0)
        a = (self.e_w * s[self.e_j]).astype(ft) + ft(0)
        c = (self.e_w * z[self.e_j]).astype(ft) + ft(0)
        dl = (S.draw(self.seed, DELAY, b, r, self.e_slot) % np.uint32(self.T + 1)).astype(np.int64)
        dl[self.e_self] = 0   # entry 0 has no link and no delay
        self.sent[lb][r] = (a, c, dl, gone)
        for q in [q for q in self.sent[lb] if q < r - self.T]:   # nothing older can still arrive
            del self.sent[lb][q]
        ps, pz = self._arrival(lb, r, r)
        self.base[lb].pop(r, None)
        sn, zn = self.row_sums(self.e_row, self.e_pos, ps), self.row_sums(self.e_row, self.e_pos, pz)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (sn / zn).astype(ft)
        self.kept[lb].append(int(np.count_nonzero(zn == 0)))
        xn = np.where(zn > 0, q, x)
        self.s[lb], self.z[lb], self.x[lb] = sn, zn, xn
        self.hist[lb].append(xn.copy())
        self.rounds[lb] = r + 1
        self._after(lb)


class NpSchedPushSumTransitSim(ScheduleMixin, NpPushSumTransitSim):
    def __init__(self, cfg, csr, weights, schedule, transit):
        ScheduleMixin.__init__(self, cfg, csr, weights, schedule)   # (-> NpPushSumSim.__init__ below)
        self._init_transit(transit)


def transit_sim(cfg, csr, weights, transit, schedule=None):
    """The restatement of Simulator(cfg, csr=, weights=, schedule=, transit=)."""
    if schedule is None:
        return NpPushSumTransitSim(cfg, csr, weights, transit)
    return NpSchedPushSumTransitSim(cfg, csr, weights, schedule, transit)
