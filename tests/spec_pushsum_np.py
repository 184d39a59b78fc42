"""numpy restatement of rule "pushsum" (DESIGN.md §9).  TEST INFRASTRUCTURE.

A subclass of spec_weighted_np.NpWeightedSim: the flat entry list, the weights (rounded to the
config dtype once) and the drop draws (spec_np.NpSim._values, all nodes honest, no delays) are
its; only the row update is restated here, from the spec:

    state       (s_i, z_i); round 0: s = x^0, z = 1; x_i = s_i / z_i is what the engine sees
    ps_e, pz_e  (w_e * s_e) + 0.0 and (w_e * z_e) + 0.0     two roundings each, numpy never fuses
    s_i', z_i'  tree_sum(ps), tree_sum(pz)                  §A.7 in entry order, no normalisation
    x_i'        s_i' / z_i' where z_i' > 0, else x_i        IEEE divide; the pair is stored as computed
    loss        a dropped message adds +0.0 to both sums (its mass is lost)
    fp32        every operation in binary32, subnormals included

The products are laid out one receiver per row, padded with +0.0 to a power of two, for
spec_np.tree_sum_rows (the parent's row_sums); no summand is -0.0, so the padding leaves each row's
stride-halving sums unchanged (the argument of spec_weighted_np).
"""
from __future__ import annotations

import numpy as np

from spec_weighted_np import NpWeightedSim


class NpPushSumSim(NpWeightedSim):
    def __init__(self, cfg, csr, weights):
        super().__init__(cfg, csr, weights)
        assert self.fault == 0 and self.D == 0 and (self.thr == 0 or self.omit)
        self.s = self.x.copy()
        self.z = np.ones_like(self.x)
        self.kept = [[] for _ in range(self.B)]   # per round: rows with z' = 0 that kept x_i

    def restart(self, rnd, s, z=None):
        """acs_set_pushsum_state(rnd, s, z) / acs_set_state(rnd, x) (z = None: s = x, z = 1)."""
        ft = self.ft
        self.s = np.asarray(s, dtype=ft).reshape(self.B, self.N) + ft(0)
        self.z = np.ones_like(self.s) if z is None else np.asarray(z, dtype=ft).reshape(self.B, self.N) + ft(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (self.s / self.z).astype(ft)
        self.x = np.where(self.z > 0, q, self.s)
        self.rounds[:] = rnd
        for lb in range(self.B):
            self.trace[lb] = [np.nan] * rnd
            self._after(lb)

    def _step(self, lb):
        cfg = self.cfg
        b = self.gb[lb]
        bG = b - b % int(cfg.mask_group)
        r = int(self.rounds[lb])
        x, s, z = self.x[lb], self.s[lb], self.z[lb]
        ft = self.ft
        _, miss = self._values(self.e_row, self.e_j[:, None], self.e_slot[:, None], self.e_self[:, None],
                               r, b, bG, x, self.status[lb], self.lo[lb], self.hi[lb])
        gone = miss[:, 0]
        ps = np.where(gone, ft(0), (self.e_w * s[self.e_j]).astype(ft) + ft(0)).astype(ft)
        pz = np.where(gone, ft(0), (self.e_w * z[self.e_j]).astype(ft) + ft(0)).astype(ft)
        sn, zn = self.row_sums(self.e_row, self.e_pos, ps), self.row_sums(self.e_row, self.e_pos, pz)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (sn / zn).astype(ft)
        self.kept[lb].append(int(np.count_nonzero(zn == 0)))
        xn = np.where(zn > 0, q, x)
        self.s[lb], self.z[lb], self.x[lb] = sn, zn, xn
        self.hist[lb].append(xn.copy())
        self.rounds[lb] = r + 1
        self._after(lb)
