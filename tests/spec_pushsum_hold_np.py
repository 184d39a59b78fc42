"""numpy restatement of rule "pushsum" under missing_policy = "hold" (DESIGN.md §9).  TEST INFRASTRUCTURE.

A subclass of spec_pushsum_np.NpPushSumSim: the flat entry list, the weights, the drop draws and
the row sums are its; only what happens to a message on its link is restated here, from the spec.
Besides (s_i, z_i) every slot e holds a pair (h_e, k_e), +0.0 at round 0.  Per sender entry e:

    a, c     (w_e * s_j) + 0.0 and (w_e * z_j) + 0.0    as the plain rule: two roundings each
    hn, kn   h_e + a and k_e + c                         one rounding each, config dtype
    dropped  the plain rule's DROP draw of (bG, r, e)
    delivered: the entry contributes (hn, kn), the link stores (+0.0, +0.0)
    dropped:   the entry contributes (+0.0, +0.0), the link stores (hn, kn)

Entry 0 (the receiver itself) has no link.  h and k are kept per flat entry ([B][N + nnz]: the N
self entries first, always 0, then the nnz slots in slot order), so the public slot-order arrays
are h[:, N:] and k[:, N:].

The parent knows SELF and OMIT only and asserts one of them: it is given the config with
missing_policy = "omit", which draws exactly the drops HOLD draws.
"""
from __future__ import annotations

import numpy as np

from spec_pushsum_np import NpPushSumSim


class NpPushSumHoldSim(NpPushSumSim):
    def __init__(self, cfg, csr, weights):
        assert cfg.missing_policy == "hold"
        super().__init__(cfg.replace(missing_policy="omit"), csr, weights)
        self.nnz = self.e_row.size - self.N
        self.h = np.zeros((self.B, self.N + self.nnz), dtype=self.ft)
        self.k = np.zeros((self.B, self.N + self.nnz), dtype=self.ft)

    def links(self, lb=0):
        """(h[nnz], k[nnz]) of one instance in slot order (acs_get_pushsum_links)."""
        return self.h[lb, self.N:].copy(), self.k[lb, self.N:].copy()

    def restart(self, rnd, s, z=None):
        """acs_set_pushsum_state / acs_set_state: the links are zeroed."""
        self.h[:] = 0
        self.k[:] = 0
        super().restart(rnd, s, z)

    def set_links(self, h, k):
        """acs_set_pushsum_links(h, k): B * nnz values each, instance-major; -0.0 becomes +0.0."""
        ft = self.ft
        self.h[:, self.N:] = np.asarray(h, dtype=ft).reshape(self.B, self.nnz) + ft(0)
        self.k[:, self.N:] = np.asarray(k, dtype=ft).reshape(self.B, self.nnz) + ft(0)

    def mass(self, lb=0):
        """(fsum(s) + fsum(h), fsum(z) + fsum(k)) as Python floats (Simulator.pushsum_mass)."""
        import math
        return (math.fsum(self.s[lb].tolist()) + math.fsum(self.h[lb].tolist()),
                math.fsum(self.z[lb].tolist()) + math.fsum(self.k[lb].tolist()))

    def _step(self, lb):
        cfg = self.cfg
        b = self.gb[lb]
        bG = b - b % int(cfg.mask_group)
        r = int(self.rounds[lb])
        x, s, z = self.x[lb], self.s[lb], self.z[lb]
        ft = self.ft
        _, miss = self._values(self.e_row, self.e_j[:, None], self.e_slot[:, None], self.e_self[:, None],
                               r, b, bG, x, self.status[lb], self.lo[lb], self.hi[lb])
        gone = miss[:, 0]   # (never an entry 0: those have no link and h = k = 0, so hn = a there)
        a = (self.e_w * s[self.e_j]).astype(ft) + ft(0)
        c = (self.e_w * z[self.e_j]).astype(ft) + ft(0)
        hn = (self.h[lb] + a).astype(ft)
        kn = (self.k[lb] + c).astype(ft)
        ps = np.where(gone, ft(0), hn).astype(ft)
        pz = np.where(gone, ft(0), kn).astype(ft)
        self.h[lb] = np.where(gone, hn, ft(0))
        self.k[lb] = np.where(gone, kn, ft(0))
        sn, zn = self.row_sums(self.e_row, self.e_pos, ps), self.row_sums(self.e_row, self.e_pos, pz)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (sn / zn).astype(ft)
        self.kept[lb].append(int(np.count_nonzero(zn == 0)))
        xn = np.where(zn > 0, q, x)
        self.s[lb], self.z[lb], self.x[lb] = sn, zn, xn
        self.hist[lb].append(xn.copy())
        self.rounds[lb] = r + 1
        self._after(lb)
