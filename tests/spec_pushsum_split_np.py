"""numpy restatement of push-sum with per-round splitting ("Push-sum with per-round
splitting").  TEST INFRASTRUCTURE.

A subclass of spec_pushsum_np.NpPushSumSim: the flat entry list, the DROP draws and the tree sums
are the parents'.  Restated here, from the spec:

    shares      c_p(j) = 1 + #{slots e : colidx[e] == j, bit p of avail[e] set}; share_p(j) is 1 / c_p(j)
                rounded to the config dtype, stepped one ulp down while c_p(j) * share > 1 exactly
                (decided in fractions.Fraction; acsim.graphs.split_shares is not used here)
    offer       o_j = (share_p(j) * s_j + 0.0, share_p(j) * z_j + 0.0), p = r mod P      two roundings each
    entries     entry 0 is o_i; entry 1 + t is o_colidx[e], e = rowptr[i] + t, when bit p of avail[e]
                is set and the message is not dropped, else +0.0 in both sums
    s_i', z_i'  tree sums in entry order; x_i' = s_i' / z_i' where z_i' > 0, else x_i

There is no weight argument: the handle's weights are the shares.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from spec_pushsum_np import NpPushSumSim


def share_of(c, ft):
    """1 / c in `ft`, stepped down while c * w > 1 in exact arithmetic."""
    w = ft(1) / ft(c)
    while Fraction(float(w)) * c > 1:
        w = np.nextafter(w, ft(0))
    return w


def np_split_shares(csr, schedule, ft):
    rp, ci = np.asarray(csr[0]).astype(np.int64), np.asarray(csr[1]).astype(np.int64)
    period, av = int(schedule[0]), np.asarray(schedule[1], dtype=np.uint32)
    n = rp.size - 1
    out = np.empty((period, n), dtype=ft)
    memo = {}
    for p in range(period):
        c = 1 + np.bincount(ci[(av >> np.uint32(p)) & np.uint32(1) == 1], minlength=n)
        for k in np.unique(c).tolist():
            if k not in memo:
                memo[k] = share_of(k, ft)
        out[p] = np.array([memo[k] for k in c.tolist()], dtype=ft)
    return out


class NpPushSumSplitSim(NpPushSumSim):
    def __init__(self, cfg, csr, schedule):
        n, nnz = np.asarray(csr[0]).size - 1, np.asarray(csr[1]).size
        super().__init__(cfg, csr, (np.ones(n), np.ones(nnz)))   # (the parent's weights are not read)
        assert cfg.missing_policy in ("self", "omit")
        self.period = int(schedule[0])
        av = np.asarray(schedule[1], dtype=np.uint32)
        assert 1 <= self.period <= 32 and av.shape == (nnz,)
        assert not np.any(av.astype(np.uint64) >> np.uint64(self.period))
        self.share = np_split_shares(csr, (self.period, av), self.ft)   # [P][N]
        self.e_avail = np.concatenate([np.zeros(n, np.uint32), av])      # flat entry order: self entries first
        del self.e_w

    def _step(self, lb):
        cfg = self.cfg
        b = self.gb[lb]
        bG = b - b % int(cfg.mask_group)
        r = int(self.rounds[lb])
        p = r % self.period
        x, s, z = self.x[lb], self.s[lb], self.z[lb]
        ft = self.ft
        sh = self.share[p]
        os_ = ((sh * s).astype(ft) + ft(0)).astype(ft)   # every node's offer, once
        oz = ((sh * z).astype(ft) + ft(0)).astype(ft)
        _, miss = self._values(self.e_row, self.e_j[:, None], self.e_slot[:, None], self.e_self[:, None],
                               r, b, bG, x, self.status[lb], self.lo[lb], self.hi[lb])
        down = ~self.e_self & ((self.e_avail & np.uint32(1 << p)) == 0)
        gone = miss[:, 0] | down
        ps = np.where(gone, ft(0), os_[self.e_j]).astype(ft)
        pz = np.where(gone, ft(0), oz[self.e_j]).astype(ft)
        sn, zn = self.row_sums(self.e_row, self.e_pos, ps), self.row_sums(self.e_row, self.e_pos, pz)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (sn / zn).astype(ft)
        self.kept[lb].append(int(np.count_nonzero(zn == 0)))
        xn = np.where(zn > 0, q, x)
        self.s[lb], self.z[lb], self.x[lb] = sn, zn, xn
        self.hist[lb].append(xn.copy())
        self.rounds[lb] = r + 1
        self._after(lb)

    def effective_weights(self, p):
        """(w_self, w_edge) of the static push-sum handle that runs phase p: the sender's share on an
        up slot, +0.0 on a down one."""
        av = self.e_avail[self.N:]
        ci = self.e_j[self.N:]
        we = np.where((av >> np.uint32(p)) & np.uint32(1) == 1, self.share[p][ci], self.ft(0))
        return self.share[p].astype(np.float64), we.astype(np.float64)
