"""numpy restatement of rule "weighted" (DESIGN.md §9).  TEST INFRASTRUCTURE.

A subclass of spec_np.NpSim: topology, faults, drops, delays and the §A.6 resolution are NpSim's
(`_values`); only the CSR row update is restated here, from the spec:

    entry 0 weighs w_self[i], entry 1+t weighs w_edge[rowptr[i]+t]
    p_e  = (w_e * v_e) + 0.0                     two roundings, numpy never fuses them
    x_i' = tree_sum(p) / tree_sum(w)             §A.7 tree sums in entry order, IEEE divide
    SELF: a missing entry takes x_i and keeps its weight
    OMIT: a missing entry adds +0.0 to both sums; a zero weight sum keeps x_i
    fp32: weights rounded to binary32 once, every operation in binary32

All receivers are resolved in one `_values` call over the flat list of their entries (one entry
per "row" of that call, so no draw is spent on padding), and the products and weights are then laid
out one receiver per row, padded with +0.0 to a power of two, for spec_np.tree_sum_rows
(spec_np.RaggedTreeSum: rows of like width together, so one 8192-entry hub row does not widen every
other row).  No summand is -0.0, so zeros past a row's end leave its stride-halving sums unchanged
(the argument of spec_np.apply_rule_omit's masked windows): each row's result is that of tree sums
over its own m_i entries.
"""
from __future__ import annotations

import numpy as np

import spec_np as S


class NpWeightedSim(S.NpSim):
    def __init__(self, cfg, csr, weights):
        super().__init__(cfg.replace(rule="average"), csr=csr)   # NpSim needs a rule it knows
        self.cfg = cfg
        assert self.topo == 2 and self.t == 0
        w_self = np.asarray(weights[0], dtype=np.float64).astype(self.ft)
        w_edge = np.asarray(weights[1], dtype=np.float64).astype(self.ft)
        self.zero_den = 0   # rows whose present weights summed to 0 (OMIT) and kept x_i, over the run
        N = self.N
        deg = np.diff(self.rowptr)
        self.mmax = int(deg.max(initial=0)) + 1
        self.row_sums = S.RaggedTreeSum(deg + 1)   # the rows' tree sums, grouped by width
        own = np.arange(N, dtype=np.int64)
        edge_row = np.repeat(own, deg)
        nnz = edge_row.size
        # flat entry list: the N self entries (entry 0, no slot), then the nnz messages by slot
        self.e_row = np.concatenate([own, edge_row])
        self.e_pos = np.concatenate([np.zeros(N, np.int64), 1 + np.arange(nnz) - self.rowptr[edge_row]])
        self.e_j = np.concatenate([own, self.colidx[:nnz]])
        self.e_slot = np.concatenate([np.zeros(N, np.int64), np.arange(nnz)]).astype(np.uint64)
        self.e_self = np.concatenate([np.ones(N, bool), np.zeros(nnz, bool)])
        self.e_w = np.concatenate([w_self, w_edge]).astype(self.ft)

    def _step(self, lb):
        cfg = self.cfg
        b = self.gb[lb]
        bG = b - b % int(cfg.mask_group)
        r = int(self.rounds[lb])
        x = self.x[lb]
        st = self.status[lb]
        ft = self.ft
        crash_node = (st != S.HONEST) & (st != S.BYZ)
        active = (st == S.HONEST) | (crash_node & (np.uint64(r) < st))
        xn = x.copy()
        E = np.nonzero(active[self.e_row])[0]   # the entries of the active receivers
        if E.size:
            rows = self.e_row[E]
            V, miss = self._values(rows, self.e_j[E][:, None], self.e_slot[E][:, None], self.e_self[E][:, None],
                                   r, b, bG, x, st, self.lo[lb], self.hi[lb])
            V, miss = V[:, 0], miss[:, 0]
            gone = miss if self.omit else np.zeros_like(miss)
            w = np.where(gone, ft(0), self.e_w[E]).astype(ft)
            p = np.where(gone, ft(0), (w * V).astype(ft) + ft(0)).astype(ft)
            num, den = self.row_sums(rows, self.e_pos[E], p), self.row_sums(rows, self.e_pos[E], w)
            with np.errstate(divide="ignore", invalid="ignore"):
                q = (num / den).astype(ft)
            self.zero_den += int(np.count_nonzero(active & (den == 0)))
            xn = np.where(active & (den > 0), q, x)
        self.x[lb] = xn
        self.hist[lb].append(xn.copy())
        self.rounds[lb] = r + 1
        self._after(lb)
