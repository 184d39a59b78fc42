#!/usr/bin/env python3
"""Per-round kernel time of rule weighted with quantized messages against the plain rule on the same
CSR graph and weights ("Quantized messages").

Workload: the 2^20-node skewed graph of tests/test_csr.py::test_csr_full_size_skewed_2e20
(skewed_csr(2^20, 11, 32, seed 11)), every weight 1 (rows average their entries), no loss, 100 FIXED
rounds after 5 warm-up rounds.  In ONE process, for fp64 and then fp32, the four sides alternate
within every repetition:
  plain        no quant:                          k_round_weighted<32,csr>         (the yardstick)
  partial      quant=(8, "partial", True):        k_round_weighted<32,csr,quant>
  total        quant=(8, "total", True):          k_round_weighted<32,csr,quant>
  compensated  quant=(8, "compensated", True):    k_round_weighted<32,csr,quant>
Every round is bracketed by device events (set_kernel_timing); one record per run goes to the
output file, then one summary record per dtype with the medians, the spreads, the ratios to the
plain rule and the byte-count expectation.

    python tools/quant_ab.py --out FILE.jsonl [--reps 5] [--sha COMMIT]

profiles/quant_ab.jsonl holds one such run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximate-consensus-simulation_amd"))

import acsim  # noqa: E402
from acsim.config import Config  # noqa: E402
from acsim.graphs import skewed_csr  # noqa: E402

SIDES = {   # side: (quant, kernel)
    "plain": (None, "k_round_weighted<32,csr>"),
    "partial": ("partial", "k_round_weighted<32,csr,quant>"),
    "total": ("total", "k_round_weighted<32,csr,quant>"),
    "compensated": ("compensated", "k_round_weighted<32,csr,quant>"),
}


def timed_run(cfg, csr, weights, quant, rounds, warmup, want):
    with acsim.Simulator(cfg, csr=csr, weights=weights, quant=quant) as g:
        name = g.kernel_name()
        assert name == want + (" [f32]" if cfg.dtype == "f32" else ""), (name, want)
        g.round(warmup)                  # warm-up: code objects loaded, clocks up, both buffers of x and q in use
        g.set_kernel_timing(True)
        g.run()
        ms, n, _ = g.kernel_timing()
        assert n == rounds, (n, rounds)
        return 1000.0 * ms / n, name


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--sha", default=None, help="commit measured (default: git rev-parse, where there is a checkout)")
    ap.add_argument("--box", default="MI355X (gfx950)")
    a = ap.parse_args()
    rp, ci = skewed_csr(a.n, 11, 32, 11)
    w = (np.ones(a.n), np.ones(ci.size))
    sha = a.sha
    if sha is None:
        try:
            sha = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                 text=True).stdout.strip() or None
        except OSError:
            sha = None
    box = {"gpu": a.box, "runtime": acsim._abi.runtime_info()["versions"]}
    slots = ci.size / a.n
    out = [{"what": "per-round device us (HIP events around every round, %d FIXED rounds after %d warm-up rounds), rule "
                    "weighted, no loss: the plain rule and quantized messages (step 2^-%d, dithered) in modes partial, "
                    "total and compensated on the same unit weights, alternating in one process" % (a.rounds, a.warmup, a.k),
            "graph": "skewed_csr(%d, 11, 32, seed 11)" % a.n, "nnz": int(ci.size), "slots_per_row": round(slots, 3),
            "box": box, "sha": sha}]
    for dtype in ("f64", "f32"):
        base = dict(n_nodes=a.n, topology="csr", rule="weighted", termination="fixed", max_rounds=a.rounds + a.warmup,
                    seed=12, dtype=dtype)
        es = 4 if dtype == "f32" else 8
        us = {side: [] for side in SIDES}
        for rep in range(a.reps):
            for side, (mode, kernel) in SIDES.items():
                quant = None if mode is None else (a.k, mode, True)
                t, name = timed_run(Config(**base), (rp, ci), w, quant, a.rounds, a.warmup, kernel)
                us[side].append(t)
                out.append({"dtype": dtype, "side": side, "rep": rep, "us_per_round": round(t, 3), "kernel": name})
                print(out[-1], flush=True)
        med = {side: statistics.median(v) for side, v in us.items()}
        # per row: per slot 4 B of id, one weight and one gathered value; w_self, rowptr, deg, x_i and the store of x_i'.
        # Quantized: the same slots (the gathers read q instead of x), plus q_i read and q_i' stored.
        plain = slots * (4 + 2 * es) + 8 + 1 + 3 * es
        out.append({"summary": True, "dtype": dtype,
                    "us_median": {side: round(m, 3) for side, m in med.items()},
                    "us_minmax": {side: [round(min(v), 3), round(max(v), 3)] for side, v in us.items()},
                    "ratio_to_plain": {side: round(m / med["plain"], 4) for side, m in med.items()},
                    "allowed_ratio": 1.10,
                    "bytes_per_row_plain": round(plain, 1),
                    "byte_ratio_expected": round((plain + 2 * es) / plain, 4)})
        print(out[-1], flush=True)
    with open(a.out, "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
