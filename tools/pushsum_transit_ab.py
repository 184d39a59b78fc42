#!/usr/bin/env python3
"""Per-round kernel time of push-sum with messages in transit against the plain rule and HOLD on the
same CSR graph, weights and drop draws ("Push-sum with messages in transit").

Workload: the 2^20-node skewed graph of tests/test_csr.py::test_csr_full_size_skewed_2e20
(skewed_csr(2^20, 11, 32, seed 11)), weights 1 / (outdeg + 1) (graphs.pushsum_weights in the run's
dtype), loss_p = 0.1, 100 FIXED rounds after 5 warm-up rounds.  In ONE process, for fp64 and then
fp32, the four sides alternate within every repetition:
  omit      missing_policy="omit":              k_round_pushsum<32,csr>           (the yardstick)
  hold      missing_policy="hold":              k_round_pushsum_hold<32,csr>
  transit1  missing_policy="omit", transit=1:   k_round_pushsum_transit<32,csr>
  transit3  missing_policy="omit", transit=3:   k_round_pushsum_transit<32,csr>
Every round is bracketed by device events (set_kernel_timing); one record per run goes to the
output file, then one summary record per dtype with the medians, the spreads and the byte-count
expectation.

    python tools/pushsum_transit_ab.py --out FILE.jsonl [--reps 5] [--sha COMMIT]

profiles/pushsum_transit_ab.jsonl holds one such run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximate-consensus-simulation_amd"))

import acsim  # noqa: E402
from acsim.config import Config  # noqa: E402
from acsim.graphs import pushsum_weights, skewed_csr  # noqa: E402

SIDES = {   # side: (missing_policy, transit, kernel)
    "omit": ("omit", None, "k_round_pushsum<32,csr>"),
    "hold": ("hold", None, "k_round_pushsum_hold<32,csr>"),
    "transit1": ("omit", 1, "k_round_pushsum_transit<32,csr>"),
    "transit3": ("omit", 3, "k_round_pushsum_transit<32,csr>"),
}


def timed_run(cfg, csr, weights, transit, rounds, warmup, want):
    with acsim.Simulator(cfg, csr=csr, weights=weights, transit=transit) as g:
        name = g.kernel_name()
        assert name == want + (" [f32]" if cfg.dtype == "f32" else ""), (name, want)
        g.round(warmup)                  # warm-up: code objects loaded, clocks up, links and planes in use
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
    ap.add_argument("--loss", type=float, default=0.1)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--sha", default=None, help="commit measured (default: git rev-parse, where there is a checkout)")
    ap.add_argument("--box", default="MI355X (gfx950)")
    a = ap.parse_args()
    rp, ci = skewed_csr(a.n, 11, 32, 11)
    sha = a.sha
    if sha is None:
        try:
            sha = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                 text=True).stdout.strip() or None
        except OSError:
            sha = None
    box = {"gpu": a.box, "runtime": acsim._abi.runtime_info()["versions"]}
    out = [{"what": "per-round device us (HIP events around every round, %d FIXED rounds after %d warm-up rounds), rule "
                    "pushsum with loss_p = %g: the plain rule (omit), hold, and messages in transit with transit_max 1 and "
                    "3 on the same weights 1 / (outdeg + 1), alternating in one process" % (a.rounds, a.warmup, a.loss),
            "graph": "skewed_csr(%d, 11, 32, seed 11)" % a.n, "nnz": int(ci.size), "box": box, "sha": sha}]
    for dtype in ("f64", "f32"):
        w = pushsum_weights(rp, ci, dtype=dtype)
        base = dict(n_nodes=a.n, topology="csr", rule="pushsum", termination="fixed", max_rounds=a.rounds + a.warmup,
                    seed=12, dtype=dtype, loss_p=a.loss)
        es = 4 if dtype == "f32" else 8
        us = {side: [] for side in SIDES}
        for rep in range(a.reps):
            for side, (policy, transit, kernel) in SIDES.items():
                t, name = timed_run(Config(missing_policy=policy, **base), (rp, ci), w, transit, a.rounds, a.warmup, kernel)
                us[side].append(t)
                out.append({"dtype": dtype, "side": side, "rep": rep, "us_per_round": round(t, 3), "kernel": name})
                print(out[-1], flush=True)
        med = {side: statistics.median(v) for side, v in us.items()}
        plain = 4 + 3 * es   # per slot: 4 B of id + one weight + one gathered pair
        out.append({"summary": True, "dtype": dtype,
                    "us_median": {side: round(m, 3) for side, m in med.items()},
                    "us_minmax": {side: [round(min(v), 3), round(max(v), 3)] for side, v in us.items()},
                    "ratio_to_omit": {side: round(m / med["omit"], 4) for side, m in med.items()},
                    "ratio_to_hold": {side: round(m / med["hold"], 4) for side, m in med.items()},
                    # HOLD adds one link pair read and, at most, written; transit one cell read and, for delta > 0
                    # (a share D / (D + 1) of the sent messages), a read and a write of another cell
                    "byte_ratio_expected": {"hold": round((plain + 4 * es) / plain, 4),
                                            "transit1": round((plain + 2 * es + 0.5 * 0.9 * 4 * es) / plain, 4),
                                            "transit3": round((plain + 2 * es + 0.75 * 0.9 * 4 * es) / plain, 4)}})
        print(out[-1], flush=True)
    with open(a.out, "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
