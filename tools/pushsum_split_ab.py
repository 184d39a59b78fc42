#!/usr/bin/env python3
"""A/B of one round of push-sum with per-round splitting (acs_create_csr_split) against the scheduled
push-sum handles with fixed weights (acs_create_csr_scheduled), DESIGN.md §9, "Push-sum with
per-round splitting".

Workload: the 2^20-node skewed graph of tests/test_csr.py::test_csr_full_size_skewed_2e20
(skewed_csr(2^20, 11, 32, seed 11)), 100 FIXED rounds after 5 warm-up rounds, no loss.  In ONE
process, for fp64 and then fp32, three pairs, each alternating --reps times:
  hold_phase   split vs HOLD with weights 1 / (outdeg + 1), both on the one-phase-of-4 schedule
               (HOLD there is the yardstick: the other mean-preserving scheduled push-sum)
  omit_phase   split vs OMIT with the same weights on the same schedule
  omit_full    split vs OMIT on full masks (period 4): every gather is used
Every round is bracketed by device events (set_kernel_timing); one record per run goes to the
output file, then one summary record per (dtype, pair) with the medians, the ranges and the byte
ratio per padded slot.  Per padded slot a split lane reads 4 (id) + 4 (mask) bytes and gathers one
pair; a scheduled OMIT lane reads 4 + es (weight) + 4 and gathers one pair; HOLD adds the link pair,
read and written.  The tool asserts both kernel names.

    python tools/pushsum_split_ab.py --out FILE.jsonl [--reps 5] [--sha COMMIT]

profiles/pushsum_split_ab.jsonl holds one such run.
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
from acsim.graphs import full_schedule, phase_schedule, pushsum_weights, skewed_csr  # noqa: E402

SPLIT_KERNEL = "k_round_pushsum_split<32,csr>"


def slot_bytes(side, es):
    """Bytes per padded slot: id, [weight], mask, the gathered pair, [the link pair read and written]."""
    return {"split": 4 + 4 + 2 * es, "omit": 4 + es + 4 + 2 * es, "hold": 4 + es + 4 + 2 * es + 4 * es}[side]


def timed_run(cfg, csr, weights, schedule, rounds, warmup, want):
    kw = dict(split=True) if weights is None else dict(weights=weights)
    with acsim.Simulator(cfg, csr=csr, schedule=schedule, **kw) as g:
        name = g.kernel_name()
        assert name == want + (" [f32]" if cfg.dtype == "f32" else ""), (name, want)
        g.round(warmup)                  # warm-up: code objects loaded, clocks up, links in use
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
                    "pushsum, no loss: the split handle vs the scheduled handle with weights 1 / (outdeg + 1) under HOLD "
                    "and under OMIT, alternating in one process" % (a.rounds, a.warmup),
            "graph": "skewed_csr(%d, 11, 32, seed 11)" % a.n, "nnz": int(ci.size), "box": box, "sha": sha}]
    full = full_schedule(ci.size, 4)
    phase = phase_schedule(rp, ci, 4, seed=0)
    pairs = {"hold_phase": ("hold", phase), "omit_phase": ("omit", phase), "omit_full": ("omit", full)}
    for dtype in ("f64", "f32"):
        w = pushsum_weights(rp, ci, dtype=dtype)
        es = 4 if dtype == "f32" else 8
        for pair, (policy, sch) in pairs.items():
            other = "k_round_pushsum%s<32,csr,sched>" % ("_hold" if policy == "hold" else "")
            cfg = Config(n_nodes=a.n, topology="csr", rule="pushsum", termination="fixed", max_rounds=a.rounds + a.warmup,
                         seed=12, dtype=dtype, missing_policy=policy)
            sides = {"split": (cfg.replace(missing_policy="omit"), None, SPLIT_KERNEL), policy: (cfg, w, other)}
            us = {side: [] for side in sides}
            for rep in range(a.reps):
                for side, (c, weights, want) in sides.items():
                    t, name = timed_run(c, (rp, ci), weights, sch, a.rounds, a.warmup, want)
                    us[side].append(t)
                    out.append({"dtype": dtype, "pair": pair, "side": side, "rep": rep, "us_per_round": round(t, 3),
                                "kernel": name})
                    print(out[-1], flush=True)
            med = {side: statistics.median(v) for side, v in us.items()}
            rec = {"summary": True, "dtype": dtype, "pair": pair,
                   "ratio_split_over_%s" % policy: round(med["split"] / med[policy], 4),
                   "byte_ratio_expected": round(slot_bytes("split", es) / slot_bytes(policy, es), 4)}
            for side, v in us.items():
                rec[side + "_us_median"] = round(med[side], 3)
                rec[side + "_us_minmax"] = [round(min(v), 3), round(max(v), 3)]
            out.append(rec)
            print(rec, flush=True)
    with open(a.out, "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
