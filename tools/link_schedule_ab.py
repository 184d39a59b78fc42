#!/usr/bin/env python3
"""A/B of one round of a scheduled handle (acs_create_csr_scheduled, full masks) against the
unscheduled handle of the same config, for rules weighted and pushsum ("Link
schedules").

Workload: the 2^20-node skewed graph of tests/test_csr.py::test_csr_full_size_skewed_2e20
(skewed_csr(2^20, 11, 32, seed 11)), weights 1 / (outdeg + 1) (graphs.pushsum_weights in the run's
dtype), 100 FIXED rounds after 5 warm-up rounds.  In ONE process, for fp64 and then fp32, for
weighted (SELF), pushsum OMIT and pushsum HOLD, alternating:
  A  no schedule:                 k_round_*<32,csr>          (the yardstick)
  B  full masks, period 4:        k_round_*<32,csr,sched>    (the same values, bit for bit: asserted)
and for HOLD also
  C  one phase of 4 per slot:     k_round_pushsum_hold<32,csr,sched>   (three messages in four wait on
                                  their links: most link stores happen)
Every round is bracketed by device events (set_kernel_timing); one record per run goes to the
output file, then one summary record per (dtype, rule) with the medians and the byte ratio per
padded slot: the schedule adds a 4-byte mask to the id, the weight and the gathered value or pair
(and, under HOLD, the link pair read and written).

    python tools/link_schedule_ab.py --out FILE.jsonl [--reps 5] [--sha COMMIT]

profiles/link_schedule_ab.jsonl holds one such run.
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
from acsim.graphs import full_schedule, phase_schedule, pushsum_weights, skewed_csr  # noqa: E402

# rule -> (config fields, kernel, bytes per padded slot without a schedule as a function of the value size)
RULES = {
    "weighted": (dict(rule="weighted"), "k_round_weighted", lambda es: 4 + es + es),
    "pushsum_omit": (dict(rule="pushsum", missing_policy="omit"), "k_round_pushsum", lambda es: 4 + es + 2 * es),
    "pushsum_hold": (dict(rule="pushsum", missing_policy="hold"), "k_round_pushsum_hold", lambda es: 4 + es + 2 * es + 4 * es),
}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def timed_run(cfg, csr, weights, schedule, rounds, warmup, want):
    with acsim.Simulator(cfg, csr=csr, weights=weights, schedule=schedule) as g:
        name = g.kernel_name()
        assert name == want + (" [f32]" if cfg.dtype == "f32" else ""), (name, want)
        g.round(warmup)                  # warm-up: code objects loaded, clocks up, links in use
        g.set_kernel_timing(True)
        g.run()
        ms, n, _ = g.kernel_timing()
        assert n == rounds, (n, rounds)
        final = [g.values(0)] + (list(g.pushsum_state(0)) if cfg.rule == "pushsum" else [])
        return 1000.0 * ms / n, name, final


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
    out = [{"what": "per-round device us (HIP events around every round, %d FIXED rounds after %d warm-up rounds), rules "
                    "weighted, pushsum omit and pushsum hold with weights 1 / (outdeg + 1) and no loss: the unscheduled "
                    "handle vs the scheduled handle with full masks (period 4), alternating in one process; hold also on a "
                    "one-phase-of-4 schedule" % (a.rounds, a.warmup),
            "graph": "skewed_csr(%d, 11, 32, seed 11)" % a.n, "nnz": int(ci.size), "box": box, "sha": sha}]
    full = full_schedule(ci.size, 4)
    phase = phase_schedule(rp, ci, 4, seed=0)
    for dtype in ("f64", "f32"):
        w = pushsum_weights(rp, ci, dtype=dtype)
        es = 4 if dtype == "f32" else 8
        for rule, (fields, kernel, slot_bytes) in RULES.items():
            cfg = Config(n_nodes=a.n, topology="csr", termination="fixed", max_rounds=a.rounds + a.warmup, seed=12,
                         dtype=dtype, **fields)
            sides = {"plain": (None, kernel + "<32,csr>"), "full": (full, kernel + "<32,csr,sched>")}
            if rule == "pushsum_hold":
                sides["phase"] = (phase, kernel + "<32,csr,sched>")
            us = {side: [] for side in sides}
            final = {}
            for rep in range(a.reps):
                for side, (sch, want) in sides.items():
                    t, name, final[side] = timed_run(cfg, (rp, ci), w, sch, a.rounds, a.warmup, want)
                    us[side].append(t)
                    out.append({"dtype": dtype, "rule": rule, "side": side, "rep": rep, "us_per_round": round(t, 3),
                                "kernel": name})
                    print(out[-1], flush=True)
                assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(final["plain"], final["full"])), \
                    "full masks: final values differ from the unscheduled handle's"
            med = {side: statistics.median(v) for side, v in us.items()}
            rec = {"summary": True, "dtype": dtype, "rule": rule,
                   "ratio_full": round(med["full"] / med["plain"], 4),
                   "byte_ratio_expected": round((slot_bytes(es) + 4) / slot_bytes(es), 4),
                   "final_values_bit_identical": True}
            for side, v in us.items():
                rec[side + "_us_median"] = round(med[side], 3)
                rec[side + "_us_minmax"] = [round(min(v), 3), round(max(v), 3)]
            if "phase" in med:
                rec["ratio_phase"] = round(med["phase"] / med["plain"], 4)
            out.append(rec)
            print(rec, flush=True)
    with open(a.out, "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
