#!/usr/bin/env python3
"""A/B of rule "weighted" on the binned exchange against its per-lane kernel.

Workload: the 2^20-node skewed graph of tools/weighted_ab.py (skewed_csr(2^20, 11, 32, seed 11)) with
the same random weights, 100 FIXED rounds.  In ONE process, alternating:
  A  ACSIM_BIN_WEIGHTED unset:  k_round_weighted<32,csr>
  B  ACSIM_BIN_WEIGHTED=1:      k_bin_scatter+k_bin_gather_w<32,csr>
first lossless, then with loss_p = 0.1 under missing_policy = omit.  Every round after 5 warm-up
rounds is bracketed by device events (set_kernel_timing).  Both kernel names are asserted, and so is
that the two sides' final values are bit-identical.  One record per run goes to the output file, then
one summary record per variant with the medians, their ranges, the ratio and the byte account.

    python tools/weighted_binned_ab.py --out profiles/weighted_binned_ab.jsonl [--reps 5] [--sha COMMIT]
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

import numpy as np  # noqa: E402

import acsim  # noqa: E402
from acsim.config import Config  # noqa: E402
from acsim.graphs import skewed_csr  # noqa: E402

NAMES = {"per_lane": "k_round_weighted<32,csr>", "binned": "k_bin_scatter+k_bin_gather_w<32,csr>"}


def timed_run(cfg, csr, weights, rounds, binned):
    if binned:
        os.environ["ACSIM_BIN_WEIGHTED"] = "1"   # read once per create
    else:
        os.environ.pop("ACSIM_BIN_WEIGHTED", None)
    with acsim.Simulator(cfg, csr=csr, weights=weights) as g:
        name = g.kernel_name()
        assert name == NAMES["binned" if binned else "per_lane"], name
        g.round(5)                       # warm-up: code objects loaded, clocks up
        g.set_kernel_timing(True)
        g.run()
        ms, n, _ = g.kernel_timing()
        assert n == rounds - 5, (n, rounds)
        return 1000.0 * ms / n, name, g.values(0)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--sha", default=None, help="commit measured (default: git rev-parse, where there is a checkout)")
    ap.add_argument("--box", default="MI355X (gfx950)")
    a = ap.parse_args()
    for k in ("ACSIM_BINNED", "ACSIM_BIN_SA"):   # the defaults on both sides
        os.environ.pop(k, None)
    rp, ci = skewed_csr(a.n, 11, 32, 11)
    rng = np.random.default_rng(12)
    ws, we = rng.random(a.n) * 0.5 + 0.25, rng.random(ci.size)
    deg = np.diff(rp.astype(np.int64))
    nnz = int(ci.size)
    # weight bytes of one round: the padded array cut at each lane's degree (32-byte groups of 4
    # columns), at each 64-row slice's widest row (the per-lane kernel), and in full
    grp_lane = int(((deg + 3) // 4).sum())
    pad = (-a.n) % 64
    grp_slice = int((np.concatenate([(deg + 3) // 4, np.zeros(pad, np.int64)]).reshape(-1, 64).max(axis=1) * 64).sum())
    sha = a.sha
    if sha is None:
        try:
            sha = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                 text=True).stdout.strip() or None
        except OSError:
            sha = None
    box = {"gpu": a.box, "runtime": acsim._abi.runtime_info()["versions"]}
    base = dict(n_nodes=a.n, topology="csr", rule="weighted", termination="fixed", max_rounds=a.rounds, seed=12)
    head = {"what": "per-round device us (HIP events around every round, rounds 6..%d of a FIXED run), rule weighted on "
                    "the per-lane kernel (ACSIM_BIN_WEIGHTED unset) vs the binned exchange (ACSIM_BIN_WEIGHTED=1), "
                    "alternating in one process; final values compared bit for bit" % a.rounds,
            "graph": "skewed_csr(%d, 11, 32, seed 11)" % a.n, "nnz": nnz, "mean_degree": round(nnz / a.n, 3),
            "dtype": "f64", "box": box, "sha": sha}
    recs = [head]
    for variant, kw in (("lossless", dict()), ("loss_0.1_omit", dict(loss_p=0.1, missing_policy="omit"))):
        cfg = Config(**base, **kw)
        us = {"per_lane": [], "binned": []}
        for rep in range(a.reps):
            x = {}
            for side in ("per_lane", "binned"):
                t, name, x[side] = timed_run(cfg, (rp, ci), (ws, we), a.rounds, side == "binned")
                us[side].append(t)
                recs.append({"variant": variant, "side": side, "rep": rep, "us_per_round": round(t, 3), "kernel": name})
                print(recs[-1], flush=True)
            assert np.array_equal(x["per_lane"].view(np.uint64), x["binned"].view(np.uint64)), "final values differ"
        ma, mb = statistics.median(us["per_lane"]), statistics.median(us["binned"])
        recs.append({"summary": True, "variant": variant, "final_values_bit_identical": True,
                     "per_lane_us_median": round(ma, 3), "binned_us_median": round(mb, 3),
                     "per_lane_us_minmax": [round(min(us["per_lane"]), 3), round(max(us["per_lane"]), 3)],
                     "binned_us_minmax": [round(min(us["binned"]), 3), round(max(us["binned"]), 3)],
                     "ratio_binned_over_per_lane": round(mb / ma, 4),
                     # per present slot.  Per-lane: 4 B id + 8 B weight + the x gather (8 B asked, a
                     # sector moved).  Binned, one level: 1.75 + 8 (phase A) + 8 + 2 (phase B) + the
                     # weight groups the lanes load (32 B each, padding columns included)
                     "bytes_per_slot_per_lane_excl_gather": 12,
                     "bytes_per_slot_binned": round(19.75 + 32.0 * grp_lane / nnz, 3),
                     "weight_MB_lane_predicate": round(32e-6 * grp_lane, 2),
                     "weight_MB_slice_width": round(32e-6 * grp_slice, 2),
                     "weight_MB_full_padding": round(8e-6 * 32 * a.n, 2)})
        print(recs[-1], flush=True)
    with open(a.out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
