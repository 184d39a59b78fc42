"""VALU share of cfg4's phase B by kind of round from one rocprofv3 --pmc
pass over tools/bench_configs.py cfg4 (one warm-up run of 100 FIXED rounds, then the timed run of 100;
counters SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES GRBM_GUI_ACTIVE, no
tracing in the same run).
usage: python tools/uniform_pmc_json.py <session dir> <out.json> <tag>...   (<session dir>/<tag>/ holds
the pass's counter_collection.csv)

Dispatches are ordered by Dispatch_Id; the timed run's k_bin_gather dispatches are 100-199: rounds
1-14 are 8-byte rounds, 15-39 4-byte, 40 on uniform (the same split as tools/narrow_traces_json.py).
valu_busy_frac = SQ_ACTIVE_INST_VALU x 4 / (1024 SIMDs x GRBM_GUI_ACTIVE / 8), as
tools/pmc_cfg3_json.py; valu_insts_per_wave = SQ_INSTS_VALU / SQ_WAVES.  Each figure is the median
over the class's dispatches."""
import collections
import csv
import glob
import json
import os
import statistics as st
import sys

CLASSES = {"rounds_1_14": (101, 115), "rounds_15_39": (115, 139), "rounds_40_99": (140, 200)}


def gather_dispatches(d):
    disp = collections.defaultdict(dict)
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_bin_gather" in r["Kernel_Name"]:
                disp[int(r["Dispatch_Id"])][r["Counter_Name"]] = float(r["Counter_Value"])
    return [disp[k] for k in sorted(disp)]


def main():
    d, out, tags = sys.argv[1], sys.argv[2], sys.argv[3:]
    res = {"what": " ".join(__doc__.split("\n\n")[1].split()), "runs": {}}
    for t in tags:
        g = gather_dispatches(os.path.join(d, t))
        run = {"gather_dispatches": len(g)}
        for name, (lo, hi) in CLASSES.items():
            rows = g[lo:hi]
            m = {c: st.median(r[c] for r in rows) for c in rows[0]}
            cyc = m["GRBM_GUI_ACTIVE"] / 8
            m["dispatch_cycles_per_xcd"] = cyc
            m["valu_busy_frac"] = st.median(r["SQ_ACTIVE_INST_VALU"] * 4 / (1024 * r["GRBM_GUI_ACTIVE"] / 8) for r in rows)
            m["valu_insts_per_wave"] = m["SQ_INSTS_VALU"] / m["SQ_WAVES"]
            run[name] = m
        res["runs"][t] = run
        print(t, {n: (round(run[n]["valu_busy_frac"], 3), round(run[n]["valu_insts_per_wave"], 1),
                      round(run[n]["dispatch_cycles_per_xcd"])) for n in CLASSES})
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
