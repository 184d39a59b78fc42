#!/usr/bin/env python3
"""Kernel names of one handle per creation branch (csrc/create.hip), and the recorder of
tests/golden/kernel_names.json.

    python tools/record_kernel_names.py tests/golden/kernel_names.json     (needs the GPU)

CASES is shared with tests/test_gpu_kernel_names.py.  Every case creates one handle, reads
kernel_name() and runs no round.  The golden file is recorded from a build of the commit BEFORE a
change to handle creation, never from the changed code: the test then pins every name against it.

A case is (name, kind, config, graph, environment):
  kind    "plain" (acs_create), ("parts", P) (P virtual partitions), "csr", "weighted" or "pushsum"
  graph   None, or (builder name, arguments) in GRAPHS
Every ACSIM_* knob in KNOBS that a case does not set is unset while its handle is created.
"""
import contextlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximate-consensus-simulation_amd"))

KNOBS = ("ACSIM_BINNED", "ACSIM_BIN_SA", "ACSIM_BIN_SB", "ACSIM_BIN_SPLIT", "ACSIM_BIN_PACK", "ACSIM_BIN_POL",
         "ACSIM_BIN_MIMG", "ACSIM_BIN_AWG", "ACSIM_BIN_NOFIX", "ACSIM_BIN_NARROW", "ACSIM_BIN_TS", "ACSIM_MFMA",
         "ACSIM_DEFER_FIN", "ACSIM_EPS_PUB", "ACSIM_DENSE_PERSIST", "ACSIM_CSR_FAST", "ACSIM_XCHUNKS",
         "ACSIM_BATCH_SPLIT")


@contextlib.contextmanager
def env(**kw):
    """The knobs exactly as given: every knob not named is unset for the duration."""
    want = {k: None for k in KNOBS}
    want.update(kw)
    old = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------ graphs
def _skewed(n, dmin, dmax, seed):
    from acsim.graphs import skewed_csr
    return skewed_csr(n, dmin, dmax, seed)


def _power_law_hubs(n, seed):
    """tests/test_csr.py hub_graph: about 15 % of the rows above 32 entries, two above 8192."""
    from acsim.graphs import skewed_csr
    rowptr, _ = skewed_csr(n, 10, 12000, seed, alpha=2.6)
    deg = np.diff(rowptr.astype(np.int64))
    deg[[7, n // 2]] = [9000, 8200]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    rng = np.random.default_rng(seed + 1)
    return rowptr, rng.integers(0, n, size=int(rowptr[-1])).astype(np.uint32)


def _few_big_rows(n, hubs, seed):
    """tests/test_limits.py hub_csr: rows of 6..20 entries, `hubs` rows of 8500..12000."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(6, 21, size=n)
    deg[rng.choice(n, size=hubs, replace=False)] = rng.integers(8500, 12001, size=hubs)
    rowptr = np.zeros(n + 1, dtype=np.uint64)
    rowptr[1:] = np.cumsum(deg)
    return rowptr, rng.integers(0, n, size=int(rowptr[-1])).astype(np.uint32)


def _uniform(n, dmin, dmax, seed, head=()):
    """Uniform degrees in [dmin, dmax]; the first rows' degrees as given."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(dmin, dmax + 1, n)
    deg[:len(head)] = head
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    return rowptr, rng.integers(0, n, int(rowptr[-1])).astype(np.uint32)


GRAPHS = {"skewed": _skewed, "power_law_hubs": _power_law_hubs, "few_big_rows": _few_big_rows, "uniform": _uniform}
_graphs = {}


def graph(spec):
    key = repr(spec)
    if key not in _graphs:
        _graphs[key] = GRAPHS[spec[0]](*spec[1:])
    return _graphs[key]


def weights_of(rowptr, colidx, dtype):
    """Admissible weights for both weighted rules: 1 / (out-degree + 1) per sender (column sums at most 1
    in the config's dtype)."""
    from acsim.graphs import pushsum_weights
    return pushsum_weights(rowptr, colidx, dtype=dtype)


# ------------------------------------------------------------------------------------- cases
def _reg(n, d, rule="trimmed", trim=5, **kw):
    return dict(n_nodes=n, topology="regular", degree=d, rule=rule, trim=trim, termination="fixed", max_rounds=4,
                seed=5, **kw)


def _complete(n, b=1, rule="average", trim=0, **kw):
    return dict(n_nodes=n, n_instances=b, topology="complete", rule=rule, trim=trim, termination="fixed",
                max_rounds=4, seed=9, **kw)


def _csr(n, rule="trimmed", trim=5, **kw):
    return dict(n_nodes=n, topology="csr", rule=rule, trim=trim, termination="fixed", max_rounds=4, seed=8, **kw)


BYZ = dict(fault_model="byzantine", n_faulty=300, byz_strategy="random", byz_delta=0.1, loss_p=0.05)
CRASH = dict(fault_model="crash", n_faulty=600, crash_window=4, loss_p=0.1)
HUBS_W = ("uniform", 3000, 0, 40, 21, (0, 4, 8, 16, 32, 1, 3, 7, 15, 31, 33, 40))   # under a quarter above 32
NOHUB_W = ("uniform", 333, 0, 7, 23, (7, 5))
SK32 = ("skewed", 20000, 11, 32, 7)
PL = ("power_law_hubs", 20000, 43)

CASES = [
    # --- batched (N <= 64): plain / faulty, split factors, MFMA by mask_group and by switch, fp32
    ("batched_n16_plain", "plain", _complete(16, 8), None, {}),
    ("batched_n16_crash", "plain", _complete(16, 8, "midpoint", fault_model="crash", n_faulty=3, crash_window=3), None, {}),
    ("batched_n64_loss", "plain", _complete(64, 300, loss_p=0.2), None, {}),
    ("batched_n64_split2", "plain", _complete(64, 300, loss_p=0.2), None, {"ACSIM_BATCH_SPLIT": 2}),
    ("batched_n64_split4", "plain", _complete(64, 300, loss_p=0.2), None, {"ACSIM_BATCH_SPLIT": 4}),
    ("batched_n64_group16_mfma", "plain", _complete(64, 48, loss_p=0.2, mask_group=16), None, {}),
    ("batched_n64_group16_mfma_off", "plain", _complete(64, 48, loss_p=0.2, mask_group=16), None, {"ACSIM_MFMA": 0}),
    ("batched_n40_group32_offset", "plain", _complete(40, 100, loss_p=0.3, mask_group=32, instance_offset=32), None, {}),
    ("batched_n64_f32", "plain", _complete(64, 128, loss_p=0.2, dtype="f32"), None, {}),
    ("batched_n64_f32_group16", "plain", _complete(64, 48, loss_p=0.2, mask_group=16, dtype="f32"), None, {}),
    # --- dense: persistent, two-kernel by switch and by size, several instances
    ("dense_persist_n1024", "plain", _complete(1024, 1, "trimmed", 341), None, {}),
    ("dense_persist_n700_b5", "plain", _complete(700, 5, "trimmed", 200), None, {}),
    ("dense_persist_f32", "plain", _complete(1024, 1, "trimmed", 341, dtype="f32"), None, {}),
    ("dense_two_kernel_switch", "plain", _complete(1024, 1, "trimmed", 341), None, {"ACSIM_DENSE_PERSIST": 0}),
    ("dense_two_kernel_n8192", "plain", _complete(8192, 1, "trimmed", 100), None, {}),
    ("dense_b5_switch_off_goes_generic", "plain", _complete(700, 5, "trimmed", 200), None, {"ACSIM_DENSE_PERSIST": 0}),
    # --- register kernel
    ("regular_b10_clean", "plain", _reg(1000, 8, trim=2, n_instances=10), None, {}),
    ("regular_b10_crash", "plain", _reg(1000, 8, trim=2, n_instances=10, fault_model="crash", n_faulty=120,
                                        crash_window=4, loss_p=0.1), None, {}),
    ("regular_binned_off", "plain", _reg(30000, 32), None, {"ACSIM_BINNED": 0}),
    ("regular_binned_off_f32", "plain", _reg(30000, 32, dtype="f32"), None, {"ACSIM_BINNED": 0}),
    ("regular_delay2", "plain", _reg(30000, 16, delay_max=2), None, {"ACSIM_BIN_SA": 1024}),
    ("regular_tiny_default_sa", "plain", _reg(1000, 8, trim=2), None, {}),
    # --- binned, one level
    ("bin_d32_default", "plain", _reg(50001, 32), None, {"ACSIM_BIN_SA": 1024}),
    ("bin_d32_narrow_off", "plain", _reg(50001, 32), None, {"ACSIM_BIN_SA": 1024, "ACSIM_BIN_NARROW": 0}),
    ("bin_d32_pack_off", "plain", _reg(50001, 32), None, {"ACSIM_BIN_SA": 1024, "ACSIM_BIN_PACK": 0}),
    ("bin_d32_one_pass", "plain", _reg(50001, 32), None, {"ACSIM_BIN_SA": 1024, "ACSIM_BIN_SPLIT": 1}),
    ("bin_d32_three_pass_narrow_refused", "plain", _reg(50001, 32), None, {"ACSIM_BIN_SA": 1024, "ACSIM_BIN_SPLIT": 3}),
    ("bin_d32_sa16k", "plain", _reg(65536, 32), None, {}),
    ("bin_d32_sb128", "plain", _reg(40000, 32), None, {"ACSIM_BIN_SA": 2048, "ACSIM_BIN_SB": 128}),
    ("bin_d32_defer_fin_off", "plain", _reg(40000, 32), None, {"ACSIM_BIN_SA": 2048, "ACSIM_DEFER_FIN": 0}),
    ("bin_d32_eps_pub_off", "plain", _reg(40000, 32), None, {"ACSIM_BIN_SA": 2048, "ACSIM_EPS_PUB": 0}),
    ("bin_d16_avg", "plain", _reg(30011, 16, "average", 0), None, {"ACSIM_BIN_SA": 1024}),
    ("bin_d8_mid", "plain", _reg(12345, 8, "midpoint", 2), None, {"ACSIM_BIN_SA": 1024}),
    ("bin_d32_loss", "plain", _reg(30000, 32, loss_p=0.1), None, {"ACSIM_BIN_SA": 1024}),
    ("bin_d32_loss_split2", "plain", _reg(160000, 32, loss_p=0.1), None, {"ACSIM_BIN_SA": 2048}),
    ("bin_d32_byz_fixup", "plain", _reg(40000, 32, **BYZ), None, {"ACSIM_BIN_SA": 2048}),
    ("bin_d32_byz_tag", "plain", _reg(40000, 32, **BYZ), None, {"ACSIM_BIN_SA": 2048, "ACSIM_BIN_NOFIX": 1}),
    ("bin_d16_crash", "plain", _reg(30000, 16, "wmsr", **CRASH), None, {"ACSIM_BIN_SA": 1024}),
    ("bin_d32_byz_sb128", "plain", _reg(40000, 32, **BYZ), None, {"ACSIM_BIN_SA": 2048, "ACSIM_BIN_SB": 128}),
    ("bin_d32_f32", "plain", _reg(30000, 32, dtype="f32"), None, {"ACSIM_BIN_SA": 1024}),
    ("bin_d16_f32_split2", "plain", _reg(30011, 16, "wmsr", dtype="f32"), None, {"ACSIM_BIN_SA": 512, "ACSIM_BIN_SPLIT": 2}),
    ("bin_d32_f32_crash", "plain", _reg(30000, 32, dtype="f32", **CRASH), None, {"ACSIM_BIN_SA": 1024}),
    # --- binned, two levels
    ("bin2_d16", "plain", _reg(100000, 16), None, {"ACSIM_BIN_SA": 256}),
    ("bin2_d32_mid", "plain", _reg(150001, 32, "midpoint"), None, {"ACSIM_BIN_SA": 512}),
    ("bin2_d16_crash", "plain", _reg(100000, 16, **CRASH), None, {"ACSIM_BIN_SA": 256}),
    ("bin2_d16_byz_tag", "plain", _reg(100000, 16, **BYZ), None, {"ACSIM_BIN_SA": 256, "ACSIM_BIN_NOFIX": 1}),
    ("bin2_d16_f32", "plain", _reg(100000, 16, dtype="f32"), None, {"ACSIM_BIN_SA": 256}),
    # --- virtual partitions: chunked exchange, its switch, shapes it refuses, faulty, two levels,
    #     and the plan refused once laid out (every partition back on the register kernel)
    ("parts2_xchunks4", ("parts", 2), _reg(1 << 18, 16), None, {"ACSIM_BIN_SA": 1024}),
    ("parts2_xchunks_off", ("parts", 2), _reg(1 << 18, 16), None, {"ACSIM_BIN_SA": 1024, "ACSIM_XCHUNKS": 0}),
    ("parts4_xchunks2", ("parts", 4), _reg(1 << 18, 16), None, {"ACSIM_BIN_SA": 1024, "ACSIM_XCHUNKS": 2}),
    ("parts2_sa64_chunked", ("parts", 2), _reg(6144, 16), None, {"ACSIM_BIN_SA": 64, "ACSIM_XCHUNKS": 4}),
    ("parts2_sa64_ragged_unchunked", ("parts", 2), _reg(3000, 16), None, {"ACSIM_BIN_SA": 64, "ACSIM_XCHUNKS": 4}),
    ("parts3_crash", ("parts", 3), _reg(45000, 16, **CRASH), None, {"ACSIM_BIN_SA": 512}),
    ("parts3_two_level", ("parts", 3), _reg(100000, 16), None, {"ACSIM_BIN_SA": 256}),
    ("parts2_d32_no_narrow", ("parts", 2), _reg(50001, 32), None, {"ACSIM_BIN_SA": 1024}),
    ("parts2_binned_off", ("parts", 2), _reg(50001, 32), None, {"ACSIM_BINNED": 0}),
    ("parts3_plan_refused", ("parts", 3), _reg(46081, 8, "average", 0), None, {"ACSIM_BIN_SA": 256}),
    # --- CSR: compiled degree, hub rows, fp32, the generic path
    ("csr_fast_binned", "csr", _csr(20000), SK32, {"ACSIM_BIN_SA": 1024}),
    ("csr_fast_per_lane", "csr", _csr(20000), SK32, {"ACSIM_BINNED": 0}),
    ("csr_fast_default_sa", "csr", _csr(20000), SK32, {}),
    ("csr_fast_d8_byz_binned", "csr", _csr(20000, "midpoint", 2, **BYZ), ("skewed", 20000, 5, 8, 7), {"ACSIM_BIN_SA": 1024}),
    ("csr_fast_d16_crash_binned", "csr", _csr(20000, "average", 0, **CRASH), ("skewed", 20000, 3, 16, 7), {"ACSIM_BIN_SA": 1024}),
    ("csr_fast_f32", "csr", _csr(5000, dtype="f32"), ("skewed", 5000, 11, 16, 9), {"ACSIM_BIN_SA": 1024}),
    ("csr_fast_b3_delay2", "csr", _csr(5000, n_instances=3, delay_max=2), ("skewed", 5000, 11, 16, 9), {}),
    ("csr_hubs_binned", "csr", _csr(20000), PL, {"ACSIM_BIN_SA": 1024}),
    ("csr_hubs_binned_loss", "csr", _csr(20000, loss_p=0.2), PL, {"ACSIM_BIN_SA": 1024}),
    ("csr_hubs_per_lane", "csr", _csr(20000), PL, {"ACSIM_BINNED": 0}),
    ("csr_hubs_default_sa", "csr", _csr(20000), PL, {}),
    ("csr_hubs_f32", "csr", _csr(20000, dtype="f32"), PL, {"ACSIM_BIN_SA": 1024}),
    ("csr_fast_off_generic", "csr", _csr(20000), SK32, {"ACSIM_CSR_FAST": 0}),
    ("csr_generic_big_rows", "csr", _csr(20000, trim=2), ("few_big_rows", 20000, 7, 37), {"ACSIM_CSR_FAST": 0}),
    ("csr_hubs_above_quarter_generic", "csr", _csr(3000, "average", 0), ("uniform", 3000, 20, 60, 3), {}),
    # --- rules WEIGHTED and PUSHSUM: with and without hub rows, fp32, the generic path
    ("weighted_hubs", "weighted", _csr(3000, "weighted", 0), HUBS_W, {}),
    ("weighted_hubs_f32", "weighted", _csr(3000, "weighted", 0, dtype="f32"), HUBS_W, {}),
    ("weighted_d8", "weighted", _csr(333, "weighted", 0, loss_p=0.2), NOHUB_W, {}),
    ("weighted_generic", "weighted", _csr(3000, "weighted", 0), HUBS_W, {"ACSIM_CSR_FAST": 0}),
    ("weighted_binned_knobs_ignored", "weighted", _csr(3000, "weighted", 0), HUBS_W, {"ACSIM_BIN_SA": 64}),
    ("pushsum_hubs", "pushsum", _csr(3000, "pushsum", 0), HUBS_W, {}),
    ("pushsum_hubs_f32", "pushsum", _csr(3000, "pushsum", 0, dtype="f32"), HUBS_W, {}),
    ("pushsum_d8", "pushsum", _csr(333, "pushsum", 0), NOHUB_W, {}),
    ("pushsum_generic", "pushsum", _csr(3000, "pushsum", 0), HUBS_W, {"ACSIM_CSR_FAST": 0}),
    # --- generic kernels on complete / regular graphs
    ("generic_complete_delay", "plain", _complete(100, 1, delay_max=1), None, {}),
    ("generic_complete_b3_loss", "plain", _complete(5000, 3, loss_p=0.3), None, {}),
    ("generic_regular_d10", "plain", _reg(1000, 10, trim=2), None, {}),
    ("generic_regular_d10_f32", "plain", _reg(1000, 10, trim=2, dtype="f32"), None, {}),
    ("big_m_complete_8300_loss", "plain", _complete(8300, 1, loss_p=0.3), None, {}),
    ("big_m_complete_8300_clean", "plain", _complete(8300, 1, "trimmed", 100), None, {}),
    ("big_m_complete_8300_f32_delay", "plain", _complete(8300, 1, "trimmed", 60, dtype="f32", delay_max=2), None, {}),
]


def kernel_name(case):
    """Create the case's handle and return its kernel_name(); no round runs."""
    import acsim
    from acsim.config import Config
    name, kind, cfg_kw, gspec, envs = case
    cfg = Config(**cfg_kw)
    kw = {}
    if isinstance(kind, tuple):
        kw["partitions"] = kind[1]
    elif kind != "plain":
        rowptr, colidx = graph(gspec)
        kw["csr"] = (rowptr, colidx)
        if kind in ("weighted", "pushsum"):
            kw["weights"] = weights_of(rowptr, colidx, cfg_kw.get("dtype", "f64"))
    with env(**envs), acsim.Simulator(cfg, device=0, **kw) as g:
        return g.kernel_name()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out = {}
    for case in CASES:
        out[case[0]] = kernel_name(case)   # (a case that cannot be created is an error: nothing is written)
        print(f"{case[0]:40s} {out[case[0]]}", flush=True)
    assert len(out) == len(CASES), "case names must be unique"
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
