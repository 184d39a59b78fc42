"""bench.py as a command: a plain run (`--gpus 1 --steps K --warmup W`) times the headline only,
`--steps` sets the timed rounds, and `--dump-outputs DIR` writes what those rounds computed, bit for
bit the oracle's state after warm-up + timed rounds (the cfg4 shape at 2^17 nodes: the binned
exchange, several source blocks)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from acsim.config import preset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, WARM, STEPS = 1 << 17, 2, 3
LEG_KEYS = ("cfg4_f32", "cfg3_sharded", "cfg4_narrow", "cfg5_partitioned")


def run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARM), "--n-nodes", str(N), *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_plain_run_is_lean_and_dumps_what_it_computed(tmp_path, oracle_mod, dtype):
    out = tmp_path / "dump"
    d = run_bench("--dtype", dtype, "--dump-outputs", str(out))
    assert d["steps"] == STEPS and d["warmup"] == WARM and d["dtype"] == dtype and d["full"] is False
    assert d["unit"] == "node-rounds/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(N / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # nothing but the headline ran
    assert d["cpu_baseline"] is None and d["parity"]["golden_match"] is None and d["legs_failed"] == []
    assert not any(k in d for k in LEG_KEYS)
    assert sorted(os.listdir(out)) == ["round_info.npy", "values.npy"]
    x, info = np.load(out / "values.npy"), np.load(out / "round_info.npy")
    cfg = preset("cfg4", n_nodes=N, max_rounds=WARM + STEPS, dtype=dtype)
    with oracle_mod.OracleSimulator(cfg, threads=8) as o:
        o.round(WARM)
        oi = o.round(STEPS)
        ox = o.values(0)
    assert x.dtype == ox.dtype == (np.float32 if dtype == "f32" else np.float64)
    bits = np.uint32 if dtype == "f32" else np.uint64
    assert np.array_equal(x.view(bits), ox.view(bits))
    want = np.array([oi.round, oi.done, oi.spread, oi.lo, oi.hi, oi.instances_done], dtype=np.float64)
    assert info.dtype == np.float64 and np.array_equal(info.view(np.uint64), want.view(np.uint64))
    assert info[0] == WARM + STEPS
