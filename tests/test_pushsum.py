"""Rule "pushsum" (DESIGN.md §9): push-sum / ratio consensus on directed CSR graphs.

CPU part: the ABI and its validation, the numpy restatement (spec_pushsum_np) against the unchanged
oracle and against the restatement of rule "weighted" through the three exactness consequences of
the spec, the mean property, and the graph helpers.
GPU part: k_round_pushsum<D> (+ k_round_generic for hub rows) and the all-generic path
(ACSIM_CSR_FAST=0) against the restatement, bit for bit in x, the (s, z) pairs, rounds, converged
flags and the spread trace.
"""
import contextlib
import ctypes as C
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import acsim
from acsim import _abi
from acsim import graphs as G
from acsim.config import Config
from spec_pushsum_np import NpPushSumSim
from spec_weighted_np import NpWeightedSim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------- ABI, validation
def test_header_abi_module_and_library_agree(acsim_lib):
    hdr = open(os.path.join(ROOT, "include", "acsim.h")).read()
    assert int(re.search(r"#define\s+ACS_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4
    assert acsim_lib.acs_abi_version() == 4 == _abi.ABI_VERSION
    assert int(re.search(r"#define\s+ACS_RULE_PUSHSUM\s+(\d+)", hdr).group(1)) == 6 == _abi.RULE_PUSHSUM
    for name in ("acs_get_pushsum_state", "acs_set_pushsum_state"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(acsim_lib, name), name
    assert Config(rule="pushsum").to_c().rule == 6 == Config(rule="push_sum").to_c().rule


def _create(lib, cfg, rp, ci, ws, we):
    c = cfg.to_c()
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    rp = np.ascontiguousarray(rp, dtype=np.uint64)
    ci = np.ascontiguousarray(ci, dtype=np.uint32)
    ws = np.ascontiguousarray(ws, dtype=np.float64)
    we = np.ascontiguousarray(we, dtype=np.float64)
    rc = lib.acs_create_csr_weighted(C.byref(c), rp.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     ci.ctypes.data_as(C.POINTER(C.c_uint32)), ws.ctypes.data_as(dp),
                                     we.ctypes.data_as(dp), 0, C.byref(h))
    if rc == _abi.OK:
        lib.acs_destroy(h)
    return rc, lib.acs_last_error().decode()


def _small():
    rp, ci = G.random_csr(100, 1, 8, 2)
    return (rp, ci) + G.pushsum_weights(rp, ci)


PCFG = dict(n_nodes=100, topology="csr", rule="pushsum")


def _bump(ws, j, by):
    ws = ws.copy()
    ws[j] += by
    return ws


REJECT = [
    ("trim_1", _abi.EINVAL, dict(trim=1), None),
    ("crash", _abi.EINVAL, dict(fault_model="crash", n_faulty=3, crash_window=4), None),
    ("byzantine", _abi.EINVAL, dict(fault_model="byzantine", n_faulty=3), None),
    ("loss_self", _abi.EINVAL, dict(loss_p=0.1), None),
    ("delay", _abi.EUNSUPPORTED, dict(delay_max=1), None),
    ("column_sum", _abi.EINVAL, dict(), lambda ws: _bump(ws, 17, 2.0 ** -20)),
    ("f32_rounds", _abi.EINVAL, dict(dtype="f32", max_rounds=(1 << 22) + 1), None),
]


@pytest.mark.parametrize("name,code,kw,wfix", REJECT, ids=[r[0] for r in REJECT])
def test_pushsum_create_rejects(acsim_lib, name, code, kw, wfix):
    rp, ci, ws, we = _small()
    if wfix:
        ws = wfix(ws)
    rc, msg = _create(acsim_lib, Config(**{**PCFG, **kw}), rp, ci, ws, we)
    assert rc == code, (rc, msg)
    assert msg
    if name == "loss_self":
        assert "SELF" in msg and "mass" in msg   # the message says why
    if name == "column_sum":
        assert "column sum" in msg and "sender 17" in msg


def _ok(rc, msg):   # validation passed: the handle exists, or the machine has no GPU to make one on
    return rc == _abi.OK or (rc == _abi.EDEVICE and "no HIP device" in msg)


def test_valid_pushsum_configs_pass_validation(acsim_lib):
    rp, ci, ws, we = _small()
    for kw in (dict(), dict(loss_p=0.3, missing_policy="omit"), dict(missing_policy="omit"),
               dict(n_instances=3, mask_group=2, instance_offset=9)):
        assert _ok(*_create(acsim_lib, Config(**{**PCFG, **kw}), rp, ci, ws, we)), kw
    # fp32 handles hold binary32 weights: 1 / (outdeg + 1) is rounded and stepped in binary32 for them
    f32 = Config(**PCFG, dtype="f32", max_rounds=1 << 22)
    assert _ok(*_create(acsim_lib, f32, rp, ci, *G.pushsum_weights(rp, ci, dtype="f32")))
    rc, msg = _create(acsim_lib, f32, rp, ci, ws, we)   # the float64 weights round up past 1 in some column
    assert rc == _abi.EINVAL and "after rounding to binary32" in msg, (rc, msg)
    # a column sum inside the admitted 1 + 2^-30 (the exact sums of pushsum_weights are <= 1)
    assert _ok(*_create(acsim_lib, Config(**PCFG), rp, ci, _bump(ws, 17, 2.0 ** -31), we))
    # rule "weighted" is still served by the same entry point, with no column rule
    assert _ok(*_create(acsim_lib, Config(**{**PCFG, "rule": "weighted"}), rp, ci, _bump(ws, 17, 0.25), we))


def test_other_entry_points_reject_rule_6(acsim_lib):
    rp, ci, _, _ = _small()
    h = C.c_void_p()
    c = Config(**PCFG).to_c()
    rc = acsim_lib.acs_create_csr(C.byref(c), rp.ctypes.data_as(C.POINTER(C.c_uint64)),
                                  ci.ctypes.data_as(C.POINTER(C.c_uint32)), 0, C.byref(h))
    assert rc == _abi.EINVAL and acsim_lib.acs_last_error()
    for topo in (dict(topology="csr"), dict(topology="complete"), dict(topology="random_regular", degree=8)):
        c = Config(n_nodes=100, rule="pushsum", **topo).to_c()
        rc = acsim_lib.acs_create(C.byref(c), _abi.BACKEND_HIP, (C.c_int * 1)(0), 1, C.byref(h))
        assert rc == _abi.EINVAL and acsim_lib.acs_last_error(), topo
    rc, msg = _create(acsim_lib, Config(**{**PCFG, "rule": "average"}), *_small())
    assert rc == _abi.EINVAL and msg


def test_row_above_8192_entries_is_unsupported(acsim_lib):
    n = 9000
    deg = np.full(n, 2)
    deg[17] = 8192   # m = 8193 > kGenericMaxM
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    ci = (np.arange(int(rp[-1])) % n).astype(np.uint32)
    rc, msg = _create(acsim_lib, Config(n_nodes=n, topology="csr", rule="pushsum"), rp, ci, *G.pushsum_weights(rp, ci))
    assert rc == _abi.EUNSUPPORTED and "8192" in msg, (rc, msg)


# -------------------------------------------------------------------------------- graph helpers
def test_pushsum_weights_have_exact_column_sums_at_most_one():
    rp, ci = G.random_csr(2000, 1, 12, 3)
    ws, we = G.pushsum_weights(rp, ci)
    k = np.bincount(ci, minlength=2000) + 1
    assert np.array_equal(we, ws[ci])
    lowered = 0
    for j in range(2000):
        w = Fraction(float(ws[j]))
        assert w * int(k[j]) <= 1, j                       # the exact column sum
        near = 1.0 / k[j]
        assert ws[j] in (near, np.nextafter(near, 0.0)), j
        lowered += ws[j] != near
        assert (Fraction(float(np.nextafter(ws[j], 1.0))) * int(k[j]) > 1), j   # and no lower than needed
    assert lowered > 0   # e.g. 5 * fl(1/5) > 1: the one-ulp step is exercised
    cs = G.column_sums(rp, ci, ws, we)
    assert cs.shape == (2000,) and cs.max() <= 1.0 and cs.min() >= 1.0 - 2.0 ** -50
    # column_sums is a correctly rounded sum of what it is given
    ws2 = ws.copy()
    ws2[5] += 2.0 ** -20
    assert G.column_sums(rp, ci, ws2, we)[5] > 1.0 + 2.0 ** -21
    ws32, we32 = G.pushsum_weights(rp, ci, dtype="f32")
    assert np.array_equal(ws32.astype(np.float32), ws32) and np.array_equal(we32, ws32[ci])
    assert all(Fraction(float(ws32[j])) * int(k[j]) <= 1 for j in range(2000))
    assert np.abs(ws32 * k - 1).max() <= 2.0 ** -22


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "acsim", *args], capture_output=True, text=True,
                          cwd=os.path.join(ROOT, "approximate-consensus-simulation_amd"))


def test_cli_says_which_weights_it_used(tmp_path):
    rp, ci = G.random_csr(200, 1, 9, 9)
    G.save_csr(str(tmp_path / "g.npz"), rp, ci)
    sets = ["--set", "rule=pushsum", "--set", "fault_model=none", "--set", "n_faulty=0"]
    r = _cli("validate", "--graph", str(tmp_path / "g.npz"), *sets)
    assert r.returncode == 0 and "pushsum_weights" in r.stderr, r.stderr
    ws, we = G.pushsum_weights(rp, ci)
    ws[3] += 0.5
    G.save_csr(str(tmp_path / "w.npz"), rp, ci, weights=(ws, we))
    r = _cli("validate", "--graph", str(tmp_path / "w.npz"), *sets)
    assert r.returncode == 1 and "using the weights of" in r.stderr and "column sum" in r.stderr, r.stderr


# ------------------------------------------------- consequence 1: the oracle's `average`, bit for bit
def circulant(n, d):
    """Receiver i hears i+1 .. i+d (mod n): every row has d + 1 entries, every node d + 1 listeners
    (itself included), so with all weights 1 / (d + 1) every row sum and column sum is 1."""
    rp = (np.arange(n + 1) * d).astype(np.uint64)
    ci = ((np.arange(n)[:, None] + 1 + np.arange(d)[None, :]) % n).astype(np.uint32).reshape(-1)
    w = 1.0 / (d + 1)
    return rp, ci, (np.full(n, w), np.full(ci.size, w))


def circ_cfg(dtype):
    return Config(n_nodes=301, topology="csr", rule="pushsum", eps=1e-9 if dtype == "f64" else 1e-5, max_rounds=80,
                  seed=41, trace_spread=True, dtype=dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("d", [3, 7, 15, 31])
def test_power_of_two_rows_equal_the_oracles_average(oracle_mod, d, dtype):
    """Rows of 2^k entries weighing 2^-k: every product is exact, z stays exactly 1 and s / 1 = s is
    the plain average's tree sum times 2^-k, i.e. tree_sum / m, in every round."""
    rp, ci, w = circulant(301, d)
    cfg = circ_cfg(dtype)
    n = NpPushSumSim(cfg, (rp, ci), w)
    with oracle_mod.OracleSimulator(cfg.replace(rule="average"), csr=(rp, ci)) as o:
        while not n.done[0]:
            n.round(1)
            o.round(1)
            assert np.all(n.z[0] == 1.0)
            assert np.array_equal(bits(o.values(0)), bits(n.x[0])), int(n.rounds[0])
        assert np.array_equal(o.rounds(), n.rounds) and n.rounds[0] > 3
        assert np.array_equal(o.spread_trace(0), np.array(n.trace[0], dtype=np.float64))


# --------------------------------------------------- consequences 2 and 3: against rule "weighted"
N_BIG = 3001   # not a multiple of 64 or 256: the last SELL slice and the last block are partial


def big_graph():
    """Degrees 0..40: rows with no senders, every width up to D = 32, and hub rows above it (8 of
    41 degrees: under a quarter of the rows, so the fast path keeps D = 32 and the hubs go generic)."""
    rp, ci = G.random_csr(N_BIG, 0, 40, 7)
    deg = np.diff(rp.astype(np.int64))
    assert (deg == 0).any() and 0 < (deg > 32).sum() * 4 <= N_BIG
    return rp, ci


def heard_graph():
    """big_graph with one sender given to every row that had none: with positive weights every x_i
    then moves, so the spread can fall to eps (a row with no senders keeps x_i^0 for ever:
    s and z shrink by the same w_self)."""
    rp, ci = big_graph()
    deg = np.diff(rp.astype(np.int64))
    rng = np.random.default_rng(71)
    rows = [np.concatenate([ci[int(rp[i]):int(rp[i + 1])], rng.integers(0, N_BIG, 1 if deg[i] == 0 else 0)])
            for i in range(N_BIG)]
    rp2 = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.uint64)
    return rp2, np.concatenate(rows).astype(np.uint32)


def random_ps_weights(rp, ci, seed):
    """Random weights in [0, 1] with exact zeros (about 6 % of the edges, 12 % of w_self; an all-zero
    row gets w_self = 0.5), then every column with a sum above 1 is scaled down to sum to
    1 / (1 + 2^-20) at most: under the 1 + 2^-30 of the rule in fp64 and after rounding to binary32."""
    rng = np.random.default_rng(seed)
    n, nnz = rp.size - 1, int(rp[-1])
    ws, we = rng.random(n), rng.random(nnz)
    ws[rng.random(n) < 0.12] = 0.0
    we[rng.random(nnz) < 0.06] = 0.0
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    ws[(ws + np.bincount(rows, weights=we, minlength=n)) == 0] = 0.5
    col = ws + np.bincount(ci, weights=we, minlength=n)
    f = 1.0 / (np.maximum(col, 1.0) * (1.0 + 2.0 ** -20))
    f[col <= 1.0] = 1.0
    ws, we = ws * f, we * f[ci]
    assert (ws == 0).any() and (we == 0).any() and G.column_sums(rp, ci, ws, we).max() <= 1.0
    return ws, we


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_first_round_is_weighteds_and_later_rounds_are_not(dtype):
    rp, ci = big_graph()
    w = random_ps_weights(rp, ci, 8)
    cfg = Config(n_nodes=N_BIG, topology="csr", rule="pushsum", loss_p=0.4, missing_policy="omit",
                 termination="fixed", max_rounds=5, seed=43, dtype=dtype)
    p = NpPushSumSim(cfg, (rp, ci), w)
    q = NpWeightedSim(cfg.replace(rule="weighted"), (rp, ci), w)
    p.round(1)
    q.round(1)
    # from z = 1 the z sum is the weight sum of the present entries: the same divide, the same keep
    assert np.array_equal(bits(p.x[0]), bits(q.x[0]))
    assert p.kept[0][0] == q.zero_den > 0   # rows that kept x_i because nothing with weight arrived
    p.round(4)
    q.round(4)
    assert np.count_nonzero(bits(p.x[0]) != bits(q.x[0])) > N_BIG // 2   # consequence 3: not the same rule


# ----------------------------------------------------------------------------- the mean property
def test_pushsum_finds_the_mean_on_a_directed_graph_and_the_other_rules_do_not(oracle_mod):
    """Directed graph, weights 1 / (outdeg + 1), eps = 1e-12.  Every x_i ends within
        B = eps + 2 R (ceil(log2 m_max) + k_max + 4) 2^-53 max|x^0|
    of fsum(x^0) / N (R rounds run, k_max = largest out-degree + 1).  Derivation:
    (1) x_i = s_i / z_i, so S / Z = sum_i z_i x_i / sum_i z_i (S = sum s, Z = sum z, exact sums) is a
        weighted mean of the x_i with weights z_i >= 0: it lies between min x and max x, and at the
        end these are eps apart, so |x_i - S / Z| <= eps (up to the one rounding of each divide,
        which the + 4 below covers).
    (2) In exact arithmetic a round multiplies sender j's mass by its column sum c_j.  The weights
        are 1 / k_j rounded and at most one ulp lower, so 1 - 3 * 2^-53 <= c_j <= 1: the k_j equal
        weights are each off by at most 3 * 2^-53 / k_j, which moves sum |s| by at most
        3 * 2^-53 sum |s| per round (the bound's k_max + 4 allows for more than that).  Each s_i'
        is a product rounding and a tree sum of ceil(log2 m_i) levels: relative error
        (ceil(log2 m_max) + 1) 2^-53 on sum_e |p_e|.  Per round,
        |S' - S| <= (ceil(log2 m_max) + k_max + 4) 2^-53 sum |s|, and sum |s| <= N max|x^0|
        (column sums <= 1; x^0 >= 0 here); the same holds for Z against N.
    (3) After R rounds S / N has moved from the mean by at most R (..) 2^-53 max|x^0| and Z / N from 1
        by R (..) 2^-53; the ratio S / Z by at most twice that (max|x^0| <= 1 scales the Z term).
    `average` and row-normalised `weighted` on the same inputs converge too, but to another number."""
    n = 2000
    rp, ci = G.random_csr(n, 1, 12, 3)
    ws, we = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=n, topology="csr", rule="pushsum", eps=1e-12, max_rounds=500, seed=44)
    p = NpPushSumSim(cfg, (rp, ci), (ws, we))
    x0 = p.x[0].copy()
    mean = math.fsum(x0) / n
    p.run()
    R = int(p.rounds[0])
    m_max = int(np.diff(rp.astype(np.int64)).max()) + 1
    k_max = int(np.bincount(ci, minlength=n).max()) + 1
    B = cfg.eps + 2 * R * (math.ceil(math.log2(m_max)) + k_max + 4) * 2.0 ** -53 * float(np.abs(x0).max())
    err = float(np.abs(p.x[0] - mean).max())
    print(f"pushsum: {R} rounds, max |x - mean| = {err:.3e}, bound {B:.3e}")
    assert p.converged[0] and R < 500
    assert err <= B
    wn = NpWeightedSim(cfg.replace(rule="weighted"), (rp, ci), (ws, we))
    wn.run()
    werr = float(np.abs(wn.x[0] - mean).min())
    with oracle_mod.OracleSimulator(cfg.replace(rule="average"), csr=(rp, ci)) as o:
        o.run()
        aerr, ar = float(np.abs(o.values(0) - mean).min()), int(o.rounds()[0])
    print(f"weighted: {int(wn.rounds[0])} rounds, {werr:.3e} away; average: {ar} rounds, {aerr:.3e} away")
    assert wn.converged[0] and werr > 1e-6 and aerr > 1e-6


# ------------------------------------------------------------------------------------------ GPU
GPU_CASES = {
    "lossless_fixed": dict(termination="fixed", max_rounds=30),
    "loss_omit_fixed": dict(termination="fixed", max_rounds=30, loss_p=0.4, missing_policy="omit"),
    "eps": dict(eps=1e-9, max_rounds=200),
    "inst3_group2_offset": dict(n_instances=3, mask_group=2, instance_offset=5, loss_p=0.3, missing_policy="omit",
                                eps=1e-9, max_rounds=200),
    "f32": dict(dtype="f32", termination="fixed", max_rounds=30, loss_p=0.2, missing_policy="omit"),
}
PATHS = {"fast": {}, "generic": {"ACSIM_CSR_FAST": 0}}
_ref = {}


def gpu_cfg(name, **over):
    return Config(**{**dict(n_nodes=N_BIG, topology="csr", rule="pushsum", seed=45, trace_spread=True),
                     **GPU_CASES[name], **over})


def gpu_inputs(name):
    """FIXED cases: big_graph (rows with no senders) and random weights with exact zeros.  EPS cases:
    heard_graph and the all-positive 1 / (outdeg + 1), on which the spread does reach eps."""
    if GPU_CASES[name].get("termination") == "fixed":
        rp, ci = big_graph()
        return rp, ci, random_ps_weights(rp, ci, 8)
    rp, ci = heard_graph()
    return rp, ci, G.pushsum_weights(rp, ci)


def reference(name):
    """The restatement's run of one case, computed once and shared by both paths."""
    if name not in _ref:
        rp, ci, w = gpu_inputs(name)
        n = NpPushSumSim(gpu_cfg(name), (rp, ci), w)
        n.run()
        _ref[name] = n
    return _ref[name]


def kname(path, f32, d=32, hubs=True):
    nm = f"k_round_pushsum<{d},csr>" + ("+k_round_generic(hubs)" if hubs else "") if path == "fast" else "k_round_generic"
    return nm + (" [f32]" if f32 else "")


def read_all(g):
    pairs = [g.pushsum_state(b) for b in range(g.B)]
    return dict(rounds=g.rounds(), conv=g.converged(), x=g.all_values(), s=np.stack([p[0] for p in pairs]),
                z=np.stack([p[1] for p in pairs]), trace=[g.spread_trace(b) for b in range(g.B)])


def assert_same(got, n):
    assert np.array_equal(got["rounds"], n.rounds)
    assert np.array_equal(got["conv"], n.converged)
    assert np.array_equal(bits(got["x"]), bits(n.x))
    assert np.array_equal(bits(got["s"]), bits(n.s))
    assert np.array_equal(bits(got["z"]), bits(n.z))
    for b in range(n.B):
        assert np.array_equal(got["trace"][b], np.array(n.trace[b], dtype=np.float64)), b


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_gpu_matches_restatement(name, path):
    rp, ci, w = gpu_inputs(name)
    cfg = gpu_cfg(name)
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
        assert g.kernel_name() == kname(path, cfg.dtype == "f32")
        g.run()
        got = read_all(g)
    n = reference(name)
    if cfg.loss_p > 0 and cfg.termination == "fixed":
        assert sum(n.kept[0]) > 0   # the z' = 0 keep was exercised
    if cfg.termination != "fixed":
        assert n.converged.all() and 10 < n.rounds.min() and n.rounds.max() < 200   # stopped by the eps test
    if name == "inst3_group2_offset":
        assert len(set((n.rounds % 2).tolist())) > 1   # instances end in different pair buffers
    assert_same(got, n)


def small_graph(dmax, seed):
    rng = np.random.default_rng(seed)
    n = 333
    deg = rng.integers(0, dmax + 1, n)
    deg[:2] = [dmax, 0]
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    ci = rng.integers(0, n, int(rp[-1])).astype(np.uint32)
    return rp, ci


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dmax,D", [(3, 4), (7, 8), (15, 16)])
def test_gpu_narrow_widths(dmax, D, path):
    rp, ci = small_graph(dmax, 50 + dmax)
    w = random_ps_weights(rp, ci, 9)
    cfg = Config(n_nodes=333, topology="csr", rule="pushsum", eps=1e-9, max_rounds=120, seed=46, loss_p=0.2,
                 missing_policy="omit", trace_spread=True)
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
        assert g.kernel_name() == kname(path, False, D, hubs=False)
        g.run()
        got = read_all(g)
    n = NpPushSumSim(cfg, (rp, ci), w)
    n.run()
    assert_same(got, n)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_f32_z_decays_through_subnormals_to_zero(path):
    """loss_p = 0.5 halves the mass about every round: within 200 rounds z passes through the
    binary32 subnormals to 0 everywhere, and x is kept from then on."""
    rng = np.random.default_rng(61)
    deg = rng.integers(8, 16, 333)   # 9 to 16 holders per unit of mass, half of them lost: about 0.54 per round
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    ci = rng.integers(0, 333, int(rp[-1])).astype(np.uint32)
    w = G.pushsum_weights(rp, ci, dtype="f32")
    cfg = Config(n_nodes=333, topology="csr", rule="pushsum", dtype="f32", termination="fixed", max_rounds=200, seed=47,
                 loss_p=0.5, missing_policy="omit", trace_spread=True)
    n = NpPushSumSim(cfg, (rp, ci), w)
    subnormal_rounds = 0
    for _ in range(200):
        n.round(1)
        subnormal_rounds += bool(((n.z[0] > 0) & (n.z[0] < np.float32(2.0 ** -126))).any())
    assert subnormal_rounds > 3 and np.all(n.z[0] == 0) and n.kept[0][-1] == 333
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
        g.run()
        got = read_all(g)
    assert_same(got, n)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_power_of_two_rows_equal_the_oracles_average(oracle_mod, dtype, path):
    rp, ci, w = circulant(301, 31)
    cfg = circ_cfg(dtype)
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
        assert g.kernel_name() == kname(path, dtype == "f32", 32, hubs=False)
        g.run()
        got = read_all(g)
    with oracle_mod.OracleSimulator(cfg.replace(rule="average"), csr=(rp, ci)) as o:
        o.run()
        assert np.array_equal(o.rounds(), got["rounds"])
        assert np.array_equal(bits(o.values(0)), bits(got["x"][0]))
        assert np.array_equal(o.spread_trace(0), got["trace"][0])
    assert np.all(got["z"] == 1.0) and np.array_equal(bits(got["s"]), bits(got["x"]))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_resume_and_stepping(path):
    rp, ci = big_graph()
    w = random_ps_weights(rp, ci, 8)
    cfg = gpu_cfg("loss_omit_fixed")
    n = reference("loss_omit_fixed")
    with env(**PATHS[path]):
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
            g.round(7)
            s7, z7 = g.pushsum_state(0)
            x7 = g.values(0)
            for k in (1, 5, 30):   # stepped round(k) ends where run() does
                g.round(k)
            stepped = read_all(g)
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:   # resume with the pairs
            g.set_pushsum_state(7, s7, z7)
            xr7 = g.values(0)
            g.run()
            resumed = read_all(g)
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:   # resume with x alone: z restarts at 1
            g.set_state(7, x7)
            s, z = g.pushsum_state(0)
            assert np.array_equal(bits(s), bits(x7)) and np.all(z == 1.0)
            g.run()
            from_x = read_all(g)
            with pytest.raises(Exception):
                g.set_pushsum_state(7, s7, -np.abs(z7) - 1.0)   # z < 0
        with acsim.Simulator(cfg.replace(rule="weighted"), csr=(rp, ci), weights=w) as g:
            with pytest.raises(Exception):   # the pair calls are push-sum's alone
                g.pushsum_state(0)
    assert_same(stepped, n)
    # The pairs never depend on x, so the resumed run's pairs are the uninterrupted run's.  x is
    # recomputed from the pairs at the resume: where z = 0 it is s (= 0), not the value the
    # uninterrupted run had kept, and it can differ later only where z is 0 again.
    assert (z7 == 0).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(bits(xr7), bits(np.where(z7 > 0, s7 / z7, s7)))
    assert np.array_equal(resumed["rounds"], stepped["rounds"])
    assert np.array_equal(bits(resumed["s"]), bits(stepped["s"])) and np.array_equal(bits(resumed["z"]), bits(stepped["z"]))
    live = stepped["z"] > 0
    assert np.array_equal(bits(resumed["x"][live]), bits(stepped["x"][live]))
    # and the whole resumed run is the restatement's, restarted the same way
    m = NpPushSumSim(cfg, (rp, ci), w)
    m.restart(7, s7, z7)
    m.run()
    assert_same({**resumed, "trace": [resumed["trace"][0][7:]]}, _tail(m, 7))
    m = NpPushSumSim(cfg, (rp, ci), w)
    m.restart(7, x7)
    m.run()
    assert_same({**from_x, "trace": [from_x["trace"][0][7:]]}, _tail(m, 7))
    assert not np.array_equal(bits(from_x["x"]), bits(stepped["x"]))   # z restarted at 1: another run


def _tail(m, k):
    """The restatement with its spread traces cut to the rounds from k on (a resumed handle has no
    earlier ones)."""
    m.trace = [tr[k:] for tr in m.trace]
    return m
