"""Push-sum with per-round splitting ("Push-sum with per-round splitting"): rule "pushsum"
on a periodic link schedule with no weights; in round r, phase p = r mod P, sender j divides its pair by
c_p(j) = 1 + (its out-links that are up in phase p).  Every round's matrix is column-stochastic, so the
mean is kept with no per-link state.

CPU part: the two ABI symbols and their validation, graphs.split_shares against exact Fractions, the
four consequences of the rule on the numpy restatement (spec_pushsum_split_np), the CLI.
GPU part: k_round_pushsum_split<D,csr> (+ k_round_generic for hub rows) and the all-generic path
(ACSIM_CSR_FAST=0) against the restatement, bit for bit in x, the (s, z) pairs, rounds, converged flags
and the spread trace.
"""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import acsim
from acsim import _abi
from acsim import graphs as G
from acsim.config import Config
from hub_graphs import check_hub_class_graph, hub_class_graph
from spec_pushsum_np import NpPushSumSim
from spec_pushsum_split_np import NpPushSumSplitSim
from spec_sched_np import sched_sim
from test_link_schedule import (assert_same, assert_same_handles, env, random_masks, read_all,  # noqa: F401 (env: fixture)
                                same_runs)
from test_pushsum import PATHS, _cli, big_graph, bits, small_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64p, u32p, dblp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
SCFG = dict(n_nodes=100, topology="csr", rule="pushsum")


# ------------------------------------------------------------------------------- ABI, validation
def test_header_declares_and_library_exports_both_symbols(acsim_lib):
    hdr = open(os.path.join(ROOT, "include", "acsim.h")).read()
    for name in ("acs_create_csr_split", "acs_get_split_shares"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name           # declared
        assert hasattr(acsim_lib, name), name                            # exported
        assert getattr(acsim_lib, name).argtypes, name                   # bound with a signature
    assert int(re.search(r"#define\s+ACS_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4
    assert acsim_lib.acs_abi_version() == 4 == _abi.ABI_VERSION


def test_header_parses_as_c_with_the_declared_signatures():
    """A C compiler takes the header, and the two declarations have the documented types (assigning them
    to function pointers of those types is an error otherwise under -Werror)."""
    src = ('#include <acsim.h>\n'
           'int (*p1)(const acs_config*, const uint64_t*, const uint32_t*, uint32_t, const uint32_t*, int, '
           'struct acs_sim**) = acs_create_csr_split;\n'
           'int (*p2)(struct acs_sim*, double*, uint64_t) = acs_get_split_shares;\n'
           'int main(void) { return p1 == 0 || p2 == 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", c, "-o",
                            os.path.join(d, "p.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _create(lib, cfg, rp, ci, period, avail):
    c = cfg.to_c()
    h = C.c_void_p()
    rp = np.ascontiguousarray(rp, dtype=np.uint64)
    ci = np.ascontiguousarray(ci, dtype=np.uint32)
    av = None if avail is None else np.ascontiguousarray(avail, dtype=np.uint32)
    rc = lib.acs_create_csr_split(C.byref(c), rp.ctypes.data_as(u64p), ci.ctypes.data_as(u32p), period,
                                  None if av is None else av.ctypes.data_as(u32p), 0, C.byref(h))
    if rc == _abi.OK:
        lib.acs_destroy(h)
    return rc, lib.acs_last_error().decode()


def _ok(rc, msg):   # validation passed: the handle exists, or the machine has no GPU to make one on
    return rc == _abi.OK or (rc == _abi.EDEVICE and "no HIP device" in msg)


def _small():
    return G.random_csr(100, 1, 8, 2)


REJECT = [
    ("rule_weighted", _abi.EINVAL, dict(rule="weighted")),
    ("rule_average", _abi.EINVAL, dict(rule="average")),
    ("rule_wmsr", _abi.EINVAL, dict(rule="wmsr", trim=1)),
    ("trim_1", _abi.EINVAL, dict(trim=1)),
    ("crash", _abi.EINVAL, dict(fault_model="crash", n_faulty=3, crash_window=4)),
    ("byzantine", _abi.EINVAL, dict(fault_model="byzantine", n_faulty=3)),
    ("loss_self", _abi.EINVAL, dict(loss_p=0.1)),
    ("hold", _abi.EUNSUPPORTED, dict(missing_policy="hold")),
    ("hold_lossy", _abi.EUNSUPPORTED, dict(missing_policy="hold", loss_p=0.2)),
    ("delay", _abi.EUNSUPPORTED, dict(delay_max=1)),
    ("delay_omit", _abi.EUNSUPPORTED, dict(delay_max=2, missing_policy="omit")),
    ("f32_rounds", _abi.EINVAL, dict(dtype="f32", max_rounds=(1 << 22) + 1)),
]


@pytest.mark.parametrize("name,code,kw", REJECT, ids=[r[0] for r in REJECT])
def test_create_rejects(acsim_lib, name, code, kw):
    rp, ci = _small()
    rc, msg = _create(acsim_lib, Config(**{**SCFG, **kw}), rp, ci, *G.phase_schedule(rp, ci, 4))
    assert rc == code and msg, (rc, msg)
    if name == "loss_self":
        assert "SELF" in msg and "mass" in msg
    if name.startswith("hold"):
        assert "HOLD" in msg and "OMIT" in msg
    if name.startswith("rule"):
        assert "PUSHSUM" in msg


def test_row_above_8192_entries_is_unsupported(acsim_lib):
    n = 8300
    deg = np.ones(n, np.int64)
    deg[0] = 8192   # row 0: 8192 senders (8193 entries)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    ci = (np.arange(int(rp[-1])) % n).astype(np.uint32)
    rc, msg = _create(acsim_lib, Config(**{**SCFG, "n_nodes": n}), rp, ci, *G.full_schedule(ci.size, 2))
    assert rc == _abi.EUNSUPPORTED and "8192" in msg, (rc, msg)
    deg[0] = 8191   # 8192 entries: served
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    ci = (np.arange(int(rp[-1])) % n).astype(np.uint32)
    assert _ok(*_create(acsim_lib, Config(**{**SCFG, "n_nodes": n}), rp, ci, *G.full_schedule(ci.size, 2)))


def test_valid_configs_pass_validation(acsim_lib):
    rp, ci = _small()
    nnz = ci.size
    scheds = (G.full_schedule(nnz, 1), G.full_schedule(nnz, 32), random_masks(nnz, 5, 1), random_masks(nnz, 32, 2),
              (7, np.zeros(nnz, np.uint32)), G.phase_schedule(rp, ci, 4, seed=3))
    for sch in scheds:   # SELF without loss takes dead links and slots that are down in some phases
        for kw in (dict(), dict(missing_policy="omit"), dict(missing_policy="omit", loss_p=0.3),
                   dict(n_instances=3, mask_group=2, instance_offset=5), dict(dtype="f32", max_rounds=1 << 22)):
            assert _ok(*_create(acsim_lib, Config(**{**SCFG, **kw}), rp, ci, *sch)), (kw, sch[0])


def test_every_schedule_sched_check_refuses_is_refused(acsim_lib):
    rp, ci = _small()
    nnz = ci.size
    cfg = Config(**SCFG, missing_policy="omit")
    full = np.full(nnz, 7, np.uint32)
    for period in (0, 33, 64, 0xFFFFFFFF):
        rc, msg = _create(acsim_lib, cfg, rp, ci, period, full)
        assert rc == _abi.EINVAL and f"period {period} outside 1..32" in msg, (period, rc, msg)
    rc, msg = _create(acsim_lib, cfg, rp, ci, 3, None)
    assert rc == _abi.EINVAL and "null avail" in msg, (rc, msg)
    bad = full.copy()
    bad[[17, 40]] = [8, 0x80000000]
    rc, msg = _create(acsim_lib, cfg, rp, ci, 3, bad)   # the first offending slot is named
    assert rc == _abi.EINVAL and "avail[17]" in msg and "0x00000008" in msg and "period 3" in msg, (rc, msg)
    rc, msg = _create(acsim_lib, cfg, rp, ci, 31, np.full(nnz, 0xFFFFFFFF, np.uint32))
    assert rc == _abi.EINVAL and "avail[0]" in msg and "period 31" in msg, (rc, msg)
    h = C.c_void_p()
    c = Config(n_nodes=16, rule="pushsum").to_c()   # not a CSR config
    rc = acsim_lib.acs_create_csr_split(C.byref(c), rp.ctypes.data_as(u64p), ci.ctypes.data_as(u32p), 3,
                                        full.ctypes.data_as(u32p), 0, C.byref(h))
    assert rc == _abi.EINVAL and "ACS_TOPO_CSR" in acsim_lib.acs_last_error().decode()
    c = cfg.to_c()
    rc = acsim_lib.acs_create_csr_split(C.byref(c), None, ci.ctypes.data_as(u32p), 3, full.ctypes.data_as(u32p), 0, C.byref(h))
    assert rc == _abi.EINVAL
    bad_ci = ci.copy()
    bad_ci[5] = 100
    rc, msg = _create(acsim_lib, cfg, rp, bad_ci, 3, full)   # the graph checks are acs_create_csr's
    assert rc == _abi.EINVAL and "colidx[5]" in msg, (rc, msg)


def test_simulator_arguments():
    rp, ci = _small()
    with pytest.raises(ValueError, match="no weights"):
        acsim.Simulator(Config(**SCFG), csr=(rp, ci), weights=G.pushsum_weights(rp, ci), split=True)
    with pytest.raises(ValueError):
        acsim.Simulator(Config(**SCFG), split=True)
    with pytest.raises(ValueError):   # one mask per slot
        acsim.Simulator(Config(**SCFG), csr=(rp, ci), schedule=(2, np.ones(3, np.uint32)), split=True)
    with pytest.raises(_abi.AcsError) as e:   # the value rules are the library's
        acsim.Simulator(Config(**SCFG), csr=(rp, ci), schedule=(2, np.full(ci.size, 4, np.uint32)), split=True)
    assert e.value.code == _abi.EINVAL and "avail[0]" in str(e.value)
    with pytest.raises(_abi.AcsError) as e:
        acsim.Simulator(Config(**SCFG, missing_policy="hold"), csr=(rp, ci), split=True)
    assert e.value.code == _abi.EUNSUPPORTED


# ------------------------------------------------------------------------------------- shares
@pytest.mark.parametrize("dtype,p", [("f64", 53), ("f32", 24)])
def test_split_shares_against_exact_fractions(dtype, p):
    """c * w <= 1 exactly, and w is fl(1 / c) or its predecessor: w' = the next value above w has
    c * w' > 1 or w is the round-to-nearest of 1 / c."""
    ft = np.float32 if dtype == "f32" else np.float64
    rp, ci = G.skewed_csr(3000, 1, 60, 5)
    period, av = random_masks(ci.size, 6, 3)
    sh = G.split_shares(rp, ci, period, av, dtype=dtype)
    assert sh.shape == (6, 3000) and sh.dtype == np.float64
    assert np.array_equal(sh.astype(ft).astype(np.float64), sh)   # exact in the config dtype
    lowered = 0
    for ph in range(period):
        c = 1 + np.bincount(ci[(av >> np.uint32(ph)) & np.uint32(1) == 1], minlength=3000)
        for cj, w in {(int(a), float(b)) for a, b in zip(c, sh[ph])}:
            assert Fraction(w) * cj <= 1, (cj, w)
            near = ft(1) / ft(cj)
            if float(near) == w:
                continue
            lowered += 1
            assert float(np.nextafter(near, ft(0))) == w and Fraction(float(near)) * cj > 1, (cj, w)
    assert lowered > 0 and sh.max() == 1.0 and sh.min() < 0.05   # both branches; isolated and hub senders
    assert np.array_equal(G.split_shares(rp, ci, *G.full_schedule(ci.size, 1), dtype=dtype)[0],
                          G.pushsum_weights(rp, ci, dtype=dtype)[0])
    # the restatement's own table agrees
    q = NpPushSumSplitSim(Config(n_nodes=3000, topology="csr", rule="pushsum", dtype=dtype), (rp, ci), (period, av))
    assert np.array_equal(q.share.astype(np.float64), sh)
    with pytest.raises(ValueError):
        G.split_shares(rp, ci, 3, np.full(ci.size, 8, np.uint32))


# ------------------------------------------------------------- the four consequences, restated
def static_sim(cfg, csr, w):
    return NpPushSumSim(cfg, csr, w)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("loss", [0.0, 0.3])
def test_c1_period_one_full_masks_is_the_weighted_handle_on_the_restatement(loss, dtype):
    rp, ci = G.random_csr(301, 0, 12, 3)
    cfg = Config(n_nodes=301, topology="csr", rule="pushsum", missing_policy="omit", loss_p=loss, termination="fixed",
                 max_rounds=15, seed=61, dtype=dtype, n_instances=2, trace_spread=True)
    a = NpPushSumSplitSim(cfg, (rp, ci), G.full_schedule(ci.size, 1))
    a.run()
    b = static_sim(cfg, (rp, ci), G.pushsum_weights(rp, ci, dtype=dtype))
    b.run()
    same_runs(a, b)


def chain_check(split_step, split_pairs, make_static, period, rounds):
    """Consequence 2: before each round the phase's static handle takes the split run's pairs and runs
    one round; its pairs are the split run's next pairs, bit for bit."""
    for r in range(rounds):
        s, z = split_pairs()
        nxt = make_static(r % period, r, s, z)
        split_step()
        s2, z2 = split_pairs()
        assert np.array_equal(bits(nxt[0]), bits(s2)) and np.array_equal(bits(nxt[1]), bits(z2)), r


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c2_phase_chaining_on_the_restatement(dtype):
    rp, ci = small_graph(15, 65)
    sch = random_masks(ci.size, 5, 7)
    cfg = Config(n_nodes=333, topology="csr", rule="pushsum", missing_policy="omit", termination="fixed", max_rounds=12,
                 seed=9, dtype=dtype)
    q = NpPushSumSplitSim(cfg, (rp, ci), sch)
    statics = [static_sim(cfg, (rp, ci), q.effective_weights(p)) for p in range(5)]

    def one(p, r, s, z):
        statics[p].restart(r, s, z)
        statics[p].round(1)
        return statics[p].s.copy(), statics[p].z.copy()
    chain_check(lambda: q.round(1), lambda: (q.s.copy(), q.z.copy()), one, 5, 12)


def dyadic_case(dtype):
    """Every c_p(j) is a power of two: node j has 3 listeners (i = j - 1, j - 3, j - 5 mod n); phase 0
    has all three links up (c = 4), phase 1 only the first, and only into even rows (c = 2 or 1: the
    rows are treated unequally, so z leaves 1), phase 2 none (c = 1).  Shares are 2^-k with k <= 2, so
    after R rounds every z is a multiple of 2^(-2 R) and every sum is exact while 2 R + 2 <= 53 (fp32: 24)."""
    from test_pushsum_hold import odd_circulant
    rp, ci, _ = odd_circulant(301, 3)
    t = np.arange(ci.size) % 3   # slot t of every row
    row = np.arange(ci.size) // 3
    av = np.where((t == 0) & (row % 2 == 0), 0b011, 0b001).astype(np.uint32)
    R = 25 if dtype == "f64" else 11
    assert 2 * R + 2 <= (53 if dtype == "f64" else 24)
    cfg = Config(n_nodes=301, topology="csr", rule="pushsum", termination="fixed", max_rounds=R, seed=5, dtype=dtype)
    return cfg, (rp, ci), (3, av)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c3_dyadic_counts_keep_the_mass_exactly_on_the_restatement(dtype):
    cfg, csr, sch = dyadic_case(dtype)
    q = NpPushSumSplitSim(cfg, csr, sch)
    c = np.round(1.0 / q.share.astype(np.float64))
    assert set(np.unique(c).tolist()) == {1.0, 2.0, 4.0}
    q.run()
    assert math.fsum(q.z[0].tolist()) == 301.0
    assert len(set(q.z[0].tolist())) > 5   # not the trivial z = 1 everywhere
    # fixed weights 1 / (outdeg + 1) under OMIT on the same schedule lose mass
    p = sched_sim(cfg.replace(missing_policy="omit"), csr, G.pushsum_weights(*csr, dtype=dtype), sch)
    p.run()
    assert math.fsum(p.z[0].tolist()) < 301.0 / 2


def test_c4_split_finds_the_mean_on_a_schedule_and_fixed_weights_under_omit_do_not():
    """random_csr(2000, 1, 12, 3) on phase_schedule(.., 4), seed 0 (the schedule of
    test_link_schedule's HOLD test: 110 rounds, 3.8e-13), eps = 1e-12, no loss.  Every round's matrix is
    column-stochastic up to the one-ulp steps, so the plain rule's drift bound holds round by round:
    |x_i - mean| <= 2 R (ceil(log2 m_max) + 5) 2^-53 max|x^0| + the final spread."""
    n, P = 2000, 4
    rp, ci = G.random_csr(n, 1, 12, 3)
    sch = G.phase_schedule(rp, ci, P, seed=0)
    cfg = Config(n_nodes=n, topology="csr", rule="pushsum", eps=1e-12, max_rounds=3000, seed=11)
    q = NpPushSumSplitSim(cfg, (rp, ci), sch)
    x0 = q.x[0].copy()
    mean = math.fsum(x0.tolist()) / n
    q.run()
    R = int(q.rounds[0])
    m_max = int(np.diff(rp.astype(np.int64)).max()) + 1
    spread = float(q.x[0].max() - q.x[0].min())
    bound = 2 * R * (math.ceil(math.log2(m_max)) + 5) * 2.0 ** -53 * float(np.abs(x0).max()) + spread
    err = float(np.abs(q.x[0] - mean).max())
    print(f"split: {R} rounds, max |x - mean| = {err:.3e}, bound {bound:.3e}, z mass - N = {math.fsum(q.z[0].tolist()) - n:.3e}")
    assert q.converged[0] and R < 3000
    assert err <= bound
    assert bound < 1e-9
    p = sched_sim(cfg.replace(missing_policy="omit"), (rp, ci), G.pushsum_weights(rp, ci), sch)
    p.run()
    oerr = float(np.abs(p.x[0] - mean).min())
    print(f"omit, fixed weights: {int(p.rounds[0])} rounds, converged {bool(p.converged[0])}, min |x - mean| = {oerr:.3e}")
    assert oerr > 1e-4


# ----------------------------------------------------------------------------------------- CLI
def test_cli_split_uses_the_files_schedule_and_says_so(tmp_path):
    rp, ci = G.random_csr(200, 1, 9, 9)
    sch = G.phase_schedule(rp, ci, 4)
    G.save_csr(str(tmp_path / "s.npz"), rp, ci, schedule=sch)
    got = G.load_csr(str(tmp_path / "s.npz"), schedule=True)
    assert got[2] == 4 and np.array_equal(got[3], sch[1])
    sets = ["--set", "rule=pushsum", "--set", "fault_model=none", "--set", "n_faulty=0"]
    r = _cli("validate", "--graph", str(tmp_path / "s.npz"), "--split", *sets)
    assert r.returncode == 0 and "ok" in r.stdout and "--split" in r.stderr and "period 4" in r.stderr, (r.stdout, r.stderr)
    # SELF with down phases is refused without --split and served with it
    G.save_csr(str(tmp_path / "w.npz"), rp, ci, weights=G.pushsum_weights(rp, ci), schedule=sch)
    r = _cli("validate", "--graph", str(tmp_path / "w.npz"), *sets)
    assert r.returncode == 1 and "create mass" in r.stderr, r.stderr
    r = _cli("validate", "--graph", str(tmp_path / "w.npz"), "--split", *sets)
    assert r.returncode == 0 and "using the link schedule of" in r.stderr, r.stderr
    # no schedule in the file: every link up; HOLD: the library's refusal
    G.save_csr(str(tmp_path / "g.npz"), rp, ci)
    r = _cli("validate", "--graph", str(tmp_path / "g.npz"), "--split", *sets)
    assert r.returncode == 0 and "no link schedule" in r.stderr, r.stderr
    r = _cli("validate", "--graph", str(tmp_path / "s.npz"), "--split", *sets, "--set", "missing_policy=hold")
    assert r.returncode == 1 and "EUNSUPPORTED" in r.stderr and "HOLD" in r.stderr, r.stderr
    r = _cli("validate", "--graph", str(tmp_path / "s.npz"), "--split", "--set", "rule=weighted")
    assert r.returncode == 2 and "rule=pushsum" in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------ GPU
N_BIG = 3001
_ref = {}


def cached(key, make):
    if key not in _ref:
        _ref[key] = make()
    n = _ref[key]
    if not n.done.all():
        n.run()
    return n


def kname(path, f32, d=32, hubs=True):
    nm = "k_round_generic"
    if path == "fast":
        nm = f"k_round_pushsum_split<{d},csr>" + ("+k_round_generic(hubs)" if hubs else "")
    return nm + (" [f32]" if f32 else "")


def run_split(cfg, csr, sch, steps=None):
    with acsim.Simulator(cfg, csr=csr, schedule=sch, split=True) as g:
        name = g.kernel_name()
        if steps is None:
            g.run()
        else:
            for k in steps:
                g.round(k)
        return name, read_all(g)


def check(key, cfg, csr, sch, name):
    got_name, got = run_split(cfg, csr, sch)
    assert got_name == name
    n = cached(key, lambda: NpPushSumSplitSim(cfg, csr, sch))
    assert_same(got, n)
    return got, n


def big_cfg(dtype="f64", **over):
    return Config(**{**dict(n_nodes=N_BIG, topology="csr", rule="pushsum", missing_policy="omit", seed=45, trace_spread=True,
                            termination="fixed", dtype=dtype), **over})


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("loss", [0.0, 0.3])
def test_gpu_c1_period_one_full_masks_equal_the_weighted_handle(env, loss, path):
    """3001 nodes, degrees 0 .. 40: D = 32 plus hub rows, a partial last block and SELL slice, rows with
    no senders.  12 FIXED rounds."""
    rp, ci = big_graph()
    cfg = big_cfg(loss_p=loss, max_rounds=12)
    env(**PATHS[path])
    name, split = run_split(cfg, (rp, ci), G.full_schedule(ci.size, 1))
    with acsim.Simulator(cfg, csr=(rp, ci), weights=G.pushsum_weights(rp, ci)) as g:
        wname = g.kernel_name()
        g.run()
        weighted = read_all(g)
    assert name == kname(path, False) and wname == ("k_round_pushsum<32,csr>+k_round_generic(hubs)" if path == "fast"
                                                    else "k_round_generic")
    assert_same_handles(split, weighted)
    assert_same(split, cached(("c1", loss), lambda: NpPushSumSplitSim(cfg, (rp, ci), G.full_schedule(ci.size, 1))))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_c2_phase_chaining_against_the_static_handles(env, path):
    """333 nodes, P = 5, 12 rounds: the split handle stepped one round at a time; before each round the
    phase's unscheduled push-sum handle takes its pairs through set_pushsum_state(r, s, z) and runs one
    round."""
    rp, ci = small_graph(15, 65)
    sch = random_masks(ci.size, 5, 7)
    cfg = Config(n_nodes=333, topology="csr", rule="pushsum", missing_policy="omit", termination="fixed", max_rounds=12,
                 seed=9, trace_spread=True)
    ref = NpPushSumSplitSim(cfg, (rp, ci), sch)
    env(**PATHS[path])
    statics = [acsim.Simulator(cfg, csr=(rp, ci), weights=ref.effective_weights(p)) for p in range(5)]
    try:
        with acsim.Simulator(cfg, csr=(rp, ci), schedule=sch, split=True) as g:
            assert g.kernel_name() == kname(path, False, 16, hubs=False)
            assert statics[0].kernel_name() == ("k_round_pushsum<16,csr>" if path == "fast" else "k_round_generic")

            def one(p, r, s, z):
                statics[p].set_pushsum_state(r, s, z)
                statics[p].round(1)
                return statics[p].pushsum_state(0)
            chain_check(lambda: g.round(1), lambda: g.pushsum_state(0), one, 5, 12)
            ref.run()
            assert_same(read_all(g), ref)
    finally:
        for h in statics:
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("period", [1, 5, 32])
@pytest.mark.parametrize("dmax,D", [(3, 4), (7, 8), (15, 16)])
def test_gpu_random_masks_narrow_widths(env, dmax, D, period, path):
    """333 nodes, random masks with dead links and always-up links, 37 FIXED rounds: the phase wraps."""
    rp, ci = small_graph(dmax, 50 + dmax)
    sch = random_masks(ci.size, period, 7)
    cfg = Config(n_nodes=333, topology="csr", rule="pushsum", missing_policy="omit", seed=46, trace_spread=True,
                 termination="fixed", max_rounds=37, loss_p=0.2 if period == 5 else 0.0)
    env(**PATHS[path])
    check(("narrow", dmax, period), cfg, (rp, ci), sch, kname(path, False, D, hubs=False))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_random_masks_one_block_with_a_partly_empty_wave(env, path):
    rng = np.random.default_rng(45)
    deg = rng.integers(0, 9, 70)
    deg[:3] = [8, 0, 5]
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    ci = rng.integers(0, 70, int(rp[-1])).astype(np.uint32)
    cfg = Config(n_nodes=70, topology="csr", rule="pushsum", seed=46, trace_spread=True, termination="fixed", max_rounds=37)
    env(**PATHS[path])
    check("n70", cfg, (rp, ci), random_masks(ci.size, 5, 8), kname(path, False, 8, hubs=False))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_three_instances_under_eps_with_loss(env, path):
    """mask_group = 2 and instance_offset = 5: instances 5 | 6, 7 draw two drop masks.  The instances stop
    by the spread test at rounds of their own."""
    rp, ci = G.random_csr(333, 1, 15, 66)   # every row hears someone
    cfg = Config(n_nodes=333, topology="csr", rule="pushsum", missing_policy="omit", seed=45, trace_spread=True,
                 n_instances=3, mask_group=2, instance_offset=5, eps=1e-9, max_rounds=400, loss_p=0.2)
    env(**PATHS[path])
    _, n = check("eps", cfg, (rp, ci), G.phase_schedule(rp, ci, 4, seed=2), kname(path, False, 16, hubs=False))
    assert n.converged.all() and 20 < n.rounds.min() and n.rounds.max() < 400


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_fp32(env, path):
    rp, ci = small_graph(15, 65)
    cfg = Config(n_nodes=333, topology="csr", rule="pushsum", missing_policy="omit", seed=46, trace_spread=True,
                 termination="fixed", max_rounds=37, dtype="f32", loss_p=0.1)
    env(**PATHS[path])
    check("f32", cfg, (rp, ci), random_masks(ci.size, 5, 10), kname(path, True, 16, hubs=False))
    rp, ci = big_graph()
    check("f32-big", big_cfg("f32", max_rounds=9), (rp, ci), random_masks(ci.size, 3, 4), kname(path, True))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_hub_rows_of_every_generic_size_class_write_offers(env, path):
    """hub_class_graph: a hub row at both ends of every size class of k_round_generic.  Seven rounds on a
    period-3 schedule: a hub row's offer of round r + 1, written by the generic kernel, is gathered by
    lane rows and by other hub rows."""
    rp, ci = hub_class_graph()
    check_hub_class_graph(rp, ci)
    cfg = Config(n_nodes=rp.size - 1, topology="csr", rule="pushsum", seed=47, trace_spread=True, termination="fixed",
                 max_rounds=7)
    env(**PATHS[path])
    check("hubs", cfg, (rp, ci), random_masks(ci.size, 3, 13), kname(path, False))


STEP_P = 5


def step_case():
    rp, ci = big_graph()
    return big_cfg(max_rounds=41, loss_p=0.2), (rp, ci), random_masks(ci.size, STEP_P, 11)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_stepped_rounds_equal_one_run(env, path):
    cfg, csr, sch = step_case()
    env(**PATHS[path])
    _, stepped = run_split(cfg, csr, sch, steps=(1, 7, 16, 17))
    _, once = run_split(cfg, csr, sch)
    assert_same_handles(stepped, once)
    assert_same(once, cached("step", lambda: NpPushSumSplitSim(cfg, csr, sch)))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_resume_rebuilds_the_offers_with_the_rounds_phase(env, path):
    """A resume at round 7 (7 % 5 = 2) through set_pushsum_state: the offers are rebuilt with phase 2's
    shares, and the run continues as the straight one."""
    cfg, csr, sch = step_case()
    r0 = 7
    env(**PATHS[path])
    with acsim.Simulator(cfg, csr=csr, schedule=sch, split=True) as g:
        g.round(r0)
        at = read_all(g)
    with acsim.Simulator(cfg, csr=csr, schedule=sch, split=True) as g:
        g.set_pushsum_state(r0, at["s"], at["z"])
        g.run()
        resumed = read_all(g)
    n = cached("step", lambda: NpPushSumSplitSim(cfg, csr, sch))
    assert np.array_equal(resumed["rounds"], n.rounds)
    for key in ("s", "z"):
        assert np.array_equal(bits(resumed[key]), bits(getattr(n, key))), key
    live = n.z > 0   # (x is recomputed from the pairs at a resume: it can differ only where z is 0)
    assert np.array_equal(bits(resumed["x"][live]), bits(n.x[live]))
    sh = G.split_shares(*csr, *sch)
    assert not np.array_equal(sh[r0 % STEP_P], sh[0])   # phase 0's shares would be another run
    # set_state: s = x, z = 1 at round 3, against the restatement restarted the same way
    m = NpPushSumSplitSim(cfg, csr, sch)
    x3 = np.linspace(0.0, 1.0, cfg.n_nodes)
    m.restart(3, x3)
    m.run()
    with acsim.Simulator(cfg, csr=csr, schedule=sch, split=True) as g:
        g.set_state(3, x3)
        g.run()
        assert_same(read_all(g), m, trace_from=3)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_c3_dyadic_mass_is_exactly_n(env, dtype, path):
    cfg, csr, sch = dyadic_case(dtype)
    env(**PATHS[path])
    with acsim.Simulator(cfg, csr=csr, schedule=sch, split=True) as g:
        assert g.kernel_name() == kname(path, dtype == "f32", 4, hubs=False)
        g.run()
        _, z = g.pushsum_state(0)
        assert g.pushsum_mass(0)[1] == 301.0
    assert math.fsum(z.tolist()) == 301.0 and len(set(z.tolist())) > 5


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_getters_return_the_shares_the_schedule_and_phase_zeros_weights(env, dtype, path):
    rp, ci = big_graph()
    sch = random_masks(ci.size, 32, 12)
    want = G.split_shares(rp, ci, *sch, dtype=dtype)
    env(**PATHS[path])
    with acsim.Simulator(big_cfg(dtype, max_rounds=3), csr=(rp, ci), schedule=sch, split=True) as g:
        sh = g.split_shares()
        g.run()
        assert np.array_equal(g.split_shares(), sh)
        period, av = g.link_schedule()
        ws, we = g.weights()
        out = np.empty(5, dtype=np.float64)
        rc = g._lib.acs_get_split_shares(g._h, out.ctypes.data_as(dblp), 5)   # n must be P * N
        assert rc == _abi.EINVAL
    assert sh.shape == (32, N_BIG) and np.array_equal(sh, want)
    assert period == 32 and np.array_equal(av, sch[1])
    assert np.array_equal(ws, want[0]) and np.array_equal(we, np.where(sch[1] & 1, want[0][ci], 0.0))
    with acsim.Simulator(big_cfg(dtype, max_rounds=3), csr=(rp, ci), split=True) as g:   # no schedule: P = 1, all up
        assert g.link_schedule()[0] == 1 and np.all(g.link_schedule()[1] == 1)
        assert np.array_equal(g.split_shares()[0], G.pushsum_weights(rp, ci, dtype=dtype)[0])
    with acsim.Simulator(big_cfg(dtype, max_rounds=3), csr=(rp, ci), weights=G.pushsum_weights(rp, ci, dtype=dtype),
                         schedule=sch) as g:
        with pytest.raises(_abi.AcsError) as e:   # EINVAL on any other handle
            g.split_shares()
        assert e.value.code == _abi.EINVAL


@pytest.mark.gpu
def test_gpu_c4_split_finds_the_mean(env):
    """Consequence 4 on the device: the run of the CPU test, bit for bit, so its bound holds here."""
    n = 2000
    rp, ci = G.random_csr(n, 1, 12, 3)
    sch = G.phase_schedule(rp, ci, 4, seed=0)
    cfg = Config(n_nodes=n, topology="csr", rule="pushsum", eps=1e-12, max_rounds=3000, seed=11, trace_spread=True)
    got, ref = check("c4", cfg, (rp, ci), sch, kname("fast", False, 16, hubs=False))
    assert ref.converged[0]
