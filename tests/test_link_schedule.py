"""Periodic link schedules for rules "weighted" and "pushsum" on CSR graphs ("Link
schedules"): a period P <= 32 and one uint32 mask per CSR slot; a message on a slot that is down in
round r (bit r % P clear) is missing exactly as a dropped one.

CPU part: the ABI and its validation, the three consequences of the rule on the numpy restatement
(spec_sched_np: full masks are the unscheduled rule, masks filled from the DROP draws replay a lossy
run, and the means that SELF / HOLD keep and OMIT does not), the helpers of acsim.graphs and the CLI.
GPU part: k_round_weighted / k_round_pushsum / k_round_pushsum_hold <D,csr,sched> (+ k_round_generic
for hub rows) and the all-generic path (ACSIM_CSR_FAST=0) against the restatement and, where named,
against a second handle, bit for bit in x, the (s, z) pairs, the (h, k) links, rounds, converged flags
and the spread trace.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import acsim
import spec_np as S
from acsim import _abi
from acsim import graphs as G
from acsim.config import Config
from spec_sched_np import plain_sim, sched_sim
from test_pushsum import PATHS, _cli, big_graph, bits, random_ps_weights, small_graph
from test_pushsum_hold import odd_circulant
from test_weighted import random_weights, symmetric_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64p, u32p, dblp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)

# the four rule / policy pairs a schedule is defined for (pushsum with SELF takes full masks only)
PAIRS = {
    "weighted_self": dict(rule="weighted", missing_policy="self"),
    "weighted_omit": dict(rule="weighted", missing_policy="omit"),
    "pushsum_omit": dict(rule="pushsum", missing_policy="omit"),
    "pushsum_hold": dict(rule="pushsum", missing_policy="hold"),
}


@pytest.fixture
def env(monkeypatch):
    """env(NAME=value, ...) sets variables for the rest of the test (None: unset); restored after it."""
    def set_(**kw):
        for k, v in kw.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
    return set_


def weights_for(pair, rp, ci):
    return random_weights(rp, 22) if PAIRS[pair]["rule"] == "weighted" else random_ps_weights(rp, ci, 8)


def random_masks(nnz, period, seed):
    """Random masks below 1 << period; about an eighth of the links dead (0) and an eighth always up."""
    rng = np.random.default_rng(seed)
    full = (1 << period) - 1
    av = rng.integers(0, full + 1, nnz, dtype=np.uint64)
    u = rng.random(nnz)
    av[u < 0.125] = 0
    av[u > 0.875] = full
    av[:2] = [0, full]
    return period, av.astype(np.uint32)


def drop_masks(cfg, nnz, R):
    """Consequence 2: bit r of avail[e] = (draw(DROP, bG, r, e) >= thr), r < R = the period; bG is the
    mask group every instance of the config shares."""
    assert 1 <= R <= 32 and cfg.n_instances <= cfg.mask_group and cfg.instance_offset % cfg.mask_group == 0
    thr = np.uint32(S.drop_threshold(cfg.loss_p))
    e = np.arange(nnz, dtype=np.uint64)
    av = np.zeros(nnz, dtype=np.uint32)
    for r in range(R):
        av |= (S.draw(int(cfg.seed), S.DROP, int(cfg.instance_offset), r, e) >= thr).astype(np.uint32) << np.uint32(r)
    return R, av


# ------------------------------------------------------------------------------- ABI, validation
def test_header_abi_module_and_library_agree(acsim_lib):
    hdr = open(os.path.join(ROOT, "include", "acsim.h")).read()
    assert int(re.search(r"#define\s+ACS_SCHEDULE_MAX_PERIOD\s+(\d+)", hdr).group(1)) == 32 == _abi.SCHEDULE_MAX_PERIOD
    assert G.SCHEDULE_MAX_PERIOD == 32
    for name in ("acs_create_csr_scheduled", "acs_get_link_schedule"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name           # declared
        assert hasattr(acsim_lib, name), name                            # exported
        assert getattr(acsim_lib, name).argtypes, name                   # bound with a signature
    assert int(re.search(r"#define\s+ACS_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4
    assert acsim_lib.acs_abi_version() == 4 == _abi.ABI_VERSION


def _create_s(lib, cfg, rp, ci, ws, we, period, avail):
    c = cfg.to_c()
    h = C.c_void_p()
    rp = np.ascontiguousarray(rp, dtype=np.uint64)
    ci = np.ascontiguousarray(ci, dtype=np.uint32)
    ws = np.ascontiguousarray(ws, dtype=np.float64)
    we = np.ascontiguousarray(we, dtype=np.float64)
    av = None if avail is None else np.ascontiguousarray(avail, dtype=np.uint32)
    rc = lib.acs_create_csr_scheduled(C.byref(c), rp.ctypes.data_as(u64p), ci.ctypes.data_as(u32p),
                                      ws.ctypes.data_as(dblp), we.ctypes.data_as(dblp), period,
                                      None if av is None else av.ctypes.data_as(u32p), 0, C.byref(h))
    if rc == _abi.OK:
        lib.acs_destroy(h)
    return rc, lib.acs_last_error().decode()


def _small(dtype="f64"):
    rp, ci = G.random_csr(100, 1, 8, 2)
    return (rp, ci) + G.pushsum_weights(rp, ci, dtype=dtype)


SCFG = dict(n_nodes=100, topology="csr")


def _ok(rc, msg):   # validation passed: the handle exists, or the machine has no GPU to make one on
    return rc == _abi.OK or (rc == _abi.EDEVICE and "no HIP device" in msg)


def test_valid_schedules_pass_validation(acsim_lib):
    g = _small()
    nnz = g[1].size
    for pair in PAIRS.values():
        for period, av in (G.full_schedule(nnz, 1), G.full_schedule(nnz, 32), random_masks(nnz, 5, 1),
                           random_masks(nnz, 32, 2), (7, np.zeros(nnz, np.uint32)),
                           G.phase_schedule(g[0], g[1], 4, seed=3)):
            assert _ok(*_create_s(acsim_lib, Config(**SCFG, **pair), *g, period, av)), (pair, period)
    ps_self = Config(**SCFG, rule="pushsum")   # SELF: the schedule that never takes a link down
    assert _ok(*_create_s(acsim_lib, ps_self, *g, *G.full_schedule(nnz, 6)))
    lossy = Config(**SCFG, rule="pushsum", missing_policy="hold", loss_p=0.3, n_instances=3, mask_group=2)
    assert _ok(*_create_s(acsim_lib, lossy, *g, *random_masks(nnz, 9, 3)))
    f32 = Config(**SCFG, rule="weighted", dtype="f32", delay_max=2)
    assert _ok(*_create_s(acsim_lib, f32, *_small("f32"), *random_masks(nnz, 9, 3)))


def test_schedule_validation_rules(acsim_lib):
    g = _small()
    nnz = g[1].size
    cfg = Config(**SCFG, rule="weighted")
    full = np.full(nnz, 7, np.uint32)
    for period in (0, 33, 64, 0xFFFFFFFF):
        rc, msg = _create_s(acsim_lib, cfg, *g, period, full)
        assert rc == _abi.EINVAL and f"period {period} outside 1..32" in msg, (period, rc, msg)
    rc, msg = _create_s(acsim_lib, cfg, *g, 3, None)
    assert rc == _abi.EINVAL and "null avail" in msg, (rc, msg)
    bad = full.copy()
    bad[[17, 40]] = [8, 0x80000000]
    rc, msg = _create_s(acsim_lib, cfg, *g, 3, bad)   # the first offending slot is named
    assert rc == _abi.EINVAL and "avail[17]" in msg and "0x00000008" in msg and "period 3" in msg, (rc, msg)
    bad = np.full(nnz, 0xFFFFFFFF, np.uint32)
    rc, msg = _create_s(acsim_lib, cfg.replace(rule="pushsum", missing_policy="hold"), *g, 31, bad)
    assert rc == _abi.EINVAL and "avail[0]" in msg and "period 31" in msg, (rc, msg)
    # rules 0 - 4
    for kw in (dict(rule="average"), dict(rule="trimmed_mean", trim=1), dict(rule="midpoint", trim=1),
               dict(rule="dlpsw", trim=1), dict(rule="wmsr", trim=1)):
        rc, msg = _create_s(acsim_lib, Config(**SCFG, **kw), *g, 3, full)
        assert rc == _abi.EUNSUPPORTED and "link schedules are served for rules WEIGHTED and PUSHSUM" in msg, (kw, rc, msg)
    # PUSHSUM with SELF and a slot that is not up in every phase
    down = full.copy()
    down[23] = 5
    rc, msg = _create_s(acsim_lib, Config(**SCFG, rule="pushsum"), *g, 3, down)
    assert rc == _abi.EINVAL and "SELF" in msg and "avail[23]" in msg and "create mass" in msg, (rc, msg)
    for policy in ("omit", "hold"):
        assert _ok(*_create_s(acsim_lib, Config(**SCFG, rule="pushsum", missing_policy=policy), *g, 3, down))
    assert _ok(*_create_s(acsim_lib, cfg, *g, 3, down))


def test_pinned_rejections_hold_through_the_new_entry_point(acsim_lib):
    """Every check of acs_create_csr_weighted applies unchanged (tests/test_pushsum.py, test_pushsum_hold.py,
    test_weighted.py pin them there)."""
    rp, ci, ws, we = _small()
    sch = G.full_schedule(ci.size, 4)
    ps = dict(SCFG, rule="pushsum", missing_policy="hold")
    for code, kw in ((_abi.EUNSUPPORTED, dict(delay_max=1)),
                     (_abi.EINVAL, dict(fault_model="crash", n_faulty=3, crash_window=4)),
                     (_abi.EINVAL, dict(fault_model="byzantine", n_faulty=3)),
                     (_abi.EINVAL, dict(trim=1)),
                     (_abi.EINVAL, dict(dtype="f32", max_rounds=(1 << 22) + 1))):
        for policy in ("hold", "omit"):
            rc, msg = _create_s(acsim_lib, Config(**{**ps, **kw, "missing_policy": policy}), rp, ci, ws, we, *sch)
            assert rc == code and msg, (kw, policy, rc, msg)
    rc, msg = _create_s(acsim_lib, Config(**{**ps, "missing_policy": "self", "loss_p": 0.1}), rp, ci, ws, we, *sch)
    assert rc == _abi.EINVAL and "SELF" in msg, (rc, msg)
    rc, msg = _create_s(acsim_lib, Config(**SCFG, rule="weighted", missing_policy="hold"), rp, ci, ws, we, *sch)
    assert rc == _abi.EINVAL and "HOLD" in msg and "PUSHSUM" in msg, (rc, msg)
    bad = we.copy()
    bad[3] = 1.5
    rc, msg = _create_s(acsim_lib, Config(**SCFG, rule="weighted"), rp, ci, ws, bad, *sch)
    assert rc == _abi.EINVAL and "w_edge[3]" in msg, (rc, msg)
    col = ws.copy()
    col[5] += 0.5
    rc, msg = _create_s(acsim_lib, Config(**ps), rp, ci, col, we, *sch)
    assert rc == _abi.EINVAL and "column sum" in msg, (rc, msg)
    # a row above 8192 entries
    n = 8300
    deg = np.ones(n, np.int64)
    deg[0] = 8192   # row 0: 8192 senders (8193 entries), every other row one
    rp2 = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    ci2 = np.zeros(int(rp2[-1]), np.uint32)
    ci2[:8192] = np.arange(8192) % n
    for rule in ("weighted", "pushsum"):
        w = (np.full(n, 1e-5), np.full(ci2.size, 1e-5))
        rc, msg = _create_s(acsim_lib, Config(n_nodes=n, topology="csr", rule=rule, missing_policy="omit"), rp2, ci2, *w,
                            *G.full_schedule(ci2.size, 2))
        assert rc == _abi.EUNSUPPORTED and "8192" in msg, (rule, rc, msg)
    h = C.c_void_p()
    c = Config(n_nodes=16, rule="weighted").to_c()   # not a CSR config
    rc = acsim_lib.acs_create_csr_scheduled(C.byref(c), rp.ctypes.data_as(u64p), ci.ctypes.data_as(u32p),
                                            ws.ctypes.data_as(dblp), we.ctypes.data_as(dblp), 2,
                                            sch[1].ctypes.data_as(u32p), 0, C.byref(h))
    assert rc == _abi.EINVAL and "ACS_TOPO_CSR" in acsim_lib.acs_last_error().decode()


def test_simulator_arguments():
    rp, ci, ws, we = _small()
    with pytest.raises(ValueError):
        acsim.Simulator(Config(**SCFG, rule="average"), csr=(rp, ci), schedule=G.full_schedule(ci.size, 2))
    with pytest.raises(ValueError):   # one mask per slot
        acsim.Simulator(Config(**SCFG, rule="weighted"), csr=(rp, ci), weights=(ws, we), schedule=(2, np.ones(3, np.uint32)))
    with pytest.raises(_abi.AcsError) as e:   # the value rules are the library's
        acsim.Simulator(Config(**SCFG, rule="weighted"), csr=(rp, ci), weights=(ws, we),
                        schedule=(2, np.full(ci.size, 4, np.uint32)))
    assert e.value.code == _abi.EINVAL and "avail[0]" in str(e.value)


# ------------------------------------------------------------------------------ graphs helpers
def test_phase_schedule_gives_one_phase_per_slot():
    rp, ci = symmetric_graph(500, 700, 4)
    for period in (1, 3, 4, 32):
        p, av = G.phase_schedule(rp, ci, period, seed=9)
        assert p == period and av.dtype == np.uint32 and av.shape == ci.shape
        assert np.all(av != 0) and np.all(av & (av - np.uint32(1)) == 0)   # exactly one bit
        assert not np.any(av.astype(np.uint64) >> np.uint64(period))
        G.check_schedule(rp, p, av)
        if period > 1:
            assert np.unique(av).size == period   # every phase is in use
        assert np.array_equal(av, G.phase_schedule(rp, ci, period, seed=9)[1])   # a function of its arguments
    assert not np.array_equal(G.phase_schedule(rp, ci, 4, seed=9)[1], G.phase_schedule(rp, ci, 4, seed=10)[1])
    # symmetric: slot (i <- j) and slot (j <- i) share their mask
    _, av = G.phase_schedule(rp, ci, 5, seed=2, symmetric=True)
    rows = np.repeat(np.arange(500), np.diff(rp.astype(np.int64)))
    of = {(int(i), int(j)): int(a) for i, j, a in zip(rows, ci, av)}
    assert all(of[(j, i)] == a for (i, j), a in of.items())
    assert np.all(av & (av - np.uint32(1)) == 0) and np.unique(av).size == 5
    _, plain = G.phase_schedule(rp, ci, 5, seed=2)
    assert any(int(plain[k]) != of[(int(ci[k]), int(rows[k]))] for k in range(ci.size))   # which the plain hash does not
    # the documented hash, restated on Python integers for three slots
    M = (1 << 64) - 1

    def mix(v):
        v ^= v >> 30
        v = v * 0xBF58476D1CE4E5B9 & M
        v ^= v >> 27
        v = v * 0x94D049BB133111EB & M
        return v ^ (v >> 31)
    s0 = mix((2 + 0x9E3779B97F4A7C15) & M)
    for e in (0, 17, ci.size - 1):
        assert int(plain[e]) == 1 << (mix((s0 + e) & M) % 5)
        lo, hi = sorted((int(rows[e]), int(ci[e])))
        assert int(av[e]) == 1 << (mix((mix((s0 + lo) & M) + hi) & M) % 5)


def test_full_and_check_schedule():
    assert np.array_equal(G.full_schedule(4, 3)[1], np.full(4, 7, np.uint32))
    assert np.array_equal(G.full_schedule(2, 32)[1], np.full(2, 0xFFFFFFFF, np.uint32))
    rp = np.array([0, 2, 3], np.uint64)
    p, av = G.check_schedule(rp, 3, [7, 0, 5])
    assert p == 3 and av.dtype == np.uint32 and av.tolist() == [7, 0, 5]
    for period, av, what in ((0, [1, 1, 1], "period 0"), (33, [1, 1, 1], "period 33"), (3, [7, 8, 16], "avail[1]"),
                             (3, [7, 7], "one per CSR slot"), (3, [1.0, 1.0, 1.0], "integer"), (2.0, [1, 1, 1], "integer"),
                             (3, [1, -1, 1], "uint32")):
        with pytest.raises(ValueError, match=re.escape(what)):
            G.check_schedule(rp, period, av)
    for bad in (0, 33):
        with pytest.raises(ValueError):
            G.full_schedule(3, bad)
        with pytest.raises(ValueError):
            G.phase_schedule(rp, np.array([1, 0, 0], np.uint32), bad)


def test_npz_roundtrip_with_a_schedule(tmp_path):
    rp, ci = G.random_csr(200, 1, 9, 9)
    w = G.pushsum_weights(rp, ci)
    sch = random_masks(ci.size, 11, 5)
    path = str(tmp_path / "s.npz")
    G.save_csr(path, rp, ci, weights=w, schedule=sch)
    got = G.load_csr(path, weights=True, schedule=True)
    assert len(got) == 6 and got[4] == 11 and got[5].dtype == np.uint32
    for a, b in zip(got[:4] + got[5:], (rp, ci) + w + sch[1:]):
        assert np.array_equal(a, b)
    got = G.load_csr(path, schedule=True)
    assert len(got) == 4 and got[2] == 11 and np.array_equal(got[3], sch[1])
    assert len(G.load_csr(path)) == 2 and len(G.load_csr(path, weights=True)) == 4   # as before
    G.save_csr(path, rp, ci, weights=w)
    with pytest.raises(ValueError, match="no link schedule"):
        G.load_csr(path, schedule=True)
    with pytest.raises(ValueError, match=re.escape("avail[0]")):
        G.save_csr(path, rp, ci, schedule=(3, np.full(ci.size, 8)))


def test_cli_validates_a_scheduled_file(tmp_path):
    rp, ci = G.random_csr(200, 1, 9, 9)
    sets = ["--set", "fault_model=none", "--set", "n_faulty=0"]
    G.save_csr(str(tmp_path / "s.npz"), rp, ci, weights=G.pushsum_weights(rp, ci), schedule=G.phase_schedule(rp, ci, 4))
    r = _cli("validate", "--graph", str(tmp_path / "s.npz"), "--set", "rule=pushsum", "--set", "missing_policy=hold", *sets)
    assert r.returncode == 0 and "ok" in r.stdout and "using the link schedule of" in r.stderr and "period 4" in r.stderr, \
        (r.stdout, r.stderr)
    r = _cli("validate", "--graph", str(tmp_path / "s.npz"), "--set", "rule=weighted", *sets)
    assert r.returncode == 0 and "using the link schedule of" in r.stderr, (r.stdout, r.stderr)
    # push-sum with SELF on a schedule with down phases: the library's message
    r = _cli("validate", "--graph", str(tmp_path / "s.npz"), "--set", "rule=pushsum", *sets)
    assert r.returncode == 1 and "invalid" in r.stderr and "create mass" in r.stderr, r.stderr
    # a file without a schedule behaves as before; other rules do not read the schedule
    G.save_csr(str(tmp_path / "w.npz"), rp, ci, weights=G.pushsum_weights(rp, ci))
    r = _cli("validate", "--graph", str(tmp_path / "w.npz"), "--set", "rule=pushsum", *sets)
    assert r.returncode == 0 and "link schedule" not in r.stderr, r.stderr
    r = _cli("validate", "--graph", str(tmp_path / "s.npz"), "--set", "rule=average", "--set", "trim=0", *sets)
    assert r.returncode == 0 and "link schedule" not in r.stderr, r.stderr


# ------------------------------------------------- consequences 1 and 2 on the restatements
def same_runs(a, b):
    assert np.array_equal(a.rounds, b.rounds) and np.array_equal(a.converged, b.converged)
    assert np.array_equal(bits(a.x), bits(b.x))
    for key in ("s", "z", "h", "k"):
        assert hasattr(a, key) == hasattr(b, key)
        if hasattr(a, key):
            assert np.array_equal(bits(getattr(a, key)), bits(getattr(b, key))), key
    assert a.trace == b.trace


def spec_graph(n):
    return big_graph() if n == 3001 else G.random_csr(n, 0, 12, 3)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("n", [301, 3001])
def test_full_masks_and_loss_replay_on_the_restatement(n, pair, dtype):
    """Three instances (B = 3 <= mask_group = 4, instance_offset = 4: one mask group).  The lossy
    unscheduled restatement equals (1) the scheduled one with full masks and the same loss, and (2) the
    scheduled lossless one whose masks are the run's DROP draws."""
    rp, ci = spec_graph(n)
    w = weights_for(pair, rp, ci)
    R = 10
    cfg = Config(n_nodes=n, topology="csr", loss_p=0.4, termination="fixed", max_rounds=R, seed=61, dtype=dtype,
                 n_instances=3, mask_group=4, instance_offset=4, trace_spread=True, **PAIRS[pair])
    lossy = plain_sim(cfg, (rp, ci), w)
    lossy.run()
    full = sched_sim(cfg, (rp, ci), w, G.full_schedule(ci.size, 3))
    full.run()
    same_runs(full, lossy)
    replay = sched_sim(cfg.replace(loss_p=0.0), (rp, ci), w, drop_masks(cfg, ci.size, R))
    replay.run()
    same_runs(replay, lossy)
    if pair == "pushsum_hold":
        assert np.count_nonzero(lossy.k) > ci.size // 2   # links hold mass at the end
    clean = plain_sim(cfg.replace(loss_p=0.0), (rp, ci), w)   # the loss matters: not a vacuous equality
    clean.run()
    assert not np.array_equal(bits(clean.x), bits(lossy.x))


@pytest.mark.parametrize("pair", ["weighted_self", "weighted_omit"])
def test_loss_replay_with_crash_faults_on_the_restatement(pair):
    rp, ci = spec_graph(301)
    w = weights_for(pair, rp, ci)
    cfg = Config(n_nodes=301, topology="csr", loss_p=0.3, termination="fixed", max_rounds=12, seed=62, trace_spread=True,
                 fault_model="crash", n_faulty=40, crash_window=6, **PAIRS[pair])
    lossy = plain_sim(cfg, (rp, ci), w)
    lossy.run()
    replay = sched_sim(cfg.replace(loss_p=0.0), (rp, ci), w, drop_masks(cfg, ci.size, 12))
    replay.run()
    same_runs(replay, lossy)


# ----------------------------------------------------------------------------- consequence 3: means
def test_symmetric_schedule_keeps_the_mean_under_self_and_not_under_omit():
    """Consequence 3(a).  Symmetric graph, Metropolis weights (W symmetric, rows and columns sum to 1),
    one phase of 5 per unordered edge, 200 FIXED rounds.  Under SELF a down entry takes x_i and keeps
    its weight, which moves w_ij from column j to the diagonal of row i; the schedule does the same in
    row j, so every round's effective matrix is symmetric with unit row sums, hence doubly stochastic,
    and the mean moves only by rounding: per round at most (ceil(log2 m_max) + 4) 2^-53 max|x^0|, the
    bound of tests/test_weighted.py's Metropolis test (products, ceil(log2 m) tree levels in each of
    the two sums and the divide; |x| never exceeds max|x^0|).  Under OMIT a down entry leaves the row's
    weights to be renormalised, the matrix is no longer column stochastic and the mean drifts."""
    n, R = 1500, 200
    rp, ci = symmetric_graph(n, 2200, 26)
    w = G.metropolis_weights(rp, ci)
    sch = G.phase_schedule(rp, ci, 5, seed=1, symmetric=True)
    m_max = int(np.diff(rp.astype(np.int64)).max()) + 1
    cfg = Config(n_nodes=n, topology="csr", rule="weighted", termination="fixed", max_rounds=R, seed=33)
    q = sched_sim(cfg, (rp, ci), w, sch)
    x0 = q.x[0].copy()
    bound = R * (math.ceil(math.log2(m_max)) + 4) * 2.0 ** -53 * float(np.abs(x0).max())
    q.run()
    drift = abs(math.fsum(q.x[0].tolist()) / n - math.fsum(x0.tolist()) / n)
    p = sched_sim(cfg.replace(missing_policy="omit"), (rp, ci), w, sch)
    p.run()
    odrift = abs(math.fsum(p.x[0].tolist()) / n - math.fsum(x0.tolist()) / n)
    print(f"SELF mean drift {drift:.3e} (bound {bound:.3e}, m_max {m_max}), OMIT mean drift {odrift:.3e}")
    assert q.rounds[0] == R and float(q.x[0].max() - q.x[0].min()) < float(x0.max() - x0.min())
    assert drift <= bound
    assert bound < 1e-11
    assert odrift > 1e-4


def test_hold_finds_the_mean_on_a_schedule_and_omit_does_not():
    """Consequence 3(b).  Directed graph, weights 1 / (outdeg + 1), every slot up in exactly one of 4
    phases, eps = 1e-12, no random loss.  The bound of test_pushsum_hold.py's
    test_hold_finds_the_mean_under_loss_and_omit_does_not carries over:
        B = W + (2 L + 6) 2^-53 max|x^0| + 2 R (ceil(log2 m_max) + k_max + 5) 2^-53 max|x^0|.
    Its step (1), the total mass S* = sum s + sum h and Z* = sum z + sum k, never asks why a message
    failed to cross: its mass goes to the receiver or stays on the link.  Its step (2) needs L, the
    longest run of missing messages still open on any link at the end: a slot that is up once in
    every P rounds is down for at most P - 1 in a row, so L = P - 1 = 3, and W is the width of the
    hull of x^(R-L) .. x^R as the run reports it.  OMIT loses the mass of three messages in four."""
    n, P = 2000, 4
    rp, ci = G.random_csr(n, 1, 12, 3)
    ws, we = G.pushsum_weights(rp, ci)
    sch = G.phase_schedule(rp, ci, P, seed=0)
    cfg = Config(n_nodes=n, topology="csr", rule="pushsum", eps=1e-12, max_rounds=3000, seed=11, missing_policy="hold")
    q = sched_sim(cfg, (rp, ci), (ws, we), sch)
    x0 = q.x[0].copy()
    mean = math.fsum(x0.tolist()) / n
    q.run()
    R = int(q.rounds[0])
    m_max = int(np.diff(rp.astype(np.int64)).max()) + 1
    k_max = int(np.bincount(ci, minlength=n).max()) + 1
    L = P - 1
    hull = np.stack(q.hist[0][R - L:R + 1])
    W = float(hull.max() - hull.min())
    xmax = float(np.abs(x0).max())
    B = W + (2 * L + 6) * 2.0 ** -53 * xmax + 2 * R * (math.ceil(math.log2(m_max)) + k_max + 5) * 2.0 ** -53 * xmax
    err = float(np.abs(q.x[0] - mean).max())
    ms, mz = q.mass(0)
    print(f"hold: {R} rounds, max |x - mean| = {err:.3e}, bound {B:.3e} (L = {L}, W = {W:.3e}), "
          f"z mass - N = {mz - n:.3e}, s mass / N - mean = {ms / n - mean:.3e}")
    assert q.converged[0] and L < R < 3000
    assert err <= B
    assert B < 1e-9   # the bound separates the two policies: OMIT below is five orders away
    p = sched_sim(cfg.replace(missing_policy="omit"), (rp, ci), (ws, we), sch)
    p.run()
    oerr = float(np.abs(p.x[0] - mean).min())
    print(f"omit: {int(p.rounds[0])} rounds, converged {bool(p.converged[0])}, z mass {math.fsum(p.z[0].tolist()):.3e}, "
          f"min |x - mean| = {oerr:.3e}")
    assert oerr > 1e-4


def dyadic_cfg(rounds, dtype, policy, **over):
    return Config(**{**dict(n_nodes=301, topology="csr", rule="pushsum", missing_policy=policy, termination="fixed",
                            max_rounds=rounds, seed=5, dtype=dtype), **over})


@pytest.mark.parametrize("sched", ["phase3", "random7", "random32_lossy"])
@pytest.mark.parametrize("d,rounds,dtype", [(3, 20, "f64"), (3, 9, "f32"), (15, 12, "f64")])
def test_mass_is_exactly_n_on_dyadic_weights_under_any_schedule(d, rounds, dtype, sched):
    """Consequence 3(c), the argument of test_mass_is_conserved_exactly_on_dyadic_weights: every weight
    is 2^-k and every column sum is 1, so after R rounds every z and k is a multiple of 2^(-k R) below
    2^2 and every sum is exact while k R + 2 <= 53 (fp32: 24); whether a slot is down, dropped or up
    only decides where a term goes.  fsum(z) + fsum(k) is exactly N."""
    k = int(math.log2(d + 1))
    assert 2 ** k == d + 1 and k * rounds + 2 <= (53 if dtype == "f64" else 24)
    rp, ci, w = odd_circulant(301, d)
    assert np.all(G.column_sums(rp, ci, *w) == 1.0)
    sch = G.phase_schedule(rp, ci, 3, seed=4) if sched == "phase3" else random_masks(ci.size, 7 if sched == "random7" else 32, 6)
    over = dict(loss_p=0.3) if sched.endswith("lossy") else {}
    q = sched_sim(dyadic_cfg(rounds, dtype, "hold", **over), (rp, ci), w, sch)
    q.run()
    zmass = math.fsum(q.z[0].tolist() + q.k[0].tolist())
    p = sched_sim(dyadic_cfg(rounds, dtype, "omit", **over), (rp, ci), w, sch)
    p.run()
    omit = math.fsum(p.z[0].tolist())
    print(f"d={d} {dtype} {rounds} rounds, {sched}: hold z mass {zmass!r} ({np.count_nonzero(q.k[0])} links hold mass), "
          f"OMIT z mass {omit:.3g}")
    assert zmass == 301.0 and q.mass(0)[1] == 301.0
    assert np.count_nonzero(q.k[0]) > 100
    assert omit < 301.0 / 2


# ------------------------------------------------------------------------------------------ GPU
N_BIG = 3001
_ref = {}


def cached(key, make):
    if key not in _ref:
        _ref[key] = make()
    return _ref[key]


def kname(pair, path, f32, d=32, hubs=True, sched=True):
    kernel = {"weighted": "k_round_weighted", "pushsum": "k_round_pushsum"}[PAIRS[pair]["rule"]]
    if pair == "pushsum_hold":
        kernel += "_hold"
    nm = "k_round_generic"
    if path == "fast":
        nm = f"{kernel}<{d},csr{',sched' if sched else ''}>" + ("+k_round_generic(hubs)" if hubs else "")
    return nm + (" [f32]" if f32 else "")


def read_all(g):
    out = dict(rounds=g.rounds(), conv=g.converged(), x=g.all_values(), trace=[g.spread_trace(b) for b in range(g.B)])
    if g.cfg.rule == "pushsum":
        pairs = [g.pushsum_state(b) for b in range(g.B)]
        out.update(s=np.stack([p[0] for p in pairs]), z=np.stack([p[1] for p in pairs]))
        if g.cfg.missing_policy == "hold":
            lk = [g.pushsum_links(b) for b in range(g.B)]
            out.update(h=np.stack([p[0] for p in lk]), k=np.stack([p[1] for p in lk]))
    return out


def assert_same(got, n, trace_from=0):
    """A handle's read_all against a restatement: x, pairs, links, rounds, converged flags, spread trace."""
    assert np.array_equal(got["rounds"], n.rounds)
    assert np.array_equal(got["conv"], n.converged)
    assert np.array_equal(bits(got["x"]), bits(n.x)), "x"
    assert ("s" in got) == hasattr(n, "s") and ("h" in got) == hasattr(n, "h")
    if "s" in got:
        assert np.array_equal(bits(got["s"]), bits(n.s)), "s"
        assert np.array_equal(bits(got["z"]), bits(n.z)), "z"
    if "h" in got:
        assert np.array_equal(bits(got["h"]), bits(n.h[:, n.N:])), "h"
        assert np.array_equal(bits(got["k"]), bits(n.k[:, n.N:])), "k"
    for b in range(n.B):
        assert np.array_equal(got["trace"][b][trace_from:], np.array(n.trace[b][trace_from:], dtype=np.float64)), b


def assert_same_handles(a, b):
    assert a.keys() == b.keys()
    assert np.array_equal(a["rounds"], b["rounds"]) and np.array_equal(a["conv"], b["conv"])
    for key in ("x", "s", "z", "h", "k"):
        if key in a:
            assert np.array_equal(bits(a[key]), bits(b[key])), key
    for u, v in zip(a["trace"], b["trace"]):
        assert np.array_equal(bits(u), bits(v))


def run_handle(cfg, csr, w, sch=None, steps=None):
    with acsim.Simulator(cfg, csr=csr, weights=w, schedule=sch) as g:
        name = g.kernel_name()
        if steps is None:
            g.run()
        else:
            for k in steps:
                g.round(k)
        return name, read_all(g)


def big_cfg(pair, dtype, **over):
    return Config(**{**dict(n_nodes=N_BIG, topology="csr", seed=45, trace_spread=True, termination="fixed", dtype=dtype),
                     **PAIRS[pair], **over})


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_gpu_full_masks_equal_the_unscheduled_handle(env, pair, dtype, path):
    """3001 nodes, degrees 0 .. 40: D = 32 plus hub rows, a partial last block and SELL slice, rows with
    no senders.  loss_p = 0.4, 12 FIXED rounds, every mask 0b111 (P = 3)."""
    rp, ci = big_graph()
    w = weights_for(pair, rp, ci)
    cfg = big_cfg(pair, dtype, loss_p=0.4, max_rounds=12)
    env(**PATHS[path])
    sname, sched = run_handle(cfg, (rp, ci), w, G.full_schedule(ci.size, 3))
    pname, plain = run_handle(cfg, (rp, ci), w)
    f32 = dtype == "f32"
    assert sname == kname(pair, path, f32) and pname == kname(pair, path, f32, sched=False)
    if path == "fast":
        assert sname == pname.replace(",csr>", ",csr,sched>") != pname
    assert_same_handles(sched, plain)
    n = cached(("full", pair, dtype), lambda: sched_sim(cfg, (rp, ci), w, G.full_schedule(ci.size, 3)))
    if not n.done.all():
        n.run()
    assert_same(sched, n)


REPLAY = {**{p: {} for p in PAIRS},
          "weighted_self_crash": dict(fault_model="crash", n_faulty=60, crash_window=8),
          "weighted_omit_crash": dict(fault_model="crash", n_faulty=60, crash_window=8),
          "pushsum_hold_inst3": dict(n_instances=3, mask_group=4, instance_offset=4),
          "weighted_self_inst3": dict(n_instances=3, mask_group=4, instance_offset=4)}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", list(REPLAY))
def test_gpu_loss_replay_equals_the_lossy_handle(env, case, path):
    """P = R = 32 (bit 31 is in use): the scheduled lossless handle whose masks are the DROP draws of the
    lossy config equals the lossy unscheduled handle, and both equal the restatement."""
    pair = case if case in PAIRS else case.rsplit("_", 1)[0]
    rp, ci = big_graph()
    w = weights_for(pair, rp, ci)
    cfg = big_cfg(pair, "f64", loss_p=0.35, max_rounds=32, **REPLAY[case])
    sch = drop_masks(cfg, ci.size, 32)
    assert np.count_nonzero(sch[1] >> np.uint32(31)) > ci.size // 2
    env(**PATHS[path])
    sname, sched = run_handle(cfg.replace(loss_p=0.0), (rp, ci), w, sch)
    pname, lossy = run_handle(cfg, (rp, ci), w)
    assert sname == kname(pair, path, False) and pname == kname(pair, path, False, sched=False)
    assert_same_handles(sched, lossy)
    n = cached(("replay", case), lambda: sched_sim(cfg.replace(loss_p=0.0), (rp, ci), w, sch))
    if not n.done.all():
        n.run()
    assert_same(sched, n)
    if pair == "pushsum_hold":
        assert np.count_nonzero(sched["k"]) > 1000   # links hold mass at the end


def width_cfg(pair, n, dtype="f64", **over):
    return Config(**{**dict(n_nodes=n, topology="csr", seed=46, trace_spread=True, termination="fixed", max_rounds=37,
                            dtype=dtype), **PAIRS[pair], **over})


def check_against_restatement(key, cfg, csr, w, sch, name):
    got_name, got = run_handle(cfg, csr, w, sch)
    assert got_name == name
    n = cached(key, lambda: sched_sim(cfg, csr, w, sch))
    if not n.done.all():
        n.run()
    assert_same(got, n)
    return got, n


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("period", [1, 5, 32])
@pytest.mark.parametrize("dmax,D", [(3, 4), (7, 8), (15, 16)])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_gpu_random_masks_narrow_widths(env, pair, dmax, D, period, path):
    """333 nodes, random masks with dead links and always-up links, 37 FIXED rounds: the phase wraps."""
    rp, ci = small_graph(dmax, 50 + dmax)
    w = weights_for(pair, rp, ci)
    sch = random_masks(ci.size, period, 7)
    cfg = width_cfg(pair, 333, loss_p=0.2 if period == 5 else 0.0)
    env(**PATHS[path])
    _, n = check_against_restatement(("narrow", pair, dmax, period), cfg, (rp, ci), w, sch,
                                     kname(pair, path, False, D, hubs=False))
    plain = cached(("narrow-plain", pair, dmax, period), lambda: plain_sim(cfg, (rp, ci), w))
    if not plain.done.all():
        plain.run()
    assert not np.array_equal(bits(n.x), bits(plain.x))   # the schedule matters


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_gpu_random_masks_one_block_with_a_partly_empty_wave(env, pair, path):
    rng = np.random.default_rng(45)
    deg = rng.integers(0, 9, 70)
    deg[:3] = [8, 0, 5]
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    ci = rng.integers(0, 70, int(rp[-1])).astype(np.uint32)
    w = weights_for(pair, rp, ci)
    env(**PATHS[path])
    check_against_restatement(("n70", pair), width_cfg(pair, 70), (rp, ci), w, random_masks(ci.size, 5, 8),
                              kname(pair, path, False, 8, hubs=False))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("pair", ["weighted_self", "weighted_omit"])
def test_gpu_random_masks_with_delays_and_three_instances(env, pair, path):
    """delay_max = 2: the availability tested is that of the delivery round."""
    rp, ci = small_graph(15, 65)
    w = weights_for(pair, rp, ci)
    cfg = width_cfg(pair, 333, delay_max=2, n_instances=3, loss_p=0.1)
    env(**PATHS[path])
    check_against_restatement(("delay", pair), cfg, (rp, ci), w, random_masks(ci.size, 5, 9),
                              kname(pair, path, False, 16, hubs=False))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_gpu_random_masks_fp32(env, pair, path):
    rp, ci = small_graph(15, 65)
    w = weights_for(pair, rp, ci)
    cfg = width_cfg(pair, 333, dtype="f32", loss_p=0.1)
    env(**PATHS[path])
    check_against_restatement(("f32", pair), cfg, (rp, ci), w, random_masks(ci.size, 5, 10),
                              kname(pair, path, True, 16, hubs=False))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_hold_converges_on_a_one_phase_of_four_schedule(env, path):
    """An EPS run: the three instances stop by the spread test."""
    rp, ci = G.random_csr(333, 1, 15, 66)   # every row hears someone: every x_i moves, the spread falls to eps
    w = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=333, topology="csr", rule="pushsum", missing_policy="hold", seed=45, trace_spread=True,
                 n_instances=3, eps=1e-9, max_rounds=400)
    env(**PATHS[path])
    got, n = check_against_restatement("eps", cfg, (rp, ci), w, G.phase_schedule(rp, ci, 4, seed=2),
                                       kname("pushsum_hold", path, False, 16, hubs=False))
    assert n.converged.all() and 20 < n.rounds.min() and n.rounds.max() < 400


STEP_P = 5


def step_case(pair):
    rp, ci = big_graph()
    cfg = big_cfg(pair, "f64", max_rounds=41, loss_p=0.2)
    return cfg, (rp, ci), weights_for(pair, rp, ci), random_masks(ci.size, STEP_P, 11)


def step_reference(pair):
    def make():
        n = sched_sim(*step_case(pair))
        n.run()
        return n
    return cached(("step", pair), make)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_gpu_stepped_rounds_equal_one_run(env, pair, path):
    cfg, csr, w, sch = step_case(pair)
    env(**PATHS[path])
    _, stepped = run_handle(cfg, csr, w, sch, steps=(1, 7, 16, 17))
    _, once = run_handle(cfg, csr, w, sch)
    assert_same_handles(stepped, once)
    assert_same(once, step_reference(pair))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_gpu_resume_continues_at_the_rounds_phase(env, pair, path):
    """A resume at round r0 = 7 (7 % 5 = 2) continues with phase 2: the handle's round index, not the
    number of rounds it has run, selects the bit."""
    cfg, csr, w, sch = step_case(pair)
    r0 = 7
    assert r0 % STEP_P != 0
    env(**PATHS[path])
    with acsim.Simulator(cfg, csr=csr, weights=w, schedule=sch) as g:
        g.round(r0)
        at = read_all(g)
    with acsim.Simulator(cfg, csr=csr, weights=w, schedule=sch) as g:
        if cfg.rule == "weighted":
            g.set_state(r0, at["x"])
        else:
            g.set_pushsum_state(r0, at["s"], at["z"])
            if "h" in at:
                g.set_pushsum_links(at["h"], at["k"])   # (after it: set_pushsum_state empties the links)
        g.run()
        resumed = read_all(g)
    # the restatement, restarted the same way ...
    m = sched_sim(cfg, csr, w, sch)
    if cfg.rule == "weighted":
        m.x = at["x"].astype(m.ft).reshape(m.B, m.N) + m.ft(0)
        m.hist = [[None] * r0 + [m.x[lb].copy()] for lb in range(m.B)]
        m.rounds[:] = r0
        for lb in range(m.B):
            m.trace[lb] = [np.nan] * r0
            m._after(lb)
    else:
        m.restart(r0, at["s"], at["z"])
        if "h" in at:
            m.set_links(at["h"], at["k"])
    m.run()
    assert_same(resumed, m, trace_from=r0)
    # ... and the straight run (x is recomputed from the pairs at a push-sum resume, so it can differ
    # only where z is 0: rows that kept an older x)
    n = step_reference(pair)
    assert np.array_equal(resumed["rounds"], n.rounds)
    live = n.z > 0 if hasattr(n, "z") else np.ones(n.x.shape, bool)
    assert np.array_equal(bits(resumed["x"][live]), bits(n.x[live]))
    for key in ("s", "z"):
        if key in resumed:
            assert np.array_equal(bits(resumed[key]), bits(getattr(n, key))), key
    if "h" in resumed:
        assert np.array_equal(bits(resumed["h"]), bits(n.h[:, n.N:])) and np.array_equal(bits(resumed["k"]), bits(n.k[:, n.N:]))
    # a resume that began at phase 0 instead would be another run
    wrong = sched_sim(cfg, csr, w, (sch[0], ((sch[1] >> np.uint32(r0 % STEP_P)) | (sch[1] << np.uint32(STEP_P - r0 % STEP_P)))
                                    & np.uint32((1 << STEP_P) - 1)))
    wrong.round(r0)
    assert not np.array_equal(bits(wrong.x), bits(at["x"]))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_dyadic_mass_is_exactly_n(env, path):
    """The dyadic circulant (N = 301, d = 3, weights 1/4), one phase of 3 per slot, 20 rounds."""
    rp, ci, w = odd_circulant(301, 3)
    sch = G.phase_schedule(rp, ci, 3, seed=4)
    env(**PATHS[path])
    with acsim.Simulator(dyadic_cfg(20, "f64", "hold"), csr=(rp, ci), weights=w, schedule=sch) as g:
        assert g.kernel_name() == kname("pushsum_hold", path, False, 4, hubs=False)
        g.run()
        mass = g.pushsum_mass(0)
        _, k = g.pushsum_links(0)
    with acsim.Simulator(dyadic_cfg(20, "f64", "omit"), csr=(rp, ci), weights=w, schedule=sch) as g:
        g.run()
        omit = g.pushsum_mass(0)
    assert mass[1] == 301.0 and np.count_nonzero(k) > 100
    assert omit[1] < 301.0 / 2


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_link_schedule_returns_what_went_in(env, dtype, path):
    rp, ci = big_graph()
    sch = random_masks(ci.size, 32, 12)
    env(**PATHS[path])
    with acsim.Simulator(big_cfg("weighted_self", dtype, max_rounds=3), csr=(rp, ci), weights=random_weights(rp, 22),
                         schedule=sch) as g:
        period, av = g.link_schedule()
        g.run()
        assert g.link_schedule()[0] == 32 and np.array_equal(g.link_schedule()[1], sch[1])
    assert period == 32 and av.dtype == np.uint32 and np.array_equal(av, sch[1])
    with acsim.Simulator(big_cfg("weighted_self", dtype, max_rounds=3), csr=(rp, ci), weights=random_weights(rp, 22)) as g:
        with pytest.raises(_abi.AcsError) as e:   # EINVAL on an unscheduled handle
            g.link_schedule()
        assert e.value.code == _abi.EINVAL


@pytest.mark.gpu
def test_gpu_a_scheduled_handle_never_takes_the_binned_exchange(env):
    rp, ci = big_graph()
    w = random_weights(rp, 22)
    cfg = big_cfg("weighted_self", "f64", max_rounds=12, loss_p=0.3)
    env(ACSIM_BIN_WEIGHTED=1, ACSIM_BIN_SA=64)
    sname, sched = run_handle(cfg, (rp, ci), w, G.full_schedule(ci.size, 3))
    bname, binned = run_handle(cfg, (rp, ci), w)
    assert sname == "k_round_weighted<32,csr,sched>+k_round_generic(hubs)"
    assert bname == "k_bin_scatter+k_bin_gather_w<32,csr>+k_round_generic(hubs)"
    assert_same_handles(sched, binned)   # the exchange computes what the per-lane kernel computes
