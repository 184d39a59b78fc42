"""Rule "pushsum" with messages in transit ("Push-sum with messages in transit"): a message
sent in round r arrives in round r + delta, and until then its mass waits on the link.

CPU part: the ABI and its validation, the Simulator's argument errors, and the numpy restatement
(spec_pushsum_transit_np, written in history form: no ring) through the four consequences C1 .. C4 of
the spec and a resume.
GPU part: k_round_pushsum's transit instantiation (+ k_round_generic's for hub rows) and the
all-generic path (ACSIM_CSR_FAST=0) against the restatement, bit for bit in x, the (s, z) pairs, the
transit planes, rounds, converged flags and the spread trace.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import acsim
import spec_np as S
from acsim import _abi
from acsim import graphs as G
from acsim.config import Config
from hub_graphs import heard_hub_graph, hub_class_graph
from spec_pushsum_np import NpPushSumSim
from spec_pushsum_transit_np import DELAY, transit_sim
from spec_sched_np import NpSchedPushSumSim
from test_link_schedule import random_masks
from test_pushsum import PATHS, _cli, bits, env, random_ps_weights
from test_pushsum_hold import odd_circulant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64p, u32p, dblp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
NEW_CALLS = ("acs_create_csr_transit", "acs_get_pushsum_transit", "acs_set_pushsum_transit")


# ------------------------------------------------------------------------------- ABI, validation
def test_header_abi_module_and_library_agree(acsim_lib, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "acsim.h")).read()
    for name in NEW_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name           # declared
        assert hasattr(acsim_lib, name), name                            # exported
        assert getattr(acsim_lib, name).argtypes, name                   # bound with a signature
    assert int(re.search(r"#define\s+ACS_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4
    assert acsim_lib.acs_abi_version() == 4 == _abi.ABI_VERSION
    src = tmp_path / "probe.c"   # the header parses as C, and the three calls have the documented signatures
    src.write_text('#include "acsim.h"\n'
                   "int (*p1)(const acs_config*, const uint64_t*, const uint32_t*, const double*, const double*, uint32_t,\n"
                   "          const uint32_t*, uint32_t, int, struct acs_sim**) = acs_create_csr_transit;\n"
                   "int (*p2)(struct acs_sim*, uint64_t, void*, void*, uint64_t) = acs_get_pushsum_transit;\n"
                   "int (*p3)(struct acs_sim*, const void*, const void*, uint64_t) = acs_set_pushsum_transit;\n")
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _create_t(lib, cfg, rp, ci, ws, we, D, sched=None):
    c = cfg.to_c()
    h = C.c_void_p()
    rp = np.ascontiguousarray(rp, dtype=np.uint64)
    ci = np.ascontiguousarray(ci, dtype=np.uint32)
    ws = np.ascontiguousarray(ws, dtype=np.float64)
    we = np.ascontiguousarray(we, dtype=np.float64)
    period, av = (0, None) if sched is None else (int(sched[0]), np.ascontiguousarray(sched[1], dtype=np.uint32))
    rc = lib.acs_create_csr_transit(C.byref(c), rp.ctypes.data_as(u64p), ci.ctypes.data_as(u32p), ws.ctypes.data_as(dblp),
                                    we.ctypes.data_as(dblp), period, None if av is None else av.ctypes.data_as(u32p),
                                    D, 0, C.byref(h))
    if rc == _abi.OK:
        lib.acs_destroy(h)
    return rc, lib.acs_last_error().decode()


def _small(dtype="f64"):
    rp, ci = G.random_csr(100, 1, 8, 2)
    return (rp, ci) + G.pushsum_weights(rp, ci, dtype=dtype)


TCFG = dict(n_nodes=100, topology="csr", rule="pushsum")


def _ok(rc, msg):   # validation passed: the handle exists, or the machine has no GPU to make one on
    return rc == _abi.OK or (rc == _abi.EDEVICE and "no HIP device" in msg)


def test_valid_transit_configs_pass_validation(acsim_lib):
    g = _small()
    nnz = g[1].size
    for D in (0, 1, 3, 64):
        for kw in (dict(), dict(loss_p=0.3, missing_policy="omit"), dict(termination="fixed", max_rounds=7),
                   dict(n_instances=3, mask_group=2, instance_offset=9, trace_spread=True)):
            assert _ok(*_create_t(acsim_lib, Config(**TCFG, **kw), *g, D)), (D, kw)
        assert _ok(*_create_t(acsim_lib, Config(**TCFG, missing_policy="omit"), *g, D, random_masks(nnz, 5, 1))), D
        assert _ok(*_create_t(acsim_lib, Config(**TCFG), *g, D, G.full_schedule(nnz, 3))), D   # SELF: every slot up
    assert _ok(*_create_t(acsim_lib, Config(**TCFG, dtype="f32"), *_small("f32"), 3))


@pytest.mark.parametrize("D", [0, 5])
def test_fp32_round_cap_follows_the_transit_bound(acsim_lib, D):
    """DESIGN.md §9, mass bound: R (2^-30 + (15 + D) 2^-24) <= 4 holds for R <= floor(2^26 / (16 + D))."""
    g = _small("f32")
    cap = (1 << 26) // (16 + D)
    assert cap * (2.0 ** -30 + (15 + D) * 2.0 ** -24) <= 4.0
    assert D or cap == 1 << 22   # today's cap at D = 0
    cfg = Config(**TCFG, dtype="f32", termination="fixed")
    assert _ok(*_create_t(acsim_lib, cfg.replace(max_rounds=cap), *g, D))
    rc, msg = _create_t(acsim_lib, cfg.replace(max_rounds=cap + 1), *g, D)
    assert rc == _abi.EINVAL and "max_rounds" in msg, (rc, msg)
    assert _ok(*_create_t(acsim_lib, cfg.replace(max_rounds=cap + 1, dtype="f64"), *_small(), D))   # fp64: no cap


def test_what_is_refused(acsim_lib):
    rp, ci, ws, we = _small()
    nnz = ci.size
    cfg = Config(**TCFG)
    rc, msg = _create_t(acsim_lib, cfg.replace(missing_policy="hold"), rp, ci, ws, we, 2)
    assert rc == _abi.EUNSUPPORTED and "HOLD" in msg, (rc, msg)
    rc, msg = _create_t(acsim_lib, cfg.replace(delay_max=1), rp, ci, ws, we, 2)
    assert rc == _abi.EUNSUPPORTED and "delay_max" in msg, (rc, msg)
    for rule in ("weighted", "average"):
        rc, msg = _create_t(acsim_lib, cfg.replace(rule=rule), rp, ci, ws, we, 2)
        assert rc == _abi.EUNSUPPORTED and "PUSHSUM" in msg, (rule, rc, msg)
    for D in (65, 1000, 0xFFFFFFFF):
        rc, msg = _create_t(acsim_lib, cfg, rp, ci, ws, we, D)
        assert rc == _abi.EINVAL and "transit_max" in msg, (D, rc, msg)
    # every check of acs_create_csr_weighted / _scheduled
    for kw in (dict(fault_model="crash", n_faulty=3, crash_window=4), dict(fault_model="byzantine", n_faulty=3),
               dict(loss_p=0.1), dict(trim=1)):   # (loss with SELF)
        rc, msg = _create_t(acsim_lib, cfg.replace(**kw), rp, ci, ws, we, 2)
        assert rc == _abi.EINVAL and msg, (kw, rc, msg)
    down = G.full_schedule(nnz, 3)[1].copy()
    down[7] = 0b011
    rc, msg = _create_t(acsim_lib, cfg, rp, ci, ws, we, 2, (3, down))   # SELF with a down slot
    assert rc == _abi.EINVAL and msg, (rc, msg)
    for period in (33, 64):
        rc, msg = _create_t(acsim_lib, cfg.replace(missing_policy="omit"), rp, ci, ws, we, 2, (period, down))
        assert rc == _abi.EINVAL and "period" in msg, (period, rc, msg)
    heavy = ws.copy()
    heavy[17] += 2.0 ** -20
    rc, msg = _create_t(acsim_lib, cfg, rp, ci, heavy, we, 2)   # column sum above 1
    assert rc == _abi.EINVAL and msg, (rc, msg)
    n = 9000
    deg = np.full(n, 2)
    deg[17] = 8192   # m = 8193 entries
    brp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    bci = (np.arange(int(brp[-1])) % n).astype(np.uint32)
    rc, msg = _create_t(acsim_lib, Config(n_nodes=n, topology="csr", rule="pushsum"), brp, bci, *G.pushsum_weights(brp, bci), 2)
    assert rc == _abi.EUNSUPPORTED and msg, (rc, msg)


def test_existing_entry_points_still_refuse_delay_max(acsim_lib):
    from test_link_schedule import _create_s
    from test_pushsum import _create
    rp, ci, ws, we = _small()
    cfg = Config(**TCFG, delay_max=1, missing_policy="omit")
    rc, msg = _create(acsim_lib, cfg, rp, ci, ws, we)
    assert rc == _abi.EUNSUPPORTED and "delay_max" in msg, (rc, msg)
    rc, msg = _create_s(acsim_lib, cfg, rp, ci, ws, we, *G.full_schedule(ci.size, 2))
    assert rc == _abi.EUNSUPPORTED and "delay_max" in msg, (rc, msg)


def test_simulator_argument_errors():
    rp, ci, ws, we = _small()
    cfg = Config(**TCFG)
    for kw in (dict(transit=2), dict(transit=2, csr=(rp, ci)), dict(transit=2, weights=(ws, we)),
               dict(transit=2, csr=(rp, ci), split=True), dict(transit=-1, csr=(rp, ci), weights=(ws, we)),
               dict(transit=65, csr=(rp, ci), weights=(ws, we)), dict(transit=1.5, csr=(rp, ci), weights=(ws, we))):
        with pytest.raises(ValueError):
            acsim.Simulator(cfg, **kw)
        with pytest.raises(ValueError):
            acsim.simulate(cfg, **kw)


def test_cli_says_which_weights_and_schedule_a_transit_run_used(tmp_path):
    rp, ci = G.random_csr(200, 1, 9, 9)
    sets = ["--set", "rule=pushsum", "--set", "fault_model=none", "--set", "n_faulty=0", "--set", "missing_policy=omit"]
    G.save_csr(str(tmp_path / "g.npz"), rp, ci)
    r = _cli("validate", "--graph", str(tmp_path / "g.npz"), *sets, "--transit", "3")
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout, r.stderr)
    assert "pushsum_weights" in r.stderr and "transit 3" in r.stderr and "no link schedule" in r.stderr, r.stderr
    G.save_csr(str(tmp_path / "s.npz"), rp, ci, weights=G.pushsum_weights(rp, ci), schedule=G.phase_schedule(rp, ci, 4))
    r = _cli("validate", "--graph", str(tmp_path / "s.npz"), *sets, "--transit", "3")
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout, r.stderr)
    assert "transit 3" in r.stderr and "using the link schedule of" in r.stderr and "period 4" in r.stderr, r.stderr
    r = _cli("validate", "--graph", str(tmp_path / "s.npz"), *sets, "--transit", "65")
    assert r.returncode != 0, (r.stdout, r.stderr)
    r = _cli("validate", "--graph", str(tmp_path / "s.npz"), *sets, "--transit", "3", "--split")
    assert r.returncode != 0, (r.stdout, r.stderr)


# ----------------------------------------------------- the restatement: the consequences of the spec
def same_state(p, q):
    assert np.array_equal(p.rounds, q.rounds) and np.array_equal(p.converged, q.converged)
    for u, v in ((p.x, q.x), (p.s, q.s), (p.z, q.z)):
        assert np.array_equal(bits(u), bits(v))
    assert p.trace == q.trace


@pytest.mark.parametrize("sched", [False, True])
@pytest.mark.parametrize("loss", [0.0, 0.3])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c1_transit_bound_zero_is_the_plain_rule_bit_for_bit(dtype, loss, sched):
    """C1: with D = 0 every delta is 0, every arrival is (+0.0) + a = a, and nothing else is delivered."""
    rp, ci = G.random_csr(300, 1, 12, 2)
    w = G.pushsum_weights(rp, ci, dtype=dtype)
    sch = random_masks(ci.size, 5, 3) if sched else None
    cfg = Config(n_nodes=300, topology="csr", rule="pushsum", eps=1e-10 if dtype == "f64" else 1e-5, max_rounds=60, seed=51,
                 trace_spread=True, dtype=dtype, loss_p=loss, missing_policy="omit")
    p = NpSchedPushSumSim(cfg, (rp, ci), w, sch) if sched else NpPushSumSim(cfg, (rp, ci), w)
    q = transit_sim(cfg, (rp, ci), w, 0, sch)
    p.run()
    q.run()
    assert p.rounds[0] > 10
    same_state(p, q)
    assert q.transit(0)[0].shape == (0, ci.size)


def delta0_schedule(cfg, nnz, D, b=0):
    """Period 1, slot e up exactly when the message of round 0 on e is delivered in round 0."""
    dl = S.draw(int(cfg.seed), DELAY, b, 0, np.arange(nnz, dtype=np.uint64)) % np.uint32(D + 1)
    return 1, (dl == 0).astype(np.uint32)


@pytest.mark.parametrize("D", [1, 3, 64])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c2_round_zero_is_the_scheduled_rule_with_the_delta_zero_slots_up(dtype, D):
    """C2: nothing is in transit before round 0, so round 0 delivers exactly the messages with delta = 0:
    the scheduled OMIT rule with period 1 and mask bit (delta(0, e) == 0).  Ties the DELAY draw (stream
    7, the global instance id, the slot) to the schedule path."""
    rp, ci = G.random_csr(300, 1, 12, 2)
    w = G.pushsum_weights(rp, ci, dtype=dtype)
    cfg = Config(n_nodes=300, topology="csr", rule="pushsum", termination="fixed", max_rounds=4, seed=52, dtype=dtype,
                 loss_p=0.2, missing_policy="omit", instance_offset=3)
    sch = delta0_schedule(cfg, ci.size, D, b=3)
    up = int(sch[1].sum())
    assert abs(up - ci.size / (D + 1)) < 4 * math.sqrt(ci.size)   # about one slot in D + 1
    p = NpSchedPushSumSim(cfg, (rp, ci), w, sch)
    q = transit_sim(cfg, (rp, ci), w, D)
    p.round(1)
    q.round(1)
    for u, v in ((p.x, q.x), (p.s, q.s), (p.z, q.z)):
        assert np.array_equal(bits(u), bits(v))
    h, k = q.transit(0)
    assert np.count_nonzero(k.sum(axis=0)) > 0.5 * (ci.size - up)   # the others are in transit (or were dropped)
    p.round(1)
    q.round(1)
    assert not np.array_equal(bits(p.z), bits(q.z))   # round 1 delivers them


def dyadic_cfg(rounds, dtype):
    return Config(n_nodes=301, topology="csr", rule="pushsum", termination="fixed", max_rounds=rounds, seed=5, dtype=dtype)


@pytest.mark.parametrize("D", [2, 4])
@pytest.mark.parametrize("rounds,dtype", [(15, "f64"), (7, "f32")])
def test_mass_is_conserved_exactly_on_dyadic_weights(rounds, dtype, D):
    """C3: odd_circulant(301, 3): every weight is 2^-2 and every column sum is 1.  z starts as integers
    and the planes as 0, so after R rounds every z and every k is a multiple of 2^(-2 R) below 2^2, and
    every sum of them (a cell's fold, a row's tree) is exact while 2 R + 2 <= 53 (fp32: 24).  Nothing is
    rounded and nothing is lost (no loss, no schedule), so fsum(z) + fsum(k planes) is exactly N."""
    assert 2 * rounds + 2 <= (53 if dtype == "f64" else 24)
    rp, ci, w = odd_circulant(301, 3)
    assert np.all(G.column_sums(rp, ci, *w) == 1.0)
    q = transit_sim(dyadic_cfg(rounds, dtype), (rp, ci), w, D)
    q.run()
    h, k = q.transit(0)
    zmass = math.fsum(q.z[0].tolist() + k.reshape(-1).tolist())
    busy = np.count_nonzero(k.sum(axis=0))
    print(f"D={D} {dtype} {rounds} rounds: z mass {zmass!r}, {busy} of {ci.size} slots hold transit mass, "
          f"node z mass {math.fsum(q.z[0].tolist())!r}")
    assert zmass == 301.0 and q.mass(0)[1] == 301.0
    assert busy > 100   # not vacuous: mass is in flight at the end


C4_T = 1.62e-12   # 4 x 4.040e-13, the distance measured on the restatement below (the reference)


def c4_inputs():
    rp, ci = G.random_csr(2000, 1, 12, 3)
    cfg = Config(n_nodes=2000, topology="csr", rule="pushsum", eps=1e-12, max_rounds=500, seed=11, trace_spread=True)
    return cfg, (rp, ci), G.pushsum_weights(rp, ci)


_ref = {}


def c4_reference():
    if "c4" not in _ref:
        cfg, csr, w = c4_inputs()
        q = transit_sim(cfg, csr, w, 3)
        x0 = q.x[0].copy()
        q.run()
        _ref["c4"] = (q, x0)
    return _ref["c4"]


class StaleReadPushSum(NpPushSumSim):
    """What acs_config.delay_max would mean for pairs: in round r slot e carries its sender's PAIR of
    round r - min(r, delta).  One round's offer is then delivered twice or never."""

    def __init__(self, cfg, csr, weights, D):
        super().__init__(cfg, csr, weights)
        self.T, self.ph = D, [(self.s[0].copy(), self.z[0].copy())]

    def _step(self, lb):
        r, ft = int(self.rounds[lb]), self.ft
        dl = (S.draw(self.seed, DELAY, self.gb[lb], r, self.e_slot) % np.uint32(self.T + 1)).astype(np.int64)
        dl = np.where(self.e_self, 0, np.minimum(dl, r))
        hs, hz = np.stack([p[0] for p in self.ph]), np.stack([p[1] for p in self.ph])
        ps = (self.e_w * hs[r - dl, self.e_j]).astype(ft) + ft(0)
        pz = (self.e_w * hz[r - dl, self.e_j]).astype(ft) + ft(0)
        sn, zn = self.row_sums(self.e_row, self.e_pos, ps), self.row_sums(self.e_row, self.e_pos, pz)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.s[lb], self.z[lb], self.x[lb] = sn, zn, np.where(zn > 0, sn / zn, self.x[lb])
        self.ph.append((sn.copy(), zn.copy()))
        self.rounds[lb] = r + 1
        self._after(lb)


def test_c4_transit_finds_the_mean_and_a_stale_read_of_pairs_does_not():
    """C4: random_csr(2000, 1, 12, 3), weights 1 / (outdeg + 1), eps = 1e-12, D = 3, seed 11.
    Measured on this restatement (the reference): it stops after 108 rounds with
    max |x_i - mean(x^0)| = 4.040e-13 and sum z + sum k - N = -5.0e-12.  T = 4 x that = 1.62e-12 (the
    distances over D in {0, 1, 3, 8} and seeds 11 .. 13 span 2.9e-13 .. 6.7e-13, inside the factor 4).
    The stale-read model on the same draws converges too (109 rounds), but to another value: measured
    8.6e-4 away with sum z = 2012.3, and it must end at least 100 T away."""
    q, x0 = c4_reference()
    mean = math.fsum(x0.tolist()) / 2000
    err = float(np.abs(q.x[0] - mean).max())
    mz = q.mass(0)[1]
    print(f"transit D=3: {int(q.rounds[0])} rounds, max |x - mean| = {err:.4e} (T = {C4_T:.3e}), z mass - N = {mz - 2000:.3e}")
    assert q.converged[0] and 60 < q.rounds[0] < 500
    assert err <= C4_T
    assert abs(mz - 2000) < 1e-10   # conserved up to rounding
    assert np.count_nonzero(q.transit(0)[1]) > 1000   # the run stops with mass in transit: the test looks at x alone
    cfg, csr, w = c4_inputs()
    p = StaleReadPushSum(cfg, csr, w, 3)
    p.run()
    serr = float(np.abs(p.x[0] - mean).min())
    print(f"stale read D=3: {int(p.rounds[0])} rounds, min |x - mean| = {serr:.3e}, sum z = {math.fsum(p.z[0].tolist()):.1f}")
    assert p.converged[0] and serr >= 100 * C4_T


def test_resume_on_the_restatement_needs_the_planes():
    rp, ci = G.random_csr(300, 1, 12, 2)
    w = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=300, topology="csr", rule="pushsum", termination="fixed", max_rounds=20, seed=53, loss_p=0.2,
                 missing_policy="omit", n_instances=2)
    straight = transit_sim(cfg, (rp, ci), w, 3)
    straight.round(7)
    s7, z7 = straight.s.copy(), straight.z.copy()
    planes = [straight.transit(lb) for lb in range(2)]
    h7, k7 = np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])
    assert h7.shape == (2, 3, ci.size) and np.count_nonzero(k7) > ci.size
    straight.run()
    for with_planes in (True, False):
        m = transit_sim(cfg, (rp, ci), w, 3)
        m.round(2)   # (something is in transit: restart empties it)
        m.restart(7, s7, z7)
        assert not m.transit(0)[1].any()
        if with_planes:
            m.set_transit(h7, k7)
            assert np.array_equal(bits(m.transit(1)[1]), bits(k7[1]))
        m.run()
        same = all(np.array_equal(bits(u), bits(v)) for u, v in ((m.s, straight.s), (m.z, straight.z)))
        same = same and all(np.array_equal(bits(m.transit(lb)[1]), bits(straight.transit(lb)[1])) for lb in range(2))
        assert same == with_planes


# ------------------------------------------------------------------------------------------ GPU
def kname(path, f32, d, hubs=False, sched=False):
    if path != "fast":
        return "k_round_generic" + (" [f32]" if f32 else "")
    nm = f"k_round_pushsum_transit<{d},csr{',sched' if sched else ''}>" + ("+k_round_generic(hubs)" if hubs else "")
    return nm + (" [f32]" if f32 else "")


def read_all(g, planes=True):
    pairs = [g.pushsum_state(b) for b in range(g.B)]
    out = dict(rounds=g.rounds(), conv=g.converged(), x=g.all_values().reshape(g.B, g.N),
               s=np.stack([p[0] for p in pairs]), z=np.stack([p[1] for p in pairs]),
               trace=[g.spread_trace(b) for b in range(g.B)])
    if planes:
        tr = [g.pushsum_transit(b) for b in range(g.B)]
        out.update(h=np.stack([p[0] for p in tr]), k=np.stack([p[1] for p in tr]))
    return out


def assert_same(got, n, trace_from=0):
    assert np.array_equal(got["rounds"], n.rounds)
    assert np.array_equal(got["conv"], n.converged)
    for key, ref in (("x", n.x), ("s", n.s), ("z", n.z)):
        assert np.array_equal(bits(got[key]), bits(ref)), key
    for b in range(n.B):
        h, k = n.transit(b)
        assert np.array_equal(bits(got["h"][b]), bits(h)), ("h", b)
        assert np.array_equal(bits(got["k"][b]), bits(k)), ("k", b)
        assert np.array_equal(got["trace"][b][trace_from:], np.array(n.trace[b][trace_from:], dtype=np.float64)), b


def reference(key, cfg, csr, w, D, sch=None):
    """The restatement's run, computed once per case and shared by the two paths."""
    if key not in _ref:
        _ref[key] = transit_sim(cfg, csr, w, D, sch)
        _ref[key].run()
    return _ref[key]


def check(key, path, cfg, csr, w, D, sch=None, name=None):
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=csr, weights=w, schedule=sch, transit=D) as g:
        if name:
            assert g.kernel_name() == name
        assert g.transit_max == D
        g.run()
        got = read_all(g)
        mass = g.pushsum_mass(0)
    n = reference(key, cfg, csr, w, D, sch)
    assert_same(got, n)
    assert mass == n.mass(0)
    return got, n


def graph_n(n, dmax, seed):
    """n rows of 0 .. dmax senders with rows of exactly dmax and 0 (uniform senders, repeats allowed)."""
    rng = np.random.default_rng([seed, n])
    deg = rng.integers(0, dmax + 1, n)
    deg[:2] = [dmax, 0]
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    return rp, rng.integers(0, n, int(rp[-1])).astype(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("sched", [False, True])
@pytest.mark.parametrize("loss", [0.0, 0.3])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_c1_bound_zero_equals_the_plain_handle(dtype, loss, sched, path):
    """C1 on the device: identical bits from the plain (or scheduled) handle, another kernel."""
    rp, ci = G.random_csr(300, 1, 12, 2)
    w = G.pushsum_weights(rp, ci, dtype=dtype)
    sch = random_masks(ci.size, 5, 3) if sched else None
    cfg = Config(n_nodes=300, topology="csr", rule="pushsum", termination="fixed", max_rounds=25, seed=51, trace_spread=True,
                 dtype=dtype, loss_p=loss, missing_policy="omit")
    with env(**PATHS[path]):
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w, schedule=sch, transit=0) as g:
            tname = g.kernel_name()
            g.run()
            a = read_all(g)
            with pytest.raises(acsim._abi.AcsError):   # a D = 0 handle has no planes to set
                g.set_pushsum_transit(np.zeros(ci.size), np.zeros(ci.size))
            g.set_pushsum_transit(np.zeros(0), np.zeros(0))
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w, schedule=sch) as g:
            pname = g.kernel_name()
            g.run()
            b = read_all(g, planes=False)
            with pytest.raises(ValueError):
                g.pushsum_transit(0)
            with pytest.raises(acsim._abi.AcsError):   # the calls are EINVAL on any other handle
                g._chk(g._lib.acs_get_pushsum_transit(g._h, 0, None, None, 0))
    assert tname == kname(path, dtype == "f32", 16, sched=sched)
    if path == "fast":
        assert pname == tname.replace("_transit", "")
    assert a["h"].shape == (1, 0, ci.size)
    assert np.array_equal(a["rounds"], b["rounds"]) and np.array_equal(a["conv"], b["conv"])
    for key in ("x", "s", "z"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    assert np.array_equal(a["trace"][0], b["trace"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_c2_round_zero_equals_the_scheduled_handle(dtype, path):
    rp, ci = G.random_csr(300, 1, 12, 2)
    w = G.pushsum_weights(rp, ci, dtype=dtype)
    cfg = Config(n_nodes=300, topology="csr", rule="pushsum", termination="fixed", max_rounds=4, seed=52, dtype=dtype,
                 loss_p=0.2, missing_policy="omit", instance_offset=3, trace_spread=True)
    with env(**PATHS[path]):
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w, transit=3) as g:
            g.round(1)
            a = read_all(g, planes=False)
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w, schedule=delta0_schedule(cfg, ci.size, 3, b=3)) as g:
            g.round(1)
            b = read_all(g, planes=False)
    for key in ("x", "s", "z"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("D", [1, 2, 4, 7])
def test_gpu_ring_wrap(D, path):
    """3 (D + 1) + 2 rounds: every plane of the ring is delivered and refilled three times, with D + 1
    a power of two and not; this is where a wrong cell index shows."""
    rp, ci = graph_n(200, 12, 81)
    w = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=200, topology="csr", rule="pushsum", termination="fixed", max_rounds=3 * (D + 1) + 2, seed=54,
                 trace_spread=True, loss_p=0.2, missing_policy="omit")
    got, n = check(("wrap", D), path, cfg, (rp, ci), w, D, name=kname(path, False, 16))
    assert got["k"].shape == (1, D, ci.size) and np.count_nonzero(got["k"]) > ci.size // 4


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_largest_bound(path):
    rp, ci = graph_n(70, 8, 82)
    w = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=70, topology="csr", rule="pushsum", termination="fixed", max_rounds=140, seed=55, trace_spread=True)
    got, n = check("d64", path, cfg, (rp, ci), w, 64, name=kname(path, False, 8))
    assert np.count_nonzero(got["k"].sum(axis=2)) == 64   # every plane holds something


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dmax,width", [(4, 4), (7, 8), (13, 16), (30, 32)])
def test_gpu_every_compiled_width(dmax, width, path):
    """130 rows: a partial last slice, rows of degree 0, slices narrower than the padded width; random
    masks of period 5 and loss on top."""
    rp, ci = graph_n(130, dmax, 83)
    w = random_ps_weights(rp, ci, 9) if dmax > 4 else G.pushsum_weights(rp, ci)
    sch = random_masks(ci.size, 5, 4)
    cfg = Config(n_nodes=130, topology="csr", rule="pushsum", termination="fixed", max_rounds=20, seed=56, trace_spread=True,
                 loss_p=0.2, missing_policy="omit")
    check(("width", dmax), path, cfg, (rp, ci), w, 3, sch, name=kname(path, False, width, sched=True))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_three_instances_stop_at_different_rounds(path):
    rp, ci = G.random_csr(333, 1, 15, 66)   # every row hears someone: the spread falls to eps
    w = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=333, topology="csr", rule="pushsum", seed=45, trace_spread=True, n_instances=3, mask_group=2,
                 instance_offset=9, loss_p=0.1, missing_policy="omit", eps=1e-9, max_rounds=400)
    got, n = check("inst3", path, cfg, (rp, ci), w, 2, name=kname(path, False, 16))
    assert n.converged.all() and 10 < n.rounds.min() and n.rounds.max() < 400
    assert len(set(n.rounds.tolist())) > 1   # a finished instance's planes stay as they were when it stopped
    assert all(np.count_nonzero(got["k"][b]) > 100 for b in range(3))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_fp32(path):
    rp, ci = graph_n(200, 12, 84)
    w = G.pushsum_weights(rp, ci, dtype="f32")
    cfg = Config(n_nodes=200, topology="csr", rule="pushsum", termination="fixed", max_rounds=20, seed=57, trace_spread=True,
                 loss_p=0.2, missing_policy="omit", dtype="f32")
    check("f32", path, cfg, (rp, ci), w, 3, name=kname(path, True, 16))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_hub_rows_of_every_size_class(path):
    rp, ci = hub_class_graph()
    w = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=rp.size - 1, topology="csr", rule="pushsum", termination="fixed", max_rounds=7, seed=58,
                 trace_spread=True, loss_p=0.1, missing_policy="omit")
    check("hubs", path, cfg, (rp, ci), w, 2, name=kname(path, False, 32, hubs=True))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_hub_rows_under_eps(path):
    rp, ci = heard_hub_graph()
    w = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=rp.size - 1, topology="csr", rule="pushsum", eps=1e-6, max_rounds=300, seed=59, trace_spread=True)
    got, n = check("hubs_eps", path, cfg, (rp, ci), w, 2, name=kname(path, False, 32, hubs=True))
    assert n.converged[0] and n.rounds[0] < 300


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_stepped_rounds_equal_one_run(path):
    rp, ci = graph_n(200, 12, 81)
    w = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=200, topology="csr", rule="pushsum", termination="fixed", max_rounds=17, seed=54, trace_spread=True,
                 loss_p=0.2, missing_policy="omit")   # (test_gpu_ring_wrap's D = 4 case)
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=(rp, ci), weights=w, transit=4) as g:
        for _ in range(17):
            g.round(1)
        got = read_all(g)
    assert_same(got, reference(("wrap", 4), cfg, (rp, ci), w, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_resume_with_mass_in_flight(path):
    """Resume at round 7 with D = 3: 7 is no multiple of D + 1, so relative plane 0 is not ring plane 0."""
    rp, ci = G.random_csr(300, 1, 12, 2)
    w = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=300, topology="csr", rule="pushsum", termination="fixed", max_rounds=20, seed=53, loss_p=0.2,
                 missing_policy="omit", n_instances=2, trace_spread=True)
    n = reference("resume", cfg, (rp, ci), w, 3)
    with env(**PATHS[path]):
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w, transit=3) as g:
            g.round(7)
            st = [g.pushsum_state(b) for b in range(2)]
            tr = [g.pushsum_transit(b) for b in range(2)]
            x7 = g.all_values()
        s7, z7 = np.stack([p[0] for p in st]), np.stack([p[1] for p in st])
        h7, k7 = np.stack([p[0] for p in tr]), np.stack([p[1] for p in tr])
        assert np.count_nonzero(k7) > ci.size
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w, transit=3) as g:   # pairs and planes
            g.set_pushsum_state(7, s7, z7)
            g.set_pushsum_transit(h7, k7)
            back = [g.pushsum_transit(b) for b in range(2)]
            assert all(np.array_equal(bits(back[b][1]), bits(k7[b])) for b in range(2))
            g.run()
            resumed = read_all(g)
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w, transit=3) as g:   # set_state alone: the planes are emptied
            g.round(3)
            g.set_state(7, x7)
            h, k = g.pushsum_transit(1)
            assert not h.any() and not k.any()
            g.run()
            emptied = read_all(g)
            bad, neg = k7.copy(), k7.copy()
            bad[1, 2, 5], neg[1, 2, 5] = np.nan, -1.0
            for hh, kk in ((h7, bad), (bad, k7), (h7, neg), (h7[:, :2], k7[:, :2])):   # NaN, negative k, wrong size
                with pytest.raises(acsim._abi.AcsError):
                    g.set_pushsum_transit(hh, kk)
            g.set_pushsum_transit(-np.zeros_like(h7), -np.zeros_like(k7))   # -0.0 is stored as +0.0
            h, k = g.pushsum_transit(0)
            assert not bits(h).any() and not bits(k).any()
    assert np.array_equal(resumed["rounds"], n.rounds)
    for key, ref in (("s", n.s), ("z", n.z)):   # the pairs and planes never depend on x
        assert np.array_equal(bits(resumed[key]), bits(ref)), key
    m = transit_sim(cfg, (rp, ci), w, 3)
    m.restart(7, s7, z7)
    m.set_transit(h7, k7)
    m.run()
    assert_same(resumed, m, trace_from=7)
    m = transit_sim(cfg, (rp, ci), w, 3)
    m.restart(7, x7)
    m.run()
    assert_same(emptied, m, trace_from=7)
    assert not np.array_equal(bits(emptied["z"]), bits(resumed["z"]))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("D", [2, 4])
def test_gpu_c3_dyadic_mass_is_exactly_n(D, path):
    rp, ci, w = odd_circulant(301, 3)
    with env(**PATHS[path]), acsim.Simulator(dyadic_cfg(15, "f64"), csr=(rp, ci), weights=w, transit=D) as g:
        assert g.kernel_name() == kname(path, False, 4)
        g.run()
        mass = g.pushsum_mass(0)
        h, k = g.pushsum_transit(0)
    assert mass[1] == 301.0 and np.count_nonzero(k.sum(axis=0)) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_c4_converges_to_the_mean(path):
    """Bit-equal to the restatement of test_c4_..., hence within T of the mean."""
    cfg, csr, w = c4_inputs()
    q, x0 = c4_reference()
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=csr, weights=w, transit=3) as g:
        assert g.kernel_name() == kname(path, False, 16)
        g.run()
        got = read_all(g)
    assert_same(got, q)
    assert float(np.abs(got["x"][0] - math.fsum(x0.tolist()) / 2000).max()) <= C4_T
