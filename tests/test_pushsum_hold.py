"""Rule "pushsum" with missing_policy = "hold" (DESIGN.md §9): a dropped message's mass waits on its
link and arrives with the next message that gets through.

CPU part: the ABI and its validation, the numpy restatement (spec_pushsum_hold_np) against the
restatement of the plain rule through the three consequences of the spec, and the mean property
under loss, where OMIT ends visibly away from the mean.
GPU part: k_round_pushsum_hold<D> (+ k_round_generic for hub rows) and the all-generic path
(ACSIM_CSR_FAST=0) against the restatement, bit for bit in x, the (s, z) pairs, the (h, k) links,
rounds, converged flags and the spread trace.
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
from spec_pushsum_hold_np import NpPushSumHoldSim
from spec_pushsum_np import NpPushSumSim
from test_pushsum import PATHS, big_graph, bits, env, heard_graph, random_ps_weights, small_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64p, u32p, dblp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)


# ------------------------------------------------------------------------------- ABI, validation
def test_header_abi_module_and_library_agree(acsim_lib):
    hdr = open(os.path.join(ROOT, "include", "acsim.h")).read()
    assert int(re.search(r"#define\s+ACS_MISSING_HOLD\s+(\d+)", hdr).group(1)) == 2 == _abi.MISSING_HOLD
    assert Config(missing_policy="hold").to_c().missing_policy == 2
    for name in ("acs_get_pushsum_links", "acs_set_pushsum_links"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name           # declared
        assert hasattr(acsim_lib, name), name                            # exported
        assert getattr(acsim_lib, name).argtypes, name                   # bound with a signature
    assert int(re.search(r"#define\s+ACS_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4
    assert acsim_lib.acs_abi_version() == 4 == _abi.ABI_VERSION


def _create_w(lib, cfg, rp, ci, ws, we):
    c = cfg.to_c()
    h = C.c_void_p()
    rp = np.ascontiguousarray(rp, dtype=np.uint64)
    ci = np.ascontiguousarray(ci, dtype=np.uint32)
    ws = np.ascontiguousarray(ws, dtype=np.float64)
    we = np.ascontiguousarray(we, dtype=np.float64)
    rc = lib.acs_create_csr_weighted(C.byref(c), rp.ctypes.data_as(u64p), ci.ctypes.data_as(u32p),
                                     ws.ctypes.data_as(dblp), we.ctypes.data_as(dblp), 0, C.byref(h))
    if rc == _abi.OK:
        lib.acs_destroy(h)
    return rc, lib.acs_last_error().decode()


def _small(dtype="f64"):
    rp, ci = G.random_csr(100, 1, 8, 2)
    return (rp, ci) + G.pushsum_weights(rp, ci, dtype=dtype)


HCFG = dict(n_nodes=100, topology="csr", rule="pushsum", missing_policy="hold")


def _ok(rc, msg):   # validation passed: the handle exists, or the machine has no GPU to make one on
    return rc == _abi.OK or (rc == _abi.EDEVICE and "no HIP device" in msg)


def test_hold_is_accepted_for_pushsum(acsim_lib):
    for kw in (dict(), dict(loss_p=0.3), dict(loss_p=0.2, n_instances=3, mask_group=2, instance_offset=9)):
        assert _ok(*_create_w(acsim_lib, Config(**{**HCFG, **kw}), *_small())), kw
    f32 = Config(**HCFG, dtype="f32", loss_p=0.3, max_rounds=1 << 22)
    assert _ok(*_create_w(acsim_lib, f32, *_small("f32")))


def test_hold_with_any_other_rule_is_einval(acsim_lib):
    h = C.c_void_p()
    rp, ci, ws, we = _small()
    for kw in (dict(rule="average"), dict(rule="trimmed_mean", trim=1)):
        c = Config(n_nodes=16, missing_policy="hold", **kw).to_c()   # acs_create, complete graph
        rc = acsim_lib.acs_create(C.byref(c), _abi.BACKEND_HIP, (C.c_int * 1)(0), 1, C.byref(h))
        msg = acsim_lib.acs_last_error().decode()
        assert rc == _abi.EINVAL and "HOLD" in msg and "PUSHSUM" in msg, (kw, rc, msg)
        c = Config(n_nodes=100, topology="csr", missing_policy="hold", **kw).to_c()   # acs_create_csr
        rc = acsim_lib.acs_create_csr(C.byref(c), rp.ctypes.data_as(u64p), ci.ctypes.data_as(u32p), 0, C.byref(h))
        msg = acsim_lib.acs_last_error().decode()
        assert rc == _abi.EINVAL and "HOLD" in msg and "PUSHSUM" in msg, (kw, rc, msg)
    rc, msg = _create_w(acsim_lib, Config(**{**HCFG, "rule": "weighted"}), rp, ci, ws, we)
    assert rc == _abi.EINVAL and "HOLD" in msg and "PUSHSUM" in msg, (rc, msg)


def test_what_stays_rejected(acsim_lib):
    rp, ci, ws, we = _small()
    rc, msg = _create_w(acsim_lib, Config(**{**HCFG, "missing_policy": 3}), rp, ci, ws, we)
    assert rc == _abi.EINVAL and "missing_policy" in msg, (rc, msg)
    for code, kw in ((_abi.EINVAL, dict(fault_model="crash", n_faulty=3, crash_window=4)),
                     (_abi.EINVAL, dict(fault_model="byzantine", n_faulty=3)),
                     (_abi.EUNSUPPORTED, dict(delay_max=1))):
        for policy in ("hold", "omit"):   # as for OMIT
            rc, msg = _create_w(acsim_lib, Config(**{**HCFG, **kw, "missing_policy": policy}), rp, ci, ws, we)
            assert rc == code and msg, (kw, policy, rc, msg)
    rc, msg = _create_w(acsim_lib, Config(**{**HCFG, "missing_policy": "self", "loss_p": 0.1}), rp, ci, ws, we)
    assert rc == _abi.EINVAL and "SELF" in msg, (rc, msg)


def test_cli_validates_a_hold_run(tmp_path):
    from test_pushsum import _cli
    rp, ci = G.random_csr(200, 1, 9, 9)
    G.save_csr(str(tmp_path / "g.npz"), rp, ci)
    r = _cli("validate", "--graph", str(tmp_path / "g.npz"), "--set", "rule=pushsum", "--set", "loss_p=0.2",
             "--set", "missing_policy=hold", "--set", "fault_model=none", "--set", "n_faulty=0")
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout, r.stderr)


# --------------------------------------------------- the restatement against the plain restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_lossless_hold_is_the_plain_rule_bit_for_bit(dtype):
    """Consequence 1: with loss_p = 0 every link is +0.0 on entry and hn = a exactly."""
    rp, ci = G.random_csr(300, 1, 8, 2)
    w = G.pushsum_weights(rp, ci, dtype=dtype)
    cfg = Config(n_nodes=300, topology="csr", rule="pushsum", eps=1e-10 if dtype == "f64" else 1e-5, max_rounds=300,
                 seed=51, trace_spread=True, dtype=dtype)
    p = NpPushSumSim(cfg, (rp, ci), w)
    q = NpPushSumHoldSim(cfg.replace(missing_policy="hold"), (rp, ci), w)
    p.run()
    q.run()
    assert p.rounds[0] > 10   # (by the eps test or at max_rounds: the equality is what matters)
    assert np.array_equal(p.rounds, q.rounds)
    for u, v in ((p.x, q.x), (p.s, q.s), (p.z, q.z)):
        assert np.array_equal(bits(u), bits(v))
    assert p.trace == q.trace
    assert not q.h.any() and not q.k.any()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_first_lossy_round_is_omits_and_later_rounds_are_not(dtype):
    """Consequence 2: from empty links hn = a, so round 1 delivers what OMIT delivers; from round 2 on
    the held mass arrives and the two differ."""
    rp, ci = G.random_csr(300, 1, 8, 2)
    w = G.pushsum_weights(rp, ci, dtype=dtype)
    cfg = Config(n_nodes=300, topology="csr", rule="pushsum", loss_p=0.4, missing_policy="omit", termination="fixed",
                 max_rounds=6, seed=52, dtype=dtype)
    p = NpPushSumSim(cfg, (rp, ci), w)
    q = NpPushSumHoldSim(cfg.replace(missing_policy="hold"), (rp, ci), w)
    p.round(1)
    q.round(1)
    for u, v in ((p.x, q.x), (p.s, q.s), (p.z, q.z)):
        assert np.array_equal(bits(u), bits(v))
    held = np.count_nonzero(q.k[0])
    assert 0.3 * ci.size < held < 0.5 * ci.size   # about loss_p of the links hold mass
    assert not q.h[0, :300].any() and not q.k[0, :300].any()   # entry 0 has no link
    p.round(1)
    q.round(1)
    assert np.count_nonzero(bits(p.z[0]) != bits(q.z[0])) > 150
    p.round(4)
    q.round(4)
    assert np.count_nonzero(bits(p.x[0]) != bits(q.x[0])) > 150


def odd_circulant(n, d):
    """Receiver i hears i+1, i+3, .., i+2d-1 (mod n): every node has d listeners and itself, so with
    all weights 1 / (d + 1) every column sum is 1 (2d - 1 < n: the listeners are distinct)."""
    rp = (np.arange(n + 1) * d).astype(np.uint64)
    ci = ((np.arange(n)[:, None] + 1 + 2 * np.arange(d)[None, :]) % n).astype(np.uint32).reshape(-1)
    w = 1.0 / (d + 1)
    return rp, ci, (np.full(n, w), np.full(ci.size, w))


def dyadic_cfg(rounds, dtype, policy):
    return Config(n_nodes=301, topology="csr", rule="pushsum", loss_p=0.4, missing_policy=policy, termination="fixed",
                  max_rounds=rounds, seed=5, dtype=dtype)


@pytest.mark.parametrize("d,rounds,dtype", [(3, 20, "f64"), (3, 9, "f32"), (15, 12, "f64")])
def test_mass_is_conserved_exactly_on_dyadic_weights(d, rounds, dtype):
    """Consequence 3: every weight is 2^-k (k = log2(d + 1)) and every column sum is 1.  z and k start
    as integers, so after R rounds every value is a multiple of 2^(-k R) below 2^2 and every sum of
    them in a row is exact while k R + 2 <= 53 (fp32: 24): nothing is rounded, and the exact identity
    sum(z) + sum(k) = N holds in floating point.  Under OMIT the same run loses most of its mass
    (each round a share loss_p d / (d + 1) >= 0.3 of it), so the equality is not vacuous."""
    k = int(math.log2(d + 1))
    assert 2 ** k == d + 1 and k * rounds + 2 <= (53 if dtype == "f64" else 24)
    rp, ci, w = odd_circulant(301, d)
    assert np.all(G.column_sums(rp, ci, *w) == 1.0)
    q = NpPushSumHoldSim(dyadic_cfg(rounds, dtype, "hold"), (rp, ci), w)
    q.run()
    zmass = math.fsum(q.z[0].tolist() + q.k[0].tolist())
    held = np.count_nonzero(q.k[0])
    p = NpPushSumSim(dyadic_cfg(rounds, dtype, "omit"), (rp, ci), w)
    p.run()
    omit = math.fsum(p.z[0].tolist())
    print(f"d={d} {dtype} {rounds} rounds: hold z mass {zmass!r} ({held} links hold mass), OMIT z mass {omit:.3g}")
    assert zmass == 301.0 and q.mass(0)[1] == 301.0
    assert held > 100
    assert omit < 301.0 / 2
    assert np.all(bits(p.x[0]) != bits(q.x[0]))


# ----------------------------------------------------------------------------- the mean property
def longest_open_drop_streak(cfg, nnz, R):
    """The longest run of consecutive dropped rounds R-1, R-2, .. on any one slot, from the DROP
    draws alone (one instance, instance_offset 0)."""
    thr = np.uint32(S.drop_threshold(cfg.loss_p))
    alive = np.arange(nnz, dtype=np.uint64)
    L = 0
    while alive.size and L < R:
        alive = alive[S.draw(int(cfg.seed), S.DROP, 0, R - 1 - L, alive) < thr]
        L += alive.size > 0
    return L


def test_hold_finds_the_mean_under_loss_and_omit_does_not():
    """Directed graph, weights 1 / (outdeg + 1), loss_p = 0.4, eps = 1e-12.  After R rounds every x_i
    lies within
        B = W + (2 L + 6) 2^-53 max|x^0| + 2 R (ceil(log2 m_max) + k_max + 5) 2^-53 max|x^0|
    of fsum(x^0) / N, where L is the longest run of drops still open on any link at the end and W
    the width of the hull of x^(R-L) .. x^R.  Derivation:
    (1) Total mass.  S* = sum_i s_i + sum_e h_e and Z* = sum_i z_i + sum_e k_e.  In exact arithmetic
        a message's mass goes to its receiver or stays on its link, so a round multiplies sender j's
        share by its column sum c_j, whether messages are lost or not, and 1 - 3 * 2^-53 <= c_j <= 1
        (test_pushsum.py, step (2)).  The roundings of a round: one per product, one for the link
        add (the new one), and ceil(log2 m_i) tree levels, each relative to sum |p_e|:
        |S*' - S*| <= (ceil(log2 m_max) + k_max + 5) 2^-53 (sum |s| + sum |h|), one more than the
        plain rule's bound, and sum |s| + sum |h| <= N max|x^0| (column sums <= 1, x^0 >= 0); the
        same for Z* against N.  After R rounds S* / Z* is within the third term of the mean (step (3)
        of test_pushsum.py: max|x^0| <= 1 scales the Z term).
    (2) Where S* / Z* lies.  S / Z (node sums) is a mean of the x_i^R with weights z_i >= 0.  A link
        that has dropped its last l <= L messages holds h_e = sum_q w s_j^q and k_e = sum_q w z_j^q
        over those rounds q in [R - l, R - 1], so h_e / k_e is a mean of x_j^q with weights
        w z_j^q >= 0, and H / K (link sums) a mean of those.  S* / Z* = (Z (S / Z) + K (H / K)) / (Z + K)
        is a mean of the two.  All of these, and x_i^R itself, lie in the hull of x^(R-L) .. x^R,
        whose width is W: |x_i^R - S* / Z*| <= W.  Each x is a rounded divide and each h_e, k_e is
        l rounded adds of rounded products, which moves a ratio by at most (2 L + 6) 2^-53 max|x^0|
        (the second term).
    L comes from the drop draws and W from the spreads the run itself reports; on this run L is
    about log(nnz) / log(1 / loss_p) = 10 rounds and W a few 1e-11, far below what OMIT's lost mass
    does: the same run under OMIT converges more than 1e-4 away from the mean."""
    n = 2000
    rp, ci = G.random_csr(n, 1, 12, 3)
    ws, we = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=n, topology="csr", rule="pushsum", eps=1e-12, max_rounds=500, seed=11, loss_p=0.4,
                 missing_policy="hold")
    q = NpPushSumHoldSim(cfg, (rp, ci), (ws, we))
    x0 = q.x[0].copy()
    mean = math.fsum(x0.tolist()) / n
    q.run()
    R = int(q.rounds[0])
    m_max = int(np.diff(rp.astype(np.int64)).max()) + 1
    k_max = int(np.bincount(ci, minlength=n).max()) + 1
    L = longest_open_drop_streak(cfg, ci.size, R)
    hull = np.stack(q.hist[0][R - L:R + 1])
    W = float(hull.max() - hull.min())
    xmax = float(np.abs(x0).max())
    B = W + (2 * L + 6) * 2.0 ** -53 * xmax + 2 * R * (math.ceil(math.log2(m_max)) + k_max + 5) * 2.0 ** -53 * xmax
    err = float(np.abs(q.x[0] - mean).max())
    ms, mz = q.mass(0)
    print(f"hold: {R} rounds, max |x - mean| = {err:.3e}, bound {B:.3e} (L = {L}, W = {W:.3e}), "
          f"z mass - N = {mz - n:.3e}, s mass / N - mean = {ms / n - mean:.3e}")
    assert q.converged[0] and R < 500
    assert 0 < L < R
    assert err <= B
    assert B < 1e-9   # the bound separates the two policies: OMIT below is five orders away
    p = NpPushSumSim(cfg.replace(missing_policy="omit"), (rp, ci), (ws, we))
    p.run()
    oerr = float(np.abs(p.x[0] - mean).min())
    print(f"omit: {int(p.rounds[0])} rounds, min |x - mean| = {oerr:.3e}")
    assert p.converged[0] and oerr > 1e-4


# ------------------------------------------------------------------------------------------ GPU
N_BIG = 3001
_ref = {}


def big_cfg(dtype, **over):
    return Config(**{**dict(n_nodes=N_BIG, topology="csr", rule="pushsum", seed=45, trace_spread=True, loss_p=0.4,
                            missing_policy="hold", termination="fixed", max_rounds=30, dtype=dtype), **over})


def big_inputs():
    rp, ci = big_graph()
    return rp, ci, random_ps_weights(rp, ci, 8)


def big_reference(dtype):
    """The restatement's 30 lossy rounds on big_graph, computed once per dtype and shared."""
    if dtype not in _ref:
        rp, ci, w = big_inputs()
        n = NpPushSumHoldSim(big_cfg(dtype), (rp, ci), w)
        n.run()
        _ref[dtype] = n
    return _ref[dtype]


def kname(path, f32, d=32, hubs=True, kernel="k_round_pushsum_hold"):
    nm = f"{kernel}<{d},csr>" + ("+k_round_generic(hubs)" if hubs else "") if path == "fast" else "k_round_generic"
    return nm + (" [f32]" if f32 else "")


def read_all(g, links=True):
    pairs = [g.pushsum_state(b) for b in range(g.B)]
    out = dict(rounds=g.rounds(), conv=g.converged(), x=g.all_values(), s=np.stack([p[0] for p in pairs]),
               z=np.stack([p[1] for p in pairs]), trace=[g.spread_trace(b) for b in range(g.B)])
    if links:
        lk = [g.pushsum_links(b) for b in range(g.B)]
        out.update(h=np.stack([p[0] for p in lk]), k=np.stack([p[1] for p in lk]))
    return out


def assert_same(got, n, trace_from=0):
    assert np.array_equal(got["rounds"], n.rounds)
    assert np.array_equal(got["conv"], n.converged)
    for key, ref in (("x", n.x), ("s", n.s), ("z", n.z), ("h", n.h[:, n.N:]), ("k", n.k[:, n.N:])):
        assert np.array_equal(bits(got[key]), bits(ref)), key
    for b in range(n.B):
        assert np.array_equal(got["trace"][b][trace_from:], np.array(n.trace[b][trace_from:], dtype=np.float64)), b


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_big_graph_matches_restatement(dtype, path):
    """3001 nodes, degrees 0 .. 40: D = 32 plus hub rows, a partial last block and SELL slice, rows
    with no senders."""
    rp, ci, w = big_inputs()
    cfg = big_cfg(dtype)
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
        assert g.kernel_name() == kname(path, dtype == "f32")
        g.run()
        got = read_all(g)
        mass = g.pushsum_mass(0)
    n = big_reference(dtype)
    assert np.count_nonzero(n.k[0]) > 1000   # links hold mass at the end
    assert_same(got, n)
    assert mass == n.mass(0)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dmax,D", [(3, 4), (7, 8), (15, 16)])
def test_gpu_narrow_widths(dmax, D, path):
    rp, ci = small_graph(dmax, 50 + dmax)
    w = random_ps_weights(rp, ci, 9)
    cfg = Config(n_nodes=333, topology="csr", rule="pushsum", eps=1e-9, max_rounds=60, seed=46, loss_p=0.2,
                 missing_policy="hold", trace_spread=True)
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
        assert g.kernel_name() == kname(path, False, D, hubs=False)
        g.run()
        got = read_all(g)
    key = ("narrow", dmax)
    if key not in _ref:
        _ref[key] = NpPushSumHoldSim(cfg, (rp, ci), w)
        _ref[key].run()
    assert_same(got, _ref[key])


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_three_instances_group_and_offset(path):
    rp, ci = heard_graph()
    w = G.pushsum_weights(rp, ci)
    cfg = Config(n_nodes=N_BIG, topology="csr", rule="pushsum", seed=45, trace_spread=True, n_instances=3, mask_group=2,
                 instance_offset=5, loss_p=0.3, missing_policy="hold", eps=1e-9, max_rounds=200)
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
        g.run()
        got = read_all(g)
    if "inst3" not in _ref:
        _ref["inst3"] = NpPushSumHoldSim(cfg, (rp, ci), w)
        _ref["inst3"].run()
    n = _ref["inst3"]
    assert n.converged.all() and 10 < n.rounds.min() and n.rounds.max() < 200   # stopped by the eps test
    # instances 6 and 7 share a drop mask (group 6), instance 5 has its own: the same links hold mass
    assert np.array_equal(n.k[1] != 0, n.k[2] != 0) or n.rounds[1] != n.rounds[2]
    assert_same(got, n)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_lossless_hold_equals_omit_handle(dtype, path):
    """Consequence 1 on the device: identical bits, different kernels."""
    rp, ci, w = big_inputs()
    cfg = big_cfg(dtype, loss_p=0.0)
    with env(**PATHS[path]):
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
            hold_name = g.kernel_name()
            g.run()
            a = read_all(g)
        with acsim.Simulator(cfg.replace(missing_policy="omit"), csr=(rp, ci), weights=w) as g:
            omit_name = g.kernel_name()
            g.run()
            b = read_all(g, links=False)
    assert hold_name == kname(path, dtype == "f32")
    assert omit_name == kname(path, dtype == "f32", kernel="k_round_pushsum")
    if path == "fast":
        assert hold_name != omit_name
    assert np.array_equal(a["rounds"], b["rounds"]) and np.array_equal(a["conv"], b["conv"])
    for key in ("x", "s", "z"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    assert np.array_equal(a["trace"][0], b["trace"][0])
    assert not a["h"].any() and not a["k"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_dyadic_mass_is_exactly_n(path):
    rp, ci, w = odd_circulant(301, 3)
    with env(**PATHS[path]), acsim.Simulator(dyadic_cfg(20, "f64", "hold"), csr=(rp, ci), weights=w) as g:
        assert g.kernel_name() == kname(path, False, 4, hubs=False)
        g.run()
        mass = g.pushsum_mass(0)
        h, k = g.pushsum_links(0)
    with env(**PATHS[path]), acsim.Simulator(dyadic_cfg(20, "f64", "omit"), csr=(rp, ci), weights=w) as g:
        g.run()
        omit = g.pushsum_mass(0)   # without HOLD: the node sums alone
        with pytest.raises(acsim._abi.AcsError):   # the link calls are HOLD's alone
            g.pushsum_links(0)
    assert mass[1] == 301.0 and np.count_nonzero(k) > 100
    assert omit[1] < 301.0 / 2


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_f32_mass_survives_200_lossy_rounds(path):
    """The shape on which OMIT's z decays through the subnormals to 0 (test_pushsum.py): under HOLD no
    z reaches 0 and the z mass Z* = sum z + sum k stays within
        N (1 - 2^-22)^R (1 - u)^(15 R) <= Z* <= N (1 + u)^(15 R),   u = 2^-24, R = 200.
    A round multiplies sender j's share of Z* by its column sum, which for these binary32 weights
    lies in [1 - 2^-22, 1] (k_j weights within 2^-22 / k_j of 1 / k_j, never above), and rounds every
    entry at most 15 times: the product, the link add and up to 13 tree levels (rows of at most
    8192 entries), each by a factor in [1 - u, 1 + u] on non-negative terms.  That holds while no
    value is subnormal, which the test checks: the smallest positive z or k stays above 2^-60."""
    rng = np.random.default_rng(61)
    deg = rng.integers(8, 16, 333)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    ci = rng.integers(0, 333, int(rp[-1])).astype(np.uint32)
    w = G.pushsum_weights(rp, ci, dtype="f32")
    cfg = Config(n_nodes=333, topology="csr", rule="pushsum", dtype="f32", termination="fixed", max_rounds=200, seed=47,
                 loss_p=0.5, missing_policy="hold", trace_spread=True)
    if "f32mass" not in _ref:
        n = NpPushSumHoldSim(cfg, (rp, ci), w)
        low = np.inf
        for _ in range(200):
            n.round(1)
            low = min(low, float(n.z[0].min()), float(n.k[0][n.k[0] > 0].min()))
        _ref["f32mass"] = (n, low)
    n, low = _ref["f32mass"]
    assert low > 2.0 ** -60
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
        g.run()
        got = read_all(g)
        mass = g.pushsum_mass(0)
    assert_same(got, n)
    assert np.all(got["z"] > 0)
    u, R = 2.0 ** -24, 200
    lo, hi = 333 * (1 - 2.0 ** -22) ** R * (1 - u) ** (15 * R), 333 * (1 + u) ** (15 * R)
    print(f"f32 z mass after {R} rounds: {mass[1]!r} in [{lo!r}, {hi!r}]")
    assert lo <= mass[1] <= hi


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_stepped_rounds_equal_one_run(path):
    rp, ci, w = big_inputs()
    with env(**PATHS[path]), acsim.Simulator(big_cfg("f64"), csr=(rp, ci), weights=w) as g:
        for k in (1, 7, 16, 17):
            g.round(k)
        got = read_all(g)
    assert_same(got, big_reference("f64"))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_resume_with_links(path):
    rp, ci, w = big_inputs()
    cfg = big_cfg("f64")
    n = big_reference("f64")
    with env(**PATHS[path]):
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
            g.round(9)
            s9, z9 = g.pushsum_state(0)
            h9, k9 = g.pushsum_links(0)
        assert np.count_nonzero(k9) > 1000
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:   # pairs and links
            g.set_pushsum_state(9, s9, z9)
            g.set_pushsum_links(h9, k9)
            g.run()
            resumed = read_all(g)
        with acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:   # pairs alone: the held mass is gone
            g.round(3)   # (links hold mass now; set_pushsum_state empties them)
            g.set_pushsum_state(9, s9, z9)
            h, k = g.pushsum_links(0)
            assert not h.any() and not k.any()
            g.run()
            no_links = read_all(g)
            bad = k9.copy()
            bad[5] = np.nan
            neg = k9.copy()
            neg[5] = -1.0
            for hh, kk in ((h9, bad), (bad, k9), (h9, neg), (h9[:-1], k9[:-1])):   # NaN, negative k, wrong size
                with pytest.raises(acsim._abi.AcsError):
                    g.set_pushsum_links(hh, kk)
            g.set_pushsum_links(-np.zeros_like(h9), -np.zeros_like(k9))   # -0.0 is stored as +0.0
            h, k = g.pushsum_links(0)
            assert not bits(h).any() and not bits(k).any()
        with acsim.Simulator(cfg.replace(missing_policy="omit"), csr=(rp, ci), weights=w) as g:
            with pytest.raises(acsim._abi.AcsError):   # the link calls are EINVAL on an OMIT push-sum handle
                g.pushsum_links(0)
            with pytest.raises(acsim._abi.AcsError):
                g.set_pushsum_links(h9, k9)
    # the pairs and links never depend on x: the resumed run's are the straight run's.  x is recomputed
    # from the pairs at the resume, so it can differ only where z is 0 (rows that kept an older x).
    assert np.array_equal(resumed["rounds"], n.rounds)
    for key, ref in (("s", n.s), ("z", n.z), ("h", n.h[:, N_BIG:]), ("k", n.k[:, N_BIG:])):
        assert np.array_equal(bits(resumed[key]), bits(ref)), key
    live = n.z > 0
    assert np.array_equal(bits(resumed["x"][live]), bits(n.x[live]))
    # and both resumed runs are the restatement's, restarted the same way
    m = NpPushSumHoldSim(cfg, (rp, ci), w)
    m.restart(9, s9, z9)
    m.set_links(h9, k9)
    m.run()
    assert_same(resumed, m, trace_from=9)   # (a resumed handle has no earlier spreads)
    m = NpPushSumHoldSim(cfg, (rp, ci), w)
    m.restart(9, s9, z9)
    m.run()
    assert_same(no_links, m, trace_from=9)
    assert not np.array_equal(bits(no_links["z"]), bits(resumed["z"]))   # another run
