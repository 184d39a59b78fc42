"""Quantized messages for rule "weighted" on the device ("Quantized messages"):
k_round_weighted's QUANT instantiations (+ k_round_generic's rule-5 branch for hub rows) and the
all-generic path (ACSIM_CSR_FAST=0) against the numpy restatement (spec_quant_np), bit for bit in x,
in what the nodes transmit (q), in rounds, converged flags and the spread trace."""
import numpy as np
import pytest

import acsim
from acsim import graphs as G
from acsim.config import Config
from hub_graphs import hub_class_graph, positive_weights
from spec_quant_np import MODES, quant_sim
from test_pushsum import PATHS, big_graph, bits, env
from test_quant import A3_CAP, a1_x0, a2_x0, anchor_cfg, anchor_graph, exact_sum
from test_weighted import random_weights

pytestmark = pytest.mark.gpu
_ref = {}


def kname(path, d, f32=False, hubs=False, sched=False):
    if path != "fast":
        return "k_round_generic" + (" [f32]" if f32 else "")
    return (f"k_round_weighted<{d},csr{',sched' if sched else ''},quant>" + ("+k_round_generic(hubs)" if hubs else "") +
            (" [f32]" if f32 else ""))


def read_all(g):
    return dict(rounds=g.rounds(), conv=g.converged(), x=g.all_values().reshape(g.B, g.N),
                q=np.stack([g.quantized(b) for b in range(g.B)]),
                trace=[g.spread_trace(b) for b in range(g.B)] if g.cfg.trace_spread else None)


def assert_same(got, n, trace_from=0):
    assert np.array_equal(got["rounds"], n.rounds), (got["rounds"], n.rounds)
    assert np.array_equal(got["conv"].astype(bool), n.converged)
    assert got["x"].dtype == n.x.dtype and got["q"].dtype == n.x.dtype
    assert np.array_equal(bits(got["x"]), bits(n.x))
    assert np.array_equal(bits(got["q"]), bits(n.q))
    if got["trace"] is not None:
        for b in range(n.B):
            assert np.array_equal(got["trace"][b][trace_from:], np.array(n.trace[b], dtype=np.float64)[trace_from:]), b


def reference(key, cfg, csr, w, quant, sch=None):
    """The restatement's run, computed once per case and shared by the two paths."""
    if key not in _ref:
        _ref[key] = quant_sim(cfg, csr, w, quant, sch)
        _ref[key].run()
    return _ref[key]


def check(key, path, cfg, csr, w, quant, sch=None, name=None, envkw=None):
    with env(**{**PATHS[path], **(envkw or {})}), acsim.Simulator(cfg, csr=csr, weights=w, schedule=sch, quant=quant) as g:
        if name:
            assert g.kernel_name() == name
        g.run()
        got = read_all(g)
    n = reference(key, cfg, csr, w, quant, sch)
    assert_same(got, n)
    return got, n


# ------------------------------------------------------- the 3001-node graph: D = 32 and hub rows
BIG = {
    "clean": (dict(), 8),
    "loss_self": (dict(loss_p=0.4), 8),
    "loss_omit": (dict(loss_p=0.4, missing_policy="omit"), 8),
    "f32": (dict(dtype="f32"), 10),
}


def big_inputs():
    if "big" not in _ref:
        rp, ci = big_graph()
        _ref["big"] = ((rp, ci), random_weights(rp, 22))
    return _ref["big"]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dither", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(BIG))
def test_gpu_matches_restatement(case, mode, dither, path):
    """Degrees 0 .. 40 on 3001 rows: D = 32 beside hub rows, a partial last block and slice, rows with
    no senders (which transmit and keep averaging with themselves alone); zero weights among the
    entries.  Under OMIT with loss_p = 0.4 some rows lose every positive weight and keep x_i."""
    csr, w = big_inputs()
    kw, k = BIG[case]
    cfg = Config(**{**dict(n_nodes=3001, topology="csr", rule="weighted", termination="fixed", max_rounds=30, seed=31,
                           trace_spread=True), **kw})
    got, n = check((case, mode, dither), path, cfg, csr, w, (k, mode, dither),
                   name=kname(path, 32, f32=case == "f32", hubs=True))
    assert n.rounds[0] == 30
    if case == "loss_omit":
        assert n.zero_den > 0   # the zero-denominator keep was exercised
    step = 2.0 ** -k
    assert np.all(got["q"] / step == np.rint(got["q"] / step)) and np.abs(got["q"] - got["x"]).max() <= step
    assert not np.array_equal(got["q"], got["x"])


# ---------------------------------------------------------------- the narrower compiled widths
def small_graph(dmax, seed):
    rng = np.random.default_rng([seed, dmax])
    n = 333
    deg = rng.integers(0, dmax + 1, n)
    deg[:2] = [dmax, 0]
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    return rp, rng.integers(0, n, int(rp[-1])).astype(np.uint32)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dmax,width,mode", [(4, 4, "partial"), (7, 8, "total"), (13, 16, "compensated")])
def test_gpu_narrow_widths(dmax, width, mode, path):
    """333 rows: more than one block, a partial last slice, slices narrower than the padded width."""
    rp, ci = small_graph(dmax, 91)
    cfg = Config(n_nodes=333, topology="csr", rule="weighted", termination="fixed", max_rounds=25, seed=32, trace_spread=True,
                 loss_p=0.2)
    check(("narrow", dmax), path, cfg, (rp, ci), random_weights(rp, 24), (8, mode, True), name=kname(path, width))


@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_hub_rows_of_every_size_class(path):
    rp, ci = hub_class_graph()
    cfg = Config(n_nodes=rp.size - 1, topology="csr", rule="weighted", termination="fixed", max_rounds=7, seed=58,
                 trace_spread=True, loss_p=0.1, missing_policy="omit")
    check("hubs", path, cfg, (rp, ci), positive_weights(rp, 5), (8, "compensated", True), name=kname(path, 32, hubs=True))


# ------------------------------------------------------------------ instances, schedules, stepping
def heard():
    rp, ci = G.random_csr(333, 1, 15, 66)   # every row hears someone
    return (rp, ci), positive_weights(rp, 6)


def inst3_cfg(**kw):
    return Config(**{**dict(n_nodes=333, topology="csr", rule="weighted", seed=45, trace_spread=True, n_instances=3, mask_group=2,
                            instance_offset=9, loss_p=0.1, eps=1e-12, max_rounds=4000), **kw})


@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_three_instances_stop_at_different_rounds(path):
    """An EPS run of dithered `total`: each instance ends with every node transmitting one grid value,
    at its own round (44, 455 and 919 on the restatement).  x itself is that value up to the rule's
    roundings (a row's tree_sum(w * c) / tree_sum(w) need not return c in the last bit), which is what
    eps = 1e-12 admits.  The dither is drawn per instance (instances 10 and 11 share their loss masks,
    not their dither), and a finished instance's x and q stay as they were when it stopped."""
    csr, w = heard()
    got, n = check("inst3", path, inst3_cfg(), csr, w, (6, "total", True), name=kname(path, 16))
    assert n.converged.all() and n.rounds.max() < 4000 and len(set(n.rounds.tolist())) > 1
    assert all(np.all(got["q"][b] == got["q"][b, 0]) for b in range(3))
    assert np.abs(got["x"] - got["q"]).max() <= 1e-12


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("policy", ["self", "omit"])
def test_gpu_phase_schedule(policy, path):
    csr, w = heard()
    sch = G.phase_schedule(*csr, 4)
    cfg = inst3_cfg(n_instances=1, instance_offset=0, mask_group=1, termination="fixed", max_rounds=30, missing_policy=policy)
    check(("sched", policy), path, cfg, csr, w, (8, "partial", True), sch, name=kname(path, 16, sched=True))


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("step", [1, 7, 16, 17])
def test_gpu_stepped_rounds_equal_one_run(step, path):
    csr, w = heard()
    cfg = inst3_cfg(termination="fixed", max_rounds=34)
    quant = (8, "compensated", True)
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=csr, weights=w, quant=quant) as g:
        for _ in range(-(-34 // step)):   # (the last call is cut short at max_rounds)
            g.round(step)
        got = read_all(g)
    assert_same(got, reference("stepped", cfg, csr, w, quant))


@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_resume_reproduces_the_uninterrupted_run(path):
    """q is a pure function of (x^R, b, R, i): set_state(7, x^7) recomputes it, odd round included."""
    csr, w = heard()
    cfg = inst3_cfg(termination="fixed", max_rounds=20)
    quant = (8, "total", True)
    n = reference("resume", cfg, csr, w, quant)
    with env(**PATHS[path]):
        with acsim.Simulator(cfg, csr=csr, weights=w, quant=quant) as g:
            g.round(7)
            x7, q7 = g.all_values(), np.stack([g.quantized(b) for b in range(3)])
        with acsim.Simulator(cfg, csr=csr, weights=w, quant=quant) as g:
            g.round(2)
            g.set_state(7, x7)
            assert np.array_equal(bits(np.stack([g.quantized(b) for b in range(3)])), bits(q7))
            g.run()
            got = read_all(g)
            with pytest.raises(acsim._abi.AcsError):   # |x| * 2^k must stay finite
                g.set_state(7, np.full(x7.shape, 1e295))
        with acsim.Simulator(cfg, csr=csr, weights=w) as g:   # the getter is EINVAL on any other handle
            with pytest.raises(ValueError):
                g.quantized(0)
            with pytest.raises(acsim._abi.AcsError):
                g._chk(g._lib.acs_get_quantized(g._h, 0, x7.ctypes.data, x7.size))
    assert_same(got, n, trace_from=7)


# ------------------------------------------------------------------------------------ the anchors
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dither", [False, True])
def test_gpu_a1_compensated_keeps_the_sum_exactly(dither, path):
    csr, w = anchor_graph()
    x0 = a1_x0()
    for mode in MODES:
        with env(**PATHS[path]), acsim.Simulator(anchor_cfg(), csr=csr, weights=w, quant=(8, mode, dither)) as g:
            assert g.kernel_name() == kname(path, 4)
            g.set_state(0, x0)
            g.run()
            x = g.values(0)
        assert (exact_sum(x) == exact_sum(x0)) == (mode == "compensated"), mode


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dither", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_gpu_a2_on_the_grid_every_mode_is_plain_weighted(mode, dither, path):
    """As test_quant's A2: the handles agree bit for bit while the state is on the grid (x^1 .. x^4) and
    part at round 5."""
    csr, w = anchor_graph()
    x0 = a2_x0()
    with env(**PATHS[path]), acsim.Simulator(anchor_cfg(), csr=csr, weights=w, quant=(8, mode, dither)) as g, \
            acsim.Simulator(anchor_cfg(), csr=csr, weights=w) as p:
        g.set_state(0, x0)
        p.set_state(0, x0)
        for r in range(1, 6):
            assert np.array_equal(bits(g.quantized(0)), bits(g.values(0))) == (r <= 4), r
            g.round(1)
            p.round(1)
            assert np.array_equal(bits(g.values(0)), bits(p.values(0))) == (r <= 4), r


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("loss", [0.0, 0.3])
def test_gpu_one_round_of_total_is_plain_weighted_on_the_quantized_state(loss, path):
    """Per-round anchor: mode `total` reads nothing but q^r, so a plain `weighted` handle set to
    (r, quantized()) computes the quantized handle's x^{r+1} in its next round, bit for bit."""
    csr, w = big_inputs()
    cfg = Config(n_nodes=3001, topology="csr", rule="weighted", termination="fixed", max_rounds=12, seed=33, loss_p=loss)
    with env(**PATHS[path]), acsim.Simulator(cfg, csr=csr, weights=w, quant=(8, "total", True)) as g, \
            acsim.Simulator(cfg, csr=csr, weights=w) as p:
        for r in (0, 1, 4, 9):
            if r > g.rounds()[0]:
                g.round(r - int(g.rounds()[0]))
            p.set_state(r, g.quantized(0))
            g.round(1)
            p.round(1)
            assert np.array_equal(bits(g.values(0)), bits(p.values(0))), r


@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_a3_dithered_total_agrees_in_finite_time(path):
    """A3's dithered run (452 rounds on the restatement): the same rounds, and every node on one grid value."""
    csr, w = anchor_graph()
    cfg = anchor_cfg(termination="eps", eps=1e-12, max_rounds=A3_CAP, trace_spread=False)
    got, n = check("a3", path, cfg, csr, w, (8, "total", True), name=kname(path, 4))
    assert n.converged[0] and n.rounds[0] < A3_CAP and np.all(got["x"][0] == got["x"][0, 0])


@pytest.mark.parametrize("mode", ["partial", "compensated"])
def test_gpu_binned_plan_is_never_taken(mode):
    """ACSIM_BIN_WEIGHTED=1 gives a plain `weighted` handle of this shape the binned exchange; a
    quantized handle keeps the per-lane kernel, its name and its bits."""
    csr, w = big_inputs()
    cfg = Config(n_nodes=3001, topology="csr", rule="weighted", termination="fixed", max_rounds=30, seed=31, trace_spread=True)
    on = {"ACSIM_BIN_WEIGHTED": 1, "ACSIM_BIN_SA": 64}
    with env(**on), acsim.Simulator(cfg, csr=csr, weights=w) as p:
        assert p.kernel_name().startswith("k_bin_scatter+")
    check(("clean", mode, True), "fast", cfg, csr, w, (8, mode, True), name=kname("fast", 32, hubs=True), envkw=on)
