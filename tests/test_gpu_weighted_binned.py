"""Rule "weighted" on the binned exchange (opt-in, ACSIM_BIN_WEIGHTED=1).

Every test runs on the GPU.  The bar is bit for bit in final values, rounds, converged flags and
spread trace: against the numpy restatement (spec_weighted_np) and, in the same test, against the
same config on the per-lane kernel k_round_weighted<D> (switch off).

Sizes, from binned_levels (binned_plan.hip): one exchange level needs N*d / (P*Q0) >= 64 with
P = ceil(N / SA) source blocks and Q0 = ceil(N / 256) receiver blocks; ACSIM_BIN_SA=64 gives many
ragged source blocks on small graphs.
  3001 nodes, d = 32, SA = 64: P = 47, Q0 = 12, mean run 170 -> one level; the last receiver block
      holds 185 rows, the last source block 57 senders
  3001 nodes, every degree <= 8, SA = 64: mean run 42 -> two levels (k_bin_regroup)
  333 nodes, degrees 0..16, SA = 64: P = 6, Q0 = 2 -> one level, D = 16
  70 nodes, degrees 0..8, SA = 64: one receiver block, its second wave partly empty
Each level count is confirmed by the kernel name.
"""
import contextlib
import os

import numpy as np
import pytest

import acsim
from acsim import graphs as G
from acsim.config import Config
from spec_weighted_np import NpWeightedSim

pytestmark = pytest.mark.gpu

ON = {"ACSIM_BIN_WEIGHTED": 1, "ACSIM_BIN_SA": 64}   # switch on, small source blocks
OFF = {"ACSIM_BIN_WEIGHTED": None, "ACSIM_BIN_SA": 64}   # the same blocks, switch unset
N1 = 3001   # not a multiple of 64 or 256: the last SELL slice and the last receiver block are partial


@contextlib.contextmanager
def env(**kw):
    """Set the variables for the block (None: unset), then restore them."""
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def graph_of(n, seed, hi, head):
    """n rows of degree 0..hi (uniform), the first rows' degrees given by `head`."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, hi + 1, n)
    deg[:len(head)] = head
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    ci = rng.integers(0, n, int(rp[-1])).astype(np.uint32)
    return rp, ci


def gpu_graph():
    """Degrees 0..40 (tests/test_weighted.py's graph): rows of degree 0, rows at exactly 4, 8, 16
    and 32, and hub rows above 32 (under a quarter of the rows)."""
    rp, ci = graph_of(N1, 21, 40, [0, 4, 8, 16, 32, 1, 3, 7, 15, 31, 33, 40])
    deg = np.diff(rp.astype(np.int64))
    assert 0 < (deg > 32).sum() * 4 <= N1
    return rp, ci


def random_weights(rp, seed):
    """Weights in [0, 1] with exact zeros (about 6 % of the edges, 12 % of w_self); a row left all
    zero gets w_self = 0.5 (degree-0 rows among them)."""
    rng = np.random.default_rng(seed)
    n, nnz = rp.size - 1, int(rp[-1])
    ws, we = rng.random(n), rng.random(nnz)
    ws[rng.random(n) < 0.12] = 0.0
    we[rng.random(nnz) < 0.06] = 0.0
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    dead = (ws + np.bincount(rows, weights=we, minlength=n)) == 0
    ws[dead] = 0.5
    return ws, we


# graph name -> (csr, weights, padded degree, hub rows, exchange levels at SA = 64)
_graphs = {}


def graph(name):
    if name not in _graphs:
        if name == "d32_hubs":
            rp, ci = gpu_graph()
            _graphs[name] = ((rp, ci), random_weights(rp, 22), 32, True, 1)
        elif name == "d8_two_levels":
            rp, ci = graph_of(N1, 41, 8, [8, 0, 5, 7, 1])
            _graphs[name] = ((rp, ci), random_weights(rp, 42), 8, False, 2)
        elif name == "d16":
            rp, ci = graph_of(333, 43, 16, [16, 0, 9, 8, 15])
            _graphs[name] = ((rp, ci), random_weights(rp, 44), 16, False, 1)
        elif name == "n70":
            rp, ci = graph_of(70, 45, 8, [8, 0, 5])
            _graphs[name] = ((rp, ci), random_weights(rp, 46), 8, False, 1)
        elif name == "converging":
            # every row hears its ring predecessor on slot 0 and 2..7 random senders, all weights in
            # [0.25, 1): the run converges (38 rounds clean, 43 under loss), with no hub rows
            rng = np.random.default_rng(51)
            n = 1000
            deg = rng.integers(3, 9, n)
            deg[0] = 8
            rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
            ci = rng.integers(0, n, int(rp[-1])).astype(np.uint32)
            ci[rp[:-1].astype(np.int64)] = (np.arange(n) - 1) % n
            w = (rng.random(n) * 0.75 + 0.25, rng.random(ci.size) * 0.75 + 0.25)
            _graphs[name] = ((rp, ci), w, 8, False, 1)
        elif name == "d4":
            rp, ci = graph_of(N1, 47, 4, [4, 0, 3])
            _graphs[name] = ((rp, ci), random_weights(rp, 48), 4, False, 0)
    return _graphs[name]


LOSS = {
    "clean": dict(),
    "loss_self": dict(loss_p=0.3),
    "loss_omit": dict(loss_p=0.4, missing_policy="omit"),
    "loss_02": dict(loss_p=0.2),
    "loss_offset": dict(loss_p=0.3, instance_offset=5, mask_group=2),
    "loss_02_omit": dict(loss_p=0.2, missing_policy="omit"),
}


def cfg_of(gname, case, **over):
    n = graph(gname)[0][0].size - 1
    return Config(**{**dict(n_nodes=n, topology="csr", rule="weighted", eps=1e-9, max_rounds=200, seed=31,
                            trace_spread=True), **LOSS[case], **over})


_ref = {}


def reference(gname, case):
    """The restatement's run of one (graph, case), computed once and shared."""
    if (gname, case) not in _ref:
        csr, w = graph(gname)[:2]
        n = NpWeightedSim(cfg_of(gname, case), csr, w)
        n.run()
        _ref[(gname, case)] = n
    return _ref[(gname, case)]


def binned_name(d, hubs, levels):
    return ("k_bin_scatter+" + ("k_bin_regroup+" if levels == 2 else "") + f"k_bin_gather_w<{d},csr>" +
            ("+k_round_generic(hubs)" if hubs else ""))


def lane_name(d, hubs):
    return f"k_round_weighted<{d},csr>" + ("+k_round_generic(hubs)" if hubs else "")


def run_gpu(cfg, csr, w, name, **envkw):
    """One run to termination under the given environment: (rounds, converged, values, trace)."""
    with env(**envkw), acsim.Simulator(cfg, csr=csr, weights=w) as g:
        assert g.kernel_name() == name
        g.run()
        return g.rounds(), g.converged(), g.values(0), g.spread_trace(0)


def same(a, b):
    assert np.array_equal(a[0], b[0]), (a[0], b[0])
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(bits(a[2]), bits(b[2]))
    assert np.array_equal(bits(a[3]), bits(b[3]))


def check_case(gname, case, envkw=ON):
    csr, w, d, hubs, levels = graph(gname)
    cfg = cfg_of(gname, case)
    on = run_gpu(cfg, csr, w, binned_name(d, hubs, levels), **envkw)
    off = run_gpu(cfg, csr, w, lane_name(d, hubs), **OFF)
    n = reference(gname, case)
    same(on, (n.rounds, n.converged, n.x[0], np.array(n.trace[0], dtype=np.float64)))
    same(on, off)
    return n


# 1. D = 32 with hub rows, one level, ragged source and receiver blocks
@pytest.mark.parametrize("case", ["clean", "loss_self", "loss_omit"])
def test_d32_with_hub_rows(case):
    n = check_case("d32_hubs", case)
    if case == "loss_omit":
        assert n.zero_den > 0   # the zero-denominator keep was exercised


# 2. the same graph in one source block (the default SA)
def test_d32_default_source_block():
    check_case("d32_hubs", "clean", envkw={"ACSIM_BIN_WEIGHTED": 1, "ACSIM_BIN_SA": None})


# 3. D = 8 in two levels (phase M)
@pytest.mark.parametrize("case", ["clean", "loss_02"])
def test_d8_two_levels(case):
    assert "k_bin_regroup+k_bin_gather_w<8,csr>" in binned_name(*graph("d8_two_levels")[2:])
    check_case("d8_two_levels", case)


# 4. D = 16, and one receiver block with a partly empty wave
@pytest.mark.parametrize("case", ["clean", "loss_02"])
@pytest.mark.parametrize("gname", ["d16", "n70"])
def test_d16_and_one_block(gname, case):
    check_case(gname, case)


# an EPS run that converges, on a plan without hub rows: phase B publishes each round's (min, max)
# and the next phase A's workgroups stop on it (1000 nodes, d = 8, SA = 64: P = 16, Q0 = 4, mean
# run 125 -> one level)
@pytest.mark.parametrize("case", ["clean", "loss_02_omit"])
def test_eps_run_converges(case):
    n = check_case("converging", case)
    assert n.converged[0] and 32 < n.rounds[0] < 200   # more than two chunks of 16 rounds


# 5. the drop draws' instance index: bG from instance_offset and mask_group
def test_drop_draw_indexing():
    check_case("d32_hubs", "loss_offset")


# 6. stepping and resume under loss (FIXED 40 rounds: the done exit is not what ends the run)
def test_stepping_and_resume_under_loss():
    csr, w, d, hubs, levels = graph("d32_hubs")
    cfg = cfg_of("d32_hubs", "loss_self", termination="fixed", max_rounds=40)
    name = binned_name(d, hubs, levels)
    one = run_gpu(cfg, csr, w, name, **ON)
    assert one[0][0] == 40
    same(one, run_gpu(cfg, csr, w, lane_name(d, hubs), **OFF))
    for step in (1, 7, 16, 17):   # chunks of 16 rounds: the deferred finalize across round() calls
        with env(**ON), acsim.Simulator(cfg, csr=csr, weights=w) as g:
            assert g.kernel_name() == name
            while not g.round(step).done:
                pass
            same(one, (g.rounds(), g.converged(), g.values(0), g.spread_trace(0)))
    with env(**ON):
        with acsim.Simulator(cfg, csr=csr, weights=w) as g:
            g.round(7)
            x7 = g.values(0)
        with acsim.Simulator(cfg, csr=csr, weights=w) as g:
            g.set_state(7, x7)
            g.run()
            assert np.array_equal(g.rounds(), one[0]) and np.array_equal(bits(g.values(0)), bits(one[2]))


# 7. unit weights: `average`, bit for bit, on its own binned CSR plan and on the oracle
@pytest.mark.parametrize("loss_p", [0.0, 0.15])
def test_unit_weights_equal_average(oracle_mod, loss_p):
    csr, _, d, hubs, levels = graph("d32_hubs")
    cfg = cfg_of("d32_hubs", "clean", loss_p=loss_p, max_rounds=60)
    avg = cfg.replace(rule="average")
    ones = (np.ones(N1), np.ones(csr[1].size))
    wgt = run_gpu(cfg, csr, ones, binned_name(d, hubs, levels), **ON)
    with env(ACSIM_BIN_SA=64), acsim.Simulator(avg, csr=csr) as g:
        assert g.kernel_name().startswith("k_bin_scatter+k_bin_gather<32,0,")
        g.run()
        same(wgt, (g.rounds(), g.converged(), g.values(0), g.spread_trace(0)))
    with oracle_mod.OracleSimulator(avg, threads=8, csr=csr) as o:
        o.run()
        assert np.array_equal(wgt[0], o.rounds())
        assert np.array_equal(bits(wgt[2]), bits(o.values(0)))
        assert np.array_equal(bits(wgt[3]), bits(o.spread_trace(0)))


# 8. fallbacks: with the switch on, today's kernel and today's bits
FALLBACKS = {
    "f32": ("d32_hubs", dict(dtype="f32", eps=1e-5), {}, "k_round_weighted<32,csr>+k_round_generic(hubs) [f32]"),
    "three_instances": ("d32_hubs", dict(n_instances=3), {}, lane_name(32, True)),
    "delay_2": ("d32_hubs", dict(delay_max=2), {}, lane_name(32, True)),
    "crash": ("d32_hubs", dict(fault_model="crash", n_faulty=60, crash_window=4, loss_p=0.15), {}, lane_name(32, True)),
    "byz_split": ("d32_hubs", dict(fault_model="byzantine", n_faulty=60, byz_strategy="split", byz_delta=0.1), {},
                  lane_name(32, True)),
    "degree_4": ("d4", dict(), {}, "k_round_weighted<4,csr>"),
    "pushsum": ("d32_hubs", dict(rule="pushsum"), {}, "k_round_pushsum<32,csr>+k_round_generic(hubs)"),
    "binned_0": ("d32_hubs", dict(), {"ACSIM_BINNED": 0}, lane_name(32, True)),
    "csr_fast_0": ("d32_hubs", dict(), {"ACSIM_CSR_FAST": 0}, "k_round_generic"),
}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_fallbacks_keep_name_and_bits(name):
    gname, over, extra, kname = FALLBACKS[name]
    csr, w = graph(gname)[:2]
    if name == "pushsum":   # (its weights: column sums at most 1)
        w = G.pushsum_weights(*csr)
    cfg = cfg_of(gname, "clean", max_rounds=60, **over)

    def run(**envkw):
        with env(**envkw), acsim.Simulator(cfg, csr=csr, weights=w) as g:
            assert g.kernel_name() == kname
            g.run()
            return g.rounds(), g.converged(), g.all_values(), [g.spread_trace(b) for b in range(g.B)]

    on, off = run(**ON, **extra), run(**OFF, **extra)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert np.array_equal(bits(on[2]), bits(off[2]))
    for a, b in zip(on[3], off[3]):
        assert np.array_equal(bits(a), bits(b))


# 9. the switch is off by default, and "0" is off
@pytest.mark.parametrize("envkw", [{"ACSIM_BIN_WEIGHTED": None}, {"ACSIM_BIN_WEIGHTED": 0}], ids=["unset", "zero"])
def test_switch_off_keeps_the_per_lane_kernel(envkw):
    csr, w, d, hubs, _ = graph("d32_hubs")
    with env(ACSIM_BIN_SA=64, **envkw), acsim.Simulator(cfg_of("d32_hubs", "clean"), csr=csr, weights=w) as g:
        assert g.kernel_name() == lane_name(d, hubs)
