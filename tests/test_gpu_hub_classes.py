"""Rules "weighted" and "pushsum" on hub rows of every size class of k_round_generic (GPU).

A handle of these rules sends every row above 32 senders to k_round_generic, whose branches for them
(their own weight indexing, link update and schedule lookup, two LDS tree sums each) run on blocks of
64, 256 and 1024 threads by size class.  tests/hub_graphs.py's graph has a hub row at both ends of
every class, up to the 8192-entry row that takes the largest dynamic-LDS launch, so every case below
runs every instantiation, beside the lane kernel (fast) and alone (ACSIM_CSR_FAST=0: generic).

Every case compares x, rounds, converged flags and the spread trace with the numpy restatement bit
for bit, for push-sum also the (s, z) pairs and under HOLD the (h, k) links in slot order, hub rows'
slots included, and asserts the kernel name.  The last test holds one round of the handle itself
against exact rational arithmetic (hub_graphs.check_exact_round), independent of the numpy code.
"""
import numpy as np
import pytest

import acsim
import spec_np as S
from acsim import graphs as G
from acsim.config import Config
from hub_graphs import (N_HUB_GRAPH, admission_graph, check_exact_round, handle_state, heard_hub_graph, hub_class_graph,
                        hub_rows, hub_slots, positive_weights)
from spec_sched_np import plain_sim, sched_sim
from test_link_schedule import (PAIRS, assert_same, assert_same_handles, cached, env, kname, random_masks,  # noqa: F401
                                read_all, run_handle, weights_for)
from test_pushsum import PATHS, bits

N = N_HUB_GRAPH
ROUNDS = 12


def graph():
    return cached(("hub", "graph"), hub_class_graph)


def heard():
    return cached(("hub", "heard"), heard_hub_graph)


def masks(nnz):
    return random_masks(nnz, 5, 14)


def hub_cfg(pair, dtype="f64", **over):
    return Config(**{**dict(n_nodes=N, topology="csr", seed=81, trace_spread=True, termination="fixed", max_rounds=ROUNDS,
                            loss_p=0.2, dtype=dtype), **PAIRS[pair], **over})


def restatement(cfg, csr, w, sch):
    return plain_sim(cfg, csr, w) if sch is None else sched_sim(cfg, csr, w, sch)


def reference(key, cfg, csr, w, sch):
    """The restatement's whole run, computed once per key and left unchanged."""
    def make():
        n = restatement(cfg, csr, w, sch)
        n.run()
        return n
    return cached(("hub",) + key, make)


def check(key, cfg, csr, w, sch, pair, path, hubs=True):
    name, got = run_handle(cfg, csr, w, sch)
    assert name == kname(pair, path, cfg.dtype == "f32", hubs=hubs, sched=sch is not None)
    n = reference(key, cfg, csr, w, sch)
    assert_same(got, n)
    return got, n


def hub_links_hold_mass(n, rp):
    """Every instance of a HOLD restatement ends with mass on links of every hub row."""
    hs = hub_slots(rp)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp.astype(np.int64)))
    for lb in range(n.B):
        k = n.k[lb, n.N:]
        assert np.count_nonzero(k[hs]) > 1000
        assert set(rows[hs & (k != 0)].tolist()) == set(hub_rows(rp).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("sched", [False, True], ids=["plain", "sched5"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_gpu_every_size_class_matches_restatement(env, pair, sched, dtype, path):
    """650 nodes, hub rows of 34 .. 8192 entries, loss_p = 0.2, 12 FIXED rounds, weights with exact zeros."""
    rp, ci = graph()
    w = weights_for(pair, rp, ci)
    env(**PATHS[path])
    _, n = check(("grid", pair, sched, dtype), hub_cfg(pair, dtype), (rp, ci), w, masks(ci.size) if sched else None, pair, path)
    if pair == "pushsum_hold":
        hub_links_hold_mass(n, rp)   # the hub rows' link stores were exercised


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("pair", ["pushsum_hold", "weighted_self"])
def test_gpu_three_instances_group_and_offset(env, pair, path):
    """Instances 5, 6, 7 in mask groups 4 and 6: the per-instance link stride and bG on hub rows."""
    rp, ci = graph()
    w = weights_for(pair, rp, ci)
    cfg = hub_cfg(pair, n_instances=3, mask_group=2, instance_offset=5)
    env(**PATHS[path])
    got, n = check(("inst3", pair), cfg, (rp, ci), w, masks(ci.size), pair, path)
    assert not np.array_equal(bits(n.x[0]), bits(n.x[1])) and not np.array_equal(bits(n.x[1]), bits(n.x[2]))
    if pair == "pushsum_hold":
        hub_links_hold_mass(n, rp)
        assert np.array_equal(n.k[1] != 0, n.k[2] != 0)       # instances 6 and 7 share their drops,
        assert not np.array_equal(n.k[0] != 0, n.k[1] != 0)   # instance 5 has its own


CRASH = dict(fault_model="crash", n_faulty=160, crash_window=6, delay_max=2)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("sched", [False, True], ids=["plain", "sched5"])
@pytest.mark.parametrize("pair", ["weighted_self", "weighted_omit"])
def test_gpu_weighted_crash_faults_and_delays(env, pair, sched, path):
    """generic_entry's delay and status path from 256- and 1024-thread blocks: a quarter of the nodes
    crash within 6 rounds, hub rows among them, and messages are up to 2 rounds old."""
    rp, ci = graph()
    w = weights_for(pair, rp, ci)
    env(**PATHS[path])
    _, n = check(("crash", pair, sched), hub_cfg(pair, **CRASH), (rp, ci), w, masks(ci.size) if sched else None, pair, path)
    st = n.status[0][hub_rows(rp)]
    assert 0 < np.count_nonzero(st != S.HONEST) < st.size   # hub rows that crash and hub rows that do not


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_weighted_byzantine_split(env, path):
    rp, ci = graph()
    w = weights_for("weighted_self", rp, ci)
    cfg = hub_cfg("weighted_self", fault_model="byzantine", n_faulty=160, byz_strategy="split", byz_delta=0.1)
    env(**PATHS[path])
    with acsim.Simulator(cfg, csr=(rp, ci), weights=w) as g:
        assert g.kernel_name() == kname("weighted_self", path, False, sched=False)
        g.run()
        got, status = read_all(g), g.fault_status()
    n = reference(("byz",), cfg, (rp, ci), w, None)
    byz = n.status[0] == S.BYZ
    assert byz.sum() == 160 and np.array_equal(status.astype(np.uint64), n.status)
    assert byz[hub_rows(rp)].any() and not byz[hub_rows(rp)].all()   # a Byzantine hub row, and an honest one
    assert byz[ci[hub_slots(rp)]].any()                              # a Byzantine sender of a hub row
    assert_same(got, n)


EPS_CASES = {
    "pushsum_hold": dict(eps=1e-9, max_rounds=200),
    "weighted_self": dict(eps=1e-9, max_rounds=200, loss_p=0.1),
}


def eps_inputs(pair):
    rp, ci = heard()
    if pair == "pushsum_hold":
        return (rp, ci), G.pushsum_weights(rp, ci), G.phase_schedule(rp, ci, 4, seed=2)
    return (rp, ci), positive_weights(rp, 23), None


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("pair", list(EPS_CASES))
def test_gpu_eps_runs_stop_in_different_rounds(env, pair, path):
    """EPS termination on heard_hub_graph (every row hears someone), two instances: push-sum HOLD with
    loss_p = 0.2 on a one-phase-of-four schedule, and weighted SELF with weights in [0.25, 1)."""
    csr, w, sch = eps_inputs(pair)
    cfg = hub_cfg(pair, termination="eps", n_instances=2, **EPS_CASES[pair])
    env(**PATHS[path])
    _, n = check(("eps", pair), cfg, csr, w, sch, pair, path)
    assert n.converged.all() and n.rounds[0] != n.rounds[1] and 10 < n.rounds.min() and n.rounds.max() < cfg.max_rounds


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("pair", list(PAIRS))
def test_gpu_stepped_rounds_equal_one_run(env, pair, path):
    rp, ci = graph()
    w = weights_for(pair, rp, ci)
    cfg, sch = hub_cfg(pair), masks(ci.size)
    env(**PATHS[path])
    sname, stepped = run_handle(cfg, (rp, ci), w, sch, steps=(1, 7, 4))
    oname, once = run_handle(cfg, (rp, ci), w, sch)
    assert sname == oname == kname(pair, path, False)
    assert_same_handles(stepped, once)
    assert_same(once, reference(("grid", pair, True, "f64"), cfg, (rp, ci), w, sch))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_hold_resume_with_links_and_mass(env, dtype, path):
    """A HOLD handle read at round 5 (pairs and links) and restored into a fresh handle continues bit
    for bit.  Weights 1 / (outdeg + 1): the z mass Z* = sum z + sum k stays within
        N c^R (1 - u)^(15 R) <= Z* <= N (1 + u)^(15 R),
    the bound of test_pushsum_hold.py's test_gpu_f32_mass_survives_200_lossy_rounds for rows of at
    most 8192 entries (a product, the link add and up to 13 tree levels round every entry at most 15
    times): c = 1 - 2^-22 bounds the column sums of binary32 weights from below, c = 1 - 3 * 2^-53
    those of binary64 weights (test_pushsum.py, step (2) of the mean property).  Nothing is subnormal
    (checked: every weight is at least 2^-16 and the smallest positive z or k stays above 2^-100, so
    every product stays above 2^-116; a row without senders multiplies its z by w_self every round)."""
    rp, ci = graph()
    w = G.pushsum_weights(rp, ci, dtype=dtype)
    cfg, sch, r0 = hub_cfg("pushsum_hold", dtype), masks(ci.size), 5
    env(**PATHS[path])
    with acsim.Simulator(cfg, csr=(rp, ci), weights=w, schedule=sch) as g:
        assert g.kernel_name() == kname("pushsum_hold", path, dtype == "f32")
        g.round(r0)
        at, mass_at = read_all(g), g.pushsum_mass(0)
    with acsim.Simulator(cfg, csr=(rp, ci), weights=w, schedule=sch) as g:
        g.set_pushsum_state(r0, at["s"], at["z"])
        g.set_pushsum_links(at["h"], at["k"])   # (after it: set_pushsum_state empties the links)
        g.run()
        resumed = read_all(g)
    with acsim.Simulator(cfg, csr=(rp, ci), weights=w, schedule=sch) as g:
        g.run()
        straight, mass = read_all(g), g.pushsum_mass(0)
    n = reference(("resume", dtype), cfg, (rp, ci), w, sch)
    assert_same(straight, n)
    hub_links_hold_mass(n, rp)
    assert np.count_nonzero(at["k"][0][hub_slots(rp)]) > 1000   # the links restored hold mass
    assert np.array_equal(resumed["rounds"], straight["rounds"]) and np.array_equal(resumed["conv"], straight["conv"])
    for key in ("s", "z", "h", "k"):
        assert np.array_equal(bits(resumed[key]), bits(straight[key])), key
    live = straight["z"] > 0   # (x is recomputed from the pairs at the resume: the same wherever z > 0)
    assert live.all() and np.array_equal(bits(resumed["x"]), bits(straight["x"]))
    assert np.array_equal(bits(resumed["trace"][0][r0:]), bits(straight["trace"][0][r0:]))
    u, c = (2.0 ** -24, 1 - 2.0 ** -22) if dtype == "f32" else (2.0 ** -53, 1 - 3 * 2.0 ** -53)
    assert min(w[0].min(), w[1].min()) >= 2.0 ** -16
    assert min(float(n.z[0].min()), float(n.k[0][n.k[0] > 0].min())) > 2.0 ** -100
    for R, (_, mz) in ((r0, mass_at), (ROUNDS, mass)):
        lo, hi = N * c ** R * (1 - u) ** (15 * R), N * (1 + u) ** (15 * R)
        print(f"{dtype} z mass after {R} rounds: {mz!r} in [{lo!r}, {hi!r}]")
        assert lo <= mz <= hi
    assert mass == n.mass(0)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["weighted_self", "pushsum_hold"])
def test_gpu_admission_boundary(env, pair):
    """256 rows: with 64 hub rows (exactly N / 4) the lane kernel serves the other rows, with 65 the
    handle is all-generic on its own, no environment switch; both match the restatement."""
    env(ACSIM_CSR_FAST=None)
    for n_hubs, path in ((64, "fast"), (65, "generic")):
        rp, ci = admission_graph(n_hubs)
        w = weights_for(pair, rp, ci)
        cfg = hub_cfg(pair, n_nodes=256)
        check(("admission", pair, n_hubs), cfg, (rp, ci), w, masks(ci.size), pair, path)


EXACT = {"weighted_self": "weighted", "pushsum_omit": "pushsum OMIT", "pushsum_hold": "pushsum HOLD"}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("pair", list(EXACT))
def test_gpu_one_round_against_exact_arithmetic(env, pair, dtype, path):
    """A lossless handle under a period-5 schedule: 3 rounds, the state read, 1 round, and that round
    of every row (1 to 8192 entries) recomputed in Fractions from the state read.  The handle's x, s,
    z and links lie within hub_graphs.check_exact_round's operation-count bound (stated there):
    the plain high-precision reference for the kernels themselves, independent of the numpy code."""
    rp, ci = graph()
    w = weights_for(pair, rp, ci)
    cfg, sch = hub_cfg(pair, dtype, loss_p=0.0), masks(ci.size)
    env(**PATHS[path])
    with acsim.Simulator(cfg, csr=(rp, ci), weights=w, schedule=sch) as g:
        assert g.kernel_name() == kname(pair, path, dtype == "f32")
        g.round(3)
        before = handle_state(read_all(g))
        g.round(1)
        after = handle_state(read_all(g))
        assert g.rounds()[0] == 4
    if pair == "pushsum_hold":
        assert np.count_nonzero(before["k"][hub_slots(rp)]) > 1000   # from links that hold mass
    worst = check_exact_round(cfg.rule, cfg.missing_policy, (rp, ci), w, sch, 3, before, after, dtype)
    print(f"{pair} {dtype} {path}: worst error / bound {worst}")
