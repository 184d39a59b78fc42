"""The big-m path (k_big_resolve, k_big_sort, k_big_rule: rows above 8192 entries) at every merge-pass
count, buffer parity, partnerless tail run and tail-chunk width of k_big_sort (GPU).

tests/big_rows.py's pass_graph has one row of every size in BIG_M (8193 .. 131073 entries: one to
five merge passes, both starting buffers, every padded width of the last chunk at both ends, odd run
counts with full, short and one-entry last runs, sizes that are no multiple of the 8-output merge
step) among 3000 rows of 3 .. 6 senders, so the big rows run beside the lane (or binned) kernel and
k_round_generic in one round; all_big_graph has the same sizes and 20 larger rows on 48 nodes, so
every merge is dominated by ties and trims in the thousands are admitted (the stride-t sums of
DLPSW, W-MSR's binary searches among equal values, OMIT rows that fall to m' <= 2 t).

Every case compares values, fault status, rounds, spread and the spread trace with the C oracle bit
for bit (tests/test_big_rows.py pins the oracle to the numpy restatement on the same cases), and the
last test holds one round of the handle against exact rational arithmetic
(big_rows.check_exact_big_round).

The kernel name: a handle whose every row is on the generic kernels names the big-m kernels
("k_round_generic+k_big_resolve+sort+k_big_rule"); a handle with a fast path beside its hub rows
says "+k_round_generic(hubs)" for all of them (the names are pinned by tests/golden/kernel_names.json),
and there the rows above 8192 entries, which k_round_generic leaves at once, are served by no other
kernel than the big-m ones.
"""
import numpy as np
import pytest

import acsim
import big_rows as R
from test_link_schedule import cached, env  # noqa: F401
from test_pushsum import bits

PATHS = {"fast": dict(ACSIM_CSR_FAST=None), "generic": dict(ACSIM_CSR_FAST=0)}


def graph(name):
    return cached(("big_rows", name), getattr(R, name))


def assert_big_path(name, path, cfg):
    hubs = "+k_round_generic(hubs)" + (" [f32]" if cfg.dtype == "f32" else "")
    if path == "generic":
        assert "k_big_resolve" in name and name.startswith("k_round_generic"), name
    else:
        assert "k_big_resolve" in name or name.endswith(hubs), name


def read(s):
    return dict(x=s.all_values(), rounds=s.rounds(), spread=s.spread(), conv=s.converged(), status=s.fault_status(),
                trace=[s.spread_trace(b) for b in range(s.B)])


def oracle_run(oracle_mod, cfg, csr, state=None):
    with oracle_mod.OracleSimulator(cfg, threads=8, csr=csr) as o:
        if state is not None:
            o.set_state(*state)
        o.run()
        return read(o)


def reference(oracle_mod, graph_name, key, cfg):
    """The oracle's whole run, computed once per case and left unchanged."""
    return cached(("big_rows", "oracle", graph_name, key), lambda: oracle_run(oracle_mod, cfg, graph(graph_name)))


def gpu_run(cfg, csr, steps=None):
    with acsim.Simulator(cfg, device=0, csr=csr) as g:
        name = g.kernel_name()
        if steps is None:
            g.run()
        else:
            for k in steps:
                g.round(k)
        return name, read(g)


def assert_same(got, want):
    assert np.array_equal(got["rounds"], want["rounds"])
    assert np.array_equal(got["conv"], want["conv"])
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(bits(got["x"]), bits(want["x"])), np.nonzero(bits(got["x"]) != bits(want["x"]))
    assert np.array_equal(bits(got["spread"]), bits(want["spread"]))
    assert len(got["trace"]) == len(want["trace"])
    for a, b in zip(got["trace"], want["trace"]):
        assert np.array_equal(bits(a), bits(b))


def check(oracle_mod, graph_name, key, cfg, path):
    name, got = gpu_run(cfg, graph(graph_name))
    assert_big_path(name, path, cfg)
    want = reference(oracle_mod, graph_name, key, cfg)
    assert int(want["rounds"].min()) == cfg.max_rounds
    assert_same(got, want)
    return got


# ----------------------------------------------------------------------------- pass_graph
@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", list(R.PASS_CASES))
def test_gpu_pass_graph_matches_oracle(oracle_mod, env, case, path):
    """3000 rows, big rows of every size in BIG_M beside rows of 3 .. 6 senders, t <= 1, 3 FIXED
    rounds (4 with delays): every rule clean and with loss_p = 0.2, OMIT, crash faults, Byzantine
    RANDOM and CONSTANT senders (hundreds of equal entries in every big row), fp32, delays of up to 2
    rounds, three instances at instance_offset 5; beside the fast path and with ACSIM_CSR_FAST=0."""
    cfg = R.case_cfg("pass_graph", R.PASS_CASES[case])
    env(**PATHS[path])
    got = check(oracle_mod, "pass_graph", case, cfg, path)
    big = R.big_rows(graph("pass_graph")[0])
    if cfg.fault_model == "byzantine":
        rp, ci = graph("pass_graph")
        byz = got["status"][0] == 0xFFFFFFFE
        for i in big.tolist():   # equal (CONSTANT) or out-of-hull (RANDOM) entries in every big row
            assert byz[ci[int(rp[i]):int(rp[i + 1])]].sum() >= 100
    if cfg.fault_model == "crash":
        st = got["status"][0][big]
        assert 0 < np.count_nonzero(st != 0xFFFFFFFF) < st.size   # big rows that crash and big rows that do not
    if cfg.n_instances > 1:
        assert not np.array_equal(bits(got["x"][0]), bits(got["x"][1]))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_pass_graph_eps_run(oracle_mod, env, path):
    """EPS termination, trimmed t = 1, eps = 1e-9: the big rows' partials (slots pbase + k behind the
    fast path's and the size classes') enter every round's spread, so rounds and the whole spread
    trace equal the oracle's."""
    cfg = R.case_cfg("pass_graph", dict(rule="trimmed", trim=1), termination="eps", eps=1e-9, max_rounds=300)
    env(**PATHS[path])
    name, got = gpu_run(cfg, graph("pass_graph"))
    assert_big_path(name, path, cfg)
    want = cached(("big_rows", "oracle", "eps"), lambda: oracle_run(oracle_mod, cfg, graph("pass_graph")))
    assert want["conv"].all() and 10 < int(want["rounds"][0]) < cfg.max_rounds
    assert_same(got, want)


STEP_CASES = {"pass_graph": "trimmed_loss", "all_big_graph": "dlpsw_t37"}


@pytest.mark.gpu
@pytest.mark.parametrize("graph_name", list(STEP_CASES))
def test_gpu_stepping_and_resume(oracle_mod, env, graph_name):
    """round(1) three times equals run(); a fresh handle given the state read at round 2 continues as
    the unbroken run does."""
    case = STEP_CASES[graph_name]
    cfg = R.case_cfg(graph_name, getattr(R, "PASS_CASES" if graph_name == "pass_graph" else "ALL_BIG_CASES")[case])
    csr = graph(graph_name)
    env(ACSIM_CSR_FAST=None)
    want = reference(oracle_mod, graph_name, case, cfg)
    name, stepped = gpu_run(cfg, csr, steps=(1, 1, 1))
    assert_big_path(name, "fast" if graph_name == "pass_graph" else "generic", cfg)
    assert_same(stepped, want)
    with acsim.Simulator(cfg, device=0, csr=csr) as g:
        g.round(2)
        assert int(g.rounds()[0]) == 2
        at = g.all_values()
    with acsim.Simulator(cfg, device=0, csr=csr) as g:
        g.set_state(2, at)
        g.run()
        resumed = read(g)
    assert np.array_equal(resumed["rounds"], want["rounds"])
    assert np.array_equal(bits(resumed["x"]), bits(want["x"]))
    assert np.array_equal(bits(resumed["spread"]), bits(want["spread"]))
    assert np.array_equal(bits(resumed["trace"][0][2:]), bits(want["trace"][0][2:]))


# ----------------------------------------------------------------------------- all_big_graph
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(R.ALL_BIG_CASES))
def test_gpu_all_big_graph_matches_oracle(oracle_mod, env, case):
    """48 rows of 8193 .. 140 000 entries with at most 48 distinct values each, 3 FIXED rounds: trims
    of 3000 .. 4096 (trimmed, midpoint, DLPSW's stride-4000 sums, W-MSR among CONSTANT senders),
    DLPSW t = 37, average, fp32, and OMIT with loss_p = 0.6, where the smaller rows fall to
    m' <= 2 t and keep x_i."""
    cfg = R.case_cfg("all_big_graph", R.ALL_BIG_CASES[case])
    env(ACSIM_CSR_FAST=None)
    check(oracle_mod, "all_big_graph", case, cfg, "generic")
    if case == "trimmed_t3000_omit":
        one = cfg.replace(max_rounds=1)
        _, first = gpu_run(one, graph("all_big_graph"))
        with acsim.Simulator(one, device=0, csr=graph("all_big_graph")) as g:
            x0 = g.all_values()
        kept = bits(first["x"][0]) == bits(x0[0])
        assert kept.any() and not kept.all()   # rows that fall to m' <= 2 t keep x_i, the larger rows move


def big_caps():
    """ACSIM_BIG_CAP values: the largest row (small rows still pair up, every row above half of it is
    alone in its batch) and one that holds two or three of the larger rows, so that segments start
    at several offsets eoff[k] - eoff[k0]."""
    m = np.diff(graph("all_big_graph")[0].astype(np.int64)) + 1
    return dict(one=int(m.max()), few=3 * int(m.max()) - 5)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", ["one", "few"])
@pytest.mark.parametrize("case", ["trimmed_t4000", "dlpsw_t37", "wmsr_t2000_byz_constant", "trimmed_t3000_omit", "trimmed_f32"])
def test_gpu_all_big_graph_forced_batches(oracle_mod, env, case, cap):
    m = np.diff(graph("all_big_graph")[0].astype(np.int64)) + 1
    c = big_caps()[cap]
    eoff = np.concatenate([[0], np.cumsum(m)])
    sizes, k0 = [], 0
    while k0 < m.size:   # the batches generic_big_build forms: consecutive rows whose segments fit the cap
        k1 = k0 + 1
        while k1 < m.size and eoff[k1 + 1] - eoff[k0] <= c:
            k1 += 1
        sizes.append(k1 - k0)
        k0 = k1
    assert m.max() <= c < m.sum() and len(sizes) > 1
    assert (1 in sizes) if cap == "one" else (max(sizes) >= 3 and len(set(sizes)) > 1)
    cfg = R.case_cfg("all_big_graph", R.ALL_BIG_CASES[case])
    env(ACSIM_CSR_FAST=None, ACSIM_BIG_CAP=c)
    check(oracle_mod, "all_big_graph", case, cfg, "generic")


# ----------------------------------------------------------------------------- one exact round
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("graph_name", ["pass_graph", "all_big_graph"])
@pytest.mark.parametrize("rule", list(R.EXACT_RULES))
def test_gpu_one_round_against_exact_arithmetic(env, rule, graph_name, dtype):
    """A lossless, fault-free handle: 1 round, the state read, 1 round, and that round of every big
    row recomputed in Fractions from the state read (t = 1 on pass_graph; 3000, 4096, 37 and 2000 on
    all_big_graph).  The handle's values lie within big_rows.check_exact_big_round's operation-count
    bound (stated there): the plain high-precision reference for k_big_sort and k_big_rule
    themselves, independent of the oracle and the numpy code."""
    csr = graph(graph_name)
    cfg = R.case_cfg(graph_name, R.exact_kw(rule, graph_name), dtype=dtype, max_rounds=2)
    env(ACSIM_CSR_FAST=None)
    with acsim.Simulator(cfg, device=0, csr=csr) as g:
        assert_big_path(g.kernel_name(), "fast" if graph_name == "pass_graph" else "generic", cfg)
        g.round(1)
        before = g.values(0)
        g.round(1)
        after = g.values(0)
        assert int(g.rounds()[0]) == 2
    big = R.big_rows(csr[0])
    assert not np.array_equal(bits(before[big]), bits(after[big]))
    worst = R.check_exact_big_round(cfg, csr, before, after)
    print(f"{rule} {graph_name} {dtype}: worst error / bound {worst:.2f}")
