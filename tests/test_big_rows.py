"""The references of the big-m path's GPU tests, checked on the CPU: tests/big_rows.py's two graphs
reach every merge-pass count, buffer parity and tail-chunk width of k_big_sort (check_big_m), the C
oracle and the numpy restatement agree bit for bit on every case that tests/test_gpu_big_rows.py
runs, and one round of the restatement lies within check_exact_big_round's operation-count bound of
an exact recomputation in fractions.Fraction.
"""
import numpy as np
import pytest

import big_rows as R
import spec_np as S
from test_link_schedule import cached


def graph(name):
    return cached(("big_rows", name), getattr(R, name))


def test_big_m_reaches_every_pass_count_parity_and_tail_width():
    got = R.check_big_m(R.BIG_M)
    assert {v[1] for v in got.values()} == {1, 2, 3, 4, 5} and {v[2] for v in got.values()} == set(R.TAIL_P)
    assert got[8193] == (2, 1, 256) and got[16384] == (2, 1, 8192) and got[16385] == (3, 2, 256)
    assert got[65537] == (9, 4, 256) and got[100003] == (13, 4, 2048) and got[131073] == (17, 5, 256)
    assert R.first_buffer(8193) == "ent" and R.first_buffer(16385) == "srt" and R.first_buffer(131073) == "ent"
    assert R.lone_tails(16385) == [(8192, 1)] and R.lone_tails(40961) == [(16384, 8193)]
    assert R.lone_tails(100003) == [(8192, 1699), (16384, 1699)] and R.lone_tails(24576) == [(8192, 8192)]
    # a list that loses a class fails: without 16385 no three-run pass with a tail of one, without the
    # 8192 + 257 row no 512-wide tail at its low end, without 65536 no high end of three passes
    for gone in (16385, 8192 + 257, 65536, 100003, 8193):
        with pytest.raises(AssertionError):
            R.check_big_m([m for m in R.BIG_M if m != gone])


def test_both_graphs_hold_every_size():
    rp, ci = graph("pass_graph")
    assert R.check_pass_graph(rp, ci) == R.check_big_m(R.BIG_M)
    assert 880_000 < ci.size < 960_000
    ap, ac = graph("all_big_graph")
    got = R.check_all_big_graph(ap, ac)
    assert set(R.check_big_m(R.BIG_M)) <= set(got) and len(got) == R.N_ALL_BIG
    for i in range(R.N_ALL_BIG):   # at most 48 distinct senders in rows of 8192 and more: ties dominate
        assert np.unique(ac[int(ap[i]):int(ap[i + 1])]).size <= R.N_ALL_BIG
    again, other = R.pass_graph(), R.pass_graph(1)   # a function of its seed
    assert np.array_equal(again[0], rp) and np.array_equal(again[1], ci) and not np.array_equal(other[0], rp)


def oracle_run(oracle_mod, cfg, csr):
    with oracle_mod.OracleSimulator(cfg, threads=8, csr=csr) as o:
        o.run()
        return dict(x=o.all_values(), rounds=o.rounds(), spread=o.spread(), status=o.fault_status(),
                    trace=[o.spread_trace(b) for b in range(o.B)])


def assert_oracle_is_restatement(oracle_mod, graph_name, kw):
    csr = graph(graph_name)
    cfg = R.case_cfg(graph_name, kw)
    o = oracle_run(oracle_mod, cfg, csr)
    n = S.NpSim(cfg, csr=csr)
    n.run()
    view = np.uint32 if cfg.dtype == "f32" else np.uint64
    assert np.array_equal(o["rounds"], n.rounds) and int(n.rounds.min()) == cfg.max_rounds
    assert np.array_equal(o["status"].astype(np.uint64), n.status)
    assert np.array_equal(np.ascontiguousarray(o["x"]).view(view), n.x.view(view))
    for b in range(n.B):
        assert np.array_equal(o["trace"][b], np.array(n.trace[b]))
    return n


@pytest.mark.parametrize("name", list(R.PASS_CASES))
def test_oracle_matches_numpy_on_pass_graph(oracle_mod, name):
    assert_oracle_is_restatement(oracle_mod, "pass_graph", R.PASS_CASES[name])


@pytest.mark.parametrize("name", list(R.ALL_BIG_CASES))
def test_oracle_matches_numpy_on_all_big_graph(oracle_mod, name):
    n = assert_oracle_is_restatement(oracle_mod, "all_big_graph", R.ALL_BIG_CASES[name])
    if name == "trimmed_t3000_omit":   # rows that fall to m' <= 2 t keep x_i in round 1, others move
        kept = n.hist[0][1] == n.hist[0][0]
        assert kept.any() and not kept.all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("graph_name", ["pass_graph", "all_big_graph"])
@pytest.mark.parametrize("rule", list(R.EXACT_RULES))
def test_restatement_round_against_exact_arithmetic(rule, graph_name, dtype):
    """Round 1 of the restatement, every big row of both graphs recomputed in Fractions from x^0
    (trims 1 on pass_graph; 3000, 4096, 37 and 2000 on all_big_graph): within check_exact_big_round's
    bound ((1 + u)^(L + 1) - 1) sum |v| / cnt, L = ceil(log2 cnt); midpoint u |v_lo + v_hi| / 2.
    Worst error / bound observed, f64 / f32 (information, not the threshold):
                   pass_graph     all_big_graph
        average    0.12 / 0.11    0.14 / 0.12
        trimmed    0.11 / 0.08    0.18 / 0.10
        midpoint   1.00 / 1.00    1.00 / 1.00
        dlpsw      0.11 / 0.08    0.15 / 0.11
        wmsr       0.11 / 0.08    0.11 / 0.09
    (midpoint's bound is attained: x^0 values are multiples of 2^-53, so a sum in [1, 2) that is an
    odd multiple of 2^-53 is a tie of the one rounded add, an error of exactly u.)
    """
    csr = graph(graph_name)
    cfg = R.case_cfg(graph_name, R.exact_kw(rule, graph_name), dtype=dtype, max_rounds=1)
    n = S.NpSim(cfg, csr=csr)
    before = n.x[0].copy()
    n.round(1)
    assert int(n.rounds[0]) == 1
    worst = R.check_exact_big_round(cfg, csr, before, n.x[0])
    print(f"{rule} {graph_name} {dtype}: worst error / bound {worst:.2f}")


def test_exact_check_rejects_a_misplaced_entry():
    """The check is not vacuous: the trimmed window of the widest row shifted by one entry (what a
    merge that loses an element's place does) is far outside the bound."""
    csr = graph("pass_graph")
    cfg = R.case_cfg("pass_graph", R.exact_kw("trimmed", "pass_graph"), max_rounds=1)
    n = S.NpSim(cfg, csr=csr)
    before = n.x[0].copy()
    n.round(1)
    after = n.x[0].copy()
    rp, ci = csr
    i = int(np.argmax(np.diff(rp.astype(np.int64))))
    s = np.sort(np.concatenate([[before[i]], before[ci[int(rp[i]):int(rp[i + 1])]]]))
    t = int(cfg.trim)
    after[i] = S.tree_sum_rows(s[t + 1:s.size - t + 1][None, :])[0] / (s.size - 2 * t)
    with pytest.raises(AssertionError):
        R.check_exact_big_round(cfg, csr, before, after)
