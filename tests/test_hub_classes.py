"""The restatements of rules "weighted" and "pushsum" at hub-row sizes (CPU): tests/hub_graphs.py's
graph reaches every size class of k_round_generic, and one round of each restatement on it is held
against an exact recomputation in fractions.Fraction (hub_graphs.check_exact_round, which states the
bound).  The restatements are the only reference the GPU tests of these rules have
(tests/test_gpu_hub_classes.py); nothing else checks them at rows of thousands of entries.
"""
import numpy as np
import pytest

import spec_np as S
from acsim.config import Config
from hub_graphs import (CLASSES, HUB_DEGREES, N_HUB_GRAPH, admission_graph, check_exact_round, check_hub_class_graph,
                        heard_hub_graph, hub_class_graph, hub_rows, hub_slots, sim_state, slice_widths)
from spec_sched_np import plain_sim, sched_sim
from test_link_schedule import PAIRS, random_masks, weights_for
from test_pushsum import bits


def test_hub_class_graph_reaches_every_class_and_block_size():
    rp, ci = hub_class_graph()
    assert check_hub_class_graph(rp, ci) == {64: 64, 256: 64, 1024: 256, 4096: 1024, 8192: 1024}
    deg = np.diff(rp.astype(np.int64))
    assert rp.size - 1 == N_HUB_GRAPH and hub_rows(rp).size == len(HUB_DEGREES)
    assert sorted(deg[hub_rows(rp)].tolist()) == sorted(HUB_DEGREES)
    assert int(deg.max()) + 1 == CLASSES[-1]
    w = slice_widths(rp)
    assert w[0] == 0 and w[1] == 3 and w[2:-1] == [8] * 8 and w[-1] == 5 and len(w) == 11
    assert 40000 < ci.size < 46000 and hub_slots(rp).sum() == sum(HUB_DEGREES)
    again, other = hub_class_graph(), hub_class_graph(1)   # a function of its seed
    assert np.array_equal(again[0], rp) and np.array_equal(again[1], ci)
    assert not np.array_equal(other[1][:100], ci[:100])
    hp, hc = heard_hub_graph()
    hdeg = np.diff(hp.astype(np.int64))
    assert hdeg.min() == 1 and np.array_equal(hdeg[deg > 0], deg[deg > 0]) and np.all(hdeg[deg == 0] == 1)
    assert np.array_equal(hc[hub_slots(hp)], ci[hub_slots(rp)])
    for extra in (0, 1):
        ap, _ = admission_graph(64 + extra)
        assert (hub_rows(ap).size * 4 <= ap.size - 1) == (extra == 0)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ragged_tree_sums_are_the_padded_ones(dtype):
    """spec_np.RaggedTreeSum against tree_sum_rows on every row padded to the widest, bit for bit."""
    ft = np.float32 if dtype == "f32" else np.float64
    rp, _ = hub_class_graph()
    deg = np.diff(rp.astype(np.int64))
    rng = np.random.default_rng(5)
    rows = np.repeat(np.arange(deg.size), deg + 1)
    pos = np.arange(rows.size) - np.repeat(np.concatenate([[0], np.cumsum(deg + 1)[:-1]]), deg + 1)
    vals = rng.random(rows.size).astype(ft)
    vals[rng.random(rows.size) < 0.1] = 0
    wide = np.zeros((deg.size, int(deg.max()) + 1), dtype=ft)
    wide[rows, pos] = vals
    got = S.RaggedTreeSum(deg + 1)(rows, pos, vals)
    assert got.dtype == ft and np.array_equal(bits(got), bits(S.tree_sum_rows(wide)))
    some = rows % 3 != 0   # rows with no entry given sum to +0.0
    wide[rows[~some], pos[~some]] = 0
    assert np.array_equal(bits(S.RaggedTreeSum(deg + 1)(rows[some], pos[some], vals[some])), bits(S.tree_sum_rows(wide)))


EXACT_PAIRS = ["weighted_self", "pushsum_omit", "pushsum_hold"]


def exact_case(pair, sched, dtype):
    """-> (cfg, csr, weights, schedule, restatement at round 3): lossless, from state that a run leaves.
    HOLD without a schedule never fills a link in a lossless run, so its state at round 3, links
    included, comes from a run with loss_p = 0.2 and is set into the lossless restatement."""
    rp, ci = hub_class_graph()
    w = weights_for(pair, rp, ci)
    sch = random_masks(ci.size, 5, 13) if sched else None
    cfg = Config(n_nodes=N_HUB_GRAPH, topology="csr", termination="fixed", max_rounds=8, seed=71, dtype=dtype, **PAIRS[pair])
    make = (lambda c: sched_sim(c, (rp, ci), w, sch)) if sched else (lambda c: plain_sim(c, (rp, ci), w))
    n = make(cfg)
    if pair == "pushsum_hold" and not sched:
        lossy = make(cfg.replace(loss_p=0.2))
        lossy.round(3)
        n.restart(3, lossy.s, lossy.z)
        n.set_links(lossy.h[:, lossy.N:], lossy.k[:, lossy.N:])
    else:
        n.round(3)
    return cfg, (rp, ci), w, sch, n


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("sched", [False, True], ids=["plain", "sched5"])
@pytest.mark.parametrize("pair", EXACT_PAIRS)
def test_round_4_of_the_restatement_against_exact_arithmetic(pair, sched, dtype):
    """From the restatement's state at round 3, round 4 of every row of hub_class_graph (rows of 1 to
    8192 entries) recomputed in Fractions; the restatement's x (and s, z, and under HOLD the links)
    lie within hub_graphs.check_exact_round's bound: (2 L + 3) u for weighted, (L + 2) u for s' and z'
    (+ u under HOLD) and their sum + u for s' / z', 2 u + u^2 for a link, L = log2 of the row's power
    of two.  Worst error / bound observed, f64 / f32 (information, not the threshold):
        weighted_self   plain   x 0.40 / 0.43
                        sched5  x 0.26 / 0.30
        pushsum_omit    plain   s 0.48 / 0.47   z 0.58 / 0.54   x 0.38 / 0.36
                        sched5  s 0.48 / 0.47   z 0.48 / 0.47   x 0.38 / 0.35
        pushsum_hold    plain   s 0.32 / 0.47   z 0.32 / 0.43   x 0.27 / 0.27
                        sched5  s 0.40 / 0.31   z 0.32 / 0.38   x 0.27 / 0.26   h 0.76 / 0.81   k 0.79 / 0.83
    """
    cfg, csr, w, sch, n = exact_case(pair, sched, dtype)
    assert int(n.rounds[0]) == 3
    before = sim_state(n)
    assert before["x"].min() >= 0
    if pair == "pushsum_hold":
        held = before["k"] > 0
        assert held[hub_slots(csr[0])].sum() > 1000 and held[~hub_slots(csr[0])].sum() > 1000   # links hold mass
    n.round(1)
    after = sim_state(n)
    assert int(n.rounds[0]) == 4 and not np.array_equal(bits(before["x"]), bits(after["x"]))
    worst = check_exact_round(cfg.rule, cfg.missing_policy, csr, w, sch, 3, before, after, dtype)
    print(f"{pair} {'sched5' if sched else 'plain'} {dtype}: worst error / bound {worst}")
    # (lossless and unscheduled, every message arrives and every link ends +0.0: checked as exact zeros)
    links = {"h", "k"} if pair == "pushsum_hold" and sched else set()
    assert set(worst) == {"weighted": {"x"}, "pushsum": {"x", "s", "z"}}[cfg.rule] | links


def test_exact_check_rejects_a_dropped_entry():
    """The check is not vacuous: entry 1 of the widest row left out of the sums is far outside the bound."""
    cfg, csr, w, sch, n = exact_case("pushsum_omit", False, "f64")
    before = sim_state(n)
    n.round(1)
    after = sim_state(n)
    i = int(np.argmax(np.diff(csr[0].astype(np.int64))))
    e = int(csr[0][i])
    assert w[1][e] > 0
    after["s"][i] -= w[1][e] * before["s"][csr[1][e]]
    with pytest.raises(AssertionError):
        check_exact_round("pushsum", "omit", csr, w, sch, 3, before, after, "f64")
