"""Property-based tests of rules "weighted" and "pushsum" on CSR graphs, in the style and settings of
test_properties.py (hypothesis, derandomized, no database; the failing draw is printed).

One strategy draws a graph (every lane width D = 4, 8, 16, 32; beside D = 32 hub rows of every size
class of k_round_generic, or so many that the handle goes all-generic on its own), one of the four
rule / policy pairs, and the config fields these rules read: dtype, loss, a link schedule, instances,
mask group and offset, termination, and for rule "weighted" delays and fault models.

  GPU  the handle against the numpy restatement, bit for bit: x, rounds, converged flags, spread
       trace, fault status, the (s, z) pairs and the (h, k) links;
  CPU  one round of the restatement on lossless, fault-free draws against exact rational arithmetic
       (hub_graphs.check_exact_round, which states the bound).
"""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from acsim import graphs as G
from acsim.config import Config
from hub_graphs import FAST_D, check_exact_round, positive_weights, sim_state
from spec_sched_np import plain_sim, sched_sim
from test_link_schedule import PAIRS, assert_same, kname, random_masks, read_all
from test_pushsum import random_ps_weights
from test_weighted import random_weights

# hub sender counts spanning every size class (m = deg + 1 in (32, 64], .. (4096, 8192]); the small
# classes more often, the 8192-entry row occasionally
HUB_DEGREES = [33, 40, 63, 64, 100, 255, 256, 700, 1023, 1024, 2500, 4095, 4096, 6000, 8191]
HUB_WEIGHTS = [12, 12, 12, 8, 8, 8, 6, 6, 6, 4, 3, 3, 2, 1, 1]


class Case:
    """One draw: the recipe (printed when a draw fails) and what it builds."""

    def __init__(self, cfg, pair, dmin, base, hubs, gseed, period, wkind):
        self.cfg, self.pair = cfg, pair
        self.recipe = dict(dmin=dmin, base=base, hubs=hubs, gseed=gseed, period=period, wkind=wkind)
        n = int(cfg.n_nodes)
        rng = np.random.default_rng(gseed)
        deg = rng.integers(dmin, base + 1, n)
        deg[0] = base   # the lane width is the smallest compiled one >= base
        if hubs:
            deg[rng.permutation(n)[:len(hubs)]] = hubs
        rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
        ci = rng.integers(0, n, int(rp[-1])).astype(np.uint32)
        self.csr, self.deg = (rp, ci), deg
        if cfg.rule == "weighted":
            self.w = random_weights(rp, gseed % 1000) if wkind == "zeros" else positive_weights(rp, gseed % 1000)
        else:
            self.w = G.pushsum_weights(rp, ci, dtype=cfg.dtype)
            if wkind == "zeros":
                try:
                    self.w = random_ps_weights(rp, ci, gseed % 1000)
                except AssertionError:   # a graph too small to draw an exact zero on: keep 1 / (outdeg + 1)
                    pass
        self.sch = random_masks(ci.size, period, gseed % 1000 + 1) if period and ci.size >= 2 else None

    def __repr__(self):
        return f"Case({self.cfg!r}, pair={self.pair!r}, {self.recipe!r})"

    def restatement(self, cfg=None):
        cfg = cfg or self.cfg
        return plain_sim(cfg, self.csr, self.w) if self.sch is None else sched_sim(cfg, self.csr, self.w, self.sch)

    def kernel_name(self):
        n_hub = int((self.deg > FAST_D).sum())
        path = "fast" if n_hub * 4 <= self.deg.size else "generic"
        d = next(d for d in (4, 8, 16, 32) if d >= min(int(self.deg.max()), FAST_D))
        return kname(self.pair, path, self.cfg.dtype == "f32", d, hubs=n_hub > 0, sched=self.sch is not None)


@st.composite
def csr_rule_cases(draw, lossless=False):
    n = draw(st.integers(64, 400))
    base = draw(st.sampled_from([3, 7, 15, 32, 32, 32]))
    gseed = draw(st.integers(0, 2 ** 32))
    dmin = draw(st.sampled_from([0, 1]))   # 1: every row hears someone, so an EPS run can stop early
    hubs = []
    if base == 32:
        rng = np.random.default_rng(gseed + 1)
        if draw(st.sampled_from(["classes", "classes", "classes", "many"])) == "many":
            # more than n // 4 hub rows: the handle goes all-generic on its own
            hubs = rng.integers(33, 41, n // 4 + draw(st.integers(1, 8))).tolist()
        else:
            p = np.array(HUB_WEIGHTS, dtype=np.float64)
            hubs = rng.choice(HUB_DEGREES, size=draw(st.integers(0, min(n // 4, 24))), p=p / p.sum()).tolist()
    pair = draw(st.sampled_from(list(PAIRS)))
    kw = {}
    if PAIRS[pair]["rule"] == "weighted" and not lossless:
        kw["delay_max"] = draw(st.sampled_from([0, 0, 1, 3]))
        fault = draw(st.sampled_from(["none", "none", "crash", "byzantine"]))
        if fault != "none":
            kw.update(fault_model=fault, n_faulty=draw(st.integers(1, n // 4)))
        if fault == "crash":
            kw["crash_window"] = draw(st.integers(1, 6))
        if fault == "byzantine":
            kw["byz_strategy"] = draw(st.sampled_from(["split", "random", "constant"]))
            kw["byz_delta"] = draw(st.sampled_from([0.0, 0.05, 0.5]))
            kw["byz_const"] = draw(st.sampled_from([0.0, -2.0, 7.5]))
    cfg = Config(n_nodes=n, topology="csr", n_instances=draw(st.integers(1, 3)), dtype=draw(st.sampled_from(["f64", "f64", "f32"])),
                 loss_p=0.0 if lossless else draw(st.sampled_from([0.0, 0.1, 0.35])),
                 mask_group=draw(st.sampled_from([1, 2])), instance_offset=draw(st.sampled_from([0, 1000])),
                 termination=draw(st.sampled_from(["eps", "fixed"])), eps=draw(st.sampled_from([0.5, 0.1, 1e-7])),
                 max_rounds=draw(st.integers(1, 12)), seed=draw(st.integers(0, 2 ** 40)), trace_spread=True,
                 **PAIRS[pair], **kw)
    period = draw(st.sampled_from([0, 0, 1, 2, 5, 32]))
    return Case(cfg, pair, dmin, base, hubs, gseed, period, draw(st.sampled_from(["zeros", "plain"])))


SETTINGS = settings(deadline=None, derandomize=True, database=None,
                    suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])


@settings(SETTINGS, max_examples=15)
@given(case=csr_rule_cases(lossless=True))
def test_restatement_round_matches_exact_arithmetic_random_cases(case):
    """Instance 0 of a lossless, fault-free draw: the round after the third (or after the last but
    one, on shorter runs) of the restatement within check_exact_round's operation-count bound."""
    r = min(3, int(case.cfg.max_rounds) - 1)
    n = case.restatement(case.cfg.replace(termination="fixed", max_rounds=r + 1, n_instances=1))
    n.round(r)
    before = sim_state(n)
    n.round(1)
    assert int(n.rounds[0]) == r + 1
    check_exact_round(case.cfg.rule, case.cfg.missing_policy, case.csr, case.w, case.sch, r, before, sim_state(n),
                      case.cfg.dtype)


@pytest.mark.gpu
@settings(SETTINGS, max_examples=40)
@given(case=csr_rule_cases())
def test_gpu_csr_rules_match_restatement_random_cases(case):
    import acsim
    with acsim.Simulator(case.cfg, device=0, csr=case.csr, weights=case.w, schedule=case.sch) as g:
        name = g.kernel_name()
        g.run()
        got, status = read_all(g), g.fault_status()
    assert name == case.kernel_name(), (case, name)
    n = case.restatement()
    n.run()
    assert np.array_equal(status.astype(np.uint64), n.status), case
    assert_same(got, n)
