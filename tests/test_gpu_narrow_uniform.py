"""Uniform rounds of the narrow stage: once every node holds the same bit pattern,
the published (min, max) of x^r are equal, phase A streams nothing (width 0 in the header) and
phase B evaluates the rule on D + 1 copies of that value without a stage, an LDS image or invpos.
On a clean regular graph that state is absorbing, so a FIXED run past exact agreement spends its
remaining rounds there.

n = 4099 with ACSIM_BIN_SA=1024: 5 source blocks, 17 receiver blocks, the last one partial.  Bar:
bit-exact against the oracle (values, rounds, spread trace), and every case also checks that the
run really was uniform for several rounds: one bit pattern at the end and a trace whose last five
spreads are 0 (the EPS case ends at its first zero spread by definition, so there it is the last
one).  The round numbers in TABLE are the oracle's: round r is the first after which the values are
uniform, i.e. trace[r] == 0 < trace[r - 1] (round r + 1 is the first of width 0); they are asserted
on the oracle's trace.

The d = 16, t = 2 case has no binned kernel (binned_select.hpp compiles (16, 5) and (16, 0)), so it
runs on the per-lane kernel: it is here as the same property on a path without a stage.
"""
import contextlib
import os

import numpy as np
import pytest

import acsim
from acsim.config import Config

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, os.cpu_count() or 1))
KNOBS = ("ACSIM_BIN_NARROW", "ACSIM_BIN_SA", "ACSIM_BIN_SPLIT", "ACSIM_BIN_AWG")
N, SEED = 4099, 3


@contextlib.contextmanager
def env(**kw):
    """The binned knobs exactly as given: every knob not named is unset for the duration."""
    want = {k: None for k in KNOBS}
    want.update(kw)
    old = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
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
    return np.ascontiguousarray(a).view(np.uint64)


def regular(d, rule, trim, rounds, **kw):
    return Config(n_nodes=N, topology="regular", degree=d, rule=rule, trim=trim, termination="fixed",
                  max_rounds=rounds, seed=SEED, trace_spread=True, **kw)


# name -> (config, x^0 -> state set before the run or None, first round with uniform values)
TABLE = {
    "trimmed_t5_d32": (regular(32, "trimmed", 5, 48), None, 40),
    "average_d32": (regular(32, "average", 0, 44), None, 36),
    "trimmed_t2_d16": (regular(16, "trimmed", 2, 68), None, 60),
    "negative": (regular(32, "trimmed", 5, 45), lambda x0: -x0 - 3.0, 37),
    "across_zero": (regular(32, "trimmed", 5, 56), lambda x0: x0 - 0.5, 48),
    "tiny": (regular(32, "trimmed", 5, 46), lambda x0: 1e-300 * (x0 + 1.0), 38),
}
FIRST = TABLE["trimmed_t5_d32"][0]

_x0_cache = {}
_oracle_cache = {}


def x0_of(oracle_mod, cfg):
    """The default initial state of cfg's (n, seed): the oracle's values before any round."""
    key = (cfg.n_nodes, cfg.seed)
    if key not in _x0_cache:
        with oracle_mod.OracleSimulator(cfg, threads=THREADS) as o:
            _x0_cache[key] = o.values(0).copy()
    return _x0_cache[key]


def run_oracle(oracle_mod, cfg, state=None, tag=""):
    """(rounds, value bits, trace bits) of the oracle's run from `state` (or the default x^0),
    computed once per (config, tag)."""
    key = (repr(cfg), tag)
    if key not in _oracle_cache:
        with oracle_mod.OracleSimulator(cfg, threads=THREADS) as o:
            if state is not None:
                o.set_state(0, state[None, :])
            o.run()
            _oracle_cache[key] = (o.rounds().copy(), bits(o.values(0)).copy(), bits(o.spread_trace(0)).copy())
    return _oracle_cache[key]


def run_gpu(cfg, state=None, **kw):
    with env(**kw):
        with acsim.Simulator(cfg, device=0) as g:
            name = g.kernel_name()
            if state is not None:
                g.set_state(0, state[None, :])
            g.run()
            return name, g.rounds(), bits(g.values(0)).copy(), bits(g.spread_trace(0)).copy()


def assert_matches(got, want):
    _, r, x, t = got
    orr, ox, ot = want
    assert np.array_equal(r, orr)
    assert np.array_equal(t, ot), "spread traces differ"
    assert np.array_equal(x, ox), "final values differ from the oracle"


def assert_uniform(x, t, zeros=5):
    """One bit pattern at the end, and the last `zeros` recorded spreads are exactly 0."""
    assert np.all(x == x[0]), "the final values are not one bit pattern"
    tf = t.view(np.float64)
    assert len(tf) >= zeros and np.all(tf[-zeros:] == 0.0), tf[-zeros:]


def table_case(oracle_mod, name):
    cfg, fn, first = TABLE[name]
    state = fn(x0_of(oracle_mod, cfg)) if fn else None
    want = run_oracle(oracle_mod, cfg, state, name)
    tf = want[2].view(np.float64)
    assert tf[first] == 0.0 < tf[first - 1], (name, first, tf[first - 2:first + 2])
    return cfg, state, want


@pytest.mark.parametrize("name", list(TABLE))
def test_table(oracle_mod, name):
    cfg, state, want = table_case(oracle_mod, name)
    got = run_gpu(cfg, state, ACSIM_BIN_SA=1024)
    if name != "trimmed_t2_d16":   # (no binned kernel for that pair: module docstring)
        assert " narrow" in got[0], got[0]
    assert_matches(got, want)
    assert_uniform(got[2], got[3])
    if name == "across_zero":   # mixed signs at first (8-byte rounds), one small negative value at the end
        x0 = state
        assert x0.min() < 0.0 < x0.max()
        assert -1e-3 < got[2].view(np.float64)[0] < 0.0


def test_one_pass_phase_b(oracle_mod):
    """ACSIM_BIN_SPLIT=1 at d = 32: the one-pass NAR kernel through 8-byte, 4-byte and uniform rounds."""
    cfg, state, want = table_case(oracle_mod, "trimmed_t5_d32")
    got = run_gpu(cfg, state, ACSIM_BIN_SA=1024, ACSIM_BIN_SPLIT=1)
    assert " narrow" in got[0] and " split" not in got[0], got[0]
    assert_matches(got, want)
    assert_uniform(got[2], got[3])


def test_stepped_calls(oracle_mod):
    """round(45), then round(1) five times: each call's first round has no published pair and is an
    8-byte round over uniform values, so the widths go 0 -> 8 -> 0 again and again."""
    cfg = FIRST.replace(max_rounds=50)
    want = run_oracle(oracle_mod, cfg)
    with env(ACSIM_BIN_SA=1024):
        with acsim.Simulator(cfg, device=0) as g:
            assert " narrow" in g.kernel_name()
            g.round(45)
            for _ in range(5):
                g.round(1)
            got = ("", g.rounds(), bits(g.values(0)).copy(), bits(g.spread_trace(0)).copy())
    assert_matches(got, want)
    assert_uniform(got[2], got[3])


def test_set_state_back_to_x0(oracle_mod):
    """From a uniform state back to the original x^0, then 6 rounds: widths 0 -> 8."""
    cfg, _, want = table_case(oracle_mod, "trimmed_t5_d32")
    x0 = x0_of(oracle_mod, cfg)
    with env(ACSIM_BIN_SA=1024):
        with acsim.Simulator(cfg, device=0) as g:
            g.run()
            assert_matches(("", g.rounds(), bits(g.values(0)), bits(g.spread_trace(0))), want)
            assert_uniform(bits(g.values(0)), bits(g.spread_trace(0)))
            g.set_state(0, x0[None, :])
            g.round(6)
            r, x = g.rounds().copy(), bits(g.values(0)).copy()
            t = bits(g.spread_trace(0)[:7]).copy()
    orr, ox, ot = run_oracle(oracle_mod, cfg.replace(max_rounds=6), x0, "back_to_x0")
    assert np.array_equal(r, orr)
    assert np.array_equal(t, ot[:7])
    assert np.array_equal(x, ox)
    assert t.view(np.float64)[-1] > 0.0, "six rounds from x^0 were meant to leave a spread"


@pytest.mark.parametrize("c", [0.0, -0.0, 0.75])
def test_set_state_constant(oracle_mod, c):
    """set_state straight onto a constant vector, 4 rounds: the first at 8 bytes (nothing published),
    the rest uniform.  Zero is the value the one-side-of-zero test of the 4-byte width excludes."""
    cfg = FIRST.replace(max_rounds=4)
    state = np.full(N, c, dtype=np.float64)
    want = run_oracle(oracle_mod, cfg, state, f"const{c!r}")
    got = run_gpu(cfg, state, ACSIM_BIN_SA=1024)
    assert " narrow" in got[0], got[0]
    assert_matches(got, want)
    assert_uniform(got[2], got[3])   # (all five recorded spreads: x^0 .. x^4)


def test_eps_stops_at_the_oracles_round(oracle_mod):
    """EPS with eps = 1e-17 (below any nonzero spread here): the run ends at the first zero spread, where
    phase A's done exit and its uniform exit meet."""
    cfg = FIRST.replace(termination="eps", eps=1e-17, max_rounds=60)
    want = run_oracle(oracle_mod, cfg)
    first = TABLE["trimmed_t5_d32"][2]
    assert int(want[0][0]) == first, want[0]
    got = run_gpu(cfg, ACSIM_BIN_SA=1024)
    assert " narrow" in got[0], got[0]
    assert_matches(got, want)
    assert_uniform(got[2], got[3], zeros=1)


def test_switch_off_same_bits(oracle_mod):
    cfg, state, want = table_case(oracle_mod, "trimmed_t5_d32")
    on = run_gpu(cfg, state, ACSIM_BIN_SA=1024)
    off = run_gpu(cfg, state, ACSIM_BIN_SA=1024, ACSIM_BIN_NARROW=0)
    assert " narrow" in on[0] and " narrow" not in off[0], (on[0], off[0])
    assert np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3])
    assert_matches(off, want)
    assert_uniform(off[2], off[3])
