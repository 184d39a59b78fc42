"""Uniform rounds, the rule evaluated once per workgroup: in a round of
width 0 every receiver's D + 1 inputs are the header's one bit pattern, so wave 0 of each phase-B
workgroup evaluates the rule, the workgroup takes the value from LDS behind one barrier that dead
lanes reach too, every live lane stores it, and thread 0 writes the block's (min, max) pair as
(R, R).  The result must still be the rule's on those inputs: the tree sum of D + 1 - 2t copies of
0.1 divided by the count need not be 0.1, so a constant state may drift from round to round while
staying uniform.

Bar (as in test_gpu_narrow_uniform.py): bit-exact against the oracle in values, rounds and spread
trace; one bit pattern at the end; a trace whose last five spreads are exactly 0.  Every GPU run
asserts that the kernel name holds " narrow".  The first uniform round of a run is read from the
oracle's trace.  ACSIM_BIN_SA=1024 throughout; receiver blocks hold 256 receivers (4 waves).
"""
import contextlib
import math
import os

import numpy as np
import pytest

import acsim
from acsim.config import Config

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, os.cpu_count() or 1))
KNOBS = ("ACSIM_BIN_NARROW", "ACSIM_BIN_SA", "ACSIM_BIN_SPLIT", "ACSIM_BIN_AWG")
SEED = 3
ROUNDS = 56   # FIXED rounds of the d = 32 natural runs: past exact agreement in every case (asserted)


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


def regular(n, d, rule, trim, rounds=ROUNDS):
    return Config(n_nodes=n, topology="regular", degree=d, rule=rule, trim=trim, termination="fixed",
                  max_rounds=rounds, seed=SEED, trace_spread=True)


_oracle_cache = {}


def run_oracle(oracle_mod, cfg, state=None, tag=""):
    """(rounds, value bits, trace bits) of the oracle's run from `state` (or the default x^0),
    computed once per (config, tag) and never modified."""
    key = (repr(cfg), tag)
    if key not in _oracle_cache:
        with oracle_mod.OracleSimulator(cfg, threads=THREADS) as o:
            if state is not None:
                o.set_state(0, state[None, :])
            o.run()
            _oracle_cache[key] = (o.rounds().copy(), bits(o.values(0)).copy(), bits(o.spread_trace(0)).copy())
    return _oracle_cache[key]


def run_gpu(cfg, state=None, **kw):
    with env(ACSIM_BIN_SA=1024, **kw):
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


def first_uniform(want):
    """The first round after which the oracle's values are one bit pattern (trace[r] == 0 <
    trace[r - 1]); round r + 1 is the first of width 0.  At least five uniform rounds must follow."""
    tf = want[2].view(np.float64)
    zero = np.flatnonzero(tf == 0.0)
    assert len(zero), "the oracle's run never reaches exact agreement"
    r = int(zero[0])
    assert r >= 1 and tf[r - 1] > 0.0 and np.all(tf[r:] == 0.0), tf[max(r - 2, 0):r + 2]
    assert r + 5 <= len(tf) - 1, (r, len(tf))
    return r


def natural_case(oracle_mod, cfg, **kw):
    want = run_oracle(oracle_mod, cfg)
    first_uniform(want)
    got = run_gpu(cfg, **kw)
    assert " narrow" in got[0], got[0]
    if kw.get("ACSIM_BIN_SPLIT") == 1:
        assert " split" not in got[0], got[0]
    assert_matches(got, want)
    assert_uniform(got[2], got[3])


# ---- ragged last blocks (trimmed t = 5, d = 32): 4096 = 16 full receiver blocks; 4097: one live lane
# in the 17th, its waves 1-3 wholly dead; 4160: wave 0 full, waves 1-3 dead; 4161: one live lane in
# wave 1 (the value crosses waves in a partial block); 4351: the last block one lane short
@pytest.mark.parametrize("n", [4096, 4097, 4160, 4161, 4351])
def test_ragged_last_block(oracle_mod, n):
    natural_case(oracle_mod, regular(n, 32, "trimmed", 5))


# ---- every rule with a narrow kernel, on the default plan and on the one-pass NAR kernel
RULES = {
    "trimmed_t5_d32": (32, "trimmed", 5, ROUNDS),
    "average_d32": (32, "average", 0, ROUNDS),
    "midpoint_d32": (32, "midpoint", 5, ROUNDS),
    "dlpsw_d32": (32, "dlpsw", 5, ROUNDS),
    "wmsr_d32": (32, "wmsr", 5, ROUNDS),
    "trimmed_t5_d16": (16, "trimmed", 5, 100),   # (7 of 17 values kept: agreement takes about 90 rounds)
}
N_RULES = 4161


@pytest.mark.parametrize("split", [None, 1], ids=["default", "one_pass"])
@pytest.mark.parametrize("name", list(RULES))
def test_rules(oracle_mod, name, split):
    d, rule, trim, rounds = RULES[name]
    natural_case(oracle_mod, regular(N_RULES, d, rule, trim, rounds), ACSIM_BIN_SPLIT=split)


# ---- constants whose rule value need not be the constant: set_state, then 8 FIXED rounds (the first
# at 8 bytes: nothing is published after set_state; the rest uniform).  On the oracle -0.0 becomes
# +0.0 in the first round, 123.456 and 1.7 move by an ulp or more in some of the rounds under both
# rules below, and the others stay put.
CONSTANTS = {
    "0.1": 0.1, "third": 1.0 / 3.0, "pi": math.pi, "minus_0.1": -0.1, "1e-300": 1e-300,
    "min_subnormal": 5e-324, "plus_zero": 0.0, "minus_zero": -0.0, "123.456": 123.456, "1.7": 1.7,
}
CONST_RULES = {"trimmed_t5": ("trimmed", 5), "average": ("average", 0)}


def constant_case(oracle_mod, cname, rname, **kw):
    rule, trim = CONST_RULES[rname]
    cfg = regular(N_RULES, 32, rule, trim, rounds=8)
    state = np.full(N_RULES, CONSTANTS[cname], dtype=np.float64)
    want = run_oracle(oracle_mod, cfg, state, f"const_{cname}")
    got = run_gpu(cfg, state, **kw)
    assert_matches(got, want)
    assert_uniform(got[2], got[3], zeros=9)   # (every recorded spread: x^0 .. x^8)
    return got


@pytest.mark.parametrize("rname", list(CONST_RULES))
@pytest.mark.parametrize("cname", list(CONSTANTS))
def test_constant_state(oracle_mod, cname, rname):
    got = constant_case(oracle_mod, cname, rname)
    assert " narrow" in got[0], got[0]


def test_constant_state_one_pass(oracle_mod):
    got = constant_case(oracle_mod, "123.456", "trimmed_t5", ACSIM_BIN_SPLIT=1)
    assert " narrow" in got[0] and " split" not in got[0], got[0]


def test_constant_state_switch_off_same_bits(oracle_mod):
    """ACSIM_BIN_NARROW=0 (8-byte rounds throughout, every lane evaluating the rule): the same bits."""
    on = constant_case(oracle_mod, "123.456", "trimmed_t5")
    off = constant_case(oracle_mod, "123.456", "trimmed_t5", ACSIM_BIN_NARROW=0)
    assert " narrow" in on[0] and " narrow" not in off[0], (on[0], off[0])
    assert np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3])


# ---- stepped calls in the uniform regime, and the round info a call returns
def info_tuple(i):
    return (int(i.round), bits(np.array([i.spread, i.lo, i.hi], dtype=np.float64)).tolist())


def test_stepped_calls_and_round_info(oracle_mod):
    """From a constant state: round(1) six times (each an 8-byte round: a call's first round has no
    published pair), then round(3) (widths 8, 0, 0).  After every call the values and the returned
    round info are the oracle's; after the uniform rounds lo == hi == the value and spread == 0: the
    block pairs written as (R, R) fold to exactly that."""
    cfg = regular(N_RULES, 32, "trimmed", 5, rounds=9)
    state = np.full(N_RULES, 123.456, dtype=np.float64)   # (a constant that moves: CONSTANTS)
    with env(ACSIM_BIN_SA=1024):
        with acsim.Simulator(cfg, device=0) as g, oracle_mod.OracleSimulator(cfg, threads=THREADS) as o:
            assert " narrow" in g.kernel_name(), g.kernel_name()
            g.set_state(0, state[None, :])
            o.set_state(0, state[None, :])
            for k in (1, 1, 1, 1, 1, 1, 3):
                gi, oi = g.round(k), o.round(k)
                x, ox = bits(g.values(0)), bits(o.values(0))
                assert np.array_equal(x, ox), f"values differ after round {int(oi.round)}"
                assert info_tuple(gi) == info_tuple(oi), (gi, info_tuple(oi))
                assert np.all(x == x[0])
                assert np.all(bits(np.array([gi.lo, gi.hi], dtype=np.float64)) == x[0]) and gi.spread == 0.0, gi
            assert int(gi.round) == 9
            assert np.array_equal(g.rounds(), o.rounds())
            t, ot = bits(g.spread_trace(0)), bits(o.spread_trace(0))
            assert np.array_equal(t, ot), "spread traces differ"
            assert_uniform(x, t, zeros=10)
