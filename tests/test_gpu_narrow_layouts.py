"""Narrow stage by default: a clean one-level fp64 plan of d = 16 / 32 is a narrow
plan unless ACSIM_BIN_NARROW=0, and every round picks its stage entry width on the device.  These
runs cross from the 8-byte rounds to the 4-byte ones (and back), with tiles of every length mod 4,
one- and two-pass phase B and source blocks cut into several phase-A segments.  Bar: bit-exact
(values, rounds, spread traces) against the oracle.  ACSIM_BIN_NARROW is unset unless a case says
otherwise.

No case for a plan whose u32 image fails the build's fit check: a one-level plan has at most 4d
source blocks (binned_levels), so a block's image carries at most 12d padding entries beyond its
256 d deliveries, and the smallest phase-B buffer a narrow plan can meet (two passes) holds
256 d + 32 d + 4 u32 entries.  No shape reaches that refusal.  The refusal that can be reached, a
pass count the NAR kernels are not compiled for, is covered instead.
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


def regular(n, d, rounds, seed):
    return Config(n_nodes=n, topology="regular", degree=d, rule="trimmed", trim=5, termination="fixed",
                  max_rounds=rounds, seed=seed, trace_spread=True)


CFG = regular(50001, 32, 60, 5)

_oracle_cache = {}


def run_oracle(oracle_mod, cfg):
    """(rounds, value bits, trace bits) of the oracle's run, computed once per config."""
    key = repr(cfg)
    if key not in _oracle_cache:
        with oracle_mod.OracleSimulator(cfg, threads=THREADS) as o:
            o.run()
            _oracle_cache[key] = (o.rounds().copy(), bits(o.values(0)).copy(), bits(o.spread_trace(0)).copy())
    return _oracle_cache[key]


def run_gpu(cfg, **kw):
    with env(**kw):
        with acsim.Simulator(cfg, device=0) as g:
            name = g.kernel_name()
            g.run()
            return name, g.rounds(), bits(g.values(0)).copy(), bits(g.spread_trace(0)).copy()


def assert_matches(got, want):
    _, r, x, t = got
    orr, ox, ot = want
    assert np.array_equal(r, orr)
    assert np.array_equal(t, ot), "spread traces differ"
    assert np.array_equal(x, ox), "final values differ from the oracle"


def assert_narrowed(x, t):
    """The run reached the 4-byte rounds: its last recorded spread is below 2^32 ulps."""
    assert t.view(np.float64)[-1] < 2.0 ** 32 * np.spacing(np.abs(x.view(np.float64)).max())


def test_default_is_narrow(oracle_mod):
    got = run_gpu(CFG, ACSIM_BIN_SA=1024)
    assert " narrow" in got[0], got[0]
    assert_matches(got, run_oracle(oracle_mod, CFG))
    assert_narrowed(got[2], got[3])


def test_switch_off(oracle_mod):
    on = run_gpu(CFG, ACSIM_BIN_SA=1024)
    off = run_gpu(CFG, ACSIM_BIN_SA=1024, ACSIM_BIN_NARROW=0)
    assert " narrow" in on[0] and " narrow" not in off[0], (on[0], off[0])
    assert np.array_equal(on[2], off[2]), "the default run and ACSIM_BIN_NARROW=0 differ"
    assert_matches(off, run_oracle(oracle_mod, CFG))
    one = run_gpu(CFG, ACSIM_BIN_SA=1024, ACSIM_BIN_NARROW=1)
    assert " narrow" in one[0], one[0]
    assert np.array_equal(one[2], on[2])


@pytest.mark.parametrize("n,d,seed", [(50001, 32, 5), (40000, 16, 7), (30011, 16, 21)])
def test_pad_residues(oracle_mod, n, d, seed):
    """n is no multiple of 256 or (but for 40000 = 39 * 1024 + 64) of the source block: tiles of every
    length mod 4 (padded to 4 entries for both widths), and the run goes from 8-byte to 4-byte rounds."""
    cfg = regular(n, d, 60, seed)
    got = run_gpu(cfg, ACSIM_BIN_SA=1024)
    assert " narrow" in got[0], got[0]
    assert_matches(got, run_oracle(oracle_mod, cfg))
    assert_narrowed(got[2], got[3])


def test_one_pass_phase_b(oracle_mod):
    """ACSIM_BIN_SPLIT=1 at d = 32: the one-pass NAR kernel goes through both widths."""
    cfg = regular(30011, 32, 60, 8)
    got = run_gpu(cfg, ACSIM_BIN_SA=1024, ACSIM_BIN_SPLIT=1)
    assert " narrow" in got[0] and " split" not in got[0], got[0]
    assert_matches(got, run_oracle(oracle_mod, cfg))
    assert_narrowed(got[2], got[3])


def test_several_phase_a_segments(oracle_mod):
    """n = 65536 at the default source block: 4 source blocks; 16 phase-A workgroups per launch cut
    each block into 4 segments, streamed at both widths."""
    cfg = regular(65536, 32, 45, 6)
    got = run_gpu(cfg, ACSIM_BIN_AWG=16)
    assert " narrow" in got[0], got[0]
    assert_matches(got, run_oracle(oracle_mod, cfg))
    assert_narrowed(got[2], got[3])


def test_back_to_8_bytes(oracle_mod):
    """After the run has narrowed, set_state onto values that straddle zero (full width again) and
    more rounds: 4-byte rounds are followed by 8-byte ones on the same handle."""
    cfg = CFG.replace(max_rounds=4)
    with env(ACSIM_BIN_SA=1024):
        with acsim.Simulator(cfg.replace(max_rounds=1), device=0) as g0:
            x0 = g0.values(0).copy()
        x0 -= x0.mean()   # (four rounds leave the spread far above the drift of the centre)
        with acsim.Simulator(CFG, device=0) as g:
            assert " narrow" in g.kernel_name()
            g.run()
            assert_narrowed(bits(g.values(0)), bits(g.spread_trace(0)))
            g.set_state(0, x0[None, :])
            g.round(4)
            r, x = g.rounds().copy(), bits(g.values(0)).copy()
            t = bits(g.spread_trace(0)[:5]).copy()
    with oracle_mod.OracleSimulator(cfg, threads=THREADS) as o:
        o.set_state(0, x0[None, :])
        o.run()
        assert np.array_equal(r, o.rounds())
        assert np.array_equal(x, bits(o.values(0)))
        assert np.array_equal(t, bits(o.spread_trace(0)[:5]))
    xf = x.view(np.float64)
    assert xf.min() < 0.0 < xf.max(), "the resumed rounds were meant to straddle zero"


def test_refused_narrow_plan(oracle_mod):
    """Three passes: no NAR kernel, so the plan asks for narrow, is refused and runs on the
    default kernels."""
    got = run_gpu(CFG, ACSIM_BIN_SA=1024, ACSIM_BIN_SPLIT=3)
    assert " narrow" not in got[0] and " split3" in got[0], got[0]
    assert_matches(got, run_oracle(oracle_mod, CFG))
