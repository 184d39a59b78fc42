"""CSR graphs whose rows take the big-m path (more than 8192 entries) at every merge-pass count and
tail-chunk width of k_big_sort, and an exact one-round reference for the sort-based rules on them.
TEST INFRASTRUCTURE (tests/test_big_rows.py, tests/test_gpu_big_rows.py, tests/test_properties.py).

k_big_sort (round_generic.hip) orders a row of m = deg + 1 entries in chunks of CHUNK = 8192: every
chunk is merge-sorted in LDS, the last one (L entries) padded to P = 256 .. 8192, then
np = ceil(log2(nch)) merge-path passes over nch = ceil(m / CHUNK) runs ping-pong between two global
buffers, the chunk sorts writing the buffer that the parity of np selects.  A pass over an odd number
of runs leaves its last run without a partner, and that run may be short.  BIG_M lists row sizes that
reach each of these branches and check_big_m asserts, from the chunk arithmetic alone, that a list of
sizes does.

exact_big_round recomputes one lossless, fault-free round of every big row in fractions.Fraction, and
check_exact_big_round holds a computed round against it within a bound that follows from the
operation count alone.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

CHUNK = 8192                                    # kBigChunk: entries per LDS chunk sort
TAIL_P = (256, 512, 1024, 2048, 4096, 8192)     # the widths a last chunk is padded to
# last-chunk lengths at both ends of every padded width
TAIL_L = (1, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8191, 8192)

PASS_ENDS = (8193, 16384, 16385, 32768, 32769, 65536, 65537, 131072, 131073)   # np = 1 .. 4 at both ends, and 5
ODD_RUNS = (16385, 40961, 100003)               # a pass over an odd number of runs: 3 (a tail of 1), 3 of 16384 (a tail
#                                                 of 8193) and 13 (a tail of 1699), whose last run has no partner
FULL_LONE = (24576,)                            # three full runs: the partnerless run has full width
ONE_WITH_PARTNER = (24577,)                     # four runs: a run of one entry that has a partner
TWO_CHUNK_TAILS = tuple(CHUNK + L for L in TAIL_L)
FOUR_CHUNK_TAILS = tuple(3 * CHUNK + L for L in (1, 257, 2049, 8191))
NOT_MULTIPLE_OF_8 = (100003, 16391)             # the 8-output merge step ends inside a step
BIG_M = tuple(sorted(set(PASS_ENDS + ODD_RUNS + FULL_LONE + ONE_WITH_PARTNER + TWO_CHUNK_TAILS + FOUR_CHUNK_TAILS + NOT_MULTIPLE_OF_8)))

N_PASS_GRAPH = 3000
N_ALL_BIG = 48


def chunks(m):
    return -(-int(m) // CHUNK)


def passes(m):
    """np of k_big_sort: the merge passes over a row of m entries."""
    return (chunks(m) - 1).bit_length()


def tail_len(m):
    return int(m) - (chunks(m) - 1) * CHUNK


def tail_width(m):
    """P of the last chunk's LDS sort."""
    return max(256, 1 << (tail_len(m) - 1).bit_length())


def first_buffer(m):
    """The buffer the chunk sorts write, so that the last pass lands in srt."""
    return "ent" if passes(m) & 1 else "srt"


def pass_runs(m):
    """[(run width w, number of runs, length of the last run)] of every merge pass."""
    out, w = [], CHUNK
    while w < m:
        runs = -(-int(m) // w)
        out.append((w, runs, int(m) - (runs - 1) * w))
        w *= 2
    return out


def lone_tails(m):
    """The passes whose last run has no partner: [(w, length of that run)]."""
    return [(w, last) for w, runs, last in pass_runs(m) if runs & 1]


def check_big_m(ms):
    """The conditions BIG_M is chosen for, each from the chunk arithmetic; a size list that stops
    covering a class fails the assertion that names it."""
    ms = sorted(int(m) for m in ms)
    have = set(ms)
    assert ms[0] > CHUNK, "every row is on the big-m path"
    for np_ in (1, 2, 3, 4):   # the smallest and the largest row of np passes
        low, high = (CHUNK << (np_ - 1)) + 1, CHUNK << np_
        assert passes(low) == passes(high) == np_ and passes(low - 1) == np_ - 1 and passes(high + 1) == np_ + 1
        assert low in have, ("pass count, low end", np_, low)
        assert high in have, ("pass count, high end", np_, high)
    assert {first_buffer(m) for m in ms} == {"ent", "srt"}, "both parities of the pass count"
    assert any(passes(m) >= 5 for m in ms), "a row of five passes"
    for m in ODD_RUNS:
        assert m in have and lone_tails(m), ("odd run count", m)
    for m in ONE_WITH_PARTNER:
        assert m in have and pass_runs(m)[0][1:] == (4, 1), ("a run of one entry with a partner", m)
    lone = [t for m in ms for t in lone_tails(m)]
    assert any(last == 1 for _, last in lone), "a partnerless run of one entry"
    assert any(1 < last < w for w, last in lone), "a partnerless run that is short"
    assert any(last == w for w, last in lone), "a partnerless run of full width"
    assert any(w > CHUNK and last < w for w, last in lone), "a short partnerless run after the first pass"
    assert any(runs & 1 == 0 and last < w for m in ms for w, runs, last in pass_runs(m)), "a short run with a partner"
    for nch in (2, 4):   # every padded width of the last chunk, at both ends, behind 1 and (a few) behind 3 chunks
        got = {tail_len(m) for m in ms if chunks(m) == nch}
        if nch == 2:
            assert got >= set(TAIL_L), ("tail lengths behind one chunk", sorted(set(TAIL_L) - got))
        else:
            assert len(got) >= 4 and {tail_width(m) for m in ms if chunks(m) == nch} >= {256, 512, 4096, 8192}
    for P in TAIL_P:
        lens = {tail_len(m) for m in ms if tail_width(m) == P}
        assert (1 if P == 256 else P // 2 + 1) in lens and P in lens, ("tail width, both ends", P)
    for m in NOT_MULTIPLE_OF_8:
        assert m in have and m % 8, ("not a multiple of 8", m)
    assert any(m % 8 and passes(m) >= 2 for m in ms) and any(m % 8 and tail_len(m) < 8 for m in ms)
    return {m: (chunks(m), passes(m), tail_width(m)) for m in ms}


def big_rows(rp):
    return np.nonzero(np.diff(np.asarray(rp, dtype=np.int64)) + 1 > CHUNK)[0]


def _csr(deg, rng):
    n = deg.size
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    return rp, rng.integers(0, n, int(rp[-1])).astype(np.uint32)   # uniform senders, repeats allowed


def pass_graph(seed=0):
    """3000 rows (46 full SELL slices and a partial one), nnz about 0.9 million: one row of every size
    in BIG_M at a random place, every other row with 3 .. 6 senders, so the big rows run beside the
    lane kernel and the generic kernel of the same round.  Admits trims t <= 1."""
    rng = np.random.default_rng([seed, N_PASS_GRAPH])
    n = N_PASS_GRAPH
    deg = rng.integers(3, 7, n)
    deg[rng.permutation(n)[:len(BIG_M)]] = np.array(BIG_M) - 1
    rp, ci = _csr(deg, rng)
    check_pass_graph(rp, ci)
    return rp, ci


def check_pass_graph(rp, ci):
    deg = np.diff(rp.astype(np.int64))
    n = deg.size
    assert n == N_PASS_GRAPH and n % 64 != 0
    big = deg[big_rows(rp)] + 1
    assert sorted(big.tolist()) == list(BIG_M) and big.size * 4 <= n   # the handle keeps its fast path
    small = deg[deg + 1 <= CHUNK]
    assert small.min() == 3 and small.max() == 6
    assert ci.size == int(rp[-1]) and ci.max() < n
    return check_big_m(big)


def all_big_graph(seed=0):
    """48 rows, every one on the big-m path: one row of every size in BIG_M and the rest of 100 000 ..
    140 000 entries at random, nnz about 3.4 million.  With 48 nodes a row holds at most 48 distinct
    values, so every merge is dominated by ties, and every row admits trims up to 4096."""
    rng = np.random.default_rng([seed, N_ALL_BIG])
    n = N_ALL_BIG
    assert len(BIG_M) < n
    deg = rng.integers(100000, 140000, n)
    deg[rng.permutation(n)[:len(BIG_M)]] = np.array(BIG_M) - 1
    rp, ci = _csr(deg, rng)
    check_all_big_graph(rp, ci)
    return rp, ci


def check_all_big_graph(rp, ci):
    deg = np.diff(rp.astype(np.int64))
    assert deg.size == N_ALL_BIG and big_rows(rp).size == N_ALL_BIG
    m = deg + 1
    assert set(BIG_M) <= set(m.tolist()) and m.min() == CHUNK + 1 and m.max() <= 140000
    assert (m > 131073).any()                                     # a random row above every listed size
    assert 3_000_000 <= ci.size <= 4_000_000 and ci.max() < N_ALL_BIG
    return check_big_m(m)


# ----------------------------------------------------------------------------- the case matrices
# Config fields of the cases that tests/test_big_rows.py (oracle against spec_np.NpSim) and
# tests/test_gpu_big_rows.py (handle against oracle) both run; 3 FIXED rounds unless a case says otherwise.
RULES_T1 = dict(average=dict(rule="average", trim=0), trimmed=dict(rule="trimmed", trim=1),
                midpoint=dict(rule="midpoint", trim=1), dlpsw=dict(rule="dlpsw", trim=1), wmsr=dict(rule="wmsr", trim=1))
PASS_CASES = {}
for _name, _kw in RULES_T1.items():
    PASS_CASES[_name + "_clean"] = dict(_kw)
    PASS_CASES[_name + "_loss"] = dict(_kw, loss_p=0.2)
PASS_CASES.update(
    average_omit=dict(rule="average", trim=0, loss_p=0.2, missing_policy="omit"),
    trimmed_omit=dict(rule="trimmed", trim=1, loss_p=0.2, missing_policy="omit"),
    trimmed_crash=dict(rule="trimmed", trim=1, loss_p=0.2, fault_model="crash", n_faulty=700, crash_window=3),
    wmsr_crash=dict(rule="wmsr", trim=1, fault_model="crash", n_faulty=700, crash_window=2),
    midpoint_byz_random=dict(rule="midpoint", trim=1, fault_model="byzantine", n_faulty=600, byz_strategy="random",
                             byz_delta=0.2),
    trimmed_byz_constant=dict(rule="trimmed", trim=1, fault_model="byzantine", n_faulty=600, byz_strategy="constant",
                              byz_const=0.375, loss_p=0.2),
    wmsr_byz_constant=dict(rule="wmsr", trim=1, fault_model="byzantine", n_faulty=600, byz_strategy="constant",
                           byz_const=0.375),
    trimmed_f32=dict(rule="trimmed", trim=1, loss_p=0.2, dtype="f32"),
    dlpsw_f32=dict(rule="dlpsw", trim=1, dtype="f32"),
    midpoint_f32_byz_constant=dict(rule="midpoint", trim=1, dtype="f32", fault_model="byzantine", n_faulty=600,
                                   byz_strategy="constant", byz_const=0.375),
    trimmed_delay2=dict(rule="trimmed", trim=1, loss_p=0.2, delay_max=2, max_rounds=4),
    trimmed_inst3=dict(rule="trimmed", trim=1, loss_p=0.2, n_instances=3, instance_offset=5),
    average_inst3=dict(rule="average", trim=0, loss_p=0.2, n_instances=3, instance_offset=5, mask_group=2),
)
ALL_BIG_CASES = dict(
    trimmed_t4000=dict(rule="trimmed", trim=4000),
    trimmed_t3000_omit=dict(rule="trimmed", trim=3000, loss_p=0.6, missing_policy="omit"),
    midpoint_t4096=dict(rule="midpoint", trim=4096),
    midpoint_t4096_byz_random=dict(rule="midpoint", trim=4096, fault_model="byzantine", n_faulty=9, byz_strategy="random",
                                   byz_delta=0.2),
    dlpsw_t37=dict(rule="dlpsw", trim=37),
    dlpsw_t4000=dict(rule="dlpsw", trim=4000),
    wmsr_t2000_byz_constant=dict(rule="wmsr", trim=2000, fault_model="byzantine", n_faulty=9, byz_strategy="constant",
                                 byz_const=0.375),
    average=dict(rule="average", trim=0),
    average_omit=dict(rule="average", trim=0, loss_p=0.3, missing_policy="omit"),
    trimmed_f32=dict(rule="trimmed", trim=4000, dtype="f32"),
    trimmed_loss=dict(rule="trimmed", trim=4000, loss_p=0.2),
)
EXACT_RULES = dict(average=0, trimmed=3000, midpoint=4096, dlpsw=37, wmsr=2000)   # trims of the exact-round cases (all_big_graph)


def exact_kw(rule, graph):
    """The lossless, fault-free case of the exact-round tests: t = 1 on pass_graph, EXACT_RULES' on all_big_graph."""
    return dict(rule=rule, trim=0 if rule == "average" else 1 if graph == "pass_graph" else EXACT_RULES[rule])


def case_cfg(graph, kw, **over):
    from acsim.config import Config
    n = dict(pass_graph=N_PASS_GRAPH, all_big_graph=N_ALL_BIG)[graph]
    return Config(**{**dict(n_nodes=n, topology="csr", seed=91, trace_spread=True, termination="fixed", max_rounds=3),
                     **kw, **over})


# ----------------------------------------------------------------------------- one exact round
UNIT = {"f64": Fraction(1, 2 ** 53), "f32": Fraction(1, 2 ** 24)}


def _exact_sum(vals):
    """(sum, sum of magnitudes) of a float array, exactly: every distinct value once, times its count."""
    v, c = np.unique(np.asarray(vals, dtype=np.float64), return_counts=True)
    terms = [Fraction(a) * int(k) for a, k in zip(v.tolist(), c.tolist())]
    return sum(terms, Fraction(0)), sum((abs(t) for t in terms), Fraction(0))


def exact_big_round(cfg, csr, x):
    """One lossless, fault-free, undelayed round of every big row from state x (one instance's values,
    stored binary values taken exactly).  Row i's entries are x_i and x_j of every sender slot; they
    are sorted by value (an exact comparison sort of floats) and the rule is evaluated in Fractions:
      average   the mean of all m entries
      trimmed   the mean of sorted[t : m - t]
      midpoint  (sorted[t] + sorted[m - t - 1]) / 2
      dlpsw     the mean of every t-th entry of sorted[t : m - t]
      wmsr      the mean of sorted[lo : m - hi], lo = min(t, #entries < x_i), hi = min(t, #entries > x_i)
    -> {row: (exact result, cnt, sum of |v| over the cnt selected entries)}; for midpoint cnt = 2 and
    the third field is |v_lo + v_hi|."""
    rp = np.asarray(csr[0], dtype=np.int64)
    ci = np.asarray(csr[1], dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    rule, t = cfg.rule, int(cfg.trim)
    assert cfg.loss_p == 0 and cfg.fault_model == "none" and int(cfg.delay_max) == 0
    out = {}
    for i in big_rows(rp).tolist():
        s = np.sort(np.concatenate([[x[i]], x[ci[rp[i]:rp[i + 1]]]]), kind="stable")
        m = s.size
        if rule == "midpoint":
            both = Fraction(float(s[t])) + Fraction(float(s[m - t - 1]))
            out[i] = (both / 2, 2, abs(both))
            continue
        if rule == "average":
            sel = s
        elif rule == "trimmed":
            sel = s[t:m - t]
        elif rule == "dlpsw":
            sel = s[t:m - t][::t]
        else:
            assert rule == "wmsr"
            lo, hi = min(t, int((s < x[i]).sum())), min(t, int((s > x[i]).sum()))
            sel = s[lo:m - hi]
        total, mag = _exact_sum(sel)
        out[i] = (total / sel.size, int(sel.size), mag)
    return out


def check_exact_big_round(cfg, csr, before, after):
    """A computed round (x `before` -> x `after` of one instance) of every big row against
    exact_big_round.  The bound, from the operation count alone, u = 2^-53 (f64) or 2^-24 (f32):
      a stride-halving tree sum of cnt terms has depth L = ceil(log2 cnt), every level one rounded add,
      and one rounded division by cnt (exact in either format) follows, so
          |res - exact| <= ((1 + u)^(L + 1) - 1) * sum |v| / cnt;
      midpoint is one rounded add and an exact halving: |res - exact| <= u * |v_lo + v_hi| / 2.
    The entries are values of [2^-200, 2^200] or 0 (asserted), so nothing underflows.
    -> the worst error / bound over the rows; asserts it is at most 1."""
    u = UNIT[cfg.dtype]
    b = np.asarray(before, dtype=np.float64)
    nz = np.abs(b[b != 0])
    assert np.isfinite(b).all() and (not nz.size or (nz.min() >= 2.0 ** -200 and nz.max() <= 2.0 ** 200))
    want = exact_big_round(cfg, csr, b)
    assert len(want) == big_rows(csr[0]).size > 0
    worst = Fraction(0)
    for i, (exact, cnt, mag) in want.items():
        got = Fraction(float(after[i]))
        if cfg.rule == "midpoint":
            bound = u * mag / 2
        else:
            L = (cnt - 1).bit_length()
            bound = ((1 + u) ** (L + 1) - 1) * mag / cnt
        if bound == 0:
            assert got == exact, (i, float(got), float(exact))
            continue
        ratio = abs(got - exact) / bound
        assert ratio <= 1, (cfg.rule, i, float(got), float(exact), float(ratio))
        worst = max(worst, ratio)
    return float(worst)
