"""kernel_name() of one handle per branch of handle creation (csrc/create.hip: path choice, binned
decision, plan-refusal fallback, decorations), string for string against
tests/golden/kernel_names.json.  The golden file was recorded on the MI355X by
tools/record_kernel_names.py from a build of the commit before handle creation was split into
stages and the name derived in one place (kernel_name_of), never from that code; this test shares
the recorder's case list.  Each case creates one handle and runs no round.

Branches left out (1): the CSR plan-refusal fallback.  binned_build refuses a plan once laid out
only where a two-level phase-M image outgrows its LDS bound or a receiver block has too many runs.
The one known shape that does so is RANDOM_REGULAR (case parts3_plan_refused, the shape of
tests/test_gpu_partition.py: the local rows of three partitions); none of the CSR graphs the suite
uses is refused, and no case is contorted to find one.  Both fallbacks run the same drop_binned.
"""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "record_kernel_names", os.path.join(os.path.dirname(HERE), "tools", "record_kernel_names.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

with open(os.path.join(HERE, "golden", "kernel_names.json")) as f:
    GOLDEN = json.load(f)


def test_golden_file_covers_the_case_list():
    names = [c[0] for c in recorder.CASES]
    assert len(set(names)) == len(names)
    assert len(GOLDEN) == len(names)
    assert set(GOLDEN) == set(names)


def test_golden_file_reaches_every_branch():
    """The fragments the case list is there for, each in at least one recorded name."""
    recorded = "\n".join(GOLDEN.values())
    for frag in ("k_batched_small<", "k_batched_split<2>", "k_batched_split<4>", "k_batched_mfma<", "k_dense_persist",
                 "k_dense_sort+k_dense_recv", "k_round_regular<8,2,clean>", "k_round_regular<8,2,faulty>",
                 "k_bin_scatter+k_bin_gather<", "k_bin_regroup+", ",faulty>", "+k_bin_tag", "+k_bin_fixup", " split2",
                 " split3", " pk14A", " narrow", " sb128", " [f32]", ",csr>", ",faulty,csr>", "+k_round_generic(hubs)",
                 "k_round_weighted<32,csr>+k_round_generic(hubs)", "k_round_weighted<8,csr>",
                 "k_round_pushsum<32,csr>+k_round_generic(hubs)", "k_round_pushsum<8,csr>",
                 "k_round_generic+k_big_resolve+sort+k_big_rule", " xchunks4", " xchunks2"):
        assert frag in recorded, frag
    assert GOLDEN["parts3_plan_refused"].startswith("k_round_regular<")   # the regular plan-refusal fallback
    assert "xchunks" not in GOLDEN["parts2_xchunks_off"]
    assert GOLDEN["big_m_complete_8300_loss"] == "k_big_resolve+sort+k_big_rule"
    assert GOLDEN["generic_complete_delay"] == "k_round_generic"


@pytest.mark.gpu
@pytest.mark.parametrize("case", recorder.CASES, ids=[c[0] for c in recorder.CASES])
def test_kernel_name_matches_parent(case):
    assert recorder.kernel_name(case) == GOLDEN[case[0]]
