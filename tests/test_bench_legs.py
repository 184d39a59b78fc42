"""bench.py's multi-rank leg logic on the CPU (no GPU, no RCCL): the cfg5 leg at N > 1 reports
each exchange sequence as it finishes, takes its headline fields from the first golden-matching
sequence, and marks the leg failed when the default (all-gather) sequence errs or mismatches; the
opt-in chunked sequence's result is reported as opt_in_ok.  The sub-legs are stubbed; the real ones run on the GPU box (bench.py, rehearsal in
tools/sessions_scripts/r06_rehearsal.sh)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class FakeCtx(bench.Ctx):
    def __init__(self, rank=0, world=2):
        super().__init__(world, rank, rank, 0, None)

    def all_ok(self, ok):
        return ok

    def barrier(self, sim=None):
        pass


def run_leg(monkeypatch, results, rank=0):
    seen = []

    def fake_sub(ctx, warm, timed, xchunks, stage="cfg5_partitioned"):
        ctx.enter(stage)
        seen.append((stage, xchunks, dict(ctx.partial.get("sequences", {}))))
        r = results[stage.split(".")[-1]]
        if isinstance(r, Exception):
            raise r
        return dict(r)

    monkeypatch.setattr(bench, "_cfg5_sub", fake_sub)
    ctx = FakeCtx(rank=rank)
    ctx.partial = {"running": True}
    return bench.leg_cfg5(ctx), ctx, seen


def test_both_sequences_match(monkeypatch):
    ok = {"golden_match": True, "ms_per_round": 1.0}
    out, ctx, seen = run_leg(monkeypatch, {"allgather": dict(ok, ms_per_round=2.0), "chunked": ok})
    assert [s[0] for s in seen] == ["cfg5_partitioned.allgather", "cfg5_partitioned.chunked"]
    assert [s[1] for s in seen] == [None, 4]
    # the all-gather result was already in the printed line while the chunked sub-leg ran
    assert "allgather" in seen[1][2] and seen[1][2]["allgather"]["ms_per_round"] == 2.0
    assert out["headline_sequence"] == "allgather" and out["ms_per_round"] == 2.0
    assert out["ok"] is True and out["opt_in_ok"] is True and set(out["sequences"]) == {"allgather", "chunked"}


def test_chunked_mismatch_keeps_allgather_and_is_reported(monkeypatch):
    """The opt-in chunked sequence failing is reported (opt_in_ok) but does not fail the leg: the
    default sequence's result stands and the run keeps its exit code."""
    out, _, _ = run_leg(monkeypatch, {"allgather": {"golden_match": True, "ms_per_round": 2.0},
                                      "chunked": {"golden_match": False, "ms_per_round": 1.0}})
    assert out["headline_sequence"] == "allgather" and out["ms_per_round"] == 2.0
    assert out["ok"] is True and out["opt_in_ok"] is False


def test_allgather_error_falls_back_to_chunked(monkeypatch):
    out, _, _ = run_leg(monkeypatch, {"allgather": RuntimeError("ECOMM: invalid usage"),
                                      "chunked": {"golden_match": True, "ms_per_round": 1.0}})
    assert out["sequences"]["allgather"]["error"].startswith("RuntimeError: ECOMM")
    assert out["headline_sequence"] == "chunked" and out["ms_per_round"] == 1.0
    assert out["ok"] is False and out["opt_in_ok"] is True   # the default sequence failed: the leg fails


def test_no_sequence_matches(monkeypatch):
    out, _, _ = run_leg(monkeypatch, {"allgather": RuntimeError("a"), "chunked": RuntimeError("b")})
    assert "error" in out and out["headline_sequence"] is None and out["ok"] is False
    assert set(out["sequences"]) == {"allgather", "chunked"}


def test_other_ranks_return_nothing(monkeypatch):
    out, _, seen = run_leg(monkeypatch, {"allgather": {"golden_match": True}, "chunked": {"golden_match": True}},
                           rank=1)
    assert out == {} and len(seen) == 2   # every rank runs both sub-legs (RCCL needs all ranks)


def test_plain_run_has_no_legs_and_full_has_all():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.legs, a.dump_outputs) == (7, 2, False, "", None)
    assert bench.parse(["--legs="]).legs == ""     # what the profiling scripts pass
    assert bench.parse(["--full"]).legs == bench.ALL_LEGS
    assert set(bench.ALL_LEGS.split(",")) == set(bench.LEGS)
    assert bench.parse(["--full", "--legs="]).legs == ""
    assert bench.parse(["--full", "--legs", "cfg3"]).legs == "cfg3"
    with pytest.raises(SystemExit):
        bench.parse(["--legs", "cfg3"])


def test_dump_sample_is_fixed_and_fits():
    import numpy as np
    assert bench.dump_sample(1000, 8, 8000) is None
    idx = bench.dump_sample(1001, 8, 8000)
    assert idx.size == 500 and idx.size * (8 + 8) <= 8000
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 1001
    assert np.array_equal(idx, bench.dump_sample(1001, 8, 8000))


def test_dump_outputs_files(tmp_path, monkeypatch):
    import numpy as np
    from acsim.sim import RoundInfo
    info = RoundInfo(25, False, 0.125, -1.5, 2.5, 0)
    x = np.arange(5000, dtype=np.float32) / 3
    rec = bench.dump_outputs(str(tmp_path / "a"), x, info)
    assert rec["files"] == {"values": [5000], "round_info": [6]}
    got = np.load(tmp_path / "a" / "values.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x)
    assert np.load(tmp_path / "a" / "round_info.npy").tolist() == [25.0, 0.0, 0.125, -1.5, 2.5, 0.0]
    # above the size limit: a sample and its node indices, within the limit together
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096 + 12000)
    bench.dump_outputs(str(tmp_path / "b"), x, info)
    idx = np.load(tmp_path / "b" / "values_index.npy")
    assert idx.dtype == np.float64 and idx.size == 1000
    assert np.array_equal(np.load(tmp_path / "b" / "values.npy"), x[idx.astype(np.int64)])
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 4096 + 12000


def test_enter_records_the_stage(monkeypatch):
    monkeypatch.delenv("ACSIM_BENCH_HANG", raising=False)
    ctx = FakeCtx()
    ctx.enter("cfg3_sharded")
    assert ctx.stage == "cfg3_sharded"
