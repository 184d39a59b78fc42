"""Command line: ``python -m acsim {presets,validate,run,sweep}`` (SURVEY §5 config/flags).

  python -m acsim presets
  python -m acsim validate --preset cfg4 --set n_nodes=4096
  python -m acsim run --preset cfg4_eps --out result.npz [--device 0] [--set key=value ...]
  python -m acsim sweep --preset cfg3 --set n_instances=1000 --grid loss_p=0.1,0.2 --out runs/
  python -m acsim run --preset cfg4 --graph my_graph.npz --set trim=2 ...   (user CSR graph,
      acsim or scipy.sparse .npz layout; topology and n_nodes come from the file)
  python -m acsim run --graph weighted.npz --set rule=weighted ...   (the file's weights too)
  python -m acsim run --graph directed.npz --set rule=pushsum ...   (the file's weights when it has
      them, else graphs.pushsum_weights; the choice is reported on stderr)
  python -m acsim run --graph directed.npz --set rule=pushsum --set loss_p=0.2 --set missing_policy=hold
      (push-sum under message loss: "hold" keeps a dropped message's mass on its link, so the mean of
      x^0 is still found; "omit" loses the mass and ends away from it)
  python -m acsim run --graph scheduled.npz --set rule=pushsum --set missing_policy=hold
      (a file with a link schedule, graphs.save_csr(..., schedule=...): rules weighted and pushsum run
      on it, reported on stderr; push-sum keeps the mean on a schedule under "hold" only)
  python -m acsim run --graph g.npz --set rule=pushsum --transit 3
      (push-sum with messages in transit for up to 3 rounds, DESIGN.md §9, on the file's weights and link
      schedule, reported on stderr)
  python -m acsim run --graph scheduled.npz --set rule=pushsum --split
      (push-sum with per-round splitting on the file's schedule, DESIGN.md §9: no weights, no held
      state, and the mean is kept; reported on stderr)
  python -m acsim run --graph g.npz --set rule=weighted --quant 8 --quant-mode compensated --quant-dither
      (rule weighted with quantized messages, DESIGN.md §9: every node transmits its state on the grid
      of step 2**-8; reported on stderr)
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import sys

import numpy as np

from . import _abi
from .config import PRESETS, Config, preset


def _coerce(field: str, text: str):
    ftype = {f.name: f.type for f in dataclasses.fields(Config)}[field]
    if ftype in ("int", int):
        return int(text, 0)
    if ftype in ("float", float):
        return float(text)
    if ftype in ("bool", bool):
        return text.lower() in ("1", "true", "yes", "on")
    return text   # enum names (strings) or ints given as text are both accepted by Config


def _apply(cfg: Config, sets):
    over = {}
    for s in sets or []:
        k, _, v = s.partition("=")
        if k not in {f.name for f in dataclasses.fields(Config)}:
            raise SystemExit(f"unknown config field {k!r}")
        over[k] = _coerce(k, v)
    return cfg.replace(**over)


def _grid(specs):
    grid = {}
    for s in specs or []:
        k, _, v = s.partition("=")
        grid[k] = [_coerce(k, t) for t in v.split(",")]
    return grid


def validate(cfg: Config, csr=None, weights=None, schedule=None, split=False, transit=None, quant=None) -> int:
    """Host-side §A.8 validation through the library (no GPU needed: acs_create validates first)."""
    lib = _abi.load_library()
    c = cfg.to_c()
    h = C.c_void_p()
    if split:
        from .graphs import full_schedule
        rp, ci = csr
        period, av = schedule if schedule is not None else full_schedule(ci.size, 1)
        av = np.ascontiguousarray(av, dtype=np.uint32)
        rc = lib.acs_create_csr_split(C.byref(c), rp.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      ci.ctypes.data_as(C.POINTER(C.c_uint32)), int(period),
                                      av.ctypes.data_as(C.POINTER(C.c_uint32)), 0, C.byref(h))
    elif csr is not None and weights is not None and quant is not None:
        from .graphs import quant_args
        rp, ci = np.ascontiguousarray(csr[0], dtype=np.uint64), np.ascontiguousarray(csr[1], dtype=np.uint32)
        ws, we = (np.ascontiguousarray(w, dtype=np.float64) for w in weights)
        av = None if schedule is None else np.ascontiguousarray(schedule[1], dtype=np.uint32)
        dp = C.POINTER(C.c_double)
        rc = lib.acs_create_csr_quantized(C.byref(c), rp.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          ci.ctypes.data_as(C.POINTER(C.c_uint32)), ws.ctypes.data_as(dp),
                                          we.ctypes.data_as(dp), 0 if schedule is None else int(schedule[0]),
                                          None if av is None else av.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          *quant_args(quant, cfg.dtype), 0, C.byref(h))
    elif csr is not None and weights is not None and transit is not None:
        rp, ci = np.ascontiguousarray(csr[0], dtype=np.uint64), np.ascontiguousarray(csr[1], dtype=np.uint32)
        ws, we = (np.ascontiguousarray(w, dtype=np.float64) for w in weights)
        av = None if schedule is None else np.ascontiguousarray(schedule[1], dtype=np.uint32)
        dp = C.POINTER(C.c_double)
        rc = lib.acs_create_csr_transit(C.byref(c), rp.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        ci.ctypes.data_as(C.POINTER(C.c_uint32)), ws.ctypes.data_as(dp),
                                        we.ctypes.data_as(dp), 0 if schedule is None else int(schedule[0]),
                                        None if av is None else av.ctypes.data_as(C.POINTER(C.c_uint32)), int(transit),
                                        0, C.byref(h))
    elif csr is not None and weights is not None and schedule is not None:
        rp, ci = csr
        ws, we = (np.ascontiguousarray(w, dtype=np.float64) for w in weights)
        av = np.ascontiguousarray(schedule[1], dtype=np.uint32)
        dp = C.POINTER(C.c_double)
        rc = lib.acs_create_csr_scheduled(C.byref(c), rp.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          ci.ctypes.data_as(C.POINTER(C.c_uint32)), ws.ctypes.data_as(dp),
                                          we.ctypes.data_as(dp), int(schedule[0]),
                                          av.ctypes.data_as(C.POINTER(C.c_uint32)), 0, C.byref(h))
    elif csr is not None and weights is not None:
        rp, ci = csr
        ws, we = (np.ascontiguousarray(w, dtype=np.float64) for w in weights)
        dp = C.POINTER(C.c_double)
        rc = lib.acs_create_csr_weighted(C.byref(c), rp.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         ci.ctypes.data_as(C.POINTER(C.c_uint32)), ws.ctypes.data_as(dp),
                                         we.ctypes.data_as(dp), 0, C.byref(h))
    elif csr is not None:
        rp, ci = csr
        rc = lib.acs_create_csr(C.byref(c), rp.ctypes.data_as(C.POINTER(C.c_uint64)),
                                ci.ctypes.data_as(C.POINTER(C.c_uint32)), 0, C.byref(h))
    else:
        rc = lib.acs_create(C.byref(c), _abi.BACKEND_HIP, (C.c_int * 1)(0), 1, C.byref(h))
    if rc == _abi.OK:
        lib.acs_destroy(h)
        return 0
    msg = lib.acs_last_error().decode()
    if rc == _abi.EDEVICE and "no HIP device" in msg:
        return 0   # the config is valid; there is just no GPU here
    print(f"invalid: {_abi.STATUS_NAMES.get(rc, rc)}: {msg}", file=sys.stderr)
    return 1


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="acsim")
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("presets")
    for name in ("validate", "run", "sweep"):
        p = sub.add_parser(name)
        p.add_argument("--preset", default="cfg1", choices=sorted(PRESETS))
        p.add_argument("--set", action="append", metavar="FIELD=VALUE")
        p.add_argument("--device", type=int, default=0)
        p.add_argument("--graph", metavar="FILE.npz", help="user CSR graph (acsim.graphs.load_csr)")
        p.add_argument("--split", action="store_true",
                       help="rule pushsum with per-round splitting on the graph file's link schedule (no weights)")
        p.add_argument("--transit", type=int, metavar="D",
                       help="rule pushsum with messages in transit for up to D rounds (0 .. 64), on the graph file's "
                            "weights and link schedule")
        p.add_argument("--quant", type=int, metavar="K",
                       help="rule weighted with quantized messages: every node transmits its state on the grid of "
                            "step 2**-K (0 .. 52, dtype f32: 0 .. 23)")
        p.add_argument("--quant-mode", choices=sorted(_abi.QUANT_MODES), default=None,
                       help="with --quant: what a node averages its neighbours' quantized states with (default partial)")
        p.add_argument("--quant-dither", action="store_true",
                       help="with --quant: round up with probability equal to the fractional part, not to nearest")
        if name in ("run", "sweep"):
            p.add_argument("--out")
        if name == "sweep":
            p.add_argument("--grid", action="append", metavar="FIELD=V1,V2,...", required=True)
    a = ap.parse_args(argv)
    if a.cmd == "presets":
        for k, v in PRESETS.items():
            print(k, json.dumps(dataclasses.asdict(v)))
        return 0
    cfg = _apply(preset(a.preset), a.set)
    csr = weights = schedule = None
    if a.split and not a.graph:
        ap.error("--split needs --graph")
    if a.transit is not None:
        if not a.graph:
            ap.error("--transit needs --graph")
        if a.split:
            ap.error("--transit is not served with --split")
        if not 0 <= a.transit <= _abi.TRANSIT_MAX:
            ap.error(f"--transit must be in 0 .. {_abi.TRANSIT_MAX}")
    quant = None
    if a.quant is None and (a.quant_mode is not None or a.quant_dither):
        ap.error("--quant-mode and --quant-dither need --quant")
    if a.quant is not None:
        from .config import _enum
        from .graphs import quant_args
        if not a.graph:
            ap.error("--quant needs --graph")
        if a.split or a.transit is not None:
            ap.error("--quant is not served with --split or --transit")
        if _enum("rule", cfg.rule) != _abi.RULE_WEIGHTED:
            ap.error("--quant needs --set rule=weighted")
        quant = (a.quant, a.quant_mode or "partial", bool(a.quant_dither))
        try:
            quant_args(quant, cfg.dtype)
        except ValueError as e:
            ap.error(str(e))
        print(f"weighted: quantized messages, step 2**-{quant[0]}, mode {quant[1]}, "
              f"{'dithered' if quant[2] else 'rounded to nearest'}", file=sys.stderr)
    if a.graph:
        from .config import _enum
        from .graphs import load_csr
        if a.split:   # shares from the schedule: the file's weights are not read
            if _enum("rule", cfg.rule) != _abi.RULE_PUSHSUM:
                ap.error("--split needs --set rule=pushsum")
            csr = load_csr(a.graph)
            try:
                schedule = load_csr(a.graph, schedule=True)[2:]
                print(f"pushsum --split: using the link schedule of {a.graph} (period {schedule[0]}); every sender "
                      "splits over the links up in each round", file=sys.stderr)
            except ValueError as e:
                if "no link schedule" not in str(e):
                    raise
                print(f"pushsum --split: {a.graph} has no link schedule, every link is up in every round",
                      file=sys.stderr)
        elif _enum("rule", cfg.rule) == _abi.RULE_WEIGHTED:   # the file's weights go with the rule
            g = load_csr(a.graph, weights=True)
            csr, weights = g[:2], g[2:]
        elif _enum("rule", cfg.rule) == _abi.RULE_PUSHSUM:   # the file's weights, else 1 / (outdeg + 1)
            from .graphs import pushsum_weights
            try:
                g = load_csr(a.graph, weights=True)
                csr, weights = g[:2], g[2:]
                print(f"pushsum: using the weights of {a.graph}", file=sys.stderr)
            except ValueError as e:
                if "no weights" not in str(e):
                    raise
                csr = load_csr(a.graph)
                weights = pushsum_weights(*csr, dtype=cfg.dtype)
                print(f"pushsum: {a.graph} has no weights, using graphs.pushsum_weights (1 / (outdeg + 1))",
                      file=sys.stderr)
        else:
            csr = load_csr(a.graph)
        if weights is not None:   # rules weighted and pushsum: the file's link schedule, when it has one
            try:
                schedule = load_csr(a.graph, schedule=True)[2:]
                print(f"{cfg.rule}: using the link schedule of {a.graph} (period {schedule[0]})", file=sys.stderr)
            except ValueError as e:
                if "no link schedule" not in str(e):
                    raise
                if a.transit is not None:
                    print(f"pushsum: {a.graph} has no link schedule, every link is up in every round", file=sys.stderr)
        if a.transit is not None:
            if _enum("rule", cfg.rule) != _abi.RULE_PUSHSUM:
                ap.error("--transit needs --set rule=pushsum")
            print(f"pushsum: transit {a.transit}: a message arrives up to {a.transit} rounds after it is sent, its mass "
                  "in transit until then", file=sys.stderr)
        cfg = cfg.replace(topology="csr", n_nodes=int(csr[0].size - 1))
    if a.cmd == "validate":
        rc = validate(cfg, csr, weights, schedule, split=a.split, transit=a.transit, quant=quant)
        if rc == 0:
            print("ok")
        return rc
    if a.cmd == "run":
        from .io import save_result
        from .sim import simulate
        res = simulate(cfg, device=a.device, return_values=bool(a.out), csr=csr, weights=weights, schedule=schedule,
                       split=a.split, transit=a.transit, quant=quant)
        from .sweep import summarize
        print(json.dumps(summarize(cfg, res)))
        if a.out:
            save_result(a.out, res, cfg)
        return 0
    from .sweep import sweep
    rows = sweep(cfg, _grid(a.grid), out_dir=a.out, device=a.device, csr=csr, weights=weights, schedule=schedule,
                 split=a.split, transit=a.transit, quant=quant)
    for r in rows:
        print(json.dumps(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
