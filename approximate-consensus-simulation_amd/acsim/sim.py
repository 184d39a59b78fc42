"""User-facing API: ``simulate(cfg)`` and ``Simulator(cfg).round(k)``.

Thin ctypes layer over libacsim.so (include/acsim.h).  The per-round hot path runs in the
library's HIP kernels; this module only marshals configs and host buffers.  There is no CPU
fallback: ``backend="cpu"`` is rejected (the CPU spec reference is test infrastructure in
oracle/, not part of the product).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _abi
from .config import Config, preset


@dataclass
class RoundInfo:
    round: int
    done: bool
    spread: float
    lo: float
    hi: float
    instances_done: int


@dataclass
class Result:
    rounds: np.ndarray          # uint32 [B]
    converged: np.ndarray       # bool [B]
    spread: np.ndarray          # float64 [B], final spread per instance
    node_rounds: int
    wall_seconds: float
    rounds_max: int
    x_final: Optional[np.ndarray] = None      # [N] for B == 1, [B, N] otherwise (if requested)
    spread_trace: Optional[np.ndarray] = None  # instance 0, if cfg.trace_spread


class Simulator:
    """One device-resident simulation handle (``acs_sim``)."""

    def __init__(self, cfg: Config | str, device: int = 0, backend: str = "hip",
                 partitions: int = 1, rank: int = 0, comm_id: Optional[bytes] = None,
                 csr=None, weights=None, schedule=None, split=False, transit=None, quant=None):
        """partitions > 1 node-partitions one RANDOM_REGULAR instance: with
        comm_id (RCCL unique id from acsim.distributed) this handle is `rank`'s partition on
        `device`; without it all partitions are simulated on `device` with private x copies
        (validation mode, see include/acsim.h acs_create_partitioned).

        weights = (w_self[N], w_edge[nnz]) with csr and rule="weighted" or rule="pushsum"
        (DESIGN.md §9): receiver i's own entry weighs w_self[i], the message on slot s weighs
        w_edge[s].  For "pushsum" the column sums must not exceed 1 (graphs.pushsum_weights).

        schedule = (period, avail[nnz]) with csr and weights ("Link schedules"): bit p of
        avail[s] is set when the link on slot s is up in every round r with r % period == p; a message on
        a slot that is down is missing exactly as a dropped one.  Push-sum keeps the mean on a schedule
        only with missing_policy="hold" ("omit" loses the mass of every down link).

        split=True with csr and rule="pushsum", and no weights ("Push-sum with per-round
        splitting"): in every round a sender divides its pair over itself and its links that are up
        in that round, so the mean is kept on any schedule with no held state.  Without a schedule
        every link is up in every round (graphs.full_schedule(nnz, 1)).

        transit=D (an integer 0 .. 64) with csr, weights and rule="pushsum" ("Push-sum with
        messages in transit"): a message sent in round r arrives in round r + delta, delta drawn per slot and
        round from 0 .. D, and until then its mass is in transit on the link, so the run still finds the
        mean.  A schedule may be given too.  transit=None (the default) is the handle without delays;
        transit=0 computes the same values through the transit kernels.

        quant=(k, mode, dither) with csr, weights and rule="weighted" ("Quantized messages"):
        every node transmits its state on the grid of step 2**-k (0 <= k <= 52, dtype="f32": 23), rounded
        to nearest (dither false) or up with probability equal to the fractional part (dither true).
        mode "partial": a node averages its own exact state with its neighbours' quantized ones;
        "total": its own quantized state too; "compensated": as "total", then adds its own quantization
        error back, which keeps the mean.  A schedule may be given too; faults and delays are refused."""
        if isinstance(cfg, str):
            cfg = preset(cfg)
        if backend != "hip":
            raise ValueError("acsim implements backend='hip' only; the CPU spec reference is "
                             "test infrastructure (oracle/) and is not a product backend")
        self.cfg = cfg
        self.partitions = int(partitions)
        self._lib = _abi.load_library()
        self._c = cfg.to_c()
        h = C.c_void_p()
        if weights is not None and csr is None:
            raise ValueError("weights need a csr graph")
        if split and weights is not None:
            raise ValueError("split=True computes the shares from the schedule: it takes no weights")
        if split and csr is None:
            raise ValueError("split=True needs a csr graph")
        if schedule is not None and (csr is None or (weights is None and not split)):
            raise ValueError("a link schedule needs a csr graph with weights (rule 'weighted' or 'pushsum')")
        self._transit = None
        if transit is not None:
            if isinstance(transit, bool) or int(transit) != transit:
                raise ValueError("transit must be an integer")
            if csr is None or weights is None:
                raise ValueError("transit needs a csr graph with weights (rule 'pushsum')")
            if split:
                raise ValueError("transit is not served with split=True")
            if not 0 <= int(transit) <= _abi.TRANSIT_MAX:
                raise ValueError(f"transit must be in [0, {_abi.TRANSIT_MAX}]")
            self._transit = int(transit)
        self._quant = None
        if quant is not None:
            from .graphs import quant_args
            if csr is None or weights is None:
                raise ValueError("quant needs a csr graph with weights (rule 'weighted')")
            if split or transit is not None:
                raise ValueError("quant is not served with split=True or transit")
            self._quant = quant_args(quant, cfg.dtype)
        if split:   # rule="pushsum" with per-round splitting (acs_create_csr_split)
            from .graphs import check_schedule, full_schedule
            rp = np.ascontiguousarray(csr[0], dtype=np.uint64)
            ci = np.ascontiguousarray(csr[1], dtype=np.uint32)
            if rp.size != int(cfg.n_nodes) + 1:
                raise ValueError("rowptr must have n_nodes + 1 entries")
            self._nnz = int(ci.size)
            period, av = check_schedule(rp, *(schedule if schedule is not None else full_schedule(ci.size, 1)),
                                        values=False)
            self._period = period
            rc = self._lib.acs_create_csr_split(
                C.byref(self._c), rp.ctypes.data_as(C.POINTER(C.c_uint64)), ci.ctypes.data_as(C.POINTER(C.c_uint32)),
                period, av.ctypes.data_as(C.POINTER(C.c_uint32)), int(device), C.byref(h))
        elif csr is not None and weights is not None:   # rule="weighted" / "pushsum" (acs_create_csr_weighted)
            rp = np.ascontiguousarray(csr[0], dtype=np.uint64)
            ci = np.ascontiguousarray(csr[1], dtype=np.uint32)
            ws = np.ascontiguousarray(weights[0], dtype=np.float64)
            we = np.ascontiguousarray(weights[1], dtype=np.float64)
            if rp.size != int(cfg.n_nodes) + 1:
                raise ValueError("rowptr must have n_nodes + 1 entries")
            if ws.shape != (int(cfg.n_nodes),) or we.shape != ci.shape:
                raise ValueError("weights must be (w_self[n_nodes], w_edge[len(colidx)])")
            self._nnz = int(ci.size)
            dp = C.POINTER(C.c_double)
            if self._quant is not None:   # rule "weighted" with quantized messages (acs_create_csr_quantized)
                period, av = 0, None
                if schedule is not None:
                    from .graphs import check_schedule
                    period, av = check_schedule(rp, schedule[0], schedule[1], values=False)
                rc = self._lib.acs_create_csr_quantized(
                    C.byref(self._c), rp.ctypes.data_as(C.POINTER(C.c_uint64)), ci.ctypes.data_as(C.POINTER(C.c_uint32)),
                    ws.ctypes.data_as(dp), we.ctypes.data_as(dp), period,
                    None if av is None else av.ctypes.data_as(C.POINTER(C.c_uint32)), *self._quant, int(device),
                    C.byref(h))
            elif self._transit is not None:   # push-sum with messages in transit (acs_create_csr_transit)
                period, av = 0, None
                if schedule is not None:
                    from .graphs import check_schedule
                    period, av = check_schedule(rp, schedule[0], schedule[1], values=False)
                rc = self._lib.acs_create_csr_transit(
                    C.byref(self._c), rp.ctypes.data_as(C.POINTER(C.c_uint64)), ci.ctypes.data_as(C.POINTER(C.c_uint32)),
                    ws.ctypes.data_as(dp), we.ctypes.data_as(dp), period,
                    None if av is None else av.ctypes.data_as(C.POINTER(C.c_uint32)), self._transit, int(device),
                    C.byref(h))
            elif schedule is not None:   # acs_create_csr_scheduled checks the period and the masks' bits
                from .graphs import check_schedule
                period, av = check_schedule(rp, schedule[0], schedule[1], values=False)
                rc = self._lib.acs_create_csr_scheduled(
                    C.byref(self._c), rp.ctypes.data_as(C.POINTER(C.c_uint64)), ci.ctypes.data_as(C.POINTER(C.c_uint32)),
                    ws.ctypes.data_as(dp), we.ctypes.data_as(dp), period, av.ctypes.data_as(C.POINTER(C.c_uint32)),
                    int(device), C.byref(h))
            else:
                rc = self._lib.acs_create_csr_weighted(
                    C.byref(self._c), rp.ctypes.data_as(C.POINTER(C.c_uint64)), ci.ctypes.data_as(C.POINTER(C.c_uint32)),
                    ws.ctypes.data_as(dp), we.ctypes.data_as(dp), int(device), C.byref(h))
        elif csr is not None:   # user graph (topology="csr"): csr = (rowptr[N+1], colidx[nnz])
            rp = np.ascontiguousarray(csr[0], dtype=np.uint64)
            ci = np.ascontiguousarray(csr[1], dtype=np.uint32)
            if rp.size != int(cfg.n_nodes) + 1:
                raise ValueError("rowptr must have n_nodes + 1 entries")
            rc = self._lib.acs_create_csr(C.byref(self._c), rp.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          ci.ctypes.data_as(C.POINTER(C.c_uint32)), int(device), C.byref(h))
        elif self.partitions == 1 and comm_id is None:
            devs = (C.c_int * 1)(int(device))
            rc = self._lib.acs_create(C.byref(self._c), _abi.BACKEND_HIP, devs, 1, C.byref(h))
        else:
            idbuf = None if comm_id is None else C.create_string_buffer(bytes(comm_id), len(comm_id))
            rc = self._lib.acs_create_partitioned(C.byref(self._c), int(device), self.partitions,
                                                  int(rank), idbuf, 0 if comm_id is None else len(comm_id),
                                                  C.byref(h))
        _abi.check(self._lib, rc)
        self._h = h

    # -------------------------------------------------------------------------- lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.acs_destroy(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, code: int) -> None:
        _abi.check(self._lib, code)

    @property
    def N(self) -> int:
        return int(self.cfg.n_nodes)

    @property
    def B(self) -> int:
        return int(self.cfg.n_instances)

    # -------------------------------------------------------------------------- stepping
    def round(self, k: int = 1) -> RoundInfo:
        """Advance every unfinished instance by at most k rounds (stops at convergence)."""
        info = _abi.AcsRoundInfo()
        self._chk(self._lib.acs_round(self._h, int(k), C.byref(info)))
        return RoundInfo(info.round, bool(info.done), info.spread, info.lo, info.hi,
                         info.instances_done)

    def run(self) -> _abi.AcsResult:
        res = _abi.AcsResult()
        self._chk(self._lib.acs_run(self._h, C.byref(res)))
        return res

    def sync(self) -> None:
        self._chk(self._lib.acs_sync(self._h))

    # -------------------------------------------------------------------------- state access
    @property
    def value_dtype(self):
        """numpy dtype of node values: float64, or float32 for dtype="f32" (DESIGN.md §9)."""
        return np.float32 if int(self._c.dtype) == _abi.F32 else np.float64

    def values(self, instance: int = 0) -> np.ndarray:
        out = np.empty(self.N, dtype=self.value_dtype)
        self._chk(self._lib.acs_get_values(self._h, int(instance), out.ctypes.data, out.size))
        return out

    def partition_values(self, partition: int) -> np.ndarray:
        """Virtual partitions: the private x copy of one partition."""
        out = np.empty(self.N, dtype=self.value_dtype)
        self._chk(self._lib.acs_get_partition_values(self._h, int(partition), out.ctypes.data, out.size))
        return out

    def all_values(self) -> np.ndarray:
        """[B, N] values of every instance (one ABI call: acs_get_all_values)."""
        out = np.empty((self.B, self.N), dtype=self.value_dtype)
        self._chk(self._lib.acs_get_all_values(self._h, out.ctypes.data, out.size))
        return out

    def rounds(self) -> np.ndarray:
        out = np.empty(self.B, dtype=np.uint32)
        self._chk(self._lib.acs_get_instance_rounds(
            self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out

    def converged(self) -> np.ndarray:
        out = np.empty(self.B, dtype=np.uint8)
        self._chk(self._lib.acs_get_instance_converged(
            self._h, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
        return out.astype(bool)

    def spread(self) -> np.ndarray:
        out = np.empty(self.B, dtype=np.float64)
        self._chk(self._lib.acs_get_instance_spread(
            self._h, out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
        return out

    def spread_trace(self, instance: int = 0) -> np.ndarray:
        n = int(self.cfg.max_rounds) + 1
        out = np.empty(n, dtype=np.float64)
        got = C.c_uint64()
        self._chk(self._lib.acs_get_spread_trace(
            self._h, int(instance), out.ctypes.data_as(C.POINTER(C.c_double)), n, C.byref(got)))
        return out[: got.value].copy()

    def set_state(self, round: int, x: np.ndarray) -> None:
        xv = np.asarray(x)
        if self.value_dtype == np.float32 and xv.dtype != np.float32 and not np.array_equal(
                xv.astype(np.float32).astype(xv.dtype), xv):
            raise ValueError("fp32 set_state: values must be exactly representable in binary32")
        x = np.ascontiguousarray(xv, dtype=self.value_dtype).reshape(-1)
        self._chk(self._lib.acs_set_state(self._h, int(round), x.ctypes.data, x.size))

    def pushsum_state(self, instance: int = 0):
        """(s[N], z[N]) of one instance (rule="pushsum"); values() is s / z."""
        s = np.empty(self.N, dtype=self.value_dtype)
        z = np.empty(self.N, dtype=self.value_dtype)
        self._chk(self._lib.acs_get_pushsum_state(self._h, int(instance), s.ctypes.data, z.ctypes.data, s.size))
        return s, z

    def set_pushsum_state(self, round: int, s: np.ndarray, z: np.ndarray) -> None:
        """Resume a rule="pushsum" handle at `round` with the pairs (s, z), B*N values each
        (instance-major); x becomes s / z where z > 0 and s where z = 0."""
        arrs = []
        for v in (s, z):
            v = np.asarray(v)
            if self.value_dtype == np.float32 and v.dtype != np.float32 and not np.array_equal(
                    v.astype(np.float32).astype(v.dtype), v):
                raise ValueError("fp32 set_pushsum_state: values must be exactly representable in binary32")
            arrs.append(np.ascontiguousarray(v, dtype=self.value_dtype).reshape(-1))
        if arrs[0].size != arrs[1].size:
            raise ValueError("s and z must have the same size")
        self._chk(self._lib.acs_set_pushsum_state(self._h, int(round), arrs[0].ctypes.data, arrs[1].ctypes.data,
                                                  arrs[0].size))

    @property
    def _hold(self) -> bool:
        return int(self._c.rule) == _abi.RULE_PUSHSUM and int(self._c.missing_policy) == _abi.MISSING_HOLD

    def pushsum_links(self, instance: int = 0):
        """(h[nnz], k[nnz]) of one instance in slot order: the mass held on every link
        (rule="pushsum" with missing_policy="hold")."""
        nnz = getattr(self, "_nnz", 0)
        h = np.empty(nnz, dtype=self.value_dtype)
        k = np.empty(nnz, dtype=self.value_dtype)
        self._chk(self._lib.acs_get_pushsum_links(self._h, int(instance), h.ctypes.data, k.ctypes.data, nnz))
        return h, k

    def set_pushsum_links(self, h: np.ndarray, k: np.ndarray) -> None:
        """Set the held mass of every link, B*nnz values each (instance-major, slot order).
        set_state and set_pushsum_state empty the links: a resume with held mass calls this after."""
        arrs = []
        for v in (h, k):
            v = np.asarray(v)
            if self.value_dtype == np.float32 and v.dtype != np.float32 and not np.array_equal(
                    v.astype(np.float32).astype(v.dtype), v):
                raise ValueError("fp32 set_pushsum_links: values must be exactly representable in binary32")
            arrs.append(np.ascontiguousarray(v, dtype=self.value_dtype).reshape(-1))
        if arrs[0].size != arrs[1].size:
            raise ValueError("h and k must have the same size")
        self._chk(self._lib.acs_set_pushsum_links(self._h, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[0].size))

    @property
    def transit_max(self):
        """The transit bound D of a handle made with transit=D, else None."""
        return self._transit

    def pushsum_transit(self, instance: int = 0):
        """(h[D, nnz], k[D, nnz]) of one instance of a handle made with transit=D: plane d
        is what round R + d will deliver on every slot from messages already sent, R the instance's own
        executed rounds."""
        if self._transit is None:
            raise ValueError("pushsum_transit needs a handle made with transit=D")
        D, nnz = self._transit, getattr(self, "_nnz", 0)
        h = np.empty((D, nnz), dtype=self.value_dtype)
        k = np.empty((D, nnz), dtype=self.value_dtype)
        self._chk(self._lib.acs_get_pushsum_transit(self._h, int(instance), h.ctypes.data, k.ctypes.data, h.size))
        return h, k

    def set_pushsum_transit(self, h: np.ndarray, k: np.ndarray) -> None:
        """Set the mass in transit, B*D*nnz values each (instance-major, then plane-major as
        pushsum_transit returns them).  set_state and set_pushsum_state empty the planes: a resume with
        mass in flight calls this after."""
        if self._transit is None:
            raise ValueError("set_pushsum_transit needs a handle made with transit=D")
        arrs = []
        for v in (h, k):
            v = np.asarray(v)
            if self.value_dtype == np.float32 and v.dtype != np.float32 and not np.array_equal(
                    v.astype(np.float32).astype(v.dtype), v):
                raise ValueError("fp32 set_pushsum_transit: values must be exactly representable in binary32")
            arrs.append(np.ascontiguousarray(v, dtype=self.value_dtype).reshape(-1))
        if arrs[0].size != arrs[1].size:
            raise ValueError("h and k must have the same size")
        self._chk(self._lib.acs_set_pushsum_transit(self._h, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[0].size))

    def pushsum_mass(self, instance: int = 0):
        """(fsum(s) + fsum(h), fsum(z) + fsum(k)) of one instance as Python floats: the mass on the
        nodes plus the mass held on the links (missing_policy="hold") or in transit (transit=D);
        without either the node sums alone.  With column sums of 1 and no loss the second member
        stays N under "hold" and with transit."""
        s, z = self.pushsum_state(instance)
        ms, mz = math.fsum(s.tolist()), math.fsum(z.tolist())
        if self._hold:
            h, k = self.pushsum_links(instance)
            ms, mz = ms + math.fsum(h.tolist()), mz + math.fsum(k.tolist())
        if self._transit:
            h, k = self.pushsum_transit(instance)
            ms, mz = ms + math.fsum(h.reshape(-1).tolist()), mz + math.fsum(k.reshape(-1).tolist())
        return ms, mz

    def fault_status(self) -> np.ndarray:
        out = np.empty(self.B * self.N, dtype=np.uint32)
        self._chk(self._lib.acs_get_fault_status(
            self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out.reshape(self.B, self.N)

    def weights(self):
        """(w_self[N], w_edge[nnz]) as the device holds them (rule="weighted" / "pushsum"; with dtype="f32" the
        weights rounded to binary32, returned as float64)."""
        ws = np.empty(self.N, dtype=np.float64)
        we = np.empty(getattr(self, "_nnz", 0), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self._lib.acs_get_weights(self._h, ws.ctypes.data_as(dp), ws.size, we.ctypes.data_as(dp), we.size))
        return ws, we

    def link_schedule(self):
        """(period, avail[nnz] uint32 in slot order) of a handle made with schedule=...."""
        period = C.c_uint32()
        av = np.empty(getattr(self, "_nnz", 0), dtype=np.uint32)
        self._chk(self._lib.acs_get_link_schedule(self._h, C.byref(period), av.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                  av.size))
        return int(period.value), av

    def split_shares(self) -> np.ndarray:
        """[period, N] shares of a handle made with split=True as the device holds them (dtype="f32":
        widened to float64): share[p, j] is what node j keeps, and sends on each link that is up, in
        the rounds r with r % period == p."""
        out = np.empty((getattr(self, "_period", 1), self.N), dtype=np.float64)
        self._chk(self._lib.acs_get_split_shares(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
        return out

    def quantized(self, instance: int = 0) -> np.ndarray:
        """[N] what the nodes of one instance of a handle made with quant=... transmit in its next round
        R (its executed rounds): Q(x^R), in the config dtype."""
        if self._quant is None:
            raise ValueError("quantized needs a handle made with quant=(k, mode, dither)")
        out = np.empty(self.N, dtype=self.value_dtype)
        self._chk(self._lib.acs_get_quantized(self._h, int(instance), out.ctypes.data, out.size))
        return out

    def neighbors(self) -> np.ndarray:
        d = int(self.cfg.degree)
        out = np.empty(self.N * d, dtype=np.uint32)
        self._chk(self._lib.acs_get_neighbors(
            self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out.reshape(self.N, d)

    # -------------------------------------------------------------------------- measurement
    def set_kernel_timing(self, enable, every: int = 1, runs: bool = False) -> None:
        """Bracket round-kernel launches with HIP events: every `every`-th round when enabled, or
        with runs=True one event pair around each run of `every` consecutive rounds (no idle gap
        inside the run; every round counts as one launch)."""
        k = max(1, int(every)) if enable else 0
        self._chk(self._lib.acs_set_kernel_timing(self._h, -k if runs else k))

    def kernel_timing(self):
        """(total_ms, launches, kernel_name) of the round kernel since timing was enabled."""
        ms = C.c_double()
        n = C.c_uint64()
        name = C.create_string_buffer(256)
        self._chk(self._lib.acs_get_kernel_timing(self._h, C.byref(ms), C.byref(n), name, 256))
        return ms.value, n.value, name.value.decode()

    def kernel_name(self) -> str:
        """Name of the round kernel(s) this handle's path launches."""
        return self.kernel_timing()[2]


def simulate(cfg: Config | str, backend: str = "hip", device: int = 0,
             devices: Optional[Sequence[int]] = None, return_values: bool = True,
             csr=None, weights=None, schedule=None, split=False, transit=None, quant=None) -> Result:
    """Run one configuration to termination and return its results."""
    if devices is not None:
        devices = list(devices)
        if len(devices) != 1:
            raise ValueError("simulate() drives one device per process; shard instances across "
                             "processes with acsim.distributed (one rank per GPU)")
        device = devices[0]
    with Simulator(cfg, device=device, backend=backend, csr=csr, weights=weights, schedule=schedule,
                   split=split, transit=transit, quant=quant) as sim:
        res = sim.run()
        x = None
        if return_values:
            x = sim.values(0) if sim.B == 1 else sim.all_values()
        trace = sim.spread_trace(0) if sim.cfg.trace_spread else None
        return Result(rounds=sim.rounds(), converged=sim.converged(), spread=sim.spread(),
                      node_rounds=int(res.node_rounds), wall_seconds=float(res.wall_seconds),
                      rounds_max=int(res.rounds_max), x_final=x, spread_trace=trace)
