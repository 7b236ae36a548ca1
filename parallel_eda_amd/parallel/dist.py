"""Multi-GPU (and multi-process CPU) distributed routing.

Replaces the reference's MPI net-partitioned PathFinder
(mpi_route_load_balanced_nonblocking_send_recv_encoded.cxx:402) with the
MI355X-native model from SURVEY.md section 5.8: one process per GPU over
RCCL/xGMI ("nccl" backend; "gloo" for CPU tests), every rank holding the
FULL rr graph + congestion, nets partitioned SPATIALLY (region cuts = GPU
boundaries), and one integer occ all-reduce per PathFinder iteration in
place of the reference's per-net broadcast stream. STA is replicated per
rank (removes the reference's root-Scatterv serialization, A:1473-1496).

Integer occ deltas + fixed wave schedules make the whole distributed
iteration DETERMINISTIC (integer sums are order-independent).
"""
import os

import numpy as np


def _dist():
    import torch.distributed as dist
    return dist


def init_dist():
    """Initialize torch.distributed from torchrun env; no-op if WORLD_SIZE<=1.

    Returns (rank, world_size, local_rank)."""
    import torch
    dist = _dist()
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.is_available():
        # RCCL needs one DISTINCT device per rank; when ranks outnumber
        # GPUs (hardware testing of the multi-rank drivers on a 1-GPU
        # box) fall back to gloo with CPU-staged collectives and share
        # device 0. PNR_DIST_BACKEND overrides.
        ndev = torch.cuda.device_count()
        local = local % max(1, ndev)
        backend = "nccl" if ws <= ndev else "gloo"
    else:
        backend = "gloo"
    backend = os.environ.get("PNR_DIST_BACKEND", backend)
    if ws > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        dist.init_process_group(backend=backend, rank=rank, world_size=ws)
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
    return rank, ws, local


def allreduce_(t, op=None):
    """all_reduce that works for every (backend, tensor-device) pair:
    nccl(=RCCL) takes the device tensor directly; gloo stages a CUDA
    tensor through CPU (the 1-GPU multi-rank hardware-test path).
    In-place; returns t."""
    dist = _dist()
    if op is None:
        op = dist.ReduceOp.SUM
    if t.is_cuda and dist.get_backend() != "nccl":
        c = t.cpu()
        dist.all_reduce(c, op=op)
        t.copy_(c)
    else:
        dist.all_reduce(t, op=op)
    return t


def spatial_partition(bb, world_size, weight=None):
    """Assign nets to ranks by RECURSIVE WEIGHTED BISECTION of bb
    centers (the reference's region tree: fpga_bipartition /
    build_net_tree, partitioning_multi_sink...cxx:3064,3295) — each
    level splits the heavier child count along its WIDER axis, so 8
    ranks get a 2-D tiling instead of 8 thin strips (half the cut
    boundary, fewer cross-rank congestion conflicts). Balanced by
    estimated route cost (reference's measured-time load balancing,
    mpi_route...cxx:249, approximated by nsinks x bb semiperimeter until
    measured times land). Deterministic pure-numpy: every rank computes
    the identical partition. Returns rank_of_net (int array)."""
    n = len(bb)
    rank_of = np.zeros(n, dtype=np.int32)
    if world_size <= 1 or n == 0:
        return rank_of
    cx = (bb[:, 0].astype(np.int64) + bb[:, 2].astype(np.int64))
    cy = (bb[:, 1].astype(np.int64) + bb[:, 3].astype(np.int64))
    w = (np.ones(n, dtype=np.float64) if weight is None
         else np.asarray(weight, dtype=np.float64))

    def split(ids, k, r0):
        if k == 1 or len(ids) == 0:
            rank_of[ids] = r0
            return
        k_lo = k // 2
        # split along the wider axis of this region's bb-center extent
        ex = int(cx[ids].max() - cx[ids].min()) if len(ids) else 0
        ey = int(cy[ids].max() - cy[ids].min()) if len(ids) else 0
        key = cx[ids] if ex >= ey else cy[ids]
        order = ids[np.argsort(key, kind="stable")]
        cum = np.cumsum(w[order])
        total = cum[-1]
        # cut minimizing |left weight - fair share|
        cut = int(np.argmin(np.abs(cum - total * k_lo / k))) + 1
        cut = min(max(cut, 0), len(order))
        split(order[:cut], k_lo, r0)
        split(order[cut:], k - k_lo, r0 + k_lo)

    split(np.arange(n, dtype=np.int64), world_size, 0)
    return rank_of


class CpuEngine:
    """SerialRouter adapter for DistRouteLoop (gloo CPU testing path)."""

    def __init__(self, router, num_nodes):
        self.r = router
        self.num_nodes = num_nodes

    def route_subset(self, crit, pres_fac, net_ids, partial=False,
                     force_waves=False, device_timing=False):
        if device_timing:
            raise ValueError("device_timing needs the GPU engine: CpuEngine "
                             "routes on the host (use timing.sta.STA)")
        import numpy as _np
        self.r.set_pres_fac(pres_fac)
        # refresh pres array from occ under the new pres_fac
        self.r.set_occ(_np.asarray(self.r.occ()))
        c = np.ascontiguousarray(crit, dtype=np.float32)
        ids = np.asarray(net_ids, dtype=np.int32)
        if partial:
            self.r.route_subset_incremental(c, ids)
        else:
            self.r.route_subset(c, ids)

    def rip_up_nets(self, net_ids):
        self.r.rip_up_nets(np.asarray(net_ids, dtype=np.int32))

    def net_costs(self, num_nets, my_nets):
        return None  # no per-net measurement on the CPU oracle

    def occ_tensor(self):
        import torch
        return torch.from_numpy(np.asarray(self.r.occ()).copy())

    def set_occ(self, t):
        self.r.set_occ(t.cpu().numpy())

    def sink_delays_local(self, net_ids, device_timing=False):
        if device_timing:
            raise ValueError("device_timing needs the GPU engine")
        return np.asarray(self.r.sink_delays())

    def update_acc(self, acc_fac):
        # acc only; pres is refreshed at the next route_subset
        self.r.update_costs(self.r_pres_fac if hasattr(self, "r_pres_fac") else 0.0,
                            acc_fac)

    def num_overused(self):
        return int(self.r.count_overused())

    def congested_nets(self):
        return np.asarray(self.r.congested_nets())

    def incomplete_nets(self):
        return np.asarray(self.r.incomplete_nets())


class GpuEngine:
    """GpuRouter adapter for DistRouteLoop."""

    def __init__(self, router):
        self.g = router
        self._last_sd = np.zeros(router.n_sinks, dtype=np.float32)

    def route_subset(self, crit, pres_fac, net_ids, partial=False,
                     force_waves=False, device_timing=False):
        """device_timing: crit may be a device tensor, and the sink delays
        stay on the device (sink_delays_local(device_timing=True))."""
        _, sd = self.g.route_iteration(crit, pres_fac, net_subset=net_ids,
                                       fail_ok=True, partial=partial,
                                       force_waves=force_waves,
                                       device_delays=device_timing)
        if not device_timing:
            self._last_sd = sd

    def occ_tensor(self):
        return self.g.t_occ

    def set_occ(self, t):
        self.g.t_occ.copy_(t)

    def sink_delays_local(self, net_ids, device_timing=False):
        if device_timing:
            # the router's live buffer: current whether or not this rank
            # routed anything this iteration
            return self.g.t_sink_delay
        return self._last_sd

    def rip_up_nets(self, net_ids):
        self.g.rip_up_nets(net_ids)

    def net_costs(self, num_nets, my_nets):
        # measured per-net search cost from the last iteration's counters
        w = self.g.t_net_scans.cpu().numpy().astype(np.float64)
        mask = np.zeros(num_nets, dtype=bool)
        mask[my_nets] = True
        return np.where(mask, w, 0.0)

    def update_acc(self, acc_fac):
        self.g.update_acc(acc_fac)

    def num_overused(self):
        import torch
        return int((self.g.t_occ > self.g.t_cap.to(torch.int32)).sum().item())

    def congested_nets(self):
        return np.asarray(self.g.congested_nets())

    def incomplete_nets(self):
        """Nets with unreached sinks, tracked by the router across
        iterations (retry exhaustion under fail_ok, or rip-up without
        reroute). ADVICE r1: without this the distributed flow could
        report success with stranded connections."""
        return self.g.incomplete_nets()


class DistRouteLoop:
    """Distributed PathFinder outer loop over an engine.

    The engine abstracts CPU-oracle vs GPU-kernel routing:
      engine.route_subset(crit, pres_fac, net_ids) -> None
      engine.occ_tensor() -> torch int32 tensor (device or cpu)
      engine.set_occ(tensor) -> None
      engine.sink_delays_local(net_ids) -> np.float32 aligned with sinks
      engine.update_acc(acc_fac)
      engine.num_overused() -> int   (from its occ)
    """

    def __init__(self, engine, num_nets, bb, n_rsinks, sink_ptr,
                 rank=0, world_size=1):
        self.engine = engine
        self.rank = rank
        self.ws = world_size
        if world_size > 1:
            nsk = np.diff(np.asarray(sink_ptr))
            semi = ((bb[:, 2] - bb[:, 0]).astype(np.int64) +
                    (bb[:, 3] - bb[:, 1]).astype(np.int64) + 2)
            self.rank_of = spatial_partition(bb, world_size,
                                             weight=nsk * semi)
        else:
            self.rank_of = np.zeros(num_nets, dtype=np.int32)
        self.my_nets = np.nonzero(self.rank_of == rank)[0]
        self._bb = bb
        self._sink_ptr = np.asarray(sink_ptr)
        # sinks owned by my nets
        mask = np.zeros(n_rsinks, dtype=bool)
        for n in self.my_nets:
            mask[sink_ptr[n]:sink_ptr[n + 1]] = True
        self.my_sink_mask = mask

    def _refresh_sink_mask(self):
        mask = np.zeros(len(self.my_sink_mask), dtype=bool)
        for n in self.my_nets:
            mask[self._sink_ptr[n]:self._sink_ptr[n + 1]] = True
        self.my_sink_mask = mask

    def set_partition(self, new_rank):
        """Migrate net ownership to `new_rank` (identical on every rank).
        Nets that change owner are ripped up by the OLD owner and the occ
        deltas all-reduced (the replicated-graph analogue of the
        reference's move_route_tree, mpi_route...cxx:172: the new owner
        simply reroutes from scratch). Returns nets this rank lost+gained."""
        dist = _dist()
        old_mine = set(self.my_nets.tolist())
        new_mine = set(np.nonzero(new_rank == self.rank)[0].tolist())
        lost = sorted(old_mine - new_mine)
        gained = sorted(new_mine - old_mine)
        occ_before = self.engine.occ_tensor().clone()
        if lost:
            self.engine.rip_up_nets(np.asarray(lost, dtype=np.int64))
        occ = self.engine.occ_tensor()
        delta = occ - occ_before
        allreduce_(delta)
        self.engine.set_occ(occ_before + delta)
        self.rank_of = np.asarray(new_rank, dtype=np.int32)
        self.my_nets = np.nonzero(self.rank_of == self.rank)[0]
        self._refresh_sink_mask()
        return len(lost) + len(gained)

    def rebalance(self, weights=None):
        """Repartition nets by measured per-net route cost (reference:
        load-balanced repartition, mpi_route...cxx:249). weights: per-net
        cost with valid entries for OWNED nets (zeros elsewhere); summed
        across ranks so every rank computes the identical new partition.
        Returns the number of nets this rank lost+gained."""
        if self.ws <= 1:
            return 0
        import torch
        dist = _dist()
        if weights is None:
            weights = self.engine.net_costs(len(self.rank_of), self.my_nets)
        if weights is None:
            return 0
        w = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64))
        occ_dev = self.engine.occ_tensor().device
        if occ_dev.type == "cuda":
            w = w.to(occ_dev)
        allreduce_(w)
        wsum = np.maximum(w.cpu().numpy(), 1.0)
        new_rank = spatial_partition(self._bb, self.ws, weight=wsum)
        return self.set_partition(new_rank)

    def _global_owned_mask(self, ids):
        """Union of per-rank OWNED net id sets into a rank-identical
        boolean mask (max all-reduce)."""
        import torch
        mask = np.zeros(len(self.rank_of), dtype=np.float32)
        local = np.intersect1d(np.asarray(ids, dtype=np.int64),
                               self.my_nets)
        mask[local] = 1.0
        if self.ws > 1:
            t = torch.from_numpy(mask)
            occ_dev = self.engine.occ_tensor().device
            if occ_dev.type == "cuda":
                t = t.to(occ_dev)
            allreduce_(t, op=_dist().ReduceOp.MAX)
            mask = t.cpu().numpy()
        return mask > 0.5

    def global_congested_mask(self):
        """Boolean mask over nets whose tree crosses an overused node —
        identical on every rank (each rank reports its OWNED nets, then a
        max all-reduce unions them). Reference: phase-two congested-net
        selection, here made globally consistent for the shrink decision.
        Nets with missing sinks (never routed / partial-ripped) are
        included so selective reroute can never strand a connection."""
        m = self._global_owned_mask(self.engine.congested_nets())
        # UNCONDITIONAL second union: the incomplete set is rank-LOCAL,
        # so gating the collective on len(inc) desynchronizes ranks (one
        # all-reduces, the other doesn't — gloo aborts with a size
        # mismatch; found by tools/soak.py dist fuzzing, seed 90006).
        m |= self._global_owned_mask(self.engine.incomplete_nets())
        return m

    def shrink_active(self, active_mask, k=1):
        """Elastic comm-shrink analogue (reference: mpi_comm_shrink — the
        MPI router drops to fewer ranks when the contested endgame no
        longer fills the machine). Consolidates the ACTIVE nets onto the
        first k ranks; frozen nets keep their owners (their trees never
        move). After this, call iteration(..., active_mask=...) so idle
        ranks route nothing but still join the (cheap) collectives.
        Returns nets moved by this rank."""
        if self.ws <= 1:
            return 0
        active = np.nonzero(active_mask)[0]
        new_rank = self.rank_of.copy()
        if len(active):
            nsk = np.diff(self._sink_ptr)[active]
            semi = ((self._bb[active, 2] - self._bb[active, 0]).astype(np.int64)
                    + (self._bb[active, 3] - self._bb[active, 1]).astype(np.int64)
                    + 2)
            new_rank[active] = spatial_partition(self._bb[active], k,
                                                 weight=nsk * semi)
        return self.set_partition(new_rank)

    def iteration(self, crit, pres_fac, acc_fac, active_mask=None,
                  partial=False, force_waves=False, device_timing=False):
        """One distributed PathFinder iteration. active_mask: optional
        bool mask over nets (selective reroute); only owned ACTIVE nets
        are routed, but every rank joins the collectives. partial:
        partial rip-up on the engine (keep clean subtrees). Returns
        (overused_global, sink_delays_global).
        device_timing (GPU engine): crit may be a device tensor, and with
        one rank the returned delays are the router's device buffer; with
        more ranks they go through the same host-staged all-reduce as
        ever and come back as numpy."""
        import torch
        dist = _dist() if self.ws > 1 else None
        eng = self.engine
        nets = self.my_nets
        if active_mask is not None:
            nets = nets[np.asarray(active_mask)[nets]]
        if self.ws > 1:
            occ_before = eng.occ_tensor().clone()
        if len(nets) and device_timing:
            eng.route_subset(crit, pres_fac, nets, partial=partial,
                             force_waves=force_waves, device_timing=True)
        elif len(nets):
            eng.route_subset(crit, pres_fac, nets, partial=partial,
                             force_waves=force_waves)
        if device_timing:
            sd = eng.sink_delays_local(self.my_nets, device_timing=True)
            if self.ws > 1:
                sd = sd.cpu().numpy()
        else:
            sd = eng.sink_delays_local(self.my_nets)
        if self.ws > 1:
            occ = eng.occ_tensor()
            delta = occ - occ_before
            allreduce_(delta)
            occ_new = occ_before + delta
            eng.set_occ(occ_new)
            # sink delays: mask to my sinks, sum across ranks
            sd_t = torch.from_numpy(np.where(self.my_sink_mask, sd, 0.0)
                                    .astype(np.float32))
            if occ.is_cuda:
                sd_t = sd_t.to(occ.device)
            allreduce_(sd_t)
            sd = sd_t.cpu().numpy()
        over = eng.num_overused()
        eng.update_acc(acc_fac)
        return over, sd


def pathfinder_route_dist(loop, cmap, sta, max_iters=60, pres_fac_init=0.5,
                          pres_fac_mult=1.3, acc_fac=1.0,
                          shrink_threshold=128, verbose=False,
                          incremental=False, intra_delay=0.0,
                          device_timing=None):
    """Distributed PathFinder outer loop (flow-level driver).

    Mirrors route.gpu_router.pathfinder_route_gpu's schedule — iteration 1
    routes everything congestion-blind, later iterations re-route only the
    congested nets (reference: build_phase_two) — with the distributed
    twists from SURVEY §5.8: occ/delay all-reduce every iteration (inside
    loop.iteration) and the elastic comm-shrink analogue: once the active
    set drops below shrink_threshold nets, the endgame consolidates onto
    rank 0 (reference: mpi_comm_shrink) so the contested tail is routed by
    one engine with bb-disjoint wave scheduling instead of oscillating
    across ranks.

    loop: DistRouteLoop; cmap: route.router.ConnMap; sta: timing.sta.STA
    (or None for congestion-only). Returns a dict with success/overused/
    cpd/iters/history.

    device_timing: refresh timing on the device (timing.device_loop.
    RouteTiming) — None = on exactly when sta is a GpuSTA, False = the
    host chain below even with one. Needs the GPU engine.
    """
    import time as _time
    from ..timing.device_loop import (has_device_timing,
                                      resolve_device_timing, RouteTiming)
    if sta is not None and has_device_timing(sta) and \
            isinstance(loop.engine, CpuEngine):
        raise ValueError(
            "GpuSTA needs the GPU routing engine (GpuEngine); with "
            "CpuEngine use the CPU engine timing.sta.STA")
    device_timing = resolve_device_timing(sta, device_timing)
    rtiming = None
    if device_timing:
        if not isinstance(loop.engine, GpuEngine):
            raise ValueError(
                "device timing needs the GPU routing engine (GpuEngine); "
                f"got {type(loop.engine).__name__}")
        rtiming = RouteTiming(sta, cmap, intra_delay,
                              device=loop.engine.g.device)
    n_rsinks = len(loop.my_sink_mask)
    crit = np.zeros(n_rsinks, dtype=np.float32)
    prof = dict(route=0.0, sta=0.0, mask=0.0)
    conn_delay = None
    if sta is not None:
        conn_delay = np.zeros(cmap.num_conns, dtype=np.float32)
    pres = 0.0
    active = None
    shrunk = False
    cpd = 0.0
    history = []
    overused = -1
    prev_overused = 1 << 30
    it = 0
    for it in range(1, max_iters + 1):
        # After iteration 1 ONLY the congested ∪ incomplete set is ever
        # rerouted (reference: build_phase_two congested-only). A round-2
        # hardware run showed why: a concurrent rip-ALL reroute at high
        # pres_fac is a limit cycle (every net diverts off the same
        # congestion snapshot simultaneously and recreates it elsewhere —
        # overused oscillated 600↔4000 forever at LU32 scale). The
        # incremental cadence therefore alternates PARTIAL rip-up of the
        # active set with a FULL rip of the same set (timing refresh),
        # never a reroute of frozen feasible nets.
        resync_every = int(os.environ.get("PNR_RESYNC_EVERY", "2"))
        resync = (incremental and resync_every > 0 and it > 2 and
                  (it - 2) % resync_every == 0)
        # stall breaker (see route.gpu_router.pathfinder_route_gpu): a
        # stagnant concurrent endgame switches to the wave schedule
        n_act = int(active.sum()) if active is not None else 0
        force_waves = (it >= 4 and 0 < overused and
                       overused > 0.85 * prev_overused and
                       0 < n_act <= 2048)
        prev_overused = overused if overused > 0 else prev_overused
        _t0 = _time.perf_counter()
        if rtiming is not None:
            overused, sd = loop.iteration(crit, pres, acc_fac,
                                          active_mask=active,
                                          partial=incremental and
                                          active is not None and not resync,
                                          force_waves=force_waves,
                                          device_timing=True)
        else:
            overused, sd = loop.iteration(crit, pres, acc_fac,
                                          active_mask=active,
                                          partial=incremental and
                                          active is not None and not resync,
                                          force_waves=force_waves)
        _t1 = _time.perf_counter()
        if rtiming is not None:
            cpd, crit = rtiming.update(sd)
        elif sta is not None:
            cmap.conn_delays(sd, out=conn_delay, fill=intra_delay)
            cpd, _slack, c = sta.analyze(conn_delay)
            crit = cmap.sink_crit(c)
        _t2 = _time.perf_counter()
        # the active mask is congested ∪ incomplete (global, collective on
        # every rank) — success requires BOTH overused == 0 and no net with
        # unreached sinks (fail_ok engines can leave stranded
        # connections that never show up as overuse)
        active = loop.global_congested_mask()
        n_active = int(active.sum())
        _t3 = _time.perf_counter()
        prof["route"] += _t1 - _t0
        prof["sta"] += _t2 - _t1
        prof["mask"] += _t3 - _t2
        done = overused == 0 and n_active == 0
        if not n_active:
            active = None
        elif (overused > 0 and loop.ws > 1 and not shrunk and
              n_active < shrink_threshold):
            loop.shrink_active(active, k=1)
            shrunk = True
        history.append(dict(iter=it, overused=int(overused),
                            active=n_active, cpd=cpd, shrunk=shrunk))
        if verbose and loop.rank == 0:
            print(f"[dist] iter {it}: overused={overused} "
                  f"active={n_active} cpd={cpd*1e9:.2f}ns shrunk={shrunk} "
                  f"t_route={_t1-_t0:.2f}s t_sta={_t2-_t1:.2f}s "
                  f"t_mask={_t3-_t2:.2f}s")
        if done:
            break
        pres = pres_fac_init if pres == 0.0 else pres * pres_fac_mult
    return dict(success=done, overused=int(overused), cpd=cpd,
                iters=it, shrunk=shrunk, history=history, prof=prof)
