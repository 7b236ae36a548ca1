"""GPU SA placer driver (host side of csrc/hip/place_kernel.hip).

Shares the adaptive outer schedule with the CPU oracle (placer.py) but runs
move batches as propose + commit (resolve and apply) kernel pairs, enqueued
in chunks by the native run loop pnr_place_run. Batched moves with
exclusive net+tile claims are sequential-equivalent (disjoint winners,
exact deltas), so the anneal semantics match the reference's try_swap loop
at a per-batch granularity. The earlier driver, one four-kernel
pnr_place_batch call per batch, stays selectable (legacy_batches=True) as
the oracle the run loop is tested against. Both drivers run the same
device code for propose, resolve and apply; they differ in how claims are
taken (reset + atomicMin, or epoch keys), in the launches per batch and
in where the stop rule runs.
"""
import ctypes as ct
import math

import numpy as np

from ..arch.archdef import ArchDef
from ..ops import hip_api
from .placer import Placement, analytic_delay_matrix


class PlaceLaunchArgs(ct.Structure):
    _fields_ = [
        ("net_blk_ptr", ct.c_void_p), ("net_blks", ct.c_void_p),
        ("blk_net_ptr", ct.c_void_p), ("blk_nets", ct.c_void_p),
        ("blk_type", ct.c_void_p), ("tile_btype", ct.c_void_p),
        ("type_cols", ct.c_void_p), ("type_col_ptr", ct.c_void_p),
        ("fixed", ct.c_void_p),
        ("net_q", ct.c_void_p),
        ("net_sink_ptr", ct.c_void_p), ("conn_crit", ct.c_void_p),
        ("delay_mat", ct.c_void_p),
        ("bx", ct.c_void_p), ("by", ct.c_void_p), ("bslot", ct.c_void_p),
        ("grid", ct.c_void_p),
        ("net_cost", ct.c_void_p), ("net_tcost", ct.c_void_p),
        ("num_blocks", ct.c_int32), ("num_nets", ct.c_int32),
        ("gx", ct.c_int32), ("gy", ct.c_int32), ("cap", ct.c_int32),
        ("nx", ct.c_int32), ("ny", ct.c_int32), ("io_cap", ct.c_int32),
        ("rx0", ct.c_int32), ("rx1", ct.c_int32),
        ("macro_of", ct.c_void_p), ("macro_ptr", ct.c_void_p),
        ("macro_blk", ct.c_void_p),
        ("mv_blk", ct.c_void_p), ("mv_to", ct.c_void_p), ("mv_other", ct.c_void_p),
        ("mv_dbb", ct.c_void_p), ("mv_dtd", ct.c_void_p), ("mv_flags", ct.c_void_p),
        ("net_claim", ct.c_void_p), ("loc_claim", ct.c_void_p),
        ("counters", ct.c_void_p), ("n_moves", ct.c_int32),
        ("T", ct.c_float), ("rlim", ct.c_int32), ("timing_tradeoff", ct.c_float),
        ("inv_bb_norm", ct.c_float), ("inv_td_norm", ct.c_float),
        ("seed", ct.c_uint32), ("batch", ct.c_uint32),
        ("cost_acc", ct.c_void_p),
        # pnr_place_run only: source tiles, 64-bit epoch claims, control block
        ("mv_from", ct.c_void_p),
        ("net_claim64", ct.c_void_p), ("loc_claim64", ct.c_void_p),
        ("run_ctrl", ct.c_void_p),
        # the counter shards (128-byte lines)
        ("run_shards", ct.c_void_p), ("n_shards", ct.c_int32),
        # stored costs of accepted moves, [n_moves x cost_k] each
        ("mv_ncost", ct.c_void_p), ("mv_ntcost", ct.c_void_p),
        ("cost_k", ct.c_int32),
    ]


# Batches enqueued per pnr_place_run call (a multiple of 4, the stop rule's
# period). Between chunks the host reads the control block once; past the
# stop point the rest of a chunk costs empty launches only.
RUN_CHUNK_BATCHES = 32

# The run loop's device state is one int32 buffer of 128-byte lines:
#   line 0       counters[0..3] (the totals; in the run loop written by the
#                stop rule's fold only), then the control block: done,
#                batches executed, ticket. The first RUN_HOST_WORDS words
#                are all the host reads.
#   lines 1...   COUNTER_SHARDS lines, four counters at the start of each:
#                what the waves' counter atomics target
LINE_WORDS = 32
RUN_HOST_WORDS = 8
# Shards the run loop spreads its counter atomics over (a power of two).
# With 64 a line takes the atomics of about 9 of bitcoin_miner's 588
# workgroups; docs/MEASUREMENTS.md has the sweep (8, 64, 1024).
COUNTER_SHARDS = 64


def _lib():
    lib = hip_api.lib()
    if not hasattr(lib, "_place_ready"):
        lib.pnr_place_batch.restype = ct.c_int
        lib.pnr_place_batch.argtypes = [ct.POINTER(PlaceLaunchArgs), ct.c_void_p]
        lib.pnr_place_run.restype = ct.c_int
        lib.pnr_place_run.argtypes = [ct.POINTER(PlaceLaunchArgs), ct.c_uint32,
                                      ct.c_int32, ct.c_int32, ct.c_void_p]
        lib.pnr_place_refresh.restype = ct.c_int
        lib.pnr_place_refresh.argtypes = [ct.POINTER(PlaceLaunchArgs), ct.c_void_p]
        lib.pnr_place_args_sizeof.restype = ct.c_int64
        if lib.pnr_place_args_sizeof() != ct.sizeof(PlaceLaunchArgs):
            raise RuntimeError("PlaceLaunchArgs ABI mismatch")
        lib._place_ready = True
    return lib


def ptr(t):
    return ct.c_void_p(t.data_ptr())


class GpuPlacer:
    def __init__(self, netlist, arch: ArchDef, seed=7, timing=False,
                 device="cuda:0", n_moves=None, fixed=None,
                 delay_matrix="analytic", macros=None, legacy_batches=False):
        import torch
        self.torch = torch
        # True: one pnr_place_batch call per batch with a host check every
        # fourth (the oracle for the native run loop, pnr_place_run)
        self.legacy_batches = legacy_batches
        self.device = device
        self.arch = arch
        self.nl = netlist
        self.seed = seed
        self.timing = timing
        nb = netlist.num_blocks
        nn = netlist.num_nets
        gx, gy = arch.nx + 2, arch.ny + 2
        self.gx, self.gy = gx, gy
        self.cap = max(1, arch.io_cap)
        self.batch_counter = 0

        # net -> member blocks CSR (driver first)
        counts = 1 + np.diff(netlist.net_sink_ptr)
        net_blk_ptr = np.r_[0, np.cumsum(counts)].astype(np.int32)
        net_blks = np.empty(net_blk_ptr[-1], dtype=np.int32)
        net_blks[net_blk_ptr[:-1]] = netlist.net_driver
        is_sink = np.ones(len(net_blks), dtype=bool)
        is_sink[net_blk_ptr[:-1]] = False
        net_blks[is_sink] = netlist.net_sinks
        # block -> nets CSR (deduped per block), vectorized: sort (block,
        # net) membership pairs and drop duplicates within a block
        net_of_member = np.repeat(np.arange(nn, dtype=np.int64),
                                  np.diff(net_blk_ptr))
        key = net_blks.astype(np.int64) * nn + net_of_member
        key = np.unique(key)   # sorted by (block, net), deduped
        mb = (key // nn).astype(np.int32)
        blk_nets = (key % nn).astype(np.int32)
        blk_net_ptr = np.zeros(nb + 1, dtype=np.int32)
        np.add.at(blk_net_ptr, mb + 1, 1)
        blk_net_ptr = np.cumsum(blk_net_ptr, dtype=np.int64).astype(np.int32)
        q = _cross_count_vec(counts).astype(np.float32)

        def up(a, dtype=None):
            t = torch.from_numpy(np.ascontiguousarray(a))
            return t.to(device)

        self.t_net_blk_ptr = up(net_blk_ptr)
        self.t_net_blks = up(net_blks)
        self.t_blk_net_ptr = up(blk_net_ptr)
        self.t_blk_nets = up(blk_nets)
        self.t_blk_type = up(netlist.block_type)
        # heterogeneous fabrics carry a tile-type grid; homogeneous pass
        # nullptr so the validated perimeter-IO fast path runs unchanged
        self.t_tile_btype = (up(arch.tile_btype_grid())
                             if arch.is_heterogeneous() else None)
        self.t_type_cols = self.t_type_col_ptr = None
        if arch.is_heterogeneous():
            # sorted column lists (RAM then DSP) for the kernel's
            # sparse-column move proposals
            ram_cols = [x for x in range(1, arch.nx + 1)
                        if arch.col_block_type(x) == 2]
            dsp_cols = [x for x in range(1, arch.nx + 1)
                        if arch.col_block_type(x) == 3]
            self.t_type_cols = up(np.asarray(ram_cols + dsp_cols,
                                             dtype=np.int32))
            self.t_type_col_ptr = up(np.asarray(
                [0, len(ram_cols), len(ram_cols) + len(dsp_cols)],
                dtype=np.int32))
        self.t_net_q = up(q)
        # pinned blocks (pad_loc_file): mask on device, teleport at init
        self._fixed = fixed
        self.t_fixed = None
        if fixed is not None:
            mask = np.zeros(nb, dtype=np.uint8)
            mask[np.asarray(fixed[0], dtype=np.int64)] = 1
            self.t_fixed = up(mask)
        self.t_net_sink_ptr = up(netlist.net_sink_ptr.astype(np.int32))
        self.t_conn_crit = torch.zeros(netlist.num_conns, dtype=torch.float32,
                                       device=device)
        if timing:
            if delay_matrix == "routed":
                from .delay_matrix import routed_delay_matrix
                dm = routed_delay_matrix(arch)
            else:
                dm = analytic_delay_matrix(arch)
            self._dm = dm
            self.t_delay_mat = up(dm.ravel())
        else:
            self._dm = None
            self.t_delay_mat = None

        # initial placement (host, deterministic)
        bx, by, bslot, grid = self._initial_placement(seed)
        # carry-chain macros (reference: place_macro.c): legalize the
        # initial placement so each chain sits at its rigid offsets, and
        # upload the membership tables the kernels use to move chains
        # as one (propose/resolve/apply macro branches)
        self.t_macro_of = self.t_macro_ptr = self.t_macro_blk = None
        self.macros = macros or []
        if self.macros:
            bx, by, bslot, grid = self._legalize_macros(
                bx, by, bslot, grid, self.macros)
            macro_of = np.full(nb, -1, dtype=np.int32)
            mptr = [0]
            mblk = []
            for mi, grp in enumerate(self.macros):
                for (b, dx, dy) in grp:
                    macro_of[b] = mi
                    mblk.append(b)
                mptr.append(len(mblk))
            self.t_macro_of = up(macro_of)
            self.t_macro_ptr = up(np.asarray(mptr, dtype=np.int32))
            self.t_macro_blk = up(np.asarray(mblk, dtype=np.int32))
        self.t_bx = up(bx); self.t_by = up(by); self.t_bslot = up(bslot)
        self.t_grid = up(grid)
        self.t_net_cost = torch.zeros(nn, dtype=torch.float32, device=device)
        self.t_net_tcost = torch.zeros(nn, dtype=torch.float32, device=device)

        # batch sized for >=~0.65 claim-winner fraction (simulated at
        # bitcoin scale: nb/16 -> 0.66, nb/8 -> 0.47; measured at tseng:
        # quality degrades once conflicts bias the applied-move sample)
        self.n_moves = n_moves or int(np.clip(nb // 16, 64, 1 << 16))
        nm = self.n_moves
        self.t_mv_blk = torch.zeros(nm, dtype=torch.int32, device=device)
        self.t_mv_to = torch.zeros(nm, dtype=torch.int32, device=device)
        self.t_mv_other = torch.zeros(nm, dtype=torch.int32, device=device)
        self.t_mv_dbb = torch.zeros(nm, dtype=torch.float32, device=device)
        self.t_mv_dtd = torch.zeros(nm, dtype=torch.float32, device=device)
        self.t_mv_flags = torch.zeros(nm, dtype=torch.uint8, device=device)
        self.t_net_claim = self.t_loc_claim = None
        self.t_net_claim64 = self.t_loc_claim64 = None
        if legacy_batches:
            self.t_net_claim = torch.zeros(nn, dtype=torch.int32, device=device)
            self.t_loc_claim = torch.zeros(gx * gy, dtype=torch.int32,
                                           device=device)
        else:
            # epoch-key claims: zeroed here once, never reset (batch
            # numbers start at 1, so every key beats the zero word)
            self.t_net_claim64 = torch.zeros(nn, dtype=torch.int64,
                                             device=device)
            self.t_loc_claim64 = torch.zeros(gx * gy, dtype=torch.int64,
                                             device=device)
        self.t_mv_from = torch.zeros(nm, dtype=torch.int32, device=device)
        # Costs that propose stores for commit, one slot per net of a move's
        # two blocks. cost_k covers any two blocks of this netlist up to the
        # 64 a wave holds in one pass; a move with more nets is recomputed
        # by apply.
        max_deg = int(np.diff(blk_net_ptr).max()) if nb else 0
        self.cost_k = int(np.clip(2 * max_deg, 1, 64))
        self.t_mv_ncost = torch.zeros(nm * self.cost_k, dtype=torch.float32,
                                      device=device)
        self.t_mv_ntcost = torch.zeros(nm * self.cost_k, dtype=torch.float32,
                                       device=device)
        # counters, control block and counter shards share one buffer
        # (layout: LINE_WORDS above): one zero_() clears them all
        self.n_shards = COUNTER_SHARDS
        self.t_run_state = torch.zeros((1 + self.n_shards) * LINE_WORDS,
                                       dtype=torch.int32, device=device)
        if self.t_run_state.data_ptr() % (4 * LINE_WORDS):
            raise RuntimeError("run state is not 128-byte aligned")
        self.t_counters = self.t_run_state[:4]
        self.t_run_ctrl = self.t_run_state[4:RUN_HOST_WORDS]
        self.t_run_shards = self.t_run_state[LINE_WORDS:]
        self.t_cost_acc = torch.zeros(2, dtype=torch.float64, device=device)

        self.lib = _lib()
        self.bb_cost, self.td_cost = self.refresh_costs()

    def _initial_placement(self, seed):
        arch = self.arch
        nl = self.nl
        rng = np.random.default_rng(seed)
        nb = nl.num_blocks
        bx = np.zeros(nb, dtype=np.int32)
        by = np.zeros(nb, dtype=np.int32)
        bslot = np.zeros(nb, dtype=np.int32)
        if self._fixed is not None:
            bx2, by2, bs2, grid = self._initial_placement_free(rng)
            ids, fx, fy, fs = [np.asarray(a) for a in self._fixed]
            for b, x, y, sl in zip(ids, fx, fy, fs):
                occ = grid[x, y, sl]
                if occ == b:
                    continue
                grid[bx2[b], by2[b], bs2[b]] = occ
                if occ >= 0:
                    bx2[occ], by2[occ], bs2[occ] = bx2[b], by2[b], bs2[b]
                bx2[b], by2[b], bs2[b] = x, y, sl
                grid[x, y, sl] = b
            return bx2, by2, bs2, grid.reshape(-1)
        return self._initial_placement_free(rng, flat=True)

    def _legalize_macros(self, bx, by, bslot, grid, macros):
        """Re-place each macro's members at their rigid offsets on free
        tiles (deterministic first-fit anchor scan). Members vacate their
        initial tiles first; non-members are never displaced."""
        arch = self.arch
        g = grid.reshape(self.gx, self.gy, self.cap)
        members = [b for grp in macros for (b, _, _) in grp]
        for b in members:
            g[bx[b], by[b], bslot[b]] = -1
        tb = (arch.tile_btype_grid().reshape(self.gx, self.gy)
              if arch.is_heterogeneous() else None)

        def tile_ok(b, x, y):
            if not (0 <= x < self.gx and 0 <= y < self.gy):
                return False
            bt = int(self.nl.block_type[b])
            if tb is not None:
                if tb[x, y] != bt:
                    return False
            else:
                io = (x == 0 or x == self.gx - 1 or
                      y == 0 or y == self.gy - 1)
                inner = 1 <= x <= arch.nx and 1 <= y <= arch.ny
                if bt == 0 or io or not inner:
                    return False    # macros on logic tiles only
            return g[x, y, 0] < 0

        for grp in macros:
            placed = False
            for ax in range(1, arch.nx + 1):
                for ay in range(1, arch.ny + 1):
                    if all(tile_ok(b, ax + dx, ay + dy)
                           for (b, dx, dy) in grp):
                        for (b, dx, dy) in grp:
                            bx[b], by[b], bslot[b] = ax + dx, ay + dy, 0
                            g[ax + dx, ay + dy, 0] = b
                        placed = True
                        break
                if placed:
                    break
            if not placed:
                raise ValueError("cannot legalize macro (grid too full)")
        return bx, by, bslot, g.reshape(-1)

    def _initial_placement_free(self, rng, flat=False):
        arch = self.arch
        nl = self.nl
        nb = nl.num_blocks
        bx = np.zeros(nb, dtype=np.int32)
        by = np.zeros(nb, dtype=np.int32)
        bslot = np.zeros(nb, dtype=np.int32)
        grid = np.full((self.gx, self.gy, self.cap), -1, dtype=np.int32)
        ios = np.nonzero(nl.block_type == 0)[0]
        if not arch.is_heterogeneous():
            clbs = np.nonzero(nl.block_type == 1)[0]
            tiles = rng.permutation(arch.nx * arch.ny)[:len(clbs)]
            if len(tiles) < len(clbs):
                raise ValueError("too many CLBs for grid")
            bx[clbs] = tiles // arch.ny + 1
            by[clbs] = tiles % arch.ny + 1
            grid[bx[clbs], by[clbs], 0] = clbs
        else:
            col_t = np.asarray([arch.col_block_type(x)
                                for x in range(1, arch.nx + 1)])
            for t in (1, 2, 3):
                blks = np.nonzero(nl.block_type == t)[0]
                if not len(blks):
                    continue
                cols = np.nonzero(col_t == t)[0]
                cand = (cols[:, None] * arch.ny +
                        np.arange(arch.ny)[None, :]).ravel()
                if len(blks) > len(cand):
                    raise ValueError(f"too many type-{t} blocks for grid")
                tiles = cand[rng.permutation(len(cand))[:len(blks)]]
                bx[blks] = tiles // arch.ny + 1
                by[blks] = tiles % arch.ny + 1
                grid[bx[blks], by[blks], 0] = blks
        io_locs = ([(0, y) for y in range(1, arch.ny + 1)] +
                   [(self.gx - 1, y) for y in range(1, arch.ny + 1)] +
                   [(x, 0) for x in range(1, arch.nx + 1)] +
                   [(x, self.gy - 1) for x in range(1, arch.nx + 1)])
        slots = [(x, y, s) for (x, y) in io_locs for s in range(arch.io_cap)]
        sel = rng.permutation(len(slots))[:len(ios)]
        for b, k in zip(ios, sel):
            x, y, s = slots[k]
            bx[b], by[b], bslot[b] = x, y, s
            grid[x, y, s] = b
        return (bx, by, bslot, grid.reshape(-1)) if flat \
            else (bx, by, bslot, grid)

    def _args(self, T=0.0, rlim=1, tt=0.0, inv_bb=1.0, inv_td=1.0):
        a = PlaceLaunchArgs()
        a.net_blk_ptr = ptr(self.t_net_blk_ptr); a.net_blks = ptr(self.t_net_blks)
        a.blk_net_ptr = ptr(self.t_blk_net_ptr); a.blk_nets = ptr(self.t_blk_nets)
        a.blk_type = ptr(self.t_blk_type)
        a.tile_btype = (ptr(self.t_tile_btype)
                        if self.t_tile_btype is not None else None)
        a.type_cols = (ptr(self.t_type_cols)
                       if self.t_type_cols is not None else None)
        a.type_col_ptr = (ptr(self.t_type_col_ptr)
                          if self.t_type_col_ptr is not None else None)
        a.fixed = ptr(self.t_fixed) if self.t_fixed is not None else None
        a.net_q = ptr(self.t_net_q)
        a.net_sink_ptr = ptr(self.t_net_sink_ptr)
        a.conn_crit = ptr(self.t_conn_crit)
        a.delay_mat = ptr(self.t_delay_mat) if self.t_delay_mat is not None else None
        a.bx = ptr(self.t_bx); a.by = ptr(self.t_by); a.bslot = ptr(self.t_bslot)
        a.grid = ptr(self.t_grid)
        a.net_cost = ptr(self.t_net_cost); a.net_tcost = ptr(self.t_net_tcost)
        a.num_blocks = self.nl.num_blocks; a.num_nets = self.nl.num_nets
        a.gx = self.gx; a.gy = self.gy; a.cap = self.cap
        a.nx = self.arch.nx; a.ny = self.arch.ny; a.io_cap = self.arch.io_cap
        a.rx0, a.rx1 = getattr(self, "move_region", (-1, -1))
        if getattr(self, "t_macro_of", None) is not None:
            a.macro_of = ptr(self.t_macro_of)
            a.macro_ptr = ptr(self.t_macro_ptr)
            a.macro_blk = ptr(self.t_macro_blk)
        else:
            a.macro_of = a.macro_ptr = a.macro_blk = None
        a.mv_blk = ptr(self.t_mv_blk); a.mv_to = ptr(self.t_mv_to)
        a.mv_other = ptr(self.t_mv_other); a.mv_dbb = ptr(self.t_mv_dbb)
        a.mv_dtd = ptr(self.t_mv_dtd); a.mv_flags = ptr(self.t_mv_flags)
        if self.legacy_batches:
            a.net_claim = ptr(self.t_net_claim)
            a.loc_claim = ptr(self.t_loc_claim)
            a.net_claim64 = a.loc_claim64 = None
        else:
            a.net_claim = a.loc_claim = None
            a.net_claim64 = ptr(self.t_net_claim64)
            a.loc_claim64 = ptr(self.t_loc_claim64)
        a.mv_from = ptr(self.t_mv_from)
        a.run_ctrl = ptr(self.t_run_ctrl)
        a.run_shards = ptr(self.t_run_shards)
        a.n_shards = self.n_shards
        a.mv_ncost = ptr(self.t_mv_ncost); a.mv_ntcost = ptr(self.t_mv_ntcost)
        a.cost_k = self.cost_k
        a.counters = ptr(self.t_counters); a.n_moves = self.n_moves
        a.T = T; a.rlim = max(1, int(rlim)); a.timing_tradeoff = tt
        a.inv_bb_norm = inv_bb; a.inv_td_norm = inv_td
        a.seed = self.seed & 0xFFFFFFFF; a.batch = self.batch_counter
        a.cost_acc = ptr(self.t_cost_acc)
        return a

    def _stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def refresh_costs(self):
        self.t_cost_acc.zero_()
        a = self._args(tt=1.0 if self.timing else 0.0)
        rc = self.lib.pnr_place_refresh(ct.byref(a), self._stream())
        hip_api.check(rc, "place_refresh")
        self.torch.cuda.synchronize(self.device)
        bb, td = self.t_cost_acc.cpu().numpy()
        self.bb_cost, self.td_cost = float(bb), float(td)
        return self.bb_cost, self.td_cost

    def run_batches(self, T, rlim, target_moves, tt, bb_norm, td_norm,
                    max_batches=256):
        """Launch move batches until ~target_moves moves have been DECIDED
        (applied winners + Metropolis rejects; claim-conflict losers don't
        count — they were never decided). Returns (success_rate, attempts).
        Mirrors the serial placer's move_lim semantics under batching.

        The stop rule is evaluated after every 4th batch: by the device in
        the native run loop, by the host in the legacy loop. Both run the
        same batches and advance batch_counter by the batches executed."""
        if self.legacy_batches:
            return self._run_batches_legacy(T, rlim, target_moves, tt,
                                            bb_norm, td_norm, max_batches)
        self.t_run_state.zero_()    # counters, control block, shards
        a = self._args(T=T, rlim=rlim, tt=tt,
                       inv_bb=1.0 / bb_norm, inv_td=1.0 / td_norm)
        target = int(min(max(math.ceil(target_moves), -0x7FFFFFFF),
                         0x7FFFFFFF))
        cap = 4 * ((max_batches + 3) // 4)   # the legacy loop runs in fours
        first = self.batch_counter + 1
        enq = 0
        att = acc = executed = 0
        while enq < cap:
            n = min(RUN_CHUNK_BATCHES, cap - enq)
            rc = self.lib.pnr_place_run(ct.byref(a), first + enq, target, n,
                                        self._stream())
            hip_api.check(rc, "place_run")
            enq += n
            # one small device-to-host copy per chunk (it synchronises)
            st = self.t_run_state[:RUN_HOST_WORDS].cpu().numpy()
            att, acc = int(st[0]), int(st[1])
            done, executed = int(st[4]), int(st[5])
            if done:
                break
        self.batch_counter += executed
        srate = acc / max(1, att)
        return srate, att

    def _run_batches_legacy(self, T, rlim, target_moves, tt, bb_norm, td_norm,
                            max_batches=256):
        self.t_counters.zero_()
        batches = 0
        win = att = acc = 0
        while batches < max_batches:
            for _ in range(4):
                self.batch_counter += 1
                a = self._args(T=T, rlim=rlim, tt=tt,
                               inv_bb=1.0 / bb_norm, inv_td=1.0 / td_norm)
                rc = self.lib.pnr_place_batch(ct.byref(a), self._stream())
                hip_api.check(rc, "place_batch")
                batches += 1
            self.torch.cuda.synchronize(self.device)
            c = self.t_counters.cpu().numpy()
            att, acc, win = int(c[0]), int(c[1]), int(c[2])
            if win + (att - acc) >= target_moves:
                break
        else:
            self.torch.cuda.synchronize(self.device)
        # temperature control wants the Metropolis acceptance fraction;
        # claim-conflict losers are neither accepts nor rejects
        srate = acc / max(1, att)
        return srate, att

    def set_move_region(self, x0, x1):
        """Confine moves to columns [x0, x1] (strip-sharded distributed
        anneal, parallel/dist_place.py); (-1, -1) disables."""
        self.move_region = (x0, x1)

    def set_crit(self, conn_crit):
        t = self.torch.from_numpy(np.ascontiguousarray(conn_crit,
                                                       dtype=np.float32))
        self.t_conn_crit.copy_(t.to(self.device))

    def placement(self):
        return Placement(self.t_bx.cpu().numpy(), self.t_by.cpu().numpy(),
                         self.t_bslot.cpu().numpy(),
                         bb_cost=self.bb_cost, td_cost=self.td_cost)

    def check_place(self):
        """Host-side validation of GPU placement state (check_place:2950)."""
        bx = self.t_bx.cpu().numpy(); by = self.t_by.cpu().numpy()
        bslot = self.t_bslot.cpu().numpy()
        grid = self.t_grid.cpu().numpy().reshape(self.gx, self.gy, self.cap)
        nl = self.nl
        tb = (self.arch.tile_btype_grid().reshape(self.gx, self.gy)
              if self.arch.is_heterogeneous() else None)
        btype = np.asarray(nl.block_type)
        if tb is not None:
            bad_type = tb[bx, by] != btype
        else:
            on_io = ((bx == 0) | (bx == self.gx - 1) | (by == 0) |
                     (by == self.gy - 1))
            bad_type = (btype == 0) != on_io
        bad_grid = grid[bx, by, bslot] != np.arange(nl.num_blocks)
        bad = bad_type | bad_grid
        if bad.any():
            b = int(np.argmax(bad))     # first offending block
            if bad_type[b]:
                return False, f"block {b} type/loc mismatch"
            return False, f"grid inconsistent at block {b}"
        occ = (grid >= 0).sum()
        if occ != nl.num_blocks:
            return False, f"grid count {occ} != blocks {nl.num_blocks}"
        # carry-chain rigidity (reference: check_place macro member check)
        for grp in getattr(self, "macros", []):
            b0, dx0, dy0 = grp[0]
            for (b, dx, dy) in grp[1:]:
                if (bx[b] - bx[b0] != dx - dx0 or
                        by[b] - by[b0] != dy - dy0):
                    return False, f"macro offsets broken at block {b}"
        return True, ""


def _cross_count(n):
    q3, q50 = 1.0, 2.79
    if n <= 3:
        return q3
    if n >= 50:
        return q50 + 0.02616 * (n - 50)
    return q3 + (q50 - q3) * (n - 3) / 47.0


def _cross_count_vec(counts):
    """_cross_count over an integer array (same float64 operations)."""
    n = np.asarray(counts, dtype=np.int64)
    q3, q50 = 1.0, 2.79
    return np.where(n <= 3, q3,
                    np.where(n >= 50, q50 + 0.02616 * (n - 50),
                             q3 + (q50 - q3) * (n - 3) / 47.0))


def anneal_place_gpu(netlist, arch, seed=7, timing_tradeoff=0.5, inner_num=1.0,
                     sta=None, crit_exp=1.0, verbose=False, device="cuda:0",
                     n_moves=None, fixed=None, delay_matrix="analytic",
                     macros=None, legacy_batches=False, device_timing=None):
    """GPU anneal with the same adaptive schedule as the CPU oracle.

    device_timing: refresh criticalities on the device each temperature
    (timing.device_loop.PlaceTiming: placement -> conn delays -> GpuSTA ->
    t_conn_crit, nothing copied to the host). None = on exactly when sta
    is a GpuSTA; False forces the host chain below, which a GpuSTA serves
    through its numpy analyze()."""
    import time as _time
    from ..timing.device_loop import resolve_device_timing, PlaceTiming
    timing = sta is not None and timing_tradeoff > 0
    device_timing = resolve_device_timing(sta, device_timing) and timing
    placer = GpuPlacer(netlist, arch, seed=seed, timing=timing, device=device,
                       n_moves=n_moves, fixed=fixed, delay_matrix=delay_matrix,
                       macros=macros, legacy_batches=legacy_batches)
    nb = netlist.num_blocks
    move_lim = max(256, int(inner_num * (nb ** 1.3333)))
    rlim = float(max(arch.nx, arch.ny))
    tt = timing_tradeoff if timing else 0.0
    ptiming = PlaceTiming(placer, sta, crit_exp=crit_exp) \
        if device_timing else None
    # time in refresh_crit: every call starts after a host read of device
    # state and ends in refresh_costs' synchronise
    prof = {"refresh_s": 0.0, "refreshes": 0}

    def refresh_crit():
        if not timing:
            return
        _t0 = _time.perf_counter()
        _refresh_crit()
        prof["refresh_s"] += _time.perf_counter() - _t0
        prof["refreshes"] += 1

    def _refresh_crit():
        if ptiming is not None:
            ptiming.refresh()
            placer.refresh_costs()
            return
        # conn delays from current placement via the delay matrix
        bx = placer.t_bx.cpu().numpy(); by = placer.t_by.cpu().numpy()
        drv = netlist.net_driver
        d_per_conn = np.empty(netlist.num_conns, dtype=np.float32)
        dm = placer._dm if placer._dm is not None else analytic_delay_matrix(arch)
        net_of_conn = np.repeat(np.arange(netlist.num_nets),
                                np.diff(netlist.net_sink_ptr))
        dx = np.abs(bx[netlist.net_sinks] - bx[drv[net_of_conn]])
        dy = np.abs(by[netlist.net_sinks] - by[drv[net_of_conn]])
        d_per_conn = dm[dx, dy]
        cpd, slack, c = sta.analyze(d_per_conn)
        placer.set_crit(np.asarray(c) ** crit_exp)
        placer.refresh_costs()

    refresh_crit()
    norm_mode = tt > 0

    def norms():
        if norm_mode:
            return (max(placer.bb_cost, 1e-12), max(placer.td_cost, 1e-30))
        return (1.0, 1.0)

    bb_norm, td_norm = norms()
    # starting T = 20 * std(move deltas) (reference: place.c:1045
    # starting_t), measured from a hot probe batch's accepted deltas
    placer.run_batches(1e30, rlim, min(move_lim, 2048), tt, bb_norm, td_norm,
                       max_batches=16)
    torch = placer.torch
    flags = placer.t_mv_flags
    sel = flags >= 1
    if int(sel.sum().item()) >= 8:
        d = (1.0 - tt) * placer.t_mv_dbb[sel] / bb_norm
        if tt > 0:
            d = d + tt * placer.t_mv_dtd[sel] / td_norm
        t = float(20.0 * d.std().item())
    else:
        t = 20.0 * placer.bb_cost / max(1, netlist.num_nets) / bb_norm
    placer.refresh_costs()
    if t <= 0:
        t = 1.0
    history = []
    itemp = 0
    while True:
        refresh_crit()
        bb_norm, td_norm = norms()
        srate, _ = placer.run_batches(t, rlim, move_lim, tt, bb_norm, td_norm)
        placer.refresh_costs()  # exact resync every temperature
        cost = placer.bb_cost
        history.append((t, cost, srate, rlim))
        if verbose:
            print(f"[gpu] T={t:.3e} bb={cost:.1f} acc={srate:.2f} rlim={rlim:.0f}")
        if srate > 0.96:
            t *= 0.5
        elif srate > 0.8:
            t *= 0.9
        elif srate > 0.15 or rlim > 1:
            t *= 0.95
        else:
            t *= 0.8
        rlim = min(max(rlim * (1.0 - 0.44 + srate), 1.0),
                   float(max(arch.nx, arch.ny)))
        itemp += 1
        exit_cost = 1.0 if norm_mode else cost
        if t < 0.005 * exit_cost / max(1, netlist.num_nets):
            break
        if itemp > 500:
            break
    placer.run_batches(0.0, 1.0, move_lim, tt, bb_norm, td_norm)
    placer.refresh_costs()
    ok, err = placer.check_place()
    if not ok:
        raise RuntimeError(f"gpu check_place failed: {err}")
    pl = placer.placement()
    pl.stats = {"temps": itemp, "move_lim": move_lim, "history": history,
                "engine": "gpu", "device_timing": ptiming is not None,
                "refresh_s": prof["refresh_s"],
                "refreshes": prof["refreshes"]}
    return pl
