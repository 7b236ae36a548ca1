"""GPU STA: levelized slack/criticality sweeps as HIP kernels.

Host side of csrc/hip/sta_kernel.hip (single clock, GpuSTA) and
csrc/hip/sta_constrained.hip (clock domains, GpuConstrainedSTA). Graph
topology (levels + CSRs) is built once by the C++ TimingGraph and
uploaded; per-iteration analysis takes a device conn-delay tensor and
produces device slack/crit tensors (cpd returned to host).
"""
import ctypes as ct

import numpy as np

from ..arch.archdef import ArchDef
from ..ops import hip_api
from .. import ops


class StaLaunchArgs(ct.Structure):
    _fields_ = [
        ("level_blocks", ct.c_void_p), ("level_start", ct.c_void_p),
        ("in_ptr", ct.c_void_p), ("in_conn", ct.c_void_p),
        ("out_ptr", ct.c_void_p), ("out_conn", ct.c_void_p),
        ("conn_driver", ct.c_void_p), ("conn_sink", ct.c_void_p),
        ("is_seq", ct.c_void_p), ("blk_delay", ct.c_void_p),
        ("T_clb", ct.c_float), ("T_seq_out", ct.c_float),
        ("T_seq_in", ct.c_float), ("max_crit", ct.c_float),
        ("num_blocks", ct.c_int32), ("num_levels", ct.c_int32),
        ("num_conns", ct.c_int64),
        ("t_arr", ct.c_void_p), ("t_req", ct.c_void_p), ("cpd_out", ct.c_void_p),
        ("delay", ct.c_void_p), ("slack", ct.c_void_p), ("crit", ct.c_void_p),
        ("level_start_host", ct.c_void_p),
    ]


class StaConstrainedArgs(ct.Structure):
    _fields_ = [
        ("level_blocks", ct.c_void_p),
        ("in_ptr", ct.c_void_p), ("in_conn", ct.c_void_p),
        ("out_ptr", ct.c_void_p), ("out_conn", ct.c_void_p),
        ("conn_driver", ct.c_void_p), ("conn_sink", ct.c_void_p),
        ("is_seq", ct.c_void_p), ("blk_delay", ct.c_void_p),
        ("block_clock", ct.c_void_p),
        ("T_clb", ct.c_float), ("T_seq_out", ct.c_float),
        ("T_seq_in", ct.c_float), ("max_crit", ct.c_float),
        ("num_blocks", ct.c_int32), ("num_levels", ct.c_int32),
        ("K", ct.c_int32), ("R", ct.c_int32),
        ("num_conns", ct.c_int64),
        ("cons", ct.c_void_p), ("pair_row", ct.c_void_p),
        ("skip", ct.c_void_p),
        ("req_period", ct.c_void_p), ("req_domain", ct.c_void_p),
        ("arr", ct.c_void_p), ("req", ct.c_void_p),
        ("delay", ct.c_void_p), ("slack", ct.c_void_p), ("crit", ct.c_void_p),
        ("worst_bits", ct.c_void_p), ("period_out", ct.c_void_p),
        ("level_start_host", ct.c_void_p),
        ("launch", ct.c_void_p), ("capture", ct.c_void_p),
    ]


def _lib():
    lib = hip_api.lib()
    if not hasattr(lib, "_sta_ready"):
        lib.pnr_sta_constrained.restype = ct.c_int
        lib.pnr_sta_constrained.argtypes = [ct.POINTER(StaConstrainedArgs),
                                            ct.c_void_p]
        lib.pnr_sta_constrained_args_sizeof.restype = ct.c_int64
        if lib.pnr_sta_constrained_args_sizeof() != \
                ct.sizeof(StaConstrainedArgs):
            raise RuntimeError("StaConstrainedArgs ABI mismatch")
        lib.pnr_sta_pair_slack.restype = ct.c_int
        lib.pnr_sta_pair_slack.argtypes = [ct.POINTER(StaConstrainedArgs),
                                           ct.c_void_p, ct.c_void_p,
                                           ct.c_void_p]
        lib.pnr_sta_analyze.restype = ct.c_int
        lib.pnr_sta_analyze.argtypes = [ct.POINTER(StaLaunchArgs), ct.c_void_p]
        lib.pnr_sta_args_sizeof.restype = ct.c_int64
        if lib.pnr_sta_args_sizeof() != ct.sizeof(StaLaunchArgs):
            raise RuntimeError("StaLaunchArgs ABI mismatch")
        lib._sta_ready = True
    return lib


class GpuSTA:
    """Single-clock analysis as a loop engine (csrc/hip/sta_kernel.hip) and
    the owner of the device timing graph: levels, CSRs and per-block delays
    are uploaded once here and shared by every GpuConstrainedSTA built on
    it. analyze_device() takes a device delay tensor and leaves cpd, slack
    and crit in t_cpd / t_slack / t_crit, with no allocation, host copy or
    synchronisation. Clock domains are GpuConstrainedSTA's;
    analyze_domains() is the one-call form of it."""

    def __init__(self, netlist, arch: ArchDef, device="cuda:0", max_crit=0.99):
        import torch
        self.torch = torch
        self.device = device
        self.arch = arch
        self.netlist = netlist
        self.max_crit = max_crit
        cpu = ops.cpu()
        from .sta import block_delays
        bd = block_delays(netlist, arch)
        self.tg = cpu.TimingGraph(
            netlist.cpp(), arch.T_clb, arch.T_seq_out, arch.T_seq_in,
            bd if bd is not None else np.empty(0, dtype=np.float32))
        self._blk_delay_host = bd
        blocks, start = self.tg.level_arrays()
        in_ptr, in_conn, out_ptr, out_conn, conn_driver = self.tg.csr_arrays()
        self.level_start_host = np.ascontiguousarray(start, dtype=np.int32)
        self.num_levels = self.tg.num_levels()

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(device)

        self.t_level_blocks = up(blocks)
        self.t_level_start = up(start)
        self.t_in_ptr = up(in_ptr); self.t_in_conn = up(in_conn)
        self.t_out_ptr = up(out_ptr); self.t_out_conn = up(out_conn)
        self.t_conn_driver = up(conn_driver)
        self.t_conn_sink = up(netlist.net_sinks)
        self.t_is_seq = up(netlist.block_is_seq)
        # heterogeneous: per-block comb delay on device; homogeneous: null
        # => the validated scalar-T_clb kernel path runs unchanged
        self.t_blk_delay = (up(self._blk_delay_host)
                            if self._blk_delay_host is not None else None)
        nb = netlist.num_blocks
        nc = netlist.num_conns
        self.t_arr = torch.zeros(nb, dtype=torch.float32, device=device)
        self.t_req = torch.zeros(nb, dtype=torch.float32, device=device)
        self.t_cpd = torch.zeros(1, dtype=torch.float32, device=device)
        self.t_slack = torch.zeros(nc, dtype=torch.float32, device=device)
        self.t_crit = torch.zeros(nc, dtype=torch.float32, device=device)
        self.lib = _lib()
        self._args = self._build_args()

    @property
    def num_conns(self):
        return self.netlist.num_conns

    def _build_args(self):
        a = StaLaunchArgs()
        pt = lambda t: ct.c_void_p(t.data_ptr())
        a.level_blocks = pt(self.t_level_blocks)
        a.level_start = pt(self.t_level_start)
        a.in_ptr = pt(self.t_in_ptr); a.in_conn = pt(self.t_in_conn)
        a.out_ptr = pt(self.t_out_ptr); a.out_conn = pt(self.t_out_conn)
        a.conn_driver = pt(self.t_conn_driver)
        a.conn_sink = pt(self.t_conn_sink)
        a.is_seq = pt(self.t_is_seq)
        a.blk_delay = (pt(self.t_blk_delay)
                       if self.t_blk_delay is not None else None)
        a.T_clb = self.arch.T_clb; a.T_seq_out = self.arch.T_seq_out
        a.T_seq_in = self.arch.T_seq_in; a.max_crit = self.max_crit
        a.num_blocks = self.netlist.num_blocks
        a.num_levels = self.num_levels
        a.num_conns = self.netlist.num_conns
        a.t_arr = pt(self.t_arr); a.t_req = pt(self.t_req)
        a.cpd_out = pt(self.t_cpd)
        a.slack = pt(self.t_slack); a.crit = pt(self.t_crit)
        a.level_start_host = self.level_start_host.ctypes.data_as(ct.c_void_p)
        return a

    def analyze_device(self, t_conn_delay):
        """Device path: conn delays in, (cpd, slack_t, crit_t) out
        (slack/crit stay on device)."""
        self._args.delay = ct.c_void_p(t_conn_delay.data_ptr())
        stream = self.torch.cuda.current_stream().cuda_stream
        rc = self.lib.pnr_sta_analyze(ct.byref(self._args), stream)
        hip_api.check(rc, "sta_analyze")
        return self.t_cpd, self.t_slack, self.t_crit

    def analyze_domains(self, conn_delay, block_clock, periods,
                        pair_skip=None, pair_mult=None):
        """Multi-clock analysis on the device (reference:
        do_timing_analysis_new's (src,sink)-domain-pair loop). Returns
        (worst_achieved_period, slack[], crit[]), equal to the CPU
        TimingGraph.analyze_domains bit for bit (crit up to the max_crit
        clamp; tests/test_sta_exact.py). The worst period is the achieved
        period of the largest achieved/constraint ratio, tracked as one
        packed 64-bit max; among equal ratios the larger period wins
        (the CPU engine keeps the first it meets). With no analysable
        (source, sink) pair both engines return periods[0].

        pair_skip / pair_mult: KxK false-pair and multicycle arrays as in
        STA.analyze_domains; None means no false pair / every multiplier 1.
        One call of a temporary GpuConstrainedSTA (pnr_sta_constrained),
        which validates block_clock and periods (ValueError) and owns
        every buffer it writes: this engine's single-clock results
        (t_arr, t_req, t_slack, t_crit, t_cpd) are left as they are."""
        return GpuConstrainedSTA(self, block_clock, periods, pair_skip,
                                 pair_mult).analyze(conn_delay)

    def analyze(self, conn_delay):
        """Host-compatible API (numpy in/out), mirroring timing.sta.STA
        but with crit pre-clamped to max_crit."""
        torch = self.torch
        t_delay = torch.from_numpy(
            np.ascontiguousarray(conn_delay, dtype=np.float32)).to(self.device)
        self.analyze_device(t_delay)
        torch.cuda.synchronize(self.device)
        return (float(self.t_cpd.item()), self.t_slack.cpu().numpy(),
                self.t_crit.cpu().numpy())


class GpuConstrainedSTA:
    """The multi-clock analysis, with or without false-path and multicycle
    constraints, as a loop engine (csrc/hip/sta_constrained.hip; pair_skip
    and pair_mult None give the plain clock-pair analysis):
    analyze_device() takes a device delay tensor and leaves the worst achieved period, slack and
    crit on the device with no allocation, host copy or synchronisation,
    so timing.device_loop drives it like a GpuSTA.

    It shares the graph tensors of `gsta`, clamps crit with its max_crit
    and owns everything it writes: arr[nb*K] and req[nb*R] (block-major:
    the rows of one block are adjacent; arr_rows()/req_rows() give them
    row by row), slack, crit, the packed worst word, the float32[1]
    period, and the uploaded constraint_plan and block_clock. Results
    equal STA.analyze_domains(..., pair_skip, pair_mult) bit for bit (crit
    up to the max_crit clamp; among equal achieved/constraint ratios the
    worst period is the larger one, where the CPU engine keeps the first
    it meets).

    launch_extra / capture_extra: per-block seconds (SDC I/O delays on
    pads, timing.constraints); the plan's launch / capture tables are
    uploaded and read in place of T_seq_out / T_seq_in. Without them the
    kernels get null tables and the scalars.

    pair_slack() is the report side, outside the loops: the least slack
    per (source, sink) pair of the last analyze_device()."""

    def __init__(self, gsta, block_clock, periods, pair_skip=None,
                 pair_mult=None, launch_extra=None, capture_extra=None):
        from .constraints import constraint_plan, check_block_clock
        torch = gsta.torch
        self.torch = torch
        self.gsta = gsta
        self.device = gsta.device
        self.arch = gsta.arch
        self.netlist = gsta.netlist
        self.max_crit = gsta.max_crit
        self.plan = plan = constraint_plan(
            periods, pair_skip, pair_mult, launch_extra=launch_extra,
            capture_extra=capture_extra, T_seq_out=self.arch.T_seq_out,
            T_seq_in=self.arch.T_seq_in,
            block_is_seq=self.netlist.block_is_seq)
        nb = self.netlist.num_blocks
        nc = self.netlist.num_conns
        bc = check_block_clock(block_clock, nb, plan.K)
        self.K, self.R = plan.K, plan.R
        if gsta.level_start_host[0] != 0 or \
                gsta.level_start_host[gsta.num_levels] != nb:
            raise ValueError("GpuSTA level table does not cover the blocks")
        self.t_conn_driver = gsta.t_conn_driver
        self.t_conn_sink = gsta.t_conn_sink

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

        def buf(n, dtype=torch.float32):
            return torch.zeros(n, dtype=dtype, device=self.device)

        self.t_block_clock = up(bc)
        self.t_cons = up(plan.cons)
        self.t_pair_row = up(plan.pair_row)
        self.t_skip = up(plan.skip)
        self.t_req_period = up(plan.req_period)
        self.t_req_domain = up(plan.req_domain)
        self.t_launch = up(plan.launch) if plan.launch is not None else None
        self.t_capture = (up(plan.capture) if plan.capture is not None
                          else None)
        # pair_slack(): order-preserving bits and the decoded table; the
        # delay tensor of the last analyze_device is kept alive for it
        self.t_pair_bits = buf(plan.K * plan.K, torch.int32)
        self.t_pair_slack = buf(plan.K * plan.K)
        self._t_delay = None
        self.t_arr = buf(nb * plan.K)
        self.t_req = buf(nb * plan.R)
        self.t_slack = buf(nc)
        self.t_crit = buf(nc)
        # (ratio bits << 32) | achieved-period bits, see stc_pairs
        self.t_worst = buf(1, torch.int64)
        self.t_period = buf(1)
        self.lib = _lib()
        self._args = self._build_args()

    @property
    def num_conns(self):
        return self.netlist.num_conns

    def owned_buffers(self):
        """Every tensor analyze_device writes."""
        return (self.t_arr, self.t_req, self.t_slack, self.t_crit,
                self.t_worst, self.t_period)

    def _build_args(self):
        g = self.gsta
        a = StaConstrainedArgs()
        pt = lambda t: ct.c_void_p(t.data_ptr())
        a.level_blocks = pt(g.t_level_blocks)
        a.in_ptr = pt(g.t_in_ptr); a.in_conn = pt(g.t_in_conn)
        a.out_ptr = pt(g.t_out_ptr); a.out_conn = pt(g.t_out_conn)
        a.conn_driver = pt(g.t_conn_driver)
        a.conn_sink = pt(g.t_conn_sink)
        a.is_seq = pt(g.t_is_seq)
        a.blk_delay = (pt(g.t_blk_delay)
                       if g.t_blk_delay is not None else None)
        a.block_clock = pt(self.t_block_clock)
        a.T_clb = self.arch.T_clb; a.T_seq_out = self.arch.T_seq_out
        a.T_seq_in = self.arch.T_seq_in; a.max_crit = self.max_crit
        a.num_blocks = self.netlist.num_blocks
        a.num_levels = g.num_levels
        a.K = self.K; a.R = self.R
        a.num_conns = self.netlist.num_conns
        a.cons = pt(self.t_cons); a.pair_row = pt(self.t_pair_row)
        a.skip = pt(self.t_skip)
        a.req_period = pt(self.t_req_period)
        a.req_domain = pt(self.t_req_domain)
        a.arr = pt(self.t_arr); a.req = pt(self.t_req)
        a.slack = pt(self.t_slack); a.crit = pt(self.t_crit)
        a.worst_bits = pt(self.t_worst); a.period_out = pt(self.t_period)
        a.level_start_host = g.level_start_host.ctypes.data_as(ct.c_void_p)
        a.launch = pt(self.t_launch) if self.t_launch is not None else None
        a.capture = (pt(self.t_capture) if self.t_capture is not None
                     else None)
        return a

    def analyze_device(self, t_conn_delay):
        """Device path: conn delays in, (period_t, slack_t, crit_t) out, all
        device tensors of this engine, valid in stream order."""
        t = t_conn_delay
        if (not t.is_cuda or t.dtype != self.torch.float32
                or t.numel() != self.netlist.num_conns
                or not t.is_contiguous()):
            raise ValueError("analyze_device: need a contiguous device "
                             f"float32 tensor of {self.netlist.num_conns} "
                             "connection delays")
        self._args.delay = ct.c_void_p(t.data_ptr())
        self._t_delay = t
        stream = self.torch.cuda.current_stream().cuda_stream
        rc = self.lib.pnr_sta_constrained(ct.byref(self._args), stream)
        hip_api.check(rc, "sta_constrained")
        return self.t_period, self.t_slack, self.t_crit

    def analyze(self, conn_delay):
        """Host-compatible API (numpy in/out): (worst_achieved_period,
        slack[], crit[])."""
        torch = self.torch
        t_delay = torch.from_numpy(
            np.ascontiguousarray(conn_delay, dtype=np.float32)).to(self.device)
        self.analyze_device(t_delay)
        torch.cuda.synchronize(self.device)
        return (float(self.t_period.item()), self.t_slack.cpu().numpy(),
                self.t_crit.cpu().numpy())

    def pair_slack(self):
        """Least slack per (source, sink) clock pair of the last analysis:
        numpy [K, K] float32, +inf for a false pair or one that reaches no
        connection; ConstrainedSTA.pair_slack() bit for bit. Two launches
        (stc_pair_slack, stc_pair_slack_finish) and a synchronisation:
        for reports, not for the loops. The delay tensor of the last
        analyze_device must not have been written since."""
        if self._t_delay is None:
            raise RuntimeError("pair_slack() needs an analysis first")
        stream = self.torch.cuda.current_stream().cuda_stream
        rc = self.lib.pnr_sta_pair_slack(
            ct.byref(self._args), ct.c_void_p(self.t_pair_bits.data_ptr()),
            ct.c_void_p(self.t_pair_slack.data_ptr()), stream)
        hip_api.check(rc, "sta_pair_slack")
        self.torch.cuda.synchronize(self.device)
        return self.t_pair_slack.cpu().numpy().reshape(self.K, self.K)

    def arr_rows(self):
        """Arrival per (source domain, block), numpy [K, num_blocks]."""
        nb = self.netlist.num_blocks
        return np.ascontiguousarray(
            self.t_arr.cpu().numpy().reshape(nb, self.K).T)

    def req_rows(self):
        """Required time per (backward row, block), numpy [R, num_blocks]."""
        nb = self.netlist.num_blocks
        return np.ascontiguousarray(
            self.t_req.cpu().numpy().reshape(nb, self.R).T)
