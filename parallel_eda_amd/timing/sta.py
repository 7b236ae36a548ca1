"""Static timing analysis wrapper.

Reference semantics: vpr/SRC/timing/path_delay.c:1994 do_timing_analysis_new
(T_arr forward max-plus per level, T_req backward, slack, criticality) and
router glue router.cxx:27-40 analyze_timing. CPU engine in
csrc/cpu/sta_serial.cpp; GPU engine runs the same levelized sweeps as HIP
kernels (csrc/hip/sta_kernel.hip).
"""
import numpy as np

from ..arch.archdef import ArchDef
from .. import ops


def block_delays(netlist, arch: ArchDef):
    """Per-block combinational delay by block type (CLB/RAM/DSP), or None
    for a homogeneous arch (scalar T_clb path)."""
    if not arch.is_heterogeneous():
        return None
    bt = np.asarray(netlist.block_type)
    bd = np.full(len(bt), arch.T_clb, dtype=np.float32)
    for t in (2, 3):  # BLK_RAM, BLK_DSP
        bd[bt == t] = arch.block_delay_of(t)
    return bd


class STA:
    def __init__(self, netlist, arch: ArchDef):
        cpu = ops.cpu()
        self.netlist = netlist
        self.arch = arch
        bd = block_delays(netlist, arch)
        if bd is None:
            bd = np.empty(0, dtype=np.float32)
        self.tg = cpu.TimingGraph(netlist.cpp(), arch.T_clb, arch.T_seq_out,
                                  arch.T_seq_in, bd)

    @property
    def num_levels(self):
        return self.tg.num_levels()

    def analyze(self, conn_delay):
        """Returns (critical_path_delay, slack[], crit[]) per connection."""
        conn_delay = np.ascontiguousarray(conn_delay, dtype=np.float32)
        cpd, slack, crit = self.tg.analyze(conn_delay)
        return float(cpd), np.asarray(slack), np.asarray(crit)

    def analyze_domains(self, conn_delay, block_clock, periods,
                        pair_skip=None, pair_mult=None, launch=None,
                        capture=None, pair_slack=False):
        """Multi-clock analysis (reference: do_timing_analysis_new per
        (src,sink)-domain pairs). block_clock: per-block domain id (-1
        comb); periods: seconds per domain. pair_skip / pair_mult:
        optional KxK (src,sink)-pair constraint arrays from SDC
        set_false_path / set_multicycle_path (reference read_sdc.c).
        launch / capture: optional float32 per-block tables
        (constraints.constraint_plan): a sequential block launches at
        launch[b] instead of T_seq_out, an endpoint requires its
        constraint minus capture[b] instead of T_seq_in (SDC
        set_input_delay / set_output_delay on pads).
        Returns (worst_achieved_period, slack[], crit[]) — slack/crit
        are the worst/max over analyzed domain pairs. With pair_slack a
        fourth item: the [K, K] float32 least slack per (src, sink) pair,
        +inf where the pair is false or reaches no connection."""
        conn_delay = np.ascontiguousarray(conn_delay, dtype=np.float32)
        bc = np.ascontiguousarray(block_clock, dtype=np.int32)
        pr = np.ascontiguousarray(periods, dtype=np.float32)
        if pair_skip is not None:
            pair_skip = np.ascontiguousarray(pair_skip, dtype=np.uint8)
        if pair_mult is not None:
            pair_mult = np.ascontiguousarray(pair_mult, dtype=np.float32)
        if launch is not None:
            launch = np.ascontiguousarray(launch, dtype=np.float32)
        if capture is not None:
            capture = np.ascontiguousarray(capture, dtype=np.float32)
        out = self.tg.analyze_domains(conn_delay, bc, pr, pair_skip,
                                      pair_mult, launch=launch,
                                      capture=capture,
                                      pair_slack=bool(pair_slack))
        res = (float(out[0]), np.asarray(out[1]), np.asarray(out[2]))
        if pair_slack:
            K = len(pr)
            res += (np.asarray(out[3]).reshape(K, K),)
        return res


class ConstrainedSTA(STA):
    """The place and route loops' CPU engine under clock-pair constraints:
    analyze() is analyze_domains with the stored block_clock, periods,
    false pairs and multicycle multipliers. The "cpd" it returns is the
    worst achieved period (the achieved period of the pair with the
    largest achieved/constraint ratio; periods[0] if no pair is
    analysable), slack the minimum and crit the maximum over the analysed
    pairs, each pair's crit normalised by its own constraint."""

    def __init__(self, netlist, arch: ArchDef, block_clock, periods,
                 pair_skip=None, pair_mult=None, launch_extra=None,
                 capture_extra=None):
        from .constraints import constraint_plan, check_block_clock
        super().__init__(netlist, arch)
        self.plan = constraint_plan(
            periods, pair_skip, pair_mult, launch_extra=launch_extra,
            capture_extra=capture_extra, T_seq_out=arch.T_seq_out,
            T_seq_in=arch.T_seq_in, block_is_seq=netlist.block_is_seq)
        self._pair_slack = None
        self.block_clock = check_block_clock(block_clock, netlist.num_blocks,
                                             self.plan.K)
        self.periods = self.plan.periods
        K = self.plan.K
        self.pair_skip = (None if pair_skip is None
                          else self.plan.skip.reshape(K, K))
        self.pair_mult = (None if pair_mult is None
                          else self.plan.mult.reshape(K, K))

    @property
    def num_conns(self):
        return self.netlist.num_conns

    def analyze(self, conn_delay):
        """Returns (worst_achieved_period, slack[], crit[])."""
        wp, slack, crit, self._pair_slack = self.analyze_domains(
            conn_delay, self.block_clock, self.periods, self.pair_skip,
            self.pair_mult, launch=self.plan.launch,
            capture=self.plan.capture, pair_slack=True)
        return wp, slack, crit

    def pair_slack(self):
        """Least slack per (source, sink) clock pair of the last analyze():
        [K, K] float32, +inf for a false pair or one that reaches no
        connection."""
        if self._pair_slack is None:
            raise RuntimeError("pair_slack() needs an analyze() first")
        return self._pair_slack
