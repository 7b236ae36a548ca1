"""Clock-pair timing constraints for the place and route loops.

Host side of the constrained engines (timing.sta.ConstrainedSTA,
timing.gpu_sta.GpuConstrainedSTA): the SDC clocks, false paths and
multicycle paths as the (block_clock, periods, pair_skip, pair_mult) that
TimingGraph.analyze_domains takes, and the tables the device kernels
(csrc/hip/sta_constrained.hip) read instead of recomputing them.
"""
from types import SimpleNamespace

import numpy as np

MAX_DOMAINS = 64        # the multi-domain kernels' limit


class Constraints:
    """What a constrained engine is built from. pair_skip / pair_mult are
    KxK (source, sink) arrays or None (no false pair / all single cycle).

    launch_extra / capture_extra: per-block seconds or None (SDC
    set_input_delay / set_output_delay): added to the launch time of a
    sequential block and to its setup margin. clock_names: the domain
    names, netlist clocks first, then virtual clocks. Iteration yields the
    first four items only; io_kwargs() the two arrays for an engine."""

    def __init__(self, block_clock, periods, pair_skip=None, pair_mult=None,
                 launch_extra=None, capture_extra=None, clock_names=None):
        self.block_clock = block_clock
        self.periods = periods
        self.pair_skip = pair_skip
        self.pair_mult = pair_mult
        self.launch_extra = launch_extra
        self.capture_extra = capture_extra
        self.clock_names = clock_names

    def __iter__(self):
        return iter((self.block_clock, self.periods, self.pair_skip,
                     self.pair_mult))

    def io_kwargs(self):
        """The keywords ConstrainedSTA / GpuConstrainedSTA take besides
        the four iterated items."""
        return dict(launch_extra=self.launch_extra,
                    capture_extra=self.capture_extra)


def as_constraints(c, **kw):
    """Constraints from a Constraints, a dict with its keys (all but
    block_clock and periods optional) or a (block_clock, periods[, skip[,
    mult]]) sequence; launch_extra, capture_extra and clock_names also as
    keywords."""
    if isinstance(c, Constraints):
        if not kw:
            return c
        c = dict(block_clock=c.block_clock, periods=c.periods,
                 pair_skip=c.pair_skip, pair_mult=c.pair_mult,
                 launch_extra=c.launch_extra, capture_extra=c.capture_extra,
                 clock_names=c.clock_names)
    if isinstance(c, dict):
        extra = {k: c.get(k) for k in ("launch_extra", "capture_extra",
                                       "clock_names")}
        extra.update(kw)
        return Constraints(c["block_clock"], c["periods"],
                           c.get("pair_skip"), c.get("pair_mult"), **extra)
    return Constraints(*c, **kw)


def _block_table(extra, scalar, seq, what):
    """float32(scalar) + float32(extra[b]), rounded once."""
    nb = len(seq)
    if extra is None:
        e = np.zeros(nb, dtype=np.float32)
    else:
        e = np.asarray(extra)
        if e.ndim != 1 or e.shape[0] != nb:
            raise ValueError(f"{what} must have {nb} entries, "
                             f"got shape {e.shape}")
        e = np.ascontiguousarray(e, dtype=np.float32)
        if not (np.isfinite(e).all() and (e >= 0).all()):
            raise ValueError(f"{what} must be finite and not negative")
        if (e[~seq] != 0).any():
            raise ValueError(f"{what} is non-zero on a combinational block")
    t = np.float32(scalar) + e                   # float32 + float32, once
    assert t.dtype == np.float32
    return t


def constraint_plan(periods, pair_skip=None, pair_mult=None,
                    launch_extra=None, capture_extra=None, T_seq_out=None,
                    T_seq_in=None, block_is_seq=None):
    """The host-made tables of one constrained analysis, K = len(periods):

      cons[K*K]      float32  setup constraint of pair (ci, cj):
                              float32(periods[cj]) * float32(mult[ci, cj]),
                              rounded once, here
      req_period[R], req_domain[R]
                              the backward rows: rows 0..K-1 are
                              (cj, periods[cj]); then one row per distinct
                              (cj, mult) with mult != 1, in (ci, cj) order
                              of first use (TimingGraph.analyze_domains'
                              req_mult map)
      pair_row[K*K]  int32    the backward row pair (ci, cj) reads
      skip[K*K]      uint8    false pair
      launch[nb], capture[nb]
                     float32  per block: float32(T_seq_out) +
                              float32(launch_extra[b]) and
                              float32(T_seq_in) + float32(capture_extra[b]),
                              rounded once, here; both None when both
                              extras are None (the engines then use the
                              scalars). They need T_seq_out, T_seq_in and
                              block_is_seq.

    Raises ValueError on K outside 1..64, wrong shapes, a period or
    multiplier that is not positive and finite, or an extra of the wrong
    length, with a negative or non-finite value, or non-zero on a
    combinational block."""
    per = np.asarray(periods)
    if per.ndim != 1:
        raise ValueError("periods must be one-dimensional")
    K = int(per.shape[0])
    if K < 1 or K > MAX_DOMAINS:
        raise ValueError(f"need 1..{MAX_DOMAINS} clock domains, got {K}")
    per = np.ascontiguousarray(per, dtype=np.float32)
    if not (np.isfinite(per).all() and (per > 0).all()):
        raise ValueError("periods must be positive and finite")

    def pairs(a, dtype, what):
        a = np.asarray(a)
        if a.shape not in ((K, K), (K * K,)):
            raise ValueError(f"{what} must be {K}x{K}, got shape {a.shape}")
        return np.ascontiguousarray(a, dtype=dtype).reshape(K * K)

    if pair_skip is None:
        skip = np.zeros(K * K, dtype=np.uint8)
    else:
        skip = (pairs(pair_skip, np.uint8, "pair_skip") != 0).astype(np.uint8)
    if pair_mult is None:
        mult = np.ones(K * K, dtype=np.float32)
    else:
        mult = pairs(pair_mult, np.float32, "pair_mult")
        if not (np.isfinite(mult).all() and (mult > 0).all()):
            raise ValueError("pair_mult must be positive and finite")
    cj_of = np.tile(np.arange(K, dtype=np.int32), K)
    cons = per[cj_of] * mult                     # float32 * float32, once
    assert cons.dtype == np.float32
    if not np.isfinite(cons).all() or not (cons > 0).all():
        raise ValueError("a period times its multiplier left float32 range")
    req_period = list(per)
    req_domain = list(range(K))
    pair_row = cj_of.copy()
    rows = {}
    for p in range(K * K):
        if mult[p] == np.float32(1.0):
            continue
        key = (int(cj_of[p]), float(mult[p]))
        if key not in rows:
            rows[key] = len(req_period)
            req_period.append(cons[p])
            req_domain.append(key[0])
        pair_row[p] = rows[key]
    launch = capture = None
    if launch_extra is not None or capture_extra is not None:
        if T_seq_out is None or T_seq_in is None or block_is_seq is None:
            raise ValueError("launch_extra / capture_extra need T_seq_out, "
                             "T_seq_in and block_is_seq")
        seq = np.asarray(block_is_seq).astype(bool)
        launch = _block_table(launch_extra, T_seq_out, seq, "launch_extra")
        capture = _block_table(capture_extra, T_seq_in, seq, "capture_extra")
    return SimpleNamespace(
        launch=launch, capture=capture,
        K=K, R=len(req_period), periods=per, cons=cons,
        req_period=np.asarray(req_period, dtype=np.float32),
        req_domain=np.asarray(req_domain, dtype=np.int32),
        pair_row=pair_row.astype(np.int32), skip=skip, mult=mult)


def check_block_clock(block_clock, num_blocks, K):
    """block_clock as int32[num_blocks] with every id in [-1, K). A
    sequential block with -1 is legal and belongs to no domain."""
    bc = np.asarray(block_clock)
    if bc.ndim != 1 or bc.shape[0] != num_blocks:
        raise ValueError(f"block_clock must have {num_blocks} entries, "
                         f"got shape {bc.shape}")
    if bc.dtype.kind not in "iu":
        raise ValueError("block_clock must be an integer array")
    if num_blocks and (bc.min() < -1 or bc.max() >= K):
        raise ValueError(f"block_clock ids must lie in [-1, {K})")
    return np.ascontiguousarray(bc, dtype=np.int32)


def sdc_periods(sdc_clocks, clock_names):
    """Period per netlist clock domain: the SDC clock of that name, or the
    first SDC clock for a domain the file does not name; the first SDC
    clock alone for a netlist without clock names."""
    first = list(sdc_clocks.values())[:1]
    return [sdc_clocks.get(c, first[0]) for c in clock_names] or first


def constraints_from_sdc(sdc, netlist):
    """Constraints of a netlist from parse_sdc_constraints output. The pair
    arrays are None unless the file has a false or multicycle path."""
    from .report import pair_constraints
    if not sdc or not sdc.get("clocks"):
        raise ValueError("the SDC file defines no clock")
    bc = getattr(netlist, "block_clock", None)
    if bc is None:
        raise ValueError("the netlist has no block_clock (clock domains)")
    cnames = getattr(netlist, "clock_names", []) or []
    io_delays = sdc.get("io_delays") or []
    groups = sdc.get("clock_groups") or []
    if io_delays or groups:
        return _io_constraints(sdc, netlist, list(cnames), io_delays, groups)
    periods = sdc_periods(sdc["clocks"], cnames)
    ps = pm = None
    if sdc.get("false_paths") or sdc.get("multicycle"):
        ps, pm = pair_constraints(sdc, cnames)
    return Constraints(bc, periods, ps, pm)


def port_blocks(netlist):
    """({port name: block} of the input pads, the same of the output
    pads). A port is a block of type IO; its name is the netlist name
    without the ipad: / opad: prefix; a pad that drives a net is an input,
    one that is a sink an output."""
    from ..arch.archdef import BLK_IO
    bt = np.asarray(netlist.block_type)
    names = getattr(netlist, "names", None) or \
        [f"blk_{i}" for i in range(len(bt))]
    drives = set(np.asarray(netlist.net_driver).tolist())
    sinks = set(np.asarray(netlist.net_sinks).tolist())
    ins, outs = {}, {}
    for b in np.nonzero(bt == BLK_IO)[0].tolist():
        nm = names[b]
        for prefix in ("ipad:", "opad:"):
            if nm.startswith(prefix):
                nm = nm[len(prefix):]
                break
        if b in drives:
            ins[nm] = b
        if b in sinks:
            outs[nm] = b
    return ins, outs


def _io_constraints(sdc, netlist, cnames, io_delays, groups):
    """constraints_from_sdc for a file with set_input_delay /
    set_output_delay / set_clock_groups lines (reference read_sdc.c)."""
    import re
    from .report import pair_constraints
    clocks = sdc["clocks"]
    names = list(cnames)
    for (_kind, clk, _v, _pat) in io_delays:
        if clk not in clocks:
            raise ValueError(f"I/O delay against clock '{clk}', which no "
                             f"create_clock defines")
        if clk not in names:
            names.append(clk)                    # virtual: no latch uses it
    if len(names) > MAX_DOMAINS:
        raise ValueError(f"{len(names)} clock domains with the virtual "
                         f"clocks, at most {MAX_DOMAINS}")
    idx = {c: i for i, c in enumerate(names)}
    periods = sdc_periods(clocks, names)
    nb = len(netlist.block_type)
    bc = np.array(netlist.block_clock, dtype=np.int32, copy=True)
    launch_extra = np.zeros(nb, dtype=np.float32)
    capture_extra = np.zeros(nb, dtype=np.float32)
    ins, outs = port_blocks(netlist)
    if io_delays:
        from ..arch.archdef import BLK_IO
        bc[np.asarray(netlist.block_type) == BLK_IO] = -1   # unmatched pads
    for (kind, clk, seconds, patterns) in io_delays:
        if not (np.isfinite(seconds) and seconds >= 0):
            raise ValueError(f"set_{kind}_delay {seconds * 1e9:g} ns: need "
                             f"a finite delay that is not negative")
        ports = ins if kind == "input" else outs
        extra = launch_extra if kind == "input" else capture_extra
        if patterns is None:
            hit = list(ports.values())
        else:
            hit = []
            for pat in patterns:
                try:
                    rx = re.compile(pat)
                except re.error as e:
                    raise ValueError(f"bad port pattern '{pat}': {e}")
                m = [b for nm, b in ports.items() if rx.fullmatch(nm)]
                if not m:
                    raise ValueError(f"set_{kind}_delay: '{pat}' matches "
                                     f"no {kind} port")
                hit += m
        for b in hit:
            bc[b] = idx[clk]
            extra[b] = seconds
    ps, pm = pair_constraints(sdc, names)
    for entry in groups:
        ids = [[idx[c] for c in grp if c in idx] for grp in entry]
        for ga, a in enumerate(ids):
            for gb, b in enumerate(ids):
                if ga != gb:
                    for i in a:
                        for j in b:
                            if i != j:
                                ps[i, j] = 1
    return Constraints(bc, periods, ps, pm,
                       launch_extra if io_delays else None,
                       capture_extra if io_delays else None, names)
