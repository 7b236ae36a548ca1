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
    KxK (source, sink) arrays or None (no false pair / all single cycle)."""

    def __init__(self, block_clock, periods, pair_skip=None, pair_mult=None):
        self.block_clock = block_clock
        self.periods = periods
        self.pair_skip = pair_skip
        self.pair_mult = pair_mult

    def __iter__(self):
        return iter((self.block_clock, self.periods, self.pair_skip,
                     self.pair_mult))


def as_constraints(c):
    """Constraints from a Constraints, a dict with its four keys (the pair
    arrays optional) or a (block_clock, periods[, skip[, mult]]) sequence."""
    if isinstance(c, Constraints):
        return c
    if isinstance(c, dict):
        return Constraints(c["block_clock"], c["periods"],
                           c.get("pair_skip"), c.get("pair_mult"))
    return Constraints(*c)


def constraint_plan(periods, pair_skip=None, pair_mult=None):
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

    Raises ValueError on K outside 1..64, wrong shapes, or a period or
    multiplier that is not positive and finite."""
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
    return SimpleNamespace(
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
    periods = sdc_periods(sdc["clocks"], cnames)
    ps = pm = None
    if sdc.get("false_paths") or sdc.get("multicycle"):
        ps, pm = pair_constraints(sdc, cnames)
    return Constraints(bc, periods, ps, pm)
