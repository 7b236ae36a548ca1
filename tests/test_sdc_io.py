"""SDC I/O constraints in the timing engines: set_input_delay /
set_output_delay on ports, virtual clocks, set_clock_groups and the least
slack per clock pair (timing/report.py, timing/constraints.py,
TimingGraph.analyze_domains' launch / capture / pair_slack, the CLI's
--sdc_report). CPU only; tests/test_gpu_sdc_io.py holds the device side to
what is computed here.

Oracles:

* a hand case: pad -> comb -> flip-flop -> comb -> pad with 1 ns per
  connection, slacks written out in float64. The engine adds and subtracts
  at most six fp32 values of at most 10 ns, so it must be within
  8 * 2^-24 * 10 ns of them;
* `replay_io`: tests/test_sta_constrained.py's numpy float32 replay of the
  device algorithm with the per-block `launch` / `capture` tables of
  `constraint_plan` in place of the scalars, plus the per-pair minimum. It
  equals `STA.analyze_domains(..., launch=, capture=, pair_slack=True)` bit
  for bit, and is the only oracle for the device `arr` / `req` rows.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from parallel_eda_amd.arch.archdef import get_arch
from parallel_eda_amd.io.blif import parse_blif
from parallel_eda_amd.io.pack import pack_blif
from parallel_eda_amd.io.synth import NetlistPy
from parallel_eda_amd.timing.constraints import (Constraints, as_constraints,
                                                 constraint_plan,
                                                 constraints_from_sdc)
from parallel_eda_amd.timing.report import (parse_sdc_constraints,
                                            write_pair_slack_report)
from parallel_eda_amd.timing.sta import STA, ConstrainedSTA

from test_sta_exact import _same_bits, _ragged, _consts, F, K
from test_sta_constrained import (CPU_GRAPHS, NEG, POS, constraint_set,
                                  setup_of, replay)
from test_sdc_driven import BLIF2, _two_clock_files

IO_SETS = ("none", "false_and_mc", "mc_shared")
INF = F(np.inf)


# ------------------------------------------------------------- 1. the parser

def test_parser_io_delays_and_groups():
    sdc = parse_sdc_constraints("""
create_clock -period 5.0 -name clkA
create_clock -period 8.0 -name vclk
set_input_delay -clock vclk -max 1.5 [get_ports {a b}]
set_input_delay -clock clkA 0.25 [get_ports c]   # no braces
set_output_delay -clock vclk 2 [get_ports {y.*}]
set_output_delay -clock clkA -max 0.5
set_output_delay -clock clkA -min 0.1 [get_ports {y}]
set_clock_groups -exclusive -group {clkA vclk} -group {clkB} -group clkC
set_clock_groups -exclusive -group {clkA} -group {vclk}
""")
    io = sdc["io_delays"]
    assert [(k, c, p) for (k, c, _v, p) in io] == [
        ("input", "vclk", ["a", "b"]), ("input", "clkA", ["c"]),
        ("output", "vclk", ["y.*"]), ("output", "clkA", None)]
    assert [v for (_k, _c, v, _p) in io] == pytest.approx(
        [1.5e-9, 0.25e-9, 2e-9, 0.5e-9], rel=1e-12)
    assert sdc["clock_groups"] == [[["clkA", "vclk"], ["clkB"], ["clkC"]],
                                   [["clkA"], ["vclk"]]]
    # -clock * names the only clock; with two clocks it stays '*'
    one = parse_sdc_constraints("create_clock -period 4 -name c\n"
                                "set_input_delay -clock * 1.0\n")
    assert one["io_delays"] == [("input", "c", pytest.approx(1e-9), None)]
    two = parse_sdc_constraints("create_clock -period 4 -name c\n"
                                "create_clock -period 5 -name d\n"
                                "set_output_delay -clock * -max 1.0\n")
    assert two["io_delays"][0][1] == "*"
    none = parse_sdc_constraints("create_clock -period 4 -name c\n")
    assert none["io_delays"] == [] and none["clock_groups"] == []


def test_parser_old_keys_unchanged():
    """The input of tests/test_sta.py: every old key keeps its value."""
    sdc = parse_sdc_constraints("""
create_clock -period 5.0 -name clkA
create_clock -period 8.0 -name clkB
set_false_path -from [get_clocks clkA] -to [get_clocks clkB]
set_multicycle_path 2 -from [get_clocks clkB] -to [get_clocks clkA]
set_input_delay -clock clkA 1.0
""")
    assert sdc["clocks"] == {"clkA": 5e-9, "clkB": 8e-9}
    assert sdc["false_paths"] == [("clkA", "clkB")]
    assert sdc["multicycle"] == [("clkB", "clkA", 2)]
    assert set(sdc["input_delay"]) == {"clkA"}
    assert abs(sdc["input_delay"]["clkA"] - 1e-9) < 1e-15
    assert sdc["output_delay"] == {}
    assert sdc["io_delays"] == [("input", "clkA", pytest.approx(1e-9), None)]
    assert sdc["clock_groups"] == []


# ---------------------------------------------------------- 2. the hand case

HAND_SDC = """
create_clock -period 10.0 -name clk
create_clock -period 8.0 -name vclk
set_input_delay -clock vclk -max 2.0 [get_ports {din}]
set_output_delay -clock vclk 1.5 [get_ports dout]
"""


def hand_netlist():
    """din(0) -> n1(1) -> ff(2) -> n2(3) -> dout(4); the spare pad 5 also
    feeds n1 and no SDC line names it. Connections in net order:
    0: din->n1, 1: n1->ff, 2: ff->n2, 3: n2->dout, 4: spare->n1."""
    nl = NetlistPy([0, 1, 1, 1, 0, 0], [1, 0, 1, 0, 1, 1], [0, 1, 2, 3, 5],
                   [0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 1],
                   names=["ipad:din", "n1", "ff", "n2", "opad:dout",
                          "ipad:spare"])
    nl.block_clock = np.asarray([0, -1, 0, -1, 0, 0], np.int32)
    nl.clock_names = ["clk"]
    return nl


def test_hand_case_pad_paths():
    arch = get_arch("tiny")
    nl = hand_netlist()
    cons = constraints_from_sdc(parse_sdc_constraints(HAND_SDC), nl)
    assert cons.clock_names == ["clk", "vclk"]
    assert cons.block_clock.tolist() == [1, -1, 0, -1, 1, -1]
    assert cons.launch_extra.tolist() == [F(2e-9), 0, 0, 0, 0, 0]
    assert cons.capture_extra.tolist() == [0, 0, 0, 0, F(1.5e-9), 0]
    assert list(cons.periods) == [10e-9, 8e-9]
    eng = ConstrainedSTA(nl, arch, *cons, **cons.io_kwargs())
    d = np.full(nl.num_conns, 1e-9, F)
    wp, slack, crit = eng.analyze(d)
    t_out, t_in, t_clb = (float(arch.T_seq_out), float(arch.T_seq_in),
                          float(arch.T_clb))
    # pad -> ff: launched by vclk 2 ns late, captured by clk (10 ns)
    s_in = (10e-9 - t_in) - ((t_out + 2e-9) + 1e-9 + t_clb + 1e-9)
    # ff -> pad: launched by clk, the board needs it 1.5 ns before vclk
    s_out = (8e-9 - (t_in + 1.5e-9)) - (t_out + 1e-9 + t_clb + 1e-9)
    tol = 8 * 2.0 ** -24 * 10e-9
    assert slack[0] == pytest.approx(s_in, abs=tol)
    assert slack[1] == pytest.approx(s_in, abs=tol)
    assert slack[2] == pytest.approx(s_out, abs=tol)
    assert slack[3] == pytest.approx(s_out, abs=tol)
    assert crit[0] == pytest.approx(1 - s_in / 10e-9, abs=1e-6)
    assert crit[3] == pytest.approx(1 - s_out / 8e-9, abs=1e-6)
    # the pad no line names is not analysed
    assert slack[4] == 0 and crit[4] == 0
    # the tighter of the two binds
    ratio_in, ratio_out = (10e-9 - s_in) / 10e-9, (8e-9 - s_out) / 8e-9
    want = 10e-9 - s_in if ratio_in > ratio_out else 8e-9 - s_out
    assert wp == pytest.approx(want, abs=tol)
    ps = eng.pair_slack()
    assert ps.shape == (2, 2) and ps.dtype == np.float32
    assert ps[1, 0] == slack[0] and ps[0, 1] == slack[2]
    assert ps[0, 0] == INF and ps[1, 1] == INF
    # without the I/O lines every pad is a flip-flop of domain 0
    plain = constraints_from_sdc(
        parse_sdc_constraints("create_clock -period 10.0 -name clk\n"), nl)
    _, s0, _ = ConstrainedSTA(nl, arch, *plain).analyze(d)
    assert s0[4] != 0 and s0[0] == pytest.approx(s_in + 2e-9, abs=tol)


# ------------------------------------------------------------ 3. the replay

def io_extras(nl, periods, seed=5):
    """launch_extra / capture_extra of a graph: non-zero on every third
    sequential block (offset by one between the two), 5 to 40 percent of
    the first period."""
    rng = np.random.default_rng(seed)
    seq = np.nonzero(np.asarray(nl.block_is_seq))[0]
    le = np.zeros(nl.num_blocks, F)
    ce = np.zeros(nl.num_blocks, F)
    a, b = seq[::3], seq[1::3]
    le[a] = (rng.uniform(0.05, 0.4, len(a)) * periods[0]).astype(F)
    ce[b] = (rng.uniform(0.05, 0.4, len(b)) * periods[0]).astype(F)
    return le, ce


def replay_io(nl, arch, tg, delay, bc, plan):
    """test_sta_constrained.replay with plan.launch / plan.capture in place
    of T_seq_out / T_seq_in, and the least slack per pair. Null tables
    replay the scalars."""
    blocks, start = tg.level_arrays()
    in_ptr, in_conn, out_ptr, out_conn, drv = tg.csr_arrays()
    snk = nl.net_sinks
    seq = nl.block_is_seq.astype(bool)
    bd, t_out, t_in = _consts(nl, arch)
    delay = np.ascontiguousarray(delay, F)
    bc = np.asarray(bc)
    nb, nc = nl.num_blocks, nl.num_conns
    k_, r_ = plan.K, plan.R
    L = len(start) - 1
    launch = plan.launch if plan.launch is not None else np.full(nb, t_out, F)
    capture = (plan.capture if plan.capture is not None
               else np.full(nb, t_in, F))
    assert launch.dtype == F and capture.dtype == F

    arr = np.full((k_, nb), NEG, F)
    for lv in range(L):
        b = blocks[start[lv]:start[lv + 1]]
        ff, comb = b[seq[b]], b[~seq[b]]
        arr[:, ff] = np.where(bc[ff][None, :] == np.arange(k_)[:, None],
                              launch[ff][None, :], NEG)
        pos, own = _ragged(in_ptr, comb)
        c = in_conn[pos]
        for ci in range(k_):
            v = arr[ci, drv[c]]
            v = np.where(v > NEG, v + delay[c], v).astype(F)
            m = np.full(len(comb), NEG, F)
            np.maximum.at(m, own, v)
            arr[ci, comb] = np.where(m > NEG, m + bd[comb], NEG)

    req = np.full((r_, nb), POS, F)
    for lv in range(L - 1, -1, -1):
        b = blocks[start[lv]:start[lv + 1]]
        pos, own = _ragged(out_ptr, b)
        c = out_conn[pos]
        s = snk[c]
        for row in range(r_):
            r = req[row, s]
            ep = (plan.req_period[row] - capture[s]).astype(F)
            ri = np.where(seq[s],
                          np.where(bc[s] == plan.req_domain[row], ep, POS),
                          np.where(r < POS, r - bd[s], POS)).astype(F)
            ri = np.where(ri < POS, ri - delay[c], ri).astype(F)
            m = np.full(len(b), POS, F)
            np.minimum.at(m, own, ri)
            req[row, b] = m

    slack = np.full(nc, POS, F)
    crit = np.zeros(nc, F)
    pair_slack = np.full(k_ * k_, INF, F)
    worst_ratio, worst_period, top = F(0), plan.periods[0], set()
    for pair in range(k_ * k_):
        if plan.skip[pair]:
            continue
        ci, cj = divmod(pair, k_)
        cons = plan.cons[pair]
        a = arr[ci, drv]
        r = req[plan.pair_row[pair], snk]
        ri = np.where(seq[snk],
                      np.where(bc[snk] == cj, cons - capture[snk], POS),
                      np.where(r < POS, r - bd[snk], POS)).astype(F)
        ok = np.nonzero((a > NEG) & (ri < POS))[0]
        if not len(ok):
            continue
        s = (ri[ok] - (a[ok] + delay[ok])).astype(F)
        pair_slack[pair] = s.min()
        slack[ok] = np.minimum(slack[ok], s)
        cr = (F(1) - s / cons).astype(F)
        crit[ok] = np.maximum(crit[ok], np.clip(cr, F(0), F(1)))
        achieved = (cons - s).astype(F)
        ratio = (achieved / cons).astype(F)
        if ratio.max() > worst_ratio:
            worst_ratio = ratio.max()
            worst_period = achieved[np.argmax(ratio)]
            top = set()
        if ratio.max() == worst_ratio and worst_ratio > 0:
            top |= set(achieved[ratio == worst_ratio].tolist())
    slack[slack >= POS] = 0
    assert arr.dtype == F and req.dtype == F and slack.dtype == F
    return SimpleNamespace(arr=arr, req=req, slack=slack, crit=crit,
                           wp=F(worst_period), top=top,
                           pair_slack=pair_slack.reshape(k_, k_))


def plan_of(cs, periods, skip, mult, le, ce):
    return constraint_plan(periods, skip, mult, launch_extra=le,
                           capture_extra=ce, T_seq_out=cs.arch.T_seq_out,
                           T_seq_in=cs.arch.T_seq_in,
                           block_is_seq=cs.nl.block_is_seq)


@functools.lru_cache(maxsize=None)
def expected_io(name, set_name, tables=True):
    """CPU engine and replay of one (graph, constraint set) with the I/O
    tables (or, tables=False, without: today's analysis), computed once."""
    cs, bc, periods, d = setup_of(name)
    skip, mult = constraint_set(set_name)
    le, ce = io_extras(cs.nl, periods) if tables else (None, None)
    plan = plan_of(cs, periods, skip, mult, le, ce)
    wp, slack, crit, ps = cs.sta.analyze_domains(
        d, bc, periods, pair_skip=skip, pair_mult=mult, launch=plan.launch,
        capture=plan.capture, pair_slack=True)
    rp = replay_io(cs.nl, cs.arch, cs.sta.tg, d, bc, plan)
    return SimpleNamespace(cs=cs, bc=bc, periods=periods, d=d, skip=skip,
                           mult=mult, le=le, ce=ce, plan=plan, wp=F(wp),
                           slack=slack, crit=crit, pair_slack=ps, rp=rp)


@pytest.mark.parametrize("name", CPU_GRAPHS)
def test_replay_io_equals_cpu_engine(name):
    for set_name in IO_SETS:
        e = expected_io(name, set_name)
        tag = f"{name}/{set_name}"
        seq = e.cs.nl.block_is_seq.astype(bool)
        assert (e.le[seq][::3] > 0).all() and (e.ce[seq][1::3] > 0).all()
        assert (e.le[~seq] == 0).all() and (e.ce[~seq] == 0).all()
        _same_bits(e.plan.launch, F(e.cs.arch.T_seq_out) + e.le,
                   f"{tag} launch")
        _same_bits(e.plan.capture, F(e.cs.arch.T_seq_in) + e.ce,
                   f"{tag} capture")
        _same_bits(e.rp.slack, e.slack, f"{tag} slack")
        _same_bits(e.rp.crit, e.crit, f"{tag} crit")
        _same_bits(e.rp.wp, e.wp, f"{tag} worst period")
        assert e.pair_slack.shape == (K, K)
        _same_bits(e.rp.pair_slack.ravel(), e.pair_slack.ravel(),
                   f"{tag} pair slack")
        # the table is the minimum of what the connections see
        fin = np.isfinite(e.pair_slack)
        reached = ~((e.slack == 0) & (e.crit == 0))
        if fin.any():
            assert e.pair_slack[fin].min() == e.slack[reached].min(), tag
        assert (e.pair_slack[e.plan.skip.reshape(K, K) != 0] == INF).all()
        # the tables change the answer
        base = expected_io(name, set_name, tables=False)
        assert base.plan.launch is None and base.plan.capture is None
        if reached.any():
            assert (e.slack != base.slack).any(), tag
    # null tables: today's engine and today's replay, bit for bit
    for set_name in IO_SETS:
        base = expected_io(name, set_name, tables=False)
        wp, slack, crit = base.cs.sta.analyze_domains(
            base.d, base.bc, base.periods, pair_skip=base.skip,
            pair_mult=base.mult)
        old = replay(base.cs.nl, base.cs.arch, base.cs.sta.tg, base.d,
                     base.bc, base.plan)
        _same_bits(base.slack, slack, f"{name}/{set_name} null slack")
        _same_bits(base.crit, crit, f"{name}/{set_name} null crit")
        _same_bits(base.rp.arr, old.arr, f"{name}/{set_name} null arr")
        _same_bits(base.rp.req, old.req, f"{name}/{set_name} null req")
        assert F(wp) == base.wp


def test_constrained_sta_passes_tables_and_pair_slack():
    e = expected_io("wide_het", "false_and_mc")
    eng = ConstrainedSTA(e.cs.nl, e.cs.arch, e.bc, e.periods, e.skip, e.mult,
                         launch_extra=e.le, capture_extra=e.ce)
    with pytest.raises(RuntimeError):
        eng.pair_slack()
    wp, slack, crit = eng.analyze(e.d)
    _same_bits(slack, e.slack, "slack")
    _same_bits(crit, e.crit, "crit")
    assert F(wp) == e.wp
    _same_bits(eng.pair_slack().ravel(), e.pair_slack.ravel(), "pair slack")
    # an all-false set: nothing analysed, every entry +inf
    skip, _ = constraint_set("all_false")
    eng = ConstrainedSTA(e.cs.nl, e.cs.arch, e.bc, e.periods, skip, None,
                         launch_extra=e.le, capture_extra=e.ce)
    eng.analyze(e.d)
    assert (eng.pair_slack() == INF).all()


def test_plan_table_errors():
    cs, bc, periods, d = setup_of("chain")
    nl = cs.nl
    seq = nl.block_is_seq.astype(bool)
    ok = np.where(seq, 1e-10, 0.0)
    p = plan_of(cs, periods, None, None, ok, None)
    assert p.launch.dtype == np.float32 and p.capture.dtype == np.float32
    _same_bits(p.capture, np.full(nl.num_blocks, cs.arch.T_seq_in, F),
               "capture without extra")
    assert constraint_plan(periods).launch is None
    comb = int(np.nonzero(~seq)[0][0])
    ff = int(np.nonzero(seq)[0][0])
    for which in ("launch_extra", "capture_extra"):
        for bad in (ok[:-1], np.append(ok, 0.0)):
            with pytest.raises(ValueError):
                plan_of(cs, periods, None, None,
                        *((bad, None) if which[0] == "l" else (None, bad)))
        for v, at in ((-1e-10, ff), (np.nan, ff), (np.inf, ff),
                      (1e-10, comb)):
            bad = ok.copy()
            bad[at] = v
            with pytest.raises(ValueError):
                plan_of(cs, periods, None, None,
                        *((bad, None) if which[0] == "l" else (None, bad)))
    with pytest.raises(ValueError):     # the tables need the block kinds
        constraint_plan(periods, launch_extra=ok)


def test_constraints_keep_their_four_items():
    c = Constraints([0], [1e-9], None, None, launch_extra=[1e-10],
                    clock_names=["c"])
    assert len(list(c)) == 4
    assert c.capture_extra is None and c.clock_names == ["c"]
    assert c.io_kwargs() == dict(launch_extra=[1e-10], capture_extra=None)
    d = as_constraints(dict(block_clock=[0], periods=[1e-9],
                            capture_extra=[2e-10]))
    assert d.capture_extra == [2e-10] and d.launch_extra is None
    k = as_constraints(([0], [1e-9]), launch_extra=[3e-10])
    assert k.launch_extra == [3e-10] and k.pair_skip is None


# ------------------------------------------------- 4. constraints_from_sdc

SDC_IO = """
create_clock -period 8.0 -name clkA
create_clock -period 4.0 -name clkB
create_clock -period 6.0 -name vclk
set_input_delay -clock vclk -max 1.0 [get_ports {a}]
set_output_delay -clock clkA 0.5 [get_ports {y}]
set_clock_groups -exclusive -group {clkA} -group {clkB}
"""


@functools.lru_cache(maxsize=None)
def two_clock_netlist():
    nl, _, _ = pack_blif(parse_blif(BLIF2), get_arch("tiny"), n_ble=2)
    return nl


def test_constraints_from_sdc_io():
    nl = two_clock_netlist()
    names = list(nl.clock_names)
    blk = {n: i for i, n in enumerate(nl.names)}
    c = constraints_from_sdc(parse_sdc_constraints(SDC_IO), nl)
    assert c.clock_names == names + ["vclk"]
    want = {"clkA": 8.0 * 1e-9, "clkB": 4.0 * 1e-9, "vclk": 6.0 * 1e-9}
    assert list(c.periods) == [want[n] for n in c.clock_names]
    assert c.block_clock is not nl.block_clock
    a, y = blk["ipad:a"], blk["opad:y"]
    assert c.block_clock[a] == 2 and c.block_clock[y] == names.index("clkA")
    pads = np.nonzero(np.asarray(nl.block_type) == 0)[0]
    for b in pads:
        if b not in (a, y):
            assert c.block_clock[b] == -1, nl.names[b]
    rest = np.setdiff1d(np.arange(nl.num_blocks), pads)
    assert np.array_equal(c.block_clock[rest],
                          np.asarray(nl.block_clock)[rest])
    assert c.launch_extra[a] == F(1e-9) and c.capture_extra[y] == F(0.5e-9)
    assert np.count_nonzero(c.launch_extra) == 1
    assert np.count_nonzero(c.capture_extra) == 1
    ia, ib = names.index("clkA"), names.index("clkB")
    assert c.pair_skip.shape == (3, 3)
    assert c.pair_skip[ia, ib] == 1 and c.pair_skip[ib, ia] == 1
    assert c.pair_skip.sum() == 2 and (c.pair_mult == 1).all()
    # the engine takes it; the pad paths are analysed against the board
    arch = get_arch("tiny")
    eng = ConstrainedSTA(nl, arch, *c, **c.io_kwargs())
    eng.analyze(np.full(nl.num_conns, 1e-9, F))
    ps = eng.pair_slack()
    assert np.isfinite(ps[2]).any()              # vclk launches something
    assert ps[ia, ib] == INF and ps[ib, ia] == INF
    # false and multicycle paths may name a virtual clock; the last line
    # that matches a port wins
    c2 = constraints_from_sdc(parse_sdc_constraints(
        SDC_IO + "set_false_path -from [get_clocks vclk] -to "
        "[get_clocks clkB]\n"
        "set_multicycle_path 2 -from [get_clocks vclk] -to "
        "[get_clocks clkA]\n"
        "set_input_delay -clock clkB 0.25 [get_ports {a|b}]\n"), nl)
    assert c2.pair_skip[2, ib] == 1 and c2.pair_mult[2, ia] == 2
    assert c2.block_clock[a] == ib and c2.launch_extra[a] == F(0.25e-9)
    assert c2.block_clock[blk["ipad:b"]] == ib
    assert c2.clock_names == names + ["vclk"]
    # no get_ports: every port of that direction
    c3 = constraints_from_sdc(parse_sdc_constraints(
        "create_clock -period 8.0 -name clkA\n"
        "set_output_delay -clock clkA 0.5\n"), nl)
    outs = [blk["opad:y"], blk["opad:z"]]
    assert (c3.capture_extra[outs] == F(0.5e-9)).all()
    assert (c3.block_clock[outs] == ia).all()
    assert c3.block_clock[a] == -1 and np.count_nonzero(c3.launch_extra) == 0
    # a clock group alone: pads keep their domain, no tables
    c4 = constraints_from_sdc(parse_sdc_constraints(
        "create_clock -period 8.0 -name clkA\n"
        "create_clock -period 4.0 -name clkB\n"
        "set_clock_groups -exclusive -group {clkA} -group {clkB}\n"), nl)
    assert np.array_equal(c4.block_clock, nl.block_clock)
    assert c4.launch_extra is None and c4.capture_extra is None
    assert c4.pair_skip.sum() == 2


def test_constraints_from_sdc_errors_and_identity():
    nl = two_clock_netlist()
    head = ("create_clock -period 8.0 -name clkA\n"
            "create_clock -period 4.0 -name clkB\n")
    for bad in (
            "set_input_delay -clock nowhere 1.0 [get_ports a]\n",
            "set_input_delay -clock clkA 1.0 [get_ports {nothing}]\n",
            "set_input_delay -clock clkA 1.0 [get_ports {y}]\n",   # output
            "set_output_delay -clock clkA 1.0 [get_ports {a}]\n",  # input
            "set_input_delay -clock clkA 1.0 [get_ports {a nope}]\n",
            "set_input_delay -clock * 1.0 [get_ports a]\n"):   # two clocks
        with pytest.raises(ValueError):
            constraints_from_sdc(parse_sdc_constraints(head + bad), nl)
    # 2 netlist domains + 62 virtual clocks fit, one more does not
    many = head + "".join(
        f"create_clock -period 5.0 -name v{i}\n"
        f"set_input_delay -clock v{i} 0.1 [get_ports a]\n" for i in range(63))
    with pytest.raises(ValueError):
        constraints_from_sdc(parse_sdc_constraints(many), nl)
    fit = "\n".join(many.splitlines()[:-2]) + "\n"
    c = constraints_from_sdc(parse_sdc_constraints(fit), nl)
    assert len(c.periods) == 64 and c.clock_names[-1] == "v61"
    # no such line: what it returned before, the same objects
    from test_sdc_driven import SDC2
    c = constraints_from_sdc(parse_sdc_constraints(SDC2), nl)
    assert c.block_clock is nl.block_clock
    assert c.launch_extra is None and c.capture_extra is None
    assert c.clock_names is None
    plain = constraints_from_sdc(parse_sdc_constraints(head), nl)
    assert plain.pair_skip is None and plain.pair_mult is None
    assert plain.block_clock is nl.block_clock


def test_loop_sta_passes_the_tables():
    from parallel_eda_amd.flow import loop_sta
    nl = two_clock_netlist()
    arch = get_arch("tiny")
    c = constraints_from_sdc(parse_sdc_constraints(SDC_IO), nl)
    eng = loop_sta(nl, arch, constraints=c)
    assert type(eng) is ConstrainedSTA
    _same_bits(eng.plan.launch, F(arch.T_seq_out) + c.launch_extra, "launch")
    _same_bits(eng.plan.capture, F(arch.T_seq_in) + c.capture_extra,
               "capture")
    d = np.full(nl.num_conns, 1e-9, F)
    bare = ConstrainedSTA(nl, arch, *c)
    assert (eng.analyze(d)[1] != bare.analyze(d)[1]).any()


# ---------------------------------------------------------------- 5. the CLI

def test_pair_slack_report_file(tmp_path):
    plan = constraint_plan([2e-9, 3e-9], [[0, 1], [0, 0]])
    ps = np.asarray([[0.5e-9, np.inf], [np.inf, -0.25e-9]], F)
    p = tmp_path / "r.txt"
    assert write_pair_slack_report(p, plan, ps, ["a"]) == 2
    lines = p.read_text().splitlines()
    assert lines[0].startswith("#")
    assert lines[1:] == ["a a 2.0000 0.5000", "domain1 domain1 3.0000 -0.2500"]


def test_cli_sdc_io_driven_report(tmp_path, capsys):
    from parallel_eda_amd.__main__ import main
    argv = _two_clock_files(tmp_path)
    (tmp_path / "c.sdc").write_text(SDC_IO)
    rpt = tmp_path / "pairs.txt"
    assert main(argv + ["--sdc_driven", "--sdc_report", str(rpt)]) == 0
    out = capsys.readouterr().out
    assert "SDC: input delay 1.000 ns, clock 'vclk', ports a" in out
    assert "SDC: output delay 0.500 ns, clock 'clkA', ports y" in out
    assert "SDC: exclusive clock groups clkA | clkB" in out
    assert "SDC-driven: 3 domains, 2 false pairs, 0 multicycle pairs" in out
    assert ("SDC-driven: 1 constrained inputs, 1 constrained outputs, "
            "1 virtual clocks") in out
    assert "routed in" in out and "SDC analysis: worst achieved period" in out
    assert f"wrote {rpt}" in out
    rows = [ln.split() for ln in rpt.read_text().splitlines()
            if not ln.startswith("#")]
    assert rows and all(len(r) == 4 for r in rows)
    pairs = {(r[0], r[1]) for r in rows}
    assert ("clkA", "clkB") not in pairs and ("clkB", "clkA") not in pairs
    assert any(r[0] == "vclk" for r in rows)
    per = {"clkA": 8.0, "clkB": 4.0, "vclk": 6.0}
    for src, dst, cons, slack in rows:
        assert float(cons) == per[dst] and float(slack) < per[dst]
    # the worst achieved period printed is the table's binding pair
    worst = max(float(c) - float(s) for _a, _b, c, s in rows
                if (float(c) - float(s)) / float(c) == max(
                    (float(c2) - float(s2)) / float(c2)
                    for _x, _y, c2, s2 in rows))
    import re
    got = float(re.search(r"worst achieved period (\S+) ns", out).group(1))
    assert got == pytest.approx(worst, abs=0.6e-3)   # %.3f and two %.4f in ns
    # without --sdc_driven the CPU engine writes the same kind of table
    rpt2 = tmp_path / "pairs2.txt"
    assert main(argv + ["--sdc_report", str(rpt2)]) == 0
    out = capsys.readouterr().out
    assert "SDC-driven" not in out and f"wrote {rpt2}" in out
    assert len(rpt2.read_text().splitlines()) >= 2
    # a port pattern that matches nothing is refused with a message
    (tmp_path / "c.sdc").write_text(
        SDC_IO + "set_input_delay -clock vclk 1.0 [get_ports {nope}]\n")
    assert main(argv + ["--sdc_driven"]) == 2
    assert "nope" in capsys.readouterr().err
