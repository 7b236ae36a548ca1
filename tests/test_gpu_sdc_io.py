"""Device side of the SDC I/O constraints: GpuConstrainedSTA with the
per-block launch / capture tables and pair_slack() (stc_pair_slack in
csrc/hip/sta_constrained.hip), held bit for bit to the CPU engine and the
replay of tests/test_sdc_io.py.

Every value is a chain of single fp32 operations on both sides and the
tables are rounded once on the host, so nothing here has a tolerance; the
only freedom is the documented tie rule of the worst period. pair_slack()
is a minimum, which does not depend on the order of the atomics.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from parallel_eda_amd.route.router import ConnMap, net_rr_terminals
from parallel_eda_amd.timing.constraints import Constraints
from parallel_eda_amd.timing.sta import ConstrainedSTA

from test_sta_exact import case, _same_bits, F, ONE_PASS
from test_sta_constrained import GPU_GRAPHS, expected, setup_of, _check
from test_sdc_driven import _constraints
from test_device_timing import _case
from test_sdc_io import IO_SETS, INF, expected_io, io_extras

pytestmark = pytest.mark.gpu


def _gsta(cs):
    from parallel_eda_amd.timing.gpu_sta import GpuSTA
    return GpuSTA(cs.nl, cs.arch, max_crit=1.0)


def _engine(gs, e):
    from parallel_eda_amd.timing.gpu_sta import GpuConstrainedSTA
    return GpuConstrainedSTA(gs, e.bc, e.periods, e.skip, e.mult,
                             launch_extra=e.le, capture_extra=e.ce)


# ------------------------------------------------------ 1. bit equality

@pytest.mark.parametrize("name", GPU_GRAPHS)
def test_gpu_tables_exact(name):
    cs = case(name)
    if name == "stride":
        assert cs.nl.num_conns > ONE_PASS and cs.nl.num_blocks > ONE_PASS
    gs = _gsta(cs)
    for set_name in IO_SETS:
        e = expected_io(name, set_name)
        eng = _engine(gs, e)
        assert eng.t_launch is not None and eng.t_capture is not None
        tag = f"{name}/{set_name}/tables"
        got = eng.analyze(e.d)
        _check(eng, e, got, tag)
        _same_bits(eng.pair_slack().ravel(), e.pair_slack.ravel(),
                   f"{tag} pair slack")
        # null tables: the engine of before, built both ways
        old = expected(name, set_name)
        null = expected_io(name, set_name, tables=False)
        for how, eng0 in (("positional", type(eng)(gs, old.bc, old.periods,
                                                   old.skip, old.mult)),
                          ("keywords", _engine(gs, null))):
            assert eng0.t_launch is None and eng0.t_capture is None
            assert eng0._args.launch is None and eng0._args.capture is None
            got0 = eng0.analyze(old.d)
            _check(eng0, old, got0, f"{name}/{set_name}/null {how}")
            _same_bits(eng0.pair_slack().ravel(), null.pair_slack.ravel(),
                       f"{name}/{set_name}/null {how} pair slack")
        assert (got[1] != got0[1]).any() or not old.rp.top, tag


# ------------------------------------------------------- 2. pair_slack()

@functools.lru_cache(maxsize=None)
def many_domains(name, k):
    """k domains over the flip-flops of a graph (block index mod k),
    periods from 0.55 to 1.6 times the single-clock cpd, every 11th pair
    false, multicycle 2 on two pairs, and the I/O tables; the CPU engine's
    answer."""
    cs, _, _, d = setup_of(name)
    nl = cs.nl
    seq = nl.block_is_seq.astype(bool)
    bc = np.where(seq, np.arange(nl.num_blocks) % k, -1).astype(np.int32)
    cpd, _, _ = cs.sta.analyze(d)
    periods = (np.linspace(0.55, 1.6, k) * F(cpd)).astype(F)
    ci, cj = np.indices((k, k))
    skip = ((ci * 7 + cj * 3) % 11 == 0).astype(np.uint8)
    mult = np.ones((k, k), F)
    mult[0, 1] = 2
    mult[k - 1, 0] = 2
    le, ce = io_extras(nl, periods)
    eng = ConstrainedSTA(nl, cs.arch, bc, periods, skip, mult,
                         launch_extra=le, capture_extra=ce)
    wp, slack, crit = eng.analyze(d)
    return SimpleNamespace(cs=cs, bc=bc, periods=periods, d=d, skip=skip,
                           mult=mult, le=le, ce=ce, slack=slack, crit=crit,
                           pair_slack=eng.pair_slack())


@pytest.mark.parametrize("name,k", [("wide", 3), ("wide", 8), ("wide_het", 9),
                                    ("mid", 64), ("stride", 3), ("chain", 3)])
def test_gpu_pair_slack_exact(name, k):
    """K = 3: nine words, many lanes per word; K = 8: one wave of pairs;
    K = 9: 81 words, no multiple of 64; K = 64 on mid: the full 4096-word
    LDS table; stride: more than one grid-stride pass; chain: three
    connections, less than one workgroup."""
    if (name, k) in (("wide", 3), ("stride", 3)):
        e = expected_io(name, "false_and_mc")
    else:
        e = many_domains(name, k)
    nc = e.cs.nl.num_conns
    if name == "stride":
        assert nc * k * k > 1024 * 256           # the kernel's one pass
    if name == "chain":
        assert nc * k * k < 256
    eng = _engine(_gsta(e.cs), e)
    with pytest.raises(RuntimeError):
        eng.pair_slack()
    _, slack, crit = eng.analyze(e.d)
    _same_bits(slack, e.slack, f"{name} K={k} slack")
    _same_bits(crit, e.crit, f"{name} K={k} crit")
    got = eng.pair_slack()
    assert got.shape == (k, k) and got.dtype == np.float32
    _same_bits(got.ravel(), e.pair_slack.ravel(), f"{name} K={k} pair slack")
    if name != "chain":
        assert np.isfinite(got).any()
    assert (got[np.asarray(e.skip) != 0] == INF).all()
    # again, and after another analysis: the table follows the last one
    _same_bits(eng.pair_slack().ravel(), e.pair_slack.ravel(), "second call")
    if name == "wide":
        d2 = e.cs.delays["outlier"]
        cpu = ConstrainedSTA(e.cs.nl, e.cs.arch, e.bc, e.periods, e.skip,
                             e.mult, launch_extra=e.le, capture_extra=e.ce)
        cpu.analyze(d2)
        eng.analyze(d2)
        _same_bits(eng.pair_slack().ravel(), cpu.pair_slack().ravel(),
                   "other delays")
        assert (cpu.pair_slack() != e.pair_slack).any()


def test_gpu_pair_slack_all_false():
    e = expected_io("wide_het", "none")
    from parallel_eda_amd.timing.gpu_sta import GpuConstrainedSTA
    k = len(e.periods)
    eng = GpuConstrainedSTA(_gsta(e.cs), e.bc, e.periods,
                            np.ones((k, k), np.uint8), None,
                            launch_extra=e.le, capture_extra=e.ce)
    eng.analyze(e.d)
    got = eng.pair_slack()
    assert got.shape == (k, k) and (got == INF).all()


# ------------------------------------------------------------ 3. the flow

def test_run_flow_gpu_io_constraints():
    from parallel_eda_amd.parallel.full_flow import run_flow_gpu
    from parallel_eda_amd import rrgraph
    arch, nl, seed = _case("tiny")
    base = _constraints("tiny")
    le, ce = io_extras(nl, base.periods)
    assert np.count_nonzero(le) and np.count_nonzero(ce)
    cons = Constraints(*base, launch_extra=le, capture_extra=ce)
    g = rrgraph.build_rr_graph(arch)
    out = run_flow_gpu(nl, arch, g, seed=seed, check=True, sta_engine="gpu",
                       constraints=cons)
    assert out["success"] and out["cpd"] > 0
    assert out["place"].stats["device_timing"]
    _, _, sink_ptr, sink_rr, conn_index = net_rr_terminals(
        nl, out["place"], g, arch)
    cmap = ConnMap(conn_index, sink_ptr, nl.num_conns, len(sink_rr))
    cd = cmap.conn_delays(out["router"].t_sink_delay.cpu().numpy(),
                          fill=float(arch.T_opin + arch.T_ipin))
    fresh = ConstrainedSTA(nl, arch, *cons, **cons.io_kwargs())
    assert out["cpd"] == fresh.analyze(cd)[0]


def test_cli_sdc_report_from_gpu_engine(tmp_path, capsys):
    """--sdc_driven --sta_engine gpu --sdc_report: the table is the device
    engine's pair_slack() on the loop's last analysis; its binding pair is
    the worst achieved period the CPU report prints for the same routing."""
    import re
    from parallel_eda_amd.__main__ import main
    from test_sdc_driven import _two_clock_files
    from test_sdc_io import SDC_IO
    argv = _two_clock_files(tmp_path)
    (tmp_path / "c.sdc").write_text(SDC_IO)
    rpt = tmp_path / "pairs.txt"
    assert main(argv + ["--sdc_driven", "--engine", "gpu", "--sta_engine",
                        "gpu", "--sdc_report", str(rpt)]) == 0
    out = capsys.readouterr().out
    assert ("SDC-driven: 1 constrained inputs, 1 constrained outputs, "
            "1 virtual clocks") in out
    assert f"wrote {rpt}" in out
    rows = [ln.split() for ln in rpt.read_text().splitlines()
            if not ln.startswith("#")]
    assert rows and any(r[0] == "vclk" for r in rows)
    assert not {("clkA", "clkB"), ("clkB", "clkA")} & {(r[0], r[1])
                                                       for r in rows}
    ratio = [((float(c) - float(s)) / float(c), float(c) - float(s))
             for _a, _b, c, s in rows]
    got = float(re.search(r"worst achieved period (\S+) ns", out).group(1))
    assert got == pytest.approx(max(ratio)[1], abs=0.6e-3)   # %.3f and two %.4f in ns
