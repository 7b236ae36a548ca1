"""Native placer run loop (pnr_place_run: propose + commit per batch,
epoch-key claims, device-side stop rule) against the legacy batch loop
(pnr_place_batch, four kernels per batch, host-side stop rule).

The two paths must agree bit for bit, so every comparison here is exact.
Each scenario is driven once per path and the recorded states are shared
by the tests; a second legacy drive is the control that shows the oracle
itself is reproducible.

Both drivers share one propose/resolve/apply body, so their agreement no
longer shows that the body computes what it did before it was shared.
tests/golden/place_run_digests.json pins that: digests of every snapshot
recorded from the last commit with two separate bodies
(tools/record_place_digests.py)."""
import functools
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from parallel_eda_amd.arch.archdef import get_arch
from parallel_eda_amd.io.synth import synth_netlist, spec_for_arch
from parallel_eda_amd.timing.sta import STA

pytestmark = pytest.mark.gpu

CASES = ["tseng", "tiny_het", "tseng_macros", "tseng_fixed"]
STATE = ["t_bx", "t_by", "t_bslot", "t_grid", "t_net_cost", "t_net_tcost",
         "t_mv_flags", "t_mv_dbb", "t_mv_dtd"]
BIG = 10 ** 9       # a target_moves no run reaches: the run goes to its cap
N_PINNED = 8        # tseng_fixed: the lowest-numbered IO blocks are pinned
DIGESTS = Path(__file__).parent / "golden" / "place_run_digests.json"


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "tiny_het":
        arch = get_arch("tiny_het")
        nl = synth_netlist(spec_for_arch(arch, fill=0.6, seed=1))
        return arch, nl, 1, None
    arch = get_arch("tseng")
    nl = synth_netlist(spec_for_arch(arch, fill=0.5, seed=4))
    if name in ("tseng", "tseng_fixed"):
        return arch, nl, 4, None
    # the two carry chains of test_gpu_place.py::test_gpu_macro_moves
    clbs = np.nonzero(np.asarray(nl.block_type) == 1)[0]
    macros = [[(int(clbs[0]), 0, 0), (int(clbs[1]), 0, 1),
               (int(clbs[2]), 0, 2)],
              [(int(clbs[3]), 0, 0), (int(clbs[4]), 0, 1),
               (int(clbs[5]), 0, 2), (int(clbs[6]), 0, 3)]]
    return arch, nl, 11, macros


@functools.lru_cache(maxsize=None)
def _pins(name):
    """fixed=(ids, x, y, slot) of a scenario, or None. tseng_fixed pins
    blocks where an unpinned placer of the same seed puts them at first,
    so the pin-down teleport is a no-op and the placement stays legal."""
    if name != "tseng_fixed":
        return None
    from parallel_eda_amd.place.gpu_placer import GpuPlacer
    arch, nl, seed, _ = _case(name)
    ids = np.nonzero(np.asarray(nl.block_type) == 0)[0][:N_PINNED]
    assert len(ids) == N_PINNED
    free = GpuPlacer(nl, arch, seed=seed)
    return (ids,) + tuple(t.cpu().numpy()[ids]
                          for t in (free.t_bx, free.t_by, free.t_bslot))


def _snapshot(p, ret):
    s = {k: getattr(p, k).cpu().numpy().copy() for k in STATE}
    s["counters"] = p.t_counters.cpu().numpy()[:4].copy()
    s["batch_counter"] = p.batch_counter
    s["ret"] = ret
    s["costs"] = p.refresh_costs()
    return s


@functools.lru_cache(maxsize=None)
def _drive(name, timing, legacy, instance=0):
    """Run the scenario's run_batches calls on a fresh placer; returns
    [(label, snapshot)] with one snapshot per call."""
    from parallel_eda_amd.place.gpu_placer import GpuPlacer
    arch, nl, seed, macros = _case(name)
    p = GpuPlacer(nl, arch, seed=seed, timing=timing, macros=macros,
                  fixed=_pins(name), legacy_batches=legacy)
    tt = 0.0
    if timing:
        # criticalities from the initial placement, as the anneal does
        bx = p.t_bx.cpu().numpy(); by = p.t_by.cpu().numpy()
        net_of_conn = np.repeat(np.arange(nl.num_nets),
                                np.diff(nl.net_sink_ptr))
        drv = nl.net_driver[net_of_conn]
        d = p._dm[np.abs(bx[nl.net_sinks] - bx[drv]),
                  np.abs(by[nl.net_sinks] - by[drv])]
        _cpd, _slack, crit = STA(nl, arch).analyze(d)
        p.set_crit(np.asarray(crit))
        p.refresh_costs()
        tt = 0.5
    bbn, tdn = ((max(p.bb_cost, 1e-12), max(p.td_cost, 1e-30)) if timing
                else (1.0, 1.0))
    # a temperature of the order of one move's delta (normalised costs
    # with timing on): a mix of accepts and rejects
    t_mid = 2e-3 if timing else 2.0
    full = float(max(arch.nx, arch.ny))
    out = []

    def call(label, *a, **k):
        out.append((label, _snapshot(p, p.run_batches(*a, **k))))

    # At T=1e30 every valid proposal is accepted and the lowest accepted
    # move of a batch holds all its claims, so each batch decides at
    # least one move: a target of 8 is met by batch 8, a target of 1 by
    # batch 4 (the first test of the stop rule), both before the cap.
    call("hot8", 1e30, full, 8, tt, bbn, tdn, max_batches=16)
    call("hot1", 1e30, full, 1, tt, bbn, tdn, max_batches=16)
    call("mid_cap", t_mid, full, BIG, tt, bbn, tdn)
    call("quench", 0.0, 1.0, BIG, tt, bbn, tdn, max_batches=64)
    p.set_move_region(p.gx // 4, p.gx // 2)
    call("strip", t_mid, full, BIG, tt, bbn, tdn, max_batches=64)
    p.set_move_region(-1, -1)
    # every batch decides at least one move, so 100 is met before the cap
    call("mid_stop", t_mid, full / 2, 100, tt, bbn, tdn)
    return out


def _assert_same(got, want, what):
    assert [g[0] for g in got] == [w[0] for w in want]
    for (label, g), (_, w) in zip(got, want):
        for k in STATE + ["counters"]:
            assert np.array_equal(g[k], w[k]), f"{what}: {label}: {k} differs"
        for k in ("batch_counter", "ret", "costs"):
            assert g[k] == w[k], f"{what}: {label}: {k} {g[k]} != {w[k]}"


@pytest.mark.parametrize("timing", [False, True], ids=["bb", "timing"])
@pytest.mark.parametrize("name", CASES)
def test_legacy_loop_is_reproducible(name, timing):
    """Control: two legacy placers with the same seed agree exactly, and
    the scenario does what it is meant to (stop rule and cap both hit)."""
    a = _drive(name, timing, True)
    _assert_same(_drive(name, timing, True, 1), a, "legacy vs legacy")
    snaps = dict(a)
    prev = 0
    ran = {}
    for label, s in a:
        ran[label] = s["batch_counter"] - prev
        prev = s["batch_counter"]
    assert ran["hot8"] in (4, 8), ran       # stop rule, not the cap of 16
    assert ran["hot1"] == 4, ran
    assert ran["mid_cap"] == 256 and ran["quench"] == 64, ran
    assert ran["strip"] == 64, ran
    assert 4 <= ran["mid_stop"] < 256 and ran["mid_stop"] % 4 == 0, ran
    # moves were really applied, and conflicts really happened
    assert snaps["mid_cap"]["counters"][2] > 0
    assert snaps["hot8"]["counters"][3] > 0


@pytest.mark.parametrize("timing", [False, True], ids=["bb", "timing"])
@pytest.mark.parametrize("name", CASES)
def test_run_loop_matches_legacy(name, timing):
    _assert_same(_drive(name, timing, False), _drive(name, timing, True),
                 "run loop vs legacy")


def _digests(drive):
    """{call label: digest of its snapshot}, in the form the fixture holds:
    sha256 of each array's bytes, floats as float.hex strings."""
    out = {}
    for label, s in drive:
        d = {k: hashlib.sha256(np.ascontiguousarray(s[k]).tobytes()).hexdigest()
             for k in STATE + ["counters"]}
        d["batch_counter"] = int(s["batch_counter"])
        d["ret"] = [float(v).hex() for v in s["ret"]]
        d["costs"] = [float(v).hex() for v in s["costs"]]
        out[label] = d
    return out


@pytest.mark.parametrize("legacy", [True, False], ids=["legacy", "run"])
@pytest.mark.parametrize("timing", [False, True], ids=["bb", "timing"])
@pytest.mark.parametrize("name", CASES)
def test_matches_parent_digests(name, timing, legacy):
    """Both drivers compute, to the bit, what the legacy driver computed
    when each driver still had its own copy of the kernels' text."""
    fixture = json.loads(DIGESTS.read_text())
    want = fixture["digests"][f"{name}-{'timing' if timing else 'bb'}"]
    got = _digests(_drive(name, timing, legacy))
    assert list(got) == list(want)
    # keys that two recordings of the parent disagreed on are left out
    keys = set(got["hot8"]) - set(fixture["left_out"])
    for label in want:
        assert set(want[label]) == keys, label
        for k, v in want[label].items():
            assert got[label][k] == v, f"{label}: {k}: {got[label][k]} != {v}"


def test_pinned_blocks_stay():
    """tseng_fixed drives the `fixed` branches of propose: the pinned
    blocks never move, on either driver, while the others do."""
    ids, x, y, slot = _pins("tseng_fixed")
    free = np.ones(_case("tseng_fixed")[1].num_blocks, dtype=bool)
    free[ids] = False
    for timing in (False, True):
        for legacy in (True, False):
            drive = _drive("tseng_fixed", timing, legacy)
            for label, s in drive:
                assert np.array_equal(s["t_bx"][ids], x), label
                assert np.array_equal(s["t_by"][ids], y), label
                assert np.array_equal(s["t_bslot"][ids], slot), label
            first, last = drive[0][1], drive[-1][1]
            assert ((first["t_bx"] != last["t_bx"]) |
                    (first["t_by"] != last["t_by"]))[free].any()
    # the pins are IO blocks that an unpinned run of the same seed moves
    unpinned = dict(_drive("tseng", False, True))["mid_stop"]
    assert ((unpinned["t_bx"][ids] != x) | (unpinned["t_by"][ids] != y) |
            (unpinned["t_bslot"][ids] != slot)).any()


def test_strip_confines_moves():
    """The strip call moved blocks, and only inside the strip."""
    snaps = dict(_drive("tseng", False, False))
    before, after = snaps["quench"], snaps["strip"]
    moved = (before["t_bx"] != after["t_bx"]) | (before["t_by"] != after["t_by"])
    assert moved.any()
    from parallel_eda_amd.place.gpu_placer import GpuPlacer  # noqa: F401
    arch = _case("tseng")[0]
    gx = arch.nx + 2
    for s in (before, after):
        assert (s["t_bx"][moved] >= gx // 4).all()
        assert (s["t_bx"][moved] <= gx // 2).all()


@pytest.mark.parametrize("timing", [False, True], ids=["bb", "timing"])
def test_anneal_matches_legacy(timing):
    """Whole anneals agree: same placement, costs, temperatures, history."""
    from parallel_eda_amd.place.gpu_placer import anneal_place_gpu
    arch, nl, _seed, _ = _case("tseng")
    res = []
    for legacy in (True, False):
        sta = STA(nl, arch) if timing else None
        res.append(anneal_place_gpu(
            nl, arch, seed=7, timing_tradeoff=0.5 if timing else 0.0,
            sta=sta, legacy_batches=legacy))
    old, new = res
    for k in ("x", "y", "slot"):
        assert np.array_equal(np.asarray(getattr(new, k)),
                              np.asarray(getattr(old, k))), k
    assert new.bb_cost == old.bb_cost
    assert new.td_cost == old.td_cost
    assert new.stats["temps"] == old.stats["temps"]
    assert new.stats["history"] == old.stats["history"]
    if timing:
        assert new.td_cost > 0
