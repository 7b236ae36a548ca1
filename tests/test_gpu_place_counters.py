"""Counter shards of the native placer run loop (pnr_place_run) against the
direct counter words of the legacy batch loop (pnr_place_batch).

The run loop spreads its counter atomics over COUNTER_SHARDS lines, chosen
by workgroup, and the stop rule folds them into t_counters. Integer sums do
not depend on order, so every comparison here is exact. The batch sizes are
the ones at which sharding and folding can go wrong: fewer workgroups than
shards, workgroups with idle waves, the last shard just unused and just
used, the first shard used twice, every shard used by several workgroups.
"""
import functools

import numpy as np
import pytest

from parallel_eda_amd.arch.archdef import get_arch
from parallel_eda_amd.io.synth import synth_netlist, spec_for_arch
from parallel_eda_amd.place.gpu_placer import COUNTER_SHARDS, RUN_CHUNK_BATCHES
from parallel_eda_amd.timing.sta import STA

pytestmark = pytest.mark.gpu

S = COUNTER_SHARDS
WAVES = 4           # proposals per workgroup (PROP_WAVES of the kernels)
N_MOVES = [1, 3, 5, WAVES * S - 1, WAVES * S, WAVES * S + 1,
           2 * WAVES * S + 37]
CASES = ["tseng", "tiny_het"]
STATE = ["t_bx", "t_by", "t_bslot", "t_grid", "t_net_cost", "t_net_tcost"]
BIG = 10 ** 9       # a target_moves no run reaches: the run goes to its cap


@functools.lru_cache(maxsize=None)
def _case(name):
    """The netlists of tests/test_gpu_place_run.py, and the criticalities of
    the initial placement for the runs with timing on."""
    from parallel_eda_amd.place.gpu_placer import GpuPlacer
    if name == "tiny_het":
        arch = get_arch("tiny_het")
        nl = synth_netlist(spec_for_arch(arch, fill=0.6, seed=1))
        seed = 1
    else:
        arch = get_arch("tseng")
        nl = synth_netlist(spec_for_arch(arch, fill=0.5, seed=4))
        seed = 4
    p = GpuPlacer(nl, arch, seed=seed, timing=True, n_moves=1)
    bx = p.t_bx.cpu().numpy(); by = p.t_by.cpu().numpy()
    net_of_conn = np.repeat(np.arange(nl.num_nets), np.diff(nl.net_sink_ptr))
    drv = nl.net_driver[net_of_conn]
    d = p._dm[np.abs(bx[nl.net_sinks] - bx[drv]),
              np.abs(by[nl.net_sinks] - by[drv])]
    _cpd, _slack, crit = STA(nl, arch).analyze(d)
    return arch, nl, seed, np.asarray(crit)


class _Driver:
    """A fresh placer and the arguments its run_batches calls share."""

    def __init__(self, name, timing, legacy, n_moves):
        from parallel_eda_amd.place.gpu_placer import GpuPlacer
        arch, nl, seed, crit = _case(name)
        self.p = p = GpuPlacer(nl, arch, seed=seed, timing=timing,
                               n_moves=n_moves, legacy_batches=legacy)
        self.n_moves = n_moves
        self.tt = 0.0
        self.norms = (1.0, 1.0)
        if timing:
            p.set_crit(crit)
            p.refresh_costs()
            self.tt = 0.5
            self.norms = (max(p.bb_cost, 1e-12), max(p.td_cost, 1e-30))
        # of the order of one move's delta: a mix of accepts and rejects
        self.t_mid = 2e-3 if timing else 2.0
        self.full = float(max(arch.nx, arch.ny))

    def call(self, T, rlim, target, max_batches):
        """One run_batches call; returns what the drivers must agree on."""
        p = self.p
        before = p.batch_counter
        ret = p.run_batches(T, rlim, target, self.tt, *self.norms,
                            max_batches=max_batches)
        s = {k: getattr(p, k).cpu().numpy().copy() for k in STATE}
        s["counters"] = p.t_counters.cpu().numpy()[:4].copy()
        s["batch_counter"] = p.batch_counter
        s["ret"] = ret
        s["ran"] = p.batch_counter - before
        att, acc, win, conf = (int(v) for v in s["counters"])
        # every accepted move was decided once
        assert acc == win + conf, s["counters"]
        assert att >= acc, s["counters"]
        assert att <= self.n_moves * s["ran"], (s["counters"], s["ran"])
        return s


def _assert_same(got, want, what):
    for k in STATE + ["counters"]:
        assert np.array_equal(got[k], want[k]), \
            f"{what}: {k} differs: {got[k]} != {want[k]}"
    for k in ("batch_counter", "ret", "ran"):
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"


@pytest.mark.parametrize("timing", [False, True], ids=["bb", "timing"])
@pytest.mark.parametrize("n_moves", N_MOVES)
@pytest.mark.parametrize("name", CASES)
def test_counters_match_legacy(name, n_moves, timing):
    old = _Driver(name, timing, True, n_moves)
    new = _Driver(name, timing, False, n_moves)
    calls = [
        ("hot", (1e30, old.full, 1, 16)),
        ("capped", (old.t_mid, old.full, BIG, 8)),
        ("quench", (0.0, 1.0, BIG, 8)),
        ("capped2", (old.t_mid, old.full, BIG, 8)),
    ]
    seen = {}
    for label, args in calls:
        w, g = old.call(*args), new.call(*args)
        _assert_same(g, w, f"{name} n_moves={n_moves} {label}")
        seen[label] = w
    assert seen["capped"]["ran"] == seen["quench"]["ran"] == 8
    # Empty launches: the hot call enqueues 16 batches and the stop rule
    # fires before the cap, so the launches after it return on `done`; the
    # counters, compared above, are the legacy driver's after the batches it
    # ran. With a batch of several workgroups the first check already fires
    # (the lowest accepted move of a batch always wins).
    if n_moves >= WAVES * S - 1:
        assert seen["hot"]["ran"] == 4
        assert seen["hot"]["counters"][2] >= 1
    # Stale shards: the second capped call's counters, compared above, are
    # those of its own 8 batches and not a sum over earlier calls. The
    # bound inside call() says the same of the run loop alone, and here
    # the attempts of a call stay below what two calls would give.
    if n_moves >= WAVES * S - 1:
        assert seen["capped2"]["counters"][0] > 0
        assert (seen["capped2"]["counters"][0] <
                seen["capped"]["counters"][0] + seen["quench"]["counters"][0])


@pytest.mark.parametrize("timing", [False, True], ids=["bb", "timing"])
def test_totals_current_at_every_chunk(timing):
    """Totals current at every chunk: a target met in the second chunk of
    pnr_place_run stops the run loop where the legacy loop stops. The target
    comes from a legacy run capped one check into the second chunk."""
    n_moves = N_MOVES[-1]
    cap = RUN_CHUNK_BATCHES + 4
    probe = _Driver("tseng", timing, True, n_moves)
    s = probe.call(probe.t_mid, probe.full, BIG, cap)
    assert s["ran"] == cap
    att, acc, win, _conf = (int(v) for v in s["counters"])
    target = win + (att - acc)
    old = _Driver("tseng", timing, True, n_moves)
    new = _Driver("tseng", timing, False, n_moves)
    args = (old.t_mid, old.full, target, 2 * RUN_CHUNK_BATCHES)
    w, g = old.call(*args), new.call(*args)
    # the last four batches decided something, so no earlier check fired
    assert w["ran"] == cap
    _assert_same(g, w, "second chunk")
