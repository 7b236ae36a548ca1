"""Move evaluation of the GPU placer on netlists the pinned scenarios of
test_gpu_place_run.py do not reach.

propose_move evaluates a single move member-parallel, (net, member) items
spread over the lanes of a wave, where its per-wave staging holds the move,
and a net per lane otherwise; commit copies the costs propose stored unless
the move has more nets than the stored-cost scratch has slots. The `wide`
netlist is built by hand so that each of these paths, and each switch
between them, is taken: nets of more than 64 members, blocks whose nets
need three and more 64-item passes, blocks whose nets exceed the staging,
blocks with more nets than a wave has lanes, repeated members, a driver
that is its own sink, and many pairs of blocks sharing two nets.

Expected values are digests recorded from the kernels of the commit before
the member-parallel evaluation (tools/record_place_eval_digests.py), so
every comparison is exact. The invariant test needs no fixture: what the
batches leave in net_cost/net_tcost is what a full refresh computes."""
import functools
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from parallel_eda_amd.arch.archdef import get_arch
from parallel_eda_amd.io.synth import NetlistPy, synth_netlist, spec_for_arch

CASES = ["wide"]
STATE = ["t_bx", "t_by", "t_bslot", "t_grid", "t_net_cost", "t_net_tcost",
         "t_mv_flags", "t_mv_dbb", "t_mv_dtd"]
BIG = 10 ** 9       # a target_moves no run reaches: the run goes to its cap
DIGESTS = Path(__file__).parent / "golden" / "place_eval_digests.json"

LANES = 64          # nets of one block a wave holds in one pass
SLOTS = 64          # EVAL_SLOTS and the cap of cost_k in place_kernel.hip
ITEMS = 256         # EVAL_ITEMS in place_kernel.hip


@functools.lru_cache(maxsize=None)
def _case(name):
    """(arch, netlist, seed). `wide`: a tseng netlist plus hand-made nets
    over its CLBs c[0], c[1], ...:
      W1  c[0] drives c[1..89]: 90 members
      W2  c[1] drives c[2..70] and c[5] a second time: 71 members
      W3  c[2] drives c[0], c[2] (itself), c[3..40]: 41 members
      W4  c[105] drives c[105..128] eleven times over: 265 members
    and three hubs added as a sink to existing nets: c[120] to 70 of them,
    c[95] to 45, c[96] to 30."""
    assert name == "wide"
    arch = get_arch("tseng")
    base = synth_netlist(spec_for_arch(arch, fill=0.9, seed=5))
    c = np.nonzero(np.asarray(base.block_type) == 1)[0]
    assert len(c) >= 129
    ptr = base.net_sink_ptr
    sinks = [list(base.net_sinks[ptr[n]:ptr[n + 1]])
             for n in range(base.num_nets)]
    drivers = list(base.net_driver)
    assert len(sinks) >= 115
    for hub, nets in ((c[120], range(0, 70)), (c[95], range(70, 115)),
                      (c[96], range(20, 50))):
        for n in nets:
            sinks[n].append(int(hub))
    wide = [
        (c[0], list(c[1:90])),
        (c[1], list(c[2:71]) + [c[5]]),
        (c[2], [c[0], c[2]] + list(c[3:41])),
        (c[105], list(c[105:129]) * 11),
    ]
    for d, s in wide:
        drivers.append(int(d))
        sinks.append([int(b) for b in s])
    nl = NetlistPy(base.block_type, base.block_is_seq,
                   np.asarray(drivers, dtype=np.int32),
                   np.r_[0, np.cumsum([len(s) for s in sinks])],
                   np.concatenate([np.asarray(s, dtype=np.int32)
                                   for s in sinks]))
    _assert_reaches_every_path(nl)      # before any GPU work
    return arch, nl, 9


def _csr(nl):
    """Host-side view of what the kernels walk: members of each net (driver
    first, repeats kept) and the deduplicated nets of each block."""
    ptr = nl.net_sink_ptr
    members = [[int(nl.net_driver[n])] + [int(b) for b in
                                          nl.net_sinks[ptr[n]:ptr[n + 1]]]
               for n in range(nl.num_nets)]
    blk_nets = [set() for _ in range(nl.num_blocks)]
    for n, mem in enumerate(members):
        for b in mem:
            blk_nets[b].add(n)
    return members, blk_nets


def _assert_reaches_every_path(nl):
    """Host-side check of the builder, so that a change to it or to the
    netlist generator cannot empty the tests."""
    members, blk_nets = _csr(nl)
    size = np.asarray([len(m) for m in members])
    deg = np.asarray([len(s) for s in blk_nets])
    items = np.asarray([sum(size[n] for n in s) for s in blk_nets])
    # a net of more than 64 members, and one the staging cannot hold
    assert (size > LANES).sum() >= 2
    assert (size > ITEMS).any()
    # a block evaluated member-parallel in at least 3 passes ...
    assert ((deg <= SLOTS) & (items > 2 * LANES) & (items <= ITEMS)).any()
    # ... and in exactly one and exactly two
    assert ((items > 0) & (items <= LANES)).any()
    assert ((items > LANES) & (items <= 2 * LANES)).any()
    # a block whose nets fit the slots but not the staging: serial, stored
    assert ((deg <= SLOTS) & (items > ITEMS)).any()
    # a block with more nets than the stored-cost scratch has slots and
    # than a wave has lanes: serial in two passes, recomputed by apply
    cost_k = int(np.clip(2 * deg.max(), 1, 64))
    assert cost_k == SLOTS
    assert (deg > cost_k).any() and (deg > LANES).any()
    # two blocks that fit each but not together
    assert np.sort(deg[deg <= SLOTS])[-2:].sum() > cost_k
    # a block twice in a net, and a driver among its own sinks
    assert any(len(set(m)) < len(m) for m in members)
    assert any(m[0] in m[1:] for m in members)
    # many pairs of blocks sharing at least two nets
    both = blk_nets_pairs = 0
    ids = [b for b in range(nl.num_blocks) if deg[b]]
    for i, a in enumerate(ids):
        for b in ids[i + 1:]:
            both += len(blk_nets[a] & blk_nets[b]) >= 2
            blk_nets_pairs += 1
    assert both >= 1000, (both, blk_nets_pairs)


def test_wide_netlist_reaches_every_path():
    """Needs no GPU: _case asserts the properties on the host-side CSR."""
    _case("wide")


def _snapshot(p, ret):
    s = {k: getattr(p, k).cpu().numpy().copy() for k in STATE}
    s["counters"] = p.t_counters.cpu().numpy()[:4].copy()
    s["batch_counter"] = p.batch_counter
    s["ret"] = ret
    s["costs"] = p.refresh_costs()
    # what the full refresh wrote, for the invariant test
    s["refreshed_net_cost"] = p.t_net_cost.cpu().numpy().copy()
    s["refreshed_net_tcost"] = p.t_net_tcost.cpu().numpy().copy()
    return s


@functools.lru_cache(maxsize=None)
def _drive(name, timing, legacy):
    """Run the scenario's run_batches calls on a fresh placer; returns
    [(label, snapshot)] with one snapshot per call."""
    from parallel_eda_amd.place.gpu_placer import GpuPlacer
    arch, nl, seed = _case(name)
    p = GpuPlacer(nl, arch, seed=seed, timing=timing, legacy_batches=legacy)
    tt = 0.0
    if timing:
        # the hand-made nets close combinational loops, so no STA here:
        # any criticalities in [0, 1) serve
        crit = np.random.default_rng(3).random(nl.num_conns)
        p.set_crit(crit.astype(np.float32))
        p.refresh_costs()
        tt = 0.5
    bbn, tdn = ((max(p.bb_cost, 1e-12), max(p.td_cost, 1e-30)) if timing
                else (1.0, 1.0))
    t_mid = 2e-3 if timing else 2.0
    full = float(max(arch.nx, arch.ny))
    out = []

    def call(label, *a, **k):
        out.append((label, _snapshot(p, p.run_batches(*a, **k))))

    call("hot", 1e30, full, BIG, tt, bbn, tdn, max_batches=16)
    call("mid", t_mid, full, BIG, tt, bbn, tdn, max_batches=64)
    call("quench", 0.0, 1.0, BIG, tt, bbn, tdn, max_batches=32)
    call("near", t_mid, 3.0, BIG, tt, bbn, tdn, max_batches=32)
    return out


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


@pytest.mark.gpu
@pytest.mark.parametrize("legacy", [True, False], ids=["legacy", "run"])
@pytest.mark.parametrize("timing", [False, True], ids=["bb", "timing"])
@pytest.mark.parametrize("name", CASES)
def test_matches_parent_digests(name, timing, legacy):
    """Both drivers compute, to the bit, what the serial per-net evaluation
    and the recomputing apply computed."""
    fixture = json.loads(DIGESTS.read_text())
    want = fixture["digests"][f"{name}-{'timing' if timing else 'bb'}"]
    drive = _drive(name, timing, legacy)
    # the scenario does what it is meant to: moves won, lost and rejected
    for label, s in drive:
        att, acc, win, lost = (int(v) for v in s["counters"])
        assert win > 0 and lost > 0, (label, s["counters"])
        if label != "hot":
            assert att > acc, (label, s["counters"])
    got = _digests(drive)
    assert list(got) == list(want)
    keys = set(got["hot"]) - set(fixture["left_out"])
    for label in want:
        assert set(want[label]) == keys, label
        for k, v in want[label].items():
            assert got[label][k] == v, f"{label}: {k}: {got[label][k]} != {v}"


@pytest.mark.gpu
@pytest.mark.parametrize("legacy", [True, False], ids=["legacy", "run"])
@pytest.mark.parametrize("timing", [False, True], ids=["bb", "timing"])
@pytest.mark.parametrize("name", CASES)
def test_cached_costs_equal_full_refresh(name, timing, legacy):
    """After each run_batches call the cached net costs, as the winners'
    applies left them, are bit for bit what refresh_costs() recomputes from
    the positions."""
    for label, s in _drive(name, timing, legacy):
        for k in ("net_cost", "net_tcost"):
            assert np.array_equal(
                s["t_" + k].view(np.uint32),
                s["refreshed_" + k].view(np.uint32)), f"{label}: {k}"
        if timing:
            assert s["t_net_tcost"].any(), label
