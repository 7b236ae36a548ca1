"""The GPU router's searches against an exact shortest-path model.

Every test routes ONE net per route_iteration call on a seeded random
cost surface (acc in [1, 4), background occupancy 0/1/2 on the wires), so
the surface a search sees is static, and compares what the kernel
committed with route/exact_model.py (float64 Dijkstra, one net at a time):

  * the tree passes RouteModel.validate_tree (edges, switches, parent
    order, no duplicates, bb, SINK leaves, every sink once, Elmore delays
    within 4 * depth * 2^-24, sink_delay bit-copied to the ORIGINAL sink
    index, occupancy difference == host bincount of the tree);
  * per sink, the float64 cost of the kernel's path (attach node to sink,
    started at crit * delay(attach)) lies in
        [opt * (1 - 16 n 2^-24), (opt + eps) * (1 + 16 n 2^-24)]
    where opt is the model's optimum from the kernel's own tree so far,
    n the larger hop count of the two paths, and eps the largest amount by
    which astar_fac * lookahead overestimates the cost-to-go along the
    model's optimal path (0 at astar_fac = 0: the exact case). A kernel
    terminates when the sink's cost is <= (or <) the least frontier f, and
    some node of an optimal path is always in the frontier with its optimal
    g, so it can return at most opt + eps. Below opt means kernel and model
    disagree on what is allowed (bb, IPIN or SINK rule).

Engines: the ping-pong kernel in the dense (small-slot) and the global
(large-slot) state index, strict and non-strict termination, the calendar
kernel and the whole-device MWG engine. Case 10 (bb growth) uses nets the
model finds unroutable inside their margin-0 bb: (0,2)->(2,2) on tiny and
(1,4)->(2,4) on tseng.

The four congestion sweeps are compared exactly with numpy at the end.
"""
import numpy as np
import pytest

from parallel_eda_amd.arch.archdef import get_arch
from parallel_eda_amd import rrgraph
from parallel_eda_amd.route.exact_model import (RouteModel, cost_bounds,
                                                RR_SINK, RR_CHANX, RR_CHANY)

pytestmark = pytest.mark.gpu

ENV = ("PNR_ASTAR", "PNR_DELTA", "PNR_CALENDAR", "PNR_FORCE_STRICT",
       "PNR_RETRY_SERIAL")

# (engine label, astar_fac) -> [max cost/opt, max cost/(opt+eps),
#                               max relative delay error, sinks]
STATS = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nengine, astar_fac: max cost/opt - 1, max cost/(opt+eps) - 1, "
          "max rel delay error, sinks")
    for (eng, a), s in sorted(STATS.items()):
        print(f"EXACT {eng:16s} a={a:g}: {s[0] - 1:.3e} {s[1] - 1:.3e} "
              f"{s[2]:.3e} {s[3]}")


class Ctx:
    def __init__(self, name, nets):
        self.arch = get_arch(name)
        self.g = rrgraph.build_rr_graph(self.arch)
        self.m = RouteModel(self.g, self.arch)
        gy = self.arch.ny + 2
        ts = np.asarray(self.g.tile_source)
        tk = np.asarray(self.g.tile_sink)
        self.nets = [(int(ts[sx * gy + sy]),
                      [int(tk[x * gy + y]) for (x, y) in sinks])
                     for (sx, sy), sinks in nets]
        self.tiles = nets
        self.src_rr = np.asarray([n[0] for n in self.nets], dtype=np.int32)
        self.sink_ptr = np.r_[0, np.cumsum([len(n[1]) for n in self.nets])
                              ].astype(np.int32)
        self.sink_rr = np.asarray([s for n in self.nets for s in n[1]],
                                  dtype=np.int32)

    def margin0_routable(self, i):
        """Whether net i can be routed inside its margin-0 bb (a property
        of the graph alone)."""
        m = self.m
        src, sinks = self.nets[i]
        t = [src] + sinks
        bb = (m.xlow[t].min(), m.ylow[t].min(), m.xlow[t].max(),
              m.ylow[t].max())
        z = np.zeros(m.n, dtype=np.int32)
        _, recs, _ = m.route_net(src, sinks, np.zeros(len(sinks)), bb, z,
                                 np.ones(m.n, dtype=np.float32), 0.0)
        return all(r.opt is not None for r in recs) and \
            len(recs) == len(sinks)


# tiny is 4 x 4 CLBs, IO ring at coordinate 0 and 5
TINY_NETS = [
    ((1, 1), [(1, 2)]),             # 0 adjacent tiles
    ((3, 2), [(2, 2)]),             # 1 adjacent, other axis
    ((1, 1), [(4, 4)]),             # 2 opposite corners
    ((4, 1), [(1, 4)]),             # 3 the other diagonal
    ((0, 2), [(3, 3)]),             # 4 IO source at x = 0
    ((2, 2), [(5, 3)]),             # 5 IO sink at x = nx + 1
    ((5, 1), [(0, 4)]),             # 6 bb clipped at both chip edges
    ((2, 0), [(3, 5)]),             # 7 IO at y = 0 and y = ny + 1
    ((2, 2), [(1, 1), (4, 4), (1, 4), (4, 1), (3, 2)]),   # 8 multi-sink
    ((0, 2), [(2, 2)]),             # 9 unroutable inside its margin-0 bb
]
TINY_BBGROW = 9


def _tseng_nets():
    rng = np.random.default_rng(11)
    tiles = [(x, y) for x in range(1, 13) for y in range(1, 13)
             if (x, y) != (6, 6)]
    corners = [(1, 1), (12, 12), (1, 12), (12, 1)]
    rest = [t for t in tiles if t not in corners]
    pick = [rest[i] for i in rng.choice(len(rest), 60, replace=False)]
    sinks = pick[:30] + corners + pick[30:]
    return [
        ((6, 6), sinks),                              # 0 the 64-sink net
        ((1, 1), [(12, 12), (12, 1), (5, 9)]),        # 1
        ((12, 1), [(1, 12), (6, 6)]),                 # 2
        ((3, 3), [(9, 4), (2, 11), (11, 10), (6, 7), (4, 2), (10, 2),
                  (7, 12), (12, 6)]),                 # 3 partial rip-up net
        ((1, 4), [(2, 4)]),                           # 4 unroutable at margin 0
    ]


TSENG_BIG, TSENG_PARTIAL, TSENG_BBGROW = 0, 3, 4


@pytest.fixture(scope="module")
def tiny():
    return Ctx("tiny", TINY_NETS)


@pytest.fixture(scope="module")
def tseng():
    return Ctx("tseng", _tseng_nets())


def net_crit(ctx, i, c, k=0):
    """Criticalities of net i: c for a single sink; for a multi-sink net a
    seeded draw from {0, 0.3, 0.7, 1}, so the device order differs from the
    original order and has ties."""
    n = len(ctx.nets[i][1])
    if n == 1:
        return np.asarray([c], dtype=np.float32)
    rng = np.random.default_rng(100 + 7 * i + k)
    return rng.choice(np.asarray([0.0, 0.3, 0.7, 1.0], dtype=np.float32), n)


def seeded_surface(m, seed=3, occ_levels=3):
    """acc in [1, 4) on every node, background occupancy 0 .. occ_levels-1
    on the wires (capacity 1)."""
    rng = np.random.default_rng(seed)
    acc = rng.uniform(1.0, 4.0, m.n).astype(np.float32)
    chan = (m.type == RR_CHANX) | (m.type == RR_CHANY)
    assert (m.cap[chan] == 1).all()
    occ = np.where(chan, rng.integers(0, occ_levels, m.n), 0).astype(np.int32)
    return acc, occ


class Rig:
    """One GpuRouter on a seeded surface plus the host's books: background
    occupancy and every net's current tree."""

    def __init__(self, ctx, label, seed=3, occ_levels=3, **kw):
        import torch
        from parallel_eda_amd.route.gpu_router import GpuRouter
        self.torch = torch
        self.ctx = ctx
        self.m = ctx.m
        self.label = label
        post = {k: kw.pop(k) for k in ("bb_max_small_area", "use_calendar",
                                       "mwg_area_threshold") if k in kw}
        kw.setdefault("n_small_slots", 4)
        kw.setdefault("n_large_slots", 2)
        self.r = GpuRouter(ctx.g, ctx.arch, ctx.src_rr, ctx.sink_ptr,
                           ctx.sink_rr, **kw)
        for k, v in post.items():
            setattr(self.r, k, v)
        self.large = post.get("bb_max_small_area") == 0
        # which kernel and which termination rule each launch really asked
        # for: read from the argument block the router builds
        self.want_calendar = 1 if post.get("use_calendar") else 0
        self.want_strict = 1 if kw.get("deterministic") else 0
        self.launch_flags = []
        make_args = self.r._make_args

        def spy(*a, **k):
            args = make_args(*a, **k)
            self.launch_flags.append((int(args.use_calendar),
                                      int(args.strict_term)))
            return args
        self.r._make_args = spy
        acc, self.base_occ = seeded_surface(self.m, seed, occ_levels)
        self.set_acc(acc)
        self.r.t_occ.copy_(torch.from_numpy(self.base_occ))
        self.trees = {}
        self.crit = np.zeros(len(ctx.sink_rr), dtype=np.float32)

    def set_acc(self, acc):
        self.acc = np.ascontiguousarray(acc, dtype=np.float32)
        self.r.t_acc.copy_(self.torch.from_numpy(self.acc))

    def raise_occ(self, node, by=1):
        self.base_occ[node] += by
        self.r.t_occ[node] += by

    def occ_without(self, inet):
        occ = self.base_occ.astype(np.int64).copy()
        for i, nodes in self.trees.items():
            if i != inet:
                occ += np.bincount(nodes, minlength=self.m.n)
        return occ

    def route(self, inet, crit_net, pres_fac, partial=False, start_len=1,
              check=True):
        """Route net inet alone; validate its tree and check every routed
        sink's cost against the model. Returns (tree, sink_delay of the
        net in original order, records)."""
        r, m, ctx = self.r, self.m, self.ctx
        s0, s1 = int(ctx.sink_ptr[inet]), int(ctx.sink_ptr[inet + 1])
        src, sinks = ctx.nets[inet]
        self.crit[s0:s1] = crit_net
        occ0 = self.occ_without(inet)
        if self.large:
            assert r._bb_areas(r.bb)[inet] > r.bb_max_small_area
        self.launch_flags.clear()
        _, sd = r.route_iteration(self.crit.copy(), pres_fac,
                                  net_subset=[inet], partial=partial)
        assert self.launch_flags and set(self.launch_flags) == {
            (self.want_calendar, self.want_strict)}, self.launch_flags
        tree = r.get_tree(inet)
        occ1 = r.t_occ.cpu().numpy()
        bb = r.bb[inet]
        sd = sd[s0:s1].copy()
        self.trees[inet] = tree[0].astype(np.int64)
        bad = m.validate_tree(tree, src, sinks, bb, sd, occ0, occ1)
        assert bad == [], (self.label, inet, bad)
        if not check:
            return tree, sd, []
        recs = m.replay_tree(tree, sinks, self.crit[s0:s1], bb, occ0,
                             self.acc, pres_fac, r.astar_fac,
                             start_len=start_len)
        st = STATS.setdefault((self.label, float(r.astar_fac)),
                              [0.0, 0.0, 0.0, 0])
        st[2] = max(st[2], m.delay_rel_error(tree))
        for rec in recs:
            assert rec["opt"] is not None, (self.label, inet, rec)
            lo, hi = cost_bounds(rec)
            if rec["opt"] > 0:
                st[0] = max(st[0], rec["cost"] / rec["opt"])
                st[1] = max(st[1], rec["cost"] / (rec["opt"] + rec["eps"]))
            st[3] += 1
            if r.astar_fac == 0:
                assert rec["eps"] == 0.0
            assert rec["cost"] <= hi, (
                f"{self.label} net {inet} sink {rec['sink']} crit "
                f"{rec['crit']}: path cost {rec['cost']!r} above opt "
                f"{rec['opt']!r} + eps {rec['eps']!r} (n {rec['n']})")
            assert rec["cost"] >= lo, (
                f"{self.label} net {inet} sink {rec['sink']} crit "
                f"{rec['crit']}: path cost {rec['cost']!r} BELOW the model's "
                f"optimum {rec['opt']!r}: kernel entered a barred node")
        return tree, sd, recs

    def route_all(self, nets, crits=(0.0, 0.4, 1.0), press=(0.0, 0.7)):
        k = 0
        for pres in press:
            for c in crits:
                for i in nets:
                    k += 1
                    self.route(i, net_crit(self.ctx, i, c, k), pres)


TINY_SET = list(range(9))       # all but the bb-growth net


# ---- 1. single sink (and the small multi-sink net) on tiny ----
@pytest.mark.parametrize("bb_margin", [0, 4])
@pytest.mark.parametrize("astar_fac", [0.0, 1.0])
def test_single_sink_tiny(tiny, astar_fac, bb_margin):
    rig = Rig(tiny, "pingpong", astar_fac=astar_fac, bb_margin=bb_margin)
    rig.route_all(TINY_SET)
    if bb_margin == 0:
        # the one-tile-tight bb is really what was searched: a net the
        # model can route inside it must not have grown, the others must
        inside = [tiny.margin0_routable(i) for i in TINY_SET]
        assert sum(inside) >= 4
        for i, ok in zip(TINY_SET, inside):
            assert (rig.r.bb_margin_per_net[i] == 0) == ok, (i, ok)
    else:
        assert (rig.r.bb_margin_per_net == 4).all()
        # clipped at the chip edge
        assert rig.r.bb[6].tolist() == [0, 0, 5, 5]


@pytest.mark.parametrize("engine", ["pingpong", "calendar", "mwg"])
def test_zero_delay_hop_cannot_reenter_tree(tiny, engine):
    """SOURCE->OPIN hops have zero delay, so at crit exactly 1 a relaxation
    out of the root costs 0.0 and its state word (0.0, source) undercut the
    seed word (0.0, opin) of an OPIN already in the tree whenever
    source < opin: the next path ran through the tree and the OPIN was
    committed twice. Every sink at crit 1 makes each search start that
    way."""
    kw = dict(pingpong={}, calendar=dict(use_calendar=True),
              mwg=dict(mwg_area_threshold=0))[engine]
    rig = Rig(tiny, engine, astar_fac=0.0, **kw)
    m = tiny.m
    src = tiny.nets[8][0]
    opins = m.edge_dst[m.row_ptr[src]:m.row_ptr[src + 1]]
    assert (m.edge_hop[m.row_ptr[src]:m.row_ptr[src + 1]] == 0).all()
    assert (opins > src).any()
    for pres in (0.0, 0.7):
        rig.route(8, np.ones(5, dtype=np.float32), pres)


# ---- 2. multi-sink: the tree passes 256 nodes before the last sink ----
@pytest.fixture(scope="module")
def big_crit(tseng):
    return net_crit(tseng, TSENG_BIG, 0.0)


def _big(rig, crit, press=(0.7, 0.0)):
    """The 64-sink net at both pres_fac (the second call is a reroute).
    The kernel's own tree must cross a 256-entry stride while sinks are
    still to come (the model's does: tests/test_route_model.py)."""
    for pres in press:
        tree, sd, recs = rig.route(TSENG_BIG, crit, pres)
        assert len(tree[0]) - recs[-1]["n"] > 256
    return tree, sd


@pytest.mark.parametrize("astar_fac", [0.0, 1.0])
def test_multi_sink_tseng(tseng, big_crit, astar_fac):
    rig = Rig(tseng, "pingpong", astar_fac=astar_fac)
    r = rig.r
    assert (r._bb_areas(r.bb)[:3] <= r.bb_max_small_area).all()
    rig.route(1, net_crit(tseng, 1, 0.0), 0.7)      # another net's occupancy
    _big(rig, big_crit)
    rig.route(2, net_crit(tseng, 2, 0.0), 0.0)


# ---- 3. dense bb-local index vs global index ----
@pytest.mark.parametrize("astar_fac", [0.0, 1.0])
def test_large_class_tiny(tiny, astar_fac):
    rig = Rig(tiny, "pingpong-large", astar_fac=astar_fac,
              bb_max_small_area=0)
    rig.route_all(TINY_SET)


@pytest.mark.parametrize("astar_fac", [0.0, 1.0])
def test_large_class_tseng(tseng, big_crit, astar_fac):
    rig = Rig(tseng, "pingpong-large", astar_fac=astar_fac,
              bb_max_small_area=0)
    rig.route(1, net_crit(tseng, 1, 0.0), 0.7)
    _big(rig, big_crit)


# ---- 4. determinism at astar_fac = 0 ----
def _same(ta, tb):
    return all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32
                              else a,
                              b.view(np.uint32) if b.dtype == np.float32
                              else b) for a, b in zip(ta, tb))


def test_deterministic_bit_identical(tiny, tseng, big_crit):
    """astar_fac = 0: the lookahead is identically zero, hence admissible,
    and strict termination brings every tie to its fixpoint. Trees and
    sink delays must not depend on the slot class or the run."""
    for ctx, nets in ((tiny, TINY_SET), (tseng, [1, TSENG_BIG, 2])):
        rigs = [Rig(ctx, "pingpong-strict", astar_fac=0.0,
                    deterministic=True),
                Rig(ctx, "pingpong-strict", astar_fac=0.0,
                    deterministic=True),
                Rig(ctx, "pingpong-strict-large", astar_fac=0.0,
                    deterministic=True, bb_max_small_area=0)]
        for c in ((0.0, 0.4, 1.0) if ctx is tiny else (0.0,)):
            for i in nets:
                crit = big_crit if (ctx is tseng and i == TSENG_BIG) \
                    else net_crit(ctx, i, c)
                out = [rig.route(i, crit, 0.7, check=(k == 0))
                       for k, rig in enumerate(rigs)]
                for k in (1, 2):
                    assert _same(out[0][0], out[k][0]), (ctx.arch, i, c, k)
                    assert np.array_equal(out[0][1].view(np.uint32),
                                          out[k][1].view(np.uint32))


# ---- 5. strict termination ----
@pytest.mark.parametrize("astar_fac", [0.0, 1.0])
def test_strict_termination(tiny, tseng, big_crit, astar_fac):
    rig = Rig(tiny, "pingpong-strict", astar_fac=astar_fac,
              deterministic=True)
    rig.route_all(TINY_SET)
    rig = Rig(tseng, "pingpong-strict", astar_fac=astar_fac,
              deterministic=True)
    rig.route(1, net_crit(tseng, 1, 0.0), 0.7)
    _big(rig, big_crit)


# ---- 6. calendar engine ----
@pytest.mark.parametrize("astar_fac", [0.0, 1.0])
def test_calendar_engine(tiny, tseng, big_crit, astar_fac):
    rig = Rig(tiny, "calendar", astar_fac=astar_fac, use_calendar=True)
    rig.route_all(TINY_SET)
    rig = Rig(tseng, "calendar", astar_fac=astar_fac, use_calendar=True)
    rig.route(1, net_crit(tseng, 1, 0.0), 0.7)
    _big(rig, big_crit)


# ---- 7. MWG engine ----
@pytest.mark.parametrize("astar_fac", [0.0, 1.0])
def test_mwg_engine(tiny, tseng, big_crit, astar_fac):
    rig = Rig(tiny, "mwg", astar_fac=astar_fac, mwg_area_threshold=0)
    rig.route_all(TINY_SET)
    assert rig.r._mwg_bufs is not None      # the calls went to the MWG path
    rig = Rig(tseng, "mwg", astar_fac=astar_fac, mwg_area_threshold=0)
    rig.route(1, net_crit(tseng, 1, 0.0), 0.7)
    _big(rig, big_crit)
    assert rig.r._mwg_bufs is not None


# ---- 8. reroute on a changed surface ----
def test_reroute_after_acc_change(tiny, tseng):
    for ctx, i in ((tiny, 8), (tiny, 2), (tseng, 1)):
        rig = Rig(ctx, "pingpong", astar_fac=0.0)
        crit = net_crit(ctx, i, 0.4)
        t1, _, _ = rig.route(i, crit, 0.7)
        rng = np.random.default_rng(99)
        # expensive exactly where the old tree ran
        acc = rng.uniform(1.0, 4.0, ctx.m.n).astype(np.float32)
        acc[t1[0][1:]] *= np.float32(3.0)
        rig.set_acc(acc)
        # validate_tree inside takes the occupancy difference against the
        # books without the first tree: the old tree must be gone
        t2, _, _ = rig.route(i, crit, 0.7)
        assert not np.array_equal(t1[0], t2[0])
        want = rig.base_occ + np.bincount(t2[0], minlength=ctx.m.n)
        assert np.array_equal(rig.r.t_occ.cpu().numpy(), want)


# ---- 9. partial rip-up ----
def test_partial_rip_up(tseng):
    ctx, m, i = tseng, tseng.m, TSENG_PARTIAL
    # no background occupancy: the only overused node is the one raised
    rig = Rig(ctx, "pingpong-partial", astar_fac=0.0, occ_levels=1)
    src, sinks = ctx.nets[i]
    crit = net_crit(ctx, i, 0.0)
    (node, parent, sw, delay), sd0, _ = rig.route(i, crit, 0.7)
    n = len(node)
    # subtree sink counts, from the tree the kernel built
    below = np.zeros(n, dtype=np.int64)
    for k in range(n - 1, 0, -1):
        below[k] += m.type[node[k]] == RR_SINK
        below[parent[k]] += below[k]
    cand = [k for k in range(1, n)
            if m.type[node[k]] in (RR_CHANX, RR_CHANY)
            and 0 < below[k] < len(sinks)]
    assert cand
    x = cand[len(cand) // 2]
    rig.raise_occ(int(node[x]))
    # host replay of the serial drop: a node goes if it is overused or its
    # parent went; the root stays
    occ_now = rig.base_occ + np.bincount(node, minlength=m.n)
    drop = np.zeros(n, dtype=bool)
    for k in range(1, n):
        drop[k] = drop[parent[k]] or occ_now[node[k]] > m.cap[node[k]]
    keep = np.nonzero(~drop)[0]
    remap = -np.ones(n, dtype=np.int64)
    remap[keep] = np.arange(len(keep))
    kept_sinks = [j for j, s in enumerate(sinks) if s in set(node[keep])]
    assert 0 < len(kept_sinks) < len(sinks)
    (node2, parent2, sw2, delay2), sd1, recs = rig.route(
        i, crit, 0.7, partial=True, start_len=len(keep))
    nk = len(keep)
    assert np.array_equal(node2[:nk], node[keep])
    assert np.array_equal(parent2[1:nk], remap[parent[keep][1:]])
    assert parent2[0] == -1
    assert np.array_equal(sw2[:nk], sw[keep])
    assert np.array_equal(delay2[:nk].view(np.uint32),
                          delay[keep].view(np.uint32))
    assert np.array_equal(sd1[kept_sinks].view(np.uint32),
                          sd0[kept_sinks].view(np.uint32))
    assert len(recs) == len(sinks) - len(kept_sinks)


# ---- 10. bb growth ----
@pytest.mark.parametrize("fabric", ["tiny", "tseng"])
def test_bb_growth(tiny, tseng, fabric):
    ctx, i = (tiny, TINY_BBGROW) if fabric == "tiny" else (tseng, TSENG_BBGROW)
    assert not ctx.margin0_routable(i)
    rig = Rig(ctx, "pingpong", astar_fac=0.0, bb_margin=0)
    r = rig.r
    bb0 = r.bb[i].copy()
    rig.route(i, net_crit(ctx, i, 0.4), 0.7)    # optimal for the grown bb
    assert r.bb_margin_per_net[i] > 0
    assert len(r.last_retries) > 0
    assert r.last_retries[0] == (1, [3])        # one net, no path
    assert (r.bb[i][:2] <= bb0[:2]).all() and (r.bb[i][2:] >= bb0[2:]).all()
    assert r._bb_areas(r.bb)[i] > r._bb_areas(bb0[None])[0]


# ---- congestion sweeps, exact ----
SWEEP_N = [1, 255, 256, 257, 2048 * 256 + 1]    # last: one past a full pass


@pytest.mark.parametrize("n", SWEEP_N)
def test_update_acc_exact(n):
    import torch
    from parallel_eda_amd.ops import hip_api
    from parallel_eda_amd.route.gpu_router import ct_ptr
    rng = np.random.default_rng(n)
    occ = rng.integers(0, 5, n).astype(np.int32)
    cap = rng.integers(1, 3, n).astype(np.int16)
    acc = rng.uniform(1.0, 4.0, n).astype(np.float32)
    fac = np.float32(0.3)
    t_occ = torch.from_numpy(occ).cuda()
    t_cap = torch.from_numpy(cap).cuda()
    t_acc = torch.from_numpy(acc).cuda()
    rc = hip_api.lib().pnr_update_acc(
        ct_ptr(t_occ), ct_ptr(t_cap), ct_ptr(t_acc), hip_api.ct.c_float(fac),
        n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    over = np.maximum(occ - cap.astype(np.int32), 0)
    # `acc[i] += over * acc_fac` compiles to one fused multiply-add
    # (v_fmac_f32; device code contracts by default), i.e. a single
    # rounding of the exact acc + over * fac. In float64 the product (3 x
    # 24 bits) and the sum (both within [0.3, 16)) are exact, so rounding
    # that float64 value to float32 once IS the fused result.
    want = np.where(over > 0,
                    (acc.astype(np.float64) +
                     over.astype(np.float64) * np.float64(fac)
                     ).astype(np.float32), acc)
    got = t_acc.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("n", SWEEP_N)
def test_overuse_count_exact(n):
    import torch
    from parallel_eda_amd.ops import hip_api
    from parallel_eda_amd.route.gpu_router import ct_ptr
    rng = np.random.default_rng(n + 1)
    occ = rng.integers(0, 4, n).astype(np.int32)
    cap = rng.integers(1, 3, n).astype(np.int16)
    ty = rng.integers(0, 6, n).astype(np.int8)
    t_out = torch.zeros(8, dtype=torch.int32, device="cuda")
    t_occ = torch.from_numpy(occ).cuda()
    t_cap = torch.from_numpy(cap).cuda()
    t_ty = torch.from_numpy(ty).cuda()
    rc = hip_api.lib().pnr_overuse_count(
        ct_ptr(t_occ), ct_ptr(t_cap), ct_ptr(t_ty), ct_ptr(t_out), n,
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    want = np.bincount(ty[occ > cap], minlength=8)
    assert np.array_equal(t_out.cpu().numpy(), want)


def _synthetic_trees(n_nets, seed):
    """A GpuRouter over n_nets four-sink nets on tiny whose device trees
    are overwritten with seeded random node lists of length 0..300 (the
    sweeps only read tree_node / tree_len), occupancy set to the host
    recount."""
    import torch
    from parallel_eda_amd.route.gpu_router import GpuRouter
    arch = get_arch("tiny")
    g = rrgraph.build_rr_graph(arch)
    ts = np.asarray(g.tile_source); tk = np.asarray(g.tile_sink)
    srcs = ts[ts >= 0]; snks = tk[tk >= 0]
    rng = np.random.default_rng(seed)
    src_rr = srcs[rng.integers(0, len(srcs), n_nets)].astype(np.int32)
    sink_rr = snks[rng.integers(0, len(snks), 4 * n_nets)].astype(np.int32)
    sink_ptr = (4 * np.arange(n_nets + 1)).astype(np.int32)
    r = GpuRouter(g, arch, src_rr, sink_ptr, sink_rr, n_small_slots=4,
                  n_large_slots=2)
    assert np.diff(r.tree_off).min() >= 300
    lens = rng.choice([0, 1, 255, 256, 257, 300], n_nets)
    nodes = np.zeros(int(r.tree_off[-1]), dtype=np.int32)
    trees = []
    for i in range(n_nets):
        t = rng.integers(0, g.num_nodes, int(lens[i])).astype(np.int32)
        nodes[r.tree_off[i]:r.tree_off[i] + len(t)] = t
        trees.append(t)
    r.t_tree_node.copy_(torch.from_numpy(nodes))
    r.t_tree_len.copy_(torch.from_numpy(lens.astype(np.int32)))
    return r, g, trees


def _recount(trees, n, skip=()):
    occ = np.zeros(n, dtype=np.int64)
    for i, t in enumerate(trees):
        if i not in skip:
            occ += np.bincount(t, minlength=n)
    return occ


@pytest.mark.parametrize("n_nets", [1, 255, 256, 257])
def test_congested_nets_and_rip_up_exact(n_nets):
    import torch
    r, g, trees = _synthetic_trees(n_nets, seed=n_nets)
    n = g.num_nodes
    cap = np.asarray(g.capacity).astype(np.int64)
    rng = np.random.default_rng(n_nets + 5)
    # a few overused nodes, so that some nets are clean and some are not
    extra = (rng.random(n) < 0.004).astype(np.int64) * 7
    occ = extra
    r.t_occ.copy_(torch.from_numpy(occ.astype(np.int32)))
    over = occ > cap
    want = {i for i, t in enumerate(trees) if over[t].any()}
    got = r.congested_nets()
    assert set(got.tolist()) == want and len(got) == len(want)
    if n_nets > 1:
        assert 0 < len(want) < n_nets
    # rip-up: occupancy afterwards is the host recount over what remains
    occ = _recount(trees, n) + extra
    r.t_occ.copy_(torch.from_numpy(occ.astype(np.int32)))
    rip = np.arange(0, n_nets, 2)
    r.rip_up_nets(rip)
    want_occ = _recount(trees, n, skip=set(rip.tolist())) + extra
    assert np.array_equal(r.t_occ.cpu().numpy().astype(np.int64), want_occ)
    lens = r.t_tree_len.cpu().numpy()
    assert (lens[rip] == 0).all()
    keep = np.setdiff1d(np.arange(n_nets), rip)
    assert np.array_equal(lens[keep], [len(trees[i]) for i in keep])
