"""Float64 host model of how the GPU router routes ONE net.

The three device engines (router_kernel.hip, router_calendar.hip,
router_mwg.hip) are shortest-path searches over the same cost surface.
This module restates that surface in plain numpy/heapq so a test can say
what the cheapest allowed path of a sink costs and compare the path a
kernel committed against it (tests/test_route_model.py on the host,
tests/test_gpu_router_exact.py on the device).

Cost of entering node w through switch sw, for a sink of criticality c:

    c * hop_delay(sw, w) + (1 - c) * base_cost[type w] * acc[w] * pres(w)
    pres(w) = 1 + max(0, occ[w] + 1 - cap[w]) * pres_fac

Barred: SINKs other than the target, IPINs outside the target's tile,
nodes whose anchor (xlow, ylow) is outside the net's bb, and nodes already
in the net's tree (the kernels store those with an unbeatable state).
Sinks go in descending criticality, ties in original order; each search is
seeded from the tree's non-SINK nodes inside the bb at c * delay(node).

Everything is read from the arrays DevGraph uploads, as float64.
"""
import heapq

import numpy as np

RR_SOURCE, RR_SINK, RR_OPIN, RR_IPIN, RR_CHANX, RR_CHANY = range(6)
U = 2.0 ** -24          # fp32 unit roundoff


class SinkSearch:
    """Result of one sink's search: opt (None if unreachable), one optimal
    path (attach node first, sink last), the optimal g of each path node
    and eps for the astar_fac asked for."""
    __slots__ = ("sink", "crit", "opt", "path", "path_sw", "g", "eps")

    def __init__(self, sink, crit):
        self.sink = sink; self.crit = crit
        self.opt = None; self.path = []; self.path_sw = []; self.g = []
        self.eps = 0.0


class RouteModel:
    def __init__(self, g, arch):
        self.g = g
        self.arch = arch
        self.n = int(g.num_nodes)
        self.type = np.asarray(g.type).astype(np.int64)
        self.xlow = np.asarray(g.xlow).astype(np.int64)
        self.ylow = np.asarray(g.ylow).astype(np.int64)
        self.xhigh = np.asarray(g.xhigh).astype(np.int64)
        self.yhigh = np.asarray(g.yhigh).astype(np.int64)
        self.cap = np.asarray(g.capacity).astype(np.int64)
        self.row_ptr = np.asarray(g.row_ptr).astype(np.int64)
        self.edge_dst = np.asarray(g.edge_dst).astype(np.int64)
        self.edge_sw = np.asarray(g.edge_sw).astype(np.int64)
        self.edge_src = np.repeat(np.arange(self.n), np.diff(self.row_ptr))
        R = np.asarray(g.node_R, dtype=np.float32).astype(np.float64)
        C = np.asarray(g.node_C, dtype=np.float32).astype(np.float64)
        swR = np.asarray(g.sw_R, dtype=np.float32).astype(np.float64)
        swT = np.asarray(g.sw_Tdel, dtype=np.float32).astype(np.float64)
        self.base = np.asarray(g.base_cost, dtype=np.float32).astype(np.float64)
        d, s = self.edge_dst, self.edge_sw
        self.edge_hop = swT[s] + C[d] * (swR[s] + 0.5 * R[d])
        self._R, self._C, self._swR, self._swT = R, C, swR, swT
        self._row = self.row_ptr.tolist()
        self._dst = self.edge_dst.tolist()
        self._edge_of = None
        # lookahead constants exactly as GpuRouter passes them (fp32)
        f32 = lambda v: float(np.float32(v))
        self.seg_delay = f32(arch.T_sw + arch.C_wire * arch.L *
                             (arch.R_sw + 0.5 * arch.R_wire * arch.L))
        self.ipin_delay = f32(arch.T_ipin)
        self.seg_base = f32(arch.base_costs()[4])
        self.ipin_base = f32(arch.base_costs()[3])
        self.L = int(arch.L)

    # ---- cost surface ----
    def hop_delay(self, sw, w):
        return float(self._swT[sw] + self._C[w] *
                     (self._swR[sw] + 0.5 * self._R[w]))

    def pres(self, occ, pres_fac):
        over = np.maximum(0, np.asarray(occ).astype(np.int64) + 1 - self.cap)
        return 1.0 + over * float(np.float32(pres_fac))

    def cong_cost(self, occ, acc, pres_fac):
        """Per-node congestion cost base * acc * pres (cong_mult = 1)."""
        acc = np.asarray(acc, dtype=np.float32).astype(np.float64)
        return self.base[self.type] * acc * self.pres(occ, pres_fac)

    def in_bb(self, bb):
        """The kernels' in_bb: the node's anchor tile only."""
        x0, y0, x1, y1 = (int(v) for v in bb)
        return ((self.xlow >= x0) & (self.xlow <= x1) &
                (self.ylow >= y0) & (self.ylow <= y1))

    def expected_cost(self, sink, crit):
        """The device lookahead for every node (cong_mult = 1), float64."""
        tx, ty = self.xlow[sink], self.ylow[sink]
        dx = np.where(self.xlow > tx, self.xlow - tx,
                      np.where(self.xhigh < tx, tx - self.xhigh, 0))
        dy = np.where(self.ylow > ty, self.ylow - ty,
                      np.where(self.yhigh < ty, ty - self.yhigh, 0))
        nseg = (dx + dy + self.L - 1) // self.L
        cong = nseg * self.seg_base + self.ipin_base
        dl = nseg * self.seg_delay + self.ipin_delay
        h = crit * dl + (1.0 - crit) * cong
        return np.where(self.type == RR_SINK, 0.0, h)

    def allowed(self, sink, bb=None, tree_nodes=()):
        """Nodes a search for `sink` may enter."""
        ok = np.ones(self.n, dtype=bool)
        ok &= ~((self.type == RR_SINK) & (np.arange(self.n) != sink))
        ok &= ~((self.type == RR_IPIN) &
                ((self.xlow != self.xlow[sink]) |
                 (self.ylow != self.ylow[sink])))
        if bb is not None:
            ok &= self.in_bb(bb)
        if len(tree_nodes):
            ok[np.asarray(tree_nodes, dtype=np.int64)] = False
        return ok

    def edge_costs(self, crit, cong):
        crit = float(crit)
        return crit * self.edge_hop + (1.0 - crit) * cong[self.edge_dst]

    # ---- one sink ----
    def search_sink(self, sink, crit, seeds, cong, bb=None, tree_nodes=(),
                    astar_fac=0.0):
        """Multi-source Dijkstra to `sink`. seeds: iterable of
        (node, start_cost)."""
        crit = float(np.float32(crit))
        res = SinkSearch(int(sink), crit)
        ok = self.allowed(sink, bb, tree_nodes)
        ecost = self.edge_costs(crit, cong).tolist()
        eok = ok[self.edge_dst].tolist()
        row, dst = self._row, self._dst
        inf = float("inf")
        dist = [inf] * self.n
        prev_e = [-1] * self.n
        heap = []
        for v, c in seeds:
            v = int(v); c = float(c)
            if c < dist[v]:
                dist[v] = c
                heap.append((c, v))
        heapq.heapify(heap)
        sink = int(sink)
        found = False
        while heap:
            d, v = heapq.heappop(heap)
            if d > dist[v]:
                continue
            if v == sink:
                found = True
                break
            for e in range(row[v], row[v + 1]):
                if not eok[e]:
                    continue
                nd = d + ecost[e]
                w = dst[e]
                if nd < dist[w]:
                    dist[w] = nd
                    prev_e[w] = e
                    heapq.heappush(heap, (nd, w))
        if not found:
            return res
        res.opt = dist[sink]
        path, sws = [sink], []
        v = sink
        while prev_e[v] >= 0:
            e = prev_e[v]
            sws.append(int(self.edge_sw[e]))
            v = int(self.edge_src[e])
            path.append(v)
        path.reverse(); sws.reverse()
        res.path = path
        res.path_sw = sws
        res.g = [dist[u] for u in path]
        if astar_fac:
            h = self.expected_cost(sink, crit)
            res.eps = max([0.0] + [float(astar_fac) * float(h[u]) -
                                   (res.opt - gu)
                                   for u, gu in zip(path[:-1], res.g[:-1])])
        return res

    def cost_to_go(self, sink, crit, cong):
        """Reverse Dijkstra: cheapest allowed cost from every node to
        `sink` (inf where none), no bb and no tree."""
        crit = float(crit)
        ok = self.allowed(sink)
        ecost = self.edge_costs(crit, cong)
        order = np.argsort(self.edge_dst, kind="stable")
        rptr = np.r_[0, np.cumsum(np.bincount(self.edge_dst,
                                              minlength=self.n))].tolist()
        rsrc = self.edge_src[order].tolist()
        rcost = ecost[order].tolist()
        okl = ok.tolist()
        inf = float("inf")
        dist = [inf] * self.n
        dist[int(sink)] = 0.0
        heap = [(0.0, int(sink))]
        while heap:
            d, w = heapq.heappop(heap)
            if d > dist[w]:
                continue
            if not okl[w]:
                continue       # may start a path, may not be entered
            for k in range(rptr[w], rptr[w + 1]):
                v = rsrc[k]
                nd = d + rcost[k]
                if nd < dist[v]:
                    dist[v] = nd
                    heapq.heappush(heap, (nd, v))
        return np.asarray(dist)

    # ---- one net ----
    @staticmethod
    def sink_order(crit):
        """Device order of one net's sinks: descending crit, ties in
        original order (np.lexsort((-crit, net)) within a net)."""
        return np.argsort(-np.asarray(crit, dtype=np.float32), kind="stable")

    def route_net(self, src, sinks, crit, bb, occ, acc, pres_fac,
                  astar_fac=0.0, tree=None):
        """Route a whole net the way a correct kernel would. occ must not
        hold the net's own old tree. tree: (node, parent, sw, delay) to
        keep (partial rip-up), None for root only. Returns the tree as
        four lists, the SinkSearch per routed sink in device order, and
        the occupancy afterwards. A sink already in the tree is skipped;
        an unreachable sink ends the net (its SinkSearch has opt None)."""
        cong = self.cong_cost(occ, acc, pres_fac)
        occ_after = np.asarray(occ).astype(np.int64).copy()
        if tree is None:
            node, parent, sw, delay = [int(src)], [-1], [-1], [0.0]
            occ_after[int(src)] += 1
        else:
            node, parent, sw, delay = (list(map(int, tree[0])),
                                       list(map(int, tree[1])),
                                       list(map(int, tree[2])),
                                       [float(d) for d in tree[3]])
        inbb = self.in_bb(bb)
        out = []
        for j in self.sink_order(crit):
            sink = int(sinks[j]); c = float(np.float32(crit[j]))
            if sink in node:
                continue
            seeds = [(v, c * delay[k]) for k, v in enumerate(node)
                     if self.type[v] != RR_SINK and inbb[v]]
            r = self.search_sink(sink, c, seeds, cong, bb, node, astar_fac)
            out.append(r)
            if r.opt is None:
                break
            par = node.index(r.path[0])
            d = delay[par]
            for u, s in zip(r.path[1:], r.path_sw):
                d += self.hop_delay(s, u)
                node.append(u); parent.append(par); sw.append(s)
                delay.append(d)
                par = len(node) - 1
                occ_after[u] += 1
        return (node, parent, sw, delay), out, occ_after

    def edge_switch(self, u, w):
        """Switch of rr edge u->w, or None if there is no such edge."""
        for e in range(self._row[u], self._row[u + 1]):
            if self._dst[e] == w:
                return int(self.edge_sw[e])
        return None

    def replay_tree(self, tree, sinks, crit, bb, occ, acc, pres_fac,
                    astar_fac, start_len=1):
        """Judge the paths a kernel committed. tree = get_tree(inet); its
        entries [start_len:] were appended sink by sink in device order
        (start_len > 1: the part a partial rip-up kept). occ: occupancy
        the searches saw, i.e. without any of this net's nodes beyond what
        other nets put there. For each routed sink, seeds are the kernel's
        own tree so far with the kernel's fp32 delays. Returns a list of
        dicts: sink, j (original index), crit, opt, eps, cost (float64
        cost of the kernel's path from its attach node), n (hops, larger
        of the two paths)."""
        node, parent, sw, delay = (np.asarray(a) for a in tree)
        node_l = node.tolist()
        cong = self.cong_cost(occ, acc, pres_fac)
        inbb = self.in_bb(bb)
        kept = set(node_l[:start_len])
        out = []
        lo = start_len
        for j in self.sink_order(crit):
            sink = int(sinks[j]); c = float(np.float32(crit[j]))
            if sink in kept:
                continue
            hi = node_l.index(sink, lo)         # ValueError: sink missing
            seeds = [(v, c * float(delay[k]))
                     for k, v in enumerate(node_l[:lo])
                     if self.type[v] != RR_SINK and inbb[v]]
            r = self.search_sink(sink, c, seeds, cong, bb, node_l[:lo],
                                 astar_fac)
            attach = int(parent[lo])
            assert 0 <= attach < lo, "path does not start at the tree so far"
            cost = c * float(delay[attach])
            for k in range(lo, hi + 1):
                assert int(parent[k]) == (attach if k == lo else k - 1), \
                    "a sink's path is not one chain"
                w = node_l[k]
                cost += (c * self.hop_delay(int(sw[k]), w) +
                         (1.0 - c) * float(cong[w]))
            out.append(dict(sink=sink, j=int(j), crit=c, opt=r.opt,
                            eps=r.eps, cost=cost,
                            n=max(hi + 1 - lo, len(r.path) - 1)))
            lo = hi + 1
        assert lo == len(node_l), "tree entries after the last sink"
        return out

    # ---- tree validator ----
    def validate_tree(self, tree, src, sinks, bb, sink_delay, occ_before,
                      occ_after):
        """Every structural property of a committed route tree. sinks and
        sink_delay are the net's own, in ORIGINAL order; occ_before holds
        nothing of this net. Returns a list of findings (empty: valid)."""
        node, parent, sw, delay = (np.asarray(a) for a in tree)
        bad = []
        n = len(node)
        if n == 0 or int(node[0]) != int(src) or int(parent[0]) != -1:
            return ["root is not the source with parent -1"]
        if ((node < 0) | (node >= self.n)).any():
            return ["node id out of range"]
        if len(set(node.tolist())) != n:
            bad.append("a node occurs twice")
        inbb = self.in_bb(bb)
        out = np.nonzero(~inbb[node])[0]
        if len(out):
            bad.append(f"node {int(node[out[0]])} at entry {int(out[0])} "
                       f"is outside the bb")
        d64 = np.zeros(n)
        depth = np.zeros(n, dtype=np.int64)
        has_child = np.zeros(n, dtype=bool)
        for k in range(1, n):
            p = int(parent[k])
            if not 0 <= p < k:
                bad.append(f"entry {k}: parent {p} is not an earlier entry")
                return bad
            has_child[p] = True
            s = self.edge_switch(int(node[p]), int(node[k]))
            if s is None:
                bad.append(f"entry {k}: {int(node[p])}->{int(node[k])} "
                           f"is not an rr edge")
                continue
            if s != int(sw[k]) and not self._has_edge_sw(
                    int(node[p]), int(node[k]), int(sw[k])):
                bad.append(f"entry {k}: switch {int(sw[k])}, edge has {s}")
                continue
            depth[k] = depth[p] + 1
            d64[k] = d64[p] + self.hop_delay(int(sw[k]), int(node[k]))
            err = abs(float(delay[k]) - d64[k])
            if err > 4 * depth[k] * U * d64[k]:
                bad.append(f"entry {k}: delay {float(delay[k])!r} vs Elmore "
                           f"sum {d64[k]!r} at depth {int(depth[k])}")
        is_sink = self.type[node] == RR_SINK
        if (is_sink & has_child).any():
            bad.append("a SINK node has a child")
        node_l = node.tolist()
        for j, s in enumerate(sinks):
            cnt = node_l.count(int(s))
            if cnt != 1:
                bad.append(f"sink {int(s)} occurs {cnt} times")
                continue
            k = node_l.index(int(s))
            a = np.asarray(sink_delay[j], dtype=np.float32)
            b = np.asarray(delay[k], dtype=np.float32)
            if a.view(np.uint32) != b.view(np.uint32):
                bad.append(f"sink_delay[{j}] = {float(a)!r} is not the tree "
                           f"delay {float(b)!r} of sink {int(s)}")
        diff = (np.asarray(occ_after).astype(np.int64) -
                np.asarray(occ_before).astype(np.int64))
        want = np.bincount(node, minlength=self.n)
        if not np.array_equal(diff, want):
            w = int(np.nonzero(diff != want)[0][0])
            bad.append(f"occupancy of node {w} moved by {int(diff[w])}, "
                       f"tree holds it {int(want[w])} times")
        return bad

    def delay_rel_error(self, tree):
        """Largest relative error of tree_delay against the float64 Elmore
        sum along each root path (for a tree that passed validate_tree)."""
        node, parent, sw, delay = (np.asarray(a) for a in tree)
        d64 = np.zeros(len(node))
        worst = 0.0
        for k in range(1, len(node)):
            d64[k] = d64[int(parent[k])] + self.hop_delay(int(sw[k]),
                                                          int(node[k]))
            if d64[k] > 0:
                worst = max(worst, abs(float(delay[k]) - d64[k]) / d64[k])
        return worst

    def _has_edge_sw(self, u, w, s):
        return any(self._dst[e] == w and int(self.edge_sw[e]) == s
                   for e in range(self._row[u], self._row[u + 1]))


def cost_bounds(rec):
    """(lower, upper) the recomputed fp64 cost of a kernel's path must lie
    in: each relaxation is at most 8 fp32 roundings relative to the running
    cost, once along the kernel's path and once along the optimal one."""
    slack = 16 * rec["n"] * U
    return (rec["opt"] * (1 - slack),
            (rec["opt"] + rec["eps"]) * (1 + slack))
