"""Device-resident timing loop: placer/router <-> GpuSTA without the host.

Host side of csrc/hip/timing_loop.hip. The CPU loops refresh timing with
a device->host->device round trip per temperature (placer) or PathFinder
iteration (router); with a GpuSTA the same chain runs as kernels on the
current stream and the delays and criticalities never leave HBM:

  PlaceTiming.refresh   t_bx/t_by -> conn delay -> GpuSTA.analyze_device
                        -> (crit ^ exp) -> placer.t_conn_crit
  RouteTiming.update    sink delay -> conn delay -> GpuSTA.analyze_device
                        -> per-sink max/exp/clamp -> device crit tensor

The placer, the router and GpuSTA all enqueue on
torch.cuda.current_stream(), so stream order alone makes each kernel see
its producer's output.
"""
import ctypes as ct

import numpy as np

from ..ops import hip_api


def _lib():
    lib = hip_api.lib()
    if not hasattr(lib, "_tl_ready"):
        vp = ct.c_void_p
        lib.pnr_tl_place_conn_delay.restype = ct.c_int
        lib.pnr_tl_place_conn_delay.argtypes = [
            vp, vp, vp, vp, vp, ct.c_int32, ct.c_int64, vp, vp]
        lib.pnr_tl_crit_pow.restype = ct.c_int
        lib.pnr_tl_crit_pow.argtypes = [vp, ct.c_float, ct.c_int64, vp, vp]
        lib.pnr_tl_conn_delay_from_sinks.restype = ct.c_int
        lib.pnr_tl_conn_delay_from_sinks.argtypes = [
            vp, vp, ct.c_float, ct.c_int64, vp, vp]
        lib.pnr_tl_sink_crit.restype = ct.c_int
        lib.pnr_tl_sink_crit.argtypes = [
            vp, vp, vp, ct.c_int64, ct.c_float, ct.c_float, vp, vp]
        lib._tl_ready = True
    return lib


def _ptr(t):
    return ct.c_void_p(t.data_ptr())


def _want(t, dtype, numel, what):
    """The kernels index raw pointers: refuse anything but a contiguous
    device tensor of the exact type and length."""
    if (not t.is_cuda or t.dtype != dtype or t.numel() != numel
            or not t.is_contiguous()):
        raise ValueError(
            f"{what}: need a contiguous device {dtype} tensor of {numel} "
            f"elements, got {t.dtype} x {t.numel()} on {t.device}")
    return t


def has_device_timing(sta):
    """True for an STA engine the device loop can drive (GpuSTA)."""
    return hasattr(sta, "analyze_device")


def resolve_device_timing(sta, device_timing):
    """The loops' device_timing keyword: None = on exactly when the engine
    has analyze_device; True without such an engine is an error."""
    if device_timing is None:
        return sta is not None and has_device_timing(sta)
    if device_timing and not has_device_timing(sta):
        raise ValueError("device_timing=True needs a GpuSTA "
                         "(an STA engine with analyze_device)")
    return bool(device_timing)


class PlaceTiming:
    """Per-temperature criticality refresh of a GpuPlacer, on the device."""

    def __init__(self, placer, gsta, crit_exp=1.0):
        torch = placer.torch
        self.torch = torch
        self.placer = placer
        self.gsta = gsta
        self.crit_exp = float(crit_exp)
        nc = placer.nl.num_conns
        nb = placer.nl.num_blocks
        if placer.t_delay_mat is None:
            raise ValueError("PlaceTiming needs GpuPlacer(timing=True)")
        if gsta.num_conns != nc or gsta.netlist.num_blocks != nb:
            raise ValueError("PlaceTiming: placer and GpuSTA were built for "
                             "different netlists")
        if gsta.t_crit.device != placer.t_bx.device:
            raise ValueError("PlaceTiming: placer and GpuSTA are on "
                             "different devices")
        _want(placer.t_bx, torch.int32, nb, "t_bx")
        _want(placer.t_by, torch.int32, nb, "t_by")
        _want(gsta.t_conn_driver, torch.int32, nc, "conn_driver")
        _want(gsta.t_conn_sink, torch.int32, nc, "conn_sink")
        _want(placer.t_delay_mat, torch.float32, placer.gx * placer.gy,
              "delay matrix")
        _want(placer.t_conn_crit, torch.float32, nc, "t_conn_crit")
        self.t_conn_delay = torch.empty(nc, dtype=torch.float32,
                                        device=placer.device)
        self.lib = _lib()

    def refresh(self):
        """Enqueue conn delays -> STA -> criticalities into
        placer.t_conn_crit. No host synchronisation; returns the device
        cpd tensor (valid in stream order)."""
        p, s = self.placer, self.gsta
        nc = p.nl.num_conns
        stream = self.torch.cuda.current_stream().cuda_stream
        rc = self.lib.pnr_tl_place_conn_delay(
            _ptr(p.t_bx), _ptr(p.t_by), _ptr(s.t_conn_driver),
            _ptr(s.t_conn_sink), _ptr(p.t_delay_mat), p.gy, nc,
            _ptr(self.t_conn_delay), stream)
        hip_api.check(rc, "tl_place_conn_delay")
        t_cpd, _slack, t_crit = s.analyze_device(self.t_conn_delay)
        rc = self.lib.pnr_tl_crit_pow(_ptr(t_crit), self.crit_exp, nc,
                                      _ptr(p.t_conn_crit), stream)
        hip_api.check(rc, "tl_crit_pow")
        return t_cpd


def conn_rsink_map(cmap):
    """Inverse of ConnMap.conn/rsink: routed sink per connection, int32,
    -1 where the connection has none (driver and sink share a tile)."""
    conn = np.asarray(cmap.conn, dtype=np.int64)
    rsink = np.asarray(cmap.rsink, dtype=np.int64)
    if len(conn) and (conn.min() < 0 or conn.max() >= cmap.num_conns or
                      rsink.min() < 0 or rsink.max() >= cmap.n_rsinks):
        raise ValueError("ConnMap index out of range")
    out = np.full(cmap.num_conns, -1, dtype=np.int32)
    out[conn] = rsink
    return out


def rsink_conn_csr(cmap):
    """CSR routed sink -> its connections (rs_ptr int64 [n_rsinks+1],
    rs_conn int32), in ConnMap order within a sink."""
    conn = np.asarray(cmap.conn, dtype=np.int64)
    rsink = np.asarray(cmap.rsink, dtype=np.int64)
    order = np.argsort(rsink, kind="stable")
    counts = np.bincount(rsink, minlength=cmap.n_rsinks)
    rs_ptr = np.zeros(cmap.n_rsinks + 1, dtype=np.int64)
    np.cumsum(counts, out=rs_ptr[1:])
    return rs_ptr, conn[order].astype(np.int32)


class RouteTiming:
    """Per-iteration criticality refresh of the GPU router, on the device."""

    def __init__(self, gsta, cmap, intra_delay, max_crit=0.99, crit_exp=1.0,
                 device=None):
        import torch
        self.torch = torch
        self.gsta = gsta
        self.device = device if device is not None else gsta.device
        if cmap.num_conns != gsta.num_conns:
            raise ValueError("RouteTiming: ConnMap and GpuSTA were built "
                             "for different netlists")
        self.num_conns = int(cmap.num_conns)
        self.n_rsinks = int(cmap.n_rsinks)
        self.intra_delay = float(intra_delay)
        self.max_crit = float(max_crit)
        self.crit_exp = float(crit_exp)
        conn_rsink = conn_rsink_map(cmap)        # range-checks the map
        rs_ptr, rs_conn = rsink_conn_csr(cmap)
        self.t_conn_rsink = torch.from_numpy(conn_rsink).to(self.device)
        if self.t_conn_rsink.device != gsta.t_crit.device:
            raise ValueError("RouteTiming: GpuSTA is on another device")
        self.t_rs_ptr = torch.from_numpy(rs_ptr).to(self.device)
        self.t_rs_conn = torch.from_numpy(rs_conn).to(self.device)
        self.t_conn_delay = torch.empty(self.num_conns, dtype=torch.float32,
                                        device=self.device)
        self.t_sink_crit = torch.zeros(self.n_rsinks, dtype=torch.float32,
                                       device=self.device)
        self.lib = _lib()

    def update(self, sink_delays):
        """sink_delays: numpy array (uploaded) or device float32 tensor,
        one per routed sink. Returns (cpd, t_sink_crit); the tensor is
        this object's buffer, overwritten by the next update."""
        torch = self.torch
        if torch.is_tensor(sink_delays):
            t_sd = sink_delays
        else:
            t_sd = torch.from_numpy(np.ascontiguousarray(
                sink_delays, dtype=np.float32)).to(self.device)
        _want(t_sd, torch.float32, self.n_rsinks, "sink_delays")
        stream = torch.cuda.current_stream().cuda_stream
        rc = self.lib.pnr_tl_conn_delay_from_sinks(
            _ptr(t_sd), _ptr(self.t_conn_rsink), self.intra_delay,
            self.num_conns, _ptr(self.t_conn_delay), stream)
        hip_api.check(rc, "tl_conn_delay_from_sinks")
        t_cpd, _slack, t_crit = self.gsta.analyze_device(self.t_conn_delay)
        rc = self.lib.pnr_tl_sink_crit(
            _ptr(t_crit), _ptr(self.t_rs_ptr), _ptr(self.t_rs_conn),
            self.n_rsinks, self.crit_exp, self.max_crit,
            _ptr(self.t_sink_crit), stream)
        hip_api.check(rc, "tl_sink_crit")
        # the loop's one host read per iteration (it also keeps t_sd alive
        # until the kernels that read it have run)
        cpd = float(t_cpd.item())
        return cpd, self.t_sink_crit
