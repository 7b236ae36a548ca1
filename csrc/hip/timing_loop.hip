// Device-resident timing loop — the glue between the placer, the router
// and the STA sweeps (sta_kernel.hip), so that delays and criticalities
// stay in HBM from one engine's kernel to the next:
//
//   placer:  bx/by --place_conn_delay--> conn delay --pnr_sta_analyze-->
//            conn crit --crit_pow--> PlaceDev.conn_crit
//   router:  sink_delay --conn_delay_from_sinks--> conn delay
//            --pnr_sta_analyze--> conn crit --sink_crit--> NetsDev.crit
//
// All four kernels are memory-bound gathers: one element per thread,
// grid-stride, the per-connection (per-sink) streams coalesced, the
// indexed reads (block positions, sink delays, connection criticalities)
// left to the caches. No atomics and no write ordering: every output
// element has exactly one writer.
#include "pnr_hip.h"

#include <cmath>

namespace pnrh {

// Connection delay from the placement through the placer's delay matrix.
// Same indexing as place_kernel.hip net_td_cost: [|dx| * gy + |dy|].
__global__ void tl_place_conn_delay(const int32_t* __restrict__ bx,
                                    const int32_t* __restrict__ by,
                                    const int32_t* __restrict__ conn_driver,
                                    const int32_t* __restrict__ conn_sink,
                                    const float* __restrict__ delay_mat,
                                    int32_t gy, int64_t num_conns,
                                    float* __restrict__ out) {
  int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; c < num_conns; c += (int64_t)gridDim.x * blockDim.x) {
    int32_t d = conn_driver[c], s = conn_sink[c];
    int dx = abs(bx[s] - bx[d]);
    int dy = abs(by[s] - by[d]);
    out[c] = delay_mat[(int64_t)dx * gy + dy];
  }
}

// out = in ^ exp; POW = false is the exp == 1 case, a plain copy (powf
// need not return its argument bit for bit).
template <bool POW>
__global__ void tl_crit_pow(const float* __restrict__ in, float crit_exp,
                            int64_t n, float* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v = in[i];
    out[i] = POW ? powf(v, crit_exp) : v;
  }
}

// Routed-sink delays to connection delays. conn_rsink[c] is the routed
// sink connection c maps onto, or -1 when driver and sink share a tile
// (ConnMap.conn_delays' fill).
__global__ void tl_conn_delay_from_sinks(const float* __restrict__ sink_delay,
                                         const int32_t* __restrict__ conn_rsink,
                                         float fill, int64_t num_conns,
                                         float* __restrict__ out) {
  int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; c < num_conns; c += (int64_t)gridDim.x * blockDim.x) {
    int32_t r = conn_rsink[c];
    out[c] = r < 0 ? fill : sink_delay[r];
  }
}

// Per routed sink: max criticality over its connections (CSR rs_ptr /
// rs_conn), from 0; then the exponent; then the clamp. ConnMap.sink_crit.
template <bool POW>
__global__ void tl_sink_crit(const float* __restrict__ conn_crit,
                             const int64_t* __restrict__ rs_ptr,
                             const int32_t* __restrict__ rs_conn,
                             int64_t n_rsinks, float crit_exp, float max_crit,
                             float* __restrict__ out) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; r < n_rsinks; r += (int64_t)gridDim.x * blockDim.x) {
    float m = 0.0f;
    for (int64_t k = rs_ptr[r]; k < rs_ptr[r + 1]; ++k)
      m = fmaxf(m, conn_crit[rs_conn[k]]);
    if (POW) m = powf(m, crit_exp);
    out[r] = fminf(m, max_crit);
  }
}

static inline int tl_grid(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (int)(g < 2048 ? g : 2048);
}

}  // namespace pnrh

using namespace pnrh;

extern "C" {

int pnr_tl_place_conn_delay(const int32_t* bx, const int32_t* by,
                            const int32_t* conn_driver,
                            const int32_t* conn_sink, const float* delay_mat,
                            int32_t gy, int64_t num_conns, float* out_delay,
                            void* stream) {
  if (num_conns <= 0) return 0;
  hipLaunchKernelGGL(tl_place_conn_delay, dim3(tl_grid(num_conns)), dim3(256),
                     0, (hipStream_t)stream, bx, by, conn_driver, conn_sink,
                     delay_mat, gy, num_conns, out_delay);
  return (int)hipGetLastError();
}

int pnr_tl_crit_pow(const float* crit_in, float crit_exp, int64_t n,
                    float* crit_out, void* stream) {
  if (n <= 0) return 0;
  if (crit_exp == 1.0f)
    hipLaunchKernelGGL(tl_crit_pow<false>, dim3(tl_grid(n)), dim3(256), 0,
                       (hipStream_t)stream, crit_in, crit_exp, n, crit_out);
  else
    hipLaunchKernelGGL(tl_crit_pow<true>, dim3(tl_grid(n)), dim3(256), 0,
                       (hipStream_t)stream, crit_in, crit_exp, n, crit_out);
  return (int)hipGetLastError();
}

int pnr_tl_conn_delay_from_sinks(const float* sink_delay,
                                 const int32_t* conn_rsink, float fill,
                                 int64_t num_conns, float* out_delay,
                                 void* stream) {
  if (num_conns <= 0) return 0;
  hipLaunchKernelGGL(tl_conn_delay_from_sinks, dim3(tl_grid(num_conns)),
                     dim3(256), 0, (hipStream_t)stream, sink_delay, conn_rsink,
                     fill, num_conns, out_delay);
  return (int)hipGetLastError();
}

int pnr_tl_sink_crit(const float* conn_crit, const int64_t* rs_ptr,
                     const int32_t* rs_conn, int64_t n_rsinks, float crit_exp,
                     float max_crit, float* out, void* stream) {
  if (n_rsinks <= 0) return 0;
  if (crit_exp == 1.0f)
    hipLaunchKernelGGL(tl_sink_crit<false>, dim3(tl_grid(n_rsinks)), dim3(256),
                       0, (hipStream_t)stream, conn_crit, rs_ptr, rs_conn,
                       n_rsinks, crit_exp, max_crit, out);
  else
    hipLaunchKernelGGL(tl_sink_crit<true>, dim3(tl_grid(n_rsinks)), dim3(256),
                       0, (hipStream_t)stream, conn_crit, rs_ptr, rs_conn,
                       n_rsinks, crit_exp, max_crit, out);
  return (int)hipGetLastError();
}

}  // extern "C"
