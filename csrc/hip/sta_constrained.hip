// CDNA4 multi-clock STA: the (source, sink) clock-pair analysis, with SDC
// false paths and multicycle paths, shaped for the place and route loops:
// one launch per level for all domains, no host round trip, nothing
// synchronised. The unconstrained analysis is the trivial plan (one backward
// row per sink domain, no false pair, constraint = the sink's period).
//
// Reference semantics: csrc/cpu/sta_serial.cpp analyze_domains (pair_skip /
// pair_mult; do_timing_analysis_new's (src, sink)-domain-pair loop,
// path_delay.c:1996-2085, read_sdc.c). Per source domain a forward max-plus
// sweep of arrivals, per (sink domain, period) row a backward min-minus sweep
// of required times, level by level, then one (connection, pair) pass for
// the worst slack and the largest criticality per connection.
//
// Layout: arr[b * K + ci], req[b * R + row] (block-major, rows interleaved).
// One thread per (block of the level, row) with the row fastest, so the K
// (or R) lanes of one block read the same level_blocks / CSR / delay words
// (one fetch per wave instead of one per domain launch) and their arr / req
// words are adjacent, on the write and on every later gather.
//
// Every constraint comes from host tables (timing/constraints.py): the device
// never multiplies a period by a multiplier, so there is no product for the
// compiler to contract into the subtraction that follows it. The same holds
// for the per-block launch / capture tables (SDC I/O delays on pads): clock
// to Q plus input delay and setup plus output delay are summed on the host;
// a null table means the scalar, and then every bit is what it was without
// the tables.
//
// stc_pair_slack (pnr_sta_pair_slack) is the report side: the least slack per
// (source, sink) pair from the arr / req rows of the last analysis, on
// demand, outside the loops.
#include "pnr_hip.h"

namespace pnrh {

struct StcDev {
  const int32_t* level_blocks;
  const int64_t* in_ptr;
  const int64_t* in_conn;
  const int64_t* out_ptr;
  const int64_t* out_conn;
  const int32_t* conn_driver;
  const int32_t* conn_sink;
  const uint8_t* is_seq;
  const float* blk_delay;        // nullptr => T_clb
  const int32_t* block_clock;    // per block, -1 = no domain
  float T_clb, T_seq_out, T_seq_in, max_crit;
  int32_t num_blocks, K, R;
  int64_t num_conns;
  const float* cons;             // [K*K] setup constraint per pair
  const int32_t* pair_row;       // [K*K] backward row per pair
  const uint8_t* skip;           // [K*K] false pair
  const float* req_period;       // [R]
  const int32_t* req_domain;     // [R]
  float* arr;                    // [num_blocks * K]
  float* req;                    // [num_blocks * R]
  const float* launch;           // per block; nullptr => T_seq_out
  const float* capture;          // per block; nullptr => T_seq_in
};

#define STC_NEG (-3.0e38f)
#define STC_POS (3.0e38f)

// forward, one level, all K source domains: thread -> (block i / K, ci % K)
__global__ void stc_fwd_level(StcDev s, const float* __restrict__ delay,
                              int32_t lv0, int32_t n) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n * s.K) return;
  int32_t i = (int32_t)(t / s.K);
  int32_t ci = (int32_t)(t - (int64_t)i * s.K);
  int32_t b = s.level_blocks[lv0 + i];
  float* out = s.arr + (int64_t)b * s.K + ci;
  if (s.is_seq[b]) {
    float t0 = s.launch ? s.launch[b] : s.T_seq_out;
    *out = (s.block_clock[b] == ci) ? t0 : STC_NEG;
    return;
  }
  float m = STC_NEG;
  for (int64_t k = s.in_ptr[b]; k < s.in_ptr[b + 1]; ++k) {
    int64_t c = s.in_conn[k];
    float v = s.arr[(int64_t)s.conn_driver[c] * s.K + ci];
    if (v > STC_NEG) v += delay[c];
    m = fmaxf(m, v);
  }
  float td = s.blk_delay ? s.blk_delay[b] : s.T_clb;
  *out = (m > STC_NEG) ? m + td : STC_NEG;
}

// backward, one level, all R (sink domain, period) rows
__global__ void stc_bwd_level(StcDev s, const float* __restrict__ delay,
                              int32_t lv0, int32_t n) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n * s.R) return;
  int32_t i = (int32_t)(t / s.R);
  int32_t row = (int32_t)(t - (int64_t)i * s.R);
  int32_t b = s.level_blocks[lv0 + i];
  int32_t cj = s.req_domain[row];
  float period = s.req_period[row];
  float m = STC_POS;
  for (int64_t k = s.out_ptr[b]; k < s.out_ptr[b + 1]; ++k) {
    int64_t c = s.out_conn[k];
    int32_t snk = s.conn_sink[c];
    float ri;
    if (s.is_seq[snk]) {
      // a select, not a branch: the block that drives many flip-flops
      // walks them in one thread, and a branch here costs 5 % (null table)
      // to 19 % (table) of that walk (docs/MEASUREMENTS.md)
      float cap = s.capture ? s.capture[snk] : s.T_seq_in;
      ri = (s.block_clock[snk] == cj) ? period - cap : STC_POS;
    } else {
      float td = s.blk_delay ? s.blk_delay[snk] : s.T_clb;
      float r = s.req[(int64_t)snk * s.R + row];
      ri = (r < STC_POS) ? r - td : STC_POS;
    }
    if (ri < STC_POS) ri -= delay[c];
    m = fminf(m, ri);
  }
  s.req[(int64_t)b * s.R + row] = m;
}

// slack of connection c under pair (ci, cj) = pair; false when the pair is
// false or does not reach the connection
__device__ __forceinline__ bool stc_conn_pair_slack(
    const StcDev& s, const float* __restrict__ delay, int64_t c, int32_t pair,
    float constraint, float* sl) {
  if (s.skip[pair]) return false;             // false path
  int32_t ci = pair / s.K, cj = pair - ci * s.K;
  int32_t drv = s.conn_driver[c];
  int32_t snk = s.conn_sink[c];
  float a = s.arr[(int64_t)drv * s.K + ci];
  if (a <= STC_NEG) return false;
  float ri;
  if (s.is_seq[snk]) {
    float cap = s.capture ? s.capture[snk] : s.T_seq_in;
    ri = (s.block_clock[snk] == cj) ? constraint - cap : STC_POS;
  } else {
    float td = s.blk_delay ? s.blk_delay[snk] : s.T_clb;
    float r = s.req[(int64_t)snk * s.R + s.pair_row[pair]];
    ri = (r < STC_POS) ? r - td : STC_POS;
  }
  if (ri >= STC_POS) return false;
  *sl = ri - (a + delay[c]);
  return true;
}

// order-preserving bits of a float: unsigned order = float order. Slack can
// be negative, so a negative value has all its bits flipped and a
// non-negative one its sign bit set. All-ones (the 0xFF fill) is above the
// bits of +inf, so no atomicMin of a slack leaves it in place: it is the
// sentinel "no pair analysed here". The finish kernels test for it before
// they decode: a connection's slack becomes 0 (stc_finish), a pair's least
// slack +inf (stc_pair_slack_finish).
__device__ __forceinline__ unsigned stc_order_bits(float v) {
  unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the inverse of stc_order_bits
__device__ __forceinline__ float stc_order_value(unsigned b) {
  return __uint_as_float((b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b);
}

// one thread per (conn, ci, cj): worst slack / max criticality per conn and
// the worst achieved period. The worst period is the achieved period of the
// largest achieved / constraint ratio, tracked as one 64-bit max on
// (ratio bits << 32) | achieved bits, so the period always belongs to the
// winning ratio and the result depends on neither launch shape nor order.
// Both halves are non-negative floats (bit order = value order); equal
// ratios keep the larger period. A high half of 0 means no pair analysed.
__global__ void stc_pairs(StcDev s, const float* __restrict__ delay,
                          float* slack, float* crit,
                          unsigned long long* worst) {
  const int64_t KK = (int64_t)s.K * s.K;
  const int64_t total = s.num_conns * KK;
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t c = idx / KK;
    int32_t pair = (int32_t)(idx - c * KK);
    float constraint = s.cons[pair];
    float sl;
    if (!stc_conn_pair_slack(s, delay, c, pair, constraint, &sl)) continue;
    // min slack per conn: atomicMin on order-preserving bits
    atomicMin((unsigned*)&slack[c], stc_order_bits(sl));
    float cr = 1.0f - sl / constraint;
    cr = fminf(fmaxf(cr, 0.0f), s.max_crit);
    atomicMax((unsigned*)&crit[c], __float_as_uint(cr));  // cr >= 0
    float achieved = constraint - sl;
    unsigned long long packed =
        ((unsigned long long)__float_as_uint(achieved / constraint) << 32) |
        __float_as_uint(achieved);
    atomicMax(worst, packed);
  }
}

// decode the slack bits; thread 0 also decodes the worst word into the
// float32 period: no analysed pair (high half 0) => periods[0]
__global__ void stc_finish(int64_t num_conns, float* slack,
                           const unsigned long long* worst,
                           const float* __restrict__ req_period,
                           float* period_out) {
  int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) {
    unsigned long long w = *worst;
    period_out[0] = (w >> 32) ? __uint_as_float((unsigned)(w & 0xFFFFFFFFull))
                              : req_period[0];
  }
  for (; c < num_conns; c += (int64_t)gridDim.x * blockDim.x) {
    unsigned sb = __float_as_uint(slack[c]);
    slack[c] = (sb == 0xFFFFFFFFu) ? 0.0f : stc_order_value(sb);
  }
}

// least slack per pair over all connections, as order-preserving bits in
// out[K*K] (preset to all-ones). One thread per (conn, pair) with the pair
// fastest, so a wave's lanes spread over the words of the table: each
// workgroup takes its minima in an LDS table of K*K words (16 KB at K = 64)
// and then issues one global atomicMin per word it touched, instead of
// num_conns * K * K global atomics onto K * K words.
__global__ void stc_pair_slack(StcDev s, const float* __restrict__ delay,
                               unsigned* out) {
  extern __shared__ unsigned stc_tab[];
  const int32_t KK = s.K * s.K;
  for (int32_t p = threadIdx.x; p < KK; p += blockDim.x)
    stc_tab[p] = 0xFFFFFFFFu;
  __syncthreads();
  const int64_t total = s.num_conns * (int64_t)KK;
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t c = idx / KK;
    int32_t pair = (int32_t)(idx - c * KK);
    float sl;
    if (!stc_conn_pair_slack(s, delay, c, pair, s.cons[pair], &sl)) continue;
    atomicMin(&stc_tab[pair], stc_order_bits(sl));
  }
  __syncthreads();
  for (int32_t p = threadIdx.x; p < KK; p += blockDim.x) {
    unsigned v = stc_tab[p];
    if (v != 0xFFFFFFFFu) atomicMin(&out[p], v);
  }
}

// decode the pair table; all-ones (no analysed connection) => +inf
__global__ void stc_pair_slack_finish(int32_t KK, const unsigned* bits,
                                      float* out) {
  int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= KK) return;
  unsigned sb = bits[p];
  out[p] = (sb == 0xFFFFFFFFu) ? __uint_as_float(0x7F800000u)
                               : stc_order_value(sb);
}

}  // namespace pnrh

using namespace pnrh;

extern "C" {

struct StaConstrainedArgs {
  const int32_t* level_blocks;
  const int64_t* in_ptr; const int64_t* in_conn;
  const int64_t* out_ptr; const int64_t* out_conn;
  const int32_t* conn_driver; const int32_t* conn_sink;
  const uint8_t* is_seq;
  const float* blk_delay;        // nullptr => scalar T_clb
  const int32_t* block_clock;
  float T_clb, T_seq_out, T_seq_in, max_crit;
  int32_t num_blocks, num_levels, K, R;
  int64_t num_conns;
  const float* cons; const int32_t* pair_row; const uint8_t* skip;
  const float* req_period; const int32_t* req_domain;
  float* arr; float* req;
  const float* delay; float* slack; float* crit;
  unsigned long long* worst_bits;   // [1]
  float* period_out;                // [1]
  const int32_t* level_start_host;  // host copy for launch bounds
  const float* launch;              // [num_blocks]; nullptr => T_seq_out
  const float* capture;             // [num_blocks]; nullptr => T_seq_in
};

static bool stc_args_ok(const StaConstrainedArgs* a) {
  return !(a->K < 1 || a->K > 64 || a->R < a->K || a->R > 2 * 64 * 64 ||
           a->num_blocks < 0 || a->num_conns < 0 || a->num_levels < 0);
}

static StcDev stc_dev(const StaConstrainedArgs* a) {
  return StcDev{a->level_blocks, a->in_ptr, a->in_conn, a->out_ptr,
                a->out_conn, a->conn_driver, a->conn_sink, a->is_seq,
                a->blk_delay, a->block_clock, a->T_clb, a->T_seq_out,
                a->T_seq_in, a->max_crit, a->num_blocks, a->K, a->R,
                a->num_conns, a->cons, a->pair_row, a->skip, a->req_period,
                a->req_domain, a->arr, a->req, a->launch, a->capture};
}

int pnr_sta_constrained(const StaConstrainedArgs* a, void* stream) {
  if (!stc_args_ok(a)) return (int)hipErrorInvalidValue;
  StcDev s = stc_dev(a);
  hipStream_t st = (hipStream_t)stream;
  const int32_t* ls = a->level_start_host;
  // the level table must partition [0, num_blocks): it bounds every launch
  if (a->num_levels > 0 && (ls[0] != 0 || ls[a->num_levels] != a->num_blocks))
    return (int)hipErrorInvalidValue;
  hipError_t me;
  me = hipMemsetAsync(a->worst_bits, 0, sizeof(unsigned long long), st);
  if (me != hipSuccess) return (int)me;
  // slack sentinel: all-ones encoded bits (= +inf in the ordering)
  me = hipMemsetAsync(a->slack, 0xFF, a->num_conns * sizeof(float), st);
  if (me != hipSuccess) return (int)me;
  me = hipMemsetAsync(a->crit, 0, a->num_conns * sizeof(float), st);
  if (me != hipSuccess) return (int)me;
  for (int lv = 0; lv < a->num_levels; ++lv) {
    int n = ls[lv + 1] - ls[lv];
    if (n <= 0) continue;
    int64_t th = (int64_t)n * a->K;
    hipLaunchKernelGGL(stc_fwd_level, dim3((unsigned)((th + 255) / 256)),
                       dim3(256), 0, st, s, a->delay, ls[lv], n);
  }
  for (int lv = a->num_levels - 1; lv >= 0; --lv) {
    int n = ls[lv + 1] - ls[lv];
    if (n <= 0) continue;
    int64_t th = (int64_t)n * a->R;
    hipLaunchKernelGGL(stc_bwd_level, dim3((unsigned)((th + 255) / 256)),
                       dim3(256), 0, st, s, a->delay, ls[lv], n);
  }
  int64_t total = a->num_conns * (int64_t)a->K * a->K;
  int64_t g64 = (total + 255) / 256;
  int grid = (int)(g64 < 2048 ? g64 : 2048);
  if (grid > 0)
    hipLaunchKernelGGL(stc_pairs, dim3(grid), dim3(256), 0, st, s, a->delay,
                       a->slack, a->crit, a->worst_bits);
  int64_t c64 = (a->num_conns + 255) / 256;
  int cgrid = (int)(c64 < 2048 ? c64 : 2048);
  if (cgrid < 1) cgrid = 1;  // the period is decoded even without connections
  hipLaunchKernelGGL(stc_finish, dim3(cgrid), dim3(256), 0, st, a->num_conns,
                     a->slack, a->worst_bits, a->req_period, a->period_out);
  return (int)hipGetLastError();
}

// Least slack per (source, sink) pair of the analysis whose arr / req rows
// are in place: a->delay must be the delay vector of that analysis. bits is
// scratch [K*K], out float32 [K*K] (+inf where no connection is analysed).
int pnr_sta_pair_slack(const StaConstrainedArgs* a, unsigned* bits, float* out,
                       void* stream) {
  if (!stc_args_ok(a) || !a->delay || !bits || !out)
    return (int)hipErrorInvalidValue;
  StcDev s = stc_dev(a);
  hipStream_t st = (hipStream_t)stream;
  const int KK = a->K * a->K;
  hipError_t me = hipMemsetAsync(bits, 0xFF, KK * sizeof(unsigned), st);
  if (me != hipSuccess) return (int)me;
  int64_t total = a->num_conns * (int64_t)KK;
  int64_t g64 = (total + 255) / 256;
  int grid = (int)(g64 < 1024 ? g64 : 1024);
  if (grid > 0)
    hipLaunchKernelGGL(stc_pair_slack, dim3(grid), dim3(256),
                       KK * sizeof(unsigned), st, s, a->delay, bits);
  hipLaunchKernelGGL(stc_pair_slack_finish, dim3((KK + 255) / 256), dim3(256),
                     0, st, KK, bits, out);
  return (int)hipGetLastError();
}

int64_t pnr_sta_constrained_args_sizeof() {
  return (int64_t)sizeof(StaConstrainedArgs);
}

}  // extern "C"
