// CDNA4 batched simulated-annealing placer.
//
// Re-designs the reference's serial try_swap loop (vpr/SRC/place/place.c:1252
// try_swap, update_bb:2292, get_net_cost:2204, comp_delta_td_cost) as
// batches of parallel moves. One batch is three phases, one wavefront per
// move in each:
//   propose  lane 0 draws a range-limited move, swap or carry-chain shift;
//            the wave evaluates the EXACT bb+timing delta against the
//            frozen pre-batch state, runs Metropolis, records an accepted
//            move in mv_* and claims its nets and tiles;
//   resolve  a move wins if it holds every claim it took. Priority is the
//            move index, so the winner set is deterministic;
//   apply    winners refresh their nets' cached costs and commit grid and
//            positions. Winners touch disjoint nets and tiles, so their
//            deltas are exact and additive: a sequential-equivalent batch.
// Each phase exists once (propose_move, resolve_move, apply_move). Two
// drivers run it and must agree to the bit (tests/test_gpu_place_run.py):
//   pnr_place_batch  reset, propose, resolve, apply: four launches, stop
//                    rule on the host, MinClaims, DirectCounters. Kept as
//                    the oracle.
//   pnr_place_run    propose, then resolve + apply fused into one commit
//                    launch; stop rule on the device, EpochClaims (no
//                    reset), ShardCounters folded by the stop rule; many
//                    batches per call.
// They differ in the claim policy, the counter policy, the launches and
// the stop rule only (docs/KERNELS.md, placer section).
#include "pnr_hip.h"

namespace pnrh {

struct PlaceDev {
  // netlist
  const int32_t* net_blk_ptr;   // [num_nets+1] CSR: net -> member blocks
  const int32_t* net_blks;      //   (driver first, then sinks; may repeat)
  const int32_t* blk_net_ptr;   // [num_blocks+1] CSR: block -> nets (deduped)
  const int32_t* blk_nets;
  const int8_t* blk_type;       // 0=IO 1=CLB 2=RAM 3=DSP
  const int8_t* tile_btype;     // [gx*gy] tile block type, -1 corner;
                                // nullptr => homogeneous (perimeter IO)
  const int32_t* type_cols;     // sorted column lists: RAM cols then DSP
  const int32_t* type_col_ptr;  // [3] bounds into type_cols (RAM, DSP)
  const uint8_t* fixed;         // per-block pin-down mask; nullptr = none
  const float* net_q;           // crossing factor per net
  // timing
  const int32_t* net_sink_ptr;  // [num_nets+1] conn ranges
  const float* conn_crit;       // per conn
  const float* delay_mat;       // [gx*gy] |dx|*gy+|dy|
  // placement state
  int32_t* bx;
  int32_t* by;
  int32_t* bslot;
  int32_t* grid;                // [(x*gy+y)*cap + slot] -> block or -1
  float* net_cost;              // current bb cost per net
  float* net_tcost;             // current timing cost per net
  int32_t num_blocks, num_nets, gx, gy, cap, nx, ny, io_cap;
  int32_t rx0, rx1;             // move region (column strip) for the
                                // distributed strip-sharded anneal
                                // (parallel/dist_place.py); rx0 < 0 = off
  // carry-chain macros (reference: place_macro.c): rigid block groups
  // moved as one. macro_of: [num_blocks] macro id or -1 (nullptr = no
  // macros); macro_ptr/macro_blk: CSR of member blocks.
  const int32_t* macro_of;
  const int32_t* macro_ptr;
  const int32_t* macro_blk;
};

struct MovesDev {
  int32_t* mv_blk;      // proposer's block
  int32_t* mv_to;       // encoded dest (x*gy+y)*cap+slot; macro: see below
  int32_t* mv_other;    // block swapped with, -1 = none, -2 - mid = macro
  float* mv_dbb;        // exact bb delta
  float* mv_dtd;        // exact td delta
  uint8_t* mv_flags;    // 1 = Metropolis-accepted candidate; 2 = winner
  int32_t* net_claim;   // [num_nets] MinClaims words (pnr_place_batch)
  int32_t* loc_claim;   // [gx*gy] the same, tile granularity
  int32_t* counters;    // [4]: attempts, accepted, winners, conflicts, over
                        // all batches of a run_batches call (host zeroes).
                        // pnr_place_batch adds to them directly; in
                        // pnr_place_run they are the totals that the stop
                        // rule folds from the shards (see ShardCounters)
  // stored costs [n_moves x cost_k]: what propose found net_cost and
  // net_tcost of an accepted single move's nets to be after the move.
  // Slot k is the k-th net of blk, slot nets(blk) + k the k-th of other;
  // the slot of a net of other that blk has too holds COST_NONE.
  float* mv_ncost;
  float* mv_ntcost;     // written and read only when timing_tradeoff > 0
  int32_t cost_k;       // <= 64
  int32_t n_moves;
};

// mv_to bit of a single move whose costs are not stored (more nets than
// cost_k): apply recomputes them. Tile codes stay below it (host-checked).
#define MV_RECOMPUTE (1 << 30)
// no bb cost is negative (net_q >= 1, span >= 2)
#define COST_NONE (-1.0f)

// what one batch's propose is run with
struct Sched {
  float T; int rlim; float timing_tradeoff, inv_bb_norm, inv_td_norm;
  uint32_t seed, batch;
};

#define PROP_WAVES 4

// one wave64 per move, PROP_WAVES waves per workgroup
__device__ __forceinline__ int move_index() {
  return blockIdx.x * PROP_WAVES + (threadIdx.x >> 6);
}

__device__ __forceinline__ uint32_t rng_hash(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t h = a * 0x9E3779B9u ^ b * 0x85EBCA6Bu ^ c * 0xC2B2AE35u;
  h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
  return h;
}

__device__ __forceinline__ bool is_io_loc(const PlaceDev& p, int x, int y) {
  return x == 0 || x == p.gx - 1 || y == 0 || y == p.gy - 1;
}
__device__ __forceinline__ int cap_at(const PlaceDev& p, int x, int y) {
  bool io = is_io_loc(p, x, y);
  if (!io && x >= 1 && x <= p.nx && y >= 1 && y <= p.ny) return 1;
  if (io && ((x >= 1 && x <= p.nx) != (y >= 1 && y <= p.ny))) return p.io_cap;
  return 0;
}

// ---- where block b would be after a move: the position overrides ----
// SwapPos: up to two blocks placed elsewhere (move or swap; -1 = no block)
struct SwapPos {
  int32_t b1; int x1, y1; int32_t b2; int x2, y2;
  __device__ __forceinline__ void operator()(
      const PlaceDev&, int32_t b, int& x, int& y) const {
    if (b == b1) { x = x1; y = y1; }
    else if (b == b2) { x = x2; y = y2; }
  }
};
// every member of macro `mid` displaced by (ddx, ddy)
struct MacroPos {
  int mid, ddx, ddy;
  __device__ __forceinline__ void operator()(
      const PlaceDev& p, int32_t b, int& x, int& y) const {
    if (p.macro_of[b] == mid) { x += ddx; y += ddy; }
  }
};

// ---- pinned arithmetic ------------------------------------------------
// The digests of tests/golden pin these bits, so the roundings are spelled
// out and do not depend on what the compiler contracts (docs/KERNELS.md,
// placer section, "bit-exactness rules"):
//   cached cost   q * span, rounded            (mul_rn)
//   bb delta      fma(q, span, -net_cost[n])   (one rounding)
//   timing chain  t = fma(crit, delay, t) over the sinks in CSR order
//   td delta      t - net_tcost[n]
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// half perimeter of net n's bounding box, its members at `pos`
template <class Pos> __device__ __forceinline__
int net_span(const PlaceDev& p, int n, const Pos& pos) {
  int xmin = 1 << 28, xmax = -1, ymin = 1 << 28, ymax = -1;
  int32_t e0 = p.net_blk_ptr[n], e1 = p.net_blk_ptr[n + 1];
  for (int32_t e = e0; e < e1; ++e) {
    int32_t b = p.net_blks[e];
    int x = p.bx[b], y = p.by[b];
    pos(p, b, x, y);
    xmin = min(xmin, x); xmax = max(xmax, x);
    ymin = min(ymin, y); ymax = max(ymax, y);
  }
  return (xmax - xmin + 1) + (ymax - ymin + 1);
}

// bb cost of net n with its members at `pos`
template <class Pos> __device__ __forceinline__
float net_bb_cost(const PlaceDev& p, int n, const Pos& pos) {
  return mul_rn(p.net_q[n], (float)net_span(p, n, pos));
}

// timing cost of net n (sum over conns of crit * delay), members at `pos`
template <class Pos> __device__ __forceinline__
float net_td_cost(const PlaceDev& p, int n, const Pos& pos) {
  if (p.delay_mat == nullptr) return 0.0f;
  int32_t e0 = p.net_blk_ptr[n], e1 = p.net_blk_ptr[n + 1];
  int32_t drv = p.net_blks[e0];
  int dx0 = p.bx[drv], dy0 = p.by[drv];
  pos(p, drv, dx0, dy0);
  float t = 0.0f;
  int32_t c0 = p.net_sink_ptr[n];
  for (int32_t e = e0 + 1; e < e1; ++e) {
    int32_t b = p.net_blks[e];
    int x = p.bx[b], y = p.by[b];
    pos(p, b, x, y);
    int dx = abs(x - dx0), dy = abs(y - dy0);
    t = __builtin_fmaf(p.conn_crit[c0 + (e - e0 - 1)],
                       p.delay_mat[dx * p.gy + dy], t);
  }
  return t;
}

__device__ __forceinline__ float wave_sum_f32(float v) {
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// binary search in block b's sorted net list
__device__ __forceinline__
bool blk_has_net(const PlaceDev& p, int32_t b, int32_t n) {
  int32_t lo = p.blk_net_ptr[b], hi = p.blk_net_ptr[b + 1];
  while (lo < hi) {
    int32_t mid2 = (lo + hi) >> 1;
    if (p.blk_nets[mid2] < n) lo = mid2 + 1; else hi = mid2;
  }
  return lo < p.blk_net_ptr[b + 1] && p.blk_nets[lo] == n;
}

// f(k, n) for the k-th net n of block b, strided over the wave's lanes
template <class F> __device__ __forceinline__
void for_blk_nets_k(const PlaceDev& p, int32_t b, F f) {
  const int32_t k0 = p.blk_net_ptr[b];
  for (int32_t k = k0 + (threadIdx.x & 63); k < p.blk_net_ptr[b + 1]; k += 64)
    f(k - k0, p.blk_nets[k]);
}
// f(n) for each net n of block b
template <class F> __device__ __forceinline__
void for_blk_nets(const PlaceDev& p, int32_t b, F f) {
  for_blk_nets_k(p, b, [&](int32_t, int32_t n) { f(n); });
}
// f(j, n) for each net n of each member macro_blk[j] of a macro
template <class F> __device__ __forceinline__
void for_macro_nets(const PlaceDev& p, int32_t mm0, int32_t mm1, F f) {
  for (int32_t j = mm0; j < mm1; ++j)
    for_blk_nets(p, p.macro_blk[j], [&](int32_t n) { f(j, n); });
}

// ---- claim policies ------------------------------------------------
// A move takes the word of every net and tile it touches and wins if it
// still holds them all after every move of the batch has taken its own.
// Both policies give a word to the lowest move index that took it.
// MinClaims (pnr_place_batch): int32 words, reset to INT_MAX before every
// batch, taken with atomicMin of the move index.
struct MinClaims {
  int32_t* net; int32_t* loc; int32_t mine;
  __device__ __forceinline__ void take_net(int n) const { atomicMin(&net[n], mine); }
  __device__ __forceinline__ void take_loc(int t) const { atomicMin(&loc[t], mine); }
  __device__ __forceinline__ bool holds_net(int n) const { return net[n] == mine; }
  __device__ __forceinline__ bool holds_loc(int t) const { return loc[t] == mine; }
};
// EpochClaims (pnr_place_run): 64-bit epoch keys taken with atomicMax,
//   key = (uint64(batch) << 32) | (0xFFFFFFFF - move index)
// A later batch beats every stale word, so the arrays are zeroed once at
// construction (batch numbers start at 1) and never reset; within a batch
// the lowest move index has the largest key. The batch counter is 32
// bits: it wraps after 4 G batches and nothing guards against that.
struct EpochClaims {
  unsigned long long* net; unsigned long long* loc; unsigned long long mine;
  __device__ __forceinline__ void take_net(int n) const { atomicMax(&net[n], mine); }
  __device__ __forceinline__ void take_loc(int t) const { atomicMax(&loc[t], mine); }
  __device__ __forceinline__ bool holds_net(int n) const { return net[n] == mine; }
  __device__ __forceinline__ bool holds_loc(int t) const { return loc[t] == mine; }
};

__device__ __forceinline__ unsigned long long claim_key(uint32_t batch, int i) {
  return ((unsigned long long)batch << 32) | (0xFFFFFFFFu - (uint32_t)i);
}

// ---- counter policies ------------------------------------------------
// Every valid proposal, accepted move and verdict counts one, from lane 0.
// Integer sums do not depend on order, so both policies give the same
// totals.
enum { CNT_ATTEMPTS = 0, CNT_ACCEPTED = 1, CNT_WINNERS = 2, CNT_CONFLICTS = 3 };
// DirectCounters (pnr_place_batch): the four words of MovesDev::counters,
// which the host reads after a synchronise.
struct DirectCounters {
  int32_t* w;
  __device__ __forceinline__ void add(int k) const { atomicAdd(&w[k], 1); }
};
// ShardCounters (pnr_place_run): S shards (a power of two), each a 128-byte
// line of its own that holds the shard's four counters in its first words.
// A workgroup adds to shard blockIdx.x & (S - 1), so a line queues the
// atomics of n_workgroups / S workgroups and not of the whole launch. The
// stop rule of place_commit_kernel folds the shards into
// MovesDev::counters.
#define SHARD_WORDS 32   // int32 words of a 128-byte line
struct ShardCounters {
  int32_t* w;   // this workgroup's shard
  __device__ __forceinline__ ShardCounters(int32_t* shards, int32_t mask)
      : w(shards + (int64_t)(blockIdx.x & mask) * SHARD_WORDS) {}
  __device__ __forceinline__ void add(int k) const { atomicAdd(&w[k], 1); }
};

// ---- propose -------------------------------------------------------
// lane-0 candidate selection (same RNG stream as the round-1 per-thread
// kernel); returns the block or -1, target via out-params
__device__ __forceinline__
int propose_select(const PlaceDev& p, int rlim, uint32_t seed, uint32_t batch,
                   int i, int& x1o, int& y1o, int& slot1o) {
  uint32_t r0 = rng_hash(seed ^ 0x5BD1E995u, batch, i);
  int32_t blk = r0 % p.num_blocks;
  if (p.fixed && p.fixed[blk]) return -1;
  if (p.rx0 >= 0 && (p.bx[blk] < p.rx0 || p.bx[blk] > p.rx1))
    return -1;
  bool io = p.blk_type[blk] == 0;
  int x0 = p.bx[blk], y0 = p.by[blk];
  int x1 = -1, y1 = -1, slot1 = 0;
  int bt = p.blk_type[blk];
  if (p.tile_btype && bt >= 2 && p.type_cols) {
    // sparse column type (RAM/DSP): draw the target column from this
    // type's sorted column list clipped to the range window — rejection
    // over the square window would nearly always miss sparse columns
    // (mirrors the CPU placer's find_to for column types).
    int c0 = p.type_col_ptr[bt - 2], c1 = p.type_col_ptr[bt - 1];
    int lo = c0, hi = c1;              // first col >= x0 - rlim
    while (lo < hi) { int m = (lo + hi) >> 1;
                      if (p.type_cols[m] < x0 - rlim) lo = m + 1; else hi = m; }
    int lo2 = lo, hi2 = c1;            // first col > x0 + rlim
    while (lo2 < hi2) { int m = (lo2 + hi2) >> 1;
                        if (p.type_cols[m] <= x0 + rlim) lo2 = m + 1; else hi2 = m; }
    int ncol = lo2 - lo;
    if (ncol > 0) {
      int ylo = max(1, y0 - rlim), yhi = min(p.ny, y0 + rlim);
      for (int att = 0; att < 8; ++att) {
        uint32_t r1 = rng_hash(seed, batch, i * 131 + 7 * att + 1);
        uint32_t r2 = rng_hash(seed, batch, i * 131 + 7 * att + 2);
        int tx = p.type_cols[lo + (int)(r1 % ncol)];
        if (p.rx0 >= 0 && (tx < p.rx0 || tx > p.rx1)) continue;
        int ty = ylo + (int)(r2 % (yhi - ylo + 1));
        if (tx == x0 && ty == y0) continue;
        x1 = tx; y1 = ty; slot1 = 0;
        break;
      }
    }
  } else {
    for (int att = 0; att < 8; ++att) {
      uint32_t r1 = rng_hash(seed, batch, i * 131 + 7 * att + 1);
      uint32_t r2 = rng_hash(seed, batch, i * 131 + 7 * att + 2);
      int tx = x0 + (int)(r1 % (2 * rlim + 1)) - rlim;
      int ty = y0 + (int)(r2 % (2 * rlim + 1)) - rlim;
      if (tx < 0 || tx >= p.gx || ty < 0 || ty >= p.gy) continue;
      if (p.rx0 >= 0 && (tx < p.rx0 || tx > p.rx1)) continue;
      if (p.tile_btype) {
        // heterogeneous fabric: destination tile must match the block type
        if (p.tile_btype[tx * p.gy + ty] != p.blk_type[blk]) continue;
      } else if (is_io_loc(p, tx, ty) != io) continue;
      int c = cap_at(p, tx, ty);
      if (c <= 0) continue;
      if (tx == x0 && ty == y0) continue;
      x1 = tx; y1 = ty;
      slot1 = (int)(rng_hash(seed, batch, i * 131 + 7 * att + 3) % c);
      break;
    }
  }
  if (x1 < 0) return -1;
  x1o = x1; y1o = y1; slot1o = slot1;
  return blk;
}

// may every member of macro ms.mid shift by (ddx, ddy)? (lane 0 only)
__device__ __forceinline__
bool macro_shift_ok(const PlaceDev& p, const MacroPos& ms, int32_t mm0,
                    int32_t mm1) {
  for (int32_t j = mm0; j < mm1; ++j) {
    int32_t b = p.macro_blk[j];
    int sx = p.bx[b], sy = p.by[b];
    int tx = sx + ms.ddx, ty = sy + ms.ddy;
    if (p.fixed && p.fixed[b]) return false;
    if (tx < 0 || tx >= p.gx || ty < 0 || ty >= p.gy) return false;
    if (p.rx0 >= 0 && (tx < p.rx0 || tx > p.rx1 ||
                       sx < p.rx0 || sx > p.rx1)) return false;
    if (p.tile_btype
            ? (p.tile_btype[tx * p.gy + ty] != p.blk_type[b])
            : (is_io_loc(p, tx, ty) != (p.blk_type[b] == 0))) return false;
    if (cap_at(p, tx, ty) != 1) return false;
    int32_t occ = p.grid[((int64_t)tx * p.gy + ty) * p.cap];
    if (occ >= 0 && p.macro_of[occ] != ms.mid) return false;
  }
  return true;
}

// net n's costs after a move, as refresh_net would cache them
struct NetCosts { float bb, td; };

// Adds this lane's share of net n's exact delta under `pos`; returns the
// costs the delta was taken from.
template <class Pos> __device__ __forceinline__
NetCosts add_net_delta(const PlaceDev& p, int32_t n, const Pos& pos,
                       float timing_tradeoff, float& dbb, float& dtd) {
  const float q = p.net_q[n], span = (float)net_span(p, n, pos);
  NetCosts c{mul_rn(q, span), 0.0f};
  dbb += __builtin_fmaf(q, span, -p.net_cost[n]);
  if (timing_tradeoff > 0.0f) {
    c.td = net_td_cost(p, n, pos);
    dtd += c.td - p.net_tcost[n];
  }
  return c;
}

// ---- member-parallel evaluation of a single move ---------------------
// The serial form above gives a lane a whole net: two dependent loads per
// member, walked twice (bb, td), one member after the other. Here the
// (net, member) pairs of all nets of blk and other are spread over the
// lanes, 64 per pass, so the chain is a handful of loads deep whatever
// the nets' sizes. Per-wave LDS staging; the waves of a workgroup take
// different paths, so nothing here is a workgroup barrier.
#define EVAL_SLOTS 64    // nets of blk and of other together
#define EVAL_ITEMS 256   // members of those nets together
struct EvalStage {
  // per slot: slot k < nets(blk) is blk's k-th net, then other's nets
  int32_t incl[EVAL_SLOTS];   // inclusive prefix sum of the member counts
  int32_t e0[EVAL_SLOTS];     // net_blk_ptr[n]
  int32_t c0[EVAL_SLOTS];     // net_sink_ptr[n]
  int32_t drvx[EVAL_SLOTS], drvy[EVAL_SLOTS];   // driver after the move
  int32_t xmin[EVAL_SLOTS], xmax[EVAL_SLOTS];
  int32_t ymin[EVAL_SLOTS], ymax[EVAL_SLOTS];
  // per item, sinks only: the factors of the timing chain
  float crit[EVAL_ITEMS], delay[EVAL_ITEMS];
};

// orders this wave's LDS writes before its later LDS reads. A wave's LDS
// instructions execute in issue order; this keeps the compiler to it.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// What the two for_blk_nets_k loops of the single-move branch compute, to
// the bit: lane k ends with dbb = 0 + delta(k-th net of blk) + delta(k-th
// net of other, unless blk has it too), dtd likewise, and ca/cb hold those
// two nets' costs after the move (cb.bb == COST_NONE for a shared net).
// Needs n_a + n_b <= EVAL_SLOTS; returns false, with nothing touched, if
// the nets have more than EVAL_ITEMS members together (wave-uniform).
__device__ __forceinline__
bool eval_move_parallel(const PlaceDev& p, EvalStage& st, const SwapPos& sw,
                        int32_t blk, int32_t other, int n_a, int n_b,
                        bool timing, float& dbb, float& dtd, NetCosts& ca,
                        NetCosts& cb) {
  const int lane = threadIdx.x & 63;
  const int ns = n_a + n_b;
  // this lane's slot
  int32_t n = -1;
  if (lane < n_a) n = p.blk_nets[p.blk_net_ptr[blk] + lane];
  else if (lane < ns) n = p.blk_nets[p.blk_net_ptr[other] + lane - n_a];
  // is a net of other also one of blk's? blk's slots are sorted: binary
  // search through the lanes (range of at most 64: 7 halvings)
  int lo = 0, hi = n_a;
  for (int it = 0; it < 7; ++it) {
    const int mid = (lo + hi) >> 1;
    const int32_t v = __shfl(n, mid & 63);
    if (lo < hi) { if (v < n) lo = mid + 1; else hi = mid; }
  }
  const int32_t found = __shfl(n, lo & 63);
  const bool shared = lane >= n_a && lo < n_a && found == n;
  const bool live = lane < ns && !shared;
  int32_t e0 = 0, cnt = 0, c0 = 0;
  int dx0 = 0, dy0 = 0;
  float q = 0.0f, old_bb = 0.0f, old_td = 0.0f;
  if (live) {
    e0 = p.net_blk_ptr[n];
    cnt = p.net_blk_ptr[n + 1] - e0;
    q = p.net_q[n];
    old_bb = p.net_cost[n];
    if (timing) {
      old_td = p.net_tcost[n];
      c0 = p.net_sink_ptr[n];
      const int32_t drv = p.net_blks[e0];
      dx0 = p.bx[drv]; dy0 = p.by[drv];
      sw(p, drv, dx0, dy0);
    }
  }
  // items: slot 0's members, then slot 1's, ...
  int incl = cnt;
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  const int total = __shfl(incl, 63);
  if (total > EVAL_ITEMS) return false;
  st.incl[lane] = incl; st.e0[lane] = e0; st.c0[lane] = c0;
  st.drvx[lane] = dx0; st.drvy[lane] = dy0;
  st.xmin[lane] = 1 << 28; st.xmax[lane] = -1;
  st.ymin[lane] = 1 << 28; st.ymax[lane] = -1;
  wave_lds_sync();
  for (int base = 0; base < total; base += 64) {
    const int g = base + lane;
    if (g >= total) continue;
    // the item's slot: the first whose inclusive prefix exceeds g (shared
    // and empty slots repeat their predecessor's prefix and are passed)
    int s0 = 0, s1 = ns - 1;
    for (int it = 0; it < 6; ++it) {
      const int mid = (s0 + s1) >> 1;
      const bool in_low = st.incl[mid] > g;
      if (s0 < s1) { if (in_low) s1 = mid; else s0 = mid + 1; }
    }
    const int slot = s0;
    const int mbr = g - (slot ? st.incl[slot - 1] : 0);
    // every occurrence of a block in a net is an item of its own
    const int32_t b = p.net_blks[st.e0[slot] + mbr];
    int x = p.bx[b], y = p.by[b];
    sw(p, b, x, y);
    atomicMin(&st.xmin[slot], x); atomicMax(&st.xmax[slot], x);
    atomicMin(&st.ymin[slot], y); atomicMax(&st.ymax[slot], y);
    if (timing && mbr > 0) {
      const int dx = abs(x - st.drvx[slot]), dy = abs(y - st.drvy[slot]);
      st.crit[g] = p.conn_crit[st.c0[slot] + mbr - 1];
      st.delay[g] = p.delay_mat[dx * p.gy + dy];
    }
  }
  wave_lds_sync();
  // back on the slot's lane: the net's costs and deltas, pinned roundings
  NetCosts nc{COST_NONE, 0.0f};
  float d_bb = 0.0f, d_td = 0.0f;
  if (live) {
    const float span = (float)((st.xmax[lane] - st.xmin[lane] + 1) +
                               (st.ymax[lane] - st.ymin[lane] + 1));
    nc.bb = mul_rn(q, span);
    d_bb = __builtin_fmaf(q, span, -old_bb);
    if (timing) {
      // the chain runs left to right over the sinks in CSR order
      float t = 0.0f;
      const int i0 = incl - cnt;
      for (int j = 1; j < cnt; ++j)
        t = __builtin_fmaf(st.crit[i0 + j], st.delay[i0 + j], t);
      nc.td = t;
      d_td = t - old_td;
    }
  }
  // lane k sums what the serial form gives it: slot k, then slot n_a + k
  const int sb = (n_a + lane) & 63;
  const float b_dbb = __shfl(d_bb, sb), b_dtd = __shfl(d_td, sb);
  const float b_bb = __shfl(nc.bb, sb), b_td = __shfl(nc.td, sb);
  if (lane < n_a) {
    dbb += d_bb;
    if (timing) dtd += d_td;
    ca = nc;
  }
  if (lane < n_b) {
    if (b_bb != COST_NONE) {
      dbb += b_dbb;
      if (timing) dtd += b_dtd;
    }
    cb = NetCosts{b_bb, b_td};
  }
  return true;
}

// Reduces the lanes' delta shares over the wave (dbb and dtd come back
// summed) and takes the Metropolis decision, the same in every lane.
__device__ __forceinline__
bool metropolis(const Sched& s, int i, float& dbb, float& dtd) {
  dbb = wave_sum_f32(dbb);
  dtd = wave_sum_f32(dtd);
  float delta;
  {
#pragma clang fp contract(off)
    delta = (1.0f - s.timing_tradeoff) * dbb * s.inv_bb_norm +
            s.timing_tradeoff * dtd * s.inv_td_norm;
  }
  if (delta <= 0.0f) return true;
  if (s.T <= 0.0f) return false;
  float u = (rng_hash(s.seed, s.batch, i * 131 + 5) & 0xFFFFFF) *
            (1.0f / 16777216.0f);
  return u < __expf(-delta / s.T);
}

// lane 0 records an accepted move for resolve and apply. `from` is the
// proposer's source tile: resolve must not read it from bx/by, which the
// winners of a fused commit launch are rewriting.
template <class Counters> __device__ __forceinline__
void record_move(const MovesDev& m, const Counters& cnt, int32_t* mv_from,
                 int i, int32_t blk, int32_t to, int32_t other, float dbb,
                 float dtd, int32_t from) {
  cnt.add(CNT_ACCEPTED);
  m.mv_blk[i] = blk;
  m.mv_to[i] = to;
  m.mv_other[i] = other;
  m.mv_dbb[i] = dbb;
  m.mv_dtd[i] = dtd;
  m.mv_flags[i] = 1;
  mv_from[i] = from;
}

// One WAVEFRONT per proposal (the per-thread version left ~1 live
// thread per CU and propose was 52% of LU32 kernel time at 158 us per
// 554-move batch): lane 0 selects the candidate, the wave evaluates the
// affected nets' exact deltas in parallel and reduces them, and claims
// go out lane-strided (taking a claim is idempotent, so the block lists
// need no dedup — only the delta sum skips shared nets).
template <class Claims, class Counters> __device__ __forceinline__
void propose_move(const PlaceDev& p, const MovesDev& m, const Claims& c,
                  const Counters& cnt, int32_t* mv_from, int i,
                  const Sched& s) {
  const int lane = threadIdx.x & 63;
  int sel = -1, sx1 = -1, sy1 = -1, sslot = 0;
  if (lane == 0) {
    m.mv_flags[i] = 0;
    sel = propose_select(p, s.rlim, s.seed, s.batch, i, sx1, sy1, sslot);
  }
  sel = __shfl(sel, 0);
  if (sel < 0) return;
  const int x1 = __shfl(sx1, 0);
  const int y1 = __shfl(sy1, 0);
  const int slot1 = __shfl(sslot, 0);
  const int32_t blk = sel;
  const int x0 = p.bx[blk], y0 = p.by[blk];
  const int mid = p.macro_of ? p.macro_of[blk] : -1;
  float dbb = 0.0f, dtd = 0.0f;
  if (mid >= 0) {
    // -------- macro move (reference: place_macro.c; free-target) -----
    const MacroPos ms{mid, x1 - x0, y1 - y0};
    const int32_t mm0 = p.macro_ptr[mid], mm1 = p.macro_ptr[mid + 1];
    if (mm1 - mm0 > 16) return;
    int ok = 0;
    if (lane == 0) {
      ok = macro_shift_ok(p, ms, mm0, mm1);
      if (ok) cnt.add(CNT_ATTEMPTS);
    }
    ok = __shfl(ok, 0);
    if (!ok) return;
    // a net of several members is counted at the first of them
    for_macro_nets(p, mm0, mm1, [&](int32_t j, int32_t n) {
      bool dup = false;
      for (int32_t j2 = mm0; j2 < j && !dup; ++j2)
        dup = blk_has_net(p, p.macro_blk[j2], n);
      if (!dup) add_net_delta(p, n, ms, s.timing_tradeoff, dbb, dtd);
    });
    if (!metropolis(s, i, dbb, dtd)) return;
    if (lane == 0)
      record_move(m, cnt, mv_from, i, blk,
                  ((ms.ddx + 4096) << 13) | (ms.ddy + 4096), -2 - mid, dbb,
                  dtd, x0 * p.gy + y0);
    for_macro_nets(p, mm0, mm1, [&](int32_t, int32_t n) { c.take_net(n); });
    for (int32_t j = mm0 + lane; j < mm1; j += 64) {
      int32_t b = p.macro_blk[j];
      c.take_loc(p.bx[b] * p.gy + p.by[b]);
      c.take_loc((p.bx[b] + ms.ddx) * p.gy + p.by[b] + ms.ddy);
    }
    return;
  }
  // -------- single-block move / swap (wave-uniform checks) --------
  int32_t other = p.grid[((int64_t)x1 * p.gy + y1) * p.cap + slot1];
  if (other == blk) return;
  if (other >= 0 && p.fixed && p.fixed[other]) return;
  if (other >= 0 && p.macro_of && p.macro_of[other] >= 0)
    return;   // never swap a chain member out from under its macro
  if (lane == 0) cnt.add(CNT_ATTEMPTS);  // valid proposals only
  // nets shared by both blocks are counted once (skipped in other's pass)
  const SwapPos sw{blk, x1, y1, other, other >= 0 ? x0 : -1000,
                   other >= 0 ? y0 : -1000};
  const int n_a = p.blk_net_ptr[blk + 1] - p.blk_net_ptr[blk];
  const int n_b =
      other >= 0 ? p.blk_net_ptr[other + 1] - p.blk_net_ptr[other] : 0;
  // the costs of this lane's net of blk (a) and of other (b) after the move
  NetCosts ca{COST_NONE, 0.0f}, cb{COST_NONE, 0.0f};
  // Member-parallel where the staging holds the move; else (wave-uniform)
  // the serial form, a net per lane. Both give the same bits.
  __shared__ EvalStage stage[PROP_WAVES];
  const bool timing = s.timing_tradeoff > 0.0f;
  bool evaluated = false;
  if (n_a + n_b <= EVAL_SLOTS && (!timing || p.delay_mat != nullptr))
    evaluated = eval_move_parallel(p, stage[threadIdx.x >> 6], sw, blk, other,
                                   n_a, n_b, timing, dbb, dtd, ca, cb);
  if (!evaluated) {
    for_blk_nets_k(p, blk, [&](int32_t k, int32_t n) {
      NetCosts nc = add_net_delta(p, n, sw, s.timing_tradeoff, dbb, dtd);
      if (k < 64) ca = nc;
    });
    if (other >= 0)
      for_blk_nets_k(p, other, [&](int32_t k, int32_t n) {
        if (blk_has_net(p, blk, n)) return;
        NetCosts nc = add_net_delta(p, n, sw, s.timing_tradeoff, dbb, dtd);
        if (k < 64) cb = nc;
      });
  }
  if (!metropolis(s, i, dbb, dtd)) return;
  // cost_k <= 64: a move that fits has every net in the lanes' first pass
  const bool stored = n_a + n_b <= m.cost_k;
  if (stored) {
    const int64_t s0 = (int64_t)i * m.cost_k;
    if (lane < n_a) m.mv_ncost[s0 + lane] = ca.bb;
    if (lane < n_b) m.mv_ncost[s0 + n_a + lane] = cb.bb;
    if (s.timing_tradeoff > 0.0f) {
      if (lane < n_a) m.mv_ntcost[s0 + lane] = ca.td;
      if (lane < n_b) m.mv_ntcost[s0 + n_a + lane] = cb.td;
    }
  }
  if (lane == 0) {
    record_move(m, cnt, mv_from, i, blk,
                ((x1 * p.gy + y1) * p.cap + slot1) |
                    (stored ? 0 : MV_RECOMPUTE),
                other, dbb, dtd, x0 * p.gy + y0);
    c.take_loc(x0 * p.gy + y0);
    c.take_loc(x1 * p.gy + y1);
  }
  auto take = [&](int32_t n) { c.take_net(n); };
  for_blk_nets(p, blk, take);
  if (other >= 0) for_blk_nets(p, other, take);
}

// ---- resolve and apply, of a move as propose recorded it ------------
struct Move {
  int32_t blk, other, to;
  bool recompute;   // single move whose costs propose did not store
  __device__ __forceinline__ Move(const MovesDev& m, int i)
      : blk(m.mv_blk[i]), other(m.mv_other[i]), to(m.mv_to[i]) {
    recompute = !is_macro() && (to & MV_RECOMPUTE);
    if (recompute) to &= ~MV_RECOMPUTE;
  }
  __device__ __forceinline__ bool is_macro() const { return other <= -2; }
  __device__ __forceinline__ MacroPos macro() const {
    return MacroPos{-2 - other, (to >> 13) - 4096, (to & 0x1FFF) - 4096};
  }
};

// Verdict of accepted move i: does it hold every claim it took? Written
// for the fused commit launch, where winners rewrite bx/by while other
// waves still decide (why no verdict depends on that: docs/KERNELS.md,
// placer section). So a single move's source tile comes from mv_from, and
// a macro move, which must read its members' bx/by, tests the derived
// tiles against the grid before loading their claims: a read torn by the
// winning proposal of the same chain may point off it (such a wave has
// lost already). In a resolve launch of its own bx/by are pre-batch:
// mv_from equals what they give and the bounds test never fires.
template <class Claims, class Counters> __device__ __forceinline__
bool resolve_move(const PlaceDev& p, const MovesDev& m, const Claims& c,
                  const Counters& cnt, const int32_t* mv_from, int i,
                  const Move& mv) {
  const int lane = threadIdx.x & 63;
  bool bad = false;
  if (mv.is_macro()) {
    // every member's src+dst tile and every member net
    const MacroPos ms = mv.macro();
    const int32_t mm0 = p.macro_ptr[ms.mid], mm1 = p.macro_ptr[ms.mid + 1];
    for (int32_t j = mm0 + lane; j < mm1; j += 64) {
      int32_t b = p.macro_blk[j];
      int sx = p.bx[b], sy = p.by[b];
      int tx = sx + ms.ddx, ty = sy + ms.ddy;
      if (tx < 0 || tx >= p.gx || ty < 0 || ty >= p.gy) bad = true;
      else if (!c.holds_loc(sx * p.gy + sy) ||
               !c.holds_loc(tx * p.gy + ty)) bad = true;
    }
    for_macro_nets(p, mm0, mm1, [&](int32_t, int32_t n) {
      if (!c.holds_net(n)) bad = true;
    });
  } else {
    int x1 = mv.to / p.cap / p.gy, y1 = (mv.to / p.cap) % p.gy;
    if (lane == 0 && (!c.holds_loc(mv_from[i]) ||
                      !c.holds_loc(x1 * p.gy + y1))) bad = true;
    auto lost = [&](int32_t n) { if (!c.holds_net(n)) bad = true; };
    for_blk_nets(p, mv.blk, lost);
    if (mv.other >= 0) for_blk_nets(p, mv.other, lost);
  }
  const bool win = !__any(bad);
  if (lane == 0) {
    if (!win) { m.mv_flags[i] = 0; cnt.add(CNT_CONFLICTS); }
    else { m.mv_flags[i] = 2; cnt.add(CNT_WINNERS); }
  }
  return win;
}

template <class Pos> __device__ __forceinline__
void refresh_net(const PlaceDev& p, int32_t n, const Pos& pos,
                 float timing_tradeoff) {
  p.net_cost[n] = net_bb_cost(p, n, pos);
  if (timing_tradeoff > 0.0f) p.net_tcost[n] = net_td_cost(p, n, pos);
}

// Apply winner i. The net costs come FIRST, lane-strided: a single move
// copies what propose stored; a macro move, and a single move flagged
// MV_RECOMPUTE, recompute them with the hypothetical positions over the
// PRE-move state (so lanes never read positions another lane just wrote;
// duplicate refreshes of nets shared by both blocks are idempotent). Both
// give the same words. Then lane 0 commits grid and positions. The cost
// totals are not kept up here: place_refresh_costs_kernel recomputes them
// from the cached net costs whenever the host wants them.
__device__ __forceinline__
void apply_move(const PlaceDev& p, const MovesDev& m, int i, const Move& mv,
                float timing_tradeoff) {
  const int lane = threadIdx.x & 63;
  if (mv.is_macro()) {
    const MacroPos ms = mv.macro();
    const int32_t mm0 = p.macro_ptr[ms.mid], mm1 = p.macro_ptr[ms.mid + 1];
    for_macro_nets(p, mm0, mm1, [&](int32_t, int32_t n) {
      refresh_net(p, n, ms, timing_tradeoff);
    });
    if (lane == 0) {
      for (int32_t j = mm0; j < mm1; ++j) {
        int32_t b = p.macro_blk[j];
        p.grid[((int64_t)p.bx[b] * p.gy + p.by[b]) * p.cap + p.bslot[b]] = -1;
      }
      for (int32_t j = mm0; j < mm1; ++j) {
        int32_t b = p.macro_blk[j];
        int tx = p.bx[b] + ms.ddx, ty = p.by[b] + ms.ddy;
        p.grid[((int64_t)tx * p.gy + ty) * p.cap] = b;
        p.bx[b] = tx; p.by[b] = ty; p.bslot[b] = 0;
      }
    }
  } else {
    const int32_t blk = mv.blk, other = mv.other;
    int slot1 = mv.to % p.cap;
    int x1 = mv.to / p.cap / p.gy, y1 = (mv.to / p.cap) % p.gy;
    int x0 = p.bx[blk], y0 = p.by[blk], s0 = p.bslot[blk];
    const SwapPos sw{blk, x1, y1, other, other >= 0 ? x0 : -1000,
                     other >= 0 ? y0 : -1000};
    if (mv.recompute) {
      auto refresh = [&](int32_t n) { refresh_net(p, n, sw, timing_tradeoff); };
      for_blk_nets(p, blk, refresh);
      if (other >= 0) for_blk_nets(p, other, refresh);
    } else {
      // the costs propose stored, no member walk. A net of both blocks is
      // written from blk's slot; other's slot of it holds COST_NONE.
      const int64_t s0 = (int64_t)i * m.cost_k;
      int32_t slot0 = 0;
      auto copy = [&](int32_t k, int32_t n) {
        const float bb = m.mv_ncost[s0 + slot0 + k];
        if (bb == COST_NONE) return;
        p.net_cost[n] = bb;
        if (timing_tradeoff > 0.0f)
          p.net_tcost[n] = m.mv_ntcost[s0 + slot0 + k];
      };
      for_blk_nets_k(p, blk, copy);
      slot0 = p.blk_net_ptr[blk + 1] - p.blk_net_ptr[blk];
      if (other >= 0) for_blk_nets_k(p, other, copy);
    }
    if (lane == 0) {
      p.grid[((int64_t)x0 * p.gy + y0) * p.cap + s0] = other >= 0 ? other : -1;
      p.grid[((int64_t)x1 * p.gy + y1) * p.cap + slot1] = blk;
      p.bx[blk] = x1; p.by[blk] = y1; p.bslot[blk] = slot1;
      if (other >= 0) { p.bx[other] = x0; p.by[other] = y0; p.bslot[other] = s0; }
    }
  }
}

// ---- pnr_place_batch: reset, propose, resolve, apply ---------------
// MinClaims words back to INT_MAX, before every batch
__global__ void place_reset_claims_kernel(int32_t* net_claim, int32_t nn,
                                          int32_t* loc_claim, int32_t nl) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int total = max(nn, nl);
  for (; i < total; i += gridDim.x * blockDim.x) {
    if (i < nn) net_claim[i] = 0x7FFFFFFF;
    if (i < nl) loc_claim[i] = 0x7FFFFFFF;
  }
}

__launch_bounds__(64 * PROP_WAVES, 2)
__global__ void place_propose_kernel(PlaceDev p, MovesDev m, int32_t* mv_from,
                                     Sched s) {
  const int i = move_index();
  if (i >= m.n_moves) return;
  propose_move(p, m, MinClaims{m.net_claim, m.loc_claim, i},
               DirectCounters{m.counters}, mv_from, i, s);
}

__launch_bounds__(64 * PROP_WAVES, 2)
__global__ void place_resolve_kernel(PlaceDev p, MovesDev m,
                                     const int32_t* mv_from) {
  const int i = move_index();
  if (i >= m.n_moves || m.mv_flags[i] != 1) return;
  resolve_move(p, m, MinClaims{m.net_claim, m.loc_claim, i},
               DirectCounters{m.counters}, mv_from, i, Move(m, i));
}

__launch_bounds__(64 * PROP_WAVES, 2)
__global__ void place_apply_kernel(PlaceDev p, MovesDev m,
                                   float timing_tradeoff) {
  const int i = move_index();
  if (i >= m.n_moves || m.mv_flags[i] != 2) return;
  apply_move(p, m, i, Move(m, i), timing_tradeoff);
}

// ---- pnr_place_run: propose, commit --------------------------------
// Two launches per batch, no reset, no host round trip per batch.
// Device state of a run_batches call, zeroed by the host at its start:
//   ctrl     [0] done    set by the stop rule; every kernel returns at
//                        once on it. Read first thing by every wave.
//            [1] n_exec  batches executed so far in this run_batches call
//            [2] ticket  workgroup arrival counter of a checking commit
//                        launch
//            In the host's buffer ctrl follows the totals m.counters[0..3]
//            in one 128-byte line. The counter atomics of every wave go to
//            the shards and not to this line; the only atomics it still
//            takes are the tickets, one per workgroup at the end of every
//            fourth commit launch. A line of its own for the ticket was
//            measured and changed nothing (docs/MEASUREMENTS.md).
//   shards   n_shards lines of counters (see ShardCounters)
struct RunDev {
  int32_t* mv_from;                  // proposer's source tile x*gy+y
  unsigned long long* net_claim;     // [num_nets] EpochClaims words
  unsigned long long* loc_claim;     // [gx*gy]
  int32_t* ctrl;
  int32_t* shards;                   // [n_shards * SHARD_WORDS]
  int32_t n_shards;                  // a power of two
};

__launch_bounds__(64 * PROP_WAVES, 2)
__global__ void place_propose_run_kernel(PlaceDev p, MovesDev m, RunDev r,
                                         Sched s) {
  if (r.ctrl[0]) return;
  const int i = move_index();
  if (i >= m.n_moves) return;
  const EpochClaims c{r.net_claim, r.loc_claim, claim_key(s.batch, i)};
  propose_move(p, m, c, ShardCounters(r.shards, r.n_shards - 1), r.mv_from, i,
               s);
}

// Resolve and apply of one move by its wave: a winner applies at once,
// while other waves are still deciding (see resolve_move).
__device__ __forceinline__
void commit_move(const PlaceDev& p, const MovesDev& m, const RunDev& r,
                 float timing_tradeoff, uint32_t batch) {
  const int i = move_index();
  if (i >= m.n_moves || m.mv_flags[i] != 1) return;
  const Move mv(m, i);
  const EpochClaims c{r.net_claim, r.loc_claim, claim_key(batch, i)};
  if (resolve_move(p, m, c, ShardCounters(r.shards, r.n_shards - 1),
                   r.mv_from, i, mv))
    apply_move(p, m, i, mv, timing_tradeoff);
}

__device__ __forceinline__ int wave_sum_i32(int v) {
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// check != 0 on the 4th, 8th, ... batch of a run_batches call: the first
// wave of the last workgroup to arrive (ticket == gridDim.x - 1) folds the
// counter shards into m.counters and evaluates the stop rule on the totals.
// Nothing waits: every workgroup adds its ticket and leaves.
__launch_bounds__(64 * PROP_WAVES, 2)
__global__ void place_commit_kernel(PlaceDev p, MovesDev m, RunDev r,
                                    float timing_tradeoff, uint32_t batch,
                                    int check, int32_t target_moves) {
  if (r.ctrl[0]) return;
  commit_move(p, m, r, timing_tradeoff, batch);
  if (!check) return;
  // this wave's counter atomics have been performed ...
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  // ... and are ordered before the ticket
  __threadfence();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int ticket = 0;
  if (lane == 0)
    ticket = __hip_atomic_fetch_add(&r.ctrl[2], 1, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
  if (__shfl(ticket, 0) != (int)gridDim.x - 1) return;
  __threadfence();
  // The fold may trust the shards. Every workgroup of this launch performed
  // its commit-side adds before it took its ticket (waitcnt, barrier,
  // fence, ticket, above), and this wave holds the last ticket; the adds of
  // this batch's propose launch, and of every earlier batch, were complete
  // at a kernel boundary. Launches that returned on `done` added nothing.
  // The loads are agent-scope atomics, so they are served by L2, where the
  // adds were performed, and not by a stale line of this CU's L1.
  int tot[4] = {0, 0, 0, 0};
  for (int sh = lane; sh < r.n_shards; sh += 64)
    for (int k = 0; k < 4; ++k)
      tot[k] += __hip_atomic_load(&r.shards[(int64_t)sh * SHARD_WORDS + k],
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int k = 0; k < 4; ++k) tot[k] = wave_sum_i32(tot[k]);
  if (lane != 0) return;
  for (int k = 0; k < 4; ++k) m.counters[k] = tot[k];
  r.ctrl[1] += 4;
  if (tot[CNT_WINNERS] + (tot[CNT_ATTEMPTS] - tot[CNT_ACCEPTED]) >=
      target_moves)
    r.ctrl[0] = 1;
  __hip_atomic_store(&r.ctrl[2], 0, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// full net-cost refresh (init + periodic drift resync).
// Host must zero out[0..1] before the launch.
__global__ void place_refresh_costs_kernel(PlaceDev p, float timing_tradeoff,
                                           double* out /*[2]*/) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  for (; n < p.num_nets; n += gridDim.x * blockDim.x) {
    const SwapPos as_is{-1, 0, 0, -1, 0, 0};
    float c = net_bb_cost(p, n, as_is);
    p.net_cost[n] = c;
    unsafeAtomicAdd(&out[0], (double)c);
    float t = timing_tradeoff > 0.0f ? net_td_cost(p, n, as_is) : 0.0f;
    p.net_tcost[n] = t;
    unsafeAtomicAdd(&out[1], (double)t);
  }
}

}  // namespace pnrh

using namespace pnrh;

extern "C" {

struct PlaceLaunchArgs {
  const int32_t* net_blk_ptr; const int32_t* net_blks;
  const int32_t* blk_net_ptr; const int32_t* blk_nets;
  const int8_t* blk_type; const int8_t* tile_btype;
  const int32_t* type_cols; const int32_t* type_col_ptr;
  const uint8_t* fixed;
  const float* net_q;
  const int32_t* net_sink_ptr; const float* conn_crit; const float* delay_mat;
  int32_t* bx; int32_t* by; int32_t* bslot; int32_t* grid;
  float* net_cost; float* net_tcost;
  int32_t num_blocks, num_nets, gx, gy, cap, nx, ny, io_cap;
  int32_t rx0, rx1;
  const int32_t* macro_of; const int32_t* macro_ptr;
  const int32_t* macro_blk;
  // moves
  int32_t* mv_blk; int32_t* mv_to; int32_t* mv_other;
  float* mv_dbb; float* mv_dtd; uint8_t* mv_flags;
  int32_t* net_claim; int32_t* loc_claim; int32_t* counters;
  int32_t n_moves;
  // schedule
  float T; int32_t rlim; float timing_tradeoff;
  float inv_bb_norm, inv_td_norm;
  uint32_t seed, batch;
  double* cost_acc;
  // pnr_place_run only (see RunDev); net_claim/loc_claim above are the
  // int32 words of pnr_place_batch
  int32_t* mv_from;
  unsigned long long* net_claim64; unsigned long long* loc_claim64;
  int32_t* run_ctrl;
  // the counter shards, n_shards lines of 128 bytes (see RunDev),
  // 128-byte aligned
  int32_t* run_shards;
  int32_t n_shards;
  // stored costs of accepted moves (see MovesDev)
  float* mv_ncost; float* mv_ntcost;
  int32_t cost_k;
};

static void unpack(const PlaceLaunchArgs* a, PlaceDev& p, MovesDev& m) {
  p.net_blk_ptr = a->net_blk_ptr; p.net_blks = a->net_blks;
  p.blk_net_ptr = a->blk_net_ptr; p.blk_nets = a->blk_nets;
  p.blk_type = a->blk_type; p.tile_btype = a->tile_btype;
  p.type_cols = a->type_cols; p.type_col_ptr = a->type_col_ptr;
  p.fixed = a->fixed;
  p.net_q = a->net_q;
  p.net_sink_ptr = a->net_sink_ptr; p.conn_crit = a->conn_crit;
  p.delay_mat = a->delay_mat;
  p.bx = a->bx; p.by = a->by; p.bslot = a->bslot; p.grid = a->grid;
  p.net_cost = a->net_cost; p.net_tcost = a->net_tcost;
  p.num_blocks = a->num_blocks; p.num_nets = a->num_nets;
  p.gx = a->gx; p.gy = a->gy; p.cap = a->cap;
  p.nx = a->nx; p.ny = a->ny; p.io_cap = a->io_cap;
  p.rx0 = a->rx0; p.rx1 = a->rx1;
  p.macro_of = a->macro_of; p.macro_ptr = a->macro_ptr;
  p.macro_blk = a->macro_blk;
  m.mv_blk = a->mv_blk; m.mv_to = a->mv_to; m.mv_other = a->mv_other;
  m.mv_dbb = a->mv_dbb; m.mv_dtd = a->mv_dtd; m.mv_flags = a->mv_flags;
  m.net_claim = a->net_claim; m.loc_claim = a->loc_claim;
  m.counters = a->counters; m.n_moves = a->n_moves;
  m.mv_ncost = a->mv_ncost; m.mv_ntcost = a->mv_ntcost;
  m.cost_k = a->cost_k;
}

// what both batch drivers need besides their claim words
static bool batch_args_ok(const PlaceLaunchArgs* a) {
  return a->mv_from && a->mv_ncost && a->mv_ntcost && a->cost_k >= 1 &&
         a->cost_k <= 64 &&
         (int64_t)a->gx * a->gy * a->cap < (int64_t)MV_RECOMPUTE;
}

static Sched sched(const PlaceLaunchArgs* a, uint32_t batch) {
  return Sched{a->T, a->rlim, a->timing_tradeoff, a->inv_bb_norm,
               a->inv_td_norm, a->seed, batch};
}

int pnr_place_batch(const PlaceLaunchArgs* a, void* stream) {
  if (!batch_args_ok(a) || !a->net_claim || !a->loc_claim)
    return (int)hipErrorInvalidValue;
  PlaceDev p; MovesDev m;
  unpack(a, p, m);
  hipStream_t s = (hipStream_t)stream;
  int rg = (max(max(a->num_nets, a->gx * a->gy), a->n_moves) + 255) / 256;
  rg = rg < 2048 ? rg : 2048;
  hipLaunchKernelGGL(place_reset_claims_kernel, dim3(rg), dim3(256), 0, s,
                     m.net_claim, p.num_nets, m.loc_claim, p.gx * p.gy);
  int mg = (m.n_moves + PROP_WAVES - 1) / PROP_WAVES;
  hipLaunchKernelGGL(place_propose_kernel, dim3(mg), dim3(64 * PROP_WAVES),
                     0, s, p, m, a->mv_from, sched(a, a->batch));
  hipLaunchKernelGGL(place_resolve_kernel, dim3(mg), dim3(64 * PROP_WAVES),
                     0, s, p, m, (const int32_t*)a->mv_from);
  hipLaunchKernelGGL(place_apply_kernel, dim3(mg), dim3(64 * PROP_WAVES),
                     0, s, p, m, a->timing_tradeoff);
  return (int)hipGetLastError();
}

// Enqueue n_batches batches (numbers first_batch, first_batch + 1, ...)
// back to back, two launches each, with no host synchronisation. The
// stop rule of GpuPlacer.run_batches runs on the device after every 4th
// batch; once it fires the remaining launches return at once. n_batches
// must be a multiple of 4 so that the 4th, 8th, ... batch of the
// run_batches call is also the 4th, 8th, ... of each chunk.
int pnr_place_run(const PlaceLaunchArgs* a, uint32_t first_batch,
                  int32_t target_moves, int32_t n_batches, void* stream) {
  if (n_batches < 0 || (n_batches & 3) || first_batch == 0 ||
      !batch_args_ok(a) || !a->net_claim64 || !a->loc_claim64 ||
      !a->run_ctrl || !a->run_shards || a->n_shards < 1 ||
      (a->n_shards & (a->n_shards - 1)) || ((uintptr_t)a->run_shards & 127))
    return (int)hipErrorInvalidValue;
  PlaceDev p; MovesDev m;
  unpack(a, p, m);
  RunDev r;
  r.mv_from = a->mv_from;
  r.net_claim = a->net_claim64; r.loc_claim = a->loc_claim64;
  r.ctrl = a->run_ctrl;
  r.shards = a->run_shards;
  r.n_shards = a->n_shards;
  hipStream_t s = (hipStream_t)stream;
  int mg = (m.n_moves + PROP_WAVES - 1) / PROP_WAVES;
  for (int32_t k = 0; k < n_batches; ++k) {
    const uint32_t batch = first_batch + (uint32_t)k;
    hipLaunchKernelGGL(place_propose_run_kernel, dim3(mg),
                       dim3(64 * PROP_WAVES), 0, s, p, m, r, sched(a, batch));
    hipLaunchKernelGGL(place_commit_kernel, dim3(mg), dim3(64 * PROP_WAVES),
                       0, s, p, m, r, a->timing_tradeoff, batch,
                       (int)(((k + 1) & 3) == 0), target_moves);
  }
  return (int)hipGetLastError();
}

int pnr_place_refresh(const PlaceLaunchArgs* a, void* stream) {
  PlaceDev p; MovesDev m;
  unpack(a, p, m);
  hipStream_t s = (hipStream_t)stream;
  // the caller has zeroed cost_acc; grid-stride accumulate
  hipLaunchKernelGGL(place_refresh_costs_kernel, dim3(1024), dim3(256), 0, s,
                     p, a->timing_tradeoff, a->cost_acc);
  return (int)hipGetLastError();
}

int64_t pnr_place_args_sizeof() { return (int64_t)sizeof(PlaceLaunchArgs); }

}  // extern "C"
