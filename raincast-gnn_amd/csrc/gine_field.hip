// Member fields scored per graph: the energy score over a graph's stations, the
// variogram score over its station pairs and the ensemble scores of an area aggregate, of
// members [N, M] (M <= 64) against targets y [N], the rows of graph g being ptr[g]..ptr[g+1]-1.
//
// A member value is x = shift + scale * raw in fp64 (two roundings, -ffp-contract=off), raw an
// fp32 or fp64 element read in place through (row_stride, member_stride).  Per graph:
//   S_g = rows with a non-NaN target and at least one non-NaN member,
//   V_g = members non-NaN at every row of S_g, kept as a 64-bit mask: the AND over the rows of
//         S_g of the ballot of non-NaN lanes, lane = member (all M members for an empty S_g).
//
// Work is cut into row tiles of kTile rows that never span two graphs.  Tile k of graph g has
// the slot  ptr[g] / kTile + g + k:  ceil(n / kTile) <= (p + n) / kTile - p / kTile + 1, so the
// slots of consecutive graphs never overlap and  N / kTile + G  slots hold every tile; a
// workgroup finds its graph by bisection over ptr, on the device (no host synchronisation).
// Every tile kernel writes its partial sums to its own slot and a finishing kernel adds a
// graph's slots in ascending order: fp64, a fixed order, no atomics, the same bits every run.
#include "gine_common.hpp"

namespace gine {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTile = GINE_FIELD_ROW_TILE;  // rows of a tile (a-rows of the variogram score)
constexpr int kSub = 32;                    // b-rows staged at a time by the variogram score
constexpr int kVsSplit = 4;                 // workgroups that share one a-tile's b-rows
constexpr int kMaxMembers = 64;
constexpr int kPairSlots = (kMaxMembers * (kMaxMembers + 1) / 2 + kThreads - 1) / kThreads;
constexpr int kAreaThreads = 1024;
constexpr int kAreaWaves = kAreaThreads / kWave;
static_assert(kTile == 64 && kSub * 2 == kTile, "the thread-to-pair maps below assume 64 x 32");

struct Members {
  const void* p;
  int64_t row_stride, member_stride;
  double scale, shift;
  int f64, M;
};

__device__ __forceinline__ double member_at(const Members& mb, int64_t row, int i) {
  const int64_t off = row * mb.row_stride + (int64_t)i * mb.member_stride;
  const double raw = mb.f64 ? static_cast<const double*>(mb.p)[off]
                            : (double)static_cast<const float*>(mb.p)[off];
  return mb.shift + mb.scale * raw;
}

__device__ __forceinline__ uint64_t member_bits(int M) {
  return M >= 64 ? ~0ull : ((1ull << M) - 1ull);
}

__device__ __forceinline__ int64_t clamp_row(int64_t v, int64_t n) {
  return v < 0 ? 0 : (v > n ? n : v);
}

// rows [p0, p1) of graph g, inside [0, N] whatever ptr holds
__device__ __forceinline__ void graph_rows(const int64_t* __restrict__ ptr, int64_t g, int64_t N,
                                           int64_t& p0, int64_t& p1) {
  p0 = clamp_row(ptr[g], N);
  p1 = clamp_row(ptr[g + 1], N);
  if (p1 < p0) p1 = p0;
}

__device__ __forceinline__ int64_t first_slot(const int64_t* __restrict__ ptr, int64_t g,
                                              int64_t N) {
  return clamp_row(ptr[g], N) / kTile + g;
}

struct Tile {
  int64_t g, first, tiles, k, row0;
  int rows;
};

// the tile of slot `slot`; false for a slot no graph uses
__device__ __forceinline__ bool locate(const int64_t* __restrict__ ptr, int64_t G, int64_t N,
                                       int64_t slot, Tile& t) {
  int64_t lo = 0, hi = G;  // number of graphs whose first slot is <= slot
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (first_slot(ptr, mid, N) <= slot) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return false;
  t.g = lo - 1;
  int64_t p0, p1;
  graph_rows(ptr, t.g, N, p0, p1);
  t.first = p0 / kTile + t.g;
  t.tiles = ceil_div(p1 - p0, kTile);
  t.k = slot - t.first;
  if (t.k >= t.tiles) return false;
  t.row0 = p0 + t.k * kTile;
  const int64_t left = p1 - t.row0;
  t.rows = left < kTile ? (int)left : kTile;
  return true;
}

__device__ __forceinline__ double as_double(uint64_t v) { return __longlong_as_double((long long)v); }
__device__ __forceinline__ uint64_t as_bits(double v) { return (uint64_t)__double_as_longlong(v); }

// sum over the workgroup in a fixed tree; s holds blockDim.x doubles; every thread gets it
__device__ __forceinline__ double block_sum(double v, double* s) {
  __syncthreads();
  s[threadIdx.x] = v;
  __syncthreads();
  for (int off = blockDim.x / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  return s[0];
}

// lane j's value in every lane; j is wave-uniform
__device__ __forceinline__ double lane_value(double v, int j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = kWave / 2; off > 0; off >>= 1) v += shfl_xor_d(v, off);
  return v;
}

// One row with lane = member: its member (NaN for lane >= M), whether it is in S_g, and the
// ballot of its non-NaN members.
struct Row {
  double x;
  float y;
  uint64_t have;
  bool in_s;
};

__device__ __forceinline__ Row load_row(const Members& mb, const float* __restrict__ y,
                                        int64_t row, int lane) {
  Row r;
  r.x = __builtin_nan("");
  if (lane < mb.M) r.x = member_at(mb, row, lane);
  r.y = y[row];
  r.have = __ballot(r.x == r.x);
  r.in_s = r.y == r.y && r.have != 0ull;
  return r;
}

// the waves' masks and row counts combined: s_mask / s_rows hold one entry per wave
__device__ __forceinline__ void combine_waves(uint64_t& mask, int& rows, uint64_t* s_mask,
                                              int* s_rows, int waves) {
  const int wave = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_mask[wave] = mask;
    s_rows[wave] = rows;
  }
  __syncthreads();
  mask = ~0ull;
  rows = 0;
  for (int w = 0; w < waves; ++w) {
    mask &= s_mask[w];
    rows += s_rows[w];
  }
}

// V_g and |S_g| from the tile words of a graph: mask_words / row_words are indexed by slot
__device__ __forceinline__ void graph_validity(const double* __restrict__ mask_words,
                                               const double* __restrict__ row_words,
                                               int64_t stride, int64_t first, int64_t tiles,
                                               uint64_t& mask, int64_t& rows) {
  mask = ~0ull;
  rows = 0;
  for (int64_t k = 0; k < tiles; ++k) {
    mask &= as_bits(mask_words[(first + k) * stride]);
    rows += (int64_t)as_bits(row_words[(first + k) * stride]);
  }
}

// pair p of the lower triangle with its diagonal: p = i (i + 1) / 2 + j, j <= i
__device__ __forceinline__ void pair_of(int p, int& i, int& j) {
  int r = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
  while (r * (r + 1) / 2 > p) --r;
  while ((r + 1) * (r + 2) / 2 <= p) ++r;
  i = r;
  j = p - r * (r + 1) / 2;
}

// ---------------------------------------------------------------------------------------
// Energy score, stage 1: one workgroup per tile.  The tile is staged as [rows][M + 1] fp64 in
// LDS (column M = the target; a row outside S_g and a missing member are staged as 0, so they
// add nothing and produce no NaN).  Thread t owns the pairs p = t, t + 256, ... of (i, j < i)
// and (i, target) and adds their squared differences over the tile's rows.  Out, per slot:
// P = M (M + 1) / 2 sums, the tile's member mask and its number of rows in S_g.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_field_energy_tiles(
    Members mb, const float* __restrict__ y, const int64_t* __restrict__ ptr, int64_t G,
    int64_t N, double* __restrict__ partials) {
  __shared__ double tile[kTile * (kMaxMembers + 1)];
  __shared__ uint64_t s_mask[kWaves];
  __shared__ int s_rows[kWaves];
  Tile t;
  if (!locate(ptr, G, N, blockIdx.x, t)) return;
  const int M = mb.M, S = M + 1, P = M * (M + 1) / 2;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  uint64_t mask = ~0ull;
  int rows = 0;
  for (int r = wave; r < t.rows; r += kWaves) {
    const Row row = load_row(mb, y, t.row0 + r, lane);
    if (row.in_s) {
      mask &= row.have;
      ++rows;
    }
    if (lane < M) tile[r * S + lane] = (row.in_s && row.x == row.x) ? row.x : 0.0;
    if (lane == 0) tile[r * S + M] = row.in_s ? (double)row.y : 0.0;
  }
  combine_waves(mask, rows, s_mask, s_rows, kWaves);  // also orders the tile's writes
  int ci[kPairSlots], cj[kPairSlots];
  double acc[kPairSlots];
#pragma unroll
  for (int q = 0; q < kPairSlots; ++q) {
    const int p = threadIdx.x + q * kThreads;
    ci[q] = cj[q] = 0;
    acc[q] = 0.0;
    if (p < P) {
      pair_of(p, ci[q], cj[q]);
      if (cj[q] == ci[q]) cj[q] = M;  // the diagonal stands for (i, target)
    }
  }
  for (int r = 0; r < t.rows; ++r) {
    const double* line = tile + r * S;
#pragma unroll
    for (int q = 0; q < kPairSlots; ++q) {
      const double d = line[ci[q]] - line[cj[q]];
      acc[q] += d * d;
    }
  }
  double* out = partials + (int64_t)blockIdx.x * (P + 2);
#pragma unroll
  for (int q = 0; q < kPairSlots; ++q) {
    const int p = threadIdx.x + q * kThreads;
    if (p < P) out[p] = acc[q];
  }
  if (threadIdx.x == 0) {
    out[P] = as_double(mask);
    out[P + 1] = as_double((uint64_t)rows);
  }
}

// Energy score, stage 2: one workgroup per graph adds each pair's tile sums in tile order,
// takes the root, and sums the norms of the pairs inside V_g in a fixed tree.
__global__ __launch_bounds__(kThreads) void k_field_energy_finish(
    const double* __restrict__ partials, const int64_t* __restrict__ ptr, int64_t N, int M,
    double* __restrict__ es, double* __restrict__ es_fair, double* __restrict__ members_valid,
    double* __restrict__ rows_valid) {
  __shared__ double s_red[kThreads];
  const int64_t g = blockIdx.x;
  const int P = M * (M + 1) / 2;
  const int64_t stride = P + 2;
  int64_t p0, p1;
  graph_rows(ptr, g, N, p0, p1);
  const int64_t first = p0 / kTile + g, tiles = ceil_div(p1 - p0, kTile);
  uint64_t mask;
  int64_t rows;
  graph_validity(partials + P, partials + P + 1, stride, first, tiles, mask, rows);
  mask &= member_bits(M);
  double to_obs = 0.0, between = 0.0;
  for (int p = threadIdx.x; p < P; p += kThreads) {
    double s = 0.0;
    for (int64_t k = 0; k < tiles; ++k) s += partials[(first + k) * stride + p];
    int i, j;
    pair_of(p, i, j);
    const bool vi = (mask >> i) & 1ull, vj = (mask >> j) & 1ull;
    if (i == j) {
      if (vi) to_obs += sqrt(s);
    } else if (vi && vj) {
      between += sqrt(s);
    }
  }
  to_obs = block_sum(to_obs, s_red);
  between = block_sum(between, s_red);  // each unordered pair once: sum_ij = 2 * between
  if (threadIdx.x != 0) return;
  const double m = (double)__popcll(mask), nan = __builtin_nan("");
  const bool ok = rows > 0 && m > 0.0;
  if (es) es[g] = ok ? to_obs / m - between / (m * m) : nan;
  if (es_fair) es_fair[g] = (ok && m > 1.0) ? to_obs / m - between / (m * (m - 1.0)) : nan;
  if (members_valid) members_valid[g] = m;
  if (rows_valid) rows_valid[g] = (double)rows;
}

// ---------------------------------------------------------------------------------------
// Variogram score.  A validity pass writes every tile's member mask and S_g row count; then a
// workgroup takes one a-tile (64 rows, staged member-major [M][64]) and walks the graph's
// b-rows from that tile on in pieces of 32 ([M][32]), every kVsSplit-th piece (blockIdx.y picks
// which).  Thread t owns a-rows 2 (t / 8) + {0, 1} and b-rows 4 (t % 8) + {0..3} of a piece and
// loops over the members of V_g: 8 sums in registers, no cross-lane step.  Only a < b counts.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_field_tile_validity(
    Members mb, const float* __restrict__ y, const int64_t* __restrict__ ptr, int64_t G,
    int64_t N, double* __restrict__ mask_words, double* __restrict__ row_words) {
  __shared__ uint64_t s_mask[kWaves];
  __shared__ int s_rows[kWaves];
  Tile t;
  if (!locate(ptr, G, N, blockIdx.x, t)) return;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  uint64_t mask = ~0ull;
  int rows = 0;
  for (int r = wave; r < t.rows; r += kWaves) {
    const Row row = load_row(mb, y, t.row0 + r, lane);
    if (row.in_s) {
      mask &= row.have;
      ++rows;
    }
  }
  combine_waves(mask, rows, s_mask, s_rows, kWaves);
  if (threadIdx.x == 0) {
    mask_words[blockIdx.x] = as_double(mask);
    row_words[blockIdx.x] = as_double((uint64_t)rows);
  }
}

template <int PK>  // 0: p = 0.5, 1: p = 1, 2: p = 2, 3: any other p
__device__ __forceinline__ double power_of(double d, double p) {
  if constexpr (PK == 0) return sqrt(d);
  if constexpr (PK == 1) return d;
  if constexpr (PK == 2) return d * d;
  return pow(d, p);
}

// rows [row0, row0 + rows) member-major into x [M][W] and their targets into yv [W] (NaN for a
// row outside S_g, which is how the pair loop knows it); missing members are staged as 0
template <int W>
__device__ __forceinline__ void stage_rows(const Members& mb, const float* __restrict__ y,
                                           int64_t row0, int rows, double* x, double* yv) {
  const int M = mb.M;
  for (int r = threadIdx.x; r < W; r += kThreads) yv[r] = __builtin_nan("");
  __syncthreads();
  for (int e = threadIdx.x; e < rows * M; e += kThreads) {
    const int r = e / M, i = e - r * M;
    const double v = member_at(mb, row0 + r, i);
    const bool have = v == v;
    x[i * W + r] = have ? v : 0.0;
    const float yr = y[row0 + r];
    if (have && yr == yr) yv[r] = (double)yr;  // the same value from every writer of row r
  }
  for (int e = threadIdx.x + rows * M; e < W * M; e += kThreads) {  // rows past the end
    const int r = rows + (e - rows * M) / M, i = (e - rows * M) % M;
    x[i * W + r] = 0.0;
  }
}

template <int PK>
__global__ __launch_bounds__(kThreads) void k_field_variogram_tiles(
    Members mb, const float* __restrict__ y, const int64_t* __restrict__ ptr, int64_t G,
    int64_t N, double p, const double* __restrict__ mask_words,
    const double* __restrict__ row_words, double* __restrict__ partials) {
  __shared__ double xa[kMaxMembers * kTile];
  __shared__ double xb[kMaxMembers * kSub];
  __shared__ double ya[kTile];
  __shared__ double yb[kSub];
  Tile t;
  if (!locate(ptr, G, N, blockIdx.x, t)) return;
  double* out = partials + (int64_t)blockIdx.x * kVsSplit + blockIdx.y;
  uint64_t mask;
  int64_t rows_in_s;
  graph_validity(mask_words, row_words, 1, t.first, t.tiles, mask, rows_in_s);
  mask &= member_bits(mb.M);
  const int m = __popcll(mask);
  int64_t p0, p1;
  graph_rows(ptr, t.g, N, p0, p1);
  // pieces of b-rows: piece s covers rows p0 + 32 s ...; this a-tile starts at piece 2 k
  const int64_t pieces = ceil_div(p1 - p0, kSub);
  if (m == 0 || rows_in_s < 2 || 2 * t.k + blockIdx.y >= pieces) {  // uniform
    if (threadIdx.x == 0) *out = 0.0;
    return;
  }
  stage_rows<kTile>(mb, y, t.row0, t.rows, xa, ya);
  const int ar = 2 * (threadIdx.x / 8), br = 4 * (threadIdx.x % 8);
  const double dm = (double)m;
  double acc = 0.0;
  for (int64_t s = 2 * t.k + blockIdx.y; s < pieces; s += kVsSplit) {
    const int64_t b0 = p0 + s * kSub;
    const int64_t left = p1 - b0;
    __syncthreads();  // the previous piece has been read
    stage_rows<kSub>(mb, y, b0, left < kSub ? (int)left : kSub, xb, yb);
    __syncthreads();
    double sum[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (uint64_t todo = mask; todo != 0ull; todo &= todo - 1ull) {  // members of V_g, ascending
      const int i = __builtin_ctzll(todo);
      const double* pa = xa + i * kTile + ar;
      const double* pb = xb + i * kSub + br;
      const double a0 = pa[0], a1 = pa[1];
      const double b[4] = {pb[0], pb[1], pb[2], pb[3]};
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        sum[0][v] += power_of<PK>(fabs(a0 - b[v]), p);
        sum[1][v] += power_of<PK>(fabs(a1 - b[v]), p);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const double yu = ya[ar + u];
      const int64_t a_row = t.row0 + ar + u;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const double yv = yb[br + v];
        const bool count = yu == yu && yv == yv && a_row < b0 + br + v;
        const double term = power_of<PK>(fabs(yu - yv), p) - sum[u][v] / dm;
        acc += count ? term * term : 0.0;
      }
    }
  }
  acc = block_sum(acc, xa);  // xa is free after the barrier inside
  if (threadIdx.x == 0) *out = acc;
}

// one thread per graph adds the partial sums of its slots in ascending order
__global__ __launch_bounds__(kWave) void k_field_variogram_finish(
    const double* __restrict__ mask_words, const double* __restrict__ row_words,
    const double* __restrict__ partials, const int64_t* __restrict__ ptr, int64_t G, int64_t N,
    int M, double* __restrict__ vs, double* __restrict__ pairs,
    double* __restrict__ members_valid, double* __restrict__ rows_valid) {
  const int64_t g = blockIdx.x * (int64_t)kWave + threadIdx.x;
  if (g >= G) return;
  int64_t p0, p1;
  graph_rows(ptr, g, N, p0, p1);
  const int64_t first = p0 / kTile + g, tiles = ceil_div(p1 - p0, kTile);
  uint64_t mask;
  int64_t rows;
  graph_validity(mask_words, row_words, 1, first, tiles, mask, rows);
  mask &= member_bits(M);
  const int m = __popcll(mask);
  double s = 0.0;
  if (m > 0 && rows > 1)
    for (int64_t k = 0; k < tiles * kVsSplit; ++k) s += partials[first * kVsSplit + k];
  const bool ok = rows > 0 && m > 0;
  if (vs) vs[g] = ok ? s : __builtin_nan("");
  if (pairs) pairs[g] = (double)rows * (double)(rows - 1) / 2.0;  // exact below 2^53
  if (members_valid) members_valid[g] = (double)m;
  if (rows_valid) rows_valid[g] = (double)rows;
}

// ---------------------------------------------------------------------------------------
// Area aggregates: one workgroup of 16 waves per graph, lane = member.  Wave w walks the rows
// w, w + 16, ... and keeps the max, or the sum, of mm(x) = max(exp(x) - 0.01, 0) per member and
// of the target; wave 0 combines the 16 waves in wave order and scores the M aggregates: the
// scalar ensemble scores of DESIGN.md 6e, the pair term summed directly as sum_ij |A_i - A_j|
// (area means of many stations lie close together, where the rank form would cancel).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double to_mm(double x) { return fmax(exp(x) - 0.01, 0.0); }

template <bool MEAN>
__global__ __launch_bounds__(kAreaThreads) void k_field_area(
    Members mb, const float* __restrict__ y, const int64_t* __restrict__ ptr, int64_t N,
    double* __restrict__ members_out, double* __restrict__ obs_out, double* __restrict__ crps,
    double* __restrict__ crps_fair, double* __restrict__ rank_lo, double* __restrict__ rank_hi,
    double* __restrict__ members_valid, double* __restrict__ rows_valid) {
  __shared__ double s_agg[kAreaWaves][kWave];
  __shared__ double s_obs[kAreaWaves];
  __shared__ uint64_t s_mask[kAreaWaves];
  __shared__ int s_rows[kAreaWaves];
  const int64_t g = blockIdx.x;
  const int M = mb.M;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int64_t p0, p1;
  graph_rows(ptr, g, N, p0, p1);
  uint64_t mask = ~0ull;
  int rows = 0;
  double agg = 0.0, obs = 0.0;  // mm values are >= 0
  for (int64_t row = p0 + wave; row < p1; row += kAreaWaves) {
    const Row r = load_row(mb, y, row, lane);
    if (!r.in_s) continue;  // the whole wave
    mask &= r.have;
    ++rows;
    const double v = to_mm(r.x == r.x ? r.x : 0.0);  // a missing member's lane is masked below
    const double o = to_mm((double)r.y);
    if (MEAN) {
      agg += v;
      obs += o;
    } else {
      agg = fmax(agg, v);
      obs = fmax(obs, o);
    }
  }
  s_agg[wave][lane] = agg;
  if (lane == 0) s_obs[wave] = obs;
  combine_waves(mask, rows, s_mask, s_rows, kAreaWaves);
  if (wave != 0) return;
  agg = s_agg[0][lane];
  obs = s_obs[0];
  for (int w = 1; w < kAreaWaves; ++w) {
    agg = MEAN ? agg + s_agg[w][lane] : fmax(agg, s_agg[w][lane]);
    obs = MEAN ? obs + s_obs[w] : fmax(obs, s_obs[w]);
  }
  if (MEAN) {
    agg /= (double)rows;
    obs /= (double)rows;
  }
  mask &= member_bits(M);
  const int m = __popcll(mask);
  const double nan = __builtin_nan(""), dm = (double)m;
  const bool graph_ok = rows > 0 && m > 0;
  const bool ok = graph_ok && ((mask >> lane) & 1ull);
  const double a = ok ? agg : nan;
  if (!graph_ok) obs = nan;
  double cr = nan, cf = nan, lo = nan, hi = nan;
  if (graph_ok) {  // wave-uniform
    const double to_obs = wave_sum(ok ? fabs(a - obs) : 0.0);
    double mine = 0.0;
    for (int j = 0; j < M; ++j) {
      const double aj = lane_value(a, j);
      if (ok && aj == aj) mine += fabs(a - aj);
    }
    const double between = wave_sum(mine);  // sum_i sum_j |A_i - A_j|
    cr = to_obs / dm - between / (2.0 * dm * dm);
    if (m > 1) cf = to_obs / dm - between / (2.0 * dm * (dm - 1.0));
    lo = (double)__popcll(__ballot(a < obs));
    hi = (double)__popcll(__ballot(a <= obs));
  }
  if (members_out && lane < M) members_out[g * M + lane] = a;
  if (lane != 0) return;
  if (obs_out) obs_out[g] = obs;
  if (crps) crps[g] = cr;
  if (crps_fair) crps_fair[g] = cf;
  if (rank_lo) rank_lo[g] = lo;
  if (rank_hi) rank_hi[g] = hi;
  if (members_valid) members_valid[g] = dm;
  if (rows_valid) rows_valid[g] = (double)rows;
}

// sizes, strides and flags, before any HIP call
int check_args(int32_t dtype, int64_t row_stride, int64_t member_stride, int32_t num_members,
               int64_t num_rows, int64_t num_graphs) {
  if (dtype != GINE_FIELD_F32 && dtype != GINE_FIELD_F64) return GINE_ERR_INVALID;
  if (num_members < 1 || num_members > kMaxMembers) return GINE_ERR_INVALID;
  if (num_rows < 0 || num_graphs < 0 || row_stride < 0 || member_stride < 0)
    return GINE_ERR_INVALID;
  if (num_rows / kTile + num_graphs > 0x7fffffff / kVsSplit) return GINE_ERR_TOO_LARGE;
  return GINE_OK;
}

int64_t num_slots(int64_t num_rows, int64_t num_graphs) { return num_rows / kTile + num_graphs; }

Members members_of(const void* members, int32_t dtype, int64_t row_stride, int64_t member_stride,
                   int32_t num_members, double scale, double shift) {
  return Members{members, row_stride, member_stride, scale, shift, dtype == GINE_FIELD_F64,
                 (int)num_members};
}

}  // namespace
}  // namespace gine

using namespace gine;

extern "C" int gine_field_energy_partials(int64_t num_rows, int64_t num_graphs,
                                          int32_t num_members, size_t* count) {
  if (!count) return GINE_ERR_INVALID;
  const int rc = check_args(GINE_FIELD_F32, 0, 0, num_members, num_rows, num_graphs);
  if (rc != GINE_OK) return rc;
  const size_t per = (size_t)num_members * (size_t)(num_members + 1) / 2 + 2;
  *count = (size_t)num_slots(num_rows, num_graphs) * per;
  return GINE_OK;
}

extern "C" int gine_field_variogram_partials(int64_t num_rows, int64_t num_graphs,
                                             size_t* count) {
  if (!count) return GINE_ERR_INVALID;
  const int rc = check_args(GINE_FIELD_F32, 0, 0, 1, num_rows, num_graphs);
  if (rc != GINE_OK) return rc;
  *count = (size_t)num_slots(num_rows, num_graphs) * (size_t)(2 + kVsSplit);
  return GINE_OK;
}

extern "C" int gine_field_area_partials(int64_t num_rows, int64_t num_graphs, size_t* count) {
  if (!count) return GINE_ERR_INVALID;
  const int rc = check_args(GINE_FIELD_F32, 0, 0, 1, num_rows, num_graphs);
  if (rc != GINE_OK) return rc;
  *count = 0;  // one workgroup per graph: nothing crosses workgroups
  return GINE_OK;
}

extern "C" int gine_field_energy(const void* members, int32_t dtype, int64_t row_stride,
                                 int64_t member_stride, int32_t num_members, double scale,
                                 double shift, const float* y, int64_t num_rows,
                                 const int64_t* ptr, int64_t num_graphs, double* es,
                                 double* es_fair, double* members_valid, double* rows_valid,
                                 double* partials, void* stream) {
  const int rc = check_args(dtype, row_stride, member_stride, num_members, num_rows, num_graphs);
  if (rc != GINE_OK) return rc;
  if (num_graphs == 0 || num_rows == 0) return GINE_OK;
  if (!members || !y || !ptr || !partials) return GINE_ERR_INVALID;
  const Members mb =
      members_of(members, dtype, row_stride, member_stride, num_members, scale, shift);
  const dim3 grid((unsigned)num_slots(num_rows, num_graphs));
  hipLaunchKernelGGL(k_field_energy_tiles, grid, dim3(kThreads), 0, as_stream(stream), mb, y,
                     ptr, num_graphs, num_rows, partials);
  GINE_LAUNCH_STATUS();
  hipLaunchKernelGGL(k_field_energy_finish, dim3((unsigned)num_graphs), dim3(kThreads), 0,
                     as_stream(stream), partials, ptr, num_rows, (int)num_members, es, es_fair,
                     members_valid, rows_valid);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_field_variogram(const void* members, int32_t dtype, int64_t row_stride,
                                    int64_t member_stride, int32_t num_members, double scale,
                                    double shift, const float* y, int64_t num_rows,
                                    const int64_t* ptr, int64_t num_graphs, double p, double* vs,
                                    double* pairs, double* members_valid, double* rows_valid,
                                    double* partials, void* stream) {
  const int rc = check_args(dtype, row_stride, member_stride, num_members, num_rows, num_graphs);
  if (rc != GINE_OK) return rc;
  if (!(p > 0.0) || p > 1.0e300) return GINE_ERR_INVALID;  // also NaN and +inf
  if (num_graphs == 0 || num_rows == 0) return GINE_OK;
  if (!members || !y || !ptr || !partials) return GINE_ERR_INVALID;
  const Members mb =
      members_of(members, dtype, row_stride, member_stride, num_members, scale, shift);
  const int64_t slots = num_slots(num_rows, num_graphs);
  double* mask_words = partials;
  double* row_words = partials + slots;
  double* sums = partials + 2 * slots;
  hipLaunchKernelGGL(k_field_tile_validity, dim3((unsigned)slots), dim3(kThreads), 0,
                     as_stream(stream), mb, y, ptr, num_graphs, num_rows, mask_words, row_words);
  GINE_LAUNCH_STATUS();
  const dim3 grid((unsigned)slots, kVsSplit);
#define LAUNCH_VS(PK_)                                                                        \
  hipLaunchKernelGGL((k_field_variogram_tiles<PK_>), grid, dim3(kThreads), 0,                 \
                     as_stream(stream), mb, y, ptr, num_graphs, num_rows, p, mask_words,      \
                     row_words, sums)
  if (p == 0.5) LAUNCH_VS(0);
  else if (p == 1.0) LAUNCH_VS(1);
  else if (p == 2.0) LAUNCH_VS(2);
  else LAUNCH_VS(3);
#undef LAUNCH_VS
  GINE_LAUNCH_STATUS();
  hipLaunchKernelGGL(k_field_variogram_finish, dim3((unsigned)ceil_div(num_graphs, kWave)),
                     dim3(kWave), 0, as_stream(stream), mask_words, row_words, sums, ptr,
                     num_graphs, num_rows, (int)num_members, vs, pairs, members_valid,
                     rows_valid);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_field_area(const void* members, int32_t dtype, int64_t row_stride,
                               int64_t member_stride, int32_t num_members, double scale,
                               double shift, const float* y, int64_t num_rows,
                               const int64_t* ptr, int64_t num_graphs, int32_t stat,
                               double* members_out, double* obs, double* crps,
                               double* crps_fair, double* rank_lo, double* rank_hi,
                               double* members_valid, double* rows_valid, double* partials,
                               void* stream) {
  (void)partials;
  const int rc = check_args(dtype, row_stride, member_stride, num_members, num_rows, num_graphs);
  if (rc != GINE_OK) return rc;
  if (stat != GINE_FIELD_MAX && stat != GINE_FIELD_MEAN) return GINE_ERR_INVALID;
  if (num_graphs == 0 || num_rows == 0) return GINE_OK;
  if (!members || !y || !ptr) return GINE_ERR_INVALID;
  const Members mb =
      members_of(members, dtype, row_stride, member_stride, num_members, scale, shift);
  const dim3 grid((unsigned)num_graphs);
  if (stat == GINE_FIELD_MEAN)
    hipLaunchKernelGGL((k_field_area<true>), grid, dim3(kAreaThreads), 0, as_stream(stream), mb,
                       y, ptr, num_rows, members_out, obs, crps, crps_fair, rank_lo, rank_hi,
                       members_valid, rows_valid);
  else
    hipLaunchKernelGGL((k_field_area<false>), grid, dim3(kAreaThreads), 0, as_stream(stream), mb,
                       y, ptr, num_rows, members_out, obs, crps, crps_fair, rank_lo, rank_hi,
                       members_valid, rows_valid);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}
