// Paired score comparison: two fp64 score grids a, b over the same [T days, S
// stations], element (t, s) at  p[t * day_stride + s * station_stride]  (strides in elements,
// >= 0, nothing copied); a pair is valid when both elements are non-NaN.
//
//   gine_compare_reduce     the marginal sums: per station over the days ascending, per day over
//                           its stations (one wavefront per day: lane l adds stations l, l + 64,
//                           ... in ascending order, then the 64 lane sums fold in halves,
//                           32 + 32 -> 16 + 16 -> ... -> 1).
//   gine_compare_bootstrap  circular moving-block bootstrap: thread = one (replicate, station),
//                           which walks the replicate's T draws in order and adds every valid
//                           pair into its own (A, B, W): the sequential order of the contract,
//                           no cross-lane sum at all.  The draws come from a counter-based
//                           generator (one mix per block of block_len days); no index is stored.
//   gine_compare_dm         Diebold-Mariano per station with Bartlett weights.
//
// Lanes run across stations (a [T, S] grid is row-major in practice, so a wavefront's 64 loads
// of one day are one 512-byte line) and, where there are fewer than 64 stations, across
// replicates: a workgroup of 256 threads is SW station lanes x 256 / SW replicates, SW the power
// of two >= min(S, 64).  The SW lanes of a replicate share its block starts: each computes one
// of SW consecutive starts and the group passes them round with a lane shuffle.  Unweighted
// grids of at least 8 stations, at most 1,024 days and at least 128 replicates run against a
// tile staged in LDS instead (k_compare_bootstrap_lds below): the same bits, 2 to 2.3 times the
// rate.
//
// Every load is in bounds whatever the lane: day < T by construction (start < T, one conditional
// subtraction of T) and a lane past the last station reads station S - 1 and stores nothing.
#include "gine_common.hpp"

namespace gine {
namespace {

constexpr int kThreads = GINE_COMPARE_REP_TILE;  // replicates of a workgroup at one station lane
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxLags = GINE_COMPARE_MAX_LAGS;
constexpr int kLdsThreads = 1024;                     // the LDS form: 16 wavefronts over
constexpr int kLdsStations = 8;                       // 8 stations x
constexpr int kLdsReps = kLdsThreads / kLdsStations;  // 128 replicates a pass
constexpr int kLdsBytes = 160 * 1024;
constexpr int kLdsCell = 16 + 4;                      // (a, b) and the validity word
constexpr int kLdsMaxDays = kLdsBytes / (kLdsStations * kLdsCell);  // 1,024
constexpr int kLdsTargetBlocks = 8 * kNumCu;
static_assert(kThreads == 256, "the lane maps below assume four wavefronts");

struct Grid {
  const double* p;
  int64_t day_stride, station_stride;
};

__device__ __forceinline__ double at(const Grid& g, int64_t day, int64_t station) {
  return g.p[day * g.day_stride + station * g.station_stride];
}

__device__ __forceinline__ uint64_t mix(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// first day of block j of global replicate r: the high word of mix times T, shifted down
__device__ __forceinline__ uint32_t block_start(uint64_t seed, uint64_t r, uint64_t nb,
                                                uint64_t j, uint32_t T) {
  return __umulhi((uint32_t)(mix(seed, r * nb + j) >> 32), T);
}

// ---------------------------------------------------------------------------------------
// Marginal sums
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_compare_stations(
    Grid a, Grid b, int64_t T, int64_t S, double* __restrict__ station_a,
    double* __restrict__ station_b, double* __restrict__ station_n) {
  const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= S) return;
  double A = 0.0, B = 0.0, n = 0.0;
#pragma unroll 4
  for (int64_t t = 0; t < T; ++t) {
    const double x = at(a, t, s), y = at(b, t, s);
    const bool ok = x == x && y == y;
    A += ok ? x : 0.0;  // a sum that started at +0 is never -0: adding +0 keeps its bits
    B += ok ? y : 0.0;
    n += ok ? 1.0 : 0.0;
  }
  if (station_a) station_a[s] = A;
  if (station_b) station_b[s] = B;
  if (station_n) station_n[s] = n;
}

__global__ __launch_bounds__(kThreads) void k_compare_days(
    Grid a, Grid b, int64_t T, int64_t S, double* __restrict__ day_a,
    double* __restrict__ day_b, double* __restrict__ day_n) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t t = (int64_t)blockIdx.x * kWaves + threadIdx.x / kWave;
  if (t >= T) return;  // the whole wavefront
  double A = 0.0, B = 0.0, n = 0.0;
  for (int64_t s = lane; s < S; s += kWave) {
    const double x = at(a, t, s), y = at(b, t, s);
    const bool ok = x == x && y == y;
    A += ok ? x : 0.0;
    B += ok ? y : 0.0;
    n += ok ? 1.0 : 0.0;
  }
  for (int off = kWave / 2; off > 0; off >>= 1) {  // lane l and lane l ^ off end up equal
    A += shfl_xor_d(A, off);
    B += shfl_xor_d(B, off);
    n += shfl_xor_d(n, off);
  }
  if (lane != 0) return;
  if (day_a) day_a[t] = A;
  if (day_b) day_b[t] = B;
  if (day_n) day_n[t] = n;
}

// ---------------------------------------------------------------------------------------
// Bootstrap
// ---------------------------------------------------------------------------------------
template <int SW, bool WEIGHTED>
__global__ __launch_bounds__(kThreads) void k_compare_bootstrap(
    Grid a, Grid b, Grid w, uint32_t T, int64_t S, uint32_t L, uint64_t nb, uint64_t seed,
    uint64_t rep_first, int64_t R, double* __restrict__ sum_a, double* __restrict__ sum_b,
    double* __restrict__ sum_w, double* __restrict__ diff, double* __restrict__ skill) {
  constexpr int kReps = kThreads / SW;  // replicates of a workgroup
  const int lane = threadIdx.x & (kWave - 1);
  const int sl = threadIdx.x % SW;
  const int64_t s = (int64_t)blockIdx.y * SW + sl;
  const int64_t row = (int64_t)blockIdx.x * kReps + threadIdx.x / SW;
  const int64_t sc = s < S ? s : S - 1;  // loads of a lane past the end stay in bounds
  const uint64_t r = rep_first + (uint64_t)row;
  const double* pa = a.p + sc * a.station_stride;
  const double* pb = b.p + sc * b.station_stride;
  const double* pw = WEIGHTED ? w.p + sc * w.station_stride : nullptr;
  double A = 0.0, B = 0.0, W = 0.0;
  uint32_t left = T;  // draws to go: uniform over the workgroup, like every loop bound below
  for (uint64_t j0 = 0; j0 < nb; j0 += SW) {
    // this lane's share of the next SW block starts of its replicate (unused past nb)
    const uint32_t mine = block_start(seed, r, nb, j0 + (uint64_t)sl, T);
    const int blocks = nb - j0 < (uint64_t)SW ? (int)(nb - j0) : SW;
    for (int i = 0; i < blocks; ++i) {
      const uint32_t first = SW == 1 ? mine : (uint32_t)__shfl((int)mine, (lane & ~(SW - 1)) + i,
                                                               kWave);
      const uint32_t len = L < left ? L : left;
      left -= len;
#pragma unroll 4
      for (uint32_t k = 0; k < len; ++k) {
        uint32_t day = first + k;  // < 2 T < 2^32
        if (day >= T) day -= T;
        const double x = pa[(int64_t)day * a.day_stride];
        const double y = pb[(int64_t)day * b.day_stride];
        const bool ok = x == x && y == y;
        A += ok ? x : 0.0;
        B += ok ? y : 0.0;
        if constexpr (WEIGHTED) {
          const double v = pw[(int64_t)day * w.day_stride];
          W += ok ? v : 0.0;
        } else {
          W += ok ? 1.0 : 0.0;
        }
      }
    }
  }
  if (s >= S || row >= R) return;
  const int64_t o = row * S + s;
  if (sum_a) sum_a[o] = A;
  if (sum_b) sum_b[o] = B;
  if (sum_w) sum_w[o] = W;
  if (diff) diff[o] = (A - B) / W;
  if (skill) skill[o] = 1.0 - A / B;
}

// The same walk against a tile staged in LDS: a workgroup of 1,024 threads stages 8 stations x T
// days -- (a, b) as 16 bytes, both +0 at an invalid pair, and the pair's validity as a 32-bit
// 0 / 1 -- then runs passes of 128 replicates (8 station lanes each) against it.  A draw is two
// fp64 adds and an integer add, no compare and no select: adding +0 leaves a sum that started
// at +0 as it is, and W, a count below 2^31, is exact either way.  Each (replicate, station)
// still adds its pairs in draw order: the same bits as the kernel above, which keeps the
// weighted column, the grids too long for LDS and the runs too small to fill a tile.  UNIT is
// block_len = 1: eight draws per round, unrolled, from the eight starts of the lane group.
struct Acc {
  double A, B;
  uint32_t n;
};

__device__ __forceinline__ void draw(Acc& acc, const double2* tile, const uint32_t* flags,
                                     uint32_t slot) {
  const double2 v = tile[slot];
  acc.A += v.x;
  acc.B += v.y;
  acc.n += flags[slot];
}

template <bool UNIT>
__global__ __launch_bounds__(kLdsThreads) void k_compare_bootstrap_lds(
    Grid a, Grid b, uint32_t T, int64_t S, uint32_t L, uint32_t nb, uint64_t seed,
    uint64_t rep_first, int64_t R, int64_t reps_per_block, double* __restrict__ sum_a,
    double* __restrict__ sum_b, double* __restrict__ sum_w, double* __restrict__ diff,
    double* __restrict__ skill) {
  extern __shared__ double2 tile[];  // [T][kLdsStations], then the flags [T][kLdsStations]
  constexpr int SW = kLdsStations;
  uint32_t* flags = reinterpret_cast<uint32_t*>(tile + T * SW);
  const int lane = threadIdx.x & (kWave - 1);
  const int group = lane & ~(SW - 1);
  const uint32_t sl = threadIdx.x % SW;
  const double2* my_tile = tile + sl;  // this lane's column: slot = day * SW
  const uint32_t* my_flags = flags + sl;
  const int64_t s0 = (int64_t)blockIdx.y * SW, s = s0 + sl;
  for (uint32_t e = threadIdx.x; e < T * SW; e += kLdsThreads) {
    const int64_t t = e / SW, col = s0 + e % SW;
    const int64_t sc = col < S ? col : S - 1;
    const double x = at(a, t, sc), y = at(b, t, sc);
    const bool ok = x == x && y == y;
    tile[e] = make_double2(ok ? x : 0.0, ok ? y : 0.0);
    flags[e] = ok ? 1u : 0u;
  }
  __syncthreads();
  const int64_t row_begin = (int64_t)blockIdx.x * reps_per_block;
  const int64_t row_end = row_begin + reps_per_block < R ? row_begin + reps_per_block : R;
  for (int64_t row0 = row_begin; row0 < row_end; row0 += kLdsReps) {  // uniform
    const int64_t row = row0 + threadIdx.x / SW;
    const uint64_t r = rep_first + (uint64_t)row;
    Acc acc{0.0, 0.0, 0u};
    uint32_t j0 = 0;
    if constexpr (UNIT) {
      for (; j0 + SW <= nb; j0 += SW) {
        const uint32_t mine = block_start(seed, r, nb, j0 + sl, T) * SW;
        // the eight slots, then the eight reads, then the adds in draw order: LDS reads in flight
        uint32_t slot[SW], f[SW];
        double2 v[SW];
#pragma unroll
        for (int i = 0; i < SW; ++i) slot[i] = (uint32_t)__shfl((int)mine, group + i, kWave);
#pragma unroll
        for (int i = 0; i < SW; ++i) {
          v[i] = my_tile[slot[i]];
          f[i] = my_flags[slot[i]];
        }
#pragma unroll
        for (int i = 0; i < SW; ++i) {
          acc.A += v[i].x;
          acc.B += v[i].y;
          acc.n += f[i];
        }
      }
    }
    uint32_t left = T - (UNIT ? j0 : 0u);
    for (; j0 < nb; j0 += SW) {
      const uint32_t mine = block_start(seed, r, nb, j0 + sl, T);
      const int blocks = nb - j0 < (uint32_t)SW ? (int)(nb - j0) : SW;
      for (int i = 0; i < blocks; ++i) {
        const uint32_t first = (uint32_t)__shfl((int)mine, group + i, kWave);
        const uint32_t len = L < left ? L : left;
        left -= len;
#pragma unroll 4
        for (uint32_t k = 0; k < len; ++k) {
          const uint32_t day = first + k;  // below 2 T: day - T wraps past it unless day >= T
          draw(acc, my_tile, my_flags, (day < day - T ? day : day - T) * SW);
        }
      }
    }
    if (s < S && row < row_end) {
      const int64_t o = row * S + s;
      const double A = acc.A, B = acc.B, W = (double)acc.n;
      if (sum_a) sum_a[o] = A;
      if (sum_b) sum_b[o] = B;
      if (sum_w) sum_w[o] = W;
      if (diff) diff[o] = (A - B) / W;
      if (skill) skill[o] = 1.0 - A / B;
    }
  }
}

template <bool UNIT>
int set_lds_limit() {
  static const hipError_t e = hipFuncSetAttribute(
      reinterpret_cast<const void*>(k_compare_bootstrap_lds<UNIT>),
      hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
  return e == hipSuccess ? GINE_OK : GINE_ERR_HIP_BASE + (int)e;
}

// ---------------------------------------------------------------------------------------
// Diebold-Mariano: a workgroup takes 64 stations (lane = station); wave 0 counts the valid days
// and takes the mean difference, then wave v sums the autocovariances of lags v, v + 4, ...
// over the days ascending, and wave 0 adds them up with their Bartlett weights.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_compare_dm(
    Grid a, Grid b, int64_t T, int64_t S, int lags, double* __restrict__ n_out,
    double* __restrict__ mean_out, double* __restrict__ var_out, double* __restrict__ stat_out,
    double* __restrict__ p_out) {
  __shared__ double s_g[kMaxLags + 1][kWave];
  __shared__ double s_n[kWave], s_mean[kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t s = (int64_t)blockIdx.x * kWave + lane;
  const int64_t sc = s < S ? s : S - 1;
  const double* pa = a.p + sc * a.station_stride;
  const double* pb = b.p + sc * b.station_stride;
  if (wave == 0) {
    double sum = 0.0, n = 0.0;
#pragma unroll 4
    for (int64_t t = 0; t < T; ++t) {
      const double x = pa[t * a.day_stride], y = pb[t * b.day_stride];
      const bool ok = x == x && y == y;
      sum += ok ? x - y : 0.0;
      n += ok ? 1.0 : 0.0;
    }
    s_n[lane] = n;
    s_mean[lane] = sum / n;  // NaN at n = 0
  }
  __syncthreads();
  const double n = s_n[lane], mean = s_mean[lane];
  for (int k = wave; k <= lags; k += kWaves) {
    double g = 0.0;
#pragma unroll 2
    for (int64_t t = 0; t + k < T; ++t) {
      const double x0 = pa[t * a.day_stride], y0 = pb[t * b.day_stride];
      const double x1 = pa[(t + k) * a.day_stride], y1 = pb[(t + k) * b.day_stride];
      const double term = ((x0 - y0) - mean) * ((x1 - y1) - mean);
      g += (x0 == x0 && y0 == y0 && x1 == x1 && y1 == y1) ? term : 0.0;
    }
    s_g[k][lane] = g / n;
  }
  __syncthreads();
  if (wave != 0 || s >= S) return;
  double v = s_g[0][lane];
  const double span = (double)lags + 1.0;
  for (int k = 1; k <= lags; ++k) v += 2.0 * (1.0 - (double)k / span) * s_g[k][lane];
  const double var = v / n, nan = __builtin_nan("");
  const bool ok = n >= 2.0 && var > 0.0 && var <= 1.7976931348623157e308;
  const double stat = ok ? mean / sqrt(var) : nan;
  if (n_out) n_out[s] = n;
  if (mean_out) mean_out[s] = mean;
  if (var_out) var_out[s] = var;
  if (stat_out) stat_out[s] = stat;
  if (p_out) p_out[s] = ok ? erfc(fabs(stat) * 0.70710678118654752440) : nan;
}

// a, b and their sizes, before any HIP call
int check_grids(const double* a, int64_t a_day, int64_t a_station, const double* b,
                int64_t b_day, int64_t b_station, int64_t T, int64_t S) {
  if (!a || !b) return GINE_ERR_INVALID;
  if (a_day < 0 || a_station < 0 || b_day < 0 || b_station < 0) return GINE_ERR_INVALID;
  if (T < 1 || S < 1) return GINE_ERR_INVALID;
  if (T > 0x7fffffffll) return GINE_ERR_TOO_LARGE;
  return GINE_OK;
}

// station lanes of a bootstrap workgroup: the power of two >= min(S, 64)
int station_lanes(int64_t S) {
  int sw = 1;
  while (sw < kWave && sw < S) sw *= 2;
  return sw;
}

}  // namespace
}  // namespace gine

using namespace gine;

extern "C" int gine_compare_reduce(const double* a, int64_t a_day_stride,
                                   int64_t a_station_stride, const double* b,
                                   int64_t b_day_stride, int64_t b_station_stride,
                                   int64_t num_days, int64_t num_stations, double* day_a,
                                   double* day_b, double* day_n, double* station_a,
                                   double* station_b, double* station_n, void* stream) {
  const int rc = check_grids(a, a_day_stride, a_station_stride, b, b_day_stride,
                             b_station_stride, num_days, num_stations);
  if (rc != GINE_OK) return rc;
  const bool days = day_a || day_b || day_n, stations = station_a || station_b || station_n;
  if (!days && !stations) return GINE_ERR_INVALID;
  if (ceil_div(num_stations, kThreads) > 0x7fffffffll) return GINE_ERR_TOO_LARGE;
  const Grid ga{a, a_day_stride, a_station_stride}, gb{b, b_day_stride, b_station_stride};
  if (stations) {
    hipLaunchKernelGGL(k_compare_stations, dim3((unsigned)ceil_div(num_stations, kThreads)),
                       dim3(kThreads), 0, as_stream(stream), ga, gb, num_days, num_stations,
                       station_a, station_b, station_n);
    GINE_LAUNCH_STATUS();
  }
  if (days) {
    hipLaunchKernelGGL(k_compare_days, dim3((unsigned)ceil_div(num_days, kWaves)),
                       dim3(kThreads), 0, as_stream(stream), ga, gb, num_days, num_stations,
                       day_a, day_b, day_n);
    GINE_LAUNCH_STATUS();
  }
  return GINE_OK;
}

extern "C" int gine_compare_bootstrap(const double* a, int64_t a_day_stride,
                                      int64_t a_station_stride, const double* b,
                                      int64_t b_day_stride, int64_t b_station_stride,
                                      const double* w, int64_t w_day_stride,
                                      int64_t w_station_stride, int64_t num_days,
                                      int64_t num_stations, int64_t block_len, uint64_t seed,
                                      uint64_t rep_first, int64_t num_replicates, double* sum_a,
                                      double* sum_b, double* sum_w, double* diff, double* skill,
                                      void* stream) {
  const int rc = check_grids(a, a_day_stride, a_station_stride, b, b_day_stride,
                             b_station_stride, num_days, num_stations);
  if (rc != GINE_OK) return rc;
  if (w_day_stride < 0 || w_station_stride < 0 || num_replicates < 0) return GINE_ERR_INVALID;
  if (block_len < 1 || block_len > num_days) return GINE_ERR_INVALID;
  if (!sum_a && !sum_b && !sum_w && !diff && !skill) return GINE_ERR_INVALID;
  const int sw = station_lanes(num_stations);
  const int64_t station_tiles = ceil_div(num_stations, sw);
  const int64_t rep_tiles = ceil_div(num_replicates, kThreads / sw);
  if (station_tiles > 65535 || rep_tiles > 0x7fffffffll) return GINE_ERR_TOO_LARGE;
  if (num_replicates == 0) return GINE_OK;
  const Grid ga{a, a_day_stride, a_station_stride}, gb{b, b_day_stride, b_station_stride};
  const Grid gw{w, w_day_stride, w_station_stride};
  const uint64_t nb = (uint64_t)ceil_div(num_days, block_len);
  const int64_t lds_tiles = ceil_div(num_stations, kLdsStations);
  if (!w && num_stations >= kLdsStations && num_days <= kLdsMaxDays &&
      num_replicates >= kLdsReps && lds_tiles <= 65535) {
    // replicates of a workgroup: whole passes, and enough workgroups to fill the device
    const int64_t groups = lds_tiles >= kLdsTargetBlocks ? 1 : kLdsTargetBlocks / lds_tiles;
    const int64_t per = ceil_div(ceil_div(num_replicates, groups), kLdsReps) * kLdsReps;
    const dim3 lgrid((unsigned)ceil_div(num_replicates, per), (unsigned)lds_tiles);
    const size_t lds = (size_t)num_days * kLdsStations * kLdsCell;
#define LAUNCH_LDS(UNIT_)                                                                       \
  do {                                                                                          \
    const int lrc = set_lds_limit<UNIT_>();                                                     \
    if (lrc != GINE_OK) return lrc;                                                             \
    hipLaunchKernelGGL((k_compare_bootstrap_lds<UNIT_>), lgrid, dim3(kLdsThreads), lds,         \
                       as_stream(stream), ga, gb, (uint32_t)num_days, num_stations,             \
                       (uint32_t)block_len, (uint32_t)nb, seed, rep_first, num_replicates, per, \
                       sum_a, sum_b, sum_w, diff, skill);                                       \
  } while (0)
    if (block_len == 1) LAUNCH_LDS(true);
    else LAUNCH_LDS(false);
#undef LAUNCH_LDS
    GINE_LAUNCH_STATUS();
    return GINE_OK;
  }
  const dim3 grid((unsigned)rep_tiles, (unsigned)station_tiles);
#define LAUNCH_BOOT(SW_, W_)                                                                  \
  hipLaunchKernelGGL((k_compare_bootstrap<SW_, W_>), grid, dim3(kThreads), 0,                 \
                     as_stream(stream), ga, gb, gw, (uint32_t)num_days, num_stations,         \
                     (uint32_t)block_len, nb, seed, rep_first, num_replicates, sum_a, sum_b,  \
                     sum_w, diff, skill)
#define LAUNCH_BOOT_SW(SW_)  \
  do {                       \
    if (w) LAUNCH_BOOT(SW_, true); \
    else LAUNCH_BOOT(SW_, false);  \
  } while (0)
  switch (sw) {
    case 1: LAUNCH_BOOT_SW(1); break;
    case 2: LAUNCH_BOOT_SW(2); break;
    case 4: LAUNCH_BOOT_SW(4); break;
    case 8: LAUNCH_BOOT_SW(8); break;
    case 16: LAUNCH_BOOT_SW(16); break;
    case 32: LAUNCH_BOOT_SW(32); break;
    default: LAUNCH_BOOT_SW(64); break;
  }
#undef LAUNCH_BOOT_SW
#undef LAUNCH_BOOT
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_compare_dm(const double* a, int64_t a_day_stride, int64_t a_station_stride,
                               const double* b, int64_t b_day_stride, int64_t b_station_stride,
                               int64_t num_days, int64_t num_stations, int32_t lags, double* n,
                               double* mean_d, double* var, double* stat, double* pvalue,
                               void* stream) {
  const int rc = check_grids(a, a_day_stride, a_station_stride, b, b_day_stride,
                             b_station_stride, num_days, num_stations);
  if (rc != GINE_OK) return rc;
  if (lags < 0 || lags >= num_days) return GINE_ERR_INVALID;
  if (lags > kMaxLags) return GINE_ERR_DIM;
  if (!n && !mean_d && !var && !stat && !pvalue) return GINE_ERR_INVALID;
  if (ceil_div(num_stations, kWave) > 0x7fffffffll) return GINE_ERR_TOO_LARGE;
  const Grid ga{a, a_day_stride, a_station_stride}, gb{b, b_day_stride, b_station_stride};
  hipLaunchKernelGGL(k_compare_dm, dim3((unsigned)ceil_div(num_stations, kWave)),
                     dim3(kThreads), 0, as_stream(stream), ga, gb, num_days, num_stations,
                     (int)lags, n, mean_d, var, stat, pvalue);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}
