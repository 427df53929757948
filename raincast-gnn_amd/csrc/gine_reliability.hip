// Reliability diagrams: CORP curves, consistency bands and the MCB / DSC / UNC
// split of the Brier score on a probability lattice of q steps (levels k = 0 .. q, K = q + 1).
//
//   gine_reliability_counts    p [N, T] (through its strides), y [N], x [T] -> the level of every
//                              cell (int16, -1 = invalid) and, per column, the valid cells n_k
//                              and the events e_k of each level: histograms in LDS, flushed with
//                              integer adds (any order gives the same integers).
//   gine_reliability_fit       per column: pool-adjacent-violators over the non-empty levels
//                              ascending, decided exactly in int64, and the column statistics.
//                              One wavefront per column; the pass itself is one lane's.
//   gine_reliability_resample  per (replicate, column): synthetic events under the lattice
//                              forecast's own probabilities, U < floor(v_k * 2^53) with one
//                              counter-based U per (replicate, row) shared by the columns, their
//                              histogram in LDS, and the same fit.  A workgroup takes one
//                              replicate and a tile of columns.
//
// The fit's stack lives in LDS, in place: stage b of the E stack overwrites e[b] and of the N
// stack n[b], b <= the level just read, so the consumed part of the histograms is the stack.
// The block's first level is a third array of 16-bit words.
//
// Two traversals count the synthetic events, both order-free in the integers they produce:
//   GINE_RELIABILITY_ATOMIC   one LDS atomic add per firing cell;
//   GINE_RELIABILITY_BALLOT   K <= 64: a wavefront counts level k of its 64 rows by ballot and
//                             popcount, lane k keeps the count, and one uncontended LDS add per
//                             lane and 64 rows puts it into the histogram (no sort needed: the
//                             rows of a level need not be adjacent, and U stays shared).
// The atomic form is the faster one at K = 12 as well and is what
// GINE_RELIABILITY_AUTO takes; the ballot form stays selectable for the comparison.
// Every loop is bounded by K, N or the column tile; no workgroup waits for another.
#include "gine_common.hpp"

namespace gine {
namespace {

constexpr int kThreads = 256;
constexpr int kResampleThreads = 1024;               // 16 wavefronts share a replicate's LDS
constexpr int kResampleWaves = kResampleThreads / kWave;
constexpr int kMaxK = GINE_RELIABILITY_MAX_LEVELS + 1;
constexpr int kCountRows = 16;                       // rows of a thread in the counts kernel
constexpr int kMaxCols = 16;                         // columns of a resampling workgroup
constexpr int kLdsBytes = 80 * 1024;                 // of a resampling workgroup: two a CU
constexpr int kColBytes = 4 + 4 + 2;                 // e / E stack, n / N stack, first level

__device__ __forceinline__ uint64_t mix(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Pav {
  int blocks;
  int64_t n, E, A2;
  double S;  // the sum before the division by n
};

// One lane's pass over the levels of a column: eh[k] events and nh[k] valid cells of level k on
// entry; on return eh[b], nh[b], first[b] describe block b = 0 .. blocks - 1 (ascending).
__device__ Pav pav_column(int32_t* eh, int32_t* nh, uint16_t* first, int K, double qd) {
  Pav r{0, 0, 0, 0, 0.0};
  int64_t below = 0;  // non-events at the levels below k
  for (int k = 0; k < K; ++k) {
    const int32_t nk = nh[k];
    if (nk == 0) continue;
    const int32_t ek = eh[k];
    const double v = (double)k / qd, w = 1.0 - v;
    const double vv = v * v, ww = w * w;
    const double t0 = (double)(nk - ek) * vv, t1 = (double)ek * ww;
    const double term = t0 + t1;
    r.S = r.S + term;
    r.A2 += (int64_t)ek * (2 * below + (int64_t)(nk - ek));
    below += nk - ek;
    r.n += nk;
    r.E += ek;
    int64_t cE = ek, cN = nk;
    uint16_t cF = (uint16_t)k;
    int b = r.blocks;
    while (b > 0) {  // at most one pop per block ever pushed: bounded by K over the whole pass
      const int64_t pE = eh[b - 1], pN = nh[b - 1];
      if (pE * cN < cE * pN) break;
      cE += pE;
      cN += pN;
      cF = first[b - 1];
      --b;
    }
    eh[b] = (int32_t)cE;  // b <= k: level k is read already
    nh[b] = (int32_t)cN;
    first[b] = cF;
    r.blocks = b + 1;
  }
  return r;
}

// sum over the blocks ascending of E_b * ((N_b - E_b) / N_b), before the division by n
__device__ double calibrated_sum(const int32_t* eh, const int32_t* nh, int blocks) {
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) {
    const double Eb = (double)eh[b], Nb = (double)nh[b];
    const double frac = (double)(nh[b] - eh[b]) / Nb;
    const double term = Eb * frac;
    s = s + term;
  }
  return s;
}

// the block of level k: the last one whose first level is <= k (blocks >= 1, first[0] <= k)
__device__ __forceinline__ int block_of(const uint16_t* first, int blocks, int k) {
  int lo = 0, hi = blocks - 1;
  while (lo < hi) {  // at most 13 rounds
    const int mid = (lo + hi + 1) >> 1;
    if ((int)first[mid] <= k) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_reliability_counts(
    const double* __restrict__ p, int64_t row_stride, int64_t col_stride,
    const float* __restrict__ y, const double* __restrict__ x, int64_t N, int K, double qd,
    int32_t* __restrict__ n_k, int32_t* __restrict__ e_k, int16_t* __restrict__ level) {
  __shared__ int32_t s_n[kMaxK], s_e[kMaxK];
  const int t = blockIdx.y;
  for (int k = threadIdx.x; k < K; k += kThreads) {
    s_n[k] = 0;
    s_e[k] = 0;
  }
  __syncthreads();
  const double xt = x[t];
  const int64_t row0 = (int64_t)blockIdx.x * (kThreads * kCountRows);
  for (int j = 0; j < kCountRows; ++j) {
    const int64_t i = row0 + (int64_t)j * kThreads + threadIdx.x;
    if (i >= N) break;
    const double yi = (double)y[i];
    const double pi = p[i * row_stride + (int64_t)t * col_stride];
    const bool ok = yi == yi && xt == xt && pi >= 0.0 && pi <= 1.0;
    int k = -1;
    if (ok) {
      k = (int)rint(pi * qd);  // 0 .. q
      atomicAdd(&s_n[k], 1);
      if (yi > xt) atomicAdd(&s_e[k], 1);
    }
    level[(int64_t)t * N + i] = (int16_t)k;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += kThreads) {
    if (s_n[k]) atomicAdd(&n_k[(int64_t)t * K + k], s_n[k]);
    if (s_e[k]) atomicAdd(&e_k[(int64_t)t * K + k], s_e[k]);
  }
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void k_reliability_fit(
    const int32_t* __restrict__ n_k, const int32_t* __restrict__ e_k, int K, double qd,
    double* __restrict__ cal, int32_t* __restrict__ block_id, int32_t* __restrict__ block_e,
    int32_t* __restrict__ block_n, int32_t* __restrict__ num_blocks, int64_t* __restrict__ a2,
    double* __restrict__ stats) {
  __shared__ int32_t s_e[kMaxK], s_n[kMaxK];
  __shared__ uint16_t s_first[kMaxK];
  __shared__ int s_blocks;
  const int t = blockIdx.x, lane = threadIdx.x;
  const int64_t base = (int64_t)t * K;
  for (int k = lane; k < K; k += kWave) {
    s_n[k] = n_k[base + k];
    s_e[k] = e_k[base + k];
  }
  __syncthreads();
  if (lane == 0) {
    const Pav r = pav_column(s_e, s_n, s_first, K, qd);
    const double n = (double)r.n, E = (double)r.E;
    const double S = r.S / n;
    const double S_cal = calibrated_sum(s_e, s_n, r.blocks) / n;
    const double UNC = E * ((double)(r.n - r.E) / n) / n;
    s_blocks = r.blocks;
    if (num_blocks) num_blocks[t] = r.blocks;
    if (a2) a2[t] = r.A2;
    if (stats) {
      double* o = stats + (int64_t)t * 8;
      o[0] = n;
      o[1] = E;
      o[2] = S;
      o[3] = S_cal;
      o[4] = UNC;
      o[5] = S - S_cal;
      o[6] = UNC - S_cal;
      o[7] = (double)r.A2 / ((2.0 * E) * (double)(r.n - r.E));
    }
  }
  __syncthreads();
  const int blocks = s_blocks;
  const double nan = __builtin_nan("");
  for (int k = lane; k < K; k += kWave) {
    const bool has = n_k[base + k] > 0;  // then blocks >= 1 and first[0] <= k
    const int b = has ? block_of(s_first, blocks, k) : -1;
    if (cal) cal[base + k] = has ? (double)s_e[b] / (double)s_n[b] : nan;
    if (block_id) block_id[base + k] = b;
    if (block_e) block_e[base + k] = k < blocks ? s_e[k] : 0;
    if (block_n) block_n[base + k] = k < blocks ? s_n[k] : 0;
  }
}

// ---------------------------------------------------------------------------------------
template <bool BALLOT>
__global__ __launch_bounds__(kResampleThreads) void k_reliability_resample(
    const int16_t* __restrict__ level, const int32_t* __restrict__ n_k, int64_t N, int T, int K,
    double qd, int cols_per_block, uint64_t seed, uint64_t rep_first, double* __restrict__ cal_rep,
    double* __restrict__ stats_rep, int32_t* __restrict__ e_rep) {
  extern __shared__ uint64_t s_thr[];  // [K], then per column e [K], n [K], then first [K] each
  __shared__ int s_blocks[kMaxCols];
  int32_t* s_hist = reinterpret_cast<int32_t*>(s_thr + K);
  uint16_t* s_first = reinterpret_cast<uint16_t*>(s_hist + (size_t)cols_per_block * 2 * K);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int t0 = blockIdx.y * cols_per_block;
  const int cols = T - t0 < cols_per_block ? T - t0 : cols_per_block;
  const int64_t row = blockIdx.x;
  const uint64_t r = rep_first + (uint64_t)row;

  for (int k = threadIdx.x; k < K; k += kResampleThreads) {
    const double v = (double)k / qd;
    s_thr[k] = (uint64_t)(v * 9007199254740992.0);  // floor(v * 2^53): 0 .. 2^53
  }
  for (int c = 0; c < cols; ++c) {
    int32_t* eh = s_hist + (size_t)c * 2 * K;
    for (int k = threadIdx.x; k < K; k += kResampleThreads) {
      eh[k] = 0;
      eh[K + k] = n_k[(int64_t)(t0 + c) * K + k];
    }
  }
  __syncthreads();

  // the loop bound is uniform over the workgroup (the ballots below need whole wavefronts)
  const int64_t rounds = (N + kResampleThreads - 1) / kResampleThreads;
  for (int64_t j = 0; j < rounds; ++j) {
    const int64_t i = j * kResampleThreads + threadIdx.x;
    const bool in = i < N;
    const uint64_t U = mix(seed, r * (uint64_t)N + (uint64_t)(in ? i : 0)) >> 11;
    for (int c = 0; c < cols; ++c) {
      int32_t* eh = s_hist + (size_t)c * 2 * K;
      const int lvl = in ? (int)level[(int64_t)(t0 + c) * N + i] : -1;
      const bool cell = (unsigned)lvl < (unsigned)K;
      const bool fire = cell && U < s_thr[cell ? lvl : 0];
      if constexpr (BALLOT) {
        int mine = 0;
        for (int k = 0; k < K; ++k) {  // K <= 64
          const int cnt = __popcll(__ballot(fire && lvl == k));
          mine = lane == k ? cnt : mine;
        }
        if (mine) atomicAdd(&eh[lane], mine);  // mine != 0 only at lane < K
      } else {
        if (fire) atomicAdd(&eh[lvl], 1);
      }
    }
  }
  __syncthreads();

  if (e_rep) {
    for (int c = 0; c < cols; ++c) {
      const int32_t* eh = s_hist + (size_t)c * 2 * K;
      const int64_t o = (row * T + t0 + c) * K;
      for (int k = threadIdx.x; k < K; k += kResampleThreads) e_rep[o + k] = eh[k];
    }
    __syncthreads();
  }

  if (lane == 0) {
    for (int c = wave; c < cols; c += kResampleWaves) {
      int32_t* eh = s_hist + (size_t)c * 2 * K;
      const Pav f = pav_column(eh, eh + K, s_first + (size_t)c * K, K, qd);
      s_blocks[c] = f.blocks;
      if (stats_rep) {
        const double n = (double)f.n;
        const double S = f.S / n;
        const double S_cal = calibrated_sum(eh, eh + K, f.blocks) / n;
        double* o = stats_rep + (row * T + t0 + c) * 3;
        o[0] = S;
        o[1] = S_cal;
        o[2] = S - S_cal;
      }
    }
  }
  __syncthreads();

  if (!cal_rep) return;
  const double nan = __builtin_nan("");
  for (int c = 0; c < cols; ++c) {
    const int32_t* eh = s_hist + (size_t)c * 2 * K;
    const uint16_t* first = s_first + (size_t)c * K;
    const int blocks = s_blocks[c];
    const int64_t o = (row * T + t0 + c) * K;
    for (int k = threadIdx.x; k < K; k += kResampleThreads) {
      const bool has = n_k[(int64_t)(t0 + c) * K + k] > 0;
      double v = nan;
      if (has) {
        const int b = block_of(first, blocks, k);
        v = (double)eh[b] / (double)eh[K + b];
      }
      cal_rep[o + k] = v;
    }
  }
}

template <bool BALLOT>
int set_lds_limit() {
  static const hipError_t e = hipFuncSetAttribute(
      reinterpret_cast<const void*>(k_reliability_resample<BALLOT>),
      hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
  return e == hipSuccess ? GINE_OK : GINE_ERR_HIP_BASE + (int)e;
}

// LDS bytes of a resampling workgroup of `cols` columns (the first-level words stay aligned:
// everything before them is a multiple of 4 bytes)
size_t resample_lds(int K, int cols) { return (size_t)K * 8 + (size_t)cols * K * kColBytes; }

int check_lattice(int64_t N, int32_t T, int32_t q) {
  if (N < 0 || T < 0) return GINE_ERR_INVALID;
  if (q < 1 || q > GINE_RELIABILITY_MAX_LEVELS) return GINE_ERR_INVALID;
  if (N >= (1ll << 30) || T > 65535) return GINE_ERR_TOO_LARGE;
  return GINE_OK;
}

}  // namespace
}  // namespace gine

using namespace gine;

extern "C" int gine_reliability_counts(const double* p, int64_t p_row_stride,
                                       int64_t p_col_stride, const float* y, const double* x,
                                       int64_t num_rows, int32_t num_thresholds, int32_t q,
                                       int32_t* n_k, int32_t* e_k, int16_t* level,
                                       void* stream) {
  const int rc = check_lattice(num_rows, num_thresholds, q);
  if (rc != GINE_OK) return rc;
  if (p_row_stride < 0 || p_col_stride < 0) return GINE_ERR_INVALID;
  if (!n_k || !e_k) return GINE_ERR_INVALID;
  if (num_thresholds == 0) return GINE_OK;
  if (!x) return GINE_ERR_INVALID;
  if (num_rows > 0 && (!p || !y || !level)) return GINE_ERR_INVALID;
  const int K = q + 1;
  const size_t bytes = (size_t)num_thresholds * K * sizeof(int32_t);
  GINE_RETURN_IF_HIP(hipMemsetAsync(n_k, 0, bytes, as_stream(stream)));
  GINE_RETURN_IF_HIP(hipMemsetAsync(e_k, 0, bytes, as_stream(stream)));
  if (num_rows == 0) return GINE_OK;
  const dim3 grid((unsigned)ceil_div(num_rows, (int64_t)kThreads * kCountRows),
                  (unsigned)num_thresholds);
  hipLaunchKernelGGL(k_reliability_counts, grid, dim3(kThreads), 0, as_stream(stream), p,
                     p_row_stride, p_col_stride, y, x, num_rows, K, (double)q, n_k, e_k, level);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_reliability_fit(const int32_t* n_k, const int32_t* e_k,
                                    int32_t num_thresholds, int32_t q, double* cal,
                                    int32_t* block_id, int32_t* block_e, int32_t* block_n,
                                    int32_t* num_blocks, int64_t* a2, double* stats,
                                    void* stream) {
  const int rc = check_lattice(0, num_thresholds, q);
  if (rc != GINE_OK) return rc;
  if (!n_k || !e_k) return GINE_ERR_INVALID;
  if (!cal && !block_id && !block_e && !block_n && !num_blocks && !a2 && !stats)
    return GINE_ERR_INVALID;
  if (num_thresholds == 0) return GINE_OK;
  hipLaunchKernelGGL(k_reliability_fit, dim3((unsigned)num_thresholds), dim3(kWave), 0,
                     as_stream(stream), n_k, e_k, q + 1, (double)q, cal, block_id, block_e,
                     block_n, num_blocks, a2, stats);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_reliability_resample(const int16_t* level, const int32_t* n_k,
                                         int64_t num_rows, int32_t num_thresholds, int32_t q,
                                         uint64_t seed, uint64_t rep_first,
                                         int64_t num_replicates, int32_t traversal,
                                         double* cal_rep, double* stats_rep, int32_t* e_rep,
                                         void* stream) {
  const int rc = check_lattice(num_rows, num_thresholds, q);
  if (rc != GINE_OK) return rc;
  if (num_replicates < 0 || num_replicates > 0x7fffffffll) {
    return num_replicates < 0 ? GINE_ERR_INVALID : GINE_ERR_TOO_LARGE;
  }
  const int K = q + 1;
  if (traversal != GINE_RELIABILITY_AUTO && traversal != GINE_RELIABILITY_ATOMIC &&
      traversal != GINE_RELIABILITY_BALLOT)
    return GINE_ERR_INVALID;
  if (traversal == GINE_RELIABILITY_BALLOT && K > kWave) return GINE_ERR_INVALID;
  if (!n_k || (num_rows > 0 && !level)) return GINE_ERR_INVALID;
  if (!cal_rep && !stats_rep && !e_rep) return GINE_ERR_INVALID;
  if (num_replicates == 0 || num_thresholds == 0) return GINE_OK;
  int cols = num_thresholds < kMaxCols ? num_thresholds : kMaxCols;
  while (cols > 1 && resample_lds(K, cols) > (size_t)kLdsBytes) --cols;  // one column always fits
  const bool ballot = traversal == GINE_RELIABILITY_BALLOT;  // AUTO: the atomic form (6k)
  const dim3 grid((unsigned)num_replicates, (unsigned)ceil_div(num_thresholds, cols));
  const size_t lds = resample_lds(K, cols);
#define LAUNCH_RESAMPLE(B_)                                                                    \
  do {                                                                                         \
    const int lrc = set_lds_limit<B_>();                                                       \
    if (lrc != GINE_OK) return lrc;                                                            \
    hipLaunchKernelGGL((k_reliability_resample<B_>), grid, dim3(kResampleThreads), lds,                \
                       as_stream(stream), level, n_k, num_rows, (int)num_thresholds, K,        \
                       (double)q, cols, seed, rep_first, cal_rep, stats_rep, e_rep);           \
  } while (0)
  if (ballot) LAUNCH_RESAMPLE(true);
  else LAUNCH_RESAMPLE(false);
#undef LAUNCH_RESAMPLE
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}
