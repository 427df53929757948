// Batch assembly with permuted feature columns: the rows of B samples of a
// device-resident dataset (x [T, N, F], ens [T, N, M, F], y [T, N]) written straight into the
// inputs of a forward, the columns of col_mask taken from another (sample, station):
//   slot b, station i, column f  <-  (perm_t[idx[b]], perm_n[idx[b], i])  if bit f of col_mask
//                                    (idx[b], i)                          otherwise
//   out_y[b, i] = y[idx[b], i]
//
// One wavefront copies one output row: the N stations of a slot are dealt to workgroups of four
// waves, so the slot, the station and both source rows are wave-uniform and every index is
// read once per wave through the scalar cache.  A lane copies elements lane, lane + 64, ... of
// the row's M * F floats and picks its source row by the column of each element; the column
// advances by 64 mod F per step, so nothing is divided inside the loop.  Every access is one
// dword per lane (256 contiguous bytes per wave-instruction): a row of M * F * 4 bytes (1,540
// for 11 x 35) starts on a multiple of 4, not of 16, and a wider access would straddle it.
// kUnroll loads are issued before their stores.  Offsets are 64-bit throughout.
#include "gine_common.hpp"

namespace gine {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;  // output rows of a workgroup
constexpr int kUnroll = 8;                // 512 floats per pass: an 11 x 35 row in one
constexpr int kMaxFeatures = 64;          // the bits of col_mask

__global__ __launch_bounds__(kThreads) void k_batch_fill_permuted(
    const float* __restrict__ x, const float* __restrict__ ens, const float* __restrict__ y,
    const int64_t* __restrict__ idx, const int64_t* __restrict__ perm_t,
    const int32_t* __restrict__ perm_n, uint64_t col_mask, int N, int M, int F,
    unsigned tiles_per_slot, float* __restrict__ out_x, float* __restrict__ out_ens,
    float* __restrict__ out_y) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const unsigned b = blockIdx.x / tiles_per_slot;
  const int i = (int)(blockIdx.x - b * tiles_per_slot) * kWaves + wave;
  if (i >= N) return;  // the whole wave
  const int64_t t = idx[b];
  int64_t pt = t, pi = i;
  if (col_mask != 0ull) {
    if (perm_t) pt = perm_t[t];
    if (perm_n) pi = perm_n[t * N + i];
  }
  const int64_t own = t * N + i, other = pt * N + pi, row = (int64_t)b * N + i;

  if (lane == 0) out_y[row] = y[own];
  if (lane < F) {
    const float* src = ((col_mask >> lane) & 1ull) ? x + other * F : x + own * F;
    out_x[row * F + lane] = src[lane];
  }

  const int L = M * F;
  const float* __restrict__ s_own = ens + own * L;
  const float* __restrict__ s_other = ens + other * L;
  float* __restrict__ d = out_ens + row * L;
  const int step = kWave % F;
  int f = lane % F;  // the column of element e = lane, then of e + 64, ...
  for (int e0 = lane; e0 < L; e0 += kWave * kUnroll) {
    float v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int e = e0 + u * kWave;
      const float* src = ((col_mask >> f) & 1ull) ? s_other : s_own;
      if (e < L) v[u] = src[e];
      f += step;
      if (f >= F) f -= F;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int e = e0 + u * kWave;
      if (e < L) d[e] = v[u];
    }
  }
}

}  // namespace
}  // namespace gine

using namespace gine;

extern "C" int gine_batch_fill_permuted(const float* x, const float* ens, const float* y,
                                        const int64_t* idx, const int64_t* perm_t,
                                        const int32_t* perm_n, uint64_t col_mask, int64_t T,
                                        int32_t N, int32_t M, int32_t F, int32_t B, float* out_x,
                                        float* out_ens, float* out_y, void* stream) {
  if (T < 0 || B < 0 || N < 1 || M < 1 || F < 1) return GINE_ERR_INVALID;
  if (F > kMaxFeatures) return GINE_ERR_DIM;
  if (B == 0) return GINE_OK;
  if (T < 1) return GINE_ERR_INVALID;  // slots, and no sample to fill them from
  if (!x || !ens || !y || !idx || !out_x || !out_ens || !out_y) return GINE_ERR_INVALID;
  if (F < kMaxFeatures && (col_mask >> F) != 0ull) return GINE_ERR_INVALID;
  if (col_mask != 0ull && !perm_t && !perm_n) return GINE_ERR_INVALID;
  // a row is walked with an int, a pass at a time
  if ((int64_t)M * F > 0x7fffffff - kWave * kUnroll) return GINE_ERR_TOO_LARGE;
  const int64_t tiles = ceil_div((int64_t)N, kWaves);
  if (tiles * B > 0x7fffffff) return GINE_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_batch_fill_permuted, dim3((unsigned)(tiles * B)), dim3(kThreads), 0,
                     as_stream(stream), x, ens, y, idx, perm_t, perm_n, col_mask, (int)N, (int)M,
                     (int)F, (unsigned)tiles, out_x, out_ens, out_y);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}
