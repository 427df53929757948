// The wave roles and LDS layouts shared by the fused GINE layer forwards: gine_mpmlp.hip
// (gine_mp_fwd_mlp1, gine_mp_fwd_layer) and gine_mpeval.hip (gine_mp_fwd_layer_eval).
// See gine_mpmlp.hip for the design; everything here is per translation unit.
#pragma once
#include "gine_common.hpp"
#include "gine_bnacc.hpp"
#include "gine_edge.hpp"
#include "gine_bf16x3.hpp"
#include "gine_headrow.hpp"
#include "gine_mlpsrc.hpp"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>

namespace gine {
namespace {

constexpr int kD = 128, kD4 = kD / 4;
constexpr int kTileRows = 32;
constexpr int kLD = kD + 4;                 // padded z-tile / W row (floats)
constexpr int kKS = kD / 2;                 // MFMA k-steps per lane half
#ifndef GINE_FUSED_GATHER_WAVES
#define GINE_FUSED_GATHER_WAVES 8
#endif
constexpr int kMatThreads = 256;                                 // waves 0-3
constexpr int kGatherWaves = GINE_FUSED_GATHER_WAVES;            // waves 4-...
constexpr int kThreads = kMatThreads + kWave * kGatherWaves;
constexpr int kHalves = 2 * kGatherWaves;                        // gather half-waves
constexpr int kRowsPerHalf = kTileRows / kHalves;
static_assert(kRowsPerHalf % 2 == 0, "rows are gathered in pairs");
constexpr int kSlots = GINE_MP_FUSED_MAX_DEGREE;
constexpr int kU = 11;  // neighbour rows in flight per row, 2 rows per round (k=10: one)
constexpr int kTLD = 36;                    // per-wave transposition tile row (floats)
constexpr uint32_t kRowBytes = kD * 4;
// experiment builds only (make variant VDEFS=-DGINE_FUSED_DBG=n): 1 = no neighbour loads,
// 2 = no MFMA chain -- the two roles timed without each other
#ifndef GINE_FUSED_DBG
#define GINE_FUSED_DBG 0
#endif

typedef float floatx16 __attribute__((ext_vector_type(16)));

#ifdef GINE_LAYER_PROFILE
// Debug build only (make layerprof): thread 0 of every workgroup of the one-launch layer
// forward stamps s_memtime at its phase boundaries (tools/layer_prof.py):
// 0 entry, 1 matrix role done, 2 phase A done (block), 3 barrier arrival, 4 grid barrier
// passed, 5 BatchNorm finish + W2 fragments done, 6 r = relu(bn(a1)) done, 7 last Linear2
// chain done.
// Phase A detail: 8 W1 planes ready, 9 / 11 tile 1 / 2 chain done, 10 / 12 tile 1 / 2
// epilogue done, 13 statistics in the accumulator (matrix role, thread 0); 14 / 15 tile 1 /
// 2 gathered (gather role, thread 256).
// 16-19: s_memrealtime (the 100 MHz clock every XCD shares) at entry, barrier arrival,
// barrier release and the end, for the arrival skew across workgroups.
// 20 / 21: tile 1 / 2's planes in LDS (matrix role); 22 / 23: the window form's tile 1 / 2
// staged (gather role, thread 256, after G).
__device__ long long g_layer_prof[1024][24];
#define LAYER_RT(i)                                                              \
  do {                                                                           \
    if (threadIdx.x == 0 && blockIdx.x < 1024)                                   \
      g_layer_prof[blockIdx.x][i] = (long long)__builtin_amdgcn_s_memrealtime(); \
  } while (0)
#define LAYER_MARK_T(t, i)                                                       \
  do {                                                                           \
    if (threadIdx.x == (t) && blockIdx.x < 1024)                                 \
      g_layer_prof[blockIdx.x][i] = (long long)__builtin_amdgcn_s_memtime();    \
  } while (0)
#else
#define LAYER_MARK_T(t, i) do {} while (0)
#define LAYER_RT(i) do {} while (0)
#endif
#define LAYER_MARK(i) LAYER_MARK_T(0, i)

// The eval form calls the roles once per round of its tile loop.  Everything a role derives
// from the thread index is the same in every round, so the compiler hoists it out of that
// loop -- dozens of staging addresses live across the whole round, spilled to scratch.  The
// thread index taken through this in each round keeps those computations inside it.
__device__ __forceinline__ int per_round(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

struct TileSeq {
  int first, end, step;
  __device__ int count() const { return first < end ? (end - first + step - 1) / step : 0; }
  __device__ int at(int k) const { return first + k * step; }
};
// The row-tile GEMM's tile -> workgroup assignment (gine_mlp.hip xcd_tile_range): the tiles
// of one XCD form a contiguous range, its workgroups stride it.
__device__ __forceinline__ TileSeq tile_seq(int num_tiles, int vb, int nb) {
  const int xcd = vb % kNumXcd, pos = vb / kNumXcd;
  const int here = nb / kNumXcd + (xcd < nb % kNumXcd ? 1 : 0);
  const int span = (num_tiles + kNumXcd - 1) / kNumXcd;
  const int b = xcd * span;
  return TileSeq{b + pos, min(num_tiles, b + span), here};
}

// Edge lists run two stages ahead of their use, with nothing waiting on a load until the
// tile that consumes it: rowptr of tile k+2 and the edge slots of tile k+1 are issued while
// tile k is gathered.  Lane t keeps slot t of each of its half-wave's 4 rows; the selects
// that depend on loaded values (slot past the in-degree -> the row itself, a valid index)
// run when the slots are written to LDS, not right behind the loads.
struct RowptrStage {
  int32_t beg[kRowsPerHalf], end[kRowsPerHalf];
};
struct EdgeStage {
  int32_t nbr[kRowsPerHalf];
  float attr[kRowsPerHalf];
  int cnt[kRowsPerHalf];
};

// acc += relu(r + lin(a)) when ok (else + 0: acc is never -0, so adding +0 is exact)
template <bool FMA>
__device__ __forceinline__ void edge_acc(f4v& acc, f4v r, float a, f4v w, f4v b, bool ok) {
  const f2v lo = relu2(r.xy + edge_lin2<FMA>(a, w.xy, b.xy));
  const f2v hi = relu2(r.zw + edge_lin2<FMA>(a, w.zw, b.zw));
  const f2v zero = {0.f, 0.f};
  acc.xy = acc.xy + (ok ? lo : zero);
  acc.zw = acc.zw + (ok ? hi : zero);
}

struct FusedArgs {
  const float* x;
  const int32_t* rowptr;
  const int32_t* nbr;
  const float* attr;
  const float* lin_w;
  const float* lin_b;
  const float* eps;
  const float* W1;
  const float* b1;
  float* z;
  float* a1;
  double* partials;      // NULL: bnacc only
  long long* bnacc;      // NULL: partials only (gine_bnacc.hpp)
  int N, num_tiles;
};

struct FusedLds {
  // W1 staging (prologue only), then the matrix waves' transposition tiles and, at the end,
  // their statistics scratch (disjoint regions)
  float w[kD * kLD];
  float z[2][kTileRows * kLD];  // z tiles, gather -> matrix, double-buffered
  int32_t nbr[kHalves][kRowsPerHalf][kSlots];
  float attr[kHalves][kRowsPerHalf][kSlots];
};
static_assert(4 * 32 * kTLD * 4 + 2 * 8 * kD * 8 <= kD * kLD * 4, "scratch fits in w");

// The one-launch layer's phase A hands each z tile from the gather waves to the matrix waves
// as split-bf16 planes (hi | mid | lo, gine_bf16x3.hpp split2), split ONCE by the producers:
// in the pair form every matrix wave splits the whole 32x128 A tile inside its chain (4x the
// work, on the SIMDs the gather waves issue from: the 4 matrix waves' in-loop split is ~450
// VALU instructions each per tile against the gather waves' ~570).  The fp32 z tile is not
// kept in LDS (the rare non-finite redo reads z back from HBM): tile it's planes live in the
// z region (it even) or in the w region past the matrix waves' transposition tiles and
// statistics scratch (it odd; W1's staging there is over by then).
constexpr int kPS = kD + 8;  // split-plane row stride (bf16): conflict-free 16-byte reads
constexpr int kPlaneBytes = 3 * kTileRows * kPS * 2;
constexpr int kPlaneOffW = 4 * 32 * kTLD * 4 + 2 * 8 * kD * 8;  // bytes into w
static_assert(kPlaneOffW + kPlaneBytes <= kD * kLD * 4, "odd tiles' planes fit in w");
static_assert(kPlaneBytes <= 2 * kTileRows * kLD * 4, "even tiles' planes fit in the z tiles");
__device__ __forceinline__ uint16_t* tile_planes(FusedLds& L, int it) {
  return (it & 1) ? reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(L.w) + kPlaneOffW)
                  : reinterpret_cast<uint16_t*>(&L.z[0][0]);
}

// Matrix role (waves 0-3).  Barriers: 1 + (nt + 1), as the gather role.
// LAYER (gine_mp_fwd_layer): every a1 tile is also kept in LDS (a1k[it], row-major, at most
// kLayerTiles of them) for the second half of the layer, and the producer's phase word is
// left to the caller.
// EVAL (gine_mp_fwd_layer_eval): the pair form's chain on the fp32 z tile (its non-finite redo
// reads the tile in LDS, z is not in memory), a1 goes to a1k only, and there are no BatchNorm
// statistics: nothing is written to memory.
template <bool LAYER = false, bool EVAL = false>
__device__ __forceinline__ void matrix_role(const FusedArgs& A, FusedLds& L, const TileSeq& ts,
                                            int nt, float* a1k = nullptr) {
  static_assert(!(LAYER && EVAL), "the eval form reads fp32 z tiles, not split planes");
  int tid_ = threadIdx.x;
  if constexpr (EVAL) tid_ = per_round(tid_);
  const int tid = tid_;
  const int wave = tid / kWave, lane = tid % kWave;
  const int h = lane >> 5, c32 = lane & 31;
  const int cq = lane & 7, grp = lane >> 3;  // transposed epilogue: 4-column chunk, row group
  {
    const float4* w4 = reinterpret_cast<const float4*>(A.W1);
    float4 wt[kD * kD4 / kMatThreads];
#pragma unroll
    for (int j = 0; j < kD * kD4 / kMatThreads; ++j) wt[j] = w4[tid + kMatThreads * j];
#pragma unroll
    for (int j = 0; j < kD * kD4 / kMatThreads; ++j) {
      const int idx = tid + kMatThreads * j;
      *reinterpret_cast<float4*>(&L.w[(idx / kD4) * kLD + 4 * (idx % kD4)]) = wt[j];
    }
  }
  const float4 bias4 = *reinterpret_cast<const float4*>(A.b1 + 32 * wave + 4 * cq);
  __syncthreads();
  // W1^T fragments: B[k][j] = W1[j][k], lane half h takes k in [h*64, h*64+64)
  float bf[kKS];
  {
    const float* wr = &L.w[(32 * wave + c32) * kLD + h * kKS];
#pragma unroll
    for (int q = 0; q < kKS / 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(&wr[4 * q]);
      bf[4 * q] = v.x;
      bf[4 * q + 1] = v.y;
      bf[4 * q + 2] = v.z;
      bf[4 * q + 3] = v.w;
    }
  }
  BPlanes<kKS> bp;
  if constexpr (GINE_GEMM_BF16X3) bp.from(bf);
  __syncthreads();  // (iteration 0: the gather role stages the first tile)
  if constexpr (LAYER) LAYER_MARK(8);
  // per-column BatchNorm sums of this lane's (row group, 4 columns), kept in the statistics
  // scratch of LDS between tiles rather than in 16 VGPRs beside the B planes (the lane's own
  // slots, brought into registers for each tile's rows: the same sequential order, the same
  // bits); W1's staging is over
  double* sr = reinterpret_cast<double*>(&L.w[4 * 32 * kTLD]);  // [2][8][kD]
  if constexpr (!EVAL) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = 32 * wave + 4 * cq + k;
      sr[(0 * 8 + grp) * kD + c] = 0.0;
      sr[(1 * 8 + grp) * kD + c] = 0.0;
    }
  }
  const float bb[4] = {bias4.x, bias4.y, bias4.z, bias4.w};
  float* tt = &L.w[wave * 32 * kTLD];
  for (int it = 1; it <= nt; ++it) {
    const int T = ts.at(it - 1);
    if constexpr (LAYER) {
      if (it <= 2) LAYER_MARK(19 + it);  // (profile builds) tile it's z is in LDS
    }
    const float* arow = &L.z[(it - 1) & 1][c32 * kLD + h * kKS];
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    if constexpr (LAYER) {  // the same chain from the gather waves' split planes
      static_assert(GINE_GEMM_BF16X3, "the layer forward reads split planes");
      const uint16_t* pa = tile_planes(L, it - 1) + c32 * kPS + h * kKS;
      auto frag = [&](int s8) {
        Bf16x3 a;
        a.h = *reinterpret_cast<const bf16x8_t*>(pa + 8 * s8);
        a.m = *reinterpret_cast<const bf16x8_t*>(pa + kTileRows * kPS + 8 * s8);
        a.l = *reinterpret_cast<const bf16x8_t*>(pa + 2 * kTileRows * kPS + 8 * s8);
        return a;
      };
      // one fragment in flight beside the current block's six MFMAs (192 cycles hide the LDS
      // latency): with all eight hoisted the matrix waves' B planes (96 VGPRs) spilled
      Bf16x3 a = frag(0);
#pragma unroll
      for (int s8 = 0; s8 < (GINE_FUSED_DBG == 2 ? 1 : kKS / 8); ++s8) {
        Bf16x3 an = a;
        if (s8 + 1 < kKS / 8) an = frag(s8 + 1);
        acc = mfma_bf16x3(a, bp.f[s8], acc);
        __builtin_amdgcn_sched_barrier(0);
        a = an;
      }
      if (wave_any_nan(acc)) {  // non-finite operands: the fp32 chain on z read back from HBM
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");  // the gather waves' z stores
        const int64_t zr = min((int64_t)T * kTileRows + c32, (int64_t)A.N - 1);
        acc = mfma_f32_row_mem<kKS>(A.z + zr * kD + h * kKS,
                                    A.W1 + (size_t)(32 * wave + c32) * kD + h * kKS, 1, acc);
      }
    } else if constexpr (GINE_GEMM_BF16X3) {  // the row-tile GEMM's split-bf16 chain (gine_mlp.hip)
#pragma unroll
      for (int s = 0; s < (GINE_FUSED_DBG == 2 ? 1 : kKS / 8); ++s) {
        const float4 a0 = *reinterpret_cast<const float4*>(&arow[8 * s]);
        const float4 a1 = *reinterpret_cast<const float4*>(&arow[8 * s + 4]);
        acc = mfma_bf16x3(split8(a0, a1), bp.f[s], acc);
      }
      if (wave_any_nan(acc)) {  // non-finite operands: the fp32 chain (gine_bf16x3.hpp)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        acc = mfma_f32_row_mem<kKS>(arow, A.W1 + (size_t)(32 * wave + c32) * kD + h * kKS, 1,
                                    acc);
      }
    } else {
#pragma unroll
      for (int q = 0; q < (GINE_FUSED_DBG == 2 ? 1 : kKS / 4); ++q) {
        const float4 a4 = *reinterpret_cast<const float4*>(&arow[4 * q]);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, bf[4 * q], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, bf[4 * q + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, bf[4 * q + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, bf[4 * q + 3], acc, 0, 0, 0);
      }
    }
#ifdef GINE_LAYER_PROFILE
    if constexpr (LAYER) {
      if (it <= 2 && acc[0] == 1.2345e-30f) tt[0] = 0.f;  // the stamp waits for the chain
      if (it <= 2) LAYER_MARK(7 + 2 * it);
    }
#endif
    // this wave's 32x32 block -> row-major through its own LDS tile
#pragma unroll
    for (int r = 0; r < 16; ++r) tt[((r & 3) + 8 * (r >> 2) + 4 * h) * kTLD + c32] = acc[r];
    __builtin_amdgcn_wave_barrier();
    // the running sums come into registers for the tile's 4 rows (same order, same bits)
    [[maybe_unused]] double st1[4], st2[4];
    if constexpr (!EVAL) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        st1[k] = sr[(0 * 8 + grp) * kD + 32 * wave + 4 * cq + k];
        st2[k] = sr[(1 * 8 + grp) * kD + 32 * wave + 4 * cq + k];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = grp + 8 * i;
      const int64_t n = (int64_t)T * kTileRows + row;
      const float4 v = *reinterpret_cast<const float4*>(&tt[row * kTLD + 4 * cq]);
      if (n >= A.N) continue;
      const float vv[4] = {v.x, v.y, v.z, v.w};
      float o4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o4[k] = vv[k] + bb[k];
        if constexpr (!EVAL) {
          st1[k] += (double)o4[k];
          st2[k] += (double)o4[k] * (double)o4[k];
        }
      }
      if constexpr (!EVAL)
        *reinterpret_cast<float4*>(A.a1 + n * kD + 32 * wave + 4 * cq) =
            make_float4(o4[0], o4[1], o4[2], o4[3]);
      if constexpr (LAYER || EVAL)
        *reinterpret_cast<float4*>(&a1k[(it - 1) * kTileRows * kLD + row * kLD + 32 * wave +
                                        4 * cq]) = make_float4(o4[0], o4[1], o4[2], o4[3]);
    }
    if constexpr (!EVAL) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        sr[(0 * 8 + grp) * kD + 32 * wave + 4 * cq + k] = st1[k];
        sr[(1 * 8 + grp) * kD + 32 * wave + 4 * cq + k] = st2[k];
      }
    }
    __builtin_amdgcn_wave_barrier();  // the next tile's transposition writes come after
    if constexpr (LAYER) {
      if (it <= 2) LAYER_MARK(8 + 2 * it);
    }
    __syncthreads();
  }
  if constexpr (EVAL) return;  // no statistics
  // per-column partials: the 8 row groups added in fixed order (row-tile GEMM order)
  __builtin_amdgcn_wave_barrier();
  const int which = lane >> 5, cc = 32 * wave + (lane & 31);
  double s = 0.0;
#pragma unroll
  for (int g = 0; g < 8; ++g) s += sr[(which * 8 + g) * kD + cc];
  if (A.partials) A.partials[(size_t)blockIdx.x * 2 * kD + which * kD + cc] = s;
  if constexpr (LAYER) {
    bnacc_add<false>(A.bnacc, 2 * kD, which * kD + cc, s);
    // the atomics are performed before this workgroup arrives at the grid barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    LAYER_MARK(13);
  } else if (A.bnacc) {
    bnacc_add(A.bnacc, 2 * kD, which * kD + cc, s);
  }
}

// Gather role (waves 4-11).  Barriers: 1 + (nt + 1), as the matrix role; without LAST_SYNC
// the caller runs the last one (after work of its own beside the matrix role's last tile).
// PLANES (the one-launch layer): the tile goes to the matrix waves as split-bf16 planes
// (tile_planes) instead of an fp32 LDS tile.
// STORE_Z = false (gine_mp_fwd_layer_eval): z goes to the LDS tile only, not to memory.
template <bool FMA, bool LAST_SYNC = true, bool PLANES = false, bool STORE_Z = true>
__device__ __forceinline__ void gather_role(const FusedArgs& A, FusedLds& L, const TileSeq& ts,
                                            int nt) {
  int p_;
  if constexpr (STORE_Z) p_ = threadIdx.x - kMatThreads;
  else p_ = per_round((int)threadIdx.x) - kMatThreads;  // (the eval form)
  const int p = p_;
  const int hw = p >> 5, t = p & 31;
  const int N = A.N;
  const uint32_t qb = (uint32_t)t * 16u;
  const char* xb = reinterpret_cast<const char*>(A.x);
  RowptrStage rp;
  EdgeStage es;
#pragma unroll
  for (int i = 0; i < kRowsPerHalf; ++i) {
    rp.beg[i] = rp.end[i] = 0;
    es.nbr[i] = 0;
    es.attr[i] = 0.f;
    es.cnt[i] = 0;
  }
  auto row_of = [&](int T, int i) { return T * kTileRows + hw + kHalves * i; };
  auto clamp_row = [&](int n) { return n < N ? n : N - 1; };
  auto issue_rowptr = [&](int T) {  // -> rp (no wait)
#pragma unroll
    for (int i = 0; i < kRowsPerHalf; ++i) {
      const int n = clamp_row(row_of(T, i));
      rp.beg[i] = A.rowptr[n];
      rp.end[i] = A.rowptr[n + 1];
    }
  };
  auto issue_edges = [&](int T) {  // rp (of tile T, arrived) -> es (no wait)
#pragma unroll
    for (int i = 0; i < kRowsPerHalf; ++i) {
      const int cnt = row_of(T, i) < N ? min(rp.end[i] - rp.beg[i], kSlots) : 0;
      const int e = cnt > 0 ? rp.beg[i] + min(t, cnt - 1) : 0;  // always a valid index
      es.nbr[i] = A.nbr[e];
      es.attr[i] = A.attr[e];
      es.cnt[i] = cnt;
    }
  };
  const f4v lw = ld_f4v(reinterpret_cast<const char*>(A.lin_w), qb);
  const f4v lb = ld_f4v(reinterpret_cast<const char*>(A.lin_b), qb);
  const float ope = 1.0f + A.eps[0];
  if (nt > 0) {
    issue_rowptr(ts.at(0));
    issue_edges(ts.at(0));
  }
  if (nt > 1) issue_rowptr(ts.at(1));
  __syncthreads();

  for (int it = 0; it < nt; ++it) {
    const int T = ts.at(it);
    float* sz = L.z[it & 1];
    int cnt[kRowsPerHalf];
#pragma unroll
    for (int i = 0; i < kRowsPerHalf; ++i) {
      L.nbr[hw][i][t] = t < es.cnt[i] ? es.nbr[i] : clamp_row(row_of(T, i));
      L.attr[hw][i][t] = es.attr[i];
      cnt[i] = es.cnt[i];
    }
    __builtin_amdgcn_wave_barrier();
    if (it + 1 < nt) issue_edges(ts.at(it + 1));
    if (it + 2 < nt) issue_rowptr(ts.at(it + 2));
    f4v self[kRowsPerHalf], acc[kRowsPerHalf];
#pragma unroll
    for (int i = 0; i < kRowsPerHalf; ++i) {
      self[i] = ld_f4v(xb, (uint32_t)clamp_row(row_of(T, i)) * kRowBytes + qb);
      acc[i] = f4v_zero();
    }
#pragma unroll
    for (int pr = 0; pr < kRowsPerHalf; pr += 2) {
      const int m = GINE_FUSED_DBG == 1 ? 0 : max(cnt[pr], cnt[pr + 1]);
      for (int j0 = 0; j0 < m; j0 += kU) {
        f4v r0[kU], r1[kU];
        float a0[kU], a1v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = min(j0 + u, kSlots - 1);
          r0[u] = ld_f4v(xb, (uint32_t)L.nbr[hw][pr][j] * kRowBytes + qb);
          r1[u] = ld_f4v(xb, (uint32_t)L.nbr[hw][pr + 1][j] * kRowBytes + qb);
          a0[u] = L.attr[hw][pr][j];
          a1v[u] = L.attr[hw][pr + 1][j];
        }
        // (an unmasked copy of this loop for full batches -- the common case -- spilled: 292 B of
        // scratch in k_mp_fwd_mlp1, which then ran 34 instead of 14 us; profiles/r05_s15)
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          edge_acc<FMA>(acc[pr], r0[u], a0[u], lw, lb, j0 + u < cnt[pr]);
          edge_acc<FMA>(acc[pr + 1], r1[u], a1v[u], lw, lb, j0 + u < cnt[pr + 1]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kRowsPerHalf; ++i) {
      const int r = hw + kHalves * i;
      const int64_t n = (int64_t)T * kTileRows + r;
      const f4v zv = add_scaled(acc[i], ope, self[i]);
      if constexpr (PLANES) {
        uint32_t h0, m0, l0, h1, m1, l1;
        split2(zv.x, zv.y, h0, m0, l0);
        split2(zv.z, zv.w, h1, m1, l1);
        uint16_t* pl = tile_planes(L, it) + r * kPS + 4 * t;
        *reinterpret_cast<uint2*>(pl) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(pl + kTileRows * kPS) = make_uint2(m0, m1);
        *reinterpret_cast<uint2*>(pl + 2 * kTileRows * kPS) = make_uint2(l0, l1);
      } else {
        *reinterpret_cast<f4v*>(&sz[r * kLD + 4 * t]) = zv;
      }
      if constexpr (STORE_Z)
        if (n < N) *reinterpret_cast<f4v*>(A.z + n * kD + 4 * t) = zv;
    }
    if (it < 2) LAYER_MARK_T(kMatThreads, 14 + it);
    __builtin_amdgcn_wave_barrier();  // edge-list reads done before the next tile's writes
    __syncthreads();
  }
  if constexpr (LAST_SYNC) __syncthreads();  // (iteration nt: the matrix role multiplies the last tile)
}

// The one-launch layer forms (gine_mpmlp.hip k_mp_fwd_layer, gine_mpeval.hip).
constexpr int kLayerTiles = 2;  // a1 tiles a workgroup keeps in LDS
static_assert(kLayerTiles * 3 * kTileRows * kPS * 2 <= kD * kLD * 4, "planes fit in w");

// W2 in flight in the gather waves' registers: 8 float4 per thread (element idx = t + n*j,
// row idx / kD4, column chunk idx % kD4), staged into the padded LDS image.
template <int PER>
struct W2Regs {
  static_assert(PER == 8, "eight float4 per gather thread");
  float4 v0, v1, v2, v3, v4, v5, v6, v7;
  __device__ __forceinline__ void load(const float4* __restrict__ w4, int t, int n) {
    v0 = w4[t]; v1 = w4[t + n]; v2 = w4[t + 2 * n]; v3 = w4[t + 3 * n];
    v4 = w4[t + 4 * n]; v5 = w4[t + 5 * n]; v6 = w4[t + 6 * n]; v7 = w4[t + 7 * n];
  }
  __device__ __forceinline__ void put(float* w, int idx, float4 v) const {
    *reinterpret_cast<float4*>(&w[(idx / kD4) * kLD + 4 * (idx % kD4)]) = v;
  }
  __device__ __forceinline__ void store(float* w, int t, int n) const {
    put(w, t, v0); put(w, t + n, v1); put(w, t + 2 * n, v2); put(w, t + 3 * n, v3);
    put(w, t + 4 * n, v4); put(w, t + 5 * n, v5); put(w, t + 6 * n, v6); put(w, t + 7 * n, v7);
  }
};

struct LayerArgs {
  const float* W2;
  const float* b2;
  float* y;
  uint8_t* mask;
  BnFwdParams q;
  const int2* win;     // WIN: per 32-row tile (first window row, window rows)
  int win_rows;        // WIN: max window rows over the tiles (the dummy row's index)
  int win_slots;       // WIN: slots per row of the padded slot table (lw_slots)
  gine_layer_head hd;  // the output head folded into the epilogue (hk > 0)
  int hk;              // head outputs per node (2..5), 0: no head
};

// The output head's LDS block (gine_layer_head): weights [kMaxK][kD] | bias [8] | raw outputs
// of the workgroup's tiles [kLayerTiles][32][K] (PostProcess and the stores after the tile
// loop, one element per thread) | valid-target counts per part [GINE_COUNT_PARTS] (uint32)
constexpr int kHB = head::kMaxK * kD;
constexpr int kHR = kHB + 8;
constexpr int kHRTile = kTileRows * head::kMaxK;
constexpr int kHC = kHR + kLayerTiles * kHRTile;
constexpr int kHeadFloats = kHC + GINE_COUNT_PARTS;

struct LayerLds {
  FusedLds f;
  float a1k[kLayerTiles][kTileRows * kLD];
  float bn[2 * kD];  // alpha | shift
  double tot[2 * kD];
  float hd[kHeadFloats];  // the output head (gine_layer_head)
  int barrier_failed;  // this workgroup's grid barrier timed out (gine_bnacc.hpp)
};

// Element e of the head's outputs of 32-row tile T from its raw values in LDS (rt: [32][K],
// written by the epilogue's half-waves): raw stored and PostProcess applied once per element
// after the tile loop (coalesced rows of raw / pred), instead of on the K lanes of every row's
// half-wave inside it.
__device__ __forceinline__ void head_finish(const LayerArgs& B, const float* rt, int T, int N,
                                            int e) {
  const int64_t base = (int64_t)T * kTileRows * B.hk;
  if (base + e < (int64_t)N * B.hk) {
    const float v = rt[e];
    B.hd.raw[base + e] = v;
    B.hd.pred[base + e] = head::post(head::role_of(B.hd.kind, e % B.hk), v);
  }
}

}  // namespace
}  // namespace gine
