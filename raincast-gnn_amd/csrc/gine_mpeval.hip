// GINE layer forward in eval mode in one launch (gine_mp_fwd_layer_eval, D = 128), and the
// same at any in-degree (gine_mp_fwd_layer_eval_deep).
#include "gine_mpmlp.hpp"

namespace gine {
namespace {

// Phase B below (relu planes, Linear2's chain and redo, the row epilogue and the head's row
// reduction) restates gine_mpmlp.hip k_mp_fwd_layer's, from the same primitives, and must be
// kept in step with it.  Sharing the pieces as functions of gine_mpmlp.hpp was tried for the
// relu-plane store and for the head's row reduction, each alone: either one changes the
// instruction streams of all twelve k_mp_fwd_layer instantiations (a handful of instructions,
// another schedule), which the training kernels' unchanged-disassembly rule does not allow.
//
// Phase B's LDS (k_mp_fwd_layer's, non-window form): W2's image, then the relu planes, over
// W1's image; the output tiles over the z tiles.
__device__ __forceinline__ uint16_t* relu_plane_base(LayerLds& L) {
  return reinterpret_cast<uint16_t*>(L.f.w);  // [kLayerTiles][3][kTileRows * kPS]
}
__device__ __forceinline__ float* out_tile(LayerLds& L, int k) {
  return &L.f.z[0][0] + (k & 1) * kTileRows * kLD;
}

// r = relu(bn(a1)) of the round's tiles as split-bf16 planes, this thread's share (all 12
// waves; rows past N are zero) -- k_mp_fwd_layer's pass, alpha | shift from L.bn.
__device__ __forceinline__ void relu_planes(LayerLds& L, const TileSeq& rs, int nt, int N,
                                            int tidr) {
  uint16_t* rp = relu_plane_base(L);
#pragma unroll
  for (int j = 0; j < (kLayerTiles * kTileRows * kD4 + kThreads - 1) / kThreads; ++j) {
    const int e = tidr + kThreads * j;
    if (e >= nt * kTileRows * kD4) break;
    const int k = e / (kTileRows * kD4), r = (e / kD4) % kTileRows, q4 = e % kD4;
    float4 v = *reinterpret_cast<const float4*>(&L.a1k[k][r * kLD + 4 * q4]);
    const float4 al = *reinterpret_cast<const float4*>(&L.bn[4 * q4]);
    const float4 sh = *reinterpret_cast<const float4*>(&L.bn[kD + 4 * q4]);
    v = make_float4(relu_nan(bn_apply(v.x, al.x, sh.x)), relu_nan(bn_apply(v.y, al.y, sh.y)),
                    relu_nan(bn_apply(v.z, al.z, sh.z)), relu_nan(bn_apply(v.w, al.w, sh.w)));
    if ((int64_t)rs.at(k) * kTileRows + r >= N) v = f4_zero();
    uint32_t h0, m0, l0, h1, m1, l1;
    split2(v.x, v.y, h0, m0, l0);
    split2(v.z, v.w, h1, m1, l1);
    uint16_t* pl = rp + k * 3 * kTileRows * kPS + r * kPS + 4 * q4;
    *reinterpret_cast<uint2*>(pl) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(pl + kTileRows * kPS) = make_uint2(m0, m1);
    *reinterpret_cast<uint2*>(pl + 2 * kTileRows * kPS) = make_uint2(l0, l1);
  }
}

// One round of the matrix waves.  Barriers: (nt + 2) + 4 + nt + (head ? 1 : 0) + 1, as
// eval_round_gather.
__device__ __forceinline__ void eval_round_matrix(const FusedArgs& A, const LayerArgs& B,
                                                  LayerLds& L, const TileSeq& rs, int nt,
                                                  int wave) {
  static_assert(GINE_GEMM_BF16X3, "the layer forward's second half reads split planes");
  matrix_role<false, true>(A, L.f, rs, nt, &L.a1k[0][0]);
  __syncthreads();  // phase A's LDS use is over (L.f.w is free)
  const int tidr = per_round(threadIdx.x);
  const int lane = tidr % kWave;
  const int h = lane >> 5, c32 = lane & 31;
  const int col = 32 * wave + c32;
  __syncthreads();  // W2 staged by the gather waves
  BPlanes<kKS> bp;
  {
    float bf[kKS];
    const float* wr = &L.f.w[col * kLD + h * kKS];
#pragma unroll
    for (int q = 0; q < kKS / 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(&wr[4 * q]);
      bf[4 * q] = v.x;
      bf[4 * q + 1] = v.y;
      bf[4 * q + 2] = v.z;
      bf[4 * q + 3] = v.w;
    }
    bp.from(bf);
  }
  __syncthreads();  // W2's fragments read: the w region takes the relu planes
  relu_planes(L, rs, nt, A.N, tidr);
  __syncthreads();
  const uint16_t* rp = relu_plane_base(L);
  for (int k = 0; k < nt; ++k) {  // Linear2 chain of tile k (the row GEMM's chain and k order)
    float* sO = out_tile(L, k);
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const uint16_t* pa = rp + k * 3 * kTileRows * kPS + c32 * kPS + h * kKS;
#pragma unroll
    for (int s8 = 0; s8 < kKS / 8; ++s8) {
      Bf16x3 a;
      a.h = *reinterpret_cast<const bf16x8_t*>(pa + 8 * s8);
      a.m = *reinterpret_cast<const bf16x8_t*>(pa + kTileRows * kPS + 8 * s8);
      a.l = *reinterpret_cast<const bf16x8_t*>(pa + 2 * kTileRows * kPS + 8 * s8);
      acc = mfma_bf16x3(a, bp.f[s8], acc);
    }
    if (wave_any_nan(acc)) {  // the fp32 chain, r recomputed from a1 (mfma_f32_row_mem's order)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      const bool live = (int64_t)rs.at(k) * kTileRows + c32 < A.N;
      const float* arow = &L.a1k[k][c32 * kLD + h * kKS];
      const float* wp = B.W2 + (size_t)col * kD + h * kKS;
      auto rv = [&](int kk) -> float {
        const int c = h * kKS + kk;
        return live ? relu_nan(bn_apply(arow[kk], L.bn[c], L.bn[kD + c])) : 0.f;
      };
#pragma unroll 1
      for (int q = 0; q < kKS / 4; ++q) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(rv(4 * q), wp[4 * q], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(rv(4 * q + 1), wp[4 * q + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(rv(4 * q + 2), wp[4 * q + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(rv(4 * q + 3), wp[4 * q + 3], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sO[((r & 3) + 8 * (r >> 2) + 4 * h) * kLD + col] = acc[r];
    __syncthreads();  // output tile k in LDS
  }
  if (B.hk) __syncthreads();  // (the gather waves' head_finish)
  __syncthreads();            // the round's LDS use is over
}

// The gather role at any in-degree (gine_mp_fwd_layer_eval_deep): gather_role<FMA, false,
// false, false> of gine_mpmlp.hpp restated (sharing it through a flag would touch the
// training kernels' code), with the row's edge list walked in chunks of kSlots through the
// same nbr / attr tables.  Chunk 0 keeps the two-stage prefetch; a further chunk is loaded by
// the half-wave that owns the rows once the chunk before it is consumed (its own table rows:
// the wave's program order is the only synchronisation, as for chunk 0).  A pair's shorter row
// has count 0 in its extra chunks: wholly masked, +0 added, so every row sees acc = 0, its
// edges in CSR order, then add_scaled -- the bits of any other form.  Every address is valid
// for every lane: an edge index is clamped to the row's last edge (0 for an empty row), a
// masked slot holds the row itself, a row past N is N - 1.
// Barriers: 1 + nt (the caller runs the last one), as gather_role without LAST_SYNC.
// Neighbour rows in flight per row of the pair: a 32-slot chunk is four full steps of eight
// (gather_role's eleven, sized for k = 10 plus the self loop, would be 11 + 11 + 10 and, with
// the rows' first edge and in-degree kept for the further chunks, spills six registers).
constexpr int kUD = 8;
static_assert(kSlots % kUD == 0, "a full chunk is a whole number of steps");
template <bool FMA>
__device__ __forceinline__ void gather_role_deep(const FusedArgs& A, FusedLds& L,
                                                 const TileSeq& ts, int nt) {
  static_assert(kRowsPerHalf == 2, "one pair of rows per half-wave");
  const int p = per_round((int)threadIdx.x) - kMatThreads;
  const int hw = p >> 5, t = p & 31;
  const int N = A.N;
  const uint32_t qb = (uint32_t)t * 16u;
  const char* xb = reinterpret_cast<const char*>(A.x);
  RowptrStage rp;
  EdgeStage es;
  int32_t ebeg[kRowsPerHalf];  // the staged tile's first edge and whole in-degree per row
  int edeg[kRowsPerHalf];
#pragma unroll
  for (int i = 0; i < kRowsPerHalf; ++i) {
    rp.beg[i] = rp.end[i] = 0;
    es.nbr[i] = 0;
    es.attr[i] = 0.f;
    es.cnt[i] = 0;
    ebeg[i] = 0;
    edeg[i] = 0;
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
  auto issue_edges = [&](int T) {  // rp (of tile T, arrived) -> es: chunk 0 (no wait)
#pragma unroll
    for (int i = 0; i < kRowsPerHalf; ++i) {
      const int deg = row_of(T, i) < N ? max(rp.end[i] - rp.beg[i], 0) : 0;
      const int cnt = min(deg, kSlots);
      const int e = cnt > 0 ? rp.beg[i] + min(t, cnt - 1) : 0;  // always a valid index
      es.nbr[i] = A.nbr[e];
      es.attr[i] = A.attr[e];
      es.cnt[i] = cnt;
      ebeg[i] = rp.beg[i];
      edeg[i] = deg;
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
    int cnt[kRowsPerHalf], deg[kRowsPerHalf];
    int32_t beg[kRowsPerHalf];
#pragma unroll
    for (int i = 0; i < kRowsPerHalf; ++i) {
      L.nbr[hw][i][t] = t < es.cnt[i] ? es.nbr[i] : clamp_row(row_of(T, i));
      L.attr[hw][i][t] = es.attr[i];
      cnt[i] = es.cnt[i];
      beg[i] = ebeg[i];
      deg[i] = edeg[i];
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
    const int mdeg = max(deg[0], deg[1]);
    for (int c0 = 0;; c0 += kSlots) {  // the chunk holding edges c0 .. c0 + kSlots - 1
      const int m = max(cnt[0], cnt[1]);
      for (int j0 = 0; j0 < m; j0 += kUD) {
        f4v r0[kUD], r1[kUD];
        float a0[kUD], a1v[kUD];
#pragma unroll
        for (int u = 0; u < kUD; ++u) {
          const int j = min(j0 + u, kSlots - 1);
          r0[u] = ld_f4v(xb, (uint32_t)L.nbr[hw][0][j] * kRowBytes + qb);
          r1[u] = ld_f4v(xb, (uint32_t)L.nbr[hw][1][j] * kRowBytes + qb);
          a0[u] = L.attr[hw][0][j];
          a1v[u] = L.attr[hw][1][j];
        }
#pragma unroll
        for (int u = 0; u < kUD; ++u) {
          edge_acc<FMA>(acc[0], r0[u], a0[u], lw, lb, j0 + u < cnt[0]);
          edge_acc<FMA>(acc[1], r1[u], a1v[u], lw, lb, j0 + u < cnt[1]);
        }
      }
      if (c0 + kSlots >= mdeg) break;
      __builtin_amdgcn_wave_barrier();  // this chunk's reads done before the next one's writes
#pragma unroll
      for (int i = 0; i < kRowsPerHalf; ++i) {
        const int cn = max(0, min(deg[i] - (c0 + kSlots), kSlots));
        // slot t of the next chunk, clamped to the row's last edge (an empty row: edge 0)
        const int e = deg[i] > 0 ? beg[i] + min(c0 + kSlots + t, deg[i] - 1) : 0;
        const int32_t nb = A.nbr[e];
        L.attr[hw][i][t] = A.attr[e];
        L.nbr[hw][i][t] = t < cn ? nb : clamp_row(row_of(T, i));
        cnt[i] = cn;
      }
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int i = 0; i < kRowsPerHalf; ++i) {
      const int r = hw + kHalves * i;
      const f4v zv = add_scaled(acc[i], ope, self[i]);
      *reinterpret_cast<f4v*>(&sz[r * kLD + 4 * t]) = zv;
    }
    __builtin_amdgcn_wave_barrier();  // edge-list reads done before the next tile's writes
    __syncthreads();
  }
}

// One round of the gather waves: phase A's gather, W2's staging, their share of the relu
// planes, then the epilogue (and head) of each tile beside the matrix waves' next chain.
template <bool FMA, int EPI, bool DEEP = false>
__device__ __forceinline__ void eval_round_gather(const FusedArgs& A, const LayerArgs& B,
                                                  LayerLds& L, const TileSeq& rs, int nt) {
  constexpr int kG = kThreads - kMatThreads;
  constexpr int kW2Per = kD * kD4 / kG;
  if constexpr (DEEP) gather_role_deep<FMA>(A, L.f, rs, nt);
  else gather_role<FMA, false, false, false>(A, L.f, rs, nt);
  const int tidr = per_round(threadIdx.x);
  const int p = tidr - kMatThreads;  // 0 .. 511
  const int eq = p & 31, er = p >> 5;
  {
    W2Regs<kW2Per> w2r;  // (confined to this scope, as in k_mp_fwd_layer)
    w2r.load(reinterpret_cast<const float4*>(B.W2), p, kG);
    __syncthreads();  // gather_role's last barrier (the matrix role multiplies the last tile)
    __syncthreads();  // phase A's LDS use is over (L.f.w is free)
    w2r.store(L.f.w, p, kG);
  }
  // the epilogue's bias and residual rows, in flight under the planes pass (named vectors: an
  // array of them held across the barriers would stay in private memory)
  const char* xb = reinterpret_cast<const char*>(A.x);
  const f4v bias2 = ld_f4v(reinterpret_cast<const char*>(B.b2), (uint32_t)eq * 16u);
  static_assert(kLayerTiles == 2, "two tiles of residual rows, named");
  f4v x00 = f4v_zero(), x01 = f4v_zero(), x10 = f4v_zero(), x11 = f4v_zero();
  if constexpr (EPI == EPI_OUT_RES) {
    auto row = [&](int k, int i) -> uint32_t {
      int64_t n = (int64_t)rs.at(k < nt ? k : 0) * kTileRows + er + 16 * i;
      n = n < A.N ? n : A.N - 1;
      return (uint32_t)n * kRowBytes + (uint32_t)eq * 16u;
    };
    x00 = ld_f4v(xb, row(0, 0));
    x01 = ld_f4v(xb, row(0, 1));
    x10 = ld_f4v(xb, row(1, 0));
    x11 = ld_f4v(xb, row(1, 1));
  }
  __syncthreads();  // W2 staged
  __syncthreads();  // W2's fragments read: the w region takes the relu planes
  relu_planes(L, rs, nt, A.N, tidr);
  __syncthreads();
  float* const hwl = L.hd;
  const float bb[4] = {bias2.x, bias2.y, bias2.z, bias2.w};
  for (int k = 0; k < nt; ++k) {
    const float* sO = out_tile(L, k);
    __syncthreads();  // output tile k in LDS
    const int T = rs.at(k);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = er + 16 * i;
      const int64_t n = (int64_t)T * kTileRows + r;
      const float4 v = *reinterpret_cast<const float4*>(&sO[r * kLD + 4 * eq]);
      if (n >= A.N) continue;
      const float vv[4] = {v.x, v.y, v.z, v.w};
      float o4[4];
      if constexpr (EPI == EPI_OUT_RES) {
        const f4v xv = k == 0 ? (i == 0 ? x00 : x01) : (i == 0 ? x10 : x11);
        const float xr[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) o4[c] = xr[c] + relu_nan(vv[c] + bb[c]);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float o = vv[c] + bb[c];
          o4[c] = (EPI == EPI_OUT_RELU) ? relu_nan(o) : o;
        }
      }
      if (B.y)
        *reinterpret_cast<float4*>(B.y + n * kD + 4 * eq) =
            make_float4(o4[0], o4[1], o4[2], o4[3]);
      if (B.hk) {  // the head on this row: k_head_fwd's fma order and reduction
        float a[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const float4 wk = *reinterpret_cast<const float4*>(&hwl[kk * kD + 4 * eq]);
          a[kk] = 0.f;
          a[kk] = __builtin_fmaf(o4[0], wk.x, a[kk]);
          a[kk] = __builtin_fmaf(o4[1], wk.y, a[kk]);
          a[kk] = __builtin_fmaf(o4[2], wk.z, a[kk]);
          a[kk] = __builtin_fmaf(o4[3], wk.w, a[kk]);
        }
        const float d = head::sum4_32(a[0], a[1], a[2], a[3]);
        const int o = (eq >> 3) & 3;
        float* rt = hwl + kHR + k * kHRTile + r * B.hk;
        if ((eq & 7) == 0 && o < B.hk) rt[o] = d + hwl[kHB + o];
        if (B.hk == 5) {
          const float4 wk = *reinterpret_cast<const float4*>(&hwl[4 * kD + 4 * eq]);
          float a4 = 0.f;
          a4 = __builtin_fmaf(o4[0], wk.x, a4);
          a4 = __builtin_fmaf(o4[1], wk.y, a4);
          a4 = __builtin_fmaf(o4[2], wk.z, a4);
          a4 = __builtin_fmaf(o4[3], wk.w, a4);
          a4 = head::sum_32(a4);
          if (eq == 1) rt[4] = a4 + hwl[kHB + 4];
        }
      }
    }
  }
  if (B.hk) {  // the head's PostProcess and stores of the round's tiles
    __syncthreads();
    const int per = kTileRows * B.hk;
    const int kt = p < per ? 0 : (p < 2 * per ? 1 : kLayerTiles), e = p - kt * per;
    if (kt < nt) head_finish(B, hwl + kHR + kt * kHRTile, rs.at(kt), A.N, e);
  }
  __syncthreads();  // the round's LDS use is over
}

// ---------------------------------------------------------------------------------------
// The layer forward in eval mode in one launch (gine_mp_fwd_layer_eval).  BatchNorm from the
// running statistics is a per-channel affine map known before the launch (bn_eval_channel),
// so no tile waits for another: k_mp_fwd_layer without its statistics and its grid barrier --
// no residency requirement, any grid, any N.  A workgroup walks its tiles in rounds of
// kLayerTiles; a round is the training kernel's two phases on those tiles:
//   phase A = gather_role (z into the fp32 LDS tiles only) beside matrix_role<false, true>
//             (k_mp_fwd_mlp1's chain and redo on the LDS tile, a1 into the a1k tiles only);
//   phase B = k_mp_fwd_layer's: W2 staged over W1's image, r = relu(bn(a1)) split once into
//             planes, Linear2's chain and redo, epilogue and head on the gather waves.
// W1 and W2 are staged again every round (from L2).  Memory is written by the epilogue only:
// y (unless NULL, with a head) and the head's raw / pred / count_parts.  Same arithmetic and
// order per tile as the separate eval launches (gine_mp_fwd_mlp1, gine_bn_fwd_finalize,
// gine_mlp_fwd2, gine_head_fwd_count), whatever tile -> workgroup map the grid gives.
// ---------------------------------------------------------------------------------------
template <bool FMA, int EPI>
__global__ __launch_bounds__(kThreads, 1) void k_mp_fwd_layer_eval(FusedArgs A, LayerArgs B) {
  __shared__ __attribute__((aligned(16))) LayerLds L;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const bool mat = wave < kMatThreads / kWave;
  // the row GEMM's XCD-contiguous map where every XCD has a workgroup, else a plain stride
  const TileSeq ts = gridDim.x >= (unsigned)kNumXcd
                         ? tile_seq(A.num_tiles, blockIdx.x, gridDim.x)
                         : TileSeq{(int)blockIdx.x, A.num_tiles, (int)gridDim.x};
  const int nall = ts.count();
  float* const hwl = L.hd;
  uint32_t* const cwl = reinterpret_cast<uint32_t*>(hwl + kHC);

  // ---- once: alpha | shift, the head's weights and the valid-target counts ----
  const int p0 = tid - kMatThreads;  // (gather waves: 0 .. 511)
  if (tid < GINE_COUNT_PARTS) cwl[tid] = 0;
  if (!mat && p0 < kD) bn_eval_channel(B.q, p0, &L.bn[p0], &L.bn[kD + p0]);
  if (!mat && B.hk) {
    if (p0 < B.hk * kD4)
      *reinterpret_cast<float4*>(&hwl[4 * p0]) =
          *reinterpret_cast<const float4*>(B.hd.weight + 4 * p0);
    else if (p0 < B.hk * kD4 + B.hk)
      hwl[kHB + p0 - B.hk * kD4] = B.hd.bias[p0 - B.hk * kD4];
  }
  if (B.hk && B.hd.count_parts) {  // (k_mp_fwd_layer's count: integer sums, any order)
    __syncthreads();
    if (!mat) {
      const int64_t chunk = ((int64_t)A.N + GINE_COUNT_PARTS - 1) / GINE_COUNT_PARTS;
      for (int q = blockIdx.x; q < GINE_COUNT_PARTS; q += gridDim.x) {
        const int64_t lo = (int64_t)q * chunk, hi = min(lo + chunk, (int64_t)A.N);
        uint32_t c = 0;
        for (int64_t i = lo + p0; i < hi; i += kThreads - kMatThreads)
          c += B.hd.y_target[i] == B.hd.y_target[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
        if (tid % kWave == 0) atomicAdd(&cwl[q], c);
      }
    }
    __syncthreads();
    if (!mat) {
      const int q = (int)blockIdx.x + p0 * (int)gridDim.x;
      if (q < GINE_COUNT_PARTS) B.hd.count_parts[q] = cwl[q];
    }
  }
  // The roles keep to their own branch for the whole round (one barrier sequence each, as in
  // phase A): what one role holds in registers -- W2's planes, the residual rows -- is then
  // no live value of the other's code.
  for (int r0 = 0; r0 < nall; r0 += kLayerTiles) {
    const TileSeq rs{ts.at(r0), min(ts.end, ts.at(r0 + kLayerTiles)), ts.step};
    const int nt = rs.count();  // 1 .. kLayerTiles
    if (mat) eval_round_matrix(A, B, L, rs, nt, wave);
    else eval_round_gather<FMA, EPI>(A, B, L, rs, nt);
  }
}

// k_mp_fwd_layer_eval at any in-degree (gine_mp_fwd_layer_eval_deep): the gather waves run
// gather_role_deep; all else is the kernel above restated (a body shared as a function changes
// the instruction streams of the six instantiations above), and must be kept in step with it.
template <bool FMA, int EPI>
__global__ __launch_bounds__(kThreads, 1) void k_mp_fwd_layer_eval_deep(FusedArgs A,
                                                                        LayerArgs B) {
  __shared__ __attribute__((aligned(16))) LayerLds L;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const bool mat = wave < kMatThreads / kWave;
  // the row GEMM's XCD-contiguous map where every XCD has a workgroup, else a plain stride
  const TileSeq ts = gridDim.x >= (unsigned)kNumXcd
                         ? tile_seq(A.num_tiles, blockIdx.x, gridDim.x)
                         : TileSeq{(int)blockIdx.x, A.num_tiles, (int)gridDim.x};
  const int nall = ts.count();
  float* const hwl = L.hd;
  uint32_t* const cwl = reinterpret_cast<uint32_t*>(hwl + kHC);

  // ---- once: alpha | shift, the head's weights and the valid-target counts ----
  const int p0 = tid - kMatThreads;  // (gather waves: 0 .. 511)
  if (tid < GINE_COUNT_PARTS) cwl[tid] = 0;
  if (!mat && p0 < kD) bn_eval_channel(B.q, p0, &L.bn[p0], &L.bn[kD + p0]);
  if (!mat && B.hk) {
    if (p0 < B.hk * kD4)
      *reinterpret_cast<float4*>(&hwl[4 * p0]) =
          *reinterpret_cast<const float4*>(B.hd.weight + 4 * p0);
    else if (p0 < B.hk * kD4 + B.hk)
      hwl[kHB + p0 - B.hk * kD4] = B.hd.bias[p0 - B.hk * kD4];
  }
  if (B.hk && B.hd.count_parts) {  // (k_mp_fwd_layer's count: integer sums, any order)
    __syncthreads();
    if (!mat) {
      const int64_t chunk = ((int64_t)A.N + GINE_COUNT_PARTS - 1) / GINE_COUNT_PARTS;
      for (int q = blockIdx.x; q < GINE_COUNT_PARTS; q += gridDim.x) {
        const int64_t lo = (int64_t)q * chunk, hi = min(lo + chunk, (int64_t)A.N);
        uint32_t c = 0;
        for (int64_t i = lo + p0; i < hi; i += kThreads - kMatThreads)
          c += B.hd.y_target[i] == B.hd.y_target[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
        if (tid % kWave == 0) atomicAdd(&cwl[q], c);
      }
    }
    __syncthreads();
    if (!mat) {
      const int q = (int)blockIdx.x + p0 * (int)gridDim.x;
      if (q < GINE_COUNT_PARTS) B.hd.count_parts[q] = cwl[q];
    }
  }
  // The roles keep to their own branch for the whole round (one barrier sequence each, as in
  // phase A): what one role holds in registers -- W2's planes, the residual rows -- is then
  // no live value of the other's code.
  for (int r0 = 0; r0 < nall; r0 += kLayerTiles) {
    const TileSeq rs{ts.at(r0), min(ts.end, ts.at(r0 + kLayerTiles)), ts.step};
    const int nt = rs.count();  // 1 .. kLayerTiles
    if (mat) eval_round_matrix(A, B, L, rs, nt, wave);
    else eval_round_gather<FMA, EPI, true>(A, B, L, rs, nt);
  }
}

}  // namespace
}  // namespace gine

using namespace gine;

namespace {
// Both entries: validation before any HIP call, then one launch.  DEEP: k_mp_fwd_layer_eval_deep,
// whose only degree condition is max_in_degree >= 0 (the rows' lengths come from in_rowptr).
template <bool DEEP>
int layer_eval_launch(const float* x, const int32_t* in_rowptr, const int32_t* in_src,
                      const float* in_attr, const float* lin_w, const float* lin_b,
                      const float* eps, const float* w1, const float* b1, const float* gamma,
                      const float* beta, const float* running_mean, const float* running_var,
                      float bn_eps, const float* w2, const float* b2, float* y,
                      int64_t num_nodes, int32_t channels, int32_t max_in_degree, int32_t flags,
                      int32_t epilogue, const gine_layer_head* head, int32_t max_workgroups,
                      void* stream) {
  if (channels != kD) return GINE_ERR_DIM;
  if ((flags & ~GINE_MP_LIN_MULADD) != 0) return GINE_ERR_INVALID;
  if (max_in_degree < 0 || (!DEEP && max_in_degree > GINE_MP_FUSED_MAX_DEGREE))
    return GINE_ERR_INVALID;
  if (epilogue < GINE_EPI_NONE || epilogue > GINE_EPI_RESIDUAL_RELU) return GINE_ERR_INVALID;
  if (num_nodes < 0 || max_workgroups < 0) return GINE_ERR_INVALID;
  if (!x || !in_rowptr || !in_src || !in_attr || !lin_w || !lin_b || !eps || !w1 || !b1 ||
      !running_mean || !running_var || !w2 || !b2 || (!y && !head))
    return GINE_ERR_INVALID;
  int hk = 0;
  if (head) {
    switch (head->kind) {
      case GINE_LOSS_NORMAL: hk = 2; break;
      case GINE_LOSS_MIXED_NORMAL: hk = 3; break;
      case GINE_LOSS_MIXED: hk = 4; break;
      case GINE_LOSS_MIXED_U: hk = 5; break;
      default: return GINE_ERR_INVALID;
    }
    if (!head->weight || !head->bias || !head->raw || !head->pred ||
        (head->count_parts && !head->y_target))
      return GINE_ERR_INVALID;
  }
  if (num_nodes * channels * 4 >= (int64_t(1) << 32)) return GINE_ERR_TOO_LARGE;
  if (num_nodes == 0) return GINE_OK;
  // one workgroup per CU at most (LDS); more tiles than that are walked in rounds
  int dev = 0, cus = 0;
  GINE_RETURN_IF_HIP(hipGetDevice(&dev));
  GINE_RETURN_IF_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int tiles = (int)ceil_div(num_nodes, kTileRows);
  int grid = std::min(tiles, std::max(cus, 1));
  if (max_workgroups > 0) grid = std::min(grid, (int)max_workgroups);
  hipStream_t s = as_stream(stream);
  const FusedArgs A{x,   in_rowptr, in_src, in_attr, lin_w,   lin_b,
                    eps, w1,        b1,     nullptr, nullptr, nullptr,
                    nullptr, (int)num_nodes, tiles};
  // (the running statistics are read only: BnFwdParams is shared with the training forms)
  const LayerArgs B{w2, b2, y, nullptr,
                    BnFwdParams{gamma, beta, const_cast<float*>(running_mean),
                                const_cast<float*>(running_var), nullptr, nullptr, num_nodes,
                                0.f, bn_eps, 0},
                    nullptr, 0, 0, head ? *head : gine_layer_head{}, hk};
  const bool fma = !(flags & GINE_MP_LIN_MULADD);
#define EVAL_LAUNCH(F_, E_)                                                              \
  do {                                                                                   \
    if (DEEP)                                                                            \
      hipLaunchKernelGGL((k_mp_fwd_layer_eval_deep<F_, E_>), dim3((unsigned)grid),       \
                         dim3(kThreads), 0, s, A, B);                                    \
    else                                                                                 \
      hipLaunchKernelGGL((k_mp_fwd_layer_eval<F_, E_>), dim3((unsigned)grid),            \
                         dim3(kThreads), 0, s, A, B);                                    \
  } while (0)
  switch (epilogue) {
    case GINE_EPI_NONE:
      if (fma) EVAL_LAUNCH(true, EPI_OUT); else EVAL_LAUNCH(false, EPI_OUT);
      break;
    case GINE_EPI_RELU:
      if (fma) EVAL_LAUNCH(true, EPI_OUT_RELU); else EVAL_LAUNCH(false, EPI_OUT_RELU);
      break;
    default:
      if (fma) EVAL_LAUNCH(true, EPI_OUT_RES); else EVAL_LAUNCH(false, EPI_OUT_RES);
  }
#undef EVAL_LAUNCH
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}
}  // namespace

extern "C" int gine_mp_fwd_layer_eval(const float* x, const int32_t* in_rowptr,
                                      const int32_t* in_src, const float* in_attr,
                                      const float* lin_w, const float* lin_b, const float* eps,
                                      const float* w1, const float* b1, const float* gamma,
                                      const float* beta, const float* running_mean,
                                      const float* running_var, float bn_eps, const float* w2,
                                      const float* b2, float* y, int64_t num_nodes,
                                      int32_t channels, int32_t max_in_degree, int32_t flags,
                                      int32_t epilogue, const gine_layer_head* head,
                                      int32_t max_workgroups, void* stream) {
  return layer_eval_launch<false>(x, in_rowptr, in_src, in_attr, lin_w, lin_b, eps, w1, b1, gamma,
                                  beta, running_mean, running_var, bn_eps, w2, b2, y, num_nodes,
                                  channels, max_in_degree, flags, epilogue, head, max_workgroups,
                                  stream);
}

extern "C" int gine_mp_fwd_layer_eval_deep(const float* x, const int32_t* in_rowptr,
                                           const int32_t* in_src, const float* in_attr,
                                           const float* lin_w, const float* lin_b, const float* eps,
                                           const float* w1, const float* b1, const float* gamma,
                                           const float* beta, const float* running_mean,
                                           const float* running_var, float bn_eps, const float* w2,
                                           const float* b2, float* y, int64_t num_nodes,
                                           int32_t channels, int32_t max_in_degree, int32_t flags,
                                           int32_t epilogue, const gine_layer_head* head,
                                           int32_t max_workgroups, void* stream) {
  return layer_eval_launch<true>(x, in_rowptr, in_src, in_attr, lin_w, lin_b, eps, w1, b1, gamma,
                                  beta, running_mean, running_var, bn_eps, w2, b2, y, num_nodes,
                                  channels, max_in_degree, flags, epilogue, head, max_workgroups,
                                  stream);
}
