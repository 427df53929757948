// GINEConv message passing with K edge attributes per edge (1 <= K <= GINE_MP_MAX_EDGE_DIM)
// and the gradient with respect to them.
//
//   e_c = b_c;  for k = 0 .. K-1:  e_c = fma(a_e[k], W[c][k], e_c)     (one rounding per term)
//   m_e = relu(x[src_e] + e)     z_i = sum over in-edges of i, in CSR order, of m_e + (1 + eps) x_i
//   dm_e = (x[src_e] + e <= 0) ? 0 : dz[dst_e]
//   dx_i = sum over out-edges of i of dm_e [+ (1 + eps) dz_i] [+ dres_i]
//   dW[c][k] = sum_e dm_e[c] a_e[k]    db[c] = sum_e dm_e[c]    deps = sum dz * x
//   d a_e[k] = sum_c dm_e[c] W[c][k]                                   (EATTR instantiations)
//
// Same structure as gine_mp.hip (C == 1 shapes): a row group of L lanes owns a node, its
// edge list goes through LDS in chunks of L edges -- neighbour row offset, the K attributes
// and, for the edge gradient, the edge's id in the caller's edge_attr --, U neighbour rows
// are in flight per lane, every neighbour load is clamped and issued unconditionally, and a
// destination's sum stays sequential.  K is padded to the bucket KB in {1, 2, 4, 8}: the
// padding terms fma(0, 0, e) are exact, so the result has the bits of the K-term chain.  At
// K = 1 the chain is the fma mode of gine_mp_fwd / gine_mp_bwd.
#include "gine_common.hpp"
#include "gine_edge.hpp"
#include "gine_reduce.hpp"

namespace gine {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;

// Neighbour rows in flight per lane: the K = 8 bucket holds 32 more weight registers (and 32
// more accumulators in the backward), so it keeps fewer rows.
template <int KB>
struct EkUnroll {
  static constexpr int value = KB <= 4 ? 6 : 4;
};

// lin.weight [D, K] row-major -> per lane, KB registers of the lane's 4 channels (0 past K).
// `vec` (K == KB and lin_w 16-byte aligned, host-checked): the lane's 4 rows are 4 K
// contiguous floats, loaded as K float4 (the wave's loads are one contiguous run) and
// transposed in registers; otherwise 4 K strided scalar loads (measured at K = 8, D = 128,
// where a wave's scalar loads each touch 32 cache lines: the forward took 37 us with them).
template <int KB>
__device__ __forceinline__ void load_w_ek(f4v (&w)[KB], const float* __restrict__ lw, int q,
                                          int K, bool vec) {
  if (vec) {
    f4v flat[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j)
      flat[j] = ld_f4v(reinterpret_cast<const char*>(lw), (uint32_t)q * (16u * KB) + 16u * j);
#pragma unroll
    for (int k = 0; k < KB; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) w[k][i] = flat[(i * KB + k) / 4][(i * KB + k) % 4];
    return;
  }
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    w[k] = f4v_zero();
    if (k < K) {
#pragma unroll
      for (int i = 0; i < 4; ++i) w[k][i] = lw[(q * 4 + i) * K + k];
    }
  }
}

// One edge slot of the LDS table: the KB attributes of edge `e` (0 past K).  Every load is
// issued (past K: the edge's last attribute again, then dropped), so the KB loads and the
// neighbour id are in flight together instead of one round trip after another.
template <int KB>
__device__ __forceinline__ void stage_attr_ek(float* slot, const char* attrb, uint32_t e,
                                              int K) {
  const uint32_t off = e * (uint32_t)K * 4u;  // E*K*4 < 2^32, host-checked
  float v[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k)
    v[k] = *reinterpret_cast<const float*>(attrb + off + 4u * (uint32_t)min(k, K - 1));
#pragma unroll
  for (int k = 0; k < KB; ++k) slot[k] = k < K ? v[k] : 0.f;
}

// Between a batch of neighbour-row loads and the sums that consume it: the loads all issue
// first (U rows in flight), whatever else the scheduler would like to put before them.
__device__ __forceinline__ void loads_first() { __builtin_amdgcn_sched_barrier(0); }

template <int KB>
__device__ __forceinline__ f4v edge_lin_ek(const float* a, const f4v (&w)[KB], f4v b) {
  f4v e = b;
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const f2v av = {a[k], a[k]};
    e.xy = __builtin_elementwise_fma(av, w[k].xy, e.xy);
    e.zw = __builtin_elementwise_fma(av, w[k].zw, e.zw);
  }
  return e;
}

template <int KB>
__device__ __forceinline__ void fwd_edge_ek(f4v& acc, f4v r, const float* a,
                                            const f4v (&w)[KB], f4v b) {
  const f4v e = edge_lin_ek<KB>(a, w, b);
  acc.xy = acc.xy + relu2(r.xy + e.xy);
  acc.zw = acc.zw + relu2(r.zw + e.zw);
}

// Returns dm (the edge gradient's operand).
template <int KB>
__device__ __forceinline__ f4v bwd_edge_ek(f4v& acc, f4v (&accw)[KB], f4v r, const float* a,
                                           f4v h, const f4v (&w)[KB], f4v b) {
  const f4v e = edge_lin_ek<KB>(a, w, b);
  const f2v plo = h.xy + e.xy;
  const f2v phi = h.zw + e.zw;
  f4v dm;
  dm.x = plo.x <= 0.f ? 0.f : r.x;
  dm.y = plo.y <= 0.f ? 0.f : r.y;
  dm.z = phi.x <= 0.f ? 0.f : r.z;
  dm.w = phi.y <= 0.f ? 0.f : r.w;
  acc.xy = acc.xy + dm.xy;
  acc.zw = acc.zw + dm.zw;
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const f2v av = {a[k], a[k]};
    accw[k].xy = __builtin_elementwise_fma(dm.xy, av, accw[k].xy);
    accw[k].zw = __builtin_elementwise_fma(dm.zw, av, accw[k].zw);
  }
  return dm;
}

// d a_e[k] = sum_c dm[c] W[c][k]: the lane's 4 channels in fp32, then a fixed butterfly over
// the L lanes of the row group (padding lanes add 0); lane 0 of the group stores.
template <int L, int KB>
__device__ __forceinline__ void edge_grad_ek(f4v dm, const f4v (&w)[KB], bool lane_valid,
                                             bool store, float* __restrict__ dea, uint32_t eid,
                                             int K) {
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    if (k < K) {  // uniform
      float s = (dm.x * w[k].x + dm.y * w[k].y) + (dm.z * w[k].z + dm.w * w[k].w);
      s = lane_valid ? s : 0.f;
#pragma unroll
      for (int m = 1; m < L; m <<= 1) s += __shfl_xor(s, m, kWave);
      if (store) dea[(size_t)eid * K + k] = s;
    }
  }
}

// ----------------------------------------------------------------------------------------
// Forward
// ----------------------------------------------------------------------------------------
template <int L, int KB>
__global__ __launch_bounds__(kThreads) void k_mp_fwd_ek(
    const float4* __restrict__ x4, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ nbr, const float* __restrict__ attr,
    const float* __restrict__ lw, const float4* __restrict__ lb4,
    const float* __restrict__ eps, float4* __restrict__ z4, int64_t N, int D4, int K,
    int wvec) {
  constexpr int GPW = kWave / L;  // nodes per wave
  constexpr int U = EkUnroll<KB>::value;
  __shared__ int32_t s_nbr[kWaves][kWave];
  __shared__ __attribute__((aligned(16))) float s_attr[kWaves][kWave * KB];

  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int g = lane / L, t = lane % L;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t node = (int64_t)tile * (kWaves * GPW) + wave * GPW + g;
  if (node >= N) return;  // whole row group leaves together; no block barrier below

  // Lanes past the last float4 duplicate the last chunk (loads unconditional, stores masked).
  const char* xb = reinterpret_cast<const char*>(x4);
  const char* attrb = reinterpret_cast<const char*>(attr);
  const uint32_t rowb = (uint32_t)D4 * 16u;
  const int q = min(t, D4 - 1);
  const uint32_t qb = (uint32_t)q * 16u;
  const uint32_t own = (uint32_t)node * rowb;
  f4v w[KB];
  load_w_ek<KB>(w, lw, q, K, wvec != 0);
  const f4v b = ld_f4v(reinterpret_cast<const char*>(lb4), qb);
  const f4v self = ld_f4v(xb, own + qb);
  f4v acc = f4v_zero();
  const float ope = 1.0f + eps[0];
  const int beg = rowptr[node], end = rowptr[node + 1];
  int32_t* my_nbr = &s_nbr[wave][g * L];
  float* my_attr = &s_attr[wave][g * L * KB];

  for (int base = beg; base < end; base += L) {
    const int cnt = min(L, end - base);
    if (t < cnt) {
      const int32_t nb_t = nbr[base + t];
      stage_attr_ek<KB>(my_attr + t * KB, attrb, (uint32_t)(base + t), K);
      my_nbr[t] = (int32_t)((uint32_t)nb_t * rowb);  // row byte offset
    }
    __builtin_amdgcn_wave_barrier();
    int j = 0;
    // full batches of U neighbours: no per-edge test
    for (; j + U <= cnt; j += U) {
      f4v r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) r[u] = ld_f4v(xb, (uint32_t)my_nbr[j + u] + qb);
      loads_first();
#pragma unroll
      for (int u = 0; u < U; ++u) fwd_edge_ek<KB>(acc, r[u], my_attr + (j + u) * KB, w, b);
    }
    // tail: loads clamped to the last neighbour (always issued), sums tested
    if (j < cnt) {
      f4v r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) r[u] = ld_f4v(xb, (uint32_t)my_nbr[min(j + u, cnt - 1)] + qb);
      loads_first();
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (j + u < cnt) fwd_edge_ek<KB>(acc, r[u], my_attr + (j + u) * KB, w, b);
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (t < D4) z4[node * D4 + t] = to_float4(add_scaled(acc, ope, self));
}

// ----------------------------------------------------------------------------------------
// Backward over the out-edge CSR (source-sorted, stable)
// ----------------------------------------------------------------------------------------
// KB = 1 fits 128 VGPRs like k_mp_bwd (4 workgroups per CU); the wider buckets hold KB
// fp64 quads of dW partials per lane and take the registers they need (no scratch).
template <int L, int KB, bool EATTR>
__global__ __launch_bounds__(kThreads, KB == 1 ? 4 : 1) void k_mp_bwd_ek(
    const float4* __restrict__ dz4, const float4* __restrict__ x4,
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr,
    const float* __restrict__ attr, const int32_t* __restrict__ eids,
    const float* __restrict__ lw, const float4* __restrict__ lb4,
    const float* __restrict__ eps, const float4* __restrict__ dres4, float4* __restrict__ dx4,
    float* __restrict__ dea, double* __restrict__ partials, int64_t N, int D4, int K,
    int wvec, int num_tiles, int flags) {
  constexpr int GPW = kWave / L;
  constexpr int U = EkUnroll<KB>::value;
  __shared__ int32_t s_nbr[kWaves][kWave];
  __shared__ int32_t s_eid[EATTR ? kWaves : 1][kWave];
  __shared__ __attribute__((aligned(16))) float s_attr[kWaves][kWave * KB];
  extern __shared__ __attribute__((aligned(16))) double s_red[];  // [(K + 1) D + kWaves]

  const int D = D4 * 4;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int g = lane / L, t = lane % L;
  const float ope = 1.0f + eps[0];
  const bool add_self = (flags & GINE_MP_BWD_SELF) != 0;
  const char* dzb = reinterpret_cast<const char*>(dz4);
  const char* xb = reinterpret_cast<const char*>(x4);
  const char* attrb = reinterpret_cast<const char*>(attr);
  // the residual gradient row is loaded with the node's own rows (from dz when there is none)
  const char* rb = reinterpret_cast<const char*>(dres4 != nullptr ? dres4 : dz4);
  const uint32_t rowb = (uint32_t)D4 * 16u;
  const bool lane_valid = t < D4;

  const int q = min(t, D4 - 1);
  const uint32_t qb = (uint32_t)q * 16u;
  f4v w[KB];
  load_w_ek<KB>(w, lw, q, K, wvec != 0);
  const f4v b = ld_f4v(reinterpret_cast<const char*>(lb4), qb);
  double pw[KB][4], pb[4];  // sum dm*a_k, sum dm (per channel, per-node terms)
  double pe = 0.0;          // sum over nodes and channels of dz*x
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pb[i] = 0.0;
#pragma unroll
    for (int k = 0; k < KB; ++k) pw[k][i] = 0.0;
  }
  int32_t* my_nbr = &s_nbr[wave][g * L];
  int32_t* my_eid = &s_eid[EATTR ? wave : 0][g * L];
  float* my_attr = &s_attr[wave][g * L * KB];

  // Tiles are split into 8 contiguous XCD ranges; the blocks of one XCD stride its range.
  const int vb = blockIdx.x, nb = gridDim.x;
  const int xcd = vb % kNumXcd, pos = vb / kNumXcd;
  const int blocks_here = nb / kNumXcd + (xcd < nb % kNumXcd ? 1 : 0);
  const int span = (num_tiles + kNumXcd - 1) / kNumXcd;
  const int t_begin = xcd * span, t_end = min(num_tiles, t_begin + span);

  for (int tile = t_begin + pos; tile < t_end; tile += blocks_here) {
    const int64_t node = (int64_t)tile * (kWaves * GPW) + wave * GPW + g;
    if (node >= N) continue;
    const uint32_t own = (uint32_t)node * rowb;
    f4v acc = f4v_zero(), accw[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) accw[k] = f4v_zero();
    const f4v h = ld_f4v(xb, own + qb);
    const f4v g_self = ld_f4v(dzb, own + qb);
    const f4v r_self = ld_f4v(rb, own + qb);
    const int beg = rowptr[node], end = rowptr[node + 1];
    for (int base = beg; base < end; base += L) {
      const int cnt = min(L, end - base);
      if (t < cnt) {
        const int32_t nb_t = nbr[base + t];
        int32_t eid_t = 0;
        if constexpr (EATTR) eid_t = eids[base + t];
        stage_attr_ek<KB>(my_attr + t * KB, attrb, (uint32_t)(base + t), K);
        my_nbr[t] = (int32_t)((uint32_t)nb_t * rowb);  // row byte offset
        if constexpr (EATTR) my_eid[t] = eid_t;
      }
      __builtin_amdgcn_wave_barrier();
      int j = 0;
      // full batches of U neighbours: no per-edge test
      for (; j + U <= cnt; j += U) {
        f4v r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = ld_f4v(dzb, (uint32_t)my_nbr[j + u] + qb);
        loads_first();
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const f4v dm = bwd_edge_ek<KB>(acc, accw, r[u], my_attr + (j + u) * KB, h, w, b);
          if constexpr (EATTR)
            edge_grad_ek<L, KB>(dm, w, lane_valid, t == 0, dea, (uint32_t)my_eid[j + u], K);
        }
      }
      // tail: loads clamped to the last neighbour (always issued), sums tested; the whole row
      // group takes the same side of the test, so the butterfly's lanes are all active
      if (j < cnt) {
        f4v r[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
          r[u] = ld_f4v(dzb, (uint32_t)my_nbr[min(j + u, cnt - 1)] + qb);
        loads_first();
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (j + u < cnt) {
            const f4v dm = bwd_edge_ek<KB>(acc, accw, r[u], my_attr + (j + u) * KB, h, w, b);
            if constexpr (EATTR)
              edge_grad_ek<L, KB>(dm, w, lane_valid, t == 0, dea, (uint32_t)my_eid[j + u], K);
          }
      }
      __builtin_amdgcn_wave_barrier();
    }
    if (lane_valid) {
      // db = sum_e dm_e: each source node contributes its message-gradient sum
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        pb[i] += (double)acc[i];
#pragma unroll
        for (int k = 0; k < KB; ++k) pw[k][i] += (double)accw[k][i];
      }
      f4v o = add_self ? add_scaled(acc, ope, g_self) : acc;
      if (dres4 != nullptr) {
        o.xy = o.xy + r_self.xy;
        o.zw = o.zw + r_self.zw;
      }
      dx4[node * D4 + t] = to_float4(o);
      pe += ((double)g_self.x * (double)h.x + (double)g_self.y * (double)h.y) +
            ((double)g_self.z * (double)h.z + (double)g_self.w * (double)h.w);
    }
  }

  // Block reduction of the parameter-gradient partials: row groups of a wave first
  // (butterfly over lanes t, t+L, ...), then the waves in fixed order through LDS.
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int m = L; m < kWave; m <<= 1) {
      pb[i] += shfl_xor_d(pb[i], m);
#pragma unroll
      for (int k = 0; k < KB; ++k) pw[k][i] += shfl_xor_d(pw[k][i], m);
    }
  }
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) pe += shfl_xor_d(pe, m);
  const int ob = D * K, oe = D * (K + 1);  // offsets of db and of the eps column
  for (int wv = 0; wv < kWaves; ++wv) {
    if (wave == wv && g == 0) {
      if (lane_valid) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ch = t * 4 + i;
          if (wv == 0) s_red[ob + ch] = pb[i];
          else s_red[ob + ch] += pb[i];
#pragma unroll
          for (int k = 0; k < KB; ++k)
            if (k < K) {
              if (wv == 0) s_red[ch * K + k] = pw[k][i];
              else s_red[ch * K + k] += pw[k][i];
            }
        }
      }
      if (lane == 0) s_red[oe + wv] = pe;
    }
    __syncthreads();
  }
  // row layout [dW (D*K, [c][k]) | db (D) | sum over nodes and channels of dz*x (1) | unused]
  if (threadIdx.x == 0) {
    double e = 0.0;
    for (int wv = 0; wv < kWaves; ++wv) e += s_red[oe + wv];
    s_red[oe] = e;
  }
  __syncthreads();
  double* out = partials + (size_t)vb * (size_t)(K + 2) * D;
  for (int i = threadIdx.x; i <= oe; i += kThreads) out[i] = s_red[i];
}

// Finish of the partials (k_colsum_fin<4>): workgroups b < nb-1 own 4 of the (K + 1) D
// columns [dW | db]; the last one reduces the per-block eps column.
constexpr int kEkFinCols = 4;
struct MpBwdEkFin {
  float *dlin_w, *dlin_b, *deps;
  int DK, cols, nb;  // D*K, D*(K+1)
  __device__ int col(int b, int j) const {
    if (b == nb - 1) return j == 0 ? cols : -1;
    const int c = kEkFinCols * b + j;
    return c < cols ? c : -1;
  }
  __device__ void finish(int b, const double* tot) const {
    const int t = threadIdx.x;
    if (b == nb - 1) {
      if (t == 0) deps[0] = (float)tot[0];
      return;
    }
    const int c = kEkFinCols * b + t;
    if (t >= kEkFinCols || c >= cols) return;
    if (c < DK) dlin_w[c] = (float)tot[t];
    else dlin_b[c - DK] = (float)tot[t];
  }
};

// ----------------------------------------------------------------------------------------
// Host dispatch
// ----------------------------------------------------------------------------------------
// D % 4 == 0 and D <= 256: one float4 per lane (the C == 1 shapes of gine_mp.hip)
inline bool pick_group(int D, int* L) {
  if (D <= 0 || D % 4 != 0 || D > 256) return false;
  int l = 1;
  while (l < D / 4) l <<= 1;
  *L = l;
  return true;
}

inline int bucket(int K) { return K <= 1 ? 1 : (K <= 2 ? 2 : (K <= 4 ? 4 : 8)); }

// load_w_ek's float4 form applies
inline int w_vec(const float* lin_w, int K) {
  return K == bucket(K) && (reinterpret_cast<uintptr_t>(lin_w) & 15) == 0;
}

inline int nodes_per_block(int L) { return kWaves * (kWave / L); }

inline int bwd_grid(int64_t N, int L) {
  const int64_t tiles = ceil_div(N, nodes_per_block(L));
  const int64_t g = tiles < 1024 ? tiles : 1024;  // persistent grid cap, as gine_mp_bwd
  return (int)(g > 0 ? g : 1);
}

inline int check_sizes(int64_t N, int64_t E, int D, int K, int* L) {
  if (K < 1 || K > GINE_MP_MAX_EDGE_DIM) return GINE_ERR_INVALID;
  if (!pick_group(D, L)) return GINE_ERR_DIM;
  if (N < 0 || E < 0) return GINE_ERR_INVALID;
  if (N * D * 4 >= (int64_t(1) << 32) || E * K * 4 >= (int64_t(1) << 32))
    return GINE_ERR_TOO_LARGE;
  return GINE_OK;
}

#define GINE_EK_DISPATCH_KB(L_, KB, MACRO)                                      \
  switch (KB) {                                                                 \
    case 1: MACRO(L_, 1); break;                                                \
    case 2: MACRO(L_, 2); break;                                                \
    case 4: MACRO(L_, 4); break;                                                \
    default: MACRO(L_, 8); break;                                               \
  }

#define GINE_EK_DISPATCH(L, KB, MACRO)                                          \
  switch (L) {                                                                  \
    case 1: GINE_EK_DISPATCH_KB(1, KB, MACRO) break;                            \
    case 2: GINE_EK_DISPATCH_KB(2, KB, MACRO) break;                            \
    case 4: GINE_EK_DISPATCH_KB(4, KB, MACRO) break;                            \
    case 8: GINE_EK_DISPATCH_KB(8, KB, MACRO) break;                            \
    case 16: GINE_EK_DISPATCH_KB(16, KB, MACRO) break;                          \
    case 32: GINE_EK_DISPATCH_KB(32, KB, MACRO) break;                          \
    default: GINE_EK_DISPATCH_KB(64, KB, MACRO) break;                          \
  }

}  // namespace
}  // namespace gine

using namespace gine;

extern "C" int gine_mp_fwd_ek(const float* x, const int32_t* in_rowptr, const int32_t* in_src,
                              const float* in_attr, const float* lin_w, const float* lin_b,
                              const float* eps, float* z, int64_t num_nodes, int64_t num_edges,
                              int32_t channels, int32_t edge_dim, void* stream) {
  int L;
  const int st = check_sizes(num_nodes, num_edges, channels, edge_dim, &L);
  if (st != GINE_OK) return st;
  if (num_nodes == 0) return GINE_OK;
  if (!x || !in_rowptr || !lin_w || !lin_b || !eps || !z) return GINE_ERR_INVALID;
  if (num_edges > 0 && (!in_src || !in_attr)) return GINE_ERR_INVALID;
  const int D4 = channels / 4, KB = bucket(edge_dim);
  const int64_t tiles = ceil_div(num_nodes, nodes_per_block(L));
  hipStream_t s = as_stream(stream);
#define LAUNCH_FWD(L_, KB_)                                                                   \
  hipLaunchKernelGGL((k_mp_fwd_ek<L_, KB_>), dim3((unsigned)tiles), dim3(kThreads), 0, s,      \
                     (const float4*)x, in_rowptr, in_src, in_attr, lin_w,                      \
                     (const float4*)lin_b, eps, (float4*)z, num_nodes, D4, (int)edge_dim,      \
                     w_vec(lin_w, edge_dim))
  GINE_EK_DISPATCH(L, KB, LAUNCH_FWD)
#undef LAUNCH_FWD
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_mp_bwd_ek_num_partials(int64_t num_nodes, int32_t channels,
                                           int32_t edge_dim, int32_t* num_partials) {
  int L;
  if (!num_partials) return GINE_ERR_INVALID;
  const int st = check_sizes(num_nodes, 0, channels, edge_dim, &L);
  if (st != GINE_OK) return st;
  *num_partials = bwd_grid(num_nodes, L);
  return GINE_OK;
}

extern "C" int gine_mp_bwd_ek(const float* dz, const float* x, const int32_t* out_rowptr,
                              const int32_t* out_dst, const float* out_attr,
                              const int32_t* out_eid, const float* lin_w, const float* lin_b,
                              const float* eps, const float* dres, float* dx, float* dea,
                              double* partials, int64_t num_nodes, int64_t num_edges,
                              int32_t channels, int32_t edge_dim, int32_t flags, void* stream) {
  int L;
  const int st = check_sizes(num_nodes, num_edges, channels, edge_dim, &L);
  if (st != GINE_OK) return st;
  if ((flags & ~GINE_MP_BWD_SELF) != 0) return GINE_ERR_INVALID;
  if (num_nodes == 0) return GINE_OK;  // nothing launched, no partial row written
  if (!dz || !x || !out_rowptr || !lin_w || !lin_b || !eps || !dx || !partials)
    return GINE_ERR_INVALID;
  if (num_edges > 0 && (!out_dst || !out_attr || (dea && !out_eid))) return GINE_ERR_INVALID;
  const int D4 = channels / 4, KB = bucket(edge_dim);
  const int grid = bwd_grid(num_nodes, L);
  const int tiles = (int)ceil_div(num_nodes, nodes_per_block(L));
  const size_t smem = sizeof(double) * ((size_t)(edge_dim + 1) * channels + kWaves);
  hipStream_t s = as_stream(stream);
  const bool eattr = dea != nullptr && num_edges > 0;
#define LAUNCH_BWD_E(L_, KB_, E_)                                                             \
  hipLaunchKernelGGL((k_mp_bwd_ek<L_, KB_, E_>), dim3((unsigned)grid), dim3(kThreads), smem, s, \
                     (const float4*)dz, (const float4*)x, out_rowptr, out_dst, out_attr,       \
                     out_eid, lin_w, (const float4*)lin_b, eps, (const float4*)dres,           \
                     (float4*)dx, dea, partials, num_nodes, D4, (int)edge_dim,                 \
                     w_vec(lin_w, edge_dim), tiles, (int)flags)
#define LAUNCH_BWD_T(L_, KB_) LAUNCH_BWD_E(L_, KB_, true)
#define LAUNCH_BWD_F(L_, KB_) LAUNCH_BWD_E(L_, KB_, false)
  if (eattr) {
    GINE_EK_DISPATCH(L, KB, LAUNCH_BWD_T)
  } else {
    GINE_EK_DISPATCH(L, KB, LAUNCH_BWD_F)
  }
#undef LAUNCH_BWD_T
#undef LAUNCH_BWD_F
#undef LAUNCH_BWD_E
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_mp_bwd_ek_finalize(const double* partials, int32_t num_partials,
                                       int32_t channels, int32_t edge_dim, float* dlin_w,
                                       float* dlin_b, float* deps, void* stream) {
  if (edge_dim < 1 || edge_dim > GINE_MP_MAX_EDGE_DIM) return GINE_ERR_INVALID;
  int L;
  if (!pick_group(channels, &L)) return GINE_ERR_DIM;
  if (num_partials < 0) return GINE_ERR_INVALID;
  if (!partials || !dlin_w || !dlin_b || !deps) return GINE_ERR_INVALID;
  const int cols = (edge_dim + 1) * channels;
  const int nb = (int)ceil_div(cols, kEkFinCols) + 1;
  const MpBwdEkFin fin{dlin_w, dlin_b, deps, edge_dim * channels, cols, nb};
  hipLaunchKernelGGL((k_colsum_fin<kEkFinCols, MpBwdEkFin>), dim3(nb), dim3(256), 0,
                     as_stream(stream), partials, num_partials, (edge_dim + 2) * channels, fin);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}
