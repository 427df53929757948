// The dense layers between the DeepSet member sum and the GINE stack, fused on gfx950.
//
// Replaces (models/gnn.py:48-68, 112-113, 132-135; phi's last Linear applied after the
// member sum, see raincast_gnn/models.py DeepSetEncoder):
//   s  = r Wp2^T + M bp2          phi[2] (member-summed)
//   u  = relu(s Wr0^T + br0)      rho[0], rho[1]
//   e  = u Wr1^T + br1            rho[2]           (the DeepSet embedding)
//   h0 = [x | e] Wdr^T + bdr      dim_red(cat([x, emb], 1))
// which the reference runs as four library GEMMs, a ReLU and a concatenation forward and
// four input-gradient GEMMs, four weight-gradient GEMMs, a ReLU backward and a split
// backward.
//
// Here the chain is folded twice.  Only one nonlinearity sits in it, so the two Linears
// before the ReLU are one Linear, and so are the two after it:
//   u  = relu(r Wf^T + bf),   Wf = Wr0 Wp2,             bf = M Wr0 bp2 + br0
//   h0 = [x | u] W'^T + b',   W' = [Wdr_x | Wdr_e Wr1], b' = Wdr_e br1 + bdr
// Both folds are made from the current weights by extra workgroups of the DeepSet forward
// (gine_deepset_fwd_fold2, gine_chainfold.hpp): wfold = [W' | b' | W'^T], wfold2 = [Wf | bf].
// Neither s, e nor their gradients are formed:
//   forward   one 2-stage row-chain launch: r -> u -> h0          (gine_chain_fwd_folded2)
//   backward  one 2-stage row-chain launch: dt = (dh0 Wc) * 1[u > 0] -> dr = dt Wf, with
//             Wc = the last D columns of W'                       (gine_chain_bwd_folded2)
//   weights   one engine launch (gine_wgrad.hpp, Z = 2): G = dh0^T [x | u] (+ g = sum dh0)
//             and G2 = dt^T r (+ g2 = sum dt), one fixed-order slab reduction, and one small
//             launch that unfolds them into the eight parameter gradients
//             (gine_chain_wgrad_folded2, gine_chain_unfold_grads2):
//               dWdr = [G_x | G_u Wr1^T + g br1^T], dbdr = g, dWr1 = Wdr_e^T G_u,
//               dbr1 = Wdr_e^T g, dWr0 = G2 Wp2^T + M g2 bp2^T, dbr0 = g2,
//               dWp2 = Wr0^T G2, dbp2 = M Wr0^T g2.
// The unfolded chain stays as the comparator the tests hold the folded one against
// (raincast_gnn.chain.FOLD = False; measured slower): two 2-stage launches
// forward (F1: s, u; F2: e, h0), two backward (B1: de, dt; B2: ds, dr) and the four
// weight-gradient products in one engine launch (gine_chain_fwd / _bwd / _wgrad).
// (What else was tried -- the single fold in two and in one launch, the row stages on the
// bf16 matrix cores -- and what it measured: DESIGN.md.)
//
// Row-chain kernel: a workgroup of D/32 waves walks 32-row tiles (persistent, XCD-local
// tile ranges).  Both stages' weight fragments live in VGPRs (loaded once per workgroup);
// stage 1 reads its A tile from LDS (staged from HBM with the next tile's raw rows in
// flight), writes its output both to HBM (saved for the backward) and to a second LDS
// tile, which is stage 2's A operand -- the intermediate never round-trips through HBM
// between the two GEMMs.  The MFMA layout and the lane-half k split are k_rowgemm's
// (gine_mlp.hip): lane half h contracts k in [h*K/2, (h+1)*K/2), A fragments read as
// ds_read_b128 from rows padded by 4 floats.
#include "gine_common.hpp"
#include "gine_slab.hpp"
#include "gine_wgrad.hpp"
#include "gine_chainfold.hpp"
#include "gine_chainrow.hpp"  // tile_mma, frag_n

#include <algorithm>

namespace gine {
namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kRowTile = 32;

#ifdef GINE_CHAIN_PROFILE
// Debug build only (make variant V=chainprof VSRC=gine_chain.hip VDEFS=-DGINE_CHAIN_PROFILE,
// tools/chain_prof.py): thread 0 of every workgroup of the two-stage chain kernels stamps
// s_memtime: 0 entry, 1 weight fragments issued, then per tile k < 2 at 2 + 4k: A tile
// staged (after the barrier), 3 + 4k: stage 1 done, 4 + 4k: stage-2 A tile complete (after
// the barrier), 5 + 4k: stage 2 done; 10 end; 11 / 12: s_memrealtime at entry / end.
__device__ long long g_chain_prof[1024][16];
#define CHAIN_MARK(i)                                                          \
  do {                                                                         \
    if (threadIdx.x == 0 && blockIdx.x < 1024)                                 \
      g_chain_prof[blockIdx.x][i] = (long long)__builtin_amdgcn_s_memtime();  \
  } while (0)
#define CHAIN_RT(i)                                                            \
  do {                                                                         \
    if (threadIdx.x == 0 && blockIdx.x < 1024)                                 \
      g_chain_prof[blockIdx.x][i] = (long long)__builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define CHAIN_MARK(i) do {} while (0)
#define CHAIN_RT(i) do {} while (0)
#endif

// The doubly folded chain's two launches (F2D, B2D) and the unfolded chain's four:
//   F2D: u  = relu(r Wf^T + bf)     -> h0 = [x | u] W'^T + b'
//   B2D: dt = (dh0 Wc) * 1[u > 0]   -> dr = dt Wf
//   F1:  s  = r Wp2^T + M bp2       -> u  = relu(s Wr0^T + br0)
//   F2:  e  = u Wr1^T + br1         -> h0 = [x | e] Wdr^T + bdr
//   B1:  de = dh0 Wdr[:, F:]        -> dt = (de Wr1) * 1[u > 0]
//   B2:  ds = dt Wr0                -> dr = ds Wp2
enum ChainKind { CH_F2D, CH_B2D, CH_F1, CH_F2, CH_B1, CH_B2 };

struct ChainArgs {
  const float* in;   // stage-1 A rows [N, D]: r | dh0 | r | u | dh0 | dt
  const float* x;    // F2D / F2: node features [N, F]
  const float* aux;  // B2D / B1: u (the ReLU mask)
  const float* w1;   // stage-1 weight (B2D: W', B1: Wdr -- their last D columns)
  const float* b1;   // stage-1 bias (forward)
  const float* w2;   // stage-2 weight (not F2D)
  const float* b2;   // stage-2 bias (F1, F2)
  float* out1;       // stage-1 output [N, D]: u | dt | s | e | de | ds
  float* out2;       // stage-2 output [N, D]: - | dr | u | h0 | dt | dr
  float bias1_scale; // F1: M (phi[2]'s bias summed over members); else 1
  int F;             // x width
  const float* w3;   // F2D: last-stage weight W'^T
  float* out3;       // F2D: h0
  const float* b3;   // F2D: b'
};

__device__ __forceinline__ floatx16 zero16() {
  floatx16 v;
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = 0.f;
  return v;
}

// Y = X W^T fragment: bf[s] = W[col][h*KS + s]  (W row-major [*, ldw])
template <int K>
__device__ __forceinline__ void frag_t(float (&bf)[K / 2], const float* W, int ldw, int col,
                                       int h) {
  constexpr int KS = K / 2;
#pragma unroll
  for (int s = 0; s < KS; ++s) bf[s] = W[(size_t)col * ldw + h * KS + s];
}
// The same in 16-byte vectors (W 16-byte aligned, ldw % 4 == 0): a lane's fragment is
// KS consecutive floats of one row of W, so a wave's load touches 64 rows either way, but
// with a quarter of the load instructions (measured: the scalar form costs ~0.05 us per
// instruction and workgroup in the chain kernels).
template <int K>
__device__ __forceinline__ void frag_t4(float (&bf)[K / 2], const float* W, int ldw, int col,
                                        int h) {
  constexpr int KS = K / 2;
  const float4* row = reinterpret_cast<const float4*>(W + (size_t)col * ldw + h * KS);
#pragma unroll
  for (int s = 0; s < KS / 4; ++s) {
    const float4 v = row[s];
    bf[4 * s] = v.x;
    bf[4 * s + 1] = v.y;
    bf[4 * s + 2] = v.z;
    bf[4 * s + 3] = v.w;
  }
}
// dim_red's weight [D][F + D] seen on the padded k axis [x (F) | 0 (FP - F) | e (D)]
template <int FP, int D>
__device__ __forceinline__ void frag_dimred(float (&bf)[(FP + D) / 2], const float* W, int F,
                                            int col, int h) {
  constexpr int KS = (FP + D) / 2;
  const int ldw = F + D;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = h * KS + s;
    const int c = k < F ? k : (k < FP ? 0 : k - FP + F);
    const float v = W[(size_t)col * ldw + c];
    bf[s] = (k >= F && k < FP) ? 0.f : v;
  }
}
// The same from W^T [F + D][D] (the folded W'^T): lanes read consecutive columns.
template <int FP, int D>
__device__ __forceinline__ void frag_dimred_t(float (&bf)[(FP + D) / 2], const float* WT, int F,
                                              int col, int h) {
  constexpr int KS = (FP + D) / 2;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = h * KS + s;
    const int c = k < F ? k : (k < FP ? 0 : k - FP + F);
    const float v = WT[(size_t)c * D + col];
    bf[s] = (k >= F && k < FP) ? 0.f : v;
  }
}

// Per-XCD contiguous tile ranges (as k_rowgemm).
struct TileRange {
  int first, end, step;
};
__device__ __forceinline__ TileRange tile_range(int num_tiles, int nb) {
  const int xcd = blockIdx.x % kNumXcd, pos = blockIdx.x / kNumXcd;
  const int here = nb / kNumXcd + (xcd < nb % kNumXcd ? 1 : 0);
  const int span = (num_tiles + kNumXcd - 1) / kNumXcd;
  const int b = xcd * span;
  return TileRange{b + pos, min(num_tiles, b + span), here};
}

template <int D, int FP, int KIND>
__global__ __launch_bounds__(2 * D) void k_chain(ChainArgs a, int64_t N, int num_tiles) {
  constexpr int NT = 2 * D;
  constexpr int D4 = D / 4;
  constexpr int LDA = D + 4;
  constexpr bool kDimRed = KIND == CH_F2;
  constexpr int K2 = kDimRed ? FP + D : D;          // stage-2 contraction length
  constexpr int LDB = K2 + 4;
  constexpr int BOFF = kDimRed ? FP : 0;            // stage-1 output column offset in sB
  constexpr int ITEMS = kRowTile * D4 / NT;         // 4
  constexpr int RSTEP = NT / D4;                    // 8
  constexpr int XITEMS = (kRowTile * FP + NT - 1) / NT;
  constexpr bool kF2D = KIND == CH_F2D, kB2D = KIND == CH_B2D;
  constexpr bool kMask = KIND == CH_B1 || kB2D;     // reads u for the ReLU mask
  constexpr bool kX = kDimRed || kF2D;              // stages x rows
  constexpr int LDC = FP + D + 4;                   // F2D: last stage's A tile [x | u]
  __shared__ __attribute__((aligned(16))) float sA[kRowTile * LDA];
  __shared__ __attribute__((aligned(16))) float sB[kF2D ? 4 : kRowTile * LDB];
  __shared__ __attribute__((aligned(16))) float sC[kF2D ? kRowTile * LDC : 4];

  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int h = lane >> 5, c32 = lane & 31;
  const int col = wave * 32 + c32;
  const int q_me = threadIdx.x % D4, r_me = threadIdx.x / D4;
  CHAIN_RT(11);
  CHAIN_MARK(0);
  const int nb = gridDim.x;

  // the stages' weight fragments, once per workgroup
  float bf1[D / 2], bf2[K2 / 2];
  const bool w16 =
      ((reinterpret_cast<uintptr_t>(a.w1) | reinterpret_cast<uintptr_t>(a.w2)) & 15) == 0;
  if constexpr (KIND == CH_F1) {
    if (w16) {
      frag_t4<D>(bf1, a.w1, D, col, h);
      frag_t4<D>(bf2, a.w2, D, col, h);
    } else {
      frag_t<D>(bf1, a.w1, D, col, h);
      frag_t<D>(bf2, a.w2, D, col, h);
    }
  } else if constexpr (kF2D) {
    if (w16) frag_t4<D>(bf1, a.w1, D, col, h);
    else frag_t<D>(bf1, a.w1, D, col, h);
  } else if constexpr (KIND == CH_F2) {
    frag_t<D>(bf1, a.w1, D, col, h);
  } else if constexpr (kMask) {
    frag_n<D>(bf1, a.w1, a.F + D, a.F, col, h);     // dim_red (B2D: W') weight, e columns
  } else if constexpr (KIND == CH_B2) {
    frag_n<D>(bf1, a.w1, D, 0, col, h);
  }
  if constexpr (KIND == CH_F2) {
    frag_dimred<FP, D>(bf2, a.w2, a.F, col, h);
  } else if constexpr (KIND == CH_B1 || KIND == CH_B2 || kB2D) {
    frag_n<D>(bf2, a.w2, D, 0, col, h);   // B2D: w2 = Wf
  }
  float bf3[kF2D ? (FP + D) / 2 : 1];
  if constexpr (kF2D) frag_dimred_t<FP, D>(bf3, a.w3, a.F, col, h);  // w3 = W'^T
  float bias1 = 0.f, bias2 = 0.f, bias3 = 0.f;
  if constexpr (KIND == CH_F1 || KIND == CH_F2 || kF2D) bias1 = a.b1[col] * a.bias1_scale;
  if constexpr (KIND == CH_F1 || kDimRed) bias2 = a.b2[col];
  if constexpr (kF2D) bias3 = a.b3[col];
  CHAIN_MARK(1);

  auto load_tile = [&](int tile, float4 (&raw)[ITEMS], float (&xr)[XITEMS]) {
    const int64_t n0 = (int64_t)tile * kRowTile;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      int64_t n = n0 + r_me + i * RSTEP;
      n = n < N ? n : N - 1;  // clamped: always issued
      raw[i] = reinterpret_cast<const float4*>(a.in + n * D)[q_me];
    }
    if constexpr (kX) {
#pragma unroll
      for (int i = 0; i < XITEMS; ++i) {
        const int idx = threadIdx.x + i * NT;      // over [32][FP]
        const int r = idx / FP, c = idx % FP;
        int64_t n = n0 + r;
        n = n < N ? n : N - 1;
        // raw value only: the padding columns are zeroed at the LDS store (a select right
        // behind the load would make the compiler wait for it here, ending the prefetch)
        xr[i] = a.x[n * a.F + min(c, a.F - 1)];
      }
    }
  };

  const TileRange tr = tile_range(num_tiles, nb);
  float4 raw[ITEMS];
  float xr[XITEMS];
  if (tr.first < tr.end) load_tile(tr.first, raw, xr);
  int kt = 0;  // (profile stamps) tile index of this workgroup
  for (int tile = tr.first; tile < tr.end; tile += tr.step, ++kt) {
    const int64_t n0 = (int64_t)tile * kRowTile;
    float ep[16];
    if constexpr (kMask) {
      // the ReLU mask, in flight under the staging and stage 1 -- issued before the next
      // tile's rows, so the epilogue's wait for it (vector-memory counts retire in order)
      // does not also wait for that prefetch
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int64_t n = n0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        n = n < N ? n : N - 1;
        ep[r] = a.aux[n * D + col];
      }
    }
    __syncthreads();  // previous tile's reads of sA / sB / sC are done
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      const int r = r_me + i * RSTEP;
      const float4 v = (n0 + r < N) ? raw[i] : f4_zero();
      float* dst = &sA[r * LDA + 4 * q_me];
      *reinterpret_cast<float4*>(dst) = v;
    }
    if constexpr (kX) {
      float* sx = kF2D ? sC : sB;
      constexpr int LDX = kF2D ? LDC : LDB;
#pragma unroll
      for (int i = 0; i < XITEMS; ++i) {
        const int idx = threadIdx.x + i * NT;
        if (idx < kRowTile * FP) sx[(idx / FP) * LDX + idx % FP] = idx % FP < a.F ? xr[i] : 0.f;
      }
    }
    __syncthreads();
    if (kt < 2) CHAIN_MARK(2 + 4 * kt);
    if (tile + tr.step < tr.end) load_tile(tile + tr.step, raw, xr);  // next tile in flight

    // stage 1
    floatx16 acc;
    acc = tile_mma<D>(sA, LDA, bf1, c32, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = (r & 3) + 8 * (r >> 2) + 4 * h;
      const int64_t n = n0 + rr;
      float v = acc[r] + bias1;
      if constexpr (kB2D) v = ep[r] > 0.f ? acc[r] : 0.f;      // dt = du * 1[u > 0]
      if constexpr (kF2D) {
        v = relu_nan(v);                                       // u = relu(r Wf^T + bf)
        sC[rr * LDC + FP + col] = v;                           // the last stage's A tile
      } else {
        sB[rr * LDB + BOFF + col] = v;
      }
      if (n < N) a.out1[n * D + col] = v;
    }
    if (kt < 2) CHAIN_MARK(3 + 4 * kt);
    __syncthreads();
    if (kt < 2) CHAIN_MARK(4 + 4 * kt);

    // stage 2
    if constexpr (!kF2D) {
      acc = tile_mma<K2>(sB, LDB, bf2, c32, h);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = (r & 3) + 8 * (r >> 2) + 4 * h;
        const int64_t n = n0 + rr;
        float v = acc[r] + bias2;
        if constexpr (KIND == CH_F1) v = relu_nan(v);             // u = relu(rho[0](s))
        if constexpr (KIND == CH_B1) v = ep[r] > 0.f ? v : 0.f;   // dt = du * 1[u > 0]
        if (n < N) a.out2[n * D + col] = v;
      }
    } else {  // h0 = [x | u] W'^T + b'
      acc = tile_mma<FP + D>(sC, LDC, bf3, c32, h);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t n = n0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (n < N) a.out3[n * D + col] = acc[r] + bias3;
      }
    }
    if (kt < 2) CHAIN_MARK(5 + 4 * kt);
  }
  CHAIN_MARK(10);
  CHAIN_RT(12);
}

// Persistent grid, one workgroup per CU (two per CU measured slower at cfg2: 0.614 vs
// 0.589 ms per step).
inline int chain_grid(int64_t N) {
  const int64_t tiles = ceil_div(N, kRowTile);
  return (int)std::max<int64_t>(1, std::min<int64_t>(tiles, kNumCu));
}

template <int D, int FP, int KIND>
int launch_chain(const ChainArgs& a, int64_t N, hipStream_t s) {
  const int tiles = (int)ceil_div(N, kRowTile);
  hipLaunchKernelGGL((k_chain<D, FP, KIND>), dim3(chain_grid(N)), dim3(2 * D), 0, s, a, N,
                     tiles);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

// ----------------------------------------------------------------------------------------
// weight gradients, one engine launch (each product with its column sum behind it)
//   NZ = 2 (doubly folded): z = 0: G = dh0^T [x | u] [D x (F+D)]   z = 1: G2 = dt^T r [D x D]
//                           (the eight parameter gradients follow in gine_chain_unfold_grads2)
//   NZ = 4 (unfolded):      z = 0: dWdr = dh0^T [x | e]   z = 1: dWr1 = de^T u
//                           z = 2: dWr0 = dt^T s          z = 3: dWp2 = ds^T r
// ----------------------------------------------------------------------------------------
template <int NZ>
struct ChainWgradSrc {
  static constexpr int kZ = NZ;
  const float* p[NZ];  // P rows [N, D] of product z
  const float* q[NZ];  // Q rows [N, D] of product z (z = 0: the D columns after x)
  const float* x;
  int D, F;
  struct Raw {
    float4 v;
  };
  struct Col {
    float keep[4];  // Q of z = 0: 1 for the columns inside [x | .], 0 for the padding
  };
  template <int Z> __device__ int i_dim(int) const { return Z == 0 ? F + D : D; }
  template <int Z> __device__ Col p_col(int) const { return Col{{1.f, 1.f, 1.f, 1.f}}; }
  template <int Z> __device__ Col q_col(int q4) const {
    Col c{{1.f, 1.f, 1.f, 1.f}};
    if constexpr (Z == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) c.keep[j] = 4 * q4 + j < F + D ? 1.f : 0.f;
    }
    return c;
  }
  template <int Z> __device__ Raw p_load(int64_t n, int q4) const {
    return Raw{reinterpret_cast<const float4*>(p[Z] + n * D)[q4]};
  }
  template <int Z> __device__ Raw q_load(int64_t n, int q4) const {
    if constexpr (Z == 0) {  // [x | q0]: F + D columns, x rows are not float4-aligned
      const int I = F + D;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = min(4 * q4 + j, I - 1);
        const float* src = c < F ? x + n * F + c : q[0] + n * D + (c - F);
        v[j] = *src;  // raw: the padding is zeroed in q_xform, when the tile is staged
      }
      return Raw{make_float4(v[0], v[1], v[2], v[3])};
    } else {
      return Raw{reinterpret_cast<const float4*>(q[Z] + n * D)[q4]};
    }
  }
  template <int Z> __device__ float4 p_xform(const Raw& r, const Col&) const { return r.v; }
  template <int Z> __device__ float4 q_xform(const Raw& r, const Col& c) const {
    if constexpr (Z == 0)
      return make_float4(c.keep[0] != 0.f ? r.v.x : 0.f, c.keep[1] != 0.f ? r.v.y : 0.f,
                         c.keep[2] != 0.f ? r.v.z : 0.f, c.keep[3] != 0.f ? r.v.w : 0.f);
    return r.v;
  }
};

struct ChainWgradOut {
  float* w[4];  // product order of ChainWgradSrc
  float* b[4];
  int D, F;
  float bscale3;  // unfolded: phi[2]'s bias gradient (product 3) enters M times
  __device__ void operator()(int z, int64_t e, double v) const {
    const int64_t I = z == 0 ? F + D : D;
    const int64_t ws = (int64_t)D * I;
    if (e < ws) {
      w[z][e] = (float)v;
    } else if (e < ws + D && b[z] != nullptr) {
      b[z][e - ws] = (float)(z == 3 ? v * (double)bscale3 : v);
    }
  }
};

// The engine launch's shape and its slab for nz products: what gine_chain_bwd_slab_floats
// sizes, the weight-gradient entry points launch and the slab jobs reduce all come from
// here, so the allocation and the writes cannot disagree.
struct ChainWgradShape {
  WgPlan plan;
  int nz;
  int tiles;    // output tiles: one [D x (F+D)] product plus nz - 1 [D x D]
  size_t per;   // floats of one chunk of one product (the first's size; the others use its head)
  size_t zstride() const { return per * plan.chunks; }
  size_t slab_floats() const { return nz * zstride(); }
};
inline ChainWgradShape chain_wgrad_shape(int64_t N, int D, int F, int nz) {
  const int to = (int)ceil_div(D, 64);
  ChainWgradShape s;
  s.nz = nz;
  s.tiles = to * (int)ceil_div(F + D, kWgTI) + (nz - 1) * to * (int)ceil_div(D, kWgTI);
  s.plan = wg_plan(N, D, F + D, nz, 64, s.tiles);
  s.per = (size_t)D * (D + F) + D;
  return s;
}

// the slab job of either chain; w / b in product order
void chain_slab_job(const ChainWgradShape& sh, int D, int F, const float* slab, float bscale3,
                    float* const* w, float* const* b, gine_grad_job* job) {
  *job = gine_grad_job{};
  job->kind = GINE_GRAD_JOB_SLAB;
  job->src = slab;
  job->rows = sh.plan.chunks;
  job->cstride = (int64_t)sh.per;
  job->zstride = (int64_t)sh.zstride();
  job->nz = sh.nz;
  for (int z = 0; z < sh.nz; ++z) {
    const int64_t ws = (int64_t)D * (z == 0 ? F + D : D);
    job->per[z] = ws + D;
    job->wsize[z] = ws;
    job->w[z] = w[z];
    job->b[z] = b[z];
    job->bscale[z] = z == 3 ? bscale3 : 1.0f;
  }
}

inline bool chain_dims_ok(int D, int F) { return (D == 64 || D == 128) && F >= 1 && F <= 64; }

#define GINE_CHAIN_DISPATCH(D_, F_, CALL)                          \
  do {                                                             \
    if ((D_) == 64) {                                              \
      if ((F_) <= 40) { CALL(64, 40); } else { CALL(64, 64); }     \
    } else {                                                       \
      if ((F_) <= 40) { CALL(128, 40); } else { CALL(128, 64); }   \
    }                                                              \
  } while (0)

// One unfold job: G = gf ([D][F + D] then g [D]) of the product dY^T [x | q] where the
// rows of q feed a Linear (w1, bias b1 * bscale) whose output meets Wdr's q columns:
//   h0 = [x | u Wr1^T + br1] Wdr^T + bdr:   dWdr = [G_x | G_u Wr1^T + g br1^T], dbdr = g,
//                                           dWr1 = Wdr_e^T G_u, dbr1 = Wdr_e^T g,
// and the same with F = 0 for pre = (r Wp2^T + M bp2) Wr0^T + br0:
//   dWr0 = G2 Wp2^T + M g2 bp2^T, dbr0 = g2, dWp2 = Wr0^T G2, dbp2 = M Wr0^T g2.
struct UnfoldJob {
  const float *gf, *w1, *b1, *wdr;  // w1 [D][D]; wdr [D][F + D] (its last D columns used)
  float *dwdr, *dbdr, *dw1, *db1;
  int F;
  float bscale;
};

// 2 (D/32)^2 workgroups per job, one [32 x 32] tile each (ksplit_tile): tiles of dWdr's q
// columns, G_q W1^T + g (bscale b1)^T (G_q rows staged, B = W1^T read along W1's rows), then
// tiles of dW1 = Wdr_q^T G_q (Wdr_q columns staged as rows, B = G_q); the x columns and dbdr
// (resp. db1) by the tiles of column 0.
template <int D>
__global__ __launch_bounds__(2 * D) void k_chain_unfold(UnfoldJob j0, UnfoldJob j1) {
  constexpr int NT = 2 * D, LDA = D + 4, T = D / 32, TT = T * T;
  constexpr int SI = 32 * D / NT, XI = 32 * 64 / NT;
  __shared__ __attribute__((aligned(16))) float sA[32 * LDA];
  __shared__ float sR[T * kSR];
  __shared__ float svec[D];
  const bool second = (int)blockIdx.x >= 2 * TT;
  // field by field (uniform selects; no private copy of a kernel argument)
  const UnfoldJob J{second ? j1.gf : j0.gf,     second ? j1.w1 : j0.w1,
                    second ? j1.b1 : j0.b1,     second ? j1.wdr : j0.wdr,
                    second ? j1.dwdr : j0.dwdr, second ? j1.dbdr : j0.dbdr,
                    second ? j1.dw1 : j0.dw1,   second ? j1.db1 : j0.db1,
                    second ? j1.F : j0.F,       second ? j1.bscale : j0.bscale};
  const int blk = (int)blockIdx.x - (second ? 2 * TT : 0);
  const float* __restrict__ gf = J.gf;
  const int F = J.F;
  const int LW = F + D;
  const float* g = gf + (size_t)D * LW;
  const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int h = lane >> 5, c32 = lane & 31;
  const bool e_cols = blk < TT;
  const int t = e_cols ? blk : blk - TT;
  const int r0 = 32 * (t / T), c0 = 32 * (t % T);
  float bf[16], st[SI];
  if (e_cols) {
#pragma unroll
    for (int s = 0; s < 16; ++s) bf[s] = J.w1[(size_t)(c0 + c32) * D + w * 32 + h * 16 + s];
#pragma unroll
    for (int i = 0; i < SI; ++i) {
      const int idx = threadIdx.x + i * NT;
      st[i] = gf[(size_t)(r0 + idx / D) * LW + F + idx % D];
    }
    if (c0 == 0) {
      if (F > 0) {
        float xv[XI];
#pragma unroll
        for (int i = 0; i < XI; ++i) {
          const int idx = min(threadIdx.x + i * NT, 32 * F - 1);
          xv[i] = gf[(size_t)(r0 + idx / F) * LW + idx % F];
        }
#pragma unroll
        for (int i = 0; i < XI; ++i) {
          const int idx = threadIdx.x + i * NT;
          if (idx < 32 * F) J.dwdr[(size_t)(r0 + idx / F) * LW + idx % F] = xv[i];
        }
      }
      if (threadIdx.x < 32 && J.dbdr != nullptr) J.dbdr[r0 + threadIdx.x] = g[r0 + threadIdx.x];
    }
#pragma unroll
    for (int i = 0; i < SI; ++i) {
      const int idx = threadIdx.x + i * NT;
      sA[(idx / D) * LDA + idx % D] = st[i];
    }
  } else {
#pragma unroll
    for (int s = 0; s < 16; ++s)
      bf[s] = gf[(size_t)(w * 32 + h * 16 + s) * LW + F + c0 + c32];  // G_q[k][c0 + c32]
#pragma unroll
    for (int i = 0; i < SI; ++i) {
      const int idx = threadIdx.x + i * NT;
      st[i] = J.wdr[(size_t)(idx / 32) * LW + F + r0 + idx % 32];
    }
    const float gv = threadIdx.x < D ? g[threadIdx.x] : 0.f;
#pragma unroll
    for (int i = 0; i < SI; ++i) {
      const int idx = threadIdx.x + i * NT;
      sA[(idx % 32) * LDA + idx / 32] = st[i];
    }
    if (threadIdx.x < D) svec[threadIdx.x] = gv;
  }
  __syncthreads();
  ksplit_tile<D>(sA, bf, sR, c32, h);
  if (!e_cols && c0 == 0) {
    const float v = rows_dot<D>(sA, svec);  // (Wdr_q^T g)[r0 + r]
    constexpr int TPR = NT / 32;
    if (threadIdx.x % TPR == 0 && J.db1 != nullptr) J.db1[r0 + threadIdx.x / TPR] = v * J.bscale;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 1024 / NT; ++i) {
    const int o = threadIdx.x + i * NT, rr = o / 32, cc = o % 32;
    const float v = ksplit_sum<D>(sR, rr, cc);
    if (e_cols)
      J.dwdr[(size_t)(r0 + rr) * LW + F + c0 + cc] =
          fmaf(g[r0 + rr], J.b1[c0 + cc] * J.bscale, v);
    else
      J.dw1[(size_t)(r0 + rr) * D + c0 + cc] = v;
  }
}

int launch_unfold(int D, const UnfoldJob& j0, const UnfoldJob& j1, hipStream_t st) {
  if (D == 64)
    hipLaunchKernelGGL((k_chain_unfold<64>), dim3(2 * 2 * 4), dim3(128), 0, st, j0, j1);
  else
    hipLaunchKernelGGL((k_chain_unfold<128>), dim3(2 * 2 * 16), dim3(256), 0, st, j0, j1);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

}  // namespace
}  // namespace gine

using namespace gine;

extern "C" int gine_chain_bwd_slab_floats(int64_t num_nodes, int32_t hidden,
                                          int32_t in_features, size_t* floats) {
  if (!floats || num_nodes < 0) return GINE_ERR_INVALID;
  if (!chain_dims_ok(hidden, in_features)) return GINE_ERR_DIM;
  // enough for either chain (2 products folded, 4 unfolded)
  *floats = std::max(chain_wgrad_shape(num_nodes, hidden, in_features, 2).slab_floats(),
                     chain_wgrad_shape(num_nodes, hidden, in_features, 4).slab_floats());
  return GINE_OK;
}

extern "C" int gine_chain_fwd_folded2(const float* r, const float* x, const float* wfold,
                                      const float* wfold2, float* u, float* h0,
                                      int64_t num_nodes, int32_t hidden, int32_t in_features,
                                      void* stream) {
  if (!chain_dims_ok(hidden, in_features)) return GINE_ERR_DIM;
  if (num_nodes < 0) return GINE_ERR_INVALID;
  if (num_nodes >= (int64_t(1) << 31)) return GINE_ERR_TOO_LARGE;
  if (num_nodes == 0) return GINE_OK;
  if (!r || !x || !wfold || !wfold2 || !u || !h0) return GINE_ERR_INVALID;
  hipStream_t st = as_stream(stream);
  const int D = hidden, F = in_features;
  const float* bfold = wfold + (size_t)D * (F + D);
  ChainArgs f{r, x, nullptr, wfold2, wfold2 + (size_t)D * D, nullptr, nullptr, u, nullptr,
              1.f, F};
  f.w3 = bfold + D;  // W'^T
  f.b3 = bfold;
  f.out3 = h0;
  int rc = GINE_OK;
#define CALL_F(DD, FF) rc = launch_chain<DD, FF, CH_F2D>(f, num_nodes, st)
  GINE_CHAIN_DISPATCH(D, F, CALL_F);
#undef CALL_F
  return rc;
}

extern "C" int gine_chain_bwd_folded2(const float* dh0, const float* u, const float* wfold,
                                      const float* wfold2, float* dt, float* dr,
                                      int64_t num_nodes, int32_t hidden, int32_t in_features,
                                      void* stream) {
  if (!chain_dims_ok(hidden, in_features)) return GINE_ERR_DIM;
  if (num_nodes <= 0) return GINE_ERR_INVALID;
  if (num_nodes >= (int64_t(1) << 31)) return GINE_ERR_TOO_LARGE;
  if (!dh0 || !u || !wfold || !wfold2 || !dt || !dr) return GINE_ERR_INVALID;
  hipStream_t st = as_stream(stream);
  const int F = in_features;
  const ChainArgs b{dh0, nullptr, u, wfold, nullptr, wfold2, nullptr, dt, dr, 1.f, F};
  int rc = GINE_OK;
#define CALL_B(DD, FF) rc = launch_chain<DD, FF, CH_B2D>(b, num_nodes, st)
  GINE_CHAIN_DISPATCH(hidden, F, CALL_B);
#undef CALL_B
  return rc;
}

extern "C" int gine_chain_wgrad_folded2(const float* dh0, const float* x, const float* r,
                                        const float* u, const float* dt, float* slab,
                                        float* gfold, float* g2fold, int64_t num_nodes,
                                        int32_t hidden, int32_t in_features, void* stream) {
  if (!chain_dims_ok(hidden, in_features)) return GINE_ERR_DIM;
  if (num_nodes <= 0) return GINE_ERR_INVALID;
  if (!dh0 || !x || !r || !u || !dt || !slab) return GINE_ERR_INVALID;
  // gfold, g2fold both NULL: the slab is left for gine_grad_finalize_batch
  const bool reduce = gfold || g2fold;
  if (reduce && (!gfold || !g2fold)) return GINE_ERR_INVALID;
  hipStream_t st = as_stream(stream);
  const int D = hidden, F = in_features;
  const ChainWgradShape sh = chain_wgrad_shape(num_nodes, D, F, 2);
  const ChainWgradSrc<2> src{{dh0, dt}, {u, r}, x, D, F};
  int rc = launch_wgrad_engine<64>(src, num_nodes, D, D + F, sh.tiles, sh.plan, sh.zstride(),
                                   sh.per, slab, st);
  if (rc != GINE_OK || !reduce) return rc;
  return launch_slab_sum(slab, sh.plan.chunks, (int64_t)sh.per, sh.per, sh.zstride(), sh.nz,
                         ChainWgradOut{{gfold, g2fold, nullptr, nullptr},
                                       {gfold + (size_t)D * (F + D), g2fold + (size_t)D * D,
                                        nullptr, nullptr},
                                       D, F, 1.f},
                         st);
}

extern "C" int gine_chain_wgrad_folded2_grad_job(int64_t num_nodes, int32_t hidden,
                                                 int32_t in_features, const float* slab,
                                                 float* gfold, float* g2fold,
                                                 gine_grad_job* job) {
  if (!chain_dims_ok(hidden, in_features)) return GINE_ERR_DIM;
  if (num_nodes <= 0 || !slab || !gfold || !g2fold || !job) return GINE_ERR_INVALID;
  const int D = hidden, F = in_features;
  float* w[2] = {gfold, g2fold};  // product order of ChainWgradSrc<2>
  float* b[2] = {gfold + (size_t)D * (D + F), g2fold + (size_t)D * D};
  chain_slab_job(chain_wgrad_shape(num_nodes, D, F, 2), D, F, slab, 1.f, w, b, job);
  return GINE_OK;
}

extern "C" int gine_chain_unfold_grads2(const float* gfold, const float* wr1, const float* br1,
                                        const float* wdr, float* dwdr, float* dbdr, float* dwr1,
                                        float* dbr1, const float* g2fold, const float* wp2,
                                        const float* bp2, const float* wr0, float* dwr0,
                                        float* dbr0, float* dwp2, float* dbp2, float members,
                                        int32_t hidden, int32_t in_features, void* stream) {
  if (!chain_dims_ok(hidden, in_features)) return GINE_ERR_DIM;
  if (!gfold || !wr1 || !br1 || !wdr || !dwdr || !dwr1) return GINE_ERR_INVALID;
  if (!g2fold || !wp2 || !bp2 || !wr0 || !dwr0 || !dwp2) return GINE_ERR_INVALID;
  return launch_unfold(hidden,
                       UnfoldJob{gfold, wr1, br1, wdr, dwdr, dbdr, dwr1, dbr1, in_features, 1.f},
                       UnfoldJob{g2fold, wp2, bp2, wr0, dwr0, dbr0, dwp2, dbp2, 0, members},
                       as_stream(stream));
}

// ---------------------------------------------------------------------------------------
// Unfolded chain (the tests' comparator; raincast_gnn.chain.FOLD = False)
// ---------------------------------------------------------------------------------------
extern "C" int gine_chain_fwd(const float* r, const float* x, const float* wp2, const float* bp2,
                              float bias_scale, const float* wr0, const float* br0,
                              const float* wr1, const float* br1, const float* wdr,
                              const float* bdr, float* s, float* u, float* e, float* h0,
                              int64_t num_nodes, int32_t hidden, int32_t in_features,
                              void* stream) {
  if (!chain_dims_ok(hidden, in_features)) return GINE_ERR_DIM;
  if (num_nodes < 0) return GINE_ERR_INVALID;
  if (num_nodes >= (int64_t(1) << 31)) return GINE_ERR_TOO_LARGE;
  if (num_nodes == 0) return GINE_OK;
  if (!r || !x || !wp2 || !bp2 || !wr0 || !br0 || !wr1 || !br1 || !wdr || !bdr || !s || !u ||
      !e || !h0)
    return GINE_ERR_INVALID;
  hipStream_t st = as_stream(stream);
  const ChainArgs f1{r, nullptr, nullptr, wp2, bp2, wr0, br0, s, u, bias_scale, in_features};
  const ChainArgs f2{u, x, nullptr, wr1, br1, wdr, bdr, e, h0, 1.f, in_features};
  int rc = GINE_OK;
#define CALL_F(DD, FF)                                                  \
  rc = launch_chain<DD, FF, CH_F1>(f1, num_nodes, st);                  \
  if (rc == GINE_OK) rc = launch_chain<DD, FF, CH_F2>(f2, num_nodes, st)
  GINE_CHAIN_DISPATCH(hidden, in_features, CALL_F);
#undef CALL_F
  return rc;
}

extern "C" int gine_chain_bwd(const float* dh0, const float* x, const float* r, const float* s,
                              const float* u, const float* e, const float* wp2,
                              const float* wr0, const float* wr1, const float* wdr, float* de,
                              float* dt, float* ds, float* dr, float* slab, float* dwp2,
                              float* dbp2, float bias_scale, float* dwr0, float* dbr0,
                              float* dwr1, float* dbr1, float* dwdr, float* dbdr,
                              int64_t num_nodes, int32_t hidden, int32_t in_features,
                              void* stream) {
  if (!chain_dims_ok(hidden, in_features)) return GINE_ERR_DIM;
  if (num_nodes <= 0) return GINE_ERR_INVALID;
  if (num_nodes >= (int64_t(1) << 31)) return GINE_ERR_TOO_LARGE;
  if (!dh0 || !x || !r || !s || !u || !e || !wp2 || !wr0 || !wr1 || !wdr || !de || !dt ||
      !ds || !dr)
    return GINE_ERR_INVALID;
  if (slab && (!dwp2 || !dwr0 || !dwr1 || !dwdr)) return GINE_ERR_INVALID;
  hipStream_t st = as_stream(stream);
  const int D = hidden, F = in_features;
  const ChainArgs b1{dh0, nullptr, u, wdr, nullptr, wr1, nullptr, de, dt, 1.f, F};
  const ChainArgs b2{dt, nullptr, nullptr, wr0, nullptr, wp2, nullptr, ds, dr, 1.f, F};
  int rc = GINE_OK;
#define CALL_B(DD, FF)                                                  \
  rc = launch_chain<DD, FF, CH_B1>(b1, num_nodes, st);                  \
  if (rc == GINE_OK) rc = launch_chain<DD, FF, CH_B2>(b2, num_nodes, st)
  GINE_CHAIN_DISPATCH(D, F, CALL_B);
#undef CALL_B
  if (rc != GINE_OK || !slab) return rc;  // no slab: weight gradients via gine_chain_wgrad
  return gine_chain_wgrad(dh0, x, r, s, u, e, de, dt, ds, slab, dwp2, dbp2, bias_scale, dwr0,
                          dbr0, dwr1, dbr1, dwdr, dbdr, num_nodes, hidden, in_features, stream);
}

extern "C" int gine_chain_wgrad(const float* dh0, const float* x, const float* r,
                                const float* s, const float* u, const float* e,
                                const float* de, const float* dt, const float* ds, float* slab,
                                float* dwp2, float* dbp2, float bias_scale, float* dwr0,
                                float* dbr0, float* dwr1, float* dbr1, float* dwdr, float* dbdr,
                                int64_t num_nodes, int32_t hidden, int32_t in_features,
                                void* stream) {
  if (!chain_dims_ok(hidden, in_features)) return GINE_ERR_DIM;
  if (num_nodes <= 0) return GINE_ERR_INVALID;
  if (!dh0 || !x || !r || !s || !u || !e || !de || !dt || !ds || !slab) return GINE_ERR_INVALID;
  // all four weight outputs NULL: the slab is left for gine_grad_finalize_batch
  const bool reduce = dwp2 || dwr0 || dwr1 || dwdr;
  if (reduce && (!dwp2 || !dwr0 || !dwr1 || !dwdr)) return GINE_ERR_INVALID;
  hipStream_t st = as_stream(stream);
  const int D = hidden, F = in_features;
  const ChainWgradShape sh = chain_wgrad_shape(num_nodes, D, F, 4);
  const ChainWgradSrc<4> src{{dh0, de, dt, ds}, {e, u, s, r}, x, D, F};
  int rc = launch_wgrad_engine<64>(src, num_nodes, D, D + F, sh.tiles, sh.plan, sh.zstride(),
                                   sh.per, slab, st);
  if (rc != GINE_OK || !reduce) return rc;
  return launch_slab_sum(slab, sh.plan.chunks, (int64_t)sh.per, sh.per, sh.zstride(), sh.nz,
                         ChainWgradOut{{dwdr, dwr1, dwr0, dwp2}, {dbdr, dbr1, dbr0, dbp2}, D,
                                       F, bias_scale},
                         st);
}

extern "C" int gine_chain_wgrad_grad_job(int64_t num_nodes, int32_t hidden, int32_t in_features,
                                         const float* slab, float bias_scale, float* dwp2,
                                         float* dbp2, float* dwr0, float* dbr0, float* dwr1,
                                         float* dbr1, float* dwdr, float* dbdr,
                                         gine_grad_job* job) {
  if (!chain_dims_ok(hidden, in_features)) return GINE_ERR_DIM;
  if (num_nodes <= 0 || !slab || !dwp2 || !dwr0 || !dwr1 || !dwdr || !job)
    return GINE_ERR_INVALID;
  float* w[4] = {dwdr, dwr1, dwr0, dwp2};  // product order of ChainWgradSrc<4>
  float* b[4] = {dbdr, dbr1, dbr0, dbp2};
  chain_slab_job(chain_wgrad_shape(num_nodes, hidden, in_features, 4), hidden, in_features,
                 slab, bias_scale, w, b, job);
  return GINE_OK;
}

#ifdef GINE_CHAIN_PROFILE
extern "C" int gine_debug_chain_prof(long long* out) {  // [1024][16] host buffer
  GINE_RETURN_IF_HIP(hipDeviceSynchronize());
  GINE_RETURN_IF_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chain_prof), sizeof(g_chain_prof)));
  return GINE_OK;
}
#endif
