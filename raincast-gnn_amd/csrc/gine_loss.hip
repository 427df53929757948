// Fused CRPS losses of the reference (models/loss.py) on gfx950: one pass computes, per
// station-node, the closed-form CRPS and its exact gradient w.r.t. the K distribution
// parameters (forward-mode dual numbers), then the NaN-masked mean over nodes.
//
// Replaces the ~700 elementwise launches per training step that the torch formulation of
// MixedLoss.crps (loss.py:203-272) + its autograd takes.  Evaluated in fp64 (the reference
// promotes the mixed losses to fp64 through c = tensor([log 0.01]), loss.py:33-34,230-231;
// its remaining fp32 sub-expressions are reproduced to within their fp32 rounding).
//   NormalCRPS      loss.py:335-369   pred = [mu, sigma]
//   MixedNormalCRPS loss.py:6-68      pred = [mu, sigma, p]
//   MixedLoss       loss.py:71-272    pred = [mu, sigma, p, sigma_u] (+ u if grad_u)
#include "gine_common.hpp"
#include "gine_crpsdual.hpp"  // Dual<K>, the closed forms, LossK
#include "gine_headrow.hpp"
#include "gine_reduce.hpp"

namespace gine {
namespace {

constexpr int kThreads = 256;
constexpr int kHeadNodes = 64;  // nodes per workgroup of the pass that runs the head backward

// The output head's backward run by the CRPS pass for a unit loss seed (gine_crps_head_fwd_grad):
// raw = the head's pre-PostProcess output, h / w its input and weight; dh and the dW | db
// partial row of each workgroup (gine_headrow.hpp) are written beside grad_unit.
struct HeadBwdArgs {
  const float* raw;
  const float* h;
  const float* w;
  float* dh;
  float* slab;
  int D;
};

// One thread per node.  Writes d crps_n / d pred_n (0 for NaN targets) and per-block
// [sum crps, count] partials; the workgroup that finishes last (ticket) reduces the partials
// into the loss -- no separate finalize launch.  HC > 0 (the head backward of these nodes
// from grad_unit, HC float4 column chunks per lane): kHeadNodes nodes per workgroup (the
// CRPS evaluation is latency-bound: one busy wave per CU costs what four do), evaluated by
// wave 0 alone, while the other waves load the head's weight and the nodes' h rows; after
// one barrier those waves run the head backward, the nodes spread over their half-waves
// (gine_headrow.hpp).  The roles stay in branches of their own: h rows held through the
// loss evaluation had pushed it past 256 registers into scratch.
template <int KIND, int HC = 0>
__global__ __launch_bounds__(kThreads) void k_crps(const float* __restrict__ pred,
                                                   const float* __restrict__ y, int64_t n,
                                                   double u_fixed, double xi, double c,
                                                   double t, double* __restrict__ dpred,
                                                   double* __restrict__ partials,
                                                   double* __restrict__ loss_out,
                                                   double* __restrict__ count_out,
                                                   unsigned int* __restrict__ ticket,
                                                   const uint32_t* __restrict__ count_parts,
                                                   float* __restrict__ grad_unit,
                                                   HeadBwdArgs hb) {
  constexpr bool HEAD = HC > 0;
  constexpr int K = LossK<KIND>::value;
  static_assert(kThreads == head::kThreads, "one CRPS node per head-backward thread");
  // the head backward's half-waves (waves 1..3) and the rows each walks
  constexpr int kHelpHW = (kThreads - kHeadNodes) / 32;
  constexpr int kHelpU = (kHeadNodes + kHelpHW - 1) / kHelpHW;
  static_assert(kHeadNodes % kWave == 0 && kHelpHW > 0, "wave 0 evaluates the loss");
  __shared__ float s_graw[HEAD ? kHeadNodes : 1][K];
  __shared__ float s_part[HEAD ? kHelpHW : 1][head::kMaxK * 256 + head::kMaxK];
  __shared__ double s_sum[kThreads];
  __shared__ double s_cnt[kThreads];
  __shared__ int s_last;
  __shared__ double s_count;
  constexpr int NPB = HEAD ? kHeadNodes : kThreads;
  static_assert(GINE_COUNT_PARTS == kWave, "one partial count per lane of wave 0");
  if (grad_unit != nullptr) {  // the count of valid targets: wave 0 sums the partials
    if (threadIdx.x < kWave) {
      uint32_t c = count_parts[threadIdx.x];
      for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
      if (threadIdx.x == 0) s_count = (double)c;
    }
    __syncthreads();
  }
  const int64_t i = blockIdx.x * (int64_t)NPB + threadIdx.x;
  const int64_t first = blockIdx.x * (int64_t)NPB;
  const int64_t n_blk = min<int64_t>(n, first + NPB);
  double val = 0.0, cnt = 0.0;
  if (!HEAD || (int)threadIdx.x < NPB) {  // the loss (wave 0 when HEAD)
    if (i < n) {
      const float yf = y[i];
      double g[K];
#pragma unroll
      for (int k = 0; k < K; ++k) g[k] = 0.0;
      if (yf == yf) {  // NaN targets are masked out (loss.py:22,220)
        const double yy = (double)yf;
        Dual<K> v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = var<K>((double)pred[i * K + k], k);
        Dual<K> r;
        if constexpr (KIND == GINE_LOSS_NORMAL) {
          r = crps_normal(v[0], v[1], yy);
        } else if constexpr (KIND == GINE_LOSS_MIXED_NORMAL) {
          r = crps_mixed_normal(v[0], v[1], v[2], yy, c);
        } else if constexpr (KIND == GINE_LOSS_MIXED) {
          r = crps_mixed<K, false>(v[0], v[1], v[2], v[3], cst<K>(u_fixed), yy, c, xi, t);
        } else {
          r = crps_mixed<K, true>(v[0], v[1], v[2], v[3], v[4], yy, c, xi, t);
        }
        val = r.v;
        cnt = 1.0;
#pragma unroll
        for (int k = 0; k < K; ++k) g[k] = r.d[k];
      }
#pragma unroll
      for (int k = 0; k < K; ++k) dpred[i * K + k] = g[k];
      if (grad_unit != nullptr) {  // d loss / d pred for gloss = 1, as k_crps_bwd rounds it
        const double cnt_all = s_count;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float gu = (float)(1.0 * g[k] / cnt_all);
          grad_unit[i * K + k] = gu;
          if constexpr (HEAD)  // d raw, as k_head_bwd forms it from grad_pred
            s_graw[threadIdx.x][k] =
                head::post_bwd(head::role_of(KIND, k), hb.raw[i * K + k], gu);
        }
      }
    }
    if constexpr (HEAD) {
      __syncthreads();  // d raw in LDS
      __syncthreads();  // the helpers' partial rows in LDS
    }
  } else if constexpr (HEAD) {  // waves 1..3: the head backward of the workgroup's nodes
    head::HeadRows<K, kHelpU, HC> rows;
    const int hw = threadIdx.x / 32 - NPB / 32;
    rows.init(hb.w, hb.D);
    rows.load(first + hw, kHelpHW, n_blk, hb.h, hb.D);  // arriving under the evaluation
    __syncthreads();  // d raw in LDS
    rows.step([&](int64_t nd, float (&gr)[K]) {
#pragma unroll
                for (int k = 0; k < K; ++k) gr[k] = s_graw[nd - first][k];
              },
              first + hw, kHelpHW, n_blk, hb.dh, hb.D);
    rows.put(s_part, hw, hb.D);
    __syncthreads();  // the partial rows in LDS
  }
  if constexpr (HEAD)
    head::reduce_rows<K>(hb.slab + (size_t)blockIdx.x * (K * hb.D + K), hb.D, s_part, kHelpHW);
  s_sum[threadIdx.x] = val;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {  // fixed-order tree
    if (threadIdx.x < s) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
    }
    __syncthreads();
  }
  // publish the partial, then draw a ticket.  The partial goes out as agent-scope atomic
  // exchanges (performed at the memory side, like the BatchNorm accumulator's adds) and the
  // last arriver reads the partials with agent-scope atomic loads: no release / acquire
  // fence -- an agent-scope release writes the XCD's whole L2 back, and with the head
  // backward's dh rows just written that write-back sat in every workgroup's tail.
  if (threadIdx.x == 0) {
    __hip_atomic_exchange(&partials[2 * blockIdx.x], s_sum[0], __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_exchange(&partials[2 * blockIdx.x + 1], s_cnt[0], __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int prev =
        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  // fixed order: thread j sums partial rows j, j + 256, ... then the same tree as above
  const int P = gridDim.x;
  double a = 0.0, b = 0.0;
  for (int p = threadIdx.x; p < P; p += kThreads) {
    a += __hip_atomic_load(&partials[2 * p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    b += __hip_atomic_load(&partials[2 * p + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  s_sum[threadIdx.x] = a;
  s_cnt[threadIdx.x] = b;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss_out[0] = s_sum[0] / s_cnt[0];  // NaN when no target is valid (torch.mean of empty)
    count_out[0] = s_cnt[0];
    *ticket = 0u;  // re-armed for the next call (stream order)
  }
}

// Number of non-NaN targets (the size of the reference's y[mask], loss.py:39-42, 234-239)
// as GINE_COUNT_PARTS partial counts: the unit-seed gradient of the CRPS pass divides by
// their sum before any workgroup of that pass could know the total.  Recounted every step
// (a replayed graph counts whatever y holds now).  The training step gets the same partials
// from the head forward (gine_head_fwd_count); this launch is the stand-alone form.
__global__ __launch_bounds__(256) void k_count_valid(const float* __restrict__ y, int64_t n,
                                                     uint32_t* __restrict__ parts) {
  count_valid_parts(y, n, parts);
}

// grad_pred = gloss * dpred / count
__global__ __launch_bounds__(kThreads) void k_crps_bwd(const double* __restrict__ dpred,
                                                       const double* __restrict__ count,
                                                       const double* __restrict__ gloss,
                                                       int64_t total, float* __restrict__ grad) {
  const int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (i >= total) return;
  grad[i] = (float)(gloss[0] * dpred[i] / count[0]);
}

// ---------------------------------------------------------------------------------------
// Threshold-weighted CRPS as a loss term: per node
//   (1 - lambda) L_kind(pred, y) + lambda twCRPS_t(pred, y),
// twCRPS_t(F, y) = int_t^inf (F(x) - 1{x >= y})^2 dx = CRPS(F_t, max(y, t)), F_t the
// distribution of max(Y, t).  With t' = max(t, c) (t for the uncensored normal) and
// y' = max(y, t') the closed forms above give it with c := t', y := y': F_t is F censored at
// t' (tw_censored for the two kinds without a tail).  Where t' has passed u only the Pareto tail is left and the form is tw_tail.  The
// distribution is the where(y < u, ...) one for a learned u too (the sigmoid blend is the
// plain term's surrogate, not the distribution's CRPS).
// ---------------------------------------------------------------------------------------
// 1 - Phi(z) from erfc: the tail's mass 1 - m_u = (1 - p)(1 - Phi(z(u))) without cancellation
template <int K>
__device__ __forceinline__ Dual<K> upper_Phi(const Dual<K>& z) {
  const double pdf = exp(-0.5 * z.v * z.v - kLogSqrt2Pi);
  return apply(z, 0.5 * erfc(z.v / kSqrt2), -pdf);
}

// t' >= u: with a = 1 - m_u, w(x) = 1 + xi (x - u) / sigma_u, e1 = -(1 - xi)/xi,
// e2 = -(2 - xi)/xi = e1 - 1/xi:
//   (y' - t') + 2 a sigma_u/(1 - xi) (w(y')^e1 - w(t')^e1) + a^2 sigma_u/(2 - xi) w(t')^e2
// (pareto_crps(y', u, m_u, sigma_u, xi) at t' = u).  w >= 1 on both arguments.
template <int K>
__device__ Dual<K> tw_tail(const Dual<K>& mu, const Dual<K>& sigma, const Dual<K>& p,
                           const Dual<K>& su, const Dual<K>& u, double yp, double tp,
                           double xi) {
  const Dual<K> a = (1.0 - p) * upper_Phi((u - mu) / sigma);
  const Dual<K> wy = 1.0 + xi * ((cst<K>(yp) - u) / su);
  const Dual<K> wt = 1.0 + xi * ((cst<K>(tp) - u) / su);
  Dual<K> py1, pt1, pt2;
  if (xi == 0.5) {  // w^-1 = (w^-2)^0.5 and w^-3 = w^-1 w^-2: pareto_crps's two shortcuts
    const Dual<K> my = pow_m2(wy), mt = pow_m2(wt);
    py1 = pow_half(my);
    pt1 = pow_half(mt);
    pt2 = pt1 * mt;
  } else {
    const double e1 = -(1.0 - xi) / xi;
    py1 = powc(wy, e1);
    pt1 = powc(wt, e1);
    pt2 = powc(wt, -(2.0 - xi) / xi);
  }
  return (yp - tp) + ((2.0 / (1.0 - xi)) * (a * su * (py1 - pt1)) +
                      (1.0 / (2.0 - xi)) * (sq(a) * su * pt2));
}

// CRPS at y' >= t' of the normal with atom p censored at t': crps_mixed_normal(mu, sigma, p,
// y', t') in upper probabilities S = q (1 - Phi), as csrc/gine_forecast.hip evaluates it,
//   (y' - t') - 2 int_t'^y' S dx + int_t'^inf S^2 dx:
// far up the tail the lower form subtracts O(sigma z) terms and leaves rounding noise where
// the value is 1e-20; here no term is larger than the result, and for y' = t' the first
// integral and its derivatives are exactly 0.
template <int K>
__device__ Dual<K> tw_censored(const Dual<K>& mu, const Dual<K>& sigma, const Dual<K>& p,
                               double yp, double tp) {
  const Dual<K> yt = (cst<K>(yp) - mu) / sigma;
  const Dual<K> ct = (cst<K>(tp) - mu) / sigma;
  const Dual<K> q = 1.0 - p;
  const Dual<K> Uc = upper_Phi(ct);
  const Dual<K> G = (yt * upper_Phi(yt) - phi(yt)) - (ct * Uc - phi(ct));
  const Dual<K> H = 2.0 * (phi(ct) * Uc) - ct * sq(Uc) - kInvSqrtPi * upper_Phi(kSqrt2 * ct);
  return (yp - tp) + sigma * (q * (q * H - 2.0 * G));
}

template <int KIND, int K>
__device__ Dual<K> tw_term(const Dual<K> (&v)[K], double u_fixed, double y, double c, double xi,
                           double t, double tw_t) {
  const double tp = KIND == GINE_LOSS_NORMAL ? tw_t : fmax(tw_t, c);
  const double yp = fmax(y, tp);
  if constexpr (KIND == GINE_LOSS_NORMAL) {
    return tw_censored(v[0], v[1], cst<K>(0.0), yp, tp);
  } else if constexpr (KIND == GINE_LOSS_MIXED_NORMAL) {
    return tw_censored(v[0], v[1], v[2], yp, tp);
  } else {
    const Dual<K> u = KIND == GINE_LOSS_MIXED_U ? v[K - 1] : cst<K>(u_fixed);
    if (tp < u.v) return crps_mixed<K, false>(v[0], v[1], v[2], v[3], u, yp, tp, xi, t);
    return tw_tail(v[0], v[1], v[2], v[3], u, yp, tp, xi);
  }
}

// k_crps without the head backward, plus the threshold-weighted term: one thread per node,
// the plain term first, then the tw term into the same accumulators (the two closed forms
// never live together: Dual<5> twice over is past 256 registers); partials, ticket and
// finish as k_crps.
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_crps_tw(
    const float* __restrict__ pred, const float* __restrict__ y, int64_t n, double u_fixed,
    double xi, double c, double t, double tw_t, double tw_w, double* __restrict__ dpred,
    double* __restrict__ partials, double* __restrict__ loss_out, double* __restrict__ count_out,
    unsigned int* __restrict__ ticket, const uint32_t* __restrict__ count_parts,
    float* __restrict__ grad_unit) {
  constexpr int K = LossK<KIND>::value;
  __shared__ double s_sum[kThreads];
  __shared__ double s_cnt[kThreads];
  __shared__ int s_last;
  __shared__ double s_count;
  static_assert(GINE_COUNT_PARTS == kWave, "one partial count per lane of wave 0");
  if (grad_unit != nullptr) {  // the count of valid targets: wave 0 sums the partials
    if (threadIdx.x < kWave) {
      uint32_t cp = count_parts[threadIdx.x];
      for (int off = 32; off > 0; off >>= 1) cp += __shfl_xor(cp, off);
      if (threadIdx.x == 0) s_count = (double)cp;
    }
    __syncthreads();
  }
  const int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  double val = 0.0, cnt = 0.0;
  if (i < n) {
    const float yf = y[i];
    double g[K];
#pragma unroll
    for (int k = 0; k < K; ++k) g[k] = 0.0;
    if (yf == yf) {  // NaN targets are masked out
      const double yy = (double)yf;
      Dual<K> v[K];
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = var<K>((double)pred[i * K + k], k);
      const double w0 = 1.0 - tw_w;
      {
        Dual<K> r;
        if constexpr (KIND == GINE_LOSS_NORMAL) {
          r = crps_normal(v[0], v[1], yy);
        } else if constexpr (KIND == GINE_LOSS_MIXED_NORMAL) {
          r = crps_mixed_normal(v[0], v[1], v[2], yy, c);
        } else if constexpr (KIND == GINE_LOSS_MIXED) {
          r = crps_mixed<K, false>(v[0], v[1], v[2], v[3], cst<K>(u_fixed), yy, c, xi, t);
        } else {
          r = crps_mixed<K, true>(v[0], v[1], v[2], v[3], v[4], yy, c, xi, t);
        }
        val = w0 * r.v;
#pragma unroll
        for (int k = 0; k < K; ++k) g[k] = w0 * r.d[k];
      }
      {
        const Dual<K> r = tw_term<KIND, K>(v, u_fixed, yy, c, xi, t, tw_t);
        val += tw_w * r.v;
#pragma unroll
        for (int k = 0; k < K; ++k) g[k] += tw_w * r.d[k];
      }
      cnt = 1.0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) dpred[i * K + k] = g[k];
    if (grad_unit != nullptr) {  // d loss / d pred for gloss = 1, as k_crps_bwd rounds it
      const double cnt_all = s_count;
#pragma unroll
      for (int k = 0; k < K; ++k) grad_unit[i * K + k] = (float)(1.0 * g[k] / cnt_all);
    }
  }
  s_sum[threadIdx.x] = val;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {  // fixed-order tree
    if (threadIdx.x < s) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
    }
    __syncthreads();
  }
  // partial out by agent-scope exchanges, then the ticket: k_crps's protocol
  if (threadIdx.x == 0) {
    __hip_atomic_exchange(&partials[2 * blockIdx.x], s_sum[0], __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_exchange(&partials[2 * blockIdx.x + 1], s_cnt[0], __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int prev =
        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  // fixed order: thread j sums partial rows j, j + 256, ... then the same tree as above
  const int P = gridDim.x;
  double a = 0.0, b = 0.0;
  for (int p = threadIdx.x; p < P; p += kThreads) {
    a += __hip_atomic_load(&partials[2 * p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    b += __hip_atomic_load(&partials[2 * p + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  s_sum[threadIdx.x] = a;
  s_cnt[threadIdx.x] = b;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss_out[0] = s_sum[0] / s_cnt[0];  // NaN when no target is valid (torch.mean of empty)
    count_out[0] = s_cnt[0];
    *ticket = 0u;  // re-armed for the next call (stream order)
  }
}

}  // namespace
}  // namespace gine

using namespace gine;

extern "C" int gine_crps_num_partials(int64_t num_nodes, int32_t* num_partials) {
  if (!num_partials || num_nodes < 0) return GINE_ERR_INVALID;
  const int64_t p = ceil_div(num_nodes, kHeadNodes);  // enough for either workgroup size
  *num_partials = (int32_t)(p > 0 ? p : 1);
  return GINE_OK;
}

namespace {
int crps_fwd_launch(const float* pred, const float* y, int64_t num_nodes, int32_t kind, double u,
                    double xi, double c, double t, double* dpred, double* partials,
                    double* loss_out, double* count_out, uint32_t* ticket,
                    const uint32_t* count_parts, float* grad_unit, void* stream,
                    const HeadBwdArgs* hb = nullptr) {
  if (num_nodes < 0 || !partials || !loss_out || !count_out || !ticket) return GINE_ERR_INVALID;
  if ((count_parts == nullptr) != (grad_unit == nullptr)) return GINE_ERR_INVALID;
  if (num_nodes > 0 && (!pred || !y || !dpred)) return GINE_ERR_INVALID;
  if (kind < GINE_LOSS_NORMAL || kind > GINE_LOSS_MIXED_U) return GINE_ERR_INVALID;
  hipStream_t s = as_stream(stream);
  const int npb = hb ? kHeadNodes : kThreads;
  const int64_t blocks = ceil_div(num_nodes, npb) > 0 ? ceil_div(num_nodes, npb) : 1;
#define LAUNCH_CRPS_H(KIND_, H_)                                                               \
  hipLaunchKernelGGL((k_crps<KIND_, H_>), dim3((unsigned)blocks), dim3(kThreads), 0, s, pred, y, \
                     num_nodes, u, xi, c, t, dpred, partials, loss_out, count_out, ticket,      \
                     count_parts, grad_unit, hb ? *hb : HeadBwdArgs{})
#define LAUNCH_CRPS(KIND_)                                 \
  do {                                                     \
    if (!hb) LAUNCH_CRPS_H(KIND_, 0);                      \
    else if (hb->D <= 128) LAUNCH_CRPS_H(KIND_, 1);        \
    else LAUNCH_CRPS_H(KIND_, 2);                          \
  } while (0)
  switch (kind) {
    case GINE_LOSS_NORMAL: LAUNCH_CRPS(GINE_LOSS_NORMAL); break;
    case GINE_LOSS_MIXED_NORMAL: LAUNCH_CRPS(GINE_LOSS_MIXED_NORMAL); break;
    case GINE_LOSS_MIXED: LAUNCH_CRPS(GINE_LOSS_MIXED); break;
    default: LAUNCH_CRPS(GINE_LOSS_MIXED_U); break;
  }
#undef LAUNCH_CRPS
#undef LAUNCH_CRPS_H
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}
}  // namespace

extern "C" int gine_crps_fwd(const float* pred, const float* y, int64_t num_nodes, int32_t kind,
                             double u, double xi, double c, double t, double* dpred,
                             double* partials, double* loss_out, double* count_out,
                             uint32_t* ticket, void* stream) {
  return crps_fwd_launch(pred, y, num_nodes, kind, u, xi, c, t, dpred, partials, loss_out,
                         count_out, ticket, nullptr, nullptr, stream);
}

extern "C" int gine_crps_fwd_grad(const float* pred, const float* y, int64_t num_nodes,
                                  int32_t kind, double u, double xi, double c, double t,
                                  double* dpred, double* partials, double* loss_out,
                                  double* count_out, uint32_t* ticket,
                                  const uint32_t* count_parts, float* grad_unit, void* stream) {
  if (!count_parts || !grad_unit) return GINE_ERR_INVALID;
  return crps_fwd_launch(pred, y, num_nodes, kind, u, xi, c, t, dpred, partials, loss_out,
                         count_out, ticket, count_parts, grad_unit, stream);
}

namespace {
int loss_k(int kind) {
  return kind == GINE_LOSS_NORMAL ? 2 : kind == GINE_LOSS_MIXED_NORMAL ? 3
         : kind == GINE_LOSS_MIXED ? 4 : kind == GINE_LOSS_MIXED_U ? 5 : -1;
}
int64_t crps_head_blocks(int64_t num_nodes) {
  const int64_t b = ceil_div(num_nodes, kHeadNodes);
  return b > 0 ? b : 1;
}
}  // namespace

extern "C" int gine_crps_head_slab_floats(int64_t num_nodes, int32_t channels, int32_t kind,
                                          size_t* floats) {
  const int K = loss_k(kind);
  if (K < 0 || num_nodes < 0 || !floats) return GINE_ERR_INVALID;
  if (channels <= 0 || channels % 4 != 0 || channels > 32 * 4 * head::kMaxChunks)
    return GINE_ERR_DIM;
  *floats = (size_t)crps_head_blocks(num_nodes) * (size_t)(K * channels + K);
  return GINE_OK;
}

extern "C" int gine_crps_head_fwd_grad(const float* pred, const float* y, int64_t num_nodes,
                                       int32_t kind, double u, double xi, double c, double t,
                                       double* dpred, double* partials, double* loss_out,
                                       double* count_out, uint32_t* ticket,
                                       const uint32_t* count_parts, float* grad_unit,
                                       const float* raw, const float* h, const float* w,
                                       int32_t channels, float* dh, float* head_slab,
                                       void* stream) {
  size_t floats = 0;
  const int rc = gine_crps_head_slab_floats(num_nodes, channels, kind, &floats);
  if (rc != GINE_OK) return rc;
  if (!count_parts || !grad_unit || !head_slab || !w) return GINE_ERR_INVALID;
  if (num_nodes > 0 && (!raw || !h || !dh)) return GINE_ERR_INVALID;
  const HeadBwdArgs hb{raw, h, w, dh, head_slab, channels};
  return crps_fwd_launch(pred, y, num_nodes, kind, u, xi, c, t, dpred, partials, loss_out,
                         count_out, ticket, count_parts, grad_unit, stream, &hb);
}

extern "C" int gine_crps_head_grad_job(int64_t num_nodes, int32_t channels, int32_t kind,
                                       const float* head_slab, float* dw, float* db,
                                       gine_grad_job* job) {
  size_t floats = 0;
  const int rc = gine_crps_head_slab_floats(num_nodes, channels, kind, &floats);
  if (rc != GINE_OK) return rc;
  if (!head_slab || !dw || !job) return GINE_ERR_INVALID;
  const int K = loss_k(kind);
  const int64_t per = (int64_t)K * channels + K;
  *job = gine_grad_job{};
  job->kind = GINE_GRAD_JOB_SLAB;
  job->src = head_slab;
  job->rows = (int32_t)crps_head_blocks(num_nodes);
  job->cstride = per;
  job->nz = 1;
  job->per[0] = per;
  job->wsize[0] = (int64_t)K * channels;
  job->w[0] = dw;
  job->b[0] = db;
  job->bscale[0] = 1.0f;
  return GINE_OK;
}

extern "C" int gine_count_valid(const float* y, int64_t num_nodes, uint32_t* count_parts,
                                void* stream) {
  if (num_nodes < 0 || !count_parts || (num_nodes > 0 && !y)) return GINE_ERR_INVALID;
  if (num_nodes > ((int64_t)1 << 32) - 1) return GINE_ERR_DIM;  // 32-bit counts
  hipLaunchKernelGGL(k_count_valid, dim3(GINE_COUNT_PARTS), dim3(256), 0, as_stream(stream), y,
                     num_nodes, count_parts);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_crps_bwd(const double* dpred, const double* count, const double* gloss,
                             int64_t num_nodes, int32_t kind, float* grad_pred, void* stream) {
  if (num_nodes < 0 || !count || !gloss) return GINE_ERR_INVALID;
  if (kind < GINE_LOSS_NORMAL || kind > GINE_LOSS_MIXED_U) return GINE_ERR_INVALID;
  const int K = kind == GINE_LOSS_NORMAL ? 2 : kind == GINE_LOSS_MIXED_NORMAL ? 3
              : kind == GINE_LOSS_MIXED ? 4 : 5;
  const int64_t total = num_nodes * K;
  if (total == 0) return GINE_OK;
  if (!dpred || !grad_pred) return GINE_ERR_INVALID;
  hipLaunchKernelGGL(k_crps_bwd, dim3((unsigned)ceil_div(total, kThreads)), dim3(kThreads), 0,
                     as_stream(stream), dpred, count, gloss, total, grad_pred);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

// ---------------------------------------------------------------------------------------
// (1 - tw_weight) * CRPS + tw_weight * twCRPS at tw_threshold: the roles of gine_crps_fwd /
// _fwd_grad / _bwd.  Both scalars are launch arguments.  No head-backward form.
// ---------------------------------------------------------------------------------------
namespace {
int crps_tw_launch(const float* pred, const float* y, int64_t num_nodes, int32_t kind, double u,
                   double xi, double c, double t, double tw_threshold, double tw_weight,
                   double* dpred, double* partials, double* loss_out, double* count_out,
                   uint32_t* ticket, const uint32_t* count_parts, float* grad_unit,
                   void* stream) {
  if (num_nodes < 0 || !partials || !loss_out || !count_out || !ticket) return GINE_ERR_INVALID;
  if ((count_parts == nullptr) != (grad_unit == nullptr)) return GINE_ERR_INVALID;
  if (num_nodes > 0 && (!pred || !y || !dpred)) return GINE_ERR_INVALID;
  if (kind < GINE_LOSS_NORMAL || kind > GINE_LOSS_MIXED_U) return GINE_ERR_INVALID;
  if (!(tw_weight >= 0.0 && tw_weight <= 1.0)) return GINE_ERR_INVALID;
  if (!(tw_threshold - tw_threshold == 0.0)) return GINE_ERR_INVALID;  // finite
  const int64_t blocks = ceil_div(num_nodes, kThreads) > 0 ? ceil_div(num_nodes, kThreads) : 1;
#define LAUNCH_CRPS_TW(KIND_)                                                                  \
  hipLaunchKernelGGL((k_crps_tw<KIND_>), dim3((unsigned)blocks), dim3(kThreads), 0,            \
                     as_stream(stream), pred, y, num_nodes, u, xi, c, t, tw_threshold,         \
                     tw_weight, dpred, partials, loss_out, count_out, ticket, count_parts,     \
                     grad_unit)
  switch (kind) {
    case GINE_LOSS_NORMAL: LAUNCH_CRPS_TW(GINE_LOSS_NORMAL); break;
    case GINE_LOSS_MIXED_NORMAL: LAUNCH_CRPS_TW(GINE_LOSS_MIXED_NORMAL); break;
    case GINE_LOSS_MIXED: LAUNCH_CRPS_TW(GINE_LOSS_MIXED); break;
    default: LAUNCH_CRPS_TW(GINE_LOSS_MIXED_U); break;
  }
#undef LAUNCH_CRPS_TW
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}
}  // namespace

extern "C" int gine_crps_tw_fwd(const float* pred, const float* y, int64_t num_nodes,
                                int32_t kind, double u, double xi, double c, double t,
                                double tw_threshold, double tw_weight, double* dpred,
                                double* partials, double* loss_out, double* count_out,
                                uint32_t* ticket, void* stream) {
  return crps_tw_launch(pred, y, num_nodes, kind, u, xi, c, t, tw_threshold, tw_weight, dpred,
                        partials, loss_out, count_out, ticket, nullptr, nullptr, stream);
}

extern "C" int gine_crps_tw_fwd_grad(const float* pred, const float* y, int64_t num_nodes,
                                     int32_t kind, double u, double xi, double c, double t,
                                     double tw_threshold, double tw_weight, double* dpred,
                                     double* partials, double* loss_out, double* count_out,
                                     uint32_t* ticket, const uint32_t* count_parts,
                                     float* grad_unit, void* stream) {
  if (!count_parts || !grad_unit) return GINE_ERR_INVALID;
  return crps_tw_launch(pred, y, num_nodes, kind, u, xi, c, t, tw_threshold, tw_weight, dpred,
                        partials, loss_out, count_out, ticket, count_parts, grad_unit, stream);
}

// grad_pred = gloss * dpred / count for the dpred of gine_crps_tw_fwd(_grad), which holds the
// weighted sum already: the two scalars are checked, not read again.
extern "C" int gine_crps_tw_bwd(const double* dpred, const double* count, const double* gloss,
                                int64_t num_nodes, int32_t kind, double tw_threshold,
                                double tw_weight, float* grad_pred, void* stream) {
  if (!(tw_weight >= 0.0 && tw_weight <= 1.0)) return GINE_ERR_INVALID;
  if (!(tw_threshold - tw_threshold == 0.0)) return GINE_ERR_INVALID;
  return gine_crps_bwd(dpred, count, gloss, num_nodes, kind, grad_pred, stream);
}
