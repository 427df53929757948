// AdamW over ONE flat fp32 buffer holding every parameter of the model (the benchmarked
// training step, train.py:67-69: zero_grad / backward / AdamW.step, lr from params.json).
//
// torch.optim.AdamW (amsgrad=False, maximize=False) per element, default (non-capturable)
// formulation:
//   step += 1
//   p  *= 1 - lr*wd
//   m   = m + (1-b1)*(g - m)                 (lerp, weight < 0.5 branch)
//   v   = v*b2 + (1-b2)*g*g
//   p  += -(lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The arithmetic below is the definition (tests/optim_oracle.py restates it and
// tests/test_gpu_optim_rows.py holds both kernels to it bit for bit).  lr, b1, b2, eps and wd
// arrive as fp32 and every scalar is formed from those fp32 values:
//   decay = (float)(1 - (double)lr (double)wd)          w1 = 1.0f - b1   (fp32 subtraction)
//   nss   = (float)(-((double)lr / (1 - (double)b1^t))) w2 = 1.0f - b2   (fp32 subtraction)
//   bc2   = (float)sqrt(1 - (double)b2^t)               t  = step[0] + 1.0f, then widened
// and per element, one fp32 rounding per operation (-ffp-contract=off, IEEE divide and sqrt):
//   p = p*decay;  m = m + w1*(g - m);  v = v*b2;  v = v + (w2*g)*g;
//   p = p + nss*(m / (sqrtf(v)/bc2 + eps))
// This is NOT how torch applies its Python scalars: torch forms 1 - beta, the bias corrections
// and the step size from the Python doubles and rounds once.  At the defaults w1 is
// 0.100000024 against torch's 0.1f (+2.2e-7 relative), w2 0.00099998713 against 0.001f
// (-1.29e-5), bc2 at t = 1 -6.4e-6, nss at t = 1 -1.9e-7; decay is the same.  The kernel's
// choice is the self-consistent one (w2 = 1 - b2 exactly, so a constant gradient keeps
// v / (1 - b2^t) at g*g); torch's values would need double-precision arguments.  step[0] is an
// fp32 count: from 2^24 on it no longer advances (2^24 + 1.0f == 2^24) and t stays 2^24,
// where both bias corrections have long been exactly 1.
// The step counter lives on the device, so the update is legal inside a captured HIP graph
// and replays correctly: every workgroup uses step[0] + 1, and the workgroup that finishes
// last stores the bump -- one launch per optimizer step.  "Last" is found by a two-level
// ticket: workgroup b draws from sub-ticket b % 8 (step[32 + 32 g], one 128-byte line each),
// the last of each group draws from the top ticket (step[1]); every ticket word is re-armed
// to 0 by its last drawer.  The step buffer is kAdamStateFloats = 288 floats
// (gine_adamw_state_floats), all zero at allocation.
#include "gine_common.hpp"


namespace gine {
namespace {

constexpr int kAdamGroups = 8;     // sub-tickets (one per XCD's share of the grid)
constexpr int kAdamSubBase = 32;   // floats: sub-ticket g at step[32 + 32 g]
constexpr int kAdamStateFloats = kAdamSubBase + 32 * kAdamGroups;

struct AdamW {
  float decay, neg_step_size, bc2_sqrt, w1, w2, beta2, eps;
  __device__ __forceinline__ void operator()(float gi, float& pi, float& mi, float& vi) const {
    pi = pi * decay;
    mi = mi + w1 * (gi - mi);
    vi = vi * beta2;
    vi = vi + w2 * gi * gi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi = pi + neg_step_size * (mi / denom);  // addcdiv: p + value * (m / denom)
  }
};

// One float4 of every buffer per thread (16-byte loads, all four issued before any use);
// the last n % 4 elements by the first threads of the grid.
__global__ __launch_bounds__(256) void k_adamw(float* __restrict__ p, const float* __restrict__ g,
                                               float* __restrict__ m, float* __restrict__ v,
                                               float* __restrict__ step, int64_t n,
                                               float lr, float beta1, float beta2, float eps,
                                               float weight_decay) {
  const float t_new = step[0] + 1.0f;
  const double t = (double)t_new;
  const AdamW op{(float)(1.0 - (double)lr * (double)weight_decay),
                 (float)(-((double)lr / (1.0 - pow((double)beta1, t)))),
                 (float)sqrt(1.0 - pow((double)beta2, t)), 1.0f - beta1, 1.0f - beta2, beta2,
                 eps};
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = tid; i < n4; i += stride) {
    const float4 gi = reinterpret_cast<const float4*>(g)[i];
    float4 pi = reinterpret_cast<float4*>(p)[i];
    float4 mi = reinterpret_cast<float4*>(m)[i];
    float4 vi = reinterpret_cast<float4*>(v)[i];
    op(gi.x, pi.x, mi.x, vi.x);
    op(gi.y, pi.y, mi.y, vi.y);
    op(gi.z, pi.z, mi.z, vi.z);
    op(gi.w, pi.w, mi.w, vi.w);
    reinterpret_cast<float4*>(p)[i] = pi;
    reinterpret_cast<float4*>(m)[i] = mi;
    reinterpret_cast<float4*>(v)[i] = vi;
  }
  if (tid < n - 4 * n4) {
    const int64_t i = 4 * n4 + tid;
    float pi = p[i], mi = m[i], vi = v[i];
    op(g[i], pi, mi, vi);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
  }
  __syncthreads();  // every thread of this workgroup has read step[0]
  if (threadIdx.x == 0) {
    unsigned int* ticket = reinterpret_cast<unsigned int*>(&step[1]);  // 0.0f == 0u
    // two-level ticket: same-word returning atomics serialise (~88 per us on one word,
    // MI355X_MICROARCH.md "dequeue"), so 512 workgroups on one ticket cost ~6 us at the
    // end of the launch; workgroup b draws from sub-ticket b % 8 (own 128-byte line),
    // the last of each group from the top ticket (one word: 6.81 -> 5.46 us, r02_s84)
    const unsigned int g = blockIdx.x % kAdamGroups;
    const unsigned int groups = min(gridDim.x, (unsigned)kAdamGroups);
    const unsigned int size = (gridDim.x - g + kAdamGroups - 1) / kAdamGroups;
    unsigned int* sub = reinterpret_cast<unsigned int*>(step + kAdamSubBase) + 32 * g;
    if (atomicAdd(sub, 1u) == size - 1) {
      *sub = 0u;  // re-armed (the next launch is ordered after this one)
      if (atomicAdd(ticket, 1u) == groups - 1) {
        step[0] = t_new;
        *ticket = 0u;
      }
    }
  }
}

}  // namespace
}  // namespace gine

using namespace gine;

extern "C" int gine_adamw_step(float* param, const float* grad, float* exp_avg,
                               float* exp_avg_sq, float* step, int64_t n, float lr,
                               float beta1, float beta2, float eps, float weight_decay,
                               void* stream) {
  if (n < 0 || !step) return GINE_ERR_INVALID;
  if (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)) return GINE_ERR_INVALID;
  hipStream_t s = as_stream(stream);
  // one float4 per thread up to 512 workgroups (few tickets to serialise on one word);
  // 16-byte accesses need 16-byte aligned buffers
  const uintptr_t al = reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) |
                       reinterpret_cast<uintptr_t>(exp_avg) |
                       reinterpret_cast<uintptr_t>(exp_avg_sq);
  if (n > 0 && (al & 15) != 0) return GINE_ERR_INVALID;
  int64_t blocks = ceil_div(n > 0 ? ceil_div(n, 4) : 1, 256);
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL(k_adamw, dim3((unsigned)blocks), dim3(256), 0, s, param, grad, exp_avg,
                     exp_avg_sq, step, n, lr, beta1, beta2, eps, weight_decay);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_adamw_state_floats(int64_t* floats) {
  if (!floats) return GINE_ERR_INVALID;
  *floats = kAdamStateFloats;
  return GINE_OK;
}

// ---------------------------------------------------------------------------------------
// The step under a device control block: learning-rate schedule, gradient clipping by the
// global norm and skipping of a step whose gradient is not finite, all decided on the device
// so that a captured step follows them on every replay.
//   gine_grad_sumsq      one pass over the gradient: per workgroup {sum g*g, #non-finite g}
//                        in fp64, fixed order, plain stores (no atomics, no ticket)
//   gine_adamw_step_ctl  every workgroup sums the partials in index order, forms the clip
//                        coefficient and this step's rate, then runs k_adamw's update
// The launch boundary between the two is the only synchronisation.
// ---------------------------------------------------------------------------------------
namespace gine {
namespace {

constexpr int kAdamMaxBlocks = 512;  // the step's grid cap, shared by the norm's grid

inline int64_t adam_blocks(int64_t n) {
  int64_t blocks = ceil_div(n > 0 ? ceil_div(n, 4) : 1, 256);
  return blocks > kAdamMaxBlocks ? kAdamMaxBlocks : blocks;
}

// Thread order: float4 i = tid, tid + stride, ... (x, y, z, w in turn), then the n % 4 tail
// element of the grid's first threads; lanes by butterfly (every lane ends with the same
// sum), the four waves in order through LDS.
__global__ __launch_bounds__(256) void k_grad_sumsq(const float* __restrict__ g, int64_t n,
                                                    double2* __restrict__ partials) {
  __shared__ double s_sum[4];
  __shared__ uint32_t s_bad[4];
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  double acc = 0.0;
  uint32_t bad = 0;
  auto take = [&](float v) {
    acc += (double)v * (double)v;
    bad += !(fabsf(v) < __builtin_inff());  // inf or NaN
  };
  for (int64_t i = tid; i < n4; i += stride) {
    const float4 gi = reinterpret_cast<const float4*>(g)[i];
    take(gi.x);
    take(gi.y);
    take(gi.z);
    take(gi.w);
  }
  if (tid < n - 4 * n4) take(g[4 * n4 + tid]);
  for (int off = 32; off > 0; off >>= 1) {
    acc += shfl_xor_d(acc, off);
    bad += __shfl_xor(bad, off, kWave);
  }
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = acc;
    s_bad[threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sum = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    const uint32_t cnt = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
    partials[blockIdx.x] = make_double2(sum, (double)cnt);
  }
}

// lr_t of step t (1-based), in double, rounded once to float by the caller.
__device__ __forceinline__ double scheduled_lr(const gine_adamw_ctl& c, double t) {
  const double lr = (double)c.lr;
  if (c.schedule != GINE_LR_COSINE && c.schedule != GINE_LR_LINEAR) return lr;
  const double W = (double)c.warmup_steps, T = (double)c.total_steps;
  if (t <= W) return lr * t / W;
  const double s = fmin(1.0, (t - W) / fmax(1.0, T - W));
  const double r = (double)c.min_lr_ratio;
  if (c.schedule == GINE_LR_COSINE) return lr * (r + (1.0 - r) * 0.5 * (1.0 + cospi(s)));
  return lr * (r + (1.0 - r) * (1.0 - s));
}

__global__ __launch_bounds__(256) void k_adamw_ctl(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, float* __restrict__ step, int64_t n,
    const gine_adamw_ctl* __restrict__ ctl, const double2* __restrict__ partials,
    int num_partials, gine_adamw_report* __restrict__ report, float beta1, float beta2,
    float eps, float weight_decay) {
  __shared__ double s_sum[kAdamMaxBlocks];
  const gine_adamw_ctl c = *ctl;
  const float t_new = step[0] + 1.0f;
  const double t = (double)t_new;
  const float lr = (float)scheduled_lr(c, t);
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  // the first trip's loads are issued before the norm is summed, which hides under them
  int64_t i = tid;
  float4 gi = f4_zero(), pi = f4_zero(), mi = f4_zero(), vi = f4_zero();
  if (i < n4) {
    gi = reinterpret_cast<const float4*>(g)[i];
    pi = reinterpret_cast<float4*>(p)[i];
    mi = reinterpret_cast<float4*>(m)[i];
    vi = reinterpret_cast<float4*>(v)[i];
  }
  // the norm of the whole gradient: the same index-order sum in every workgroup, from LDS
  // (one parallel round of global loads; a loop over global memory pays a round trip each).
  // The non-finite counts are only tested against 0: an OR over the workgroup's threads.
  double sumsq = 0.0;
  bool bad = false;
  if (num_partials > 0) {
    bool mine = false;
    for (int j = threadIdx.x; j < num_partials; j += blockDim.x) {
      const double2 q = partials[j];
      s_sum[j] = q.x;
      mine |= q.y > 0.0;
    }
    bad = __syncthreads_or(mine) != 0;
#pragma unroll 16
    for (int j = 0; j < num_partials; ++j) sumsq += s_sum[j];
  }
  const float total_norm = (float)sqrt(sumsq);
  float coef = 1.0f;
  if (num_partials > 0 && c.max_norm > 0.0f && c.max_norm < __builtin_inff()) {
    const float q = c.max_norm / (total_norm + 1e-6f);
    coef = q > 1.0f ? 1.0f : q;  // clamp(max=1): a NaN stays a NaN
  }
  const bool skip = c.skip_nonfinite != 0 && num_partials > 0 &&
                    (bad || !(total_norm < __builtin_inff()));
  if (!skip) {
    const AdamW op{(float)(1.0 - (double)lr * (double)weight_decay),
                   (float)(-((double)lr / (1.0 - pow((double)beta1, t)))),
                   (float)sqrt(1.0 - pow((double)beta2, t)), 1.0f - beta1, 1.0f - beta2, beta2,
                   eps};
    while (i < n4) {
      op(gi.x * coef, pi.x, mi.x, vi.x);  // g * coef: one rounding (-ffp-contract=off)
      op(gi.y * coef, pi.y, mi.y, vi.y);
      op(gi.z * coef, pi.z, mi.z, vi.z);
      op(gi.w * coef, pi.w, mi.w, vi.w);
      reinterpret_cast<float4*>(p)[i] = pi;
      reinterpret_cast<float4*>(m)[i] = mi;
      reinterpret_cast<float4*>(v)[i] = vi;
      i += stride;
      if (i < n4) {
        gi = reinterpret_cast<const float4*>(g)[i];
        pi = reinterpret_cast<float4*>(p)[i];
        mi = reinterpret_cast<float4*>(m)[i];
        vi = reinterpret_cast<float4*>(v)[i];
      }
    }
    if (tid < n - 4 * n4) {
      const int64_t k = 4 * n4 + tid;
      float pk = p[k], mk = m[k], vk = v[k];
      op(g[k] * coef, pk, mk, vk);
      p[k] = pk;
      m[k] = mk;
      v[k] = vk;
    }
  }
  __syncthreads();  // every thread of this workgroup has read step[0]
  if (threadIdx.x == 0) {
    // k_adamw's two-level ticket; the top winner also writes the report
    unsigned int* ticket = reinterpret_cast<unsigned int*>(&step[1]);
    const unsigned int grp = blockIdx.x % kAdamGroups;
    const unsigned int groups = min(gridDim.x, (unsigned)kAdamGroups);
    const unsigned int size = (gridDim.x - grp + kAdamGroups - 1) / kAdamGroups;
    unsigned int* sub = reinterpret_cast<unsigned int*>(step + kAdamSubBase) + 32 * grp;
    if (atomicAdd(sub, 1u) == size - 1) {
      *sub = 0u;
      if (atomicAdd(ticket, 1u) == groups - 1) {
        if (!skip) step[0] = t_new;
        report->lr_t = lr;
        report->total_norm = total_norm;
        report->clip_coef = coef;
        if (skip) report->skipped = report->skipped + 1u;
        *ticket = 0u;
      }
    }
  }
}

}  // namespace
}  // namespace gine

extern "C" int gine_grad_sumsq_num_partials(int64_t n, int32_t* num_partials) {
  if (n < 0 || !num_partials) return GINE_ERR_INVALID;
  *num_partials = n > 0 ? (int32_t)adam_blocks(n) : 0;
  return GINE_OK;
}

extern "C" int gine_grad_sumsq(const float* grad, int64_t n, double* partials,
                               int32_t num_partials, void* stream) {
  if (n < 0) return GINE_ERR_INVALID;
  const int32_t want = n > 0 ? (int32_t)adam_blocks(n) : 0;
  if (num_partials != want) return GINE_ERR_INVALID;
  if (n == 0) return GINE_OK;
  if (!grad || !partials) return GINE_ERR_INVALID;
  if (((reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(partials)) & 15) != 0)
    return GINE_ERR_INVALID;
  hipLaunchKernelGGL(k_grad_sumsq, dim3((unsigned)want), dim3(256), 0, as_stream(stream), grad,
                     n, reinterpret_cast<double2*>(partials));
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_adamw_step_ctl(float* param, const float* grad, float* exp_avg,
                                   float* exp_avg_sq, float* step, int64_t n,
                                   const gine_adamw_ctl* ctl, const double* partials,
                                   int32_t num_partials, gine_adamw_report* report, float beta1,
                                   float beta2, float eps, float weight_decay, void* stream) {
  if (n < 0 || !step || !ctl || !report) return GINE_ERR_INVALID;
  if (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)) return GINE_ERR_INVALID;
  const uintptr_t al = reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) |
                       reinterpret_cast<uintptr_t>(exp_avg) |
                       reinterpret_cast<uintptr_t>(exp_avg_sq) |
                       reinterpret_cast<uintptr_t>(partials);
  if (n > 0 && (al & 15) != 0) return GINE_ERR_INVALID;
  if (((reinterpret_cast<uintptr_t>(ctl) | reinterpret_cast<uintptr_t>(report)) & 3) != 0)
    return GINE_ERR_INVALID;
  // NULL partials: no clipping and no non-finite test; otherwise gine_grad_sumsq's count
  const int32_t want = (partials && n > 0) ? (int32_t)adam_blocks(n) : 0;
  if (num_partials != want || (partials && n == 0)) return GINE_ERR_INVALID;
  hipLaunchKernelGGL(k_adamw_ctl, dim3((unsigned)adam_blocks(n)), dim3(256), 0,
                     as_stream(stream), param, grad, exp_avg, exp_avg_sq, step, n, ctl,
                     reinterpret_cast<const double2*>(partials), (int)num_partials, report,
                     beta1, beta2, eps, weight_decay);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_adamw_ctl_bytes(int64_t* ctl_bytes, int64_t* report_bytes) {
  if (!ctl_bytes || !report_bytes) return GINE_ERR_INVALID;
  *ctl_bytes = (int64_t)sizeof(gine_adamw_ctl);
  *report_bytes = (int64_t)sizeof(gine_adamw_report);
  return GINE_OK;
}
