// EMOS (ensemble model output statistics, Gneiting et al. 2005) fitted per group of rows by
// minimum CRPS on gfx950: the baseline a post-processing model has to beat.
//
// Per row the ensemble's summary statistics z = (mean, sd, dry, sd) map affinely to the raw
// parameters raw_k = theta[2k] + theta[2k+1] z_k of the predictive distribution of the loss's
// kind, through PostProcess's links (mu = raw_0, sigma = softplus(raw_1) + 1e-6,
// p = sigmoid(raw_2), sigma_u = softplus(raw_3) + 1e-6).  Per group g over its valid rows
//   J(theta) = (1/n_g) sum crps(pred(theta; row), y_row) + ridge |theta - theta0|^2
// is minimised by BFGS with Armijo backtracking; crps is the loss's closed form
// (gine_crpsdual.hpp), differentiated exactly by forward-mode dual numbers.
//   k_emos_predictors  members (strided view) + y  ->  pack [R, 4] = (mean, sd, dry, y)
//   k_emos_fit<KIND>   pack + segments             ->  theta [G, 2K], report [G, 8]
//   k_emos_predict     pack + theta                ->  pred [N, K] fp32
// All arithmetic fp64, every sum in a fixed order, no atomics: a group's result depends on
// that group's rows alone.
#include "gine_common.hpp"
#include "gine_crpsdual.hpp"

namespace gine {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxMembers = 64;        // as gine_ensemble_score
constexpr int kStageRows = 1024;       // rows of a group held in LDS (32 KiB); larger: from memory
constexpr int kMaxP = 8;               // 2 K at K = 4
constexpr int kMaxHalvings = 40;       // Armijo: steps 1, 1/2, ..., 2^-40
constexpr double kArmijo = 1e-4;
constexpr double kCurvature = 1e-10;   // H is updated when s.y > kCurvature |s| |y|
constexpr double kSoftplusOne = 0.54132485461291801609;  // log(e - 1): softplus gives 1
constexpr double kLinkEps = 1e-6;      // PostProcess: softplus + 1e-6

enum Mode : int { kDone = 0, kNewDirection = 1, kAccepted = 2, kRetry = 3 };

__device__ __forceinline__ double softplus64(double x) {  // no threshold
  return fmax(x, 0.0) + log1p(exp(-fabs(x)));
}
__device__ __forceinline__ double sigmoid64(double x) { return 1.0 / (1.0 + exp(-x)); }

// theta0 = (0, 1, b, 0, 0, 0, b, 0) truncated: the raw ensemble's mean with unit spread
__device__ __forceinline__ double theta_start(int i) {
  return i == 1 ? 1.0 : (i == 2 || i == 6) ? kSoftplusOne : 0.0;
}

// Destination of collated row n (= day * S + station) in the group-major pack.
__device__ __forceinline__ int64_t pack_row(int64_t n, int64_t S, int64_t T) {
  return S > 0 ? (n % S) * T + n / S : n;
}

// One thread per row: the members in member order, twice (mean, then the spread about it).
__global__ __launch_bounds__(kThreads) void k_emos_predictors(
    const float* __restrict__ members, int64_t row_stride, int64_t member_stride, int M,
    double scale, double shift, double c, const float* __restrict__ y, int64_t n, int64_t S,
    double* __restrict__ pack) {
  const int64_t row = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (row >= n) return;
  const float* mem = members + row * row_stride;
  double sum = 0.0;
  int m = 0, below = 0;
#pragma unroll 1
  for (int i = 0; i < M; ++i) {
    const double x = shift + scale * (double)mem[i * member_stride];
    if (x == x) {
      sum += x;
      ++m;
      below += x <= c ? 1 : 0;
    }
  }
  const double nan = __builtin_nan("");
  double mean = nan, sd = nan, dry = nan;
  if (m > 0) {
    const double dm = (double)m;
    mean = sum / dm;
    double ss = 0.0;
#pragma unroll 1
    for (int i = 0; i < M; ++i) {
      const double x = shift + scale * (double)mem[i * member_stride];
      if (x == x) ss += (x - mean) * (x - mean);
    }
    sd = sqrt(ss / dm);
    dry = (double)below / dm;
  }
  double* out = pack + pack_row(row, S, S > 0 ? n / S : 0) * 4;
  out[0] = mean;
  out[1] = sd;
  out[2] = dry;
  out[3] = y ? (double)y[row] : nan;
}

// The K prediction columns of one row from its raw parameters; dlink[k] = d pred_k / d raw_k.
template <int K>
__device__ __forceinline__ void emos_links(const double (&raw)[K], double (&pred)[K],
                                           double (&dlink)[K]) {
  pred[0] = raw[0];
  dlink[0] = 1.0;
  pred[1] = softplus64(raw[1]) + kLinkEps;
  dlink[1] = sigmoid64(raw[1]);
  if constexpr (K > 2) {
    pred[2] = sigmoid64(raw[2]);
    dlink[2] = pred[2] * (1.0 - pred[2]);
  }
  if constexpr (K > 3) {
    pred[3] = softplus64(raw[3]) + kLinkEps;
    dlink[3] = sigmoid64(raw[3]);
  }
}

// Fixed-order sum over the workgroup of NC values per thread: thread j's values were formed
// from rows j, j + 256, ... in order; the tree adds them in an order that depends on nothing
// but the thread index.  Totals in s_red[col * kThreads].
template <int NC>
__device__ __forceinline__ void reduce_cols(const double (&acc)[NC], double* s_red) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < NC; ++j) s_red[j * kThreads + t] = acc[j];
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int j = 0; j < NC; ++j) s_red[j * kThreads + t] += s_red[j * kThreads + t + s];
    }
    __syncthreads();
  }
}

// One workgroup owns group blockIdx.x for the whole optimisation.  Every pass of the loop
// evaluates J and its gradient at the trial point (all 256 lanes, the only shared work),
// then wave 0 runs the BFGS algebra on the state in LDS: thread 0 the scalars and the
// branches, lanes i < P row i of the matrix products.  Every loop has a fixed bound.
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_emos_fit(
    const double* __restrict__ pack, const int64_t* __restrict__ ptr, int64_t num_rows,
    double u_fixed, double xi, double c, double ridge, double gtol, int max_iter, int min_rows,
    double* __restrict__ theta_out, double* __restrict__ report) {
  constexpr int K = LossK<KIND>::value;
  constexpr int P = 2 * K;
  static_assert(P <= kMaxP && P <= kWave, "one lane of wave 0 per parameter");
  __shared__ double s_rows[kStageRows * 4];
  __shared__ double s_red[(P + 1) * kThreads];
  __shared__ double s_H[P * P];
  __shared__ double s_theta[P], s_trial[P], s_g[P], s_d[P], s_s[P], s_y[P], s_Hy[P];
  __shared__ double s_J, s_crps, s_gmax, s_alpha, s_gd, s_rho, s_coef, s_nvalid;
  __shared__ int s_it, s_nev, s_ls, s_status, s_first, s_mode, s_upd;

  const int t = threadIdx.x;
  const int64_t g = blockIdx.x;
  // the segment, clamped into the pack whatever ptr holds
  int64_t lo = ptr[g], hi = ptr[g + 1];
  lo = lo < 0 ? 0 : (lo > num_rows ? num_rows : lo);
  hi = hi < lo ? lo : (hi > num_rows ? num_rows : hi);
  const int64_t n = hi - lo;
  const bool staged = n <= kStageRows;
  const double* __restrict__ grp = pack + lo * 4;
  if (staged) {
    for (int64_t i = t; i < n * 4; i += kThreads) s_rows[i] = grp[i];
  }
  __syncthreads();
  const double* rows = staged ? s_rows : grp;

  {  // the valid rows: a target and at least one member
    double cnt[1] = {0.0};
    for (int64_t i = t; i < n; i += kThreads) {
      const double mean = rows[i * 4], yy = rows[i * 4 + 3];
      cnt[0] += (mean == mean && yy == yy) ? 1.0 : 0.0;
    }
    reduce_cols<1>(cnt, s_red);
  }
  if (t == 0) {
    s_nvalid = s_red[0];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      s_theta[i] = theta_start(i);
      s_trial[i] = theta_start(i);
#pragma unroll
      for (int j = 0; j < P; ++j) s_H[i * P + j] = i == j ? 1.0 : 0.0;
    }
    s_J = s_crps = s_gmax = __builtin_nan("");
    s_alpha = 1.0;
    s_gd = 0.0;
    s_it = s_nev = s_ls = 0;
    s_first = 1;
    s_status = s_red[0] < (double)min_rows ? 3 : -1;
  }
  __syncthreads();
  const double nvalid = s_nvalid;

  if (s_status < 0) {  // uniform
    const int max_pass = 1 + max_iter * (kMaxHalvings + 1);
#pragma unroll 1
    for (int pass = 0; pass < max_pass; ++pass) {
      // ---- J and dJ/dtheta at the trial point: lane t walks rows t, t + 256, ... in order
      double th[P];
#pragma unroll
      for (int i = 0; i < P; ++i) th[i] = s_trial[i];
      double acc[P + 1];
#pragma unroll
      for (int i = 0; i <= P; ++i) acc[i] = 0.0;
#pragma unroll 1
      for (int64_t i = t; i < n; i += kThreads) {
        const double mean = rows[i * 4], sd = rows[i * 4 + 1], dry = rows[i * 4 + 2];
        const double yy = rows[i * 4 + 3];
        if (!(mean == mean && yy == yy)) continue;
        double z[K], raw[K], pred[K], dlink[K];
        z[0] = mean;
        z[1] = sd;
        if constexpr (K > 2) z[2] = dry;
        if constexpr (K > 3) z[3] = sd;
#pragma unroll
        for (int k = 0; k < K; ++k) raw[k] = th[2 * k] + th[2 * k + 1] * z[k];
        emos_links<K>(raw, pred, dlink);
        Dual<K> v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = var<K>(pred[k], k);
        Dual<K> r;
        if constexpr (KIND == GINE_LOSS_NORMAL) {
          r = crps_normal(v[0], v[1], yy);
        } else if constexpr (KIND == GINE_LOSS_MIXED_NORMAL) {
          r = crps_mixed_normal(v[0], v[1], v[2], yy, c);
        } else {
          r = crps_mixed<K, false>(v[0], v[1], v[2], v[3], cst<K>(u_fixed), yy, c, xi, 0.0);
        }
        acc[0] += r.v;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const double graw = r.d[k] * dlink[k];
          acc[1 + 2 * k] += graw;
          acc[2 + 2 * k] += graw * z[k];
        }
      }
      reduce_cols<P + 1>(acc, s_red);

      // ---- thread 0: accept or shorten the step, test for the end
      if (t == 0) {
        const double ct = s_red[0] / nvalid;
        double pen = 0.0, gt[P];
#pragma unroll
        for (int i = 0; i < P; ++i) {
          const double dv = s_trial[i] - theta_start(i);
          pen += dv * dv;
          gt[i] = s_red[(1 + i) * kThreads] / nvalid + 2.0 * ridge * dv;
        }
        const double Jt = ct + ridge * pen;
        s_nev += 1;
        int mode;
        if (s_first) {
          s_first = 0;
          s_J = Jt;
          s_crps = ct;
#pragma unroll
          for (int i = 0; i < P; ++i) s_g[i] = gt[i];
          mode = kNewDirection;
        } else if (Jt - Jt == 0.0 && Jt <= s_J + kArmijo * s_alpha * s_gd) {
          double sy = 0.0, ss = 0.0, yy2 = 0.0;
#pragma unroll
          for (int i = 0; i < P; ++i) {
            const double si = s_trial[i] - s_theta[i], yi = gt[i] - s_g[i];
            s_s[i] = si;
            s_y[i] = yi;
            s_theta[i] = s_trial[i];
            s_g[i] = gt[i];
            sy += si * yi;
            ss += si * si;
            yy2 += yi * yi;
          }
          s_J = Jt;
          s_crps = ct;
          s_it += 1;
          s_upd = sy > kCurvature * sqrt(ss) * sqrt(yy2) ? 1 : 0;
          s_rho = 1.0 / sy;
          mode = kAccepted;
        } else if (s_ls >= kMaxHalvings) {
          s_status = 2;  // no decrease along d: theta is the last accepted point
          mode = kDone;
        } else {
          s_ls += 1;
          s_alpha *= 0.5;
#pragma unroll
          for (int i = 0; i < P; ++i) s_trial[i] = s_theta[i] + s_alpha * s_d[i];
          mode = kRetry;
        }
        if (mode == kNewDirection || mode == kAccepted) {
          double gmax = 0.0;
#pragma unroll
          for (int i = 0; i < P; ++i) gmax = fmax(gmax, fabs(s_g[i]));
          s_gmax = gmax;
          if (gmax <= gtol * fmax(1.0, fabs(s_J))) s_status = 0;
          else if (s_it >= max_iter) s_status = 1;
          if (s_status >= 0) mode = kDone;
        }
        s_mode = mode;
      }
      __syncthreads();
      const int mode = s_mode;  // uniform from here on
      if (mode == kDone) break;
      if (mode == kRetry) continue;

      // ---- the inverse Hessian: H <- (I - rho s y') H (I - rho y s') + rho s s'
      if (mode == kAccepted && s_upd) {
        if (t < P) {
          double a = 0.0;
#pragma unroll
          for (int j = 0; j < P; ++j) a += s_H[t * P + j] * s_y[j];
          s_Hy[t] = a;
        }
        __syncthreads();
        if (t == 0) {
          double yHy = 0.0;
#pragma unroll
          for (int i = 0; i < P; ++i) yHy += s_y[i] * s_Hy[i];
          s_coef = s_rho * s_rho * yHy + s_rho;
        }
        __syncthreads();
        if (t < P) {
          const double rho = s_rho, coef = s_coef, si = s_s[t], hyi = s_Hy[t];
#pragma unroll
          for (int j = 0; j < P; ++j)
            s_H[t * P + j] = s_H[t * P + j] - rho * (si * s_Hy[j] + hyi * s_s[j]) +
                             coef * (si * s_s[j]);
        }
        __syncthreads();
      }
      // ---- the direction d = -H g, steepest descent when it does not descend
      if (t < P) {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) a += s_H[t * P + j] * s_g[j];
        s_d[t] = -a;
      }
      __syncthreads();
      if (t == 0) {
        double gd = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) gd += s_g[i] * s_d[i];
        if (!(gd < 0.0)) {
          gd = 0.0;
#pragma unroll
          for (int i = 0; i < P; ++i) {
#pragma unroll
            for (int j = 0; j < P; ++j) s_H[i * P + j] = i == j ? 1.0 : 0.0;
            s_d[i] = -s_g[i];
            gd -= s_g[i] * s_g[i];
          }
        }
        s_gd = gd;
        s_alpha = 1.0;
        s_ls = 0;
#pragma unroll
        for (int i = 0; i < P; ++i) s_trial[i] = s_theta[i] + s_d[i];
      }
      __syncthreads();
    }
  }

  if (t == 0) {
    if (s_status < 0) s_status = 1;  // the pass bound: cannot be reached before max_iter
#pragma unroll
    for (int i = 0; i < P; ++i) theta_out[g * P + i] = s_theta[i];
    double* rep = report + g * 8;
    rep[0] = s_J;
    rep[1] = s_crps;
    rep[2] = s_gmax;
    rep[3] = (double)s_it;
    rep[4] = (double)s_nev;
    rep[5] = nvalid;
    rep[6] = (double)s_status;
    rep[7] = 0.0;
  }
}

// One thread per collated row: the row's predictors from the pack, its station's theta.
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_emos_predict(const double* __restrict__ pack,
                                                           const double* __restrict__ theta,
                                                           int64_t n, int64_t S,
                                                           float* __restrict__ pred_out) {
  constexpr int K = LossK<KIND>::value;
  constexpr int P = 2 * K;
  const int64_t row = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (row >= n) return;
  const double* in = pack + pack_row(row, S, S > 0 ? n / S : 0) * 4;
  const double* th = theta + (S > 0 ? row % S : 0) * P;
  const double mean = in[0], sd = in[1], dry = in[2];
  double z[K], raw[K], pred[K], dlink[K];
  z[0] = mean;
  z[1] = sd;
  if constexpr (K > 2) z[2] = dry;
  if constexpr (K > 3) z[3] = sd;
#pragma unroll
  for (int k = 0; k < K; ++k) raw[k] = th[2 * k] + th[2 * k + 1] * z[k];
  emos_links<K>(raw, pred, dlink);
#pragma unroll
  for (int k = 0; k < K; ++k)
    pred_out[row * K + k] = mean == mean ? (float)pred[k] : __builtin_nanf("");
}

int emos_k(int kind) {
  return kind == GINE_LOSS_NORMAL ? 2 : kind == GINE_LOSS_MIXED_NORMAL ? 3
         : kind == GINE_LOSS_MIXED ? 4 : -1;  // MIXED_U: its u is a per-row network output
}

int check_rows(int64_t num_rows, int64_t num_stations) {
  if (num_rows < 0 || num_stations < 0) return GINE_ERR_INVALID;
  if (num_stations > 0 && num_rows % num_stations != 0) return GINE_ERR_INVALID;
  if (ceil_div(num_rows, kThreads) > 0x7fffffff) return GINE_ERR_TOO_LARGE;
  return GINE_OK;
}

}  // namespace
}  // namespace gine

using namespace gine;

extern "C" int gine_emos_predictors(const float* members, int64_t row_stride,
                                    int64_t member_stride, int32_t num_members, double scale,
                                    double shift, double c, const float* y, int64_t num_rows,
                                    int64_t num_stations, double* pack, void* stream) {
  const int rc = check_rows(num_rows, num_stations);
  if (rc != GINE_OK) return rc;
  if (row_stride < 0 || member_stride < 0) return GINE_ERR_INVALID;
  if (num_members < 1 || num_members > kMaxMembers) return GINE_ERR_INVALID;
  if (!(c == c)) return GINE_ERR_INVALID;
  if (num_rows == 0) return GINE_OK;
  if (!members || !pack) return GINE_ERR_INVALID;
  hipLaunchKernelGGL(k_emos_predictors, dim3((unsigned)ceil_div(num_rows, kThreads)),
                     dim3(kThreads), 0, as_stream(stream), members, row_stride, member_stride,
                     (int)num_members, scale, shift, c, y, num_rows, num_stations, pack);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_emos_fit(const double* pack, const int64_t* ptr, int64_t num_groups,
                             int64_t num_rows, int32_t kind, double u, double xi, double c,
                             double ridge, double gtol, int32_t max_iter, int32_t min_rows,
                             double* theta, double* report, void* stream) {
  if (emos_k(kind) < 0) return GINE_ERR_INVALID;
  if (num_groups < 0 || num_rows < 0) return GINE_ERR_INVALID;
  if (!(c == c) || !(ridge >= 0.0) || !(gtol >= 0.0)) return GINE_ERR_INVALID;
  if (ridge - ridge != 0.0 || gtol - gtol != 0.0) return GINE_ERR_INVALID;  // finite
  if (kind == GINE_LOSS_MIXED && (!(xi > 0.0 && xi < 1.0) || !(u > c))) return GINE_ERR_INVALID;
  if (max_iter < 0 || max_iter > GINE_EMOS_MAX_ITER || min_rows < 1) return GINE_ERR_INVALID;
  if (num_groups > 0x7fffffff) return GINE_ERR_TOO_LARGE;
  if (num_groups == 0) return GINE_OK;
  if (!ptr || !theta || !report || (num_rows > 0 && !pack)) return GINE_ERR_INVALID;
  const dim3 grid((unsigned)num_groups);
#define LAUNCH_EMOS_FIT(KIND_)                                                                \
  hipLaunchKernelGGL((k_emos_fit<KIND_>), grid, dim3(kThreads), 0, as_stream(stream), pack,   \
                     ptr, num_rows, u, xi, c, ridge, gtol, (int)max_iter, (int)min_rows,      \
                     theta, report)
  switch (kind) {
    case GINE_LOSS_NORMAL: LAUNCH_EMOS_FIT(GINE_LOSS_NORMAL); break;
    case GINE_LOSS_MIXED_NORMAL: LAUNCH_EMOS_FIT(GINE_LOSS_MIXED_NORMAL); break;
    default: LAUNCH_EMOS_FIT(GINE_LOSS_MIXED); break;
  }
#undef LAUNCH_EMOS_FIT
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_emos_predict(const double* pack, const double* theta, int64_t num_rows,
                                 int64_t num_stations, int32_t kind, float* pred,
                                 void* stream) {
  if (emos_k(kind) < 0) return GINE_ERR_INVALID;
  const int rc = check_rows(num_rows, num_stations);
  if (rc != GINE_OK) return rc;
  if (num_rows == 0) return GINE_OK;
  if (!pack || !theta || !pred) return GINE_ERR_INVALID;
  const dim3 grid((unsigned)ceil_div(num_rows, kThreads));
#define LAUNCH_EMOS_PREDICT(KIND_)                                                           \
  hipLaunchKernelGGL((k_emos_predict<KIND_>), grid, dim3(kThreads), 0, as_stream(stream),    \
                     pack, theta, num_rows, num_stations, pred)
  switch (kind) {
    case GINE_LOSS_NORMAL: LAUNCH_EMOS_PREDICT(GINE_LOSS_NORMAL); break;
    case GINE_LOSS_MIXED_NORMAL: LAUNCH_EMOS_PREDICT(GINE_LOSS_MIXED_NORMAL); break;
    default: LAUNCH_EMOS_PREDICT(GINE_LOSS_MIXED); break;
  }
#undef LAUNCH_EMOS_PREDICT
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}
