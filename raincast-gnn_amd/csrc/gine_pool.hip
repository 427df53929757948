// The linear pool of M checkpoint forecasts on gfx950:
//   Fbar(x) = sum_m w_m F_m(x),   sfbar(x) = sum_m w_m sf_m(x)   (members in index order),
// F_m the distribution of gine_forecast.hip for member m's row of preds [M, N, K] fp32.
// Probabilities, quantiles / return levels (inf{x : Fbar(x) >= q}, a safeguarded Newton /
// bisection between the members' quantiles) and the scores of a set of targets:
//   crps_pool(y) = sum_m w_m crps_m(y) - V,   V = int sum_m w_m (F_m - Fbar)^2 dx,
// the members' closed forms minus the pool's diversity V, which has none and is integrated
// by a fixed rule (16-point Gauss-Legendre between sorted breakpoints, one 32-point
// Gauss-Jacobi panel for the Pareto tails).  Every result and all arithmetic fp64.
// For fitting the weights, gine_pool_pairs sums per segment of rows what that
// CRPS needs as a function of w: the members' CRPS and the pairwise int (F_m - F_l)^2 dx.
//
// RowP, load_row, cdf_at, sf_at, quantile_at and crps_row are restated from
// gine_forecast.hip expression for expression (that file's kernels stay what they are): a
// pool of one member, or of copies of one member, returns the bits of gine_forecast_*.
#include "gine_common.hpp"

namespace gine {
namespace {

constexpr double kInvSqrtPi = 0.56418958354775628695;   // 1/sqrt(pi)
constexpr double kLogSqrt2Pi = 0.91893853320467274178;  // log(sqrt(2 pi))
constexpr double kSqrt2 = 1.41421356237309504880;
constexpr int kThreads = 256;
constexpr int kRows = 64;            // rows per tile of the Brier / count reduction
constexpr int kMaxPoints = 1 << 24;  // thresholds / levels per call: a tile's pairs fit 32 bits
constexpr int kPoolMaxM = 32;        // members
// k_pool_points stages rows x M RowPs (80 B each) in 40 KiB of LDS, three workgroups a CU:
// 64 rows per workgroup up to M = 8, then 512 / M (16 at M = 32).  64 x 32 RowPs would be
// the CU's whole 160 KiB.
constexpr int kPoolSlots = 512;
constexpr int kPoolK = 11;                          // mu + k sigma breakpoints per member
constexpr int kPoolMaxBp = 12 * kPoolMaxM + 2;      // + u_m per member, + c
constexpr int kGL = 16;                             // Gauss-Legendre nodes per panel
constexpr int kGJ = 32;                             // Gauss-Jacobi nodes of the tail panel
constexpr int kPoolNewton = 24;                     // iterations that may take a Newton step
constexpr int kPoolIter = kPoolNewton + 64;         // then bisection in bit space: <= 64 halvings

// 16-point Gauss-Legendre on [-1, 1]: the positive nodes and their weights
__constant__ double kGLx[8] = {0.09501250983763745, 0.2816035507792589, 0.4580167776572274,
                               0.6178762444026438,  0.755404408355003,  0.8656312023878318,
                               0.9445750230732326,  0.9894009349916499};
__constant__ double kGLw[8] = {0.1894506104550681,  0.18260341504492328, 0.16915651939500212,
                               0.14959598881657638, 0.12462897125553363, 0.09515851168249231,
                               0.06225352393864763, 0.027152459411756466};
__constant__ double kBpK[kPoolK] = {-8.0, -5.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 5.0, 8.0};

template <int KIND>
struct Kind {
  static constexpr int K = KIND == GINE_LOSS_NORMAL ? 2
                           : KIND == GINE_LOSS_MIXED_NORMAL ? 3
                           : KIND == GINE_LOSS_MIXED ? 4 : 5;
  static constexpr bool atom = KIND != GINE_LOSS_NORMAL;  // point mass at c
  static constexpr bool tail = KIND == GINE_LOSS_MIXED || KIND == GINE_LOSS_MIXED_U;
};

// ---------------------------------------------------------------------------------------
// one member: gine_forecast.hip's definitions, restated
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double upper_phi(double z) { return 0.5 * erfc(z / kSqrt2); }
__device__ __forceinline__ double lower_phi(double z) { return 0.5 * erfc(-z / kSqrt2); }

struct RowP {
  double mu, sigma, p, q;  // q = 1 - p
  double su, u;            // tail scale and threshold
  double Pc, Sc;           // F(c) and P(Y > c) = q upper_phi(z(c))
  double mU, omU;          // m_u and 1 - m_u = q upper_phi(z(u))
};

template <int KIND>
__device__ __forceinline__ RowP load_row(const float* __restrict__ pred, int64_t i,
                                         double u_fixed, double c) {
  constexpr int K = Kind<KIND>::K;
  RowP r;
  r.mu = (double)pred[i * K];
  r.sigma = (double)pred[i * K + 1];
  r.p = 0.0;
  r.su = 1.0;
  r.u = u_fixed;
  if constexpr (Kind<KIND>::atom) r.p = (double)pred[i * K + 2];
  if constexpr (Kind<KIND>::tail) r.su = (double)pred[i * K + 3];
  if constexpr (KIND == GINE_LOSS_MIXED_U) r.u = (double)pred[i * K + 4];
  r.q = 1.0 - r.p;
  r.Pc = 0.0;
  r.Sc = 1.0;
  r.mU = 1.0;
  r.omU = 0.0;
  if constexpr (Kind<KIND>::atom) {
    const double zc = (c - r.mu) / r.sigma;
    r.Pc = r.p + r.q * lower_phi(zc);
    r.Sc = r.q * upper_phi(zc);
  }
  if constexpr (Kind<KIND>::tail) {
    const double zu = (r.u - r.mu) / r.sigma;
    r.mU = r.p + r.q * lower_phi(zu);
    r.omU = r.q * upper_phi(zu);
  }
  return r;
}

__device__ __forceinline__ double gpd_upper(const RowP& r, double x, double xi) {
  const double t = (x - r.u) / r.su;
  return pow(1.0 + xi * t, -1.0 / xi);
}

template <int KIND>
__device__ __forceinline__ double cdf_at(const RowP& r, double x, double c, double xi) {
  if constexpr (Kind<KIND>::atom) {
    if (x < c) return 0.0;
  }
  if constexpr (Kind<KIND>::tail) {
    if (x >= r.u) return r.mU + r.omU * (1.0 - gpd_upper(r, x, xi));
  }
  return r.p + r.q * lower_phi((x - r.mu) / r.sigma);
}

template <int KIND>
__device__ __forceinline__ double sf_at(const RowP& r, double x, double c, double xi) {
  if constexpr (Kind<KIND>::atom) {
    if (x < c) return 1.0;
  }
  if constexpr (Kind<KIND>::tail) {
    if (x >= r.u) return r.omU * gpd_upper(r, x, xi);
  }
  return r.q * upper_phi((x - r.mu) / r.sigma);
}

__device__ __forceinline__ double upper_phi_inv(double v) { return -normcdfinv(v); }

template <int KIND>
__device__ __forceinline__ double quantile_at(const RowP& r, double level, bool upper, double c,
                                              double xi) {
  const double inf = __builtin_huge_val();
  if (!(level >= 0.0 && level <= 1.0)) return __builtin_nan("");
  if (level == (upper ? 0.0 : 1.0)) return inf;
  if constexpr (Kind<KIND>::atom) {
    if (upper ? level >= r.Sc : level <= r.Pc) return c;
  } else {
    if (level == (upper ? 1.0 : 0.0)) return -inf;
  }
  const double s = upper ? level : 1.0 - level;  // mass above the quantile
  if constexpr (Kind<KIND>::tail) {
    if (upper ? level < r.omU : level > r.mU)
      return r.u + r.su / xi * (pow(s / r.omU, -xi) - 1.0);
  }
  const double v = s / r.q;                                // above the quantile
  const double w = upper ? 1.0 - v : (level - r.p) / r.q;  // below it
  const bool high = upper ? v <= 0.5 : w > 0.5;
  const double z = upper_phi_inv(high ? v : w);
  double x = high ? r.mu + r.sigma * z : r.mu - r.sigma * z;
  if constexpr (Kind<KIND>::atom) x = fmax(x, c);
  if constexpr (Kind<KIND>::tail) x = fmin(x, r.u);
  return x;
}

__device__ __forceinline__ double Phi(double z) { return 0.5 * (1.0 + erf(z / kSqrt2)); }
__device__ __forceinline__ double phi(double z) { return exp(-0.5 * z * z - kLogSqrt2Pi); }

__device__ double crps_normal(double mu, double sigma, double y) {
  const double z = (y - mu) / sigma;
  return sigma * (z * (2.0 * Phi(z) - 1.0) + 2.0 * phi(z) - kInvSqrtPi);
}

__device__ double crps_mixed_normal(double mu, double sigma, double p, double y, double c) {
  const double yt = (y - mu) / sigma;
  const double ct = (c - mu) / sigma;
  const double q = 1.0 - p;
  const double Pc = p + q * Phi(ct);
  const double t1 = yt * (2.0 * (p + q * Phi(yt)) - 1.0);
  const double t2 = -(ct * (Pc * Pc));
  const double t3 = 2.0 * (q * (-phi(ct)) * Pc);
  const double t4 = -2.0 * (q * (-phi(yt)));
  const double t5 = (-kInvSqrtPi) * ((q * q) * (1.0 - Phi(kSqrt2 * ct)));
  return sigma * (t1 + t2 + t3 + t4 + t5);
}

__device__ double pareto_crps(double y, double u, double m, double s, double xi) {
  const double yt = (y - u) / s;
  const double cdf = yt <= 0.0 ? 0.0 : 1.0 - pow(1.0 + xi * yt, -1.0 / xi);
  const double om = 1.0 - m;
  return s * (fabs(yt) - (2.0 / (1.0 - xi)) * (om * (1.0 - pow(1.0 - cdf, 1.0 - xi))) +
              (1.0 / (2.0 - xi)) * (om * om));
}

__device__ __forceinline__ double crps_mixed(double mu, double sigma, double p, double su, double u, double y,
                             double c, double xi) {
  const double ct = (c - mu) / sigma;
  const double ut = (u - mu) / sigma;
  const double yt = (y - mu) / sigma;
  const double q = 1.0 - p;
  const double m_u = p + q * Phi(ut);
  const double Pc = p + q * Phi(ct);
  const double Pu = q * (1.0 - Phi(ut));
  const double t2 = ut * (Pu * Pu) - ct * (Pc * Pc);
  const double t3 = -2.0 * (q * phi(ct) * Pc + q * phi(ut) * Pu);
  const double t5 = (-kInvSqrtPi) * ((q * q) * (Phi(kSqrt2 * ut) - Phi(kSqrt2 * ct)));
  if (y < u) {
    const double mixed =
        sigma * (yt * (2.0 * (p + q * Phi(yt)) - 1.0) + t2 + t3 + 2.0 * (q * phi(yt)) + t5);
    return mixed + pareto_crps(u, u, m_u, su, xi);
  }
  const double upper = sigma * (ut + t2 + t3 + (-2.0) * (q * (-phi(ut)) + ut * Pu) + t5);
  return pareto_crps(y, u, m_u, su, xi) + upper;
}

template <int KIND>
__device__ __forceinline__ double crps_row(const RowP& r, double y, double c, double xi) {
  if constexpr (KIND == GINE_LOSS_NORMAL) return crps_normal(r.mu, r.sigma, y);
  else if constexpr (KIND == GINE_LOSS_MIXED_NORMAL)
    return crps_mixed_normal(r.mu, r.sigma, r.p, y, c);
  else return crps_mixed(r.mu, r.sigma, r.p, r.su, r.u, y, c, xi);
}

// ---------------------------------------------------------------------------------------
// the pool
// ---------------------------------------------------------------------------------------
// One member at x >= c for the quantile solver: f = F(x) (upper: P(Y > x)), cdf_at's / sf_at's
// expressions, and g = the density there (the Newton step's slope), from one erfc or one pow.
template <int KIND>
__device__ __forceinline__ void member_eval(const RowP& r, double x, bool upper, double xi,
                                            double& f, double& g) {
  if constexpr (Kind<KIND>::tail) {
    if (x >= r.u) {
      const double b = 1.0 + xi * ((x - r.u) / r.su);
      const double gp = pow(b, -1.0 / xi);
      f = upper ? r.omU * gp : r.mU + r.omU * (1.0 - gp);
      g = r.omU / r.su * (gp / b);
      return;
    }
  }
  const double z = (x - r.mu) / r.sigma;
  const double e = 0.5 * erfc((upper ? z : -z) / kSqrt2);
  f = upper ? r.q * e : r.p + r.q * e;
  g = r.q * phi(z) / r.sigma;
}

// Weights in LDS: w[m] = w_m / w_max, and w[kPoolMaxM] = w_max.  A weighted sum is formed as
// w_max sum_m (w_m / w_max) t_m: with equal weights the ratios are 1, so 2^k copies of one
// member give that member's bits even where t_m is subnormal (0.5 t + 0.5 t would round).
__device__ __forceinline__ void stage_weights(const double* __restrict__ wts, int M, double* w) {
  double wmax = wts[0];
  for (int m = 1; m < M; ++m) wmax = fmax(wmax, wts[m]);
  if ((int)threadIdx.x < M) w[threadIdx.x] = wts[threadIdx.x] / wmax;
  if (threadIdx.x == 0) w[kPoolMaxM] = wmax;
}

// sum_m w_m F_m(x) (UPPER: of sf_m), members in index order; the first term starts the sum,
// so one member of weight 1 gives its own bits
template <int KIND, bool UPPER>
__device__ __forceinline__ double pool_prob(const RowP* r, const double* w, int M, double x,
                                            double c, double xi) {
  if constexpr (Kind<KIND>::atom) {
    if (x < c) return UPPER ? 1.0 : 0.0;  // exactly, whatever the weights round to
  }
  double a = w[0] * (UPPER ? sf_at<KIND>(r[0], x, c, xi) : cdf_at<KIND>(r[0], x, c, xi));
  for (int m = 1; m < M; ++m)
    a += w[m] * (UPPER ? sf_at<KIND>(r[m], x, c, xi) : cdf_at<KIND>(r[m], x, c, xi));
  return w[kPoolMaxM] * a;
}

// sum_m w_m (F_m(x) - Fbar(x))^2 in two passes: equal members give exactly 0.  UPPER: from
// the exceedance probabilities (the same differences, kept to relative accuracy far out).
template <int KIND, bool UPPER>
__device__ __forceinline__ double pool_var(const RowP* r, const double* w, int M, double x,
                                           double c, double xi) {
  const double fb = pool_prob<KIND, UPPER>(r, w, M, x, c, xi);
  double v = 0.0;
  for (int m = 0; m < M; ++m) {
    const double d =
        (UPPER ? sf_at<KIND>(r[m], x, c, xi) : cdf_at<KIND>(r[m], x, c, xi)) - fb;
    v += w[m] * (d * d);
  }
  return w[kPoolMaxM] * v;
}

// doubles as integers in their own order (finite values)
__device__ __forceinline__ uint64_t ordered_bits(double v) {
  const uint64_t k = (uint64_t)__double_as_longlong(v);
  return (k >> 63) ? ~k : k | 0x8000000000000000ull;
}
__device__ __forceinline__ double from_ordered_bits(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k));
}

// inf{x : Fbar(x) >= q}; upper: `level` is s = 1 - q and the equation is sfbar(x) = s.
template <int KIND>
__device__ __forceinline__ double pool_quantile(const RowP* r, const double* w, int M, double level, bool upper,
                                double c, double xi) {
  const double inf = __builtin_huge_val();
  if (!(level >= 0.0 && level <= 1.0)) return __builtin_nan("");
  if (level == (upper ? 0.0 : 1.0)) return inf;
  if constexpr (Kind<KIND>::atom) {
    double a = w[0] * (upper ? r[0].Sc : r[0].Pc);
    for (int m = 1; m < M; ++m) a += w[m] * (upper ? r[m].Sc : r[m].Pc);
    a *= w[kPoolMaxM];
    if (upper ? level >= a : level <= a) return c;
  } else {
    if (level == (upper ? 1.0 : 0.0)) return -inf;
  }
  double lo = inf, hi = -inf;
#pragma unroll 1
  for (int m = 0; m < M; ++m) {
    const double qm = quantile_at<KIND>(r[m], level, upper, c, xi);
    lo = fmin(lo, qm);
    hi = fmax(hi, qm);
  }
  if (lo == hi) return lo;  // one member, or members that agree: its own value
  // h(x) = Fbar(x) - q, or s - sfbar(x): increasing, slope = the pool's density d; the root is
  // the least x with h(x) >= 0.  Below lo every member is under the level, so h(lo) >= 0
  // makes lo the answer (pass 0).  Then [a, b]: h(a) < 0; b = hi, or a point with h(b) >= 0.
  double a = lo, b = hi, xe = lo, h = 0.0, d = 0.0;
#pragma unroll 1
  for (int it = 0; it <= kPoolIter; ++it) {
    double xn = lo;
    if (it > 0) {
      const uint64_t ka = ordered_bits(a), kb = ordered_bits(b);
      if (kb - ka <= 1) break;  // adjacent doubles
      xn = __builtin_nan("");
      if (it <= kPoolNewton && d > 0.0) {
        // the Newton point, pushed 2^-10 of the step past it: once the step is small the
        // point lands beyond the root, so both ends of the bracket close in
        const double step = -h / d;
        xn = xe + (step + step * 0x1p-10);
      }
      if (!(xn > a && xn < b)) xn = from_ordered_bits(ka + (kb - ka) / 2);
    }
    double f = 0.0, g = 0.0;
#pragma unroll 1
    for (int m = 0; m < M; ++m) {
      double fm, gm;
      member_eval<KIND>(r[m], xn, upper, xi, fm, gm);
      f += w[m] * fm;
      g += w[m] * gm;
    }
    f *= w[kPoolMaxM];
    h = upper ? level - f : f - level;
    d = w[kPoolMaxM] * g;
    xe = xn;
    if (it == 0) {
      if (h >= 0.0) return lo;
    } else if (h >= 0.0) {
      b = xn;
    } else {
      a = xn;
    }
  }
  return b;
}

// ---------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------
// k_forecast_points's tiling: a tile is `rpw` rows and its (row, point) pairs -- one contiguous
// piece of the [N, T] output -- are dealt to lanes in output order.  One pair per lane: the
// tile's pairs are cut into `cpt` chunks of 256 and every chunk is a workgroup of its own
// (block = tile * cpt + chunk), which stages the RowPs of the rows its pairs touch and the
// weights in LDS.  (With a loop over pairs in the lane, the constants of normcdfinv, erfc, pow
// and exp were all kept in registers across it: 512 registers and scratch.)
// x_stride: 0 = one point vector for all rows, else row i reads x[i * x_stride + t].
template <int KIND, bool QUANTILE>
__global__ __launch_bounds__(kThreads) void k_pool_points(
    const float* __restrict__ preds, int M, int64_t n, int rpw, uint32_t cpt, double u_fixed,
    double xi, double c, const double* __restrict__ wts, const double* __restrict__ x,
    uint32_t T, int64_t x_stride, int upper, double* __restrict__ out) {
  __shared__ RowP s_row[kPoolSlots];
  __shared__ double s_w[kPoolMaxM + 1];
  constexpr int K = Kind<KIND>::K;
  const uint32_t tile = blockIdx.x / cpt, chunk = blockIdx.x - tile * cpt;
  const int64_t first = tile * (int64_t)rpw;
  const int rows = (int)min<int64_t>(rpw, n - first);
  const uint64_t total = (uint64_t)rows * T;  // <= 64 * 2^24
  const uint64_t begin = (uint64_t)chunk * kThreads;
  if (begin >= total) return;  // the whole workgroup (a partial last tile)
  const uint64_t last = min<uint64_t>(begin + kThreads, total) - 1;
  const int row0 = (int)(begin / T), nrows = (int)(last / T) - row0 + 1;  // <= rows <= rpw
  for (int idx = threadIdx.x; idx < nrows * M; idx += kThreads) {  // nrows * M <= kPoolSlots
    const int row = idx / M, m = idx - row * M;
    s_row[idx] = load_row<KIND>(preds + (int64_t)m * n * K, first + row0 + row, u_fixed, c);
  }
  stage_weights(wts, M, s_w);
  __syncthreads();
  const uint64_t idx = begin + threadIdx.x;
  if (idx >= total) return;
  const uint32_t row = (uint32_t)(idx / T), t = (uint32_t)(idx - (uint64_t)row * T);
  const double xt = x[(first + row) * x_stride + t];
  const RowP* r = &s_row[(row - row0) * M];
  double v;
  if constexpr (QUANTILE)
    v = pool_quantile<KIND>(r, s_w, M, xt, upper != 0, c, xi);
  else
    v = upper ? pool_prob<KIND, true>(r, s_w, M, xt, c, xi)
              : pool_prob<KIND, false>(r, s_w, M, xt, c, xi);
  out[first * (int64_t)T + (int64_t)idx] = v;
}

// Scores: one workgroup per row.  The M RowPs go to LDS; the row's breakpoints (mu_m + k
// sigma_m, every u_m, c; clipped to [lo, U]) are ranked by counting; the (panel, node) pairs
// of the diversity integral are dealt to the 256 lanes, each lane looping over the members at
// its node; one butterfly per wave and four adds give V.  Thread 0 then writes the row, the
// first T + 1 threads its Brier / count terms.  The workgroup that draws the last ticket sums
// those terms in the order of k_forecast_score (64-row tiles by butterfly, thread j tiles j,
// j + 256, ..., one tree): the bits of gine_forecast_score for a pool of one member.
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_pool_score(
    const float* __restrict__ preds, const float* __restrict__ y, int M, int64_t n,
    double u_fixed, double xi, double c, const double* __restrict__ wts,
    const double* __restrict__ x, int T, const double* __restrict__ gj_x,
    const double* __restrict__ gj_w, double* __restrict__ crps_rows,
    double* __restrict__ member_rows, double* __restrict__ div_rows,
    double* __restrict__ pit_lo, double* __restrict__ pit_hi, double* __restrict__ brier,
    double* __restrict__ valid, double* __restrict__ partials,
    unsigned int* __restrict__ ticket) {
  __shared__ RowP s_row[kPoolMaxM];
  __shared__ double s_w[kPoolMaxM + 1];
  __shared__ double s_raw[kPoolMaxBp];
  __shared__ double s_bp[kPoolMaxBp];
  __shared__ double s_red[kThreads];
  __shared__ int s_last;
  constexpr int K = Kind<KIND>::K;
  constexpr bool atom = Kind<KIND>::atom, tail = Kind<KIND>::tail;
  const double nan = __builtin_nan(""), inf = __builtin_huge_val();
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row = blockIdx.x;
  if (tid < M) s_row[tid] = load_row<KIND>(preds + (int64_t)tid * n * K, row, u_fixed, c);
  stage_weights(wts, M, s_w);
  __syncthreads();
  // the integration range [lo, U] and the tail map's scale S
  double U = -inf, S = 0.0, lo = inf, hi = -inf;
  for (int m = 0; m < M; ++m) {
    U = fmax(U, s_row[m].u);
    S = fmax(S, s_row[m].su);
    lo = fmin(lo, s_row[m].mu + kBpK[0] * s_row[m].sigma);
    hi = fmax(hi, s_row[m].mu + kBpK[kPoolK - 1] * s_row[m].sigma);
  }
  if constexpr (atom) lo = c;
  if constexpr (tail) hi = U;
  else if constexpr (atom) hi = fmax(hi, c);
  const int nb = kPoolK * M + (tail ? M : 0) + (atom ? 1 : 0);  // <= 12 M + 1
  for (int j = tid; j < nb; j += kThreads) {
    double b;
    if (j < kPoolK * M) {
      const int m = j / kPoolK, k = j - m * kPoolK;
      b = s_row[m].mu + kBpK[k] * s_row[m].sigma;
    } else if (tail && j < (kPoolK + 1) * M) {
      b = s_row[j - kPoolK * M].u;
    } else {
      b = c;
    }
    s_raw[j] = fmin(fmax(b, lo), hi);
  }
  __syncthreads();
  for (int j = tid; j < nb; j += kThreads) {  // rank by counting; ties by index
    const double b = s_raw[j];
    int rank = 0;
    for (int i = 0; i < nb; ++i) {
      const double o = s_raw[i];
      rank += (o < b || (o == b && i < j)) ? 1 : 0;
    }
    s_bp[rank] = b;
  }
  __syncthreads();
  const int body = kGL * (nb - 1);
  const int pairs = body + (tail ? kGJ : 0);
  double acc = 0.0;
  for (int idx = tid; idx < pairs; idx += kThreads) {
    if (idx < body) {
      const int p = idx / kGL, i = idx - p * kGL;
      const double a = s_bp[p], b = s_bp[p + 1];
      const double half = 0.5 * (b - a);
      if (half == 0.0) continue;  // an empty panel: exactly 0
      const double node = i < 8 ? -kGLx[7 - i] : kGLx[i - 8];
      const double wq = half * (i < 8 ? kGLw[7 - i] : kGLw[i - 8]);
      const double xq = 0.5 * (a + b) + half * node;
      acc += wq * pool_var<KIND, false>(s_row, s_w, M, xq, c, xi);
    } else if constexpr (tail) {
      // x = U + (S / xi) (1 - w) / w: the integrand is w^(2 / xi - 2), the rule's weight,
      // times g(w) = f(x) (S / xi) w^(-2 / xi)
      const double wn = gj_x[idx - body];
      const double xq = U + (S / xi) * ((1.0 - wn) / wn);
      const double g = pool_var<KIND, true>(s_row, s_w, M, xq, c, xi) * (S / xi) *
                       pow(wn, -2.0 / xi);
      acc += gj_w[idx - body] * g;
    }
  }
  for (int off = kWave / 2; off > 0; off >>= 1) acc += shfl_xor_d(acc, off);
  __syncthreads();  // (s_red is free)
  if (lane == 0) s_red[wave] = acc;
  __syncthreads();
  const double V = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
  __syncthreads();
  // the row: lane m forms member m's terms, thread 0 adds them in index order
  const float yf = y[row];
  const bool ok = yf == yf;  // NaN targets score nothing
  const double yy = (double)yf;
  const double ye = ok ? (atom ? fmax(yy, c) : yy) : nan;
  if (tid < M && ok) {
    s_red[tid] = s_w[tid] * crps_row<KIND>(s_row[tid], yy, c, xi);
    s_red[kPoolMaxM + tid] = s_w[tid] * cdf_at<KIND>(s_row[tid], ye, c, xi);
  }
  __syncthreads();
  if (tid == 0) {
    double cr = nan, mc = nan, plo = nan, phi_ = nan;
    if (ok) {
      mc = s_red[0];
      phi_ = s_red[kPoolMaxM];
      for (int m = 1; m < M; ++m) {
        mc += s_red[m];
        phi_ += s_red[kPoolMaxM + m];
      }
      mc *= s_w[kPoolMaxM];
      phi_ *= s_w[kPoolMaxM];
      cr = mc - V;
      plo = (atom && ye == c) ? 0.0 : phi_;  // [Fbar(y-), Fbar(y)]
    }
    if (crps_rows) crps_rows[row] = cr;
    if (member_rows) member_rows[row] = mc;
    if (div_rows) div_rows[row] = V;
    if (pit_lo) pit_lo[row] = plo;
    if (pit_hi) pit_hi[row] = phi_;
  }
  double* part = partials + (size_t)row * (size_t)(T + 1);
  for (int t = tid; t <= T; t += kThreads) {
    double v = 0.0;
    if (ok) {
      v = 1.0;
      if (t < T) {
        const double xt = x[t];
        const double d =
            pool_prob<KIND, true>(s_row, s_w, M, xt, c, xi) - (ye > xt ? 1.0 : 0.0);
        v = d * d;
      }
    }
    __hip_atomic_exchange(&part[t], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // every wave's terms are out
  if (tid == 0) {
    const unsigned int prev =
        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  const int64_t tiles = ceil_div(n, kRows);
  double count = 0.0;
  for (int k = 0; k <= T; ++k) {
    const int t = k == 0 ? T : k - 1;  // the count first
    double a = 0.0;
    for (int64_t base = 0; base < tiles; base += kThreads) {
      for (int i = 0; i < kWave; ++i) {  // tile base + 64 wave + i is thread (64 wave + i)'s
        const int64_t tile = base + wave * kWave + i;
        if (tile >= tiles) break;  // the whole wave
        const int64_t r = tile * kRows + lane;
        double v = 0.0;
        if (r < n)
          v = __hip_atomic_load(&partials[(size_t)r * (size_t)(T + 1) + t], __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
        for (int off = kWave / 2; off > 0; off >>= 1) v += shfl_xor_d(v, off);
        if (lane == i) a += v;
      }
    }
    s_red[tid] = a;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if (tid < s) s_red[tid] += s_red[tid + s];
      __syncthreads();
    }
    if (tid == 0) {
      if (k == 0) {
        count = s_red[0];
        if (valid) valid[0] = count;
      } else {
        brier[t] = s_red[0] / count;  // NaN when no target is valid
      }
    }
    __syncthreads();  // s_red[0] has been read
  }
  if (tid == 0) *ticket = 0u;  // re-armed for the next call (stream order)
}

// Pair sums for fitting the pool's weights.  Over the rows of a segment that have
// a target: their number, every member's closed-form CRPS, and for every pair m < l the Cramer
// distance int (F_m - F_l)^2 dx by the row's own rule above -- the breakpoints of ALL M members,
// so that V(w) = 1/2 w' D w holds node by node.
//
// A workgroup owns one tile: up to 64 consecutive rows of one segment, taken in order.  Tile k
// of segment g is block ptr[g] / 64 + g + k: that start grows with g, so a block finds its
// segment by bisection, and floor(N / 64) + G blocks cover every tile (some own none).  Per row
// the panels that are not empty are listed in order, and their nodes (the tail panel's last) go
// through LDS in chunks of 128: every lane evaluates members at nodes into s_f[node][member]
// (odd row stride), then the lane of pair (m, l) and node slice s adds wq (F_m - F_l)^2 for the
// chunk's nodes s, s + S, ... in order; S = 256 / pairs slices when there are fewer than 256
// pairs, else one slice and up to two pairs a lane.  At the row's end its slices are added in
// order: the row's own value, which joins the tile's sum; the tile's record [count, crps_m,
// pairs] is written after its last row.  The workgroup that draws the last ticket adds the records of each segment: R = 1 + M
// + pairs entries, the tiles cut into 256 / R contiguous runs (one above 256 entries), each run
// summed in tile order and the runs in order.  All of it a function of M and the segment's rows.
constexpr int kPairChunk = 128;
constexpr int kPairMax = kPoolMaxM * (kPoolMaxM - 1) / 2;  // 496
constexpr int kPairRec = 1 + kPoolMaxM + kPairMax;          // 529

__device__ __forceinline__ void pair_unpack(int p, int M, int& m, int& l) {
  m = 0;
  for (int i = 0; i < kPoolMaxM; ++i) {  // (0,1), (0,2), ..., (M-2, M-1)
    if (p < M - 1 - m) break;
    p -= M - 1 - m;
    ++m;
  }
  l = m + 1 + p;
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void k_pool_pairs(
    const float* __restrict__ preds, const float* __restrict__ y, int M, int64_t n,
    double u_fixed, double xi, double c, const double* __restrict__ gj_x,
    const double* __restrict__ gj_w, const int64_t* __restrict__ ptr, int64_t G,
    double* __restrict__ count, double* __restrict__ cbar, double* __restrict__ dist,
    double* __restrict__ partials, unsigned int* __restrict__ ticket) {
  __shared__ RowP s_row[kPoolMaxM];
  __shared__ double s_raw[kPoolMaxBp];
  __shared__ double s_bp[kPoolMaxBp];
  __shared__ int s_pan[kPoolMaxBp];
  __shared__ double s_f[kPairChunk * (kPoolMaxM + 1)];
  __shared__ double s_x[kPairChunk];
  __shared__ double s_wq[kPairChunk];
  __shared__ double s_acc[kPairRec];
  __shared__ int s_npan;
  __shared__ int s_last;
  constexpr int K = Kind<KIND>::K;
  constexpr bool atom = Kind<KIND>::atom, tail = Kind<KIND>::tail;
  const double inf = __builtin_huge_val();
  const int tid = threadIdx.x;
  const int P = M * (M - 1) / 2, R = 1 + M + P;
  const int stride = M | 1;
  // this block's tile
  const int64_t blk = blockIdx.x;
  int64_t g = 0, top = G - 1;
  for (int it = 0; it < 64; ++it) {  // the last g with ptr[g] / 64 + g <= blk
    if (g >= top) break;
    const int64_t mid = g + (top - g + 1) / 2;
    if (ptr[mid] / kRows + mid <= blk) g = mid;
    else top = mid - 1;
  }
  const int64_t seg_a = min<int64_t>(max<int64_t>(ptr[g], 0), n);
  const int64_t seg_e = min<int64_t>(max<int64_t>(ptr[g + 1], seg_a), n);
  const int64_t tile = blk - (ptr[g] / kRows + g);
  const bool owns = tile >= 0 && tile < ceil_div(seg_e - seg_a, (int64_t)kRows);
  const int64_t first = seg_a + (owns ? tile : 0) * kRows;
  const int rows = owns ? (int)min<int64_t>(kRows, seg_e - first) : 0;
  // this lane's pairs and node slice
  const int S = P >= kThreads ? 1 : (P > 0 ? kThreads / P : 0);
  const bool on0 = tid < P * S;
  const int sl = on0 ? tid / P : 0;
  const bool on1 = tid + kThreads < P;
  int m0 = 0, l0 = 0, m1 = 0, l1 = 0;
  if (on0) pair_unpack(tid - sl * P, M, m0, l0);
  if (on1) pair_unpack(tid + kThreads, M, m1, l1);
  double sum0 = 0.0, sum1 = 0.0, cacc = 0.0, cnt = 0.0;
  for (int rr = 0; rr < rows; ++rr) {
    double acc0 = 0.0, acc1 = 0.0;
    const int64_t row = first + rr;
    const float yf = y[row];
    if (!(yf == yf)) continue;  // no target: the row adds nothing (the whole workgroup)
    __syncthreads();            // the row before is done with LDS
    if (tid < M) s_row[tid] = load_row<KIND>(preds + (int64_t)tid * n * K, row, u_fixed, c);
    __syncthreads();
    if (tid < M) cacc += crps_row<KIND>(s_row[tid], (double)yf, c, xi);
    cnt += 1.0;
    if (P == 0) continue;
    // breakpoints, clipped and ranked as k_pool_score builds them
    double U = -inf, Sg = 0.0, lo = inf, hi = -inf;
    for (int m = 0; m < M; ++m) {
      U = fmax(U, s_row[m].u);
      Sg = fmax(Sg, s_row[m].su);
      lo = fmin(lo, s_row[m].mu + kBpK[0] * s_row[m].sigma);
      hi = fmax(hi, s_row[m].mu + kBpK[kPoolK - 1] * s_row[m].sigma);
    }
    if constexpr (atom) lo = c;
    if constexpr (tail) hi = U;
    else if constexpr (atom) hi = fmax(hi, c);
    const int nb = kPoolK * M + (tail ? M : 0) + (atom ? 1 : 0);
    for (int j = tid; j < nb; j += kThreads) {
      double b;
      if (j < kPoolK * M) {
        const int m = j / kPoolK, k = j - m * kPoolK;
        b = s_row[m].mu + kBpK[k] * s_row[m].sigma;
      } else if (tail && j < (kPoolK + 1) * M) {
        b = s_row[j - kPoolK * M].u;
      } else {
        b = c;
      }
      s_raw[j] = fmin(fmax(b, lo), hi);
    }
    __syncthreads();
    for (int j = tid; j < nb; j += kThreads) {
      const double b = s_raw[j];
      int rank = 0;
      for (int i = 0; i < nb; ++i) {
        const double o = s_raw[i];
        rank += (o < b || (o == b && i < j)) ? 1 : 0;
      }
      s_bp[rank] = b;
    }
    __syncthreads();
    // the panels that are not empty, in order
    for (int j = tid; j < nb - 1; j += kThreads) {
      int before = 0;
      for (int i = 0; i < j; ++i) before += 0.5 * (s_bp[i + 1] - s_bp[i]) != 0.0 ? 1 : 0;
      const bool full = 0.5 * (s_bp[j + 1] - s_bp[j]) != 0.0;
      if (full) s_pan[before] = j;
      if (j == nb - 2) s_npan = before + (full ? 1 : 0);
    }
    __syncthreads();
    const int body = kGL * s_npan;
    const int total = body + (tail ? kGJ : 0);
    for (int cb = 0; cb < total; cb += kPairChunk) {
      const int cn = min(kPairChunk, total - cb);
      if (tid < cn) {
        const int idx = cb + tid;
        if (idx < body) {
          const int p = s_pan[idx / kGL], i = idx % kGL;
          const double a = s_bp[p], b = s_bp[p + 1];
          const double half = 0.5 * (b - a);
          const double node = i < 8 ? -kGLx[7 - i] : kGLx[i - 8];
          s_wq[tid] = half * (i < 8 ? kGLw[7 - i] : kGLw[i - 8]);
          s_x[tid] = 0.5 * (a + b) + half * node;
        } else {
          // x = U + (S / xi) (1 - w) / w; the rule's weight times dx/dw over its own w^(2/xi - 2)
          const double wn = gj_x[idx - body];
          s_x[tid] = U + (Sg / xi) * ((1.0 - wn) / wn);
          s_wq[tid] = gj_w[idx - body] * ((Sg / xi) * pow(wn, -2.0 / xi));
        }
      }
      __syncthreads();
      for (int idx = tid; idx < cn * M; idx += kThreads) {  // lanes side by side: one member
        const int m = idx / cn, nd = idx - m * cn;
        const double xq = s_x[nd];
        s_f[nd * stride + m] = cb + nd < body ? cdf_at<KIND>(s_row[m], xq, c, xi)
                                              : sf_at<KIND>(s_row[m], xq, c, xi);
      }
      __syncthreads();
      if (on0) {
        for (int nd = sl; nd < cn; nd += S) {
          const double d = s_f[nd * stride + m0] - s_f[nd * stride + l0];
          acc0 += s_wq[nd] * d * d;
        }
      }
      if (on1) {
        for (int nd = 0; nd < cn; ++nd) {
          const double d = s_f[nd * stride + m1] - s_f[nd * stride + l1];
          acc1 += s_wq[nd] * d * d;
        }
      }
      __syncthreads();
    }
    // the row's value of a pair: its node slices in order; then the rows in order
    if (S > 1) {
      if (on0) s_f[tid] = acc0;  // [slice][pair]
      __syncthreads();
      if (tid < P) {
        acc0 = s_f[tid];
        for (int s = 1; s < S; ++s) acc0 += s_f[s * P + tid];
      }
    }
    sum0 += acc0;
    sum1 += acc1;
  }
  if (owns) {
    double* rec = partials + (size_t)blk * (size_t)R;
    if (tid == 0) __hip_atomic_exchange(&rec[0], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < M)
      __hip_atomic_exchange(&rec[1 + tid], cacc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < P)
      __hip_atomic_exchange(&rec[1 + M + tid], sum0, __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT);
    if (on1)
      __hip_atomic_exchange(&rec[1 + M + kThreads + tid], sum1, __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // every wave's entries are out
  if (tid == 0) {
    const unsigned int prev =
        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  const int runs = R >= kThreads ? 1 : kThreads / R;
  for (int64_t sg = 0; sg < G; ++sg) {
    const int64_t a = min<int64_t>(max<int64_t>(ptr[sg], 0), n);
    const int64_t e = min<int64_t>(max<int64_t>(ptr[sg + 1], a), n);
    const int64_t t0 = ptr[sg] / kRows + sg;
    const int64_t tiles = ceil_div(e - a, (int64_t)kRows);
    const int64_t per = ceil_div(tiles, (int64_t)runs);
    for (int it = tid; it < R * runs; it += kThreads) {
      const int run = it / R, ent = it - run * R;
      const int64_t kend = min<int64_t>(tiles, (run + 1) * per);
      double v = 0.0;
      for (int64_t k = run * per; k < kend; ++k) {
        const int64_t rec = t0 + k;
        if (rec >= 0 && rec < (int64_t)gridDim.x)
          v += __hip_atomic_load(&partials[(size_t)rec * (size_t)R + ent], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
      }
      s_acc[it] = v;
    }
    __syncthreads();
    for (int ent = tid; ent < R; ent += kThreads) {
      double v = s_acc[ent];
      for (int run = 1; run < runs; ++run) v += s_acc[run * R + ent];
      if (ent == 0) count[sg] = v;
      else if (ent <= M) cbar[sg * M + (ent - 1)] = v;
      else dist[sg * P + (ent - 1 - M)] = v;
    }
    __syncthreads();  // s_acc has been read
  }
  if (tid == 0) *ticket = 0u;  // re-armed for the next call (stream order)
}

// members, kind, sizes and the distribution's domain, before any HIP call
int check_pool(int32_t num_members, int64_t num_nodes, int32_t kind, double u, double xi,
               double c, int64_t points) {
  if (num_members < 1 || num_members > kPoolMaxM) return GINE_ERR_INVALID;
  if (kind < GINE_LOSS_NORMAL || kind > GINE_LOSS_MIXED_U) return GINE_ERR_INVALID;
  if (num_nodes < 0 || points < 0) return GINE_ERR_INVALID;
  if (!(c == c)) return GINE_ERR_INVALID;
  if (kind == GINE_LOSS_MIXED || kind == GINE_LOSS_MIXED_U) {
    if (!(xi > 0.0 && xi < 1.0)) return GINE_ERR_INVALID;
    if (kind == GINE_LOSS_MIXED && !(u > c)) return GINE_ERR_INVALID;
    if (kind == GINE_LOSS_MIXED_U && !(c < 0.0)) return GINE_ERR_INVALID;
  }
  if (points > kMaxPoints || num_nodes > 0x7fffffff) return GINE_ERR_TOO_LARGE;
  return GINE_OK;
}

template <bool QUANTILE>
int launch_pool_points(const float* preds, int32_t M, int64_t num_nodes, int32_t kind, double u,
                       double xi, double c, const double* weights, const double* x, int32_t T,
                       int64_t x_stride, int32_t flags, double* out, void* stream) {
  const int rc = check_pool(M, num_nodes, kind, u, xi, c, T);
  if (rc != GINE_OK) return rc;
  if (flags & ~GINE_FORECAST_UPPER) return GINE_ERR_INVALID;
  if (x_stride != 0 && x_stride < T) return GINE_ERR_INVALID;
  if (num_nodes == 0 || T == 0) return GINE_OK;
  if (!preds || !weights || !x || !out) return GINE_ERR_INVALID;
  const int rpw = kPoolSlots / M < kRows ? kPoolSlots / M : kRows;
  const int64_t cpt = ceil_div((int64_t)rpw * T, kThreads);  // chunks of 256 pairs per tile
  const int64_t blocks = ceil_div(num_nodes, rpw) * cpt;
  if (blocks > 0x7fffffff) return GINE_ERR_TOO_LARGE;
  const dim3 grid((unsigned)blocks);
  const int upper = (flags & GINE_FORECAST_UPPER) != 0;
#define LAUNCH_POOL_POINTS(KIND_)                                                              \
  hipLaunchKernelGGL((k_pool_points<KIND_, QUANTILE>), grid, dim3(kThreads), 0,                \
                     as_stream(stream), preds, (int)M, num_nodes, rpw, (uint32_t)cpt, u, xi, c,   \
                     weights, x, (uint32_t)T, x_stride, upper, out)
  switch (kind) {
    case GINE_LOSS_NORMAL: LAUNCH_POOL_POINTS(GINE_LOSS_NORMAL); break;
    case GINE_LOSS_MIXED_NORMAL: LAUNCH_POOL_POINTS(GINE_LOSS_MIXED_NORMAL); break;
    case GINE_LOSS_MIXED: LAUNCH_POOL_POINTS(GINE_LOSS_MIXED); break;
    default: LAUNCH_POOL_POINTS(GINE_LOSS_MIXED_U); break;
  }
#undef LAUNCH_POOL_POINTS
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

}  // namespace
}  // namespace gine

using namespace gine;

extern "C" int gine_pool_prob(const float* preds, int32_t num_members, int64_t num_nodes,
                              int32_t kind, double u, double xi, double c,
                              const double* weights, const double* x, int32_t num_x,
                              int32_t flags, double* out, void* stream) {
  return launch_pool_points<false>(preds, num_members, num_nodes, kind, u, xi, c, weights, x,
                                   num_x, 0, flags, out, stream);
}

extern "C" int gine_pool_quantile(const float* preds, int32_t num_members, int64_t num_nodes,
                                  int32_t kind, double u, double xi, double c,
                                  const double* weights, const double* level,
                                  int32_t num_levels, int64_t level_row_stride, int32_t flags,
                                  double* out, void* stream) {
  return launch_pool_points<true>(preds, num_members, num_nodes, kind, u, xi, c, weights, level,
                                  num_levels, level_row_stride, flags, out, stream);
}

extern "C" int gine_pool_score_partials(int64_t num_nodes, int32_t num_x, size_t* count) {
  if (!count || num_nodes < 0 || num_x < 0) return GINE_ERR_INVALID;
  if (num_x > kMaxPoints || num_nodes > 0x7fffffff) return GINE_ERR_TOO_LARGE;
  *count = (size_t)(num_nodes > 0 ? num_nodes : 1) * (size_t)(num_x + 1);
  return GINE_OK;
}

extern "C" int gine_pool_score(const float* preds, const float* y, int32_t num_members,
                               int64_t num_nodes, int32_t kind, double u, double xi, double c,
                               const double* weights, const double* x, int32_t num_x,
                               const double* jacobi_nodes, const double* jacobi_weights,
                               double* crps_rows, double* member_crps_rows,
                               double* diversity_rows, double* pit_lo, double* pit_hi,
                               double* brier, double* valid, double* partials,
                               uint32_t* ticket, void* stream) {
  const int rc = check_pool(num_members, num_nodes, kind, u, xi, c, num_x);
  if (rc != GINE_OK) return rc;
  if (num_nodes == 0) return GINE_OK;
  if (!preds || !y || !weights || !partials || !ticket) return GINE_ERR_INVALID;
  if (num_x > 0 && (!x || !brier)) return GINE_ERR_INVALID;
  const bool tail = kind == GINE_LOSS_MIXED || kind == GINE_LOSS_MIXED_U;
  if (tail && (!jacobi_nodes || !jacobi_weights)) return GINE_ERR_INVALID;
  const dim3 grid((unsigned)num_nodes);
#define LAUNCH_POOL_SCORE(KIND_)                                                               \
  hipLaunchKernelGGL((k_pool_score<KIND_>), grid, dim3(kThreads), 0, as_stream(stream), preds, \
                     y, (int)num_members, num_nodes, u, xi, c, weights, x, (int)num_x,         \
                     jacobi_nodes, jacobi_weights, crps_rows, member_crps_rows,                \
                     diversity_rows, pit_lo, pit_hi, brier, valid, partials, ticket)
  switch (kind) {
    case GINE_LOSS_NORMAL: LAUNCH_POOL_SCORE(GINE_LOSS_NORMAL); break;
    case GINE_LOSS_MIXED_NORMAL: LAUNCH_POOL_SCORE(GINE_LOSS_MIXED_NORMAL); break;
    case GINE_LOSS_MIXED: LAUNCH_POOL_SCORE(GINE_LOSS_MIXED); break;
    default: LAUNCH_POOL_SCORE(GINE_LOSS_MIXED_U); break;
  }
#undef LAUNCH_POOL_SCORE
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

// one record per tile: floor(N / 64) + G tiles at the most
static int pool_pairs_tiles(int64_t num_nodes, int64_t num_segments, int64_t* tiles) {
  if (num_segments < 1) return GINE_ERR_INVALID;
  if (num_segments > 0x7fffffff - num_nodes / kRows) return GINE_ERR_TOO_LARGE;
  *tiles = num_nodes / kRows + num_segments;
  return GINE_OK;
}

extern "C" int gine_pool_pairs_partials(int64_t num_nodes, int32_t num_members,
                                        int64_t num_segments, size_t* count) {
  if (!count || num_nodes < 0 || num_members < 1 || num_members > kPoolMaxM)
    return GINE_ERR_INVALID;
  if (num_nodes > 0x7fffffff) return GINE_ERR_TOO_LARGE;
  int64_t tiles = 0;
  const int rc = pool_pairs_tiles(num_nodes, num_segments, &tiles);
  if (rc != GINE_OK) return rc;
  *count = (size_t)tiles * (size_t)(1 + num_members + num_members * (num_members - 1) / 2);
  return GINE_OK;
}

extern "C" int gine_pool_pairs(const float* preds, const float* y, int32_t num_members,
                               int64_t num_nodes, int32_t kind, double u, double xi, double c,
                               const double* jacobi_nodes, const double* jacobi_weights,
                               const int64_t* ptr, int64_t num_segments, double* count,
                               double* member_crps, double* distance, double* partials,
                               uint32_t* ticket, void* stream) {
  int rc = check_pool(num_members, num_nodes, kind, u, xi, c, 0);
  if (rc != GINE_OK) return rc;
  int64_t tiles = 0;
  rc = pool_pairs_tiles(num_nodes, num_segments, &tiles);
  if (rc != GINE_OK) return rc;
  if (num_nodes == 0) return GINE_OK;
  if (!preds || !y || !ptr || !count || !member_crps || !partials || !ticket)
    return GINE_ERR_INVALID;
  if (num_members > 1 && !distance) return GINE_ERR_INVALID;
  const bool tail = kind == GINE_LOSS_MIXED || kind == GINE_LOSS_MIXED_U;
  if (tail && (!jacobi_nodes || !jacobi_weights)) return GINE_ERR_INVALID;
  const dim3 grid((unsigned)tiles);
#define LAUNCH_POOL_PAIRS(KIND_)                                                               \
  hipLaunchKernelGGL((k_pool_pairs<KIND_>), grid, dim3(kThreads), 0, as_stream(stream), preds, \
                     y, (int)num_members, num_nodes, u, xi, c, jacobi_nodes, jacobi_weights,   \
                     ptr, num_segments, count, member_crps, distance, partials, ticket)
  switch (kind) {
    case GINE_LOSS_NORMAL: LAUNCH_POOL_PAIRS(GINE_LOSS_NORMAL); break;
    case GINE_LOSS_MIXED_NORMAL: LAUNCH_POOL_PAIRS(GINE_LOSS_MIXED_NORMAL); break;
    case GINE_LOSS_MIXED: LAUNCH_POOL_PAIRS(GINE_LOSS_MIXED); break;
    default: LAUNCH_POOL_PAIRS(GINE_LOSS_MIXED_U); break;
  }
#undef LAUNCH_POOL_PAIRS
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}
