// The predictive distribution that the CRPS losses score (models/loss.py), evaluated on
// gfx950: distribution function and exceedance probability at thresholds, quantiles and
// return levels, and the verification scores of a set of targets (per-row CRPS, PIT
// interval, Brier score per threshold).  pred [N, K] fp32 as gine_crps_fwd reads it; every
// result and all arithmetic fp64.
//
//   c = censoring point, z(x) = (x - mu) / sigma, Phi = standard normal cdf
//   NORMAL        F(x) = Phi(z)
//   MIXED_NORMAL  F(x) = 0 (x < c),  p + (1 - p) Phi(z) (x >= c): an atom P_c = F(c) at c
//   MIXED(_U)     as MIXED_NORMAL below u;  x >= u: m_u + (1 - m_u) G((x - u) / sigma_u),
//                 m_u = p + (1 - p) Phi(z(u)),  G(t) = 1 - (1 + xi t)^(-1/xi)
// Upper probabilities are formed from erfc and the tail power themselves, never as 1 - F.
//
// The closed-form CRPS values are restated here in plain double: nothing is shared with
// gine_loss.hip (its kernels' instruction streams stay what they are), and the expressions
// follow that file's, so the two agree to rounding.
#include "gine_common.hpp"

namespace gine {
namespace {

constexpr double kInvSqrtPi = 0.56418958354775628695;   // 1/sqrt(pi)
constexpr double kLogSqrt2Pi = 0.91893853320467274178;  // log(sqrt(2 pi))
constexpr double kSqrt2 = 1.41421356237309504880;
constexpr int kThreads = 256;
constexpr int kRows = 64;            // rows per workgroup: one wave evaluates their invariants
constexpr int kMaxPoints = 1 << 24;  // thresholds / levels per call: a tile's pairs fit 32 bits

template <int KIND>
struct Kind {
  static constexpr int K = KIND == GINE_LOSS_NORMAL ? 2
                           : KIND == GINE_LOSS_MIXED_NORMAL ? 3
                           : KIND == GINE_LOSS_MIXED ? 4 : 5;
  static constexpr bool atom = KIND != GINE_LOSS_NORMAL;  // point mass at c
  static constexpr bool tail = KIND == GINE_LOSS_MIXED || KIND == GINE_LOSS_MIXED_U;
};

// upper / lower standard normal probability, each accurate in its own tail
__device__ __forceinline__ double upper_phi(double z) { return 0.5 * erfc(z / kSqrt2); }
__device__ __forceinline__ double lower_phi(double z) { return 0.5 * erfc(-z / kSqrt2); }

// One row's parameters and what every threshold of that row needs.
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

// (1 + xi t)^(-1/xi), t = (x - u) / sigma_u >= 0: the tail's conditional exceedance
__device__ __forceinline__ double gpd_upper(const RowP& r, double x, double xi) {
  const double t = (x - r.u) / r.su;
  return pow(1.0 + xi * t, -1.0 / xi);
}

// F(x) = P(Y <= x)
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

// P(Y > x), without 1 - F
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

// z with upper_phi(z) = v, 0 < v < 1.  The device normcdfinv as it is: measured on MI355X in
// probability space, |F(Q(q)) - q| <= 2.4e-15 and |sf(Q(s)) - s| <= 3.1e-14 s down to
// s = 1e-12 (a Newton step on erfc after it gave 2.8e-14: nothing to gain).
__device__ __forceinline__ double upper_phi_inv(double v) { return -normcdfinv(v); }

// inf{x : F(x) >= q}.  upper: `level` is the exceedance probability s = 1 - q, used as it is.
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
  // the body, through whichever tail of the normal is the smaller
  const double v = s / r.q;                                // above the quantile
  const double w = upper ? 1.0 - v : (level - r.p) / r.q;  // below it
  const bool high = upper ? v <= 0.5 : w > 0.5;
  const double z = upper_phi_inv(high ? v : w);
  double x = high ? r.mu + r.sigma * z : r.mu - r.sigma * z;
  if constexpr (Kind<KIND>::atom) x = fmax(x, c);
  if constexpr (Kind<KIND>::tail) x = fmin(x, r.u);
  return x;
}

// ---------------------------------------------------------------------------------------
// closed-form CRPS values (restated from models/loss.py; expressions as in gine_loss.hip)
// ---------------------------------------------------------------------------------------
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

// where(y < u, loss_1, loss_2): the CRPS of the distribution, for a fixed and for a per-row u
// (not the sigmoid blend that training with a learned u uses as its smooth surrogate)
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
// kernels.  A workgroup owns kRows rows: wave 0 evaluates their invariants into LDS once,
// then the tile's (row, point) pairs -- one contiguous piece of the [N, T] output -- are
// dealt to the 256 lanes in output order, so every store instruction is coalesced.  A lane
// carries rows * T / 256 evaluations of one erfc or one pow each (2 at T = 8).
// ---------------------------------------------------------------------------------------
template <int KIND, bool QUANTILE>
__global__ __launch_bounds__(kThreads) void k_forecast_points(
    const float* __restrict__ pred, int64_t n, double u_fixed, double xi, double c,
    const double* __restrict__ x, uint32_t T, int upper, double* __restrict__ out) {
  __shared__ RowP s_row[kRows];
  const int64_t first = blockIdx.x * (int64_t)kRows;
  const int rows = (int)min<int64_t>(kRows, n - first);
  if ((int)threadIdx.x < rows)
    s_row[threadIdx.x] = load_row<KIND>(pred, first + threadIdx.x, u_fixed, c);
  __syncthreads();
  const uint32_t total = (uint32_t)rows * T;  // <= 64 * 2^24
  double* __restrict__ o = out + first * (int64_t)T;
  for (uint32_t idx = threadIdx.x; idx < total; idx += kThreads) {
    const uint32_t row = idx / T;
    const double xt = x[idx - row * T];
    const RowP& r = s_row[row];
    double v;
    if constexpr (QUANTILE)
      v = quantile_at<KIND>(r, xt, upper != 0, c, xi);
    else
      v = upper ? sf_at<KIND>(r, xt, c, xi) : cdf_at<KIND>(r, xt, c, xi);
    o[idx] = v;
  }
}

// Verification scores.  Wave 0: per row the CRPS, the PIT interval and the row's invariants.
// Then the four waves take the thresholds in turn (wave w: w, w + 4, ...; index T is the
// count of valid rows), the 64 lanes of a wave being the tile's rows: one butterfly sum per
// threshold gives the workgroup's partial.  The workgroup that draws the last ticket sums the
// partials in a fixed order and leaves the ticket at 0 (as gine_crps_fwd does; nothing waits
// on another workgroup).  Targets at or below c are the atom for the PIT and the Brier score:
// a censored variable takes no value below c (the fp32 image of log 0.01 lies 6.4e-8 below
// the fp64 one); the CRPS takes y as it is, like the loss.
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_forecast_score(
    const float* __restrict__ pred, const float* __restrict__ y, int64_t n, double u_fixed,
    double xi, double c, const double* __restrict__ x, int T, double* __restrict__ crps_rows,
    double* __restrict__ pit_lo, double* __restrict__ pit_hi, double* __restrict__ brier,
    double* __restrict__ valid, double* __restrict__ partials,
    unsigned int* __restrict__ ticket) {
  __shared__ RowP s_row[kRows];
  __shared__ double s_y[kRows];
  __shared__ double s_red[kThreads];
  __shared__ int s_last;
  const double nan = __builtin_nan("");
  const int64_t first = blockIdx.x * (int64_t)kRows;
  const int rows = (int)min<int64_t>(kRows, n - first);
  if (threadIdx.x < kRows) {
    double ye = nan;
    if ((int)threadIdx.x < rows) {
      const int64_t i = first + threadIdx.x;
      const float yf = y[i];
      const RowP r = load_row<KIND>(pred, i, u_fixed, c);
      s_row[threadIdx.x] = r;
      double cr = nan, lo = nan, hi = nan;
      if (yf == yf) {  // NaN targets score nothing
        const double yy = (double)yf;
        cr = crps_row<KIND>(r, yy, c, xi);
        ye = Kind<KIND>::atom ? fmax(yy, c) : yy;
        hi = cdf_at<KIND>(r, ye, c, xi);
        lo = (Kind<KIND>::atom && ye == c) ? 0.0 : hi;  // [F(y-), F(y)]
      }
      if (crps_rows) crps_rows[i] = cr;
      if (pit_lo) pit_lo[i] = lo;
      if (pit_hi) pit_hi[i] = hi;
    }
    s_y[threadIdx.x] = ye;
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const double ye = s_y[lane];
  const bool ok = ye == ye;
  double* part = partials + (size_t)blockIdx.x * (size_t)(T + 1);
  for (int t = threadIdx.x / kWave; t <= T; t += kThreads / kWave) {
    double v = 0.0;
    if (ok) {
      v = 1.0;
      if (t < T) {
        const double xt = x[t];
        const double d = sf_at<KIND>(s_row[lane], xt, c, xi) - (ye > xt ? 1.0 : 0.0);
        v = d * d;
      }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) v += shfl_xor_d(v, off);
    // published as in k_crps: agent-scope exchanges, read back below with agent-scope loads
    if (lane == 0)
      __hip_atomic_exchange(&part[t], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // every wave's partials are out
  if (threadIdx.x == 0) {
    const unsigned int prev =
        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  // fixed order: thread j sums workgroups j, j + 256, ..., then one tree; the count first
  const int P = gridDim.x;
  double count = 0.0;
  for (int k = 0; k <= T; ++k) {
    const int t = k == 0 ? T : k - 1;
    double a = 0.0;
    for (int p = threadIdx.x; p < P; p += kThreads)
      a += __hip_atomic_load(&partials[(size_t)p * (size_t)(T + 1) + t], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    s_red[threadIdx.x] = a;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (k == 0) {
        count = s_red[0];
        if (valid) valid[0] = count;
      } else {
        brier[t] = s_red[0] / count;  // NaN when no target is valid
      }
    }
    __syncthreads();  // s_red[0] has been read
  }
  if (threadIdx.x == 0) *ticket = 0u;  // re-armed for the next call (stream order)
}

// ---------------------------------------------------------------------------------------
// The raw ensemble beside the distribution.  One wave per row, lane i = member i (M <= 64),
// four rows per workgroup; no LDS, no barrier, nothing shared between waves.  A member is
// x = shift + scale * raw (two roundings, -ffp-contract=off), read in place through
// (row_stride, member_stride); NaN = missing, and lanes >= M hold NaN too, so every
// comparison below leaves them out by itself.  The stable rank among the valid members,
//   r_i = 1 + #{j : x_j < x_i or (x_j == x_i and j < i)},
// comes from M wave-uniform lane broadcasts (v_readlane_b32 pairs).  Sums over members are
// butterflies over the 64 lanes: a fixed order, the same bits every run.
// ---------------------------------------------------------------------------------------
constexpr int kEnsRows = kThreads / kWave;  // rows per workgroup
constexpr int kEnsMaxMembers = kWave;

// lane j's value in every lane; j is wave-uniform
__device__ __forceinline__ double lane_value(double v, int j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = kWave / 2; off > 0; off >>= 1) v += shfl_xor_d(v, off);
  return v;
}

struct Member {
  double x;  // this lane's member (NaN: missing or lane >= M)
  int rank;  // 1..m among the valid ones (meaningless for a missing member)
  int m;     // valid members of the row
};

__device__ __forceinline__ Member load_member(const float* __restrict__ members, int64_t row,
                                              int64_t row_stride, int64_t member_stride, int M,
                                              double scale, double shift) {
  const int lane = threadIdx.x & (kWave - 1);
  Member e;
  e.x = __builtin_nan("");
  if (lane < M) e.x = shift + scale * (double)members[row * row_stride + lane * member_stride];
  e.m = __popcll(__ballot(e.x == e.x));
  int r = 1;
  for (int j = 0; j < M; ++j) {
    const double xj = lane_value(e.x, j);
    r += (xj < e.x || (xj == e.x && j < lane)) ? 1 : 0;
  }
  e.rank = r;
  return e;
}

// Scores of the raw ensemble against y.  The pair term of the CRPS from the ranks:
// sum_i sum_j |x_i - x_j| = 2 sum_i (2 r_i - m - 1) x_i (the sorted form; ties contribute 0
// whichever of them takes which rank).
__global__ __launch_bounds__(kThreads) void k_ensemble_score(
    const float* __restrict__ members, int64_t row_stride, int64_t member_stride, int M,
    double scale, double shift, const float* __restrict__ y, int64_t n,
    const double* __restrict__ x, int T, double* __restrict__ crps,
    double* __restrict__ crps_fair, double* __restrict__ rank_lo, double* __restrict__ rank_hi,
    double* __restrict__ members_valid, double* __restrict__ prob) {
  const int64_t row = blockIdx.x * (int64_t)kEnsRows + threadIdx.x / kWave;
  if (row >= n) return;  // the whole wave
  const int lane = threadIdx.x & (kWave - 1);
  const double nan = __builtin_nan("");
  const Member e = load_member(members, row, row_stride, member_stride, M, scale, shift);
  const bool ok = e.x == e.x;
  const double dm = (double)e.m;
  // exceedance probabilities: lane k keeps threshold t0 + k's, one coalesced store per 64
  for (int t0 = 0; t0 < T; t0 += kWave) {
    const int cnt = min(kWave, T - t0);
    double mine = nan;
    for (int k = 0; k < cnt; ++k) {
      const int above = __popcll(__ballot(e.x > x[t0 + k]));
      if (lane == k) mine = (double)above / dm;  // 0 / 0 = NaN without members
    }
    if (lane < cnt) prob[row * (int64_t)T + t0 + lane] = mine;
  }
  const float yf = y ? y[row] : __builtin_nanf("");
  double cr = nan, cf = nan, lo = nan, hi = nan;
  if (yf == yf && e.m > 0) {  // wave-uniform
    const double yy = (double)yf;
    const double a = wave_sum(ok ? fabs(e.x - yy) : 0.0);
    const double s = wave_sum(ok ? (double)(2 * e.rank - e.m - 1) * e.x : 0.0);
    cr = a / dm - s / (dm * dm);
    if (e.m > 1) cf = a / dm - s / (dm * (dm - 1.0));
    lo = (double)__popcll(__ballot(e.x < yy));
    hi = (double)__popcll(__ballot(e.x <= yy));
  }
  if (lane == 0) {
    if (crps) crps[row] = cr;
    if (crps_fair) crps_fair[row] = cf;
    if (rank_lo) rank_lo[row] = lo;
    if (rank_hi) rank_hi[row] = hi;
    if (members_valid) members_valid[row] = dm;
  }
}

// ECC-Q: member i becomes the predictive quantile at the level of its rank.
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_ensemble_ecc(
    const float* __restrict__ pred, int64_t n, double u_fixed, double xi, double c,
    const float* __restrict__ members, int64_t row_stride, int64_t member_stride, int M,
    double scale, double shift, int midpoint, double* __restrict__ out) {
  const int64_t row = blockIdx.x * (int64_t)kEnsRows + threadIdx.x / kWave;
  if (row >= n) return;  // the whole wave
  const int lane = threadIdx.x & (kWave - 1);
  const Member e = load_member(members, row, row_stride, member_stride, M, scale, shift);
  const RowP r = load_row<KIND>(pred, row, u_fixed, c);
  // one division of exact operands: the IEEE value the host computes
  const double level = midpoint ? ((double)e.rank - 0.5) / (double)e.m
                                : (double)e.rank / (double)(e.m + 1);
  double v = __builtin_nan("");
  if (e.x == e.x) v = quantile_at<KIND>(r, level, false, c, xi);
  if (lane < M) out[row * (int64_t)M + lane] = v;
}

// ---------------------------------------------------------------------------------------
// Threshold-weighted CRPS, weight 1{x >= t}:
//   twCRPS_t(F, y) = int_t^inf (F(x) - 1{x >= y})^2 dx = CRPS(F_t, max(y, t)),
// F_t the distribution of max(Y, t).  With t' = max(t, c) (t itself for the uncensored
// normal) and y' = max(y, t'), F_t is F censored at t': the closed forms above with c := t',
// y := y' (twcrps_censored for the kinds without a tail).  Where t' has passed u only the
// Pareto tail is left (twcrps_tail).
// ---------------------------------------------------------------------------------------
// t' >= u: a = 1 - m_u (omU: formed without cancellation), w(x) = 1 + xi (x - u) / sigma_u,
//   (y' - t') + 2 a sigma_u/(1 - xi) (w(y')^e1 - w(t')^e1) + a^2 sigma_u/(2 - xi) w(t')^e2,
// e1 = -(1 - xi)/xi, e2 = -(2 - xi)/xi; pareto_crps(y', u, m_u, sigma_u, xi) at t' = u.
__device__ __forceinline__ double twcrps_tail(const RowP& r, double yp, double tp, double xi) {
  const double wy = 1.0 + xi * ((yp - r.u) / r.su);
  const double wt = 1.0 + xi * ((tp - r.u) / r.su);  // >= 1
  const double e1 = -(1.0 - xi) / xi, e2 = -(2.0 - xi) / xi;
  const double a = r.omU;
  return (yp - tp) + ((2.0 / (1.0 - xi)) * (a * r.su * (pow(wy, e1) - pow(wt, e1))) +
                      (1.0 / (2.0 - xi)) * (a * a * r.su * pow(wt, e2)));
}

// CRPS at y' >= t' of the normal with atom p censored at t': crps_mixed_normal(mu, sigma, p,
// y', t') rewritten in upper probabilities S = q (1 - Phi),
//   (y' - t') - 2 int_t'^y' S dx + int_t'^inf S^2 dx,
//   int (1 - Phi) dz = z (1 - Phi) - phi,
//   int_a^inf (1 - Phi)^2 dz = -a (1 - Phi(a))^2 + 2 phi(a) (1 - Phi(a)) - (1 - Phi(sqrt2 a))/sqrt(pi):
// far up the tail the lower form subtracts terms of O(sigma z) from each other (1e-15 absolute
// on values of 1e-5); here no term is larger than the result.
__device__ __forceinline__ double twcrps_censored(double mu, double sigma, double p, double yp,
                                                  double tp) {
  const double yt = (yp - mu) / sigma;
  const double ct = (tp - mu) / sigma;
  const double q = 1.0 - p;
  const double Uy = upper_phi(yt), Uc = upper_phi(ct);
  const double G = (yt * Uy - phi(yt)) - (ct * Uc - phi(ct));
  double H;
  if (ct < 3.0) {
    H = -(ct * (Uc * Uc)) + 2.0 * (phi(ct) * Uc) - kInvSqrtPi * upper_phi(kSqrt2 * ct);
  } else {
    // the same three terms with phi(z)^2 factored out, R = (1 - Phi) / phi the Mills ratio:
    // they are 2 z^2 times their sum, and as products of exp() each also carries its argument
    // rounding z^2 eps / 2 -- z^4 eps, 1e-10 of a value at z = 26; this way only the 2 z^2
    const double kHalfPiSqrt = 1.25331413731550025121;  // sqrt(pi / 2)
    const double R = kHalfPiSqrt * erfcx(ct / kSqrt2), R2 = kHalfPiSqrt * erfcx(ct);
    const double f = phi(ct);
    H = (f * f) * (2.0 * R - ct * (R * R) - kSqrt2 * R2);
  }
  return (yp - tp) + sigma * (q * (q * H - 2.0 * G));
}

template <int KIND>
__device__ __forceinline__ double twcrps_row(const RowP& r, double y, double t, double c,
                                             double xi) {
  const double inf = __builtin_huge_val();
  if (!(t == t)) return __builtin_nan("");  // fmax would drop the NaN
  const double tp = Kind<KIND>::atom ? fmax(t, c) : t;
  if (tp == inf) return 0.0;  // nothing above
  const double yp = fmax(y, tp);
  if constexpr (KIND == GINE_LOSS_NORMAL) {
    if (tp == -inf) return crps_normal(r.mu, r.sigma, y);  // the censored form's limit
    return twcrps_censored(r.mu, r.sigma, 0.0, yp, tp);
  } else if constexpr (KIND == GINE_LOSS_MIXED_NORMAL) {
    return twcrps_censored(r.mu, r.sigma, r.p, yp, tp);
  } else {
    if (tp < r.u) return crps_mixed(r.mu, r.sigma, r.p, r.su, r.u, yp, tp, xi);
    return twcrps_tail(r, yp, tp, xi);
  }
}

// k_forecast_score's layout: wave 0 loads the tile's rows into LDS, then the four waves take
// the thresholds in turn (index T: the count of valid rows), lane = row; one butterfly sum per
// threshold gives the workgroup's partial, the last ticket sums the partials in a fixed order.
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_forecast_twcrps(
    const float* __restrict__ pred, const float* __restrict__ y, int64_t n, double u_fixed,
    double xi, double c, const double* __restrict__ x, int T, double* __restrict__ rows_out,
    double* __restrict__ mean, double* __restrict__ valid, double* __restrict__ partials,
    unsigned int* __restrict__ ticket) {
  __shared__ RowP s_row[kRows];
  __shared__ double s_y[kRows];
  __shared__ double s_red[kThreads];
  __shared__ int s_last;
  const double nan = __builtin_nan("");
  const int64_t first = blockIdx.x * (int64_t)kRows;
  const int rows = (int)min<int64_t>(kRows, n - first);
  if (threadIdx.x < kRows) {
    double ye = nan;
    if ((int)threadIdx.x < rows) {
      const int64_t i = first + threadIdx.x;
      const float yf = y[i];
      s_row[threadIdx.x] = load_row<KIND>(pred, i, u_fixed, c);
      if (yf == yf) ye = (double)yf;
    }
    s_y[threadIdx.x] = ye;
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const double ye = s_y[lane];
  const bool ok = ye == ye;  // false for the lanes past the tile's rows too
  double* part = partials + (size_t)blockIdx.x * (size_t)(T + 1);
  for (int t = threadIdx.x / kWave; t <= T; t += kThreads / kWave) {
    double v = ok ? 1.0 : 0.0;
    if (t < T) {
      const double r = ok ? twcrps_row<KIND>(s_row[lane], ye, x[t], c, xi) : nan;
      if (rows_out && lane < rows) rows_out[(first + lane) * (int64_t)T + t] = r;
      v = ok ? r : 0.0;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) v += shfl_xor_d(v, off);
    if (lane == 0)
      __hip_atomic_exchange(&part[t], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // every wave's partials are out
  if (threadIdx.x == 0) {
    const unsigned int prev =
        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  // fixed order: thread j sums workgroups j, j + 256, ..., then one tree; the count first
  const int P = gridDim.x;
  double count = 0.0;
  for (int k = 0; k <= T; ++k) {
    const int t = k == 0 ? T : k - 1;
    double a = 0.0;
    for (int p = threadIdx.x; p < P; p += kThreads)
      a += __hip_atomic_load(&partials[(size_t)p * (size_t)(T + 1) + t], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    s_red[threadIdx.x] = a;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (k == 0) {
        count = s_red[0];
        if (valid) valid[0] = count;
      } else {
        mean[t] = s_red[0] / count;  // NaN when no target is valid
      }
    }
    __syncthreads();  // s_red[0] has been read
  }
  if (threadIdx.x == 0) *ticket = 0u;  // re-armed for the next call (stream order)
}

// The raw ensemble's twCRPS: crps / crps_fair of k_ensemble_score on max(x_i, t), max(y, t).
// Clamping is monotone, so the members' stable ranks order the clamped values as well: one
// ranking per row serves every threshold.  Lane k keeps threshold t0 + k's pair of values.
__global__ __launch_bounds__(kThreads) void k_ensemble_twcrps(
    const float* __restrict__ members, int64_t row_stride, int64_t member_stride, int M,
    double scale, double shift, const float* __restrict__ y, int64_t n,
    const double* __restrict__ x, int T, double* __restrict__ rows_out,
    double* __restrict__ fair_out) {
  const int64_t row = blockIdx.x * (int64_t)kEnsRows + threadIdx.x / kWave;
  if (row >= n) return;  // the whole wave
  const int lane = threadIdx.x & (kWave - 1);
  const double nan = __builtin_nan("");
  const Member e = load_member(members, row, row_stride, member_stride, M, scale, shift);
  const bool ok = e.x == e.x;
  const double dm = (double)e.m;
  const double coef = (double)(2 * e.rank - e.m - 1);
  const float yf = y[row];
  const bool scored = yf == yf && e.m > 0;  // wave-uniform
  const double yy = (double)yf;
  for (int t0 = 0; t0 < T; t0 += kWave) {
    const int cnt = min(kWave, T - t0);
    double mine = nan, mine_fair = nan;
    for (int k = 0; k < cnt; ++k) {
      const double t = x[t0 + k];
      if (!scored || !(t == t)) continue;  // wave-uniform
      const double xc = fmax(e.x, t), yc = fmax(yy, t);
      const double a = wave_sum(ok ? fabs(xc - yc) : 0.0);
      const double s = wave_sum(ok ? coef * xc : 0.0);
      if (lane == k) {
        mine = a / dm - s / (dm * dm);
        if (e.m > 1) mine_fair = a / dm - s / (dm * (dm - 1.0));
      }
    }
    if (lane < cnt) {
      rows_out[row * (int64_t)T + t0 + lane] = mine;
      fair_out[row * (int64_t)T + t0 + lane] = mine_fair;
    }
  }
}

// members view and sizes, before any HIP call
int check_members(int64_t num_rows, int64_t row_stride, int64_t member_stride,
                  int32_t num_members) {
  if (num_rows < 0 || row_stride < 0 || member_stride < 0) return GINE_ERR_INVALID;
  if (num_members < 1 || num_members > kEnsMaxMembers) return GINE_ERR_INVALID;
  if (ceil_div(num_rows, kEnsRows) > 0x7fffffff) return GINE_ERR_TOO_LARGE;
  return GINE_OK;
}

// kind, sizes and the distribution's domain (c < u, 0 < xi < 1), before any HIP call
int check_domain(int64_t num_nodes, int32_t kind, double u, double xi, double c,
                 int64_t points) {
  if (kind < GINE_LOSS_NORMAL || kind > GINE_LOSS_MIXED_U) return GINE_ERR_INVALID;
  if (num_nodes < 0 || points < 0) return GINE_ERR_INVALID;
  if (!(c == c)) return GINE_ERR_INVALID;
  if (kind == GINE_LOSS_MIXED || kind == GINE_LOSS_MIXED_U) {
    if (!(xi > 0.0 && xi < 1.0)) return GINE_ERR_INVALID;
    if (kind == GINE_LOSS_MIXED && !(u > c)) return GINE_ERR_INVALID;
    if (kind == GINE_LOSS_MIXED_U && !(c < 0.0)) return GINE_ERR_INVALID;  // u in (0, 2.12)
  }
  if (points > kMaxPoints || ceil_div(num_nodes, kRows) > 0x7fffffff) return GINE_ERR_TOO_LARGE;
  return GINE_OK;
}

template <bool QUANTILE>
int launch_points(const float* pred, int64_t num_nodes, int32_t kind, double u, double xi,
                  double c, const double* x, int32_t T, int32_t flags, double* out,
                  void* stream) {
  const int rc = check_domain(num_nodes, kind, u, xi, c, T);
  if (rc != GINE_OK) return rc;
  if (flags & ~GINE_FORECAST_UPPER) return GINE_ERR_INVALID;
  if (num_nodes == 0 || T == 0) return GINE_OK;
  if (!pred || !x || !out) return GINE_ERR_INVALID;
  const dim3 grid((unsigned)ceil_div(num_nodes, kRows));
  const int upper = (flags & GINE_FORECAST_UPPER) != 0;
#define LAUNCH_POINTS(KIND_)                                                                  \
  hipLaunchKernelGGL((k_forecast_points<KIND_, QUANTILE>), grid, dim3(kThreads), 0,           \
                     as_stream(stream), pred, num_nodes, u, xi, c, x, (uint32_t)T, upper, out)
  switch (kind) {
    case GINE_LOSS_NORMAL: LAUNCH_POINTS(GINE_LOSS_NORMAL); break;
    case GINE_LOSS_MIXED_NORMAL: LAUNCH_POINTS(GINE_LOSS_MIXED_NORMAL); break;
    case GINE_LOSS_MIXED: LAUNCH_POINTS(GINE_LOSS_MIXED); break;
    default: LAUNCH_POINTS(GINE_LOSS_MIXED_U); break;
  }
#undef LAUNCH_POINTS
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

}  // namespace
}  // namespace gine

using namespace gine;

extern "C" int gine_forecast_prob(const float* pred, int64_t num_nodes, int32_t kind, double u,
                                  double xi, double c, const double* x, int32_t num_x,
                                  int32_t flags, double* out, void* stream) {
  return launch_points<false>(pred, num_nodes, kind, u, xi, c, x, num_x, flags, out, stream);
}

extern "C" int gine_forecast_quantile(const float* pred, int64_t num_nodes, int32_t kind,
                                      double u, double xi, double c, const double* level,
                                      int32_t num_levels, int32_t flags, double* out,
                                      void* stream) {
  return launch_points<true>(pred, num_nodes, kind, u, xi, c, level, num_levels, flags, out,
                             stream);
}

extern "C" int gine_forecast_score_partials(int64_t num_nodes, int32_t num_x, size_t* count) {
  if (!count || num_nodes < 0 || num_x < 0) return GINE_ERR_INVALID;
  if (num_x > kMaxPoints || ceil_div(num_nodes, kRows) > 0x7fffffff) return GINE_ERR_TOO_LARGE;
  const int64_t blocks = ceil_div(num_nodes, kRows) > 0 ? ceil_div(num_nodes, kRows) : 1;
  *count = (size_t)blocks * (size_t)(num_x + 1);
  return GINE_OK;
}

extern "C" int gine_forecast_score(const float* pred, const float* y, int64_t num_nodes,
                                   int32_t kind, double u, double xi, double c, const double* x,
                                   int32_t num_x, double* crps_rows, double* pit_lo,
                                   double* pit_hi, double* brier, double* valid,
                                   double* partials, uint32_t* ticket, void* stream) {
  const int rc = check_domain(num_nodes, kind, u, xi, c, num_x);
  if (rc != GINE_OK) return rc;
  if (num_nodes == 0) return GINE_OK;
  if (!pred || !y || !partials || !ticket) return GINE_ERR_INVALID;
  if (num_x > 0 && (!x || !brier)) return GINE_ERR_INVALID;
  const dim3 grid((unsigned)ceil_div(num_nodes, kRows));
#define LAUNCH_SCORE(KIND_)                                                                    \
  hipLaunchKernelGGL((k_forecast_score<KIND_>), grid, dim3(kThreads), 0, as_stream(stream),    \
                     pred, y, num_nodes, u, xi, c, x, (int)num_x, crps_rows, pit_lo, pit_hi,   \
                     brier, valid, partials, ticket)
  switch (kind) {
    case GINE_LOSS_NORMAL: LAUNCH_SCORE(GINE_LOSS_NORMAL); break;
    case GINE_LOSS_MIXED_NORMAL: LAUNCH_SCORE(GINE_LOSS_MIXED_NORMAL); break;
    case GINE_LOSS_MIXED: LAUNCH_SCORE(GINE_LOSS_MIXED); break;
    default: LAUNCH_SCORE(GINE_LOSS_MIXED_U); break;
  }
#undef LAUNCH_SCORE
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_ensemble_score(const float* members, int64_t row_stride,
                                   int64_t member_stride, int32_t num_members, double scale,
                                   double shift, const float* y, int64_t num_rows,
                                   const double* x, int32_t num_x, double* crps_rows,
                                   double* crps_fair_rows, double* rank_lo, double* rank_hi,
                                   double* members_valid, double* prob, void* stream) {
  const int rc = check_members(num_rows, row_stride, member_stride, num_members);
  if (rc != GINE_OK) return rc;
  if (num_x < 0) return GINE_ERR_INVALID;
  if (num_x > kMaxPoints) return GINE_ERR_TOO_LARGE;
  if (num_rows == 0) return GINE_OK;
  if (!members) return GINE_ERR_INVALID;
  if (num_x > 0 && (!x || !prob)) return GINE_ERR_INVALID;
  const dim3 grid((unsigned)ceil_div(num_rows, kEnsRows));
  hipLaunchKernelGGL(k_ensemble_score, grid, dim3(kThreads), 0, as_stream(stream), members,
                     row_stride, member_stride, (int)num_members, scale, shift, y, num_rows, x,
                     (int)num_x, crps_rows, crps_fair_rows, rank_lo, rank_hi, members_valid,
                     prob);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_ensemble_ecc(const float* pred, int64_t num_nodes, int32_t kind, double u,
                                 double xi, double c, const float* members, int64_t row_stride,
                                 int64_t member_stride, int32_t num_members, double scale,
                                 double shift, int32_t flags, double* out, void* stream) {
  int rc = check_domain(num_nodes, kind, u, xi, c, 0);
  if (rc != GINE_OK) return rc;
  rc = check_members(num_nodes, row_stride, member_stride, num_members);
  if (rc != GINE_OK) return rc;
  if (flags & ~GINE_ECC_MIDPOINT) return GINE_ERR_INVALID;
  if (num_nodes == 0) return GINE_OK;
  if (!pred || !members || !out) return GINE_ERR_INVALID;
  const dim3 grid((unsigned)ceil_div(num_nodes, kEnsRows));
  const int midpoint = (flags & GINE_ECC_MIDPOINT) != 0;
#define LAUNCH_ECC(KIND_)                                                                     \
  hipLaunchKernelGGL((k_ensemble_ecc<KIND_>), grid, dim3(kThreads), 0, as_stream(stream),     \
                     pred, num_nodes, u, xi, c, members, row_stride, member_stride,           \
                     (int)num_members, scale, shift, midpoint, out)
  switch (kind) {
    case GINE_LOSS_NORMAL: LAUNCH_ECC(GINE_LOSS_NORMAL); break;
    case GINE_LOSS_MIXED_NORMAL: LAUNCH_ECC(GINE_LOSS_MIXED_NORMAL); break;
    case GINE_LOSS_MIXED: LAUNCH_ECC(GINE_LOSS_MIXED); break;
    default: LAUNCH_ECC(GINE_LOSS_MIXED_U); break;
  }
#undef LAUNCH_ECC
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_forecast_twcrps_partials(int64_t num_nodes, int32_t num_x, size_t* count) {
  return gine_forecast_score_partials(num_nodes, num_x, count);  // the same tiles and columns
}

extern "C" int gine_forecast_twcrps(const float* pred, const float* y, int64_t num_nodes,
                                    int32_t kind, double u, double xi, double c, const double* x,
                                    int32_t num_x, double* rows, double* mean, double* valid,
                                    double* partials, uint32_t* ticket, void* stream) {
  const int rc = check_domain(num_nodes, kind, u, xi, c, num_x);
  if (rc != GINE_OK) return rc;
  if (num_nodes == 0) return GINE_OK;
  if (!pred || !y || !partials || !ticket) return GINE_ERR_INVALID;
  if (num_x > 0 && (!x || !mean)) return GINE_ERR_INVALID;
  const dim3 grid((unsigned)ceil_div(num_nodes, kRows));
#define LAUNCH_TW(KIND_)                                                                       \
  hipLaunchKernelGGL((k_forecast_twcrps<KIND_>), grid, dim3(kThreads), 0, as_stream(stream),   \
                     pred, y, num_nodes, u, xi, c, x, (int)num_x, rows, mean, valid, partials, \
                     ticket)
  switch (kind) {
    case GINE_LOSS_NORMAL: LAUNCH_TW(GINE_LOSS_NORMAL); break;
    case GINE_LOSS_MIXED_NORMAL: LAUNCH_TW(GINE_LOSS_MIXED_NORMAL); break;
    case GINE_LOSS_MIXED: LAUNCH_TW(GINE_LOSS_MIXED); break;
    default: LAUNCH_TW(GINE_LOSS_MIXED_U); break;
  }
#undef LAUNCH_TW
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}

extern "C" int gine_ensemble_twcrps(const float* members, int64_t row_stride,
                                    int64_t member_stride, int32_t num_members, double scale,
                                    double shift, const float* y, int64_t num_rows,
                                    const double* x, int32_t num_x, double* rows,
                                    double* fair_rows, void* stream) {
  const int rc = check_members(num_rows, row_stride, member_stride, num_members);
  if (rc != GINE_OK) return rc;
  if (num_x < 0) return GINE_ERR_INVALID;
  if (num_x > kMaxPoints) return GINE_ERR_TOO_LARGE;
  if (num_rows == 0 || num_x == 0) return GINE_OK;
  if (!members || !y || !x || !rows || !fair_rows) return GINE_ERR_INVALID;
  const dim3 grid((unsigned)ceil_div(num_rows, kEnsRows));
  hipLaunchKernelGGL(k_ensemble_twcrps, grid, dim3(kThreads), 0, as_stream(stream), members,
                     row_stride, member_stride, (int)num_members, scale, shift, y, num_rows, x,
                     (int)num_x, rows, fair_rows);
  GINE_LAUNCH_STATUS();
  return GINE_OK;
}
