// Forward-mode dual numbers and the closed-form CRPS of the reference's losses
// (models/loss.py) over them: the value and its exact gradient w.r.t. the K prediction
// columns in one evaluation.  Shared by the fused losses (gine_loss.hip) and the EMOS fit
// (gine_emos.hip); one private copy per translation unit.
#pragma once

#include "gine_common.hpp"

namespace gine {
namespace {

constexpr double kInvSqrtPi = 0.56418958354775628695;   // 1/sqrt(pi)
constexpr double kLogSqrt2Pi = 0.91893853320467274178;  // log(sqrt(2 pi))
constexpr double kSqrt2 = 1.41421356237309504880;

// ---------------------------------------------------------------------------------------
// forward-mode dual numbers: value + gradient w.r.t. the K prediction columns
// ---------------------------------------------------------------------------------------
template <int K>
struct Dual {
  double v;
  double d[K];
};

template <int K>
__device__ __forceinline__ Dual<K> cst(double v) {
  Dual<K> r;
  r.v = v;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = 0.0;
  return r;
}
template <int K>
__device__ __forceinline__ Dual<K> var(double v, int i) {
  Dual<K> r = cst<K>(v);
  r.d[i] = 1.0;
  return r;
}
// f(x) with derivative f'(x): chain rule
template <int K>
__device__ __forceinline__ Dual<K> apply(const Dual<K>& x, double f, double df) {
  Dual<K> r;
  r.v = f;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = df * x.d[i];
  return r;
}
template <int K>
__device__ __forceinline__ Dual<K> operator+(const Dual<K>& a, const Dual<K>& b) {
  Dual<K> r;
  r.v = a.v + b.v;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = a.d[i] + b.d[i];
  return r;
}
template <int K>
__device__ __forceinline__ Dual<K> operator-(const Dual<K>& a, const Dual<K>& b) {
  Dual<K> r;
  r.v = a.v - b.v;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = a.d[i] - b.d[i];
  return r;
}
template <int K>
__device__ __forceinline__ Dual<K> operator-(const Dual<K>& a) {
  return apply(a, -a.v, -1.0);
}
template <int K>
__device__ __forceinline__ Dual<K> operator*(const Dual<K>& a, const Dual<K>& b) {
  Dual<K> r;
  r.v = a.v * b.v;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
template <int K>
__device__ __forceinline__ Dual<K> operator/(const Dual<K>& a, const Dual<K>& b) {
  Dual<K> r;
  r.v = a.v / b.v;
  const double inv = 1.0 / b.v;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * inv;
  return r;
}
template <int K>
__device__ __forceinline__ Dual<K> operator*(double s, const Dual<K>& a) {
  return apply(a, s * a.v, s);
}
template <int K>
__device__ __forceinline__ Dual<K> operator+(double s, const Dual<K>& a) {
  return apply(a, s + a.v, 1.0);
}
template <int K>
__device__ __forceinline__ Dual<K> operator-(double s, const Dual<K>& a) {
  return apply(a, s - a.v, -1.0);
}
template <int K>
__device__ __forceinline__ Dual<K> sq(const Dual<K>& a) {
  return apply(a, a.v * a.v, 2.0 * a.v);
}
template <int K>
__device__ __forceinline__ Dual<K> dabs(const Dual<K>& a) {  // torch: d|x| = sign(x)
  return apply(a, fabs(a.v), a.v > 0.0 ? 1.0 : (a.v < 0.0 ? -1.0 : 0.0));
}
template <int K>
__device__ __forceinline__ Dual<K> powc(const Dual<K>& a, double c) {  // constant exponent
  const double p = pow(a.v, c);
  return apply(a, p, c * pow(a.v, c - 1.0));
}
// the two powers of pareto_crps at the experiments' xi = 0.5 (params.json "xi": 0.5):
// x^-2 and x^0.5 without pow() -- fp64 pow is the longest routine of the pass, and eight of
// them per node dominated its dependent chain.  Same values and derivatives as powc up to
// the last-bit rounding of pow (inf / NaN / signed-zero cases as pow for every argument
// the pass can produce: 1 + xi*yt and 1 - cdf with cdf <= 1).
template <int K>
__device__ __forceinline__ Dual<K> pow_m2(const Dual<K>& a) {  // a^-2, d = -2 a^-3
  const double p = 1.0 / (a.v * a.v);
  return apply(a, p, -2.0 * (p / a.v));
}
template <int K>
__device__ __forceinline__ Dual<K> pow_half(const Dual<K>& a) {  // a^0.5, d = 0.5 a^-0.5
  const double p = sqrt(a.v);
  return apply(a, p, 0.5 / p);
}
// standard normal cdf / pdf (torch.distributions.Normal(0, 1))
template <int K>
__device__ __forceinline__ Dual<K> Phi(const Dual<K>& z) {
  const double pdf = exp(-0.5 * z.v * z.v - kLogSqrt2Pi);
  return apply(z, 0.5 * (1.0 + erf(z.v / kSqrt2)), pdf);
}
template <int K>
__device__ __forceinline__ Dual<K> phi(const Dual<K>& z) {
  const double pdf = exp(-0.5 * z.v * z.v - kLogSqrt2Pi);
  return apply(z, pdf, -z.v * pdf);
}
template <int K>
__device__ __forceinline__ Dual<K> sigmoid(const Dual<K>& a) {
  const double s = 1.0 / (1.0 + exp(-a.v));
  return apply(a, s, s * (1.0 - s));
}
template <int K>
__device__ __forceinline__ Dual<K> select(bool c, const Dual<K>& a, const Dual<K>& b) {
  return c ? a : b;  // torch.where: gradient flows to the selected branch only
}

// ---------------------------------------------------------------------------------------
// closed forms (restated from models/loss.py)
// ---------------------------------------------------------------------------------------
template <int K>
__device__ Dual<K> crps_normal(const Dual<K>& mu, const Dual<K>& sigma, double y) {
  const Dual<K> z = (cst<K>(y) - mu) / sigma;
  return sigma * (z * (2.0 * Phi(z) - cst<K>(1.0)) + 2.0 * phi(z) - cst<K>(kInvSqrtPi));
}

template <int K>
__device__ Dual<K> crps_mixed_normal(const Dual<K>& mu, const Dual<K>& sigma, const Dual<K>& p,
                                     double y, double c) {
  const Dual<K> yt = (cst<K>(y) - mu) / sigma;
  const Dual<K> ct = (cst<K>(c) - mu) / sigma;
  const Dual<K> q = 1.0 - p;
  const Dual<K> Pc = p + q * Phi(ct);
  const Dual<K> t1 = yt * (2.0 * (p + q * Phi(yt)) - cst<K>(1.0));
  const Dual<K> t2 = -(ct * sq(Pc));
  const Dual<K> t3 = 2.0 * (q * (-phi(ct)) * Pc);
  const Dual<K> t4 = -2.0 * (q * (-phi(yt)));
  const Dual<K> t5 = (-kInvSqrtPi) * (sq(q) * (1.0 - Phi(kSqrt2 * ct)));
  return sigma * (t1 + t2 + t3 + t4 + t5);
}

template <int K>
__device__ Dual<K> pareto_crps(const Dual<K>& y, const Dual<K>& u, const Dual<K>& m,
                               const Dual<K>& s, double xi) {
  const Dual<K> yt = (y - u) / s;
  const bool half = xi == 0.5;  // a kernel argument: uniform
  const Dual<K> base = 1.0 + xi * yt;
  const Dual<K> cdf =
      select(yt.v <= 0.0, cst<K>(0.0), 1.0 - (half ? pow_m2(base) : powc(base, -1.0 / xi)));
  const Dual<K> om = 1.0 - m;
  const Dual<K> tail = 1.0 - cdf;
  return s * (dabs(yt) -
              (2.0 / (1.0 - xi)) * (om * (1.0 - (half ? pow_half(tail) : powc(tail, 1.0 - xi)))) +
              (1.0 / (2.0 - xi)) * sq(om));
}

template <int K, bool GRAD_U>
__device__ Dual<K> crps_mixed(const Dual<K>& mu, const Dual<K>& sigma, const Dual<K>& p,
                              const Dual<K>& su, const Dual<K>& u, double y, double c,
                              double xi, double t) {
  const Dual<K> yy = cst<K>(y);
  const Dual<K> ct = (cst<K>(c) - mu) / sigma;
  const Dual<K> ut = (u - mu) / sigma;
  const Dual<K> yt = (yy - mu) / sigma;
  const Dual<K> q = 1.0 - p;
  const Dual<K> m_u = p + q * Phi(ut);
  const Dual<K> Pc = p + q * Phi(ct);
  const Dual<K> Pu = q * (1.0 - Phi(ut));
  const Dual<K> t2 = ut * sq(Pu) - ct * sq(Pc);
  const Dual<K> t3 = -2.0 * (q * phi(ct) * Pc + q * phi(ut) * Pu);
  const Dual<K> t5 = (-kInvSqrtPi) * (sq(q) * (Phi(kSqrt2 * ut) - Phi(kSqrt2 * ct)));
  const Dual<K> mixed = sigma * (yt * (2.0 * (p + q * Phi(yt)) - cst<K>(1.0)) + t2 + t3 +
                                 2.0 * (q * phi(yt)) + t5);
  const Dual<K> upper = sigma * (ut + t2 + t3 + (-2.0) * (q * (-phi(ut)) + ut * Pu) + t5);
  const Dual<K> loss1 = mixed + pareto_crps(u, u, m_u, su, xi);
  const Dual<K> loss2 = pareto_crps(yy, u, m_u, su, xi) + upper;
  if constexpr (GRAD_U) {
    return sigmoid(t * (u - yy)) * (loss1 - loss2) + loss2;
  } else {
    return select(y < u.v, loss1, loss2);
  }
}

template <int KIND>
struct LossK {
  static constexpr int value = KIND == GINE_LOSS_NORMAL ? 2
                               : KIND == GINE_LOSS_MIXED_NORMAL ? 3
                               : KIND == GINE_LOSS_MIXED ? 4 : 5;
};

}  // namespace
}  // namespace gine
