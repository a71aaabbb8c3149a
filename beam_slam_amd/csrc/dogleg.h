// The scalar arithmetic of Ceres' DOGLEG trust-region strategy with TRADITIONAL_DOGLEG ([EXT] ceres 1.14 internal/ceres/dogleg_strategy.cc,
// recalled like SURVEY.md Appendix B; the minimiser around it is LmState, lm_state.h).  Host-compilable and free of HIP so that the driver
// (bsgpu_solve.cpp solve_dogleg) and tests/plan/test_dogleg.cpp compile the same code.
//
// Ceres' form.  The minimiser scales the Jacobian's columns, J~ = J S with s_j = 1/(1+|J_j|) (jacobi_scaling; from iteration 0), and the
// strategy works in J~'s coordinates with
//   d_j = sqrt(clamp(|J~_j|^2, min_lm_diagonal, max_lm_diagonal)),  g' = (S g) / d  (g = J^T r),  trust region |D u~| <= radius.
//   Cauchy point  -alpha g',  alpha = |g'|^2 / |J~ D^-1 g'|^2
//   Gauss-Newton  (J~^T J~ + mu D^2) y~ = S g,  gn' = -D y~      (mu from 1e-8; x10 per failed solve while mu < 1)
//   case 1  |gn'| <= radius                 : step' = gn'
//   case 2  alpha |g'| >= radius            : step' = -(radius / |g'|) g'
//   case 3  otherwise                       : step' = -alpha (1 - beta) g' + beta gn', |step'| = radius (beta: the cancellation-safe root)
//   delta = S D^-1 step'
//   StepAccepted(rho): rho < 0.25 -> radius /= 2;  rho > 0.75 -> radius = max(radius, 3 |step'|);  mu = max(1e-8, 2 mu / 10)
//   StepRejected: radius /= 2, the Gauss-Newton step and the Cauchy point are reused.  StepIsInvalid: mu *= 10, a new solve.
//
// The project's unscaled form.  The kernels keep J unscaled and store c_j = clamp(s_j^2 H_jj, lo, hi) / s_j^2 (the `dcl`
// arrays), so d_j = s_j sqrt(c_j) and every quantity above is a function of c, g and the unscaled Gauss-Newton step delta_gn alone:
//   (J~^T J~ + mu D^2) y~ = S g  <=>  (H + mu diag(c)) y = g, y = S y~: the LM system with 1 / radius replaced by mu, so delta_gn = -y comes
//   from the unchanged assembly -> factorisation -> back-substitution run at radius 1 / mu;
//   |g'|^2 = sum g_j^2 / c_j,  |gn'|^2 = sum c_j delta_gn_j^2,  g'.gn' = sum g_j delta_gn_j,
//   J~ D^-1 g' = J v with v_j = g_j / c_j,  and delta = a v + b delta_gn with (a, b) from dl_coefficients below,  |step'|^2 = sum c_j delta_j^2.
#pragma once
#include <cmath>

namespace bsg {

constexpr double kDoglegMinMu = 1e-8, kDoglegMaxMu = 1.0, kDoglegMuIncrease = 10.0;
constexpr double kDoglegDecreaseThreshold = 0.25, kDoglegIncreaseThreshold = 0.75;

// what a Gauss-Newton solve leaves for the interpolation: the reductions of the vector kernel (k_dogleg.hip) and the Cauchy denominator
struct DoglegVecs {
  double g2 = 0.0;    // |g'|^2
  double gn2 = 0.0;   // |gn'|^2
  double ggn = 0.0;   // g'.gn'
  double jv2 = 0.0;   // |J~ D^-1 g'|^2
};

// the step as delta = a v + b delta_gn (v_j = g_j / c_j); `kase` 1..3 as above, `norm` = |step'| as Ceres' dogleg_step_norm_ would hold it
// except in case 3, where it is measured on the vector the step kernel forms (norm_is_measured = true)
struct DoglegStep {
  int kase = 0;
  double a = 0.0, b = 0.0, alpha = 0.0, beta = 0.0, norm = 0.0;
  bool norm_is_measured = false;
};

inline DoglegStep dl_coefficients(const DoglegVecs& w, double radius) {
  DoglegStep s;
  const double gradient_norm = std::sqrt(w.g2), gauss_newton_norm = std::sqrt(w.gn2);
  s.alpha = w.g2 / w.jv2;
  if (gauss_newton_norm <= radius) {   // case 1
    s.kase = 1; s.a = 0.0; s.b = 1.0; s.norm = gauss_newton_norm;
    return s;
  }
  if (gradient_norm * s.alpha >= radius) {   // case 2
    s.kase = 2; s.a = -(radius / gradient_norm); s.b = 0.0; s.norm = radius;   // (delta = S D^-1 step' = -(radius / |g'|) v)
    return s;
  }
  // case 3: a = alpha * -g', b = gn';  b.a = -alpha g'.gn'
  const double b_dot_a = -s.alpha * w.ggn;
  const double a_squared_norm = std::pow(s.alpha * gradient_norm, 2.0);
  const double b_minus_a_squared_norm = a_squared_norm - 2 * b_dot_a + std::pow(gauss_newton_norm, 2);
  const double c = b_dot_a - a_squared_norm;
  const double d = std::sqrt(c * c + b_minus_a_squared_norm * (std::pow(radius, 2.0) - a_squared_norm));
  s.beta = (c <= 0) ? (d - c) / b_minus_a_squared_norm : (radius * radius - a_squared_norm) / (d + c);
  s.kase = 3;
  s.a = -s.alpha * (1.0 - s.beta);
  s.b = s.beta;
  s.norm_is_measured = true;
  return s;
}

// DoglegStrategy::StepAccepted: the radius and mu after an accepted step of quality rho and scaled norm step_norm
inline void dl_step_accepted(double rho, double step_norm, double* radius, double* mu) {
  if (rho < kDoglegDecreaseThreshold) *radius *= 0.5;
  if (rho > kDoglegIncreaseThreshold) *radius = std::fmax(*radius, 3.0 * step_norm);
  *mu = std::fmax(kDoglegMinMu, 2.0 * *mu / kDoglegMuIncrease);
}
inline void dl_step_rejected(double* radius) { *radius *= 0.5; }
inline void dl_step_invalid(double* mu) { *mu *= kDoglegMuIncrease; }
// a failed solve inside one ComputeStep: whether another attempt at the larger mu follows
inline bool dl_retry(double* mu) {
  *mu *= kDoglegMuIncrease;
  return *mu < kDoglegMaxMu;
}

}  // namespace bsg
