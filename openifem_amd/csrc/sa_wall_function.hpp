// sa_wall_function.hpp -- SpalartAllmaras::get_shear_velocity (mpi_spalart_allmaras.cpp:218-280), once, for the host entry point
// ifem_sa_get_shear_velocity and for the kernel of ifem_sa_update_shear_velocity (sa_wall.hip).  Restated literally: the |vel| < 1e-10
// test, the sublayer branch, the floor of the initial guess, the constants of the analytical wall profile (:238-258) and at most 30
// Newton steps that stop at |delta| < 1e-2 |u_tau|.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IFEM_HD __host__ __device__
#else
#define IFEM_HD
#endif

namespace ifem {

// nu = viscosity / fluid_rho, dist = spalart_allmaras_image_distance
IFEM_HD inline double sa_shear_velocity(double nu, double dist, double vel, double init_guess) {
  if (fabs(vel) < 1e-10) return 0.0; // usually not on this process or out of bound (:222-225)
  if (vel * dist / nu < sqrt(5.0)) return vel / sqrt(vel * dist / nu); // viscous sublayer (y+ < 5, u+ = y+)
  init_guess = fmax(init_guess, 5.0 * nu / dist);
  constexpr double B = 5.03339088, a1 = 8.14822158, a2 = -6.92870938, b1 = 7.46008761, b2 = 7.46814579, c1 = 2.54967735, c2 = 1.33016516,
                   c3 = 3.59945911, c4 = 3.63975319;
  constexpr double kappa = 0.41, c_nu1_cubed = 7.1 * 7.1 * 7.1, kappa_cubed = kappa * kappa * kappa;
  constexpr int max_iter = 30;
  constexpr double tol = 1e-2;
  double ut = init_guess;
  for (int i = 0; i < max_iter; ++i) {
    const double yp = ut * dist / nu;
    const double up = B + c1 * log((yp + a1) * (yp + a1) + b1 * b1) - c2 * log((yp + a2) * (yp + a2) + b2 * b2) - c3 * atan2(b1, yp + a1) -
                      c4 * atan2(b2, yp + a2);
    const double dup = (kappa_cubed * yp * yp * yp) / (c_nu1_cubed + kappa_cubed * yp * yp * yp);
    const double ut_next = ut - (ut * up - vel) / (up + ut * dist / nu * dup);
    const bool done = fabs(ut_next - ut) < tol * fabs(ut);
    ut = ut_next;
    if (done) break;
  }
  return ut;
}

} // namespace ifem
