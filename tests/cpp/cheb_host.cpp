// Host arithmetic of the smoothers' Chebyshev recurrence: struct Cheb as written in openifem_amd/csrc/solver.hip against the recurrence as the
// smoothers spelled it inline before (mg_sm_smooth, mg_uu_smooth, the mode-3 residual update, mg_uu_entry_c0).  Both must give the same BITS
// for the first coefficient c0 and for every pair (a_k, b_k).  No GPU, no library:
//   hipcc -O3 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all cheb_host.cpp -o /tmp/cheb_host && /tmp/cheb_host
// Intervals: random 0 < lo < hi over 24 decades, and the four rules of mg_sm_sweep / mg_uu_sweep at random lambda_max and ratio
// (hi = 1.1 lambda_max; lo = hi / 900, hi / 400, hi / ratio with the ratios of both multigrids); 1 to 32 steps each.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

// ---- as in solver.hip
struct ChebSweep { double lo, hi; int steps; };
struct Cheb {
  double theta, delta, sigma, rho;
  Cheb(double lo, double hi) : theta(0.5 * (hi + lo)), delta(0.5 * (hi - lo)), sigma(theta / delta), rho(1.0 / sigma) {}
  explicit Cheb(const ChebSweep &w) : Cheb(w.lo, w.hi) {}
  double c0() const { return 1.0 / theta; }
  void next(double &a, double &b) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    a = rho_new * rho; b = 2.0 * rho_new / delta; rho = rho_new;
  }
};

// ---- the inline form it replaces: c0, then (a_k, b_k) for k < nsteps
static void inline_recurrence(double lo, double hi, int nsteps, double &c0, std::vector<double> &ab) {
  const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = theta / delta;
  double rho_old = 1.0 / sigma;
  c0 = 1.0 / theta;
  for (int k = 0; k < nsteps; ++k) {
    const double rho_new = 1.0 / (2.0 * sigma - rho_old);
    ab.push_back(rho_new * rho_old);
    ab.push_back(2.0 * rho_new / delta);
    rho_old = rho_new;
  }
}
// (the residual update after the coarse correction and the entry of the cycle wrote the first coefficient as one expression)
static double inline_c0(double lo, double hi) { return 1.0 / (0.5 * (hi + lo)); }

static bool same_bits(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

int main() {
  std::mt19937_64 gen(20240611);
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  std::uniform_int_distribution<int> steps_of(1, 32);
  long cases = 0, coefficients = 0, bad = 0;
  auto check = [&](double lo, double hi) {
    if (!(lo > 0 && lo < hi)) return;
    const int nsteps = steps_of(gen);
    double c0_ref;
    std::vector<double> ref, got;
    inline_recurrence(lo, hi, nsteps, c0_ref, ref);
    const ChebSweep w{lo, hi, nsteps};
    Cheb ch(w);
    const double c0 = ch.c0(), c0_pair = Cheb(lo, hi).c0(), c0_one = inline_c0(lo, hi);
    for (int k = 0; k < w.steps; ++k) {
      double a, b;
      ch.next(a, b);
      got.push_back(a); got.push_back(b);
    }
    const bool ok = same_bits(&c0, &c0_ref, 1) && same_bits(&c0_pair, &c0_ref, 1) && same_bits(&c0_one, &c0_ref, 1) && got.size() == ref.size() &&
                    same_bits(got.data(), ref.data(), ref.size());
    if (!ok && bad++ < 10) std::fprintf(stderr, "MISMATCH lo %.17g hi %.17g steps %d\n", lo, hi, nsteps);
    ++cases; coefficients += 1 + long(ref.size());
  };
  for (int i = 0; i < 200000; ++i) {
    // any interval: hi over 24 decades, lo anywhere below it (down to 1e-6 hi, and close to hi)
    const double hi = std::pow(10.0, -12.0 + 24.0 * u01(gen));
    check(hi * std::pow(10.0, -6.0 * u01(gen)), hi);
    check(hi * (1.0 - std::pow(10.0, -1.0 - 12.0 * u01(gen))), hi);
    // the rules of the two multigrids at a random eigenvalue bound
    const double lmax = std::pow(10.0, -3.0 + 6.0 * u01(gen)), h = 1.1 * lmax;
    check(h / 900.0, h);                              // S_m, coarsest level
    check(h / 400.0, h);                              // A_uu, coarsest level
    check(h / std::fmax(1.5, 1.0 + 15.0 * u01(gen)), h); // either, any ratio an option can set (at least 1.5)
    check(h / 4.0, h);                                // S_m, default ratio
    check(h / 8.0, h);                                // A_uu, default ratio
  }
  std::printf("cheb_host: %ld intervals, %ld coefficients compared, %ld mismatches\n", cases, coefficients, bad);
  return bad == 0 ? 0 : 1;
}
