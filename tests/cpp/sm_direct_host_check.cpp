// Stand-alone check of the host side of the fast-diagonalisation S_m solve (csrc/sm_direct_host.cpp): 1D factors, generalised eigen-solver,
// refusals, mask reader.  Prints "ok (0 failures)" and returns 0 when everything holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <random>
#include "sm_direct_host.hpp"
using namespace ifem;

static int fails = 0;
static void expect(bool ok, const char *what, int a = 0, int b = 0) {
  if (!ok) { printf("FAIL %s (%d, %d)\n", what, a, b); ++fails; }
}
static bool near(double a, double b, double scale) { return std::fabs(a - b) <= 1e-14 * scale; }

// the assembled 1D tables against their closed-form entries
static void check_tables(int n, double h) {
  std::vector<double> N, G, m;
  smd_1d_tables(n, h, N, G, m);
  const int np = n + 1, nu = 2 * n + 1;
  expect(int(N.size()) == np * nu && int(G.size()) == np * nu && int(m.size()) == nu, "table sizes", n);
  for (int j = 0; j < nu; ++j) {
    const double want = j % 2 ? 8.0 * h / 15.0 : ((j == 0 || j == nu - 1) ? 2.0 * h / 15.0 : 4.0 * h / 15.0);
    expect(near(m[j], want, h), "m", n, j);
  }
  for (int i = 0; i < np; ++i)
    for (int j = 0; j < nu; ++j) {
      const int d = j - 2 * i;
      double wn = 0, wg = 0;
      if (d == 0) { wn = (i == 0 || i == n) ? h / 6.0 : h / 3.0; wg = i == 0 ? -5.0 / 6.0 : (i == n ? 5.0 / 6.0 : 0.0); }
      else if (d == 1 || d == -1) { wn = h / 3.0; wg = d * 2.0 / 3.0; }
      else if (d == 2 || d == -2) { wn = 0.0; wg = d / 2 * (1.0 / 6.0); }
      expect(near(N[size_t(i) * nu + j], wn, h), "N", i, j);
      expect(near(G[size_t(i) * nu + j], wg, 1.0), "G", i, j);
    }
  // F = X diag(d / m) X^T against the plain triple product, both masks
  for (int mask = 0; mask < 8; ++mask) {
    std::vector<double> F;
    const std::vector<double> &X = mask & 4 ? G : N;
    smd_factor(n, X, m, mask & 1, mask & 2, F);
    double worst = 0, big = 0;
    for (int i = 0; i < np; ++i)
      for (int k = 0; k < np; ++k) {
        double s = 0;
        for (int j = 0; j < nu; ++j) {
          const double d = ((j == 0 && (mask & 1)) || (j == nu - 1 && (mask & 2))) ? 0.0 : 1.0;
          s += X[size_t(i) * nu + j] * d / m[j] * X[size_t(k) * nu + j];
        }
        worst = std::max(worst, std::fabs(s - F[size_t(i) * np + k]));
        big = std::max(big, std::fabs(s));
      }
    expect(worst <= 1e-14 * big, "F against the triple product", n, mask);
  }
}

// Q^T M Q = I and K Q = M Q Lambda to 1e-12 of the norms
static void check_eig(int n, double h, int own, int other) {
  SmdAxis A;
  const int rc = smd_axis_build(n, h, own, other, A);
  if (n == 1 && other == 3) { expect(rc == SMD_RANK, "one cell, both ends masked: rank-deficient", n, other); return; }
  expect(rc == SMD_OK, "axis build", n, own * 4 + other);
  if (rc != SMD_OK) return;
  std::vector<double> N, G, m, K, M;
  smd_1d_tables(n, h, N, G, m);
  smd_factor(n, G, m, own & 1, own & 2, K);
  smd_factor(n, N, m, other & 1, other & 2, M);
  const int np = n + 1;
  auto amax = [](const std::vector<double> &v) { double a = 0; for (double x : v) a = std::max(a, std::fabs(x)); return a; };
  const double kq = amax(K), mq = amax(M), qq = amax(A.Q), lq = amax(A.lam);
  std::vector<double> MQ(size_t(np) * np, 0.0), KQ(size_t(np) * np, 0.0);
  for (int i = 0; i < np; ++i)
    for (int k = 0; k < np; ++k) {
      const double mk = M[size_t(i) * np + k], kk = K[size_t(i) * np + k];
      if (mk == 0.0 && kk == 0.0) continue;
      for (int j = 0; j < np; ++j) {
        MQ[size_t(i) * np + j] += mk * A.Q[size_t(k) * np + j];
        KQ[size_t(i) * np + j] += kk * A.Q[size_t(k) * np + j];
      }
    }
  double e_orth = 0, e_eig = 0;
  for (int i = 0; i < np; ++i)
    for (int j = 0; j < np; ++j) {
      double s = 0;
      for (int k = 0; k < np; ++k) s += A.Q[size_t(k) * np + i] * MQ[size_t(k) * np + j];
      e_orth = std::max(e_orth, std::fabs(s - (i == j ? 1.0 : 0.0)));
      e_eig = std::max(e_eig, std::fabs(KQ[size_t(i) * np + j] - MQ[size_t(i) * np + j] * A.lam[j]));
    }
  const double scale = kq * qq + mq * qq * lq;
  if (!(e_orth <= 1e-12) || !(e_eig <= 1e-12 * scale)) {
    printf("FAIL eigen-solve n %d masks %d %d: |Q^T M Q - I| %.2e, |K Q - M Q L| %.2e of %.2e\n", n, own, other, e_orth, e_eig, scale);
    ++fails;
  }
  if (n == 128 || n == 40) printf("n %d masks %d %d: |Q^T M Q - I| %.2e, |K Q - M Q L| / scale %.2e, lambda in [%.3e, %.3e]\n", n, own, other, e_orth, e_eig / scale,
                                  *std::min_element(A.lam.begin(), A.lam.end()), lq);
}

// velocity lattice of a box with whole-face constraints: comp[face] = component bits constrained on face 2 a + s
static void faces_to_flags(int dim, const int nu[3], const std::vector<int32_t> &nol, const int comp[6], std::vector<uint8_t> &is_c) {
  int64_t total = 1;
  for (int d = 0; d < dim; ++d) total *= nu[d];
  is_c.assign(size_t(total) * dim, 0);
  for (int64_t p = 0; p < total; ++p) {
    const int64_t i[3] = {p % nu[0], (p / nu[0]) % nu[1], p / (int64_t(nu[0]) * nu[1])};
    for (int a = 0; a < dim; ++a)
      for (int s = 0; s < 2; ++s)
        if (i[a] == (s ? nu[a] - 1 : 0))
          for (int c = 0; c < dim; ++c)
            if (comp[2 * a + s] & (1 << c)) is_c[size_t(nol[p]) * dim + c] = 1;
  }
}

static void check_masks() {
  for (int dim = 2; dim <= 3; ++dim)
    for (int perm = 0; perm < 2; ++perm) {
      const int nu[3] = {9, 7, dim == 3 ? 5 : 1};
      const int64_t total = int64_t(nu[0]) * nu[1] * nu[2];
      std::vector<int32_t> nol(size_t(total), 0);
      std::iota(nol.begin(), nol.end(), 0);
      if (perm) { std::mt19937 g(7); std::shuffle(nol.begin(), nol.end(), g); }
      const int all = (1 << dim) - 1;
      int face[3][3][2], mask[3][3];
      int64_t count[3];
      std::vector<uint8_t> is_c;
      // nothing constrained
      smd_masks_scan(dim, nu, nol.data(), nullptr, face, count);
      expect(smd_masks_decide(dim, nu, face, count, mask) && mask[0][0] == 0 && mask[1][1] == 0, "no constraints", dim);
      // the channel: inflow and walls, outflow free
      const int channel[6] = {all, 0, all, all, all, all};
      faces_to_flags(dim, nu, nol, channel, is_c);
      smd_masks_scan(dim, nu, nol.data(), is_c.data(), face, count);
      bool ok = smd_masks_decide(dim, nu, face, count, mask);
      for (int c = 0; c < dim; ++c) ok = ok && mask[c][0] == 1 && mask[c][1] == 3 && (dim == 2 || mask[c][2] == 3);
      expect(ok, "channel masks", dim, perm);
      // one stray interior node of one component: the count gives it away
      std::vector<uint8_t> stray = is_c;
      stray[size_t(nol[4 + nu[0] * 3 + (dim == 3 ? int64_t(nu[0]) * nu[1] * 2 : 0)]) * dim + 1] = 1;
      smd_masks_scan(dim, nu, nol.data(), stray.data(), face, count);
      expect(!smd_masks_decide(dim, nu, face, count, mask), "a stray interior constrained dof must refuse", dim, perm);
      // one face node missing
      std::vector<uint8_t> hole = is_c;
      hole[size_t(nol[0 + nu[0] * 2]) * dim + 0] = 0;
      smd_masks_scan(dim, nu, nol.data(), hole.data(), face, count);
      expect(!smd_masks_decide(dim, nu, face, count, mask), "a face with a free node must refuse", dim, perm);
      // slip faces: the normal component only
      const int slip[6] = {all, 0, 2, 2, dim == 3 ? 4 : 0, dim == 3 ? 4 : 0};
      faces_to_flags(dim, nu, nol, slip, is_c);
      smd_masks_scan(dim, nu, nol.data(), is_c.data(), face, count);
      ok = smd_masks_decide(dim, nu, face, count, mask);
      ok = ok && mask[1][1] == 3 && mask[0][1] == 0 && mask[0][0] == 1 && mask[1][0] == 1;
      expect(ok, "slip faces", dim, perm);
      // a face that constrains one tangential component only: a product set, but in 3D the mass-like factors of that axis differ
      const int tang[6] = {all, 0, 1, 0, 0, 0};
      faces_to_flags(dim, nu, nol, tang, is_c);
      smd_masks_scan(dim, nu, nol.data(), is_c.data(), face, count);
      expect(smd_masks_decide(dim, nu, face, count, mask) == (dim == 2), "tangential-only face", dim, perm);
      // 30 % random dofs
      std::mt19937 g(11);
      std::vector<uint8_t> rnd(size_t(total) * dim, 0);
      for (auto &v : rnd) v = g() % 10 < 3;
      smd_masks_scan(dim, nu, nol.data(), rnd.data(), face, count);
      expect(!smd_masks_decide(dim, nu, face, count, mask), "random constrained dofs must refuse", dim, perm);
    }
}

int main() {
  for (int n = 1; n <= 5; ++n) {
    check_tables(n, 0.37);
    check_tables(n, 2.5);
  }
  for (int n = 1; n <= 40; ++n)
    for (int masks = 0; masks < 16; ++masks) check_eig(n, n % 2 ? 0.0125 : 0.4, masks >> 2, masks & 3);
  for (int masks = 0; masks < 16; ++masks) check_eig(128, 2.0 / 128, masks >> 2, masks & 3);
  // refusals: over the cap, a singular sum (every axis with both ends constrained for its own component), an empty axis
  SmdAxis A, B, Cc;
  expect(smd_axis_build(kSmdMaxAxis, 0.01, 0, 0, A) == SMD_CAP && A.np == 0, "over the cap");
  expect(smd_axis_build(0, 0.01, 0, 0, A) == SMD_CAP, "no cell");
  expect(smd_axis_build(6, 0.3, 3, 3, A) == SMD_OK && smd_axis_build(5, 0.2, 3, 3, B) == SMD_OK && smd_axis_build(4, 0.1, 3, 3, Cc) == SMD_OK, "enclosed axes build");
  {
    const SmdAxis *ax[3] = {&A, &B, &Cc};
    double lo = 0, hi = 0;
    expect(smd_lambda_check(3, ax, &lo, &hi) == SMD_SINGULAR, "the enclosed flow must be refused");
    expect(std::fabs(lo) <= 1e-12 * hi, "its smallest Lambda is zero to rounding");
    SmdAxis O;
    expect(smd_axis_build(6, 0.3, 1, 1, O) == SMD_OK, "open axis");
    const SmdAxis *ax2[3] = {&O, &B, &Cc};
    expect(smd_lambda_check(3, ax2, &lo, &hi) == SMD_OK && lo > 0, "one open end makes the sum definite");
    expect(O.same_key(6, 0.3, 1, 1) && !O.same_key(6, 0.3, 1, 3) && !O.same_key(5, 0.3, 1, 1) && !O.same_key(6, 0.31, 1, 1), "axis key");
  }
  check_masks();
  printf("ok (%d failures)\n", fails);
  return fails ? 1 : 0;
}
