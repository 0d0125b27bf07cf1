// The weight formula of the lattice velocity transfers (csrc/mg_lattice.hpp) on the host: for 1..9 coarse cells per axis the 1D prolongation
// against the quadratic Lagrange polynomials through the coarse points, evaluated in long double (the values are dyadic: compared exactly), the 1D
// restriction as the exact transpose, a kept axis as the identity, and on 3 x 2 x 2 -> 6 x 4 x 4 cells the tensor product of the term slots
// against a brute-force table of the products.
#include <cstdio>
#include <vector>
#include "mg_lattice.hpp"
using namespace ifem;

// l_m(x), m = 0..2, the quadratic Lagrange polynomials on the points 0, 1/2, 1
static long double lagrange(int m, long double x) {
  const long double p[3] = {0.0L, 0.5L, 1.0L};
  long double v = 1;
  for (int k = 0; k < 3; ++k)
    if (k != m) v *= (x - p[k]) / (p[m] - p[k]);
  return v;
}

// dense 1D prolongation [n_f][n_c] of a halved axis with cells_c coarse cells, from the polynomials
static std::vector<long double> dense_1d(int cells_c) {
  const int n_c = 2 * cells_c + 1, n_f = 4 * cells_c + 1;
  std::vector<long double> P(size_t(n_f) * n_c, 0.0L);
  for (int i = 0; i < n_f; ++i) {
    int K = i / 4;
    if (K > cells_c - 1) K = cells_c - 1;
    const long double x = (long double)(i - 4 * K) / 4.0L;
    for (int m = 0; m < 3; ++m) P[size_t(i) * n_c + 2 * K + m] = lagrange(m, x);
  }
  return P;
}

int main() {
  int fails = 0;
  for (int cells_c = 1; cells_c <= 9; ++cells_c) {
    const int n_c = 2 * cells_c + 1, n_f = 4 * cells_c + 1;
    const std::vector<long double> P = dense_1d(cells_c);
    // prolongation rows: every slot that holds a term is the polynomial's value, every non-zero of the dense row is some slot, no column twice
    for (int i = 0; i < n_f; ++i) {
      std::vector<int> seen(n_c, 0);
      int terms = 0;
      for (int k = 0; k < mgl_prolong_slots(true); ++k) {
        int j = -1; double w = 0;
        if (!mgl_prolong_term(true, n_c, i, k, j, w)) continue;
        ++terms;
        if (j < 0 || j >= n_c || seen[j]++ || w == 0.0 || (long double)w != P[size_t(i) * n_c + j]) { printf("FAIL P cells %d row %d slot %d: column %d weight %g\n", cells_c, i, k, j, w); ++fails; }
      }
      int nz = 0;
      for (int j = 0; j < n_c; ++j) nz += P[size_t(i) * n_c + j] != 0.0L;
      if (terms != nz || terms != mgl_prolong_count(true, n_c, i)) { printf("FAIL P cells %d row %d: %d terms, %d non-zeros\n", cells_c, i, terms, nz); ++fails; }
    }
    // restriction rows: the transpose, entry for entry
    for (int j = 0; j < n_c; ++j) {
      std::vector<int> seen(n_f, 0);
      int terms = 0;
      for (int k = 0; k < mgl_restrict_slots(true); ++k) {
        int i = -1; double w = 0;
        if (!mgl_restrict_term(true, n_f, j, k, i, w)) continue;
        ++terms;
        if (i < 0 || i >= n_f || seen[i]++ || (long double)w != P[size_t(i) * n_c + j]) { printf("FAIL R cells %d row %d slot %d: column %d weight %g\n", cells_c, j, k, i, w); ++fails; }
      }
      int nz = 0;
      for (int i = 0; i < n_f; ++i) nz += P[size_t(i) * n_c + j] != 0.0L;
      if (terms != nz || terms != mgl_restrict_count(true, n_f, j)) { printf("FAIL R cells %d row %d: %d terms, %d non-zeros\n", cells_c, j, terms, nz); ++fails; }
    }
    // a kept axis: one term of weight 1 at the same index, both ways; the injection partner
    for (int i = 0; i < n_c; ++i) {
      int j = -1, i2 = -1; double w = 0, w2 = 0;
      const bool a = mgl_prolong_term(false, n_c, i, 0, j, w), b = mgl_restrict_term(false, n_c, i, 0, i2, w2);
      if (!a || !b || j != i || i2 != i || w != 1.0 || w2 != 1.0 || mgl_prolong_slots(false) != 1 || mgl_restrict_slots(false) != 1 ||
          mgl_prolong_count(false, n_c, i) != 1 || mgl_restrict_count(false, n_c, i) != 1 || mgl_inject_index(false, i) != i || mgl_inject_index(true, i) != 2 * i) {
        printf("FAIL kept axis n %d index %d\n", n_c, i); ++fails;
      }
      // the fine point a coarse point coincides with interpolates that point alone
      int jj = -1; double ww = 0; int cnt = 0;
      for (int k = 0; k < 3; ++k) { int q; double v; if (mgl_prolong_term(true, n_c, 2 * i, k, q, v)) { ++cnt; jj = q; ww = v; } }
      if (cnt != 1 || jj != i || ww != 1.0) { printf("FAIL coincident point cells %d index %d\n", cells_c, i); ++fails; }
    }
  }
  // 3 x 2 x 2 -> 6 x 4 x 4 cells: rows of P and R from the nested slots against the brute-force products of the dense 1D tables
  {
    const int cc[3] = {3, 2, 2};
    int n_c[3], n_f[3];
    std::vector<long double> P1[3];
    for (int a = 0; a < 3; ++a) { n_c[a] = 2 * cc[a] + 1; n_f[a] = 4 * cc[a] + 1; P1[a] = dense_1d(cc[a]); }
    const size_t NF = size_t(n_f[0]) * n_f[1] * n_f[2], NC = size_t(n_c[0]) * n_c[1] * n_c[2];
    std::vector<long double> T(NF * NC), Pm(NF * NC, 0.0L), Rm(NF * NC, 0.0L);
    for (int iz = 0; iz < n_f[2]; ++iz) for (int iy = 0; iy < n_f[1]; ++iy) for (int ix = 0; ix < n_f[0]; ++ix)
      for (int jz = 0; jz < n_c[2]; ++jz) for (int jy = 0; jy < n_c[1]; ++jy) for (int jx = 0; jx < n_c[0]; ++jx)
        T[(ix + size_t(n_f[0]) * (iy + size_t(n_f[1]) * iz)) * NC + (jx + size_t(n_c[0]) * (jy + size_t(n_c[1]) * jz))] =
            P1[2][size_t(iz) * n_c[2] + jz] * P1[1][size_t(iy) * n_c[1] + jy] * P1[0][size_t(ix) * n_c[0] + jx];
    size_t nP = 0, nR = 0, nT = 0;
    for (int iz = 0; iz < n_f[2]; ++iz) for (int iy = 0; iy < n_f[1]; ++iy) for (int ix = 0; ix < n_f[0]; ++ix)
      for (int kz = 0; kz < 3; ++kz) for (int ky = 0; ky < 3; ++ky) for (int kx = 0; kx < 3; ++kx) {
        int jx, jy, jz; double wx, wy, wz;
        if (!mgl_prolong_term(true, n_c[2], iz, kz, jz, wz) || !mgl_prolong_term(true, n_c[1], iy, ky, jy, wy) || !mgl_prolong_term(true, n_c[0], ix, kx, jx, wx)) continue;
        Pm[(ix + size_t(n_f[0]) * (iy + size_t(n_f[1]) * iz)) * NC + (jx + size_t(n_c[0]) * (jy + size_t(n_c[1]) * jz))] += (long double)(wz * wy * wx);
        ++nP;
      }
    for (int jz = 0; jz < n_c[2]; ++jz) for (int jy = 0; jy < n_c[1]; ++jy) for (int jx = 0; jx < n_c[0]; ++jx)
      for (int kz = 0; kz < 5; ++kz) for (int ky = 0; ky < 5; ++ky) for (int kx = 0; kx < 5; ++kx) {
        int ix, iy, iz; double wx, wy, wz;
        if (!mgl_restrict_term(true, n_f[2], jz, kz, iz, wz) || !mgl_restrict_term(true, n_f[1], jy, ky, iy, wy) || !mgl_restrict_term(true, n_f[0], jx, kx, ix, wx)) continue;
        Rm[(ix + size_t(n_f[0]) * (iy + size_t(n_f[1]) * iz)) * NC + (jx + size_t(n_c[0]) * (jy + size_t(n_c[1]) * jz))] += (long double)(wz * wy * wx);
        ++nR;
      }
    size_t bad = 0;
    for (size_t e = 0; e < NF * NC; ++e) { nT += T[e] != 0.0L; bad += (Pm[e] != T[e]) + (Rm[e] != T[e]); }
    if (bad || nP != nT || nR != nT) { printf("FAIL tensor product: %zu entries differ, %zu / %zu terms against %zu non-zeros\n", bad, nP, nR, nT); ++fails; }
    else printf("tensor product 3 x 2 x 2 -> 6 x 4 x 4: %zu non-zeros, P and R rows exact\n", nT);
  }
  printf("ok (%d failures)\n", fails);
  return fails ? 1 : 0;
}
