// sm_direct_host.cpp -- host side of the fast-diagonalisation solve of S_m (sm_direct.hip): plain C++, no device call.
#include <algorithm>
#include <cmath>
#include "sm_direct_host.hpp"

namespace ifem {

void smd_1d_tables(int n, double h, std::vector<double> &N, std::vector<double> &G, std::vector<double> &m) {
  const int np = n + 1, nu = 2 * n + 1;
  N.assign(size_t(np) * nu, 0.0);
  G.assign(size_t(np) * nu, 0.0);
  m.assign(size_t(nu), 0.0);
  const double r = std::sqrt(0.6);
  const double qt[3] = {0.5 * (1.0 - r), 0.5, 0.5 * (1.0 + r)}, qw[3] = {5.0 / 18.0, 8.0 / 18.0, 5.0 / 18.0};
  double nloc[2][3] = {{0, 0, 0}, {0, 0, 0}}, gloc[2][3] = {{0, 0, 0}, {0, 0, 0}}, mloc[3] = {0, 0, 0};
  for (int q = 0; q < 3; ++q) {
    const double t = qt[q], w = qw[q];
    const double psi[2] = {1.0 - t, t};
    const double phi[3] = {(1.0 - t) * (1.0 - 2.0 * t), 4.0 * t * (1.0 - t), t * (2.0 * t - 1.0)};
    const double dphi[3] = {4.0 * t - 3.0, 4.0 - 8.0 * t, 4.0 * t - 1.0}; // d/dt; the 1/h of d/dx cancels the h of dx
    for (int j = 0; j < 3; ++j) {
      for (int i = 0; i < 2; ++i) {
        nloc[i][j] += w * h * psi[i] * phi[j];
        gloc[i][j] += w * psi[i] * dphi[j];
      }
      mloc[j] += w * h * phi[j] * phi[j];
    }
  }
  for (int c = 0; c < n; ++c)
    for (int j = 0; j < 3; ++j) {
      for (int i = 0; i < 2; ++i) {
        N[size_t(c + i) * nu + 2 * c + j] += nloc[i][j];
        G[size_t(c + i) * nu + 2 * c + j] += gloc[i][j];
      }
      m[2 * c + j] += mloc[j];
    }
}

void smd_factor(int n, const std::vector<double> &X, const std::vector<double> &m, bool drop_lo, bool drop_hi, std::vector<double> &F) {
  const int np = n + 1, nu = 2 * n + 1;
  F.assign(size_t(np) * np, 0.0);
  // row i of X touches the columns 2 i - 2 .. 2 i + 2: rows up to two apart share a column
  for (int i = 0; i < np; ++i)
    for (int k = std::max(0, i - 2); k <= std::min(np - 1, i + 2); ++k) {
      double s = 0;
      for (int j = std::max(0, 2 * std::max(i, k) - 2); j <= std::min(nu - 1, 2 * std::min(i, k) + 2); ++j) {
        if ((j == 0 && drop_lo) || (j == nu - 1 && drop_hi)) continue;
        s += X[size_t(i) * nu + j] * X[size_t(k) * nu + j] / m[j];
      }
      F[size_t(i) * np + k] = s;
    }
}

// eigenvalues w and eigenvectors (ROWS of Vt) of the symmetric A (order n, destroyed) by cyclic Jacobi rotations
static void jacobi_eig(int n, std::vector<double> &A, std::vector<double> &Vt, std::vector<double> &w) {
  Vt.assign(size_t(n) * n, 0.0);
  for (int i = 0; i < n; ++i) Vt[size_t(i) * n + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) off += A[size_t(p) * n + q] * A[size_t(p) * n + q];
    if (off == 0.0) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[size_t(p) * n + q];
        if (apq == 0.0) continue;
        const double app = A[size_t(p) * n + p], aqq = A[size_t(q) * n + q];
        const double g = 100.0 * std::fabs(apq);
        if (sweep > 3 && std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
          A[size_t(p) * n + q] = A[size_t(q) * n + p] = 0.0;
          continue;
        }
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        double *rp = &A[size_t(p) * n], *rq = &A[size_t(q) * n];
        for (int k = 0; k < n; ++k) { // rows p and q of J^T A
          const double x = rp[k], y = rq[k];
          rp[k] = c * x - s * y;
          rq[k] = s * x + c * y;
        }
        for (int k = 0; k < n; ++k) { // columns p and q of (J^T A) J
          double *row = &A[size_t(k) * n];
          const double x = row[p], y = row[q];
          row[p] = c * x - s * y;
          row[q] = s * x + c * y;
        }
        rp[q] = rq[p] = 0.0;
        double *vp = &Vt[size_t(p) * n], *vq = &Vt[size_t(q) * n];
        for (int k = 0; k < n; ++k) {
          const double x = vp[k], y = vq[k];
          vp[k] = c * x - s * y;
          vq[k] = s * x + c * y;
        }
      }
  }
  w.resize(size_t(n));
  for (int i = 0; i < n; ++i) w[i] = A[size_t(i) * n + i];
}

int smd_gen_eig(int np, const std::vector<double> &K, const std::vector<double> &M, std::vector<double> &Q, std::vector<double> &lam) {
  const size_t n = size_t(np);
  if (np <= 0 || K.size() != n * n || M.size() != n * n) return 1;
  double dmax = 0;
  for (size_t i = 0; i < n; ++i) dmax = std::max(dmax, M[i * n + i]);
  if (!(dmax > 0) || !std::isfinite(dmax)) return 1;
  // M = L L^T
  std::vector<double> L(n * n, 0.0);
  for (size_t j = 0; j < n; ++j) {
    double d = M[j * n + j];
    for (size_t k = 0; k < j; ++k) d -= L[j * n + k] * L[j * n + k];
    if (!(d > 1e-12 * dmax) || !std::isfinite(d)) return 1;
    const double ljj = std::sqrt(d);
    L[j * n + j] = ljj;
    for (size_t i = j + 1; i < n; ++i) {
      double s = M[i * n + j];
      for (size_t k = 0; k < j; ++k) s -= L[i * n + k] * L[j * n + k];
      L[i * n + j] = s / ljj;
    }
  }
  // C = L^-1 K L^-T: X = L^-1 K (forward substitution on every column), then C^T = L^-1 X^T
  std::vector<double> X(K), C(n * n, 0.0);
  for (size_t i = 0; i < n; ++i) {
    for (size_t k = 0; k < i; ++k) {
      const double l = L[i * n + k];
      if (l != 0.0)
        for (size_t j = 0; j < n; ++j) X[i * n + j] -= l * X[k * n + j];
    }
    const double r = 1.0 / L[i * n + i];
    for (size_t j = 0; j < n; ++j) X[i * n + j] *= r;
  }
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) C[i * n + j] = X[j * n + i];
  for (size_t i = 0; i < n; ++i) {
    for (size_t k = 0; k < i; ++k) {
      const double l = L[i * n + k];
      if (l != 0.0)
        for (size_t j = 0; j < n; ++j) C[i * n + j] -= l * C[k * n + j];
    }
    const double r = 1.0 / L[i * n + i];
    for (size_t j = 0; j < n; ++j) C[i * n + j] *= r;
  }
  for (size_t i = 0; i < n; ++i)
    for (size_t j = i + 1; j < n; ++j) C[i * n + j] = C[j * n + i] = 0.5 * (C[i * n + j] + C[j * n + i]);
  std::vector<double> Zt;
  jacobi_eig(np, C, Zt, lam);
  // Q = L^-T Z: column j of Q from row j of Zt by back substitution
  Q.assign(n * n, 0.0);
  std::vector<double> q(n);
  for (size_t j = 0; j < n; ++j) {
    for (size_t ii = n; ii-- > 0;) {
      double s = Zt[j * n + ii];
      for (size_t k = ii + 1; k < n; ++k) s -= L[k * n + ii] * q[k];
      q[ii] = s / L[ii * n + ii];
    }
    for (size_t i = 0; i < n; ++i) {
      if (!std::isfinite(q[i])) return 1;
      Q[i * n + j] = q[i];
    }
    if (!std::isfinite(lam[j])) return 1;
  }
  return 0;
}

int smd_axis_build(int n_cells, double h, int mask_own, int mask_other, SmdAxis &A) {
  A.np = 0;
  if (n_cells < 1 || n_cells + 1 > kSmdMaxAxis || !(h > 0)) return SMD_CAP;
  std::vector<double> N, G, m, K, M;
  smd_1d_tables(n_cells, h, N, G, m);
  smd_factor(n_cells, G, m, mask_own & 1, mask_own & 2, K);
  smd_factor(n_cells, N, m, mask_other & 1, mask_other & 2, M);
  if (smd_gen_eig(n_cells + 1, K, M, A.Q, A.lam)) return SMD_RANK;
  A.n_cells = n_cells; A.np = n_cells + 1; A.h = h; A.mask_own = mask_own; A.mask_other = mask_other;
  return SMD_OK;
}

int smd_lambda_check(int dim, const SmdAxis *const axes[3], double *lmin, double *lmax) {
  double lo = 0, hi = 0;
  for (int a = 0; a < dim; ++a) {
    const std::vector<double> &l = axes[a]->lam;
    if (l.empty()) return SMD_SINGULAR;
    lo += *std::min_element(l.begin(), l.end());
    hi += *std::max_element(l.begin(), l.end());
  }
  if (lmin) *lmin = lo;
  if (lmax) *lmax = hi;
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo > 1e-12 * hi)) return SMD_SINGULAR;
  return SMD_OK;
}

void smd_masks_scan(int dim, const int nu[3], const int32_t *node_of_lattice, const uint8_t *is_c, int face[3][3][2], int64_t count[3]) {
  int64_t total = 1;
  for (int d = 0; d < dim; ++d) total *= nu[d];
  for (int c = 0; c < 3; ++c) {
    count[c] = 0;
    for (int a = 0; a < 3; ++a) face[c][a][0] = face[c][a][1] = 0;
  }
  if (!is_c) return;
  for (int c = 0; c < dim; ++c) {
    for (int64_t nd = 0; nd < total; ++nd) count[c] += is_c[nd * dim + c] ? 1 : 0;
    for (int a = 0; a < dim; ++a)
      for (int s = 0; s < 2; ++s) face[c][a][s] = is_c[int64_t(node_of_lattice[smd_face_centre(dim, nu, a, s)]) * dim + c] ? 1 : 0;
  }
}

bool smd_masks_decide(int dim, const int nu[3], const int face[3][3][2], const int64_t count[3], int mask[3][3]) {
  int64_t total = 1;
  for (int d = 0; d < dim; ++d) total *= nu[d];
  for (int c = 0; c < 3; ++c)
    for (int a = 0; a < 3; ++a) mask[c][a] = 0;
  for (int c = 0; c < dim; ++c) {
    int64_t free_dofs = 1;
    for (int a = 0; a < dim; ++a) {
      mask[c][a] = (face[c][a][0] ? 1 : 0) | (face[c][a][1] ? 2 : 0);
      free_dofs *= std::max(0, nu[a] - (face[c][a][0] ? 1 : 0) - (face[c][a][1] ? 1 : 0));
    }
    if (count[c] != total - free_dofs) return false; // the constrained dofs are not whole faces
  }
  for (int a = 0; a < dim; ++a) { // the mass-like factors of axis a: the components other than a
    int first = -1;
    for (int c = 0; c < dim; ++c) {
      if (c == a) continue;
      if (first < 0) first = mask[c][a];
      else if (mask[c][a] != first) return false; // a face that constrains one tangential component only
    }
  }
  return true;
}

} // namespace ifem
