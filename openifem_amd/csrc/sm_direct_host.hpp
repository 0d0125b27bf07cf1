// sm_direct_host.hpp -- host side of the fast-diagonalisation solve of S_m on a uniform Q2/Q1 box level (sm_direct.hip): the 1D factors of
// the Kronecker sum, the constraint masks, and the dense generalised symmetric eigen-solver.  Plain C++, no device call, no LAPACK.
#pragma once
#include <cstdint>
#include <vector>

namespace ifem {

constexpr int kSmdMaxAxis = 513; // pressure nodes per axis: Q_a <= 2.1 MB and an O(n^3) host solve; longer axes keep CG

// 1D tables of an axis of n cells of edge h, integrated with the 3-point Gauss rule as the assembly does: N [n + 1][2 n + 1] = int psi_i phi_j
// (Q1 x Q2 mass coupling), G the same with phi_j', m [2 n + 1] the diagonal of the Q2 mass matrix
void smd_1d_tables(int n, double h, std::vector<double> &N, std::vector<double> &G, std::vector<double> &m);

// F = X diag(d / m) X^T, [n + 1][n + 1], d = 1 except d_0 = 0 (drop_lo) and d_2n = 0 (drop_hi)
void smd_factor(int n, const std::vector<double> &X, const std::vector<double> &m, bool drop_lo, bool drop_hi, std::vector<double> &F);

// K q = lambda M q for symmetric K and symmetric positive definite M of order np (row-major): Cholesky of M, reduction of K, cyclic Jacobi,
// back-transformation.  Q [np][np], column j the eigenvector of lam[j], Q^T M Q = I.  Returns 0, or 1 when the Cholesky factorisation meets
// a pivot <= 1e-12 of the largest diagonal entry (M rank-deficient or indefinite) or a number that is not finite
int smd_gen_eig(int np, const std::vector<double> &K, const std::vector<double> &M, std::vector<double> &Q, std::vector<double> &lam);

// The factors of one axis: K = G diag(d_own / m) G^T with the mask of the axis' own velocity component, M~ = N diag(d_other / m) N^T with the
// mask of the other components; masks as bits (1: first node dropped, 2: last node dropped)
struct SmdAxis {
  int n_cells = 0, np = 0, mask_own = 0, mask_other = 0;
  double h = 0;
  std::vector<double> Q, lam;
  bool same_key(int n, double hh, int own, int other) const { return np > 0 && n == n_cells && hh == h && own == mask_own && other == mask_other; }
};
enum { SMD_OK = 0, SMD_CAP = 1, SMD_RANK = 2, SMD_SINGULAR = 3, SMD_MASKS = 4 };
int smd_axis_build(int n_cells, double h, int mask_own, int mask_other, SmdAxis &A); // SMD_OK, SMD_CAP or SMD_RANK
// min / max of Lambda = sum_a lambda_a over the lattice; SMD_SINGULAR when min <= 1e-12 max (the enclosed flow) or one of them is not finite
int smd_lambda_check(int dim, const SmdAxis *const axes[3], double *lmin, double *lmax);

// The constraint masks.  face[c][a][s]: velocity component c is constrained at the centre node of the face s (0 first, 1 last) of axis a;
// count[c]: constrained dofs of component c.  smd_masks_scan reads both from the velocity lattice (nu nodes per axis, point -> node) and the
// flags is_c [node * dim + c] (nullptr: nothing is constrained) -- the host form of sm_direct.hip::k_smd_masks.  smd_masks_decide: the
// unconstrained dofs of every component are the product of ranges the faces imply (the counts agree) and the mass-like factors of every
// axis coincide (in 3D the two components across an axis have the same mask there); mask[c][a] as the bits above
void smd_masks_scan(int dim, const int nu[3], const int32_t *node_of_lattice, const uint8_t *is_c, int face[3][3][2], int64_t count[3]);
bool smd_masks_decide(int dim, const int nu[3], const int face[3][3][2], const int64_t count[3], int mask[3][3]);
inline int64_t smd_face_centre(int dim, const int nu[3], int a, int s) { // lattice point of the centre node of a face (interior to it)
  int64_t p = 0, mul = 1;
  for (int d = 0; d < dim; ++d) {
    p += int64_t(d == a ? (s ? nu[d] - 1 : 0) : (nu[d] - 1) / 2) * mul;
    mul *= nu[d];
  }
  return p;
}

} // namespace ifem
