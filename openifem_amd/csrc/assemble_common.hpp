// assemble_common.hpp -- argument block and small helpers shared by the InsIM assembly driver (assemble.hip) and its cell
// kernels (assemble3.hip: 3D Q2/Q1 on the FP64 matrix cores; assemble2.hip: every other (dim, kv), quadrature-point-outer with
// register accumulators); Geo, the small inverses, the cell geometry of the d-linear map, the Neumann face term, pick and grid_for also
// serve the one-wavefront-per-cell kernels of assemble_scns.hip, sa.hip and scnsex.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "ctx.hpp"

namespace ifem {

template <int DIM, int KV>
struct Geo {
  static constexpr int N1 = KV + 1;
  static constexpr int NU = (DIM == 2) ? N1 * N1 : N1 * N1 * N1;
  static constexpr int NP = (DIM == 2) ? 4 : 8;
  static constexpr int NQ = NU;
  static constexpr int ND = NU * DIM + NP;
};

struct AsmArgs {
  int64_t n_cells;
  const int32_t *order; // cells of the colour being assembled (nullptr: all cells, atomics)
  int64_t first, count; // range of `order` handled by this launch
  int64_t nUo, nUl, nPo;
  const FeTables *fe;
  const double *vcoords;
  const int32_t *cell_unodes, *cell_pnodes, *cell_face_bid, *indicator;
  const uint16_t *posUU, *posUP, *posPU, *posPP;
  const uint16_t *scat3; const uint8_t *hdr3; const Tabs3 *tabs3; // 3D Q2/Q1 cell kernel only (assemble3.hip)
  const int64_t *rp_uu, *rp_bt, *rp_b, *rp_mp;
  double *v_uu, *v_bt, *v_b, *v_mp, *diagMu, *rhs;
  double *v_s; // scalar velocity operator (one value per A_uu block) or nullptr
  const uint8_t *is_c;
  const double *cval;
  const double *eval, *present, *fsi_acc;
  double mu, rho, gamma, inv_dt;
  double g[3];
  int n_neumann;
  int neumann_id[8];
  double neumann_p[8];
  int use_inhom; // constraint set carries non-zero inhomogeneities
  int imex;     // InsIMEX (mpi_insimex.cpp:248-262): the matrix drops the two convective terms (explicit convection)
  int rhs_only; // InsIMEX with assemble_system = false: only the right-hand side is integrated and scattered (:343-346)
  int xcd_swizzle; // contiguous cell ranges per XCD (IFEM_XCD=0 switches it off)
  int skip_geo;   // B, B^T, M_p and diag(M_u) of the previous assembly are still valid (same mesh, same constraint set):
                  // integrate them only where a constrained dof needs their entries for the right-hand side
  int skip_uu;    // geometry-only assembly (multigrid levels): the velocity-velocity block is neither integrated nor scattered
  int debug_skip; // measurement builds only (-DIFEM_ASM_PROBES, ifem_tuning::asm_skip): 1 = no A_uu scatter, 2 = no contraction either
  double *pd;     // 3D Q2/Q1 cell kernel, optional output: the point data of the A_uu contraction, [cell][27 points][rwu 3 | gqs 9], for the
                  // row-owner kernel (assemble_rows.hip); nullptr: not written
  double *fe_out; // with pd: the cell's local right-hand side [cell][96] (velocity [c][a], pressure at 81 + b) goes there instead of being added to
                  // rhs with atomics -- the row owners sum it in a fixed order
};

template <int DIM, typename R = double>
__device__ inline R inv_small(const R *J, R *Ji) {
  if constexpr (DIM == 2) {
    const R det = J[0] * J[3] - J[1] * J[2];
    const R r = R(1) / det;
    Ji[0] = J[3] * r; Ji[1] = -J[1] * r; Ji[2] = -J[2] * r; Ji[3] = J[0] * r;
    return det;
  } else {
    const R c00 = J[4] * J[8] - J[5] * J[7], c01 = J[5] * J[6] - J[3] * J[8], c02 = J[3] * J[7] - J[4] * J[6];
    const R det = J[0] * c00 + J[1] * c01 + J[2] * c02;
    const R r = R(1) / det;
    Ji[0] = c00 * r; Ji[3] = c01 * r; Ji[6] = c02 * r;
    Ji[1] = (J[2] * J[7] - J[1] * J[8]) * r; Ji[4] = (J[0] * J[8] - J[2] * J[6]) * r; Ji[7] = (J[1] * J[6] - J[0] * J[7]) * r;
    Ji[2] = (J[1] * J[5] - J[2] * J[4]) * r; Ji[5] = (J[2] * J[3] - J[0] * J[5]) * r; Ji[8] = (J[0] * J[4] - J[1] * J[3]) * r;
    return det;
  }
}

// ---- cell geometry under the d-linear map of the 2^DIM vertices, for the one-wavefront-per-cell kernels of sa.hip, scnsex.hip and
// assemble_scns.hip (assemble2.hip / assemble3.hip form J from tensor factors and keep their own)
// J = sum_v X_v (x) dpsi_v at quadrature point q of the table dpsi ([point][2^DIM][DIM]; q = 0: dpsi is the point's own rows), Ji = J^-1;
// returns det J.  Keep it forced inline, and pass table and index from a cell kernel's quadrature loop: the loops of the callers sit at the
// unroller's thresholds, and with either changed some 3D kernels spill or take more registers (profiles/scalar_node_refactor.txt)
template <int DIM>
__device__ __forceinline__ double cell_jacobian(const double *X, const double *dpsi, double *Ji, int q = 0) {
  constexpr int NP = 1 << DIM;
  double J[DIM * DIM];
  for (int i = 0; i < DIM * DIM; ++i) J[i] = 0;
  for (int v = 0; v < NP; ++v)
    for (int d = 0; d < DIM; ++d)
      for (int e = 0; e < DIM; ++e) J[d * DIM + e] += X[v * DIM + d] * dpsi[(q * NP + v) * DIM + e];
  return inv_small<DIM>(J, Ji);
}

// Neumann pressure faces of cell cc (mpi_scnsim.cpp:521-549, mpi_scnsex.cpp:312-340): fe[a * DIM + c] -= int_f N_a p n_c over every face whose
// boundary id is listed in A.neumann_id.  The lanes lane, lane + stride, ... of the cell's group share the entries; X: the cell's vertices
template <int DIM, int NU, class Args>
__device__ __forceinline__ void neumann_faces(const Args &A, const FeTables &T, int64_t cc, const double *X, int lane, int stride, double *fe) {
  constexpr int NP = 1 << DIM;
  for (int f = 0; f < 2 * DIM; ++f) {
    const int bid = A.cell_face_bid[cc * 2 * DIM + f];
    if (bid < 0) continue;
    double pbc = 0; bool hit = false;
    for (int k = 0; k < A.n_neumann; ++k) if (A.neumann_id[k] == bid) { pbc = A.neumann_p[k]; hit = true; }
    if (!hit) continue;
    const int nd = f >> 1; const double sgn = (f & 1) ? 1.0 : -1.0;
    for (int i = lane; i < NU * DIM; i += stride) {
      const int a = i / DIM, c = i - a * DIM;
      double acc = 0;
      for (int qf = 0; qf < T.nqf; ++qf) {
        double Ji[DIM * DIM];
        const double det = cell_jacobian<DIM>(X, &T.fdpsi[(f * T.nqf + qf) * NP * DIM], Ji);
        acc += T.fphi[(f * T.nqf + qf) * NU + a] * (sgn * Ji[nd * DIM + c]) * pbc * fabs(det) * T.fw[qf];
      }
      fe[i] -= acc;
    }
  }
}

// the (dim, kv) instantiation of a launcher or kernel: a = <2, 1>, b = <2, 2>, c = <3, 1>, d = <3, 2>
template <class F>
inline F pick(int dim, int kv, F a, F b, F c, F d) { return dim == 2 ? (kv == 1 ? a : b) : (kv == 1 ? c : d); }

// blocks of 256 lanes that cover n
inline unsigned grid_for(int64_t n) { return unsigned((n + 255) / 256); }

// scatter add into global memory: hardware atomic, or plain read-modify-write when the launch covers one colour
template <bool ATOMIC>
__device__ inline void gadd(double *p, double v) {
  if constexpr (ATOMIC) unsafeAtomicAdd(p, v);
  else *p += v;
}

// 1D tensor factors of the Q_kv shape functions at the Gauss points (assemble2.hip, assemble3.hip)
struct Tab1D {
  double N[9];  // [q][i] 1D Lagrange shape i (equidistant nodes) at Gauss point q
  double dN[9]; // its derivative
  double xi[3], w[3];
};

__device__ inline void wsync2() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 3D Q2 (assemble3.hip, assemble_rows.hip): N_a(q) and the reference gradient of N_a at q from the tensor factors of Tabs3;
// q9 = (q % 9) * 9, q4 = (q / 9) * 4, a9 = a % 9, a3 = a / 9.
// The z factor is zero for q = 27 and a >= 27 (padding of the MFMA tiles): no masks in the contraction.
__device__ __forceinline__ void shape_ref4(const Tabs3 &T, int q9, int q4, int a9, int a3, double &N, double r[3]) {
  const int i2 = q9 + a9, i1 = q4 + a3;
  const double n2 = T.N2[i2], dx2 = T.DX2[i2], dy2 = T.DY2[i2], nz = T.Nz[i1], dz = T.dNz[i1];
  N = n2 * nz;
  r[0] = dx2 * nz; r[1] = dy2 * nz; r[2] = n2 * dz;
}

inline void tab1d(Tab1D &t, int kv) {
  const int n1 = kv + 1;
  std::memset(&t, 0, sizeof(t));
  if (n1 == 2) {
    const double a = 0.5 / std::sqrt(3.0);
    t.xi[0] = 0.5 - a; t.xi[1] = 0.5 + a; t.w[0] = t.w[1] = 0.5;
  } else {
    const double a = 0.5 * std::sqrt(0.6);
    t.xi[0] = 0.5 - a; t.xi[1] = 0.5; t.xi[2] = 0.5 + a;
    t.w[0] = t.w[2] = 5.0 / 18.0; t.w[1] = 8.0 / 18.0;
  }
  for (int q = 0; q < n1; ++q)
    for (int i = 0; i < n1; ++i) {
      const double xi_i = double(i) / kv;
      double v = 1, d = 0;
      for (int j = 0; j < n1; ++j)
        if (j != i) v *= (t.xi[q] - double(j) / kv) / (xi_i - double(j) / kv);
      for (int k = 0; k < n1; ++k) {
        if (k == i) continue;
        double p = 1.0 / (xi_i - double(k) / kv);
        for (int j = 0; j < n1; ++j)
          if (j != i && j != k) p *= (t.xi[q] - double(j) / kv) / (xi_i - double(j) / kv);
        d += p;
      }
      t.N[q * n1 + i] = v;
      t.dN[q * n1 + i] = d;
    }
}

} // namespace ifem
