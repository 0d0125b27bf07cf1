// sa.hip -- Fluid::MPI::SpalartAllmaras (source/mpi_spalart_allmaras.cpp) on gfx950: the one-equation turbulence model that feeds the eddy
// viscosity of SCnsIM::assemble (assemble_scns.hip, ScnsArgs::eddy).
//   sa_set_wall_points()       setup_cell_property  (:409-539)  nodal distance to the nearest wall point, brute force
//   sa_assemble()              assemble             (:620-862)  one wavefront per cell, modelled on k_scns_assemble
//   sa_solve()                 solve                (:864-889)  FGMRES(30) + ILU(0) (bilu.hip with dim = 1), then distribute()
//   sa_newton_step()           run_one_step         (:283-345)
//   sa_update_eddy_viscosity() update_eddy_viscosity (:892-914) writes ctx->eddy_viscosity, the buffer of ifem_set_eddy_viscosity
// The unknown nu~ lives on the scalar Q_kv space = the velocity nodes; the matrix is one value per block of the A_uu node pattern
// (Auu.rowptr / col, scattered through posUU), rows of owned nodes only.
// Geometry is the d-linear map of vcoords (MappingQ1, as everywhere in this library): the reference maps the support points of the
// wall distance with MappingQGeneric(degree), which differs from it on curved cells only.
// ONE deliberate deviation from the reference: at :757-770 it discards the result of std::min and returns an uninitialised r whenever
// |S~| > 1e-8.  Here r = min(nu~_present / (S~ kappa^2 d^2), 10) in that branch and r = 10 in the other: the evident intent.
// The FSI wall function (update_moving_wall_distance, update_boundary_condition, get_shear_velocity) is sa_wall.hip; the assembly reads its
// effective distance min(moving, fixed) through SaArgs::wall_d.
// Out of scope: refinement transfer, checkpoint payload, hanging-node lines (refused by sa_check), and partitioned contexts for the
// wall-function entry points.
// Partitioned contexts: rows of owned nodes only (owner computes, the ghost-layer cells are integrated redundantly), the ghost entries of nu~
// are refreshed through the velocity halo plan before every assembly and before the eddy viscosity, the operator input before every product,
// and the preconditioner is the ILU(0) of the owned x owned block (what bilu_analyse keeps).  Every rank passes ALL wall points and the
// constraint lines of its owned and ghost nodes, and keeps the ghost entries of IFEM_VEC_PRESENT current as for ifem_scns_assemble.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <vector>
#include "assemble_common.hpp"
#include "kernels.hpp"
#include "krylov.hpp"

namespace ifem {

namespace {

// ---- wall distance ---------------------------------------------------------------------------------------------------------------
// support point of local node a of every cell under the d-linear map.  Cells that share a node map it to the same point up to rounding (and to
// different points where the caller's per-cell vertex copies do not agree): the node takes the image from the touching cell of HIGHEST index
// (`last`, filled by k_sa_last_touch), so the result does not depend on the order in which the lanes run.
__global__ __launch_bounds__(256) void k_sa_last_touch(int64_t n_entries, const int32_t *__restrict__ cell_unodes, unsigned long long *__restrict__ last) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t < n_entries) atomicMax(&last[cell_unodes[t]], (unsigned long long)t);
}

template <int DIM, int KV>
__global__ __launch_bounds__(256) void k_sa_node_points(int64_t n_cells, const double *__restrict__ vcoords, const int32_t *__restrict__ cell_unodes,
                                                        const unsigned long long *__restrict__ last, double *__restrict__ xn) {
  using G_ = Geo<DIM, KV>;
  constexpr int NU = G_::NU, NP = G_::NP, N1 = G_::N1;
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= n_cells * NU || last[cell_unodes[t]] != (unsigned long long)t) return;
  const int64_t cell = t / NU;
  const int a = int(t - cell * NU);
  double xi[DIM];
  int r = a;
  for (int d = 0; d < DIM; ++d) { xi[d] = double(r % N1) / KV; r /= N1; }
  double x[DIM];
  for (int d = 0; d < DIM; ++d) x[d] = 0;
  for (int v = 0; v < NP; ++v) {
    double w = 1;
    for (int d = 0; d < DIM; ++d) w *= ((v >> d) & 1) ? xi[d] : 1.0 - xi[d];
    for (int d = 0; d < DIM; ++d) x[d] += w * vcoords[(cell * NP + v) * DIM + d];
  }
  const int64_t nd = cell_unodes[t];
  for (int d = 0; d < DIM; ++d) xn[nd * DIM + d] = x[d];
}

// one lane per local node, the wall points streamed through LDS in tiles of 256
template <int DIM>
__global__ __launch_bounds__(256) void k_sa_wall_distance(int64_t n_nodes, const double *__restrict__ xn, int64_t n_pts, const double *__restrict__ pts,
                                                          double *__restrict__ dist) {
  __shared__ double tile[256 * DIM];
  const int64_t nd = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const bool live = nd < n_nodes;
  double x[DIM];
  for (int d = 0; d < DIM; ++d) x[d] = live ? xn[nd * DIM + d] : 0.0;
  // min_i sqrt(s_i) = sqrt(min_i s_i) exactly (a correctly rounded square root is monotone): one square root per node, not per pair
  double best2 = DBL_MAX;
  for (int64_t base = 0; base < n_pts; base += 256) {
    const int cnt = int(n_pts - base < 256 ? n_pts - base : 256);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * DIM; i += 256) tile[i] = pts[base * DIM + i];
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      double cur = 0;
      for (int d = 0; d < DIM; ++d) { const double t = tile[i * DIM + d] - x[d]; cur += t * t; }
      best2 = fmin(best2, cur);
    }
  }
  if (live) dist[nd] = n_pts > 0 ? sqrt(best2) : DBL_MAX; // min_dist of :522 starts at DBL_MAX
}

// ---- cell kernel -----------------------------------------------------------------------------------------------------------------
struct SaArgs {
  int64_t n_cells, nUo, nUl;
  const FeTables *fe;
  const double *vcoords;
  const int32_t *cell_unodes, *indicator;
  const uint16_t *posUU;
  const int64_t *rp;
  double *val, *rhs;
  const uint8_t *is_c; // constraint object used (nullptr: none)
  const double *cval;
  const double *fluid;            // IFEM_VEC_PRESENT of the fluid: velocity dof DIM * node + c
  const double *nu_eval, *nu_present, *wall_d;
  double mu, rho, dt;
};

template <int DIM>
struct SaQPoint {
  double JxW, nu, nu0, diff, P, D;
  double u[DIM], gnu[DIM];
};

template <int DIM, int KV>
struct SaScratch {
  using G_ = Geo<DIM, KV>;
  double X[G_::NP * DIM];
  double gN[G_::NQ * G_::NU * DIM];
  SaQPoint<DIM> qp[G_::NQ];
  double ue[G_::NU * DIM], ne[G_::NU], n0e[G_::NU], de[G_::NU], fe[G_::NU], kd[G_::NU], cv[G_::NU];
  int64_t rs[G_::NU];
  int32_t len[G_::NU], un[G_::NU];
  uint8_t cf[G_::NU + 7];
};

// LDS per wavefront: gN dominates (NQ NU DIM doubles): 0.3 / 1.3 / 1.5 / 17.1 KiB for (2,1) / (2,2) / (3,1) / (3,2); whole scratch 0.9 / 3.0 / 3.0 /
// 22.6 KiB, times WPB = 4 / 4 / 4 / 2 wavefronts per workgroup
template <int DIM, int KV, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_sa_assemble(SaArgs A) {
  using G_ = Geo<DIM, KV>;
  constexpr int NU = G_::NU, NP = G_::NP, NQ = G_::NQ;
  // constants of :625-630
  constexpr double cv1 = 7.1, cv2 = 0.7, cv3 = 0.9, cb1 = 0.1355, cb2 = 0.622, ct3 = 1.2, ct4 = 0.5, kappa = 0.41, cw2 = 0.3, cw3 = 2.0, cn1 = 16.0;
  constexpr double sigma = 2.0 / 3.0, cw1 = cb1 / (kappa * kappa) + (1.0 + cb2) / sigma;
  extern __shared__ __align__(16) unsigned char smem_c[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  auto &S = *reinterpret_cast<SaScratch<DIM, KV> *>(smem_c + size_t(wave) * sizeof(SaScratch<DIM, KV>));
  const FeTables &T = *A.fe;
  const int64_t cell = int64_t(blockIdx.x) * WPB + wave;
  const bool active = cell < A.n_cells;
  const int64_t cc = active ? cell : 0;
  const int ind = (A.indicator && active) ? A.indicator[cc] : 0;
  const double laminar_nu = (ind == 1) ? 1.0 / A.rho : A.mu / A.rho; // :720-729
  // ---- phase 0: gather
  for (int i = lane; i < NP * DIM; i += 64) S.X[i] = A.vcoords[cc * NP * DIM + i];
  for (int a = lane; a < NU; a += 64) {
    const int32_t nd = A.cell_unodes[cc * NU + a];
    S.un[a] = nd;
    const bool own = nd < A.nUo;
    const int64_t r0 = own ? A.rp[nd] : 0, r1 = own ? A.rp[nd + 1] : 0;
    S.rs[a] = r0; S.len[a] = own ? int32_t(r1 - r0) : -1;
    for (int c = 0; c < DIM; ++c) S.ue[a * DIM + c] = A.fluid[int64_t(DIM) * nd + c];
    S.ne[a] = A.nu_eval[nd];
    S.n0e[a] = A.nu_present[nd];
    S.de[a] = A.wall_d[nd];
    S.cf[a] = A.is_c ? A.is_c[nd] : 0;
    S.cv[a] = A.cval ? A.cval[nd] : 0.0;
  }
  __syncthreads();
  // ---- phase 1: geometry, fields and model coefficients per quadrature point (:731-791)
  for (int q = lane; q < NQ; q += 64) {
    double Ji[DIM * DIM];
    const double det = cell_jacobian<DIM>(S.X, T.dpsi, Ji, q);
    SaQPoint<DIM> &Q = S.qp[q];
    Q.JxW = fabs(det) * T.w[q];
    double u[DIM], G[DIM * DIM], gnu[DIM];
    double nu = 0, nu0 = 0, d = 0;
    for (int c = 0; c < DIM; ++c) { u[c] = 0; gnu[c] = 0; }
    for (int i = 0; i < DIM * DIM; ++i) G[i] = 0;
    for (int a = 0; a < NU; ++a) {
      double ga[DIM];
      for (int k = 0; k < DIM; ++k) {
        double g = 0;
        for (int e = 0; e < DIM; ++e) g += T.dphi[(q * NU + a) * DIM + e] * Ji[e * DIM + k];
        ga[k] = g;
        S.gN[(q * NU + a) * DIM + k] = g;
      }
      const double N = T.phi[q * NU + a];
      for (int c = 0; c < DIM; ++c) {
        const double ue = S.ue[a * DIM + c];
        u[c] += N * ue;
        for (int k = 0; k < DIM; ++k) G[c * DIM + k] += ue * ga[k]; // d u_c / d x_k
      }
      nu += N * S.ne[a];
      nu0 += N * S.n0e[a];
      d += N * S.de[a];
      for (int k = 0; k < DIM; ++k) gnu[k] += S.ne[a] * ga[k];
    }
    double Sv; // |curl u|
    if constexpr (DIM == 2) Sv = fabs(G[1 * DIM + 0] - G[0 * DIM + 1]);
    else {
      const double w0 = G[2 * DIM + 1] - G[1 * DIM + 2], w1 = G[0 * DIM + 2] - G[2 * DIM + 0], w2 = G[1 * DIM + 0] - G[0 * DIM + 1];
      Sv = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    }
    const double chi = nu0 / laminar_nu, chi3 = chi * chi * chi;
    const double ft2 = ct3 * exp(-ct4 * chi * chi);
    const double fv1 = chi3 / (chi3 + cv1 * cv1 * cv1);
    const double fv2 = 1.0 - chi / (1.0 + chi * fv1);
    const double k2d2 = kappa * kappa * d * d;
    const double S_bar = nu0 / k2d2 * fv2;
    const double S_tilde = S_bar >= -cv2 * Sv ? Sv + S_bar : Sv + Sv * (cv2 * cv2 * Sv - cv3 * S_bar) / ((cv3 - 2 * cv2) * Sv - S_bar);
    const double r = fabs(S_tilde) > 1e-8 ? fmin(nu0 / (S_tilde * k2d2), 10.0) : 10.0; // the deviation stated at the head of this file
    const double r2 = r * r, r6 = r2 * r2 * r2;
    const double g = r + cw2 * (r6 - r);
    const double g2 = g * g, g6 = g2 * g2 * g2, c6 = cw3 * cw3 * cw3 * cw3 * cw3 * cw3;
    const double fw = g * pow((1 + c6) / (g6 + c6), 1.0 / 6.0);
    const bool pos = nu0 >= 0;
    Q.P = pos ? cb1 * (1 - ft2) * S_tilde : cb1 * (1 - ct3) * Sv;
    Q.D = pos ? (cw1 * fw - cb1 / (kappa * kappa) * ft2) / (d * d) : -cw1 / (d * d);
    const double fn = pos ? 1.0 : (cn1 + chi3) / (cn1 - chi3);
    Q.diff = 1 / sigma * (laminar_nu + fn * nu0);
    Q.nu = nu; Q.nu0 = nu0;
    for (int c = 0; c < DIM; ++c) { Q.u[c] = u[c]; Q.gnu[c] = gnu[c]; }
  }
  __syncthreads();
  // ---- phase 2: right-hand side (:823-841) and the diagonal of the local matrix (the constrained rows need all of it)
  for (int i = lane; i < NU; i += 64) {
    double f = 0, kii = 0;
    for (int q = 0; q < NQ; ++q) {
      const SaQPoint<DIM> &Q = S.qp[q];
      const double N = T.phi[q * NU + i];
      const double *gi = &S.gN[(q * NU + i) * DIM];
      double ug = 0, gg = 0, gign = 0, gigi = 0, ugi = 0;
      for (int k = 0; k < DIM; ++k) { ug += Q.u[k] * Q.gnu[k]; gg += Q.gnu[k] * Q.gnu[k]; gign += gi[k] * Q.gnu[k]; gigi += gi[k] * gi[k]; ugi += Q.u[k] * gi[k]; }
      f += -(N * (Q.nu - Q.nu0) / A.dt + N * ug + Q.diff * gign - cb2 / sigma * N * gg - Q.P * N * Q.nu + Q.D * N * Q.nu * Q.nu) * Q.JxW;
      kii += (N * N / A.dt + N * ugi + Q.diff * gigi - 2 * cb2 / sigma * N * gign - Q.P * N * N + 2 * Q.D * N * N * Q.nu) * Q.JxW;
    }
    S.fe[i] = f;
    S.kd[i] = kii;
  }
  __syncthreads();
  double avg = 0; // mean |diagonal| of the cell: what a constrained row with K_ii = 0 takes
  for (int i = 0; i < NU; ++i) avg += fabs(S.kd[i]);
  avg /= NU;
  // ---- phase 3: local matrix (:799-820) and scatter by the rule of distribute_local_to_global(..., true)
  for (int t = lane; t < NU * NU; t += 64) {
    const int i = t / NU, j = t - i * NU;
    if (!active || S.len[i] < 0) continue; // row owned elsewhere
    const bool ri = S.cf[i], cj = S.cf[j];
    if (ri ? (i != j) : cj && S.cv[j] == 0.0) continue; // a dropped entry
    double *dst = A.val + S.rs[i] + A.posUU[(cc * NU + i) * NU + j];
    if (ri) {
      const double kd = fabs(S.kd[i]) != 0 ? fabs(S.kd[i]) : avg;
      unsafeAtomicAdd(dst, kd);
      unsafeAtomicAdd(&A.rhs[S.un[i]], S.cv[i] * kd);
      continue;
    }
    double v = 0;
    for (int q = 0; q < NQ; ++q) {
      const SaQPoint<DIM> &Q = S.qp[q];
      const double Ni = T.phi[q * NU + i], Nj = T.phi[q * NU + j];
      const double *gi = &S.gN[(q * NU + i) * DIM], *gj = &S.gN[(q * NU + j) * DIM];
      double ugj = 0, gigj = 0, gjgn = 0;
      for (int k = 0; k < DIM; ++k) { ugj += Q.u[k] * gj[k]; gigj += gi[k] * gj[k]; gjgn += gj[k] * Q.gnu[k]; }
      v += (Ni * Nj / A.dt + Ni * ugj + Q.diff * gigj - 2 * cb2 / sigma * Ni * gjgn - Q.P * Ni * Nj + 2 * Q.D * Ni * Nj * Q.nu) * Q.JxW;
    }
    if (cj) unsafeAtomicAdd(&S.fe[i], -v * S.cv[j]); // the column is dropped, its inhomogeneity moves to the right-hand side
    else unsafeAtomicAdd(dst, v);
  }
  __syncthreads();
  if (active)
    for (int i = lane; i < NU; i += 64)
      if (!S.cf[i] && S.len[i] >= 0) unsafeAtomicAdd(&A.rhs[S.un[i]], S.fe[i]);
}

template <int DIM, int KV>
void launch_sa_t(ifem_ctx *ctx, const SaArgs &A) {
  constexpr int WPB = (DIM == 3 && KV == 2) ? 2 : 4;
  const size_t smem = WPB * sizeof(SaScratch<DIM, KV>);
  IFEM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sa_assemble<DIM, KV, WPB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  const int64_t nblk = (A.n_cells + WPB - 1) / WPB;
  hipLaunchKernelGGL((k_sa_assemble<DIM, KV, WPB>), dim3((unsigned)nblk), dim3(64 * WPB), smem, ctx->stream, A);
  IFEM_HIP_CHECK(hipGetLastError());
}

template <int DIM, int KV>
void launch_node_points_t(ifem_ctx *ctx, double *xn) {
  const int64_t n = ctx->n_cells * Geo<DIM, KV>::NU;
  if (n == 0) return;
  DBuf<unsigned long long> last;
  last.alloc((size_t)ctx->nUl);
  IFEM_HIP_CHECK(hipMemsetAsync(last.p, 0, last.n * sizeof(unsigned long long), ctx->stream));
  const dim3 g(unsigned((n + 255) / 256)), b(256);
  hipLaunchKernelGGL(k_sa_last_touch, g, b, 0, ctx->stream, n, ctx->cell_unodes.p, last.p);
  IFEM_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_sa_node_points<DIM, KV>), g, b, 0, ctx->stream, ctx->n_cells, ctx->vcoords.p, ctx->cell_unodes.p, last.p, xn);
  IFEM_HIP_CHECK(hipGetLastError());
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // `last` is released on return
}

// ---- the linear system: y = A x over the owned rows is linalg.hip::spmv_node_scalar with one component ---------------------------------
// mu_t = f_v1 nu~ rho (:904-911)
__global__ void k_sa_eddy(int64_t n, const double *__restrict__ nu, double laminar_nu, double rho, double *__restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr double cv1_3 = 7.1 * 7.1 * 7.1;
  const double chi = nu[i] / laminar_nu, chi3 = chi * chi * chi;
  out[i] = chi3 / (chi3 + cv1_3) * nu[i] * rho;
}

// ghost entries of a nodal scalar [nUl] := the owners' values (collective; nothing to do on one rank)
void refresh_ghosts(ifem_ctx *ctx, double *x) {
  if (ctx->halo.nranks == 1) return;
  KScope ks(ctx, IFEM_KC_OTHER);
  halo_refresh_nodal(ctx, 1, x);
}

void check_params(const ifem_sa_params *p) {
  if (!p || !(p->dt > 0) || !(p->viscosity > 0) || !(p->rho > 0)) throw Error(IFEM_E_BADPARAM, "bad ifem_sa_params");
}

} // namespace

// every compute entry point: what the model does not cover is refused before anything is allocated
void sa_check(ifem_ctx *ctx) {
  if (ctx->hang.n > 0 || ctx->hang.active)
    throw Error(IFEM_E_BADPARAM, "ifem_sa_*: contexts with hanging nodes are not supported by the Spalart-Allmaras model");
  if (ctx->dim < 2 || ctx->dim > 3 || ctx->kv < 1 || ctx->kv > 2) throw Error(IFEM_E_BADPARAM, "unsupported (dim, kv)");
}

// state on first use: zero vectors, no constraints, no wall points (d = DBL_MAX)
void sa_ensure(ifem_ctx *ctx) {
  SaState &sa = ctx->sa;
  const size_t n = (size_t)ctx->nUl;
  if (sa.vec[0].n == n && sa.wall_d.n == n) return;
  hipStream_t s = ctx->stream;
  for (auto &v : sa.vec) { v.alloc(n); IFEM_HIP_CHECK(hipMemsetAsync(v.p, 0, n * sizeof(double), s)); }
  for (int w = 0; w < 2; ++w) {
    sa.is_c[w].alloc(n); sa.cval[w].alloc(n);
    IFEM_HIP_CHECK(hipMemsetAsync(sa.is_c[w].p, 0, n, s));
    IFEM_HIP_CHECK(hipMemsetAsync(sa.cval[w].p, 0, n * sizeof(double), s));
    sa.has_c[w] = false;
  }
  const std::vector<double> far(n, DBL_MAX);
  sa.wall_d.upload(far.data(), n, s);
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
}

// the support points of the local nodes: they depend on the mesh alone, once per context
const double *sa_node_points(ifem_ctx *ctx) {
  DBuf<double> &xn = ctx->sa.node_points;
  const int64_t n = ctx->nUl;
  const int dim = ctx->dim;
  if (xn.n != (size_t)n * dim) {
    xn.alloc((size_t)n * dim);
    IFEM_HIP_CHECK(hipMemsetAsync(xn.p, 0, xn.n * sizeof(double), ctx->stream));
    pick(dim, ctx->kv, launch_node_points_t<2, 1>, launch_node_points_t<2, 2>, launch_node_points_t<3, 1>, launch_node_points_t<3, 2>)(ctx, xn.p);
  }
  return xn.p;
}

void sa_set_wall_points(ifem_ctx *ctx, int64_t n_pts, const double *pts) {
  sa_check(ctx);
  if (n_pts < 0 || (n_pts > 0 && !pts)) throw Error(IFEM_E_BADPARAM, "ifem_sa_set_wall_points: n < 0 or no points");
  sa_ensure(ctx);
  hipStream_t s = ctx->stream;
  const int dim = ctx->dim;
  const int64_t n = ctx->nUl;
  DBuf<double> dp;
  dp.upload(pts, (size_t)n_pts * dim, s);
  KScope ks(ctx, IFEM_KC_OTHER, double(n) * (dim + 1) * 8 + double(n_pts) * dim * 8);
  const double *xn = sa_node_points(ctx);
  if (dim == 2) hipLaunchKernelGGL((k_sa_wall_distance<2>), dim3(grid_for(n)), dim3(256), 0, s, n, xn, n_pts, dp.p, ctx->sa.wall_d.p);
  else hipLaunchKernelGGL((k_sa_wall_distance<3>), dim3(grid_for(n)), dim3(256), 0, s, n, xn, n_pts, dp.p, ctx->sa.wall_d.p);
  IFEM_HIP_CHECK(hipGetLastError());
  sa_wall_refresh_d_eff(ctx); // the effective distance of a moving wall follows the new fixed one
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
}

// a node listed twice keeps its LAST line, as for ifem_set_constraints
void sa_set_constraints(ifem_ctx *ctx, int which, int32_t n, const int32_t *node, const double *inhom) {
  sa_check(ctx);
  if (which < 0 || which > 1 || n < 0 || (n > 0 && !node)) throw Error(IFEM_E_BADPARAM, "ifem_sa_set_constraints: which / n / node");
  std::vector<int32_t> kept;
  std::vector<double> kept_val;
  DBuf<uint8_t> flag;
  DBuf<double> cval;
  if (!build_line_set(ctx, (size_t)ctx->nUl, n, node, which == 1 ? inhom : nullptr, kept, kept_val, flag, cval))
    throw Error(IFEM_E_BADPARAM, "ifem_sa_set_constraints: node outside [0, n_unodes_local)");
  sa_ensure(ctx);
  SaState &sa = ctx->sa;
  sa.is_c[which].swap(flag);
  sa.cval[which].swap(cval);
  sa.has_c[which] = n > 0;
}

void sa_assemble(ifem_ctx *ctx, const ifem_sa_params *p, int use_nonzero) {
  sa_check(ctx);
  check_params(p);
  sa_ensure(ctx);
  SaState &sa = ctx->sa;
  hipStream_t s = ctx->stream;
  const size_t nnz = (size_t)ctx->Auu.nnzb;
  if (sa.val.n != nnz) sa.val.alloc(nnz, "the Spalart-Allmaras matrix");
  refresh_ghosts(ctx, sa.vec[IFEM_SA_EVAL].p);
  refresh_ghosts(ctx, sa.vec[IFEM_SA_PRESENT].p);
  {
    KScope ks(ctx, IFEM_KC_ZERO_FILL, double(nnz + ctx->nUl) * 8);
    IFEM_HIP_CHECK(hipMemsetAsync(sa.val.p, 0, nnz * sizeof(double), s));
    IFEM_HIP_CHECK(hipMemsetAsync(sa.vec[IFEM_SA_RHS].p, 0, sa.vec[IFEM_SA_RHS].n * sizeof(double), s));
  }
  const int w = use_nonzero ? 1 : 0;
  SaArgs A{};
  A.n_cells = ctx->n_cells; A.nUo = ctx->nUo; A.nUl = ctx->nUl;
  A.fe = ctx->d_fe.p;
  A.vcoords = ctx->vcoords.p; A.cell_unodes = ctx->cell_unodes.p; A.indicator = ctx->indicator.p;
  A.posUU = ctx->posUU.p; A.rp = ctx->Auu.rowptr.p;
  A.val = sa.val.p; A.rhs = sa.vec[IFEM_SA_RHS].p;
  A.is_c = sa.has_c[w] ? sa.is_c[w].p : nullptr;
  A.cval = sa.has_c[w] ? sa.cval[w].p : nullptr;
  A.fluid = ctx->vec[IFEM_VEC_PRESENT].p;
  A.nu_eval = sa.vec[IFEM_SA_EVAL].p; A.nu_present = sa.vec[IFEM_SA_PRESENT].p;
  A.wall_d = sa.mw.updated ? sa.mw.d_eff.p : sa.wall_d.p; // min(moving, fixed) once a moving wall was measured (:711-719)
  A.mu = p->viscosity; A.rho = p->rho; A.dt = p->dt;
  {
    // algorithmic bytes: the values written + the node data and position tables read
    const int nu = ctx->nu;
    KScope ks(ctx, IFEM_KC_ASSEMBLE, double(nnz) * 8 + double(ctx->n_cells) * (double(nu) * nu * 2 + double(nu) * (4 + 8 * (ctx->dim + 4)) + ctx->np * ctx->dim * 8));
    if (ctx->n_cells > 0) pick(ctx->dim, ctx->kv, launch_sa_t<2, 1>, launch_sa_t<2, 2>, launch_sa_t<3, 1>, launch_sa_t<3, 2>)(ctx, A);
  }
  sa.assembled = true;
  sa.val_order = ctx->Auu.order_version;
  sa.ilu.factored = false;
}

// SolverFGMRES + PreconditionEuclid of :870-882, then constraints_used.distribute(newton_update)
void sa_solve(ifem_ctx *ctx, int use_nonzero, uint32_t *iters, double *res_out) {
  sa_check(ctx);
  SaState &sa = ctx->sa;
  if (!sa.assembled) throw Error(IFEM_E_BADPARAM, "ifem_sa_solve called before ifem_sa_assemble");
  hipStream_t s = ctx->stream;
  const int64_t n = ctx->nUo;
  BIlu &I = sa.ilu;
  // the first stored fluid assembly of a 3D Q2 context re-orders the blocks of the A_uu rows in place (setup.hip::reorder_uu_rows)
  if (sa.val_order != ctx->Auu.order_version)
    throw Error(IFEM_E_BADPARAM, "ifem_sa_solve: the A_uu row order changed since ifem_sa_assemble (first fluid assembly): assemble again");
  if (!I.analysed || sa.ilu_order != ctx->Auu.order_version) {
    bilu_analyse(ctx, I, 1, n, ctx->Auu.rowptr.p, ctx->Auu.col.p);
    sa.ilu_order = ctx->Auu.order_version;
  }
  if (!I.factored) {
    sa.ilu_ok = bilu_factor(ctx, I, sa.val.p);
    if (!sa.ilu_ok) { // as scns_solve: a factorisation that broke down is not applied
      if (sa.dinv.n != (size_t)n) sa.dinv.alloc((size_t)n);
      KScope ks(ctx, IFEM_KC_OTHER);
      scalar_diag(ctx, ctx->Auu, sa.val.p, sa.dinv.p);
    }
  }
  const bool ranks = ctx->halo.nranks > 1;
  if (ranks && sa.xext.n != (size_t)ctx->nUl) sa.xext.alloc((size_t)ctx->nUl);
  const OpFn Aop = [&](const double *x, double *y) {
    if (ranks) { // the compact owned input, ghost-extended
      v_copy(ctx, n, x, sa.xext.p);
      refresh_ghosts(ctx, sa.xext.p);
      x = sa.xext.p;
    }
    KScope ks(ctx, IFEM_KC_OTHER, double(ctx->Auu.nnzb) * 12 + double(n) * 24);
    spmv_node_scalar(ctx, 1, sa.val.p, nullptr, nullptr, x, y);
  };
  const OpFn Pop = [&](const double *x, double *y) {
    if (sa.ilu_ok) bilu_apply(ctx, I, /*sweeps=*/-1, x, y);
    else vec_div(ctx, n, sa.dinv.p, x, y);
  };
  const MdotFn mdot = [ctx, n](int k, const double *V, int64_t ld, const double *w, double *out) { v_mdot(ctx, n, k, V, ld, w, out, /*all_ranks=*/true); };
  const double *rhs = sa.vec[IFEM_SA_RHS].p;
  double *upd = sa.vec[IFEM_SA_UPDATE].p;
  double bn;
  mdot(1, rhs, n, rhs, &bn);
  bn = std::sqrt(bn);
  const double tol = 1e-8 * bn; // :870-871
  const int maxit = (int)std::min<int64_t>(2 * (ctx->n_global_u / ctx->dim), 1 << 30); // n_global_u counts velocity dofs: dim per node of the scalar space
  const int m = 30;
  const int64_t ld = basis_ld(ctx, n);
  if (sa.w.n != (size_t)ld) sa.w.alloc((size_t)ld);
  grow_basis(ctx, sa.V, ld, kBasisStart, m + 1);
  grow_basis(ctx, sa.Z, ld, kBasisStart, m);
  const auto grow = basis_grower(ctx, sa.V, sa.Z, ld, m + 1);
  double res = 0;
  const int it = gmres(ctx, n, ld, /*reorth=*/true, Aop, Pop, /*flexible=*/true, rhs, upd, m, maxit, tol, sa.V.p, sa.Z.p, sa.w.p, &res, mdot, nullptr, &grow);
  const int w = use_nonzero ? 1 : 0;
  if (sa.has_c[w]) {
    KScope ks(ctx, IFEM_KC_OTHER);
    distribute_lines(ctx, ctx->nUl, ctx->nUl, 0, sa.is_c[w].p, sa.cval[w].p, upd);
  }
  IFEM_HIP_CHECK(hipGetLastError());
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  if (iters) *iters = (uint32_t)it;
  if (res_out) *res_out = res;
  if (!(res <= tol)) throw_noconv("Spalart-Allmaras FGMRES", it, res, tol);
}

void sa_update_eddy_viscosity(ifem_ctx *ctx, const ifem_sa_params *p, double *host_out) {
  sa_check(ctx);
  check_params(p);
  sa_ensure(ctx);
  hipStream_t s = ctx->stream;
  const int64_t n = ctx->nUl;
  if (ctx->eddy_viscosity.n != (size_t)n) ctx->eddy_viscosity.alloc((size_t)n);
  refresh_ghosts(ctx, ctx->sa.vec[IFEM_SA_PRESENT].p);
  {
    KScope ks(ctx, IFEM_KC_OTHER, double(n) * 16);
    hipLaunchKernelGGL(k_sa_eddy, dim3(grid_for(n)), dim3(256), 0, s, n, ctx->sa.vec[IFEM_SA_PRESENT].p, p->viscosity / p->rho, p->rho, ctx->eddy_viscosity.p);
  }
  IFEM_HIP_CHECK(hipGetLastError());
  if (host_out) IFEM_HIP_CHECK(hipMemcpyAsync(host_out, ctx->eddy_viscosity.p, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, s));
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
}

int sa_newton_step(ifem_ctx *ctx, const ifem_sa_params *p, int apply_nonzero, double tolerance, int max_iterations, double *log) {
  sa_check(ctx);
  check_params(p);
  sa_ensure(ctx);
  SaState &sa = ctx->sa;
  const int64_t n = ctx->nUl, no = ctx->nUo;
  v_copy(ctx, n, sa.vec[IFEM_SA_PRESENT].p, sa.vec[IFEM_SA_EVAL].p);
  const int outer = newton_loop(1e-14, apply_nonzero, tolerance, max_iterations, log, [&](int nz) { // :296-297
    v_zero(ctx, n, sa.vec[IFEM_SA_UPDATE].p);
    sa_assemble(ctx, p, nz);
    uint32_t its = 0;
    double res = 0, rr;
    sa_solve(ctx, nz, &its, &res);
    v_mdot(ctx, no, 1, sa.vec[IFEM_SA_RHS].p, no, sa.vec[IFEM_SA_RHS].p, &rr, /*all_ranks=*/true);
    v_axpy(ctx, n, 1.0, sa.vec[IFEM_SA_UPDATE].p, sa.vec[IFEM_SA_EVAL].p);
    return NewtonIter{std::sqrt(rr), double(its), res};
  });
  v_copy(ctx, n, sa.vec[IFEM_SA_EVAL].p, sa.vec[IFEM_SA_PRESENT].p);
  sa_update_eddy_viscosity(ctx, p, nullptr);
  return outer;
}

} // namespace ifem
