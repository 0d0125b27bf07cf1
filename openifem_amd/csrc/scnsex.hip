// scnsex.hip -- Fluid::MPI::SCnsEX (source/mpi_scnsex.cpp) on gfx950: the explicit split solver of the slightly compressible equations.
//   scnsex_setup()        assemble(true, .), matrices  (:248-279)  one wavefront per cell, modelled on k_sa_assemble
//   scnsex_assemble_rhs() assemble(., .), right sides  (:282-340)  the same shape of kernel, one flag for the two sides; then the lift
//   scnsex_solve()        solve                        (:389-427)  cg_device + Jacobi, then distribute()
//   scnsex_step()         run_one_step, outer loop     (:448-503)
// Both linear systems are scalar, symmetric positive definite and depend on the geometry, mu, rho, dt and the PML field alone.  The
// velocity matrix of :258-267 couples equal components only: it is I_dim (x) A_v with A_v = mu K + rho / dt M + rho M_sigma; the pressure
// matrix of :271-277 is A_p = (M / dt + M_sigma) / atm on the same nodes (the class demands equal order, :12-14).  Each is ONE value per
// block of the A_uu node pattern (Auu.rowptr / col, scattered through posUU, as ctx->sa.val): the block CSR of A_uu is never allocated.
// A_v and A_p are kept UNCONSTRAINED.  For component c, with P_c the mask of the dofs of c that the non-zero constraint set leaves free,
// the operator of the velocity solve is  y_c = P_c A_v P_c x_c + (I - P_c) diag(A_v) x_c  (one kernel, all components per matrix read),
// and the right-hand side takes rhs_c <- P_c (rhs_c - A_v g_c), g the constraint values: what distribute_local_to_global(..., false) does
// to the free rows, constrained rows 0.  The reference re-scatters the whole velocity matrix from stored local matrices every outer
// iteration while boundary values depend on time (:355,362-371); here that is the one product A_v g.
// Right-hand sides: each cell sums its NU (x dim) entries in LDS and adds them to memory with one fp64 atomic per entry -- 128^3 Q1 cells add
// 0.40 GB (velocity) / 0.13 GB (pressure) per side in pieces of 24 / 8 bytes; measured 1.17 ms per launch for the whole kernel there
// (profiles/scnsex.txt), the share of the atomics not separated.
// ONE deliberate deviation from the reference: Jacobi takes the place of BoomerAMG (:407-417) -- preconditioner only; operator, zero
// start vector (:402,:465) and stopping rule 1e-6 ||rhs|| (:396-397) are the reference's.  The Jacobi-scaled matrices are mass-dominated.
// Out of scope, refused with IFEM_E_BADPARAM before any launch: partitioned contexts, hanging-node lines, velocity and pressure on
// different nodes (Taylor-Hood); refinement and the turbulence model attached to SCnsEX are not built.
#include <hip/hip_runtime.h>
#include <cmath>
#include <vector>
#include "assemble_common.hpp"
#include "kernels.hpp"
#include "krylov.hpp"

namespace ifem {

namespace {

constexpr double kAtm = 1013250.0, kCpToCv = 1.4; // :177-178

struct ExArgs {
  int64_t n_cells, p_off; // p_off: offset of the pressure block in a block vector (dim * nUl)
  const FeTables *fe;
  const double *vcoords;
  const int32_t *cell_unodes, *cell_face_bid;
  const uint16_t *posUU;
  const int64_t *rp;
  double *av, *ap, *dv, *dp;       // set-up: values on the node pattern, nodal diagonals
  const double *sigma, *body_force; // [n_cells][NQ], [n_cells][NQ][DIM] or nullptr
  const double *eval, *present;
  double *rhs;
  double mu, rho, dt;
  double g[3];
  int n_neumann;
  int neumann_id[8];
  double neumann_p[8];
  int velocity;
};

template <int DIM, int KV>
struct ExSetupScratch {
  using G_ = Geo<DIM, KV>;
  double X[G_::NP * DIM];
  double gN[G_::NQ * G_::NU * DIM];
  double JxW[G_::NQ], sg[G_::NQ];
  int64_t rs[G_::NU];
  int32_t un[G_::NU];
};

// ---- 1. matrices: K_e, M_e, M_sigma,e of one cell, combined and scattered (:248-279)
template <int DIM, int KV, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_ex_setup(ExArgs A) {
  using G_ = Geo<DIM, KV>;
  constexpr int NU = G_::NU, NP = G_::NP, NQ = G_::NQ;
  extern __shared__ __align__(16) unsigned char smem_c[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  auto &S = *reinterpret_cast<ExSetupScratch<DIM, KV> *>(smem_c + size_t(wave) * sizeof(ExSetupScratch<DIM, KV>));
  const FeTables &T = *A.fe;
  const int64_t cell = int64_t(blockIdx.x) * WPB + wave;
  const bool active = cell < A.n_cells;
  const int64_t cc = active ? cell : 0;
  for (int i = lane; i < NP * DIM; i += 64) S.X[i] = A.vcoords[cc * NP * DIM + i];
  for (int a = lane; a < NU; a += 64) {
    const int32_t nd = A.cell_unodes[cc * NU + a];
    S.un[a] = nd;
    S.rs[a] = A.rp[nd];
  }
  __syncthreads();
  for (int q = lane; q < NQ; q += 64) {
    double Ji[DIM * DIM];
    const double det = cell_jacobian<DIM>(S.X, T.dpsi, Ji, q);
    S.JxW[q] = fabs(det) * T.w[q];
    S.sg[q] = A.sigma ? A.sigma[cc * NQ + q] : 0.0; // a missing field is zero (:181-187)
    for (int a = 0; a < NU; ++a)
      for (int k = 0; k < DIM; ++k) {
        double g = 0;
        for (int e = 0; e < DIM; ++e) g += T.dphi[(q * NU + a) * DIM + e] * Ji[e * DIM + k];
        S.gN[(q * NU + a) * DIM + k] = g;
      }
  }
  __syncthreads();
  if (!active) return;
  for (int t = lane; t < NU * NU; t += 64) {
    const int i = t / NU, j = t - i * NU;
    double k = 0, m = 0, ms = 0;
    for (int q = 0; q < NQ; ++q) {
      const double *gi = &S.gN[(q * NU + i) * DIM], *gj = &S.gN[(q * NU + j) * DIM];
      double gg = 0;
      for (int d = 0; d < DIM; ++d) gg += gi[d] * gj[d];
      const double nn = T.phi[q * NU + i] * T.phi[q * NU + j] * S.JxW[q];
      k += gg * S.JxW[q];
      m += nn;
      ms += nn * S.sg[q];
    }
    const double v = A.mu * k + A.rho / A.dt * m + A.rho * ms; // :258-267
    const double p = (m / A.dt + ms) / kAtm;                    // :271-277
    const int64_t at = S.rs[i] + A.posUU[(cc * NU + i) * NU + j];
    unsafeAtomicAdd(&A.av[at], v);
    unsafeAtomicAdd(&A.ap[at], p);
    if (i == j) {
      unsafeAtomicAdd(&A.dv[S.un[i]], v);
      unsafeAtomicAdd(&A.dp[S.un[i]], p);
    }
  }
}

// ---- 3. explicit right-hand sides (:282-340): A.velocity selects the side
template <int DIM, int KV>
struct ExRhsScratch {
  using G_ = Geo<DIM, KV>;
  double X[G_::NP * DIM];
  double f[G_::NQ * DIM]; // integrand x JxW per quadrature point: DIM components (velocity) or one scalar at [q * DIM] (pressure)
  double ue[G_::NU * DIM], u0e[G_::NU * DIM], pe[G_::NU], p0e[G_::NU];
  double fe[G_::NU * DIM];
  int32_t un[G_::NU];
};

// LPC lanes per cell = NQ rounded up to a power of two (4 / 16 / 8 / 32 for (2,1) / (2,2) / (3,1) / (3,2)): a workgroup of 256 lanes takes
// 256 / LPC cells, so that every lane owns a quadrature point in the heaviest phase (one cell per wavefront left 8 of 64 lanes working
// on 3D Q1 cells)
template <int DIM, int KV, int LPC>
__global__ __launch_bounds__(256) void k_ex_rhs(ExArgs A) {
  constexpr int CPB = 256 / LPC;
  using G_ = Geo<DIM, KV>;
  constexpr int NU = G_::NU, NP = G_::NP, NQ = G_::NQ;
  extern __shared__ __align__(16) unsigned char smem_c[];
  const int sub = threadIdx.x / LPC, lane = threadIdx.x % LPC;
  auto &S = *reinterpret_cast<ExRhsScratch<DIM, KV> *>(smem_c + size_t(sub) * sizeof(ExRhsScratch<DIM, KV>));
  const FeTables &T = *A.fe;
  const int64_t cell = int64_t(blockIdx.x) * CPB + sub;
  const bool active = cell < A.n_cells;
  const int64_t cc = active ? cell : 0;
  const bool vel = A.velocity != 0;
  for (int i = lane; i < NP * DIM; i += LPC) S.X[i] = A.vcoords[cc * NP * DIM + i];
  for (int a = lane; a < NU; a += LPC) {
    const int32_t nd = A.cell_unodes[cc * NU + a];
    S.un[a] = nd;
    for (int c = 0; c < DIM; ++c) {
      S.ue[a * DIM + c] = A.eval[int64_t(DIM) * nd + c];
      S.u0e[a * DIM + c] = A.present[int64_t(DIM) * nd + c];
    }
    S.pe[a] = A.eval[A.p_off + nd];
    S.p0e[a] = A.present[A.p_off + nd];
  }
  __syncthreads();
  for (int q = lane; q < NQ; q += LPC) {
    double Ji[DIM * DIM];
    const double det = cell_jacobian<DIM>(S.X, T.dpsi, Ji, q);
    const double JxW = fabs(det) * T.w[q];
    double u[DIM], u0[DIM], G[DIM * DIM], gp[DIM];
    double p = 0, p0 = 0;
    for (int c = 0; c < DIM; ++c) { u[c] = 0; u0[c] = 0; gp[c] = 0; }
    for (int i = 0; i < DIM * DIM; ++i) G[i] = 0;
    for (int a = 0; a < NU; ++a) {
      double ga[DIM];
      for (int k = 0; k < DIM; ++k) {
        double g = 0;
        for (int e = 0; e < DIM; ++e) g += T.dphi[(q * NU + a) * DIM + e] * Ji[e * DIM + k];
        ga[k] = g;
      }
      const double N = T.phi[q * NU + a];
      for (int c = 0; c < DIM; ++c) {
        const double ue = S.ue[a * DIM + c];
        u[c] += N * ue;
        u0[c] += N * S.u0e[a * DIM + c];
        for (int k = 0; k < DIM; ++k) G[c * DIM + k] += ue * ga[k]; // d u_c / d x_k
      }
      p += N * S.pe[a];
      p0 += N * S.p0e[a];
      for (int k = 0; k < DIM; ++k) gp[k] += S.pe[a] * ga[k];
    }
    if (vel) { // :284-291
      for (int c = 0; c < DIM; ++c) {
        double Gu = 0; // (grad u) u
        for (int k = 0; k < DIM; ++k) Gu += G[c * DIM + k] * u[k];
        const double bf = A.body_force ? A.body_force[(cc * NQ + q) * DIM + c] : 0.0;
        S.f[q * DIM + c] = (A.rho * (u0[c] / A.dt - Gu) - gp[c] + (A.g[c] + bf) * A.rho) * JxW;
      }
    } else { // :295-302
      double div = 0, gpu = 0;
      for (int c = 0; c < DIM; ++c) { div += G[c * DIM + c]; gpu += gp[c] * u[c]; }
      S.f[q * DIM] = (-kCpToCv * (kAtm + p) * div + p0 / A.dt - gpu) / kAtm * JxW;
    }
  }
  __syncthreads();
  const int NF = vel ? NU * DIM : NU;
  for (int i = lane; i < NF; i += LPC) {
    const int a = vel ? i / DIM : i, c = vel ? i - a * DIM : 0;
    double s = 0;
    for (int q = 0; q < NQ; ++q) s += T.phi[q * NU + a] * S.f[q * DIM + c];
    S.fe[i] = s;
  }
  __syncthreads();
  // Neumann faces (:312-340)
  if (vel && A.n_neumann != 0 && active) neumann_faces<DIM, NU>(A, T, cc, S.X, lane, LPC, S.fe);
  __syncthreads();
  if (!active) return;
  for (int i = lane; i < NF; i += LPC) {
    const int a = vel ? i / DIM : i, c = vel ? i - a * DIM : 0;
    unsafeAtomicAdd(&A.rhs[vel ? int64_t(DIM) * S.un[a] + c : int64_t(S.un[a])], S.fe[i]);
  }
}

template <int DIM, int KV>
void launch_setup_t(ifem_ctx *ctx, const ExArgs &A) {
  constexpr int WPB = (DIM == 3 && KV == 2) ? 2 : 4;
  const size_t smem = WPB * sizeof(ExSetupScratch<DIM, KV>);
  IFEM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ex_setup<DIM, KV, WPB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL((k_ex_setup<DIM, KV, WPB>), dim3(unsigned((A.n_cells + WPB - 1) / WPB)), dim3(64 * WPB), smem, ctx->stream, A);
  IFEM_HIP_CHECK(hipGetLastError());
}
template <int DIM, int KV>
void launch_rhs_t(ifem_ctx *ctx, const ExArgs &A) {
  constexpr int NQ = Geo<DIM, KV>::NQ;
  constexpr int LPC = NQ <= 4 ? 4 : NQ <= 8 ? 8 : NQ <= 16 ? 16 : 32, CPB = 256 / LPC;
  static_assert(NQ <= LPC, "a lane per quadrature point");
  const size_t smem = CPB * sizeof(ExRhsScratch<DIM, KV>);
  IFEM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ex_rhs<DIM, KV, LPC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL((k_ex_rhs<DIM, KV, LPC>), dim3(unsigned((A.n_cells + CPB - 1) / CPB)), dim3(256), smem, ctx->stream, A);
  IFEM_HIP_CHECK(hipGetLastError());
}

// ---- 2. the masked operators on the node pattern are linalg.hip::spmv_node_scalar (apply_op below).  The lift: rhs_c <- P_c (rhs_c - A_v g_c);
// g is zero where no line stands.  16 lanes per row (a Q2 row holds up to 25 / 125 nodes)
template <int DIM>
__global__ __launch_bounds__(256) void k_ex_lift(int64_t n_rows, const int64_t *__restrict__ rp, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                 const uint8_t *__restrict__ flag, const double *__restrict__ g, double *__restrict__ rhs) {
  const int64_t row = (int64_t(blockIdx.x) * 256 + threadIdx.x) >> 4;
  const int lig = threadIdx.x & 15;
  double acc[DIM];
  for (int c = 0; c < DIM; ++c) acc[c] = 0;
  if (row < n_rows) {
    const int64_t rs = rp[row], re = rp[row + 1];
    for (int64_t k = rs + lig; k < re; k += 16) {
      const double a = val[k];
      const int64_t j = int64_t(DIM) * col[k];
      for (int c = 0; c < DIM; ++c) acc[c] += a * g[j + c];
    }
  }
  for (int c = 0; c < DIM; ++c)
    for (int o = 8; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 16);
  if (lig == 0 && row < n_rows)
    for (int c = 0; c < DIM; ++c) {
      const int64_t i = int64_t(DIM) * row + c;
      rhs[i] = flag[i] ? 0.0 : rhs[i] - acc[c];
    }
}

// the Jacobi diagonal of the stacked velocity system: diag(A_v) once per component
__global__ void k_ex_stack_diag(int64_t n_nodes, int dim, const double *__restrict__ d, double *__restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n_nodes * dim) out[i] = d[i / dim];
}

// the two norms of an outer iteration in one pass: out[0] += |eval - last|^2, out[1] += |eval|^2, last = eval (:482-489,500)
__global__ __launch_bounds__(256) void k_ex_norms(int64_t n, const double *__restrict__ ev, double *__restrict__ last, double *__restrict__ out) {
  __shared__ double sh[2][4];
  double a = 0, b = 0;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
    const double e = ev[i], d = e - last[i];
    a += d * d; b += e * e;
    last[i] = e;
  }
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsafeAtomicAdd(&out[0], sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3]);
    unsafeAtomicAdd(&out[1], sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]);
  }
}

void check_params(const ifem_scns_params *p) {
  if (!p || !(p->dt > 0) || !(p->viscosity > 0) || !(p->rho > 0)) throw Error(IFEM_E_BADPARAM, "ifem_scnsex_*: bad ifem_scns_params (dt, viscosity and rho must be positive)");
  if (p->n_neumann < 0 || p->n_neumann > 8) throw Error(IFEM_E_BADPARAM, "ifem_scnsex_*: ifem_scns_params.n_neumann outside [0, 8]");
}

void apply_op(ifem_ctx *ctx, bool velocity, const double *x, double *y) {
  ExState &ex = ctx->ex;
  KScope ks(ctx, IFEM_KC_OTHER, double(ctx->Auu.nnzb) * 12 + double(ctx->nUo) * 24 * (velocity ? ctx->dim : 1));
  if (!velocity) spmv_node_scalar(ctx, 1, ex.ap.p, nullptr, ex.dpn.p, x, y);
  else spmv_node_scalar(ctx, ctx->dim, ex.av.p, ctx->has_c[1] ? ctx->is_c[1].p : nullptr, ex.dvn.p, x, y);
}

void fill_args(ifem_ctx *ctx, const ifem_scns_params *p, ExArgs &A) {
  A.n_cells = ctx->n_cells; A.p_off = int64_t(ctx->dim) * ctx->nUl;
  A.fe = ctx->d_fe.p;
  A.vcoords = ctx->vcoords.p; A.cell_unodes = ctx->cell_unodes.p; A.cell_face_bid = ctx->cell_face_bid.p;
  A.posUU = ctx->posUU.p; A.rp = ctx->Auu.rowptr.p;
  A.sigma = ctx->sigma_pml.n ? ctx->sigma_pml.p : nullptr;
  A.body_force = ctx->body_force.n ? ctx->body_force.p : nullptr;
  A.mu = p->viscosity; A.rho = p->rho; A.dt = p->dt;
  for (int i = 0; i < 3; ++i) A.g[i] = p->gravity[i];
  A.n_neumann = p->n_neumann;
  for (int i = 0; i < 8; ++i) { A.neumann_id[i] = p->neumann_id[i]; A.neumann_p[i] = p->neumann_p[i]; }
}

} // namespace

// every entry point: what the solver does not cover is refused before anything is allocated or launched
void scnsex_check(ifem_ctx *ctx) {
  if (ctx->hang.n > 0 || ctx->hang.active)
    throw Error(IFEM_E_BADPARAM, "ifem_scnsex_*: contexts with hanging nodes are not supported by the explicit solver");
  if (ctx->halo.nranks > 1) throw Error(IFEM_E_BADPARAM, "ifem_scnsex_*: partitioned contexts are not supported by the explicit solver (single rank only)");
  if (ctx->dim < 2 || ctx->dim > 3 || ctx->kv < 1 || ctx->kv > 2) throw Error(IFEM_E_BADPARAM, "unsupported (dim, kv)");
  ExState &ex = ctx->ex;
  if (ex.equal_order == 0) { // decided once: the mesh tables never change
    if (ctx->nPl != ctx->nUl || ctx->nPo != ctx->nUo) ex.equal_order = -1;
    else {
      const auto cu = ctx->cell_unodes.download(ctx->stream);
      const auto cp = ctx->cell_pnodes.download(ctx->stream);
      const int nu = ctx->nu, np = ctx->np, n1 = ctx->kv + 1;
      ex.equal_order = 1;
      for (int64_t c = 0; c < ctx->n_cells && ex.equal_order == 1; ++c)
        for (int v = 0; v < np; ++v) {
          int a = 0, stride = 1; // local node at vertex v
          for (int d = 0; d < ctx->dim; ++d) { a += ((v >> d) & 1) * ctx->kv * stride; stride *= n1; }
          if (cp[c * np + v] != cu[c * nu + a]) { ex.equal_order = -2; break; }
        }
    }
  }
  if (ex.equal_order == -1)
    throw Error(IFEM_E_BADPARAM, "ifem_scnsex_*: velocity degree must be the same as pressure (kv != kp: this context has " + std::to_string(ctx->nUl) +
                                     " velocity and " + std::to_string(ctx->nPl) + " pressure nodes, a Taylor-Hood pair)");
  if (ex.equal_order == -2)
    throw Error(IFEM_E_BADPARAM, "ifem_scnsex_*: the velocity and pressure node tables differ (cell_pnodes must be the vertex nodes of cell_unodes)");
}

// A_v, A_p and their diagonals; re-integrated only when mu, rho, dt, the PML field or the order of the pattern's rows changed
void scnsex_setup(ifem_ctx *ctx, const ifem_scns_params *p) {
  scnsex_check(ctx);
  check_params(p);
  ExState &ex = ctx->ex;
  if (ex.ready && ex.key[0] == p->viscosity && ex.key[1] == p->rho && ex.key[2] == p->dt && ex.key_fields == ex.fields_version &&
      ex.order == ctx->Auu.order_version)
    return;
  hipStream_t s = ctx->stream;
  const size_t nnz = (size_t)ctx->Auu.nnzb, n = (size_t)ctx->nUl, dim = (size_t)ctx->dim;
  if (ex.av.n != nnz) { ex.av.alloc(nnz, "the SCnsEX velocity matrix"); ex.ap.alloc(nnz, "the SCnsEX pressure matrix"); }
  if (ex.dvn.n != n) {
    ex.dvn.alloc(n); ex.dpn.alloc(n); ex.dvs.alloc(dim * n);
    for (auto &w : ex.w) w.alloc(dim * n);
    ex.last.alloc((dim + 1) * n);
    ex.red.alloc(2);
  }
  ex.ready = false;
  {
    KScope ks(ctx, IFEM_KC_ZERO_FILL, double(2 * nnz + 2 * n) * 8);
    IFEM_HIP_CHECK(hipMemsetAsync(ex.av.p, 0, nnz * sizeof(double), s));
    IFEM_HIP_CHECK(hipMemsetAsync(ex.ap.p, 0, nnz * sizeof(double), s));
    IFEM_HIP_CHECK(hipMemsetAsync(ex.dvn.p, 0, n * sizeof(double), s));
    IFEM_HIP_CHECK(hipMemsetAsync(ex.dpn.p, 0, n * sizeof(double), s));
  }
  ExArgs A{};
  fill_args(ctx, p, A);
  A.av = ex.av.p; A.ap = ex.ap.p; A.dv = ex.dvn.p; A.dp = ex.dpn.p;
  {
    const int nu = ctx->nu;
    KScope ks(ctx, IFEM_KC_ASSEMBLE, double(nnz) * 16 + double(ctx->n_cells) * (double(nu) * nu * 2 + double(nu) * 4 + ctx->np * ctx->dim * 8));
    if (ctx->n_cells > 0) pick(ctx->dim, ctx->kv, launch_setup_t<2, 1>, launch_setup_t<2, 2>, launch_setup_t<3, 1>, launch_setup_t<3, 2>)(ctx, A);
    if (n > 0) hipLaunchKernelGGL(k_ex_stack_diag, dim3(grid_for(int64_t(dim * n))), dim3(256), 0, s, (int64_t)n, (int)dim, ex.dvn.p, ex.dvs.p);
    IFEM_HIP_CHECK(hipGetLastError());
  }
  ex.key[0] = p->viscosity; ex.key[1] = p->rho; ex.key[2] = p->dt;
  ex.key_fields = ex.fields_version;
  ex.order = ctx->Auu.order_version;
  ex.ready = true;
}

// the explicit side of the velocity (lift included) or the pressure equation at IFEM_VEC_EVAL / IFEM_VEC_PRESENT into its block of IFEM_VEC_RHS
void scnsex_assemble_rhs(ifem_ctx *ctx, const ifem_scns_params *p, int velocity) {
  scnsex_setup(ctx, p); // (checks; the lift reads A_v)
  ExState &ex = ctx->ex;
  hipStream_t s = ctx->stream;
  const int dim = ctx->dim;
  const int64_t n = ctx->nUl, nv = int64_t(dim) * n;
  double *rhs = ctx->vec[IFEM_VEC_RHS].p + (velocity ? 0 : nv);
  {
    KScope ks(ctx, IFEM_KC_ZERO_FILL, double(velocity ? nv : n) * 8);
    IFEM_HIP_CHECK(hipMemsetAsync(rhs, 0, size_t(velocity ? nv : n) * sizeof(double), s));
  }
  ExArgs A{};
  fill_args(ctx, p, A);
  A.eval = ctx->vec[IFEM_VEC_EVAL].p; A.present = ctx->vec[IFEM_VEC_PRESENT].p;
  A.rhs = rhs;
  A.velocity = velocity ? 1 : 0;
  {
    KScope ks(ctx, IFEM_KC_ASSEMBLE, double(ctx->n_cells) * ctx->nu * (4 + 8.0 * (2 * (dim + 1) + (velocity ? dim : 1))));
    if (ctx->n_cells > 0) pick(dim, ctx->kv, launch_rhs_t<2, 1>, launch_rhs_t<2, 2>, launch_rhs_t<3, 1>, launch_rhs_t<3, 2>)(ctx, A);
  }
  if (velocity && ctx->has_c[1] && ctx->nUo > 0) {
    KScope ks(ctx, IFEM_KC_OTHER, double(ctx->Auu.nnzb) * 12 + double(nv) * 25);
    const dim3 g(grid_for(ctx->nUo * 16)), b(256);
    if (dim == 2) hipLaunchKernelGGL((k_ex_lift<2>), g, b, 0, s, ctx->nUo, ctx->Auu.rowptr.p, ctx->Auu.col.p, ex.av.p, ctx->is_c[1].p, ctx->cval[1].p, rhs);
    else hipLaunchKernelGGL((k_ex_lift<3>), g, b, 0, s, ctx->nUo, ctx->Auu.rowptr.p, ctx->Auu.col.p, ex.av.p, ctx->is_c[1].p, ctx->cval[1].p, rhs);
  }
  IFEM_HIP_CHECK(hipGetLastError());
}

// PETScWrappers::SolverCG of :396-422 on the block of IFEM_VEC_RHS into the block of IFEM_VEC_UPDATE (intermediate_solution), then
// nonzero_constraints.distribute (:424).  The velocity block is ONE CG over the stacked dim * n vector, as block(0,0) is one system
void scnsex_solve(ifem_ctx *ctx, int velocity, uint32_t *iters, double *res_out) {
  scnsex_check(ctx);
  ExState &ex = ctx->ex;
  if (!ex.ready) throw Error(IFEM_E_BADPARAM, "ifem_scnsex_solve called before ifem_scnsex_setup");
  if (ex.order != ctx->Auu.order_version)
    throw Error(IFEM_E_BADPARAM, "ifem_scnsex_solve: the A_uu row order changed since ifem_scnsex_setup (first stored fluid assembly): set up again");
  const int64_t nn = ctx->nUl, nv = int64_t(ctx->dim) * nn;
  const int64_t n = velocity ? nv : nn;
  const double *b = ctx->vec[IFEM_VEC_RHS].p + (velocity ? 0 : nv);
  double *x = ctx->vec[IFEM_VEC_UPDATE].p + (velocity ? 0 : nv);
  const bool vel = velocity != 0;
  const OpFn Aop = [ctx, vel](const double *xx, double *yy) { apply_op(ctx, vel, xx, yy); };
  const double bn = std::sqrt(v_dot(ctx, n, b, b));
  const double tol = 1e-6 * bn; // :396-397
  const int maxit = (int)std::min<int64_t>(ctx->n_local, 1 << 30); // system_matrix.m()
  const int it = cg_device(ctx, n, Aop, vel ? ex.dvs.p : ex.dpn.p, b, x, tol, maxit, ex.w[0].p, ex.w[1].p, ex.w[2].p, ex.w[3].p, 4, ex.w[4].p);
  const double res = std::sqrt(cgd_rr(ctx));
  if (vel && ctx->has_c[1]) {
    KScope ks(ctx, IFEM_KC_OTHER, double(nv));
    distribute_lines(ctx, nv, nv, 0, ctx->is_c[1].p, ctx->cval[1].p, x);
  }
  IFEM_HIP_CHECK(hipGetLastError());
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (iters) *iters = (uint32_t)it;
  if (res_out) *res_out = res;
  if (!(res <= tol)) throw_noconv(vel ? "SCnsEX velocity CG" : "SCnsEX pressure CG", it, res, tol);
}

// the outer loop of run_one_step (:448-503): present is replaced by the converged evaluation point
void scnsex_step(ifem_ctx *ctx, const ifem_scns_params *p, double tolerance, int max_iterations, ifem_scnsex_stats *stats) {
  scnsex_setup(ctx, p);
  ExState &ex = ctx->ex;
  hipStream_t s = ctx->stream;
  const int64_t nn = ctx->nUl, nv = int64_t(ctx->dim) * nn, n = nv + nn;
  double *ev = ctx->vec[IFEM_VEC_EVAL].p, *upd = ctx->vec[IFEM_VEC_UPDATE].p;
  v_copy(ctx, n, ctx->vec[IFEM_VEC_PRESENT].p, ev); // evaluation_point = present_solution (:452)
  v_zero(ctx, n, ex.last.p);
  double cur = 1.0, init = 1.0, rel = 1.0; // :448-450
  uint32_t outer = 0, vit = 0, pit = 0;
  double vres = 0, pres = 0;
  while (rel > tolerance && cur > 1e-12) {
    if ((int64_t)outer >= (int64_t)max_iterations) throw Error(IFEM_E_NEWTON_MAXIT, "Too many iterations!"); // :462-463
    scnsex_assemble_rhs(ctx, p, 1);
    scnsex_solve(ctx, 1, &vit, &vres);
    v_copy(ctx, nv, upd, ev); // :476 -- the pressure side sees the new velocity
    scnsex_assemble_rhs(ctx, p, 0);
    scnsex_solve(ctx, 0, &pit, &pres);
    v_copy(ctx, nn, upd + nv, ev + nv);
    double h[2];
    {
      KScope ks(ctx, IFEM_KC_VECTOR, double(n) * 24);
      IFEM_HIP_CHECK(hipMemsetAsync(ex.red.p, 0, 2 * sizeof(double), s));
      hipLaunchKernelGGL(k_ex_norms, dim3(std::min(grid_for(n), 1024u)), dim3(256), 0, s, n, ev, ex.last.p, ex.red.p);
      IFEM_HIP_CHECK(hipGetLastError());
    }
    IFEM_HIP_CHECK(hipMemcpyAsync(h, ex.red.p, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s)); // the one host wait of the outer iteration's norms
    cur = std::sqrt(h[0]);
    if (outer == 0) init = std::sqrt(h[1]);
    rel = cur / init; // init == 0 gives NaN, which ends the loop: the reference's outcome for a state at rest
    ++outer;
  }
  v_copy(ctx, n, ev, ctx->vec[IFEM_VEC_PRESENT].p); // :503
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  if (stats) {
    stats->outer_iterations = outer;
    stats->vel_iters = vit; stats->pre_iters = pit;
    stats->vel_res = vres; stats->pre_res = pres;
    stats->abs_res = cur; stats->rel_res = rel;
  }
}

} // namespace ifem
