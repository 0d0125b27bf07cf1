// transfer.hip -- SolutionTransfer::interpolate for FE_Q between two meshes of one box (FluidSolver::refine_mesh,
// source/mpi_fluid_solver.cpp:449-481): every node of the new mesh takes the value of the old finite-element function at that node.
// The host names, per new node, an old cell whose closure holds it and the node's position in that cell in units of 1 / (2 deg)
// (host/refine.cpp::make_transfer_table; ifem_hip.h, ifem_transfer_solution); the weights of the tensor-product Lagrange basis at
// such a dyadic point are exact in binary, and terms of weight 0 are skipped, so a node of both meshes keeps its value bit for bit.
#include <hip/hip_runtime.h>
#include <vector>
#include "ctx.hpp"
#include "kernels.hpp"

namespace ifem {

// the deg + 1 Lagrange polynomials on the nodes j / deg at t = p / (2 deg): every factor (t - x_m) / (x_j - x_m) is a small dyadic number
__device__ inline void dyadic_lagrange(int deg, int p, double *w) {
  const double t = double(p) / double(2 * deg);
  for (int j = 0; j <= deg; ++j) {
    double v = 1.0;
    for (int m = 0; m <= deg; ++m)
      if (m != j) v *= (t - double(m) / deg) / (double(j) / deg - double(m) / deg);
    w[j] = v;
  }
}

// one thread per new node: velocity nodes [0, nU) write their DIM components, pressure nodes [nU, nU + nP) their entry of the pressure block
template <int DIM>
__global__ void k_transfer_solution(int64_t nU, int64_t nP, int kv, const int32_t *__restrict__ u_cell, const int32_t *__restrict__ u_pos,
                                    const int32_t *__restrict__ p_cell, const int32_t *__restrict__ p_pos,
                                    const int32_t *__restrict__ src_unodes, const int32_t *__restrict__ src_pnodes, int64_t src_nU,
                                    const double *__restrict__ xs, double *__restrict__ xd) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= nU + nP) return;
  const bool vel = i < nU;
  const int deg = vel ? kv : 1, n1 = deg + 1;
  int nn = 1;
  for (int d = 0; d < DIM; ++d) nn *= n1;
  const int64_t k = vel ? i : i - nU;
  const int32_t cell = vel ? u_cell[k] : p_cell[k], pos = vel ? u_pos[k] : p_pos[k];
  const int32_t *nodes = (vel ? src_unodes : src_pnodes) + int64_t(cell) * nn;
  double w1[3][3];
  for (int d = 0; d < DIM; ++d) dyadic_lagrange(deg, (pos >> (8 * d)) & 0xff, w1[d]);
  const int ncomp = vel ? DIM : 1;
  double s[DIM];
  bool any = false;
  for (int c = 0; c < DIM; ++c) s[c] = 0.0;
  for (int a = 0; a < nn; ++a) {
    int r = a;
    double w = 1.0;
    for (int d = 0; d < DIM; ++d) { w *= w1[d][r % n1]; r /= n1; }
    if (w == 0.0) continue;
    const int64_t base = vel ? int64_t(DIM) * nodes[a] : int64_t(DIM) * src_nU + nodes[a];
    for (int c = 0; c < ncomp; ++c) s[c] = any ? s[c] + w * xs[base + c] : w * xs[base + c]; // (the first term as it is: keeps -0.0)
    any = true;
  }
  if (vel) for (int c = 0; c < DIM; ++c) xd[int64_t(DIM) * k + c] = s[c];
  else xd[int64_t(DIM) * nU + k] = s[0];
}

void transfer_solution(ifem_ctx *src, ifem_ctx *dst, int vec, const int32_t *u_cell, const int32_t *u_pos, const int32_t *p_cell,
                       const int32_t *p_pos) {
  if (!src || !dst || src == dst) throw Error(IFEM_E_BADPARAM, "ifem_transfer_solution: two different contexts");
  if (src->halo.nranks > 1 || dst->halo.nranks > 1) throw Error(IFEM_E_BADPARAM, "ifem_transfer_solution: single-rank contexts only");
  if (src->dim != dst->dim || src->kv != dst->kv || src->device != dst->device)
    throw Error(IFEM_E_BADPARAM, "ifem_transfer_solution: the contexts must share dimension, velocity degree and device");
  if (!u_cell || !u_pos || !p_cell || !p_pos) throw Error(IFEM_E_BADPARAM, "ifem_transfer_solution: null table");
  if (dst->kv != 1 && dst->kv != 2) throw Error(IFEM_E_BADPARAM, "ifem_transfer_solution: velocity degree 1 or 2");
  const int dim = dst->dim;
  auto check = [&](const int32_t *cell, const int32_t *pos, int64_t n, int deg) {
    for (int64_t i = 0; i < n; ++i) {
      if (cell[i] < 0 || cell[i] >= src->n_cells) throw Error(IFEM_E_BADPARAM, "ifem_transfer_solution: old cell out of range");
      bool ok = pos[i] >= 0 && (pos[i] >> (8 * dim)) == 0;
      for (int d = 0; d < dim; ++d) ok = ok && ((pos[i] >> (8 * d)) & 0xff) <= 2 * deg;
      if (!ok) throw Error(IFEM_E_BADPARAM, "ifem_transfer_solution: node position out of range (0 ... 2 deg per direction)");
    }
  };
  check(u_cell, u_pos, dst->nUl, dst->kv);
  check(p_cell, p_pos, dst->nPl, 1);
  DBuf<int32_t> d_uc, d_up, d_pc, d_pp;
  hipStream_t s = dst->stream;
  d_uc.upload(u_cell, size_t(dst->nUl), s); d_up.upload(u_pos, size_t(dst->nUl), s);
  d_pc.upload(p_cell, size_t(dst->nPl), s); d_pp.upload(p_pos, size_t(dst->nPl), s);
  IFEM_HIP_CHECK(hipStreamSynchronize(src->stream)); // whatever wrote the source vector has finished
  const int64_t n = dst->nUl + dst->nPl;
  if (n) {
    // algorithmic bytes: the table, the result, and the source vector once
    KScope ks(dst, IFEM_KC_REFINE, 8.0 * double(n) + 8.0 * double(dst->n_local) + 8.0 * double(src->n_local));
    const dim3 grid(unsigned((n + 255) / 256)), block(256);
    if (dim == 3)
      hipLaunchKernelGGL((k_transfer_solution<3>), grid, block, 0, s, dst->nUl, dst->nPl, dst->kv, d_uc.p, d_up.p, d_pc.p, d_pp.p,
                         src->cell_unodes.p, src->cell_pnodes.p, src->nUl, src->vec[vec].p, dst->vec[vec].p);
    else
      hipLaunchKernelGGL((k_transfer_solution<2>), grid, block, 0, s, dst->nUl, dst->nPl, dst->kv, d_uc.p, d_up.p, d_pc.p, d_pp.p,
                         src->cell_unodes.p, src->cell_pnodes.p, src->nUl, src->vec[vec].p, dst->vec[vec].p);
    IFEM_HIP_CHECK(hipGetLastError());
  }
  IFEM_HIP_CHECK(hipStreamSynchronize(s)); // the tables are locals
}

} // namespace ifem
