// sa_wall.hip -- the wall function of Fluid::MPI::SpalartAllmaras at a moving FSI wall, on gfx950: what MPI::FSI does between its device-side
// inputs in every time step (mpi_fsi.cpp:782-844, 655-660, 1199-1203).
//   sa_set_moving_wall()             the solid-side lists (wall vertices, their normals, the 2D boundary edges), shear velocities = 0,
//                                    moving distance absent, y+ = 201 (mpi_spalart_allmaras.cpp:427-430)
//   sa_update_shear_velocity()       find_solid_bc, mpi_fsi.cpp:782-844: the fluid velocity at every wall vertex (or its image point) through the
//                                    locator of ifem_fsi_fluid_at_points, tangential speed, get_shear_velocity (sa_wall_function.hpp)
//   sa_update_moving_wall_distance() update_moving_wall_distance (:17-127): brute force over nodes x (edges, vertices), exact on every node
//   sa_update_boundary_condition()   update_boundary_condition (:130-215) on the model's two constraint objects
// Scope: single-rank contexts without hanging-node lines.  The reference sums per-rank shear velocities that treat "not found" as 0; a point in
// the ghost layer of a partitioned context would be found, and counted, twice.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <numeric>
#include <vector>
#include "assemble_common.hpp"
#include "kernels.hpp"
#include "sa_wall_function.hpp"

namespace ifem {

namespace {

constexpr int kTile = 256;
constexpr int kEdgeRec = 7; // v1x v1y v2x v2y utau1 utau2 |v2 - v1|^2

// sample point of every wall vertex: the vertex itself (as mpi_fsi.cpp:810-814 is written) or vertex + image_distance * normal (:807)
__global__ __launch_bounds__(256) void k_sa_sample_points(int32_t n, int dim, const int32_t *__restrict__ vertex, const double *__restrict__ vert,
                                                          const double *__restrict__ normal, double image_distance, int at_image, double *__restrict__ pts) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int d = 0; d < dim; ++d) {
    const double v = vert[(size_t)vertex[i] * dim + d];
    pts[(size_t)i * dim + d] = at_image ? v + image_distance * normal[(size_t)i * dim + d] : v;
  }
}

// one lane per wall vertex (:815-841): |u - (n . u) n| and the Newton solve from the previous shear velocity; a point in no cell gives 0
__global__ __launch_bounds__(256) void k_sa_shear_velocity(int32_t n, int dim, const double *__restrict__ val, const int32_t *__restrict__ cell,
                                                           const double *__restrict__ normal, double nu, double image_distance, double *__restrict__ utau) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (cell[i] < 0) { utau[i] = 0.0; return; }
  double ndotu = 0;
  for (int d = 0; d < dim; ++d) ndotu += normal[(size_t)i * dim + d] * val[(size_t)i * (dim + 1) + d];
  double t2 = 0;
  for (int d = 0; d < dim; ++d) {
    const double t = val[(size_t)i * (dim + 1) + d] - ndotu * normal[(size_t)i * dim + d];
    t2 += t * t;
  }
  utau[i] = sa_shear_velocity(nu, image_distance, sqrt(t2), utau[i]);
}

// the records k_sa_moving_wall streams, rebuilt from the solid's current position and the current shear velocities
__global__ __launch_bounds__(256) void k_sa_wall_records(int32_t ne, int32_t nv, int dim, const int32_t *__restrict__ edge, const int32_t *__restrict__ by_id,
                                                         const int32_t *__restrict__ vertex, const double *__restrict__ vert, const double *__restrict__ utau,
                                                         double *__restrict__ erec, double *__restrict__ vrec) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ne) { // dim == 2
    const int32_t p1 = edge[2 * i], p2 = edge[2 * i + 1];
    const double *v1 = vert + (size_t)vertex[p1] * 2, *v2 = vert + (size_t)vertex[p2] * 2;
    const double dx = v2[0] - v1[0], dy = v2[1] - v1[1];
    const double measure = sqrt(dx * dx + dy * dy); // s_face->measure()
    double *r = erec + (size_t)i * kEdgeRec;
    r[0] = v1[0]; r[1] = v1[1]; r[2] = v2[0]; r[3] = v2[1];
    r[4] = utau[p1]; r[5] = utau[p2];
    r[6] = measure * measure;
  }
  if (i < nv) {
    const int32_t p = by_id[i];
    for (int d = 0; d < dim; ++d) vrec[(size_t)i * (dim + 1) + d] = vert[(size_t)vertex[p] * dim + d];
    vrec[(size_t)i * (dim + 1) + dim] = utau[p];
  }
}

// update_moving_wall_distance (:17-127).  One lane per local node, 256 per workgroup; the edge records, then the vertex records, go through LDS in
// tiles of 256 (every lane reads the same record: a broadcast, no bank conflict).  Each lane carries (best distance, u_tau at the best) through both
// loops; a candidate replaces the minimum only if strictly smaller, so on ties the earliest in the reference's order stands.  The edge distance is
// formed as the reference forms it.  The vertex loop compares squared distances and takes one square root at its end, as k_sa_wall_distance argues;
// its winner then meets the edge minimum in the reference's comparison.
template <int DIM>
__global__ __launch_bounds__(256) void k_sa_moving_wall(int64_t n_nodes, const double *__restrict__ xn, int32_t ne, const double *__restrict__ erec, int32_t nv,
                                                        const double *__restrict__ vrec, double nu, const double *__restrict__ d_fixed,
                                                        double *__restrict__ d_mov, double *__restrict__ yplus, double *__restrict__ d_eff) {
  constexpr int VR = DIM + 1;
  __shared__ double tile[kTile * (DIM == 2 ? kEdgeRec : VR)];
  const int64_t nd = int64_t(blockIdx.x) * kTile + threadIdx.x;
  const bool live = nd < n_nodes;
  double x[DIM];
  for (int d = 0; d < DIM; ++d) x[d] = live ? xn[nd * DIM + d] : 0.0;
  double best = DBL_MAX, ut_best = 0.0;
  if constexpr (DIM == 2) {
    for (int32_t base = 0; base < ne; base += kTile) {
      const int cnt = ne - base < kTile ? ne - base : kTile;
      __syncthreads();
      for (int i = threadIdx.x; i < cnt * kEdgeRec; i += kTile) tile[i] = erec[(size_t)base * kEdgeRec + i];
      __syncthreads();
      for (int i = 0; i < cnt; ++i) {
        const double *r = tile + i * kEdgeRec;
        const double v1x = r[0], v1y = r[1], v2x = r[2], v2y = r[3];
        const double p1 = (v1x - x[0]) * (v1x - v2x) + (v1y - x[1]) * (v1y - v2y); // dot_product(v1, v0, v2)
        const double p2 = (v2x - x[0]) * (v2x - v1x) + (v2y - x[1]) * (v2y - v1y); // dot_product(v2, v0, v1)
        if (p1 > 0 && p2 > 0) {
          const double ratio = p1 / r[6];
          const double fx = x[0] - (v1x + ratio * (v2x - v1x)), fy = x[1] - (v1y + ratio * (v2y - v1y));
          const double cur = sqrt(fx * fx + fy * fy);
          if (cur < best) {
            best = cur;
            ut_best = r[4] + (r[5] - r[4]) * ratio;
          }
        }
      }
    }
  }
  double best2 = DBL_MAX, ut_v = 0.0;
  for (int32_t base = 0; base < nv; base += kTile) {
    const int cnt = nv - base < kTile ? nv - base : kTile;
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * VR; i += kTile) tile[i] = vrec[(size_t)base * VR + i];
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      double cur = 0;
      for (int d = 0; d < DIM; ++d) { const double t = x[d] - tile[i * VR + d]; cur += t * t; }
      if (cur < best2) { best2 = cur; ut_v = tile[i * VR + DIM]; }
    }
  }
  if (nv > 0) {
    const double dv = sqrt(best2);
    if (dv < best) { best = dv; ut_best = ut_v; }
  }
  if (!live) return;
  d_mov[nd] = best;
  yplus[nd] = best * ut_best / nu;
  const double df = d_fixed[nd];
  d_eff[nd] = best < df ? best : df;
}

__global__ __launch_bounds__(256) void k_sa_d_eff(int64_t n, const double *__restrict__ d_mov, const double *__restrict__ d_fixed, double *__restrict__ d_eff) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) d_eff[i] = d_mov[i] < d_fixed[i] ? d_mov[i] : d_fixed[i];
}

__global__ __launch_bounds__(256) void k_sa_fill(int64_t n, double v, double *__restrict__ x) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) x[i] = v;
}

// first touch over (cell, local node), as fsi.hip::k_fsi_first_touch.  pass 0: the smallest order among ALL cells that touch the node, and bit 0 of
// `flags` where an indicator cell touches it; pass 1: bit 1 where the cell of that smallest order is an indicator cell
__global__ __launch_bounds__(256) void k_sa_bc_first_touch(int pass, int64_t n_entries, int nu, const int32_t *__restrict__ cell_unodes,
                                                           const int32_t *__restrict__ indicator, const int32_t *__restrict__ cell_order,
                                                           uint32_t *__restrict__ order_min, uint32_t *__restrict__ flags) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= n_entries) return;
  const int64_t c = t / nu;
  const uint32_t ord = cell_order ? (uint32_t)cell_order[c] : (uint32_t)c;
  const int32_t node = cell_unodes[t];
  const bool ind = indicator[c] == 1;
  if (pass == 0) {
    atomicMin(&order_min[node], ord);
    if (ind) atomicOr(&flags[node], 1u);
  } else if (ind && order_min[node] == ord)
    atomicOr(&flags[node], 2u);
}

// one lane per node, both objects (:163-214 with right_object_wins: the line replaces a boundary line on the same node)
__global__ __launch_bounds__(256) void k_sa_bc_lines(int64_t n, const uint32_t *__restrict__ flags, const double *__restrict__ d_mov, const double *__restrict__ yplus,
                                                     const double *__restrict__ nu_present, double wall_function_distance, double mu, double rho,
                                                     uint8_t *__restrict__ is_c0, double *__restrict__ cval0, uint8_t *__restrict__ is_c1, double *__restrict__ cval1,
                                                     unsigned long long *__restrict__ count) {
  const int64_t nd = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (nd >= n) return;
  constexpr double kappa = 0.41;
  const uint32_t f = flags[nd];
  const double d = d_mov[nd] == DBL_MAX ? 2.0 : d_mov[nd]; // moving_wall_distance.value_or(2.0)
  const bool qualifies = d < wall_function_distance && yplus[nd] < 200.0;
  double v;
  if ((f & 1u) && !(qualifies && !(f & 2u))) v = -nu_present[nd];
  else if (qualifies) v = kappa * yplus[nd] * mu / rho - nu_present[nd];
  else return;
  is_c0[nd] = 1; cval0[nd] = 0.0;
  is_c1[nd] = 1; cval1[nd] = v;
  atomicAdd(count, 1ull);
}

void wall_check(ifem_ctx *ctx, const ifem_sa_params *p, bool need_wall) {
  sa_check(ctx);
  if (ctx->halo.nranks > 1)
    throw Error(IFEM_E_BADPARAM, "ifem_sa_*: the moving-wall entry points do not support partitioned contexts (a wall vertex in the ghost layer would count twice)");
  if (p && (!(p->dt > 0) || !(p->viscosity > 0) || !(p->rho > 0))) throw Error(IFEM_E_BADPARAM, "bad ifem_sa_params");
  if (!need_wall) return;
  const SaState::MovingWall &W = ctx->sa.mw;
  if (!W.set) throw Error(IFEM_E_BADPARAM, "no moving wall: call ifem_sa_set_moving_wall first");
  if (!ctx->fsi.valid) throw Error(IFEM_E_BADPARAM, "no solid: call ifem_fsi_set_solid first");
  if (W.max_vertex >= ctx->fsi.nv) throw Error(IFEM_E_BADPARAM, "the solid has fewer vertices than the moving wall was set for: call ifem_sa_set_moving_wall again");
}

void fill(ifem_ctx *ctx, DBuf<double> &b, size_t n, double v) {
  if (b.n != n) b.alloc(n);
  if (n) hipLaunchKernelGGL(k_sa_fill, dim3(grid_for((int64_t)n)), dim3(256), 0, ctx->stream, (int64_t)n, v, b.p);
}

} // namespace

void sa_set_moving_wall(ifem_ctx *ctx, const ifem_sa_wall *w) {
  wall_check(ctx, nullptr, false);
  SaState::MovingWall &W = ctx->sa.mw;
  hipStream_t s = ctx->stream;
  if (!w) { // as if no moving wall had ever been set
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
    W.clear();
    return;
  }
  if (!ctx->fsi.valid) throw Error(IFEM_E_BADPARAM, "ifem_sa_set_moving_wall: no solid: call ifem_fsi_set_solid first");
  const int dim = ctx->dim;
  if (w->n_vertices <= 0 || !w->vertex || !w->normal) throw Error(IFEM_E_BADPARAM, "ifem_sa_set_moving_wall: no wall vertices or no normals");
  if (w->n_edges < 0 || (w->n_edges > 0 && (dim != 2 || !w->edge))) throw Error(IFEM_E_BADPARAM, "ifem_sa_set_moving_wall: edges belong to dim 2 and need their list");
  for (int32_t i = 0; i < w->n_vertices; ++i)
    if (w->vertex[i] < 0 || w->vertex[i] >= ctx->fsi.nv) throw Error(IFEM_E_BADPARAM, "ifem_sa_set_moving_wall: wall vertex outside the solid's vertices");
  for (int64_t i = 0; i < 2 * (int64_t)w->n_edges; ++i)
    if (w->edge[i] < 0 || w->edge[i] >= w->n_vertices) throw Error(IFEM_E_BADPARAM, "ifem_sa_set_moving_wall: edge end outside the wall vertex list");
  sa_ensure(ctx);
  const int32_t nv = w->n_vertices, ne = w->n_edges;
  std::vector<int32_t> by_id((size_t)nv);
  std::iota(by_id.begin(), by_id.end(), 0);
  std::stable_sort(by_id.begin(), by_id.end(), [&](int32_t a, int32_t b) { return w->vertex[a] < w->vertex[b]; });
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  W.clear();
  W.nv = nv; W.ne = ne;
  W.max_vertex = *std::max_element(w->vertex, w->vertex + nv);
  W.image_distance = w->image_distance;
  W.wall_function_distance = w->wall_function_distance;
  W.sample_at_image_point = w->sample_at_image_point != 0;
  W.vertex.upload(w->vertex, (size_t)nv, s);
  W.by_id.upload(by_id.data(), (size_t)nv, s);
  W.normal.upload(w->normal, (size_t)nv * dim, s);
  if (ne) W.edge.upload(w->edge, (size_t)2 * ne, s);
  W.utau.alloc((size_t)nv);
  IFEM_HIP_CHECK(hipMemsetAsync(W.utau.p, 0, (size_t)nv * sizeof(double), s)); // shear_velocities.reinit
  fill(ctx, W.d_mov, (size_t)ctx->nUl, DBL_MAX);
  fill(ctx, W.yplus, (size_t)ctx->nUl, 201.0);
  IFEM_HIP_CHECK(hipGetLastError());
  IFEM_HIP_CHECK(hipStreamSynchronize(s)); // the host arrays may go away
  W.set = true;
}

void sa_set_shear_velocities(ifem_ctx *ctx, const double *utau) {
  wall_check(ctx, nullptr, true);
  if (!utau) throw Error(IFEM_E_BADPARAM, "ifem_sa_set_shear_velocities: no values");
  IFEM_HIP_CHECK(hipMemcpyAsync(ctx->sa.mw.utau.p, utau, (size_t)ctx->sa.mw.nv * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

void sa_update_shear_velocity(ifem_ctx *ctx, const ifem_sa_params *p, double *host_out) {
  if (!p) throw Error(IFEM_E_BADPARAM, "bad ifem_sa_params");
  wall_check(ctx, p, true);
  SaState::MovingWall &W = ctx->sa.mw;
  hipStream_t s = ctx->stream;
  const int dim = ctx->dim;
  const int32_t nv = W.nv;
  if (W.pts.n != (size_t)nv * dim) {
    W.pts.alloc((size_t)nv * dim);
    W.val.alloc((size_t)nv * (dim + 1));
    W.cell.alloc((size_t)nv);
  }
  {
    KScope ks(ctx, IFEM_KC_OTHER);
    hipLaunchKernelGGL(k_sa_sample_points, dim3(grid_for(nv)), dim3(256), 0, s, nv, dim, W.vertex.p, ctx->fsi.vert.p, W.normal.p, W.image_distance,
                       W.sample_at_image_point, W.pts.p);
    fsi_fluid_at_points_dev(ctx, nv, W.pts.p, W.val.p, nullptr, W.cell.p);
    hipLaunchKernelGGL(k_sa_shear_velocity, dim3(grid_for(nv)), dim3(256), 0, s, nv, dim, W.val.p, W.cell.p, W.normal.p, p->viscosity / p->rho, W.image_distance,
                       W.utau.p);
    IFEM_HIP_CHECK(hipGetLastError());
  }
  if (host_out) IFEM_HIP_CHECK(hipMemcpyAsync(host_out, W.utau.p, (size_t)nv * sizeof(double), hipMemcpyDeviceToHost, s));
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
}

void sa_update_moving_wall_distance(ifem_ctx *ctx, const ifem_sa_params *p, double *host_d, double *host_yplus) {
  if (!p) throw Error(IFEM_E_BADPARAM, "bad ifem_sa_params");
  wall_check(ctx, p, true);
  sa_ensure(ctx);
  SaState &sa = ctx->sa;
  SaState::MovingWall &W = sa.mw;
  hipStream_t s = ctx->stream;
  const int dim = ctx->dim;
  const int64_t n = ctx->nUl;
  const double *xn = sa_node_points(ctx);
  if (W.vrec.n != (size_t)W.nv * (dim + 1)) W.vrec.alloc((size_t)W.nv * (dim + 1));
  if (W.erec.n != (size_t)W.ne * kEdgeRec) W.erec.alloc((size_t)W.ne * kEdgeRec);
  if (W.d_eff.n != (size_t)n) W.d_eff.alloc((size_t)n);
  {
    KScope ks(ctx, IFEM_KC_OTHER, double(n) * (dim + 4) * 8 + double(W.ne) * kEdgeRec * 8 + double(W.nv) * (dim + 1) * 8);
    hipLaunchKernelGGL(k_sa_wall_records, dim3(grid_for(std::max(W.nv, W.ne))), dim3(256), 0, s, W.ne, W.nv, dim, W.edge.p, W.by_id.p, W.vertex.p, ctx->fsi.vert.p,
                       W.utau.p, W.erec.p, W.vrec.p);
    const double nu = p->viscosity / p->rho;
    if (n > 0) {
      if (dim == 2)
        hipLaunchKernelGGL((k_sa_moving_wall<2>), dim3(grid_for(n)), dim3(kTile), 0, s, n, xn, W.ne, W.erec.p, W.nv, W.vrec.p, nu, sa.wall_d.p, W.d_mov.p, W.yplus.p,
                           W.d_eff.p);
      else
        hipLaunchKernelGGL((k_sa_moving_wall<3>), dim3(grid_for(n)), dim3(kTile), 0, s, n, xn, 0, (const double *)nullptr, W.nv, W.vrec.p, nu, sa.wall_d.p, W.d_mov.p,
                           W.yplus.p, W.d_eff.p);
    }
    IFEM_HIP_CHECK(hipGetLastError());
  }
  W.updated = true;
  if (host_d) IFEM_HIP_CHECK(hipMemcpyAsync(host_d, W.d_mov.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (host_yplus) IFEM_HIP_CHECK(hipMemcpyAsync(host_yplus, W.yplus.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
}

// after ifem_sa_set_wall_points: d_eff follows the new fixed distance
void sa_wall_refresh_d_eff(ifem_ctx *ctx) {
  SaState::MovingWall &W = ctx->sa.mw;
  if (!W.updated) return;
  const int64_t n = ctx->nUl;
  if (n > 0) hipLaunchKernelGGL(k_sa_d_eff, dim3(grid_for(n)), dim3(256), 0, ctx->stream, n, W.d_mov.p, ctx->sa.wall_d.p, W.d_eff.p);
  IFEM_HIP_CHECK(hipGetLastError());
}

void sa_get_moving_wall(ifem_ctx *ctx, double *host_d, double *host_yplus) {
  wall_check(ctx, nullptr, false);
  const SaState::MovingWall &W = ctx->sa.mw;
  const size_t n = (size_t)ctx->nUl;
  if (!W.set) { // absent, and the y+ of setup_cell_property (:427-430)
    if (host_d) std::fill(host_d, host_d + n, DBL_MAX);
    if (host_yplus) std::fill(host_yplus, host_yplus + n, 201.0);
    return;
  }
  if (host_d) IFEM_HIP_CHECK(hipMemcpyAsync(host_d, W.d_mov.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (host_yplus) IFEM_HIP_CHECK(hipMemcpyAsync(host_yplus, W.yplus.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

void sa_update_boundary_condition(ifem_ctx *ctx, const ifem_sa_params *p, int first_step, const int32_t *cell_order, int64_t *n_lines) {
  if (!p) throw Error(IFEM_E_BADPARAM, "bad ifem_sa_params");
  wall_check(ctx, p, true);
  if (ctx->indicator.n != (size_t)ctx->n_cells) throw Error(IFEM_E_BADPARAM, "No available indicator function for SA model! (ifem_fsi_update_indicator / ifem_set_cell_fields)");
  if (cell_order)
    for (int64_t c = 0; c < ctx->n_cells; ++c)
      if (cell_order[c] < 0) throw Error(IFEM_E_BADPARAM, "ifem_sa_update_boundary_condition: negative cell_order");
  sa_ensure(ctx);
  SaState &sa = ctx->sa;
  SaState::MovingWall &W = sa.mw;
  hipStream_t s = ctx->stream;
  const int64_t n = ctx->nUl, entries = ctx->n_cells * ctx->nu;
  DBuf<int32_t> d_order;
  if (cell_order) d_order.upload(cell_order, (size_t)ctx->n_cells, s);
  if (W.order_min.n != (size_t)n) { W.order_min.alloc((size_t)n); W.first_ind.alloc((size_t)n); }
  if (W.count.n != 1) W.count.alloc(1);
  unsigned long long cnt = 0;
  {
    KScope ks(ctx, IFEM_KC_OTHER);
    if (!first_step) { // nonzero_constraints.copy_from(zero_constraints) (:139-143)
      IFEM_HIP_CHECK(hipMemcpyAsync(sa.is_c[1].p, sa.is_c[0].p, (size_t)n, hipMemcpyDeviceToDevice, s));
      IFEM_HIP_CHECK(hipMemsetAsync(sa.cval[1].p, 0, (size_t)n * sizeof(double), s));
      sa.has_c[1] = sa.has_c[0];
    }
    IFEM_HIP_CHECK(hipMemsetAsync(W.order_min.p, 0xFF, (size_t)n * sizeof(uint32_t), s));
    IFEM_HIP_CHECK(hipMemsetAsync(W.first_ind.p, 0, (size_t)n * sizeof(uint32_t), s));
    IFEM_HIP_CHECK(hipMemsetAsync(W.count.p, 0, sizeof(int64_t), s));
    if (entries > 0)
      for (int pass = 0; pass < 2; ++pass)
        hipLaunchKernelGGL(k_sa_bc_first_touch, dim3(grid_for(entries)), dim3(256), 0, s, pass, entries, ctx->nu, ctx->cell_unodes.p, ctx->indicator.p, d_order.p,
                           W.order_min.p, W.first_ind.p);
    if (n > 0)
      hipLaunchKernelGGL(k_sa_bc_lines, dim3(grid_for(n)), dim3(256), 0, s, n, W.first_ind.p, W.d_mov.p, W.yplus.p, sa.vec[IFEM_SA_PRESENT].p, W.wall_function_distance,
                         p->viscosity, p->rho, sa.is_c[0].p, sa.cval[0].p, sa.is_c[1].p, sa.cval[1].p, (unsigned long long *)W.count.p);
    IFEM_HIP_CHECK(hipGetLastError());
    IFEM_HIP_CHECK(hipMemcpyAsync(&cnt, W.count.p, sizeof(cnt), hipMemcpyDeviceToHost, s));
  }
  IFEM_HIP_CHECK(hipStreamSynchronize(s)); // d_order is released on return
  if (cnt) sa.has_c[0] = sa.has_c[1] = true;
  if (n_lines) *n_lines = (int64_t)cnt;
}

void sa_get_constraints(ifem_ctx *ctx, int which, uint8_t *flags, double *inhom) {
  sa_check(ctx);
  if (which < 0 || which > 1) throw Error(IFEM_E_BADPARAM, "ifem_sa_get_constraints: which must be 0 or 1");
  sa_ensure(ctx);
  const SaState &sa = ctx->sa;
  const size_t n = (size_t)ctx->nUl;
  if (flags) IFEM_HIP_CHECK(hipMemcpyAsync(flags, sa.is_c[which].p, n, hipMemcpyDeviceToHost, ctx->stream));
  if (inhom) IFEM_HIP_CHECK(hipMemcpyAsync(inhom, sa.cval[which].p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

} // namespace ifem
