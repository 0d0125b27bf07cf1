// kelly.hip -- KellyErrorEstimator<dim>::estimate on the velocity, the first step of FluidSolver::refine_mesh
// (source/mpi_fluid_solver.cpp:422-430): for every cell K
//     eta_K = sqrt( h_K / 24 * sum_{F in dK} int_F sum_{c < dim} [d u_c / d n]^2 ds ),
// face quadrature QGauss<dim-1>(kv + 1) (face_quad_formula, :35), strategy cell_diameter_over_24, no Neumann map (a boundary face
// contributes 0), no coefficient.  The formula restates the documented behaviour of deal.II from memory ([3P-memory] in SURVEY): deal.II
// is not in the reference tree, nothing here was compared with a deal.II run.  ifem_hip.h describes the face table and the scope.
//
// One wavefront (= one workgroup) per cell, no atomics: a cell evaluates all of its own face integrals, an interior face is therefore
// evaluated from both sides, and the result does not depend on any order of execution.  On axis-aligned boxes the normal derivative on
// face f = 2 d + side is (1 / h_d) d/dxi_d, a 1D derivative in the normal direction times 1D values in the tangential ones:
//   stage 1  the cell's nodal values -> LDS
//   stage 2  the normal derivative at the (kv+1)^(dim-1) face nodes: of the cell itself on its 2 dim faces (from LDS), and of every
//            neighbour on the opposite face (from the neighbour's nodal values) -- what remains is a Q_kv function ON the face
//   stage 3  lanes over (subface, face, quadrature point): both face functions at the point (1D tables at the Gauss points of the face,
//            of its lower half or of its upper half, whichever side of a hanging face the cell is on), squared jump, weight
//   stage 4  a shuffle reduction in a fixed order, eta_K by lane 0
// 3D Q2: 54 points on regular faces (one pass of the wave), up to 216 with subfaces.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "ctx.hpp"
#include "kernels.hpp"

namespace ifem {

__host__ __device__ constexpr int kelly_ipow(int b, int e) { return e <= 0 ? 1 : b * kelly_ipow(b, e - 1); }

// local node of the cell with index `in` along direction d and (j, k) along the tangential directions in ascending order
template <int DIM, int N1>
__device__ inline int face_node(int d, int in, int jk) {
  if (DIM == 2) return d == 0 ? in + N1 * jk : jk + N1 * in;
  const int j = jk % N1, k = jk / N1;
  return d == 0 ? in + N1 * (j + N1 * k) : (d == 1 ? j + N1 * (in + N1 * k) : j + N1 * (k + N1 * in));
}

template <int DIM, int KV>
__global__ __launch_bounds__(64) void k_kelly(int64_t n_cells, const double *__restrict__ vcoords, const int32_t *__restrict__ cell_unodes,
                                              const int32_t *__restrict__ faces, const double *__restrict__ x,
                                              const KellyTabs *__restrict__ tabs, double *__restrict__ eta) {
  constexpr int N1 = KV + 1, NU = kelly_ipow(N1, DIM), NT = kelly_ipow(N1, DIM - 1), NS = 1 << (DIM - 1), NF = 2 * DIM, FS = 1 + NS,
                NV = 1 << DIM;
  __shared__ double s_u[DIM * NU];            // [c][a] nodal values of the cell
  __shared__ double s_go[NF * DIM * NT];      // [f][c][jk] its normal derivative at the face nodes
  __shared__ double s_gn[NS * NF * DIM * NT]; // [s][f][c][jk] the neighbours' on the opposite face
  __shared__ KellyTabs s_t;
  __shared__ int32_t s_face[NF * FS];
  __shared__ double s_h[3];
  const int lane = threadIdx.x;
  const int64_t cell = xcd_swizzle(blockIdx.x, gridDim.x);
  if (cell >= n_cells) return; // (never: the grid is n_cells; wave-uniform)
  if (lane < int(sizeof(KellyTabs) / sizeof(double))) reinterpret_cast<double *>(&s_t)[lane] = reinterpret_cast<const double *>(tabs)[lane];
  if (lane < NF * FS) s_face[lane] = faces[cell * (NF * FS) + lane];
  if (lane < DIM) s_h[lane] = vcoords[(cell * NV + (NV - 1)) * DIM + lane] - vcoords[cell * NV * DIM + lane];
  for (int i = lane; i < DIM * NU; i += 64) {
    const int a = i / DIM, c = i - a * DIM;
    s_u[c * NU + a] = x[int64_t(DIM) * cell_unodes[cell * NU + a] + c];
  }
  __syncthreads();
  for (int i = lane; i < NF * DIM * NT; i += 64) {
    const int f = i / (DIM * NT), c = (i / NT) % DIM, jk = i % NT, d = f >> 1, side = f & 1;
    double g = 0;
#pragma unroll
    for (int in = 0; in < N1; ++in) g += s_t.dn[side][in] * s_u[c * NU + face_node<DIM, N1>(d, in, jk)];
    s_go[i] = g / s_h[d];
  }
  for (int i = lane; i < NS * NF * DIM * NT; i += 64) { // (subface outermost: a cell without finer neighbours is done after NF DIM NT items)
    const int s = i / (NF * DIM * NT), f = (i / (DIM * NT)) % NF, c = (i / NT) % DIM, jk = i % NT, d = f >> 1, side = f & 1;
    const int kind = s_face[f * FS] & 0xff;
    if (kind == IFEM_FACE_BOUNDARY || (kind != IFEM_FACE_FINER && s > 0)) continue;
    const int64_t nb = s_face[f * FS + 1 + s];
    const double hn = vcoords[(nb * NV + (NV - 1)) * DIM + d] - vcoords[nb * NV * DIM + d];
    double g = 0;
#pragma unroll
    for (int in = 0; in < N1; ++in) g += s_t.dn[1 - side][in] * x[int64_t(DIM) * cell_unodes[nb * NU + face_node<DIM, N1>(d, in, jk)] + c];
    s_gn[i] = g / hn;
  }
  __syncthreads();
  double sum = 0;
  for (int i = lane; i < NS * NF * NT; i += 64) {
    const int s = i / (NF * NT), f = (i / NT) % NF, q = i % NT, d = f >> 1;
    const int kind = s_face[f * FS] & 0xff, sub = s_face[f * FS] >> 8;
    if (kind == IFEM_FACE_BOUNDARY || (kind != IFEM_FACE_FINER && s > 0)) continue;
    // which 1D table each side reads along the two tangential directions: a whole face, or the half the subface covers
    const int so0 = kind == IFEM_FACE_FINER ? 1 + (s & 1) : 0, so1 = kind == IFEM_FACE_FINER ? 1 + ((s >> 1) & 1) : 0;
    const int sn0 = kind == IFEM_FACE_COARSER ? 1 + (sub & 1) : 0, sn1 = kind == IFEM_FACE_COARSER ? 1 + ((sub >> 1) & 1) : 0;
    const int q0 = q % N1, q1 = q / N1;
    double jump2 = 0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const double *go = s_go + (f * DIM + c) * NT, *gn = s_gn + ((s * NF + f) * DIM + c) * NT;
      double vo = 0, vn = 0;
      if (DIM == 2) {
#pragma unroll
        for (int j = 0; j < N1; ++j) { vo += s_t.tv[so0][q0][j] * go[j]; vn += s_t.tv[sn0][q0][j] * gn[j]; }
      } else {
#pragma unroll
        for (int k = 0; k < N1; ++k) {
          double ro = 0, rn = 0;
#pragma unroll
          for (int j = 0; j < N1; ++j) { ro += s_t.tv[so0][q0][j] * go[j + N1 * k]; rn += s_t.tv[sn0][q0][j] * gn[j + N1 * k]; }
          vo += s_t.tv[so1][q1][k] * ro;
          vn += s_t.tv[sn1][q1][k] * rn;
        }
      }
      jump2 += (vo - vn) * (vo - vn);
    }
    double wgt = s_t.w[q0] * (DIM == 3 ? s_t.w[q1] : 1.0); // times the measure of the (sub)face
#pragma unroll
    for (int t = 0; t < DIM; ++t) if (t != d) wgt *= s_h[t];
    if (kind == IFEM_FACE_FINER) wgt *= 1.0 / NS;
    sum += wgt * jump2;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (lane == 0) {
    double h2 = 0;
#pragma unroll
    for (int t = 0; t < DIM; ++t) h2 += s_h[t] * s_h[t];
    eta[cell] = sqrt(sqrt(h2) / 24.0 * sum);
  }
}

static void build_kelly_tabs(KellyTabs &t, int kv) {
  std::memset(&t, 0, sizeof(t));
  const int n = kv + 1;
  double g[3], N[3], dN[3];
  fe_gauss01(n, g, t.w);
  for (int side = 0; side < 2; ++side) {
    fe_lagrange_1d(kv, double(side), N, dN);
    for (int i = 0; i < n; ++i) t.dn[side][i] = dN[i];
  }
  for (int set = 0; set < 3; ++set)
    for (int q = 0; q < n; ++q) {
      const double p = set == 0 ? g[q] : (set == 1 ? 0.5 * g[q] : 0.5 * (1.0 + g[q]));
      fe_lagrange_1d(kv, p, N, dN);
      for (int j = 0; j < n; ++j) t.tv[set][q][j] = N[j];
    }
}

// every local cell is an axis-aligned box with positive edges (decided once per context: vcoords never change)
static bool kelly_cells_are_boxes(ifem_ctx *ctx) {
  KellyState &K = ctx->kelly;
  if (K.boxes == 0) {
    if (ctx->mf_uniform) K.boxes = 1;
    else {
      const std::vector<double> vc = ctx->vcoords.download(ctx->stream);
      const int dim = ctx->dim, nv = 1 << dim;
      bool ok = true;
      for (int64_t c = 0; c < ctx->n_cells && ok; ++c) {
        const double *v = vc.data() + c * nv * dim;
        double h[3] = {0, 0, 0}, scale = 0;
        for (int d = 0; d < dim; ++d) { h[d] = v[(nv - 1) * dim + d] - v[d]; scale = std::max(scale, std::fabs(h[d])); }
        for (int d = 0; d < dim; ++d) ok = ok && h[d] > 0;
        for (int a = 0; a < nv && ok; ++a)
          for (int d = 0; d < dim; ++d) ok = ok && std::fabs(v[a * dim + d] - (v[d] + (((a >> d) & 1) ? h[d] : 0.0))) <= 1e-12 * scale;
      }
      K.boxes = ok ? 1 : -1;
    }
  }
  return K.boxes == 1;
}

void kelly_estimate(ifem_ctx *ctx, const double *x, const int32_t *face_table) {
  KellyState &K = ctx->kelly;
  const int dim = ctx->dim, kv = ctx->kv;
  if (ctx->halo.nranks > 1) throw Error(IFEM_E_BADPARAM, "ifem_kelly_estimate: single-rank contexts only (a partitioned context would need the neighbours' values across ranks)");
  if ((dim != 2 && dim != 3) || (kv != 1 && kv != 2)) throw Error(IFEM_E_BADPARAM, "ifem_kelly_estimate: dim 2 or 3 and velocity degree 1 or 2");
  if (!kelly_cells_are_boxes(ctx)) throw Error(IFEM_E_BADPARAM, "ifem_kelly_estimate: every cell must be an axis-aligned box (uniform box meshes and their one-level refinements)");
  const int nf = 2 * dim, fs = IFEM_FACE_STRIDE(dim), ns = 1 << (dim - 1);
  const size_t n_tab = size_t(ctx->n_cells) * nf * fs;
  if (face_table) { // bounds first: the kernel indexes the cell tables with these entries
    for (int64_t c = 0; c < ctx->n_cells; ++c)
      for (int f = 0; f < nf; ++f) {
        const int32_t *r = face_table + (c * nf + f) * fs;
        const int kind = r[0] & 0xff, sub = r[0] >> 8;
        if (r[0] < 0 || kind > IFEM_FACE_FINER || sub >= ns || (kind != IFEM_FACE_COARSER && sub != 0))
          throw Error(IFEM_E_BADPARAM, "ifem_kelly_estimate: face table: unknown kind or subface out of range");
        const int need = kind == IFEM_FACE_BOUNDARY ? 0 : (kind == IFEM_FACE_FINER ? ns : 1);
        for (int k = 0; k < need; ++k)
          if (r[1 + k] < 0 || r[1 + k] >= ctx->n_cells || r[1 + k] == c) throw Error(IFEM_E_BADPARAM, "ifem_kelly_estimate: face table: neighbour cell out of range");
      }
    K.faces.upload(face_table, n_tab, ctx->stream);
    IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // the caller's array may go
  } else if (K.faces.n != n_tab)
    throw Error(IFEM_E_BADPARAM, "ifem_kelly_estimate: no face table given and none kept from an earlier call");
  if (!K.tabs.p) {
    KellyTabs t;
    build_kelly_tabs(t, kv);
    K.tabs.upload(&t, 1, ctx->stream);
    IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  if (K.eta.n != size_t(ctx->n_cells)) K.eta.alloc(size_t(ctx->n_cells), "the Kelly indicators");
  if (!ctx->n_cells) return;
  // algorithmic bytes: the velocity block once, the cell tables (nodes, vertices), the face table, the result
  const int nu = ctx->nu, nv = 1 << dim;
  KScope ks(ctx, IFEM_KC_REFINE, 8.0 * dim * double(ctx->nUl) + double(ctx->n_cells) * (4.0 * nu + 8.0 * nv * dim + 4.0 * nf * fs + 8.0));
  const dim3 grid(unsigned(ctx->n_cells)), block(64);
#define IFEM_KELLY_LAUNCH(D, KVV) \
  hipLaunchKernelGGL((k_kelly<D, KVV>), grid, block, 0, ctx->stream, ctx->n_cells, ctx->vcoords.p, ctx->cell_unodes.p, K.faces.p, x, K.tabs.p, K.eta.p)
  if (dim == 2 && kv == 1) IFEM_KELLY_LAUNCH(2, 1);
  else if (dim == 2) IFEM_KELLY_LAUNCH(2, 2);
  else if (kv == 1) IFEM_KELLY_LAUNCH(3, 1);
  else IFEM_KELLY_LAUNCH(3, 2);
#undef IFEM_KELLY_LAUNCH
  IFEM_HIP_CHECK(hipGetLastError());
}

} // namespace ifem
