// mp_direct.hip -- x = M_p^-1 b on a uniform box level by tensor-product line solves (ifem_solver_opts::mp_solver = 0).
//
// On an axis-aligned uniform box whose pressure nodes fill the whole lattice n_x x n_y (x n_z), the Q1 mass matrix is the Kronecker product
// M_x (x) M_y (x) M_z of the 1D mass matrices M_d = h_d tridiag(1/6, 2/3, 1/6) (end diagonals 1/3) -- the assembly's Gauss rule integrates
// Q1 x Q1 exactly -- and so is its inverse: one sweep of tridiagonal (Thomas) line solves per axis, in fp64, instead of the ~36 iterations
// of Jacobi-preconditioned CG that solver.hip::solve_mp runs to mp_rel = 1e-6.  The stopping rule max(mp_abs, mp_rel ||b||) of that CG is met
// trivially: the result is the solution up to the rounding of three line solves (kappa(M_d) <= 6 per axis).
//
// The closed form is never trusted on its own.  mp_direct_ready() probes the tables against the matrix the assembly wrote (a pseudo-random
// e, x = direct(e), max |M_p x - e| <= 1e-12 max |e| with the fp64 SpMV) after the first assembly and again whenever M_p is re-integrated
// (ctx.hpp::geometry_written); a context that fails keeps CG from then on.
//
// Eligibility (mp_direct_build, once per context; the lattice map is the context's, setup.hip::p_lattice_ensure / lattice.cpp): one rank, no hanging-node line, ifem_ctx::mf_uniform as detected at creation, Q1 pressure in
// 2D / 3D, every cell vertex on a lattice point i_d = round((x_d - x_min,d) / h_d) within 8 eps max|x| (the allowance of
// setup.hip::detect_uniform_cells), the map node -> lattice point a bijection onto the full box (holes, L-shapes, duplicates: CG), and
// CAP: at most kLatticeMaxLine = 65536 nodes per line (the factor tables and the 32-bit position along a line) and fewer than 2^31 nodes.
//
// Kernels.  The work vector w is lattice-ordered, x fastest.  The node order is folded into the sweeps: the first sweep reads b[node_of_lattice[.]],
// the last one stores x[node_of_lattice[.]]; there is no permutation pass.
//   k_mpd_contig   the x axis (contiguous in w), always the first sweep: a block stages 64 lines x 32 columns through LDS (row pitch 33 doubles:
//                  the 64 owner lanes read conflict-free), all 256 threads load / store the tile with 256-byte runs per line, the first wave
//                  carries the recurrence of its 64 lines from chunk to chunk in a register.  The forward pass leaves d' in w, the backward
//                  pass re-reads it chunk by chunk from the end (every thread re-reads exactly the entries it stored itself).  17 KB of LDS.
//                  (The alternative of the issue, a layout in which the solved axis is never the fastest one, needs a transposing pass or a
//                  second index table and was not built; the choice is by the byte account, not by a measurement of both.)
//   k_mpd_strided  the y and z axes: one thread per line, neighbouring threads on neighbouring lines (consecutive addresses at every step of the
//                  recurrence).  The loads of the next 16 entries are issued before the dependent recurrence of the present 16 runs -- the data
//                  do not depend on it.  Forward pass in place in w, backward pass in place or, in the last sweep, scattered to x.
// Plain loads and stores only, no LDS beyond the tile, no scratch.
// Bytes per node and application: x sweep 4 + 8 + 8 | 8 + 8, y sweep 8 + 8 | 8 + 8, z sweep the same + 4 for the scatter index.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
#include "ctx.hpp"
#include "kernels.hpp"

namespace ifem {

constexpr int kMpdTL = 64, kMpdTC = 32, kMpdPitch = kMpdTC + 1; // tile of k_mpd_contig: lines, columns, LDS row pitch
constexpr int kMpdU = 16;                                       // entries per batch of k_mpd_strided

// ---- host side: Thomas factors (plain C++, no device call; the lattice map is setup.hip::p_lattice_ensure)

// Thomas factors of M = h tridiag(1/6, 2/3, 1/6) with end diagonals 1/3, n >= 2 rows, no pivoting (SPD, strictly diagonally dominant):
// forward d'_i = rpiv_i d_i - mult_i d'_{i-1}, backward x_i = d'_i - mult_i x_{i+1}; mult_i = (h / 6) rpiv_i serves both (the matrix is symmetric
// with a constant off-diagonal; d'_{-1} = x_n = 0)
void mpd_thomas_factors(int n, double h, std::vector<double> &rpiv, std::vector<double> &mult) {
  rpiv.assign(size_t(n), 0.0);
  mult.assign(size_t(n), 0.0);
  const double off = h / 6.0;
  double cprev = 0; // c'_{i-1} = off * rpiv_{i-1}
  for (int i = 0; i < n; ++i) {
    const double diag = (i == 0 || i == n - 1) ? h / 3.0 : 2.0 * h / 3.0;
    rpiv[i] = 1.0 / (diag - off * cprev);
    mult[i] = off * rpiv[i];
    cprev = mult[i];
  }
}

// ---- kernels

// The x axis: line l holds w[l * n .. l * n + n).  Always the first sweep: the input is src[idx[.]], the caller's node order.
__global__ __launch_bounds__(256) void k_mpd_contig(int64_t n_lines, int n, const double *__restrict__ rpiv, const double *__restrict__ mult,
                                                    const double *__restrict__ src, const int32_t *__restrict__ idx, double *__restrict__ w) {
  __shared__ double tile[kMpdTL * kMpdPitch];
  const int tid = threadIdx.x, col = tid & (kMpdTC - 1), lr = tid >> 5; // this thread moves column `col` of the lines lr, lr + 8, ...
  const int64_t L0 = int64_t(blockIdx.x) * kMpdTL;
  const bool owner = tid < kMpdTL && L0 + tid < n_lines; // ... and the first wave owns one line each
  double carry = 0;
  // forward: d'_i = rpiv_i d_i - mult_i d'_{i-1}
  for (int c0 = 0; c0 < n; c0 += kMpdTC) {
    const int i = c0 + col;
#pragma unroll
    for (int k = 0; k < kMpdTL / 8; ++k) {
      const int line = lr + 8 * k;
      if (L0 + line < n_lines && i < n) {
        const int64_t a = (L0 + line) * n + i;
        tile[line * kMpdPitch + col] = src[idx[a]];
      }
    }
    __syncthreads();
    if (owner) {
      const int m = min(kMpdTC, n - c0);
      for (int j = 0; j < m; ++j) {
        carry = tile[tid * kMpdPitch + j] * rpiv[c0 + j] - mult[c0 + j] * carry;
        tile[tid * kMpdPitch + j] = carry;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kMpdTL / 8; ++k) {
      const int line = lr + 8 * k;
      if (L0 + line < n_lines && i < n) w[(L0 + line) * n + i] = tile[line * kMpdPitch + col];
    }
  }
  // backward: x_i = d'_i - mult_i x_{i+1}; every thread reads back the entries of w it stored itself, and the same tile slots
  carry = 0;
  for (int c0 = ((n - 1) / kMpdTC) * kMpdTC; c0 >= 0; c0 -= kMpdTC) {
    const int i = c0 + col;
#pragma unroll
    for (int k = 0; k < kMpdTL / 8; ++k) {
      const int line = lr + 8 * k;
      if (L0 + line < n_lines && i < n) tile[line * kMpdPitch + col] = w[(L0 + line) * n + i];
    }
    __syncthreads();
    if (owner) {
      const int m = min(kMpdTC, n - c0);
      for (int j = m - 1; j >= 0; --j) {
        carry = tile[tid * kMpdPitch + j] - mult[c0 + j] * carry;
        tile[tid * kMpdPitch + j] = carry;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kMpdTL / 8; ++k) {
      const int line = lr + 8 * k;
      if (L0 + line < n_lines && i < n) w[(L0 + line) * n + i] = tile[line * kMpdPitch + col];
    }
  }
}

// A strided axis: line t = inner + n_inner * outer starts at w[inner + outer * outer_stride], its entries are `stride` apart.  SCATTER: the result
// goes to out[idx[.]] (the caller's node order) instead of back into w.
template <bool SCATTER>
__global__ __launch_bounds__(64) void k_mpd_strided(int64_t n_lines, int64_t n_inner, int64_t outer_stride, int n, int64_t stride,
                                                    const double *__restrict__ rpiv, const double *__restrict__ mult, double *__restrict__ w,
                                                    double *__restrict__ out, const int32_t *__restrict__ idx) {
  const int64_t t = int64_t(blockIdx.x) * 64 + threadIdx.x;
  if (t >= n_lines) return;
  double *const line = w + (t % n_inner) + (t / n_inner) * outer_stride;
  double cur[kMpdU], nxt[kMpdU];
  // forward
#pragma unroll
  for (int k = 0; k < kMpdU; ++k) cur[k] = k < n ? line[k * stride] : 0.0;
  double carry = 0;
  for (int j0 = 0; j0 < n; j0 += kMpdU) {
#pragma unroll
    for (int k = 0; k < kMpdU; ++k) nxt[k] = j0 + kMpdU + k < n ? line[(j0 + kMpdU + k) * stride] : 0.0;
#pragma unroll
    for (int k = 0; k < kMpdU; ++k)
      if (j0 + k < n) {
        carry = cur[k] * rpiv[j0 + k] - mult[j0 + k] * carry;
        line[(j0 + k) * stride] = carry;
      }
#pragma unroll
    for (int k = 0; k < kMpdU; ++k) cur[k] = nxt[k];
  }
  // backward, batches from the end: entry j0 - k of the batch at j0 (this thread reads what it stored above)
  int32_t ci[kMpdU], ni[kMpdU];
  const int64_t off = line - w;
#pragma unroll
  for (int k = 0; k < kMpdU; ++k) {
    const int j = n - 1 - k;
    cur[k] = j >= 0 ? line[j * stride] : 0.0;
    if (SCATTER) ci[k] = j >= 0 ? idx[off + j * stride] : 0;
  }
  carry = 0;
  for (int j0 = n - 1; j0 >= 0; j0 -= kMpdU) {
#pragma unroll
    for (int k = 0; k < kMpdU; ++k) {
      const int j = j0 - kMpdU - k;
      nxt[k] = j >= 0 ? line[j * stride] : 0.0;
      if (SCATTER) ni[k] = j >= 0 ? idx[off + j * stride] : 0;
    }
#pragma unroll
    for (int k = 0; k < kMpdU; ++k) {
      const int j = j0 - k;
      if (j >= 0) {
        carry = cur[k] - mult[j] * carry;
        if (SCATTER) out[ci[k]] = carry; else line[j * stride] = carry;
      }
    }
#pragma unroll
    for (int k = 0; k < kMpdU; ++k) { cur[k] = nxt[k]; if (SCATTER) ci[k] = ni[k]; }
  }
}

// ---- host drivers

// decides the context once: tables built (state 1) or CG for good (state -1)
static void mp_direct_build(ifem_ctx *ctx) {
  MpDirect &D = ctx->mp_direct;
  D.state = -1;
  const int dim = ctx->dim;
  if (!p_lattice_ensure(ctx) || ctx->Mp.n_rows != ctx->nPo) return;
  const PLattice &L = ctx->p_lattice;
  hipStream_t s = ctx->stream;
  std::vector<double> rp, mu;
  for (int d = 0; d < dim; ++d) {
    mpd_thomas_factors(L.n[d], ctx->mf_h[d], rp, mu);
    D.rpiv[d].upload(rp.data(), rp.size(), s);
    D.mult[d].upload(mu.data(), mu.size(), s);
    IFEM_HIP_CHECK(hipStreamSynchronize(s)); // (rp / mu are reused)
  }
  D.w.alloc(size_t(ctx->nPo), "the work vector of the direct M_p solve");
  D.state = 1;
}

void mp_direct_apply(ifem_ctx *ctx, const double *b, double *x) {
  MpDirect &D = ctx->mp_direct;
  if (D.state != 1) throw Error(IFEM_E_BADPARAM, "mp_direct_apply: the context has no line-solve tables");
  const int dim = ctx->dim;
  const PLattice &L = ctx->p_lattice;
  const int64_t nx = L.n[0], ny = L.n[1], nz = dim == 3 ? L.n[2] : 1, N = nx * ny * nz;
  hipStream_t s = ctx->stream;
  KScope ks(ctx, IFEM_KC_SPMV_MP, double(N) * (36.0 + 32.0 * (dim - 2) + 36.0));
  const int32_t *nol = L.node_of_lattice.p;
  double *w = D.w.p;
  { // x: the contiguous axis, gathers b
    const int64_t lines = ny * nz;
    hipLaunchKernelGGL(k_mpd_contig, dim3(unsigned((lines + kMpdTL - 1) / kMpdTL)), dim3(256), 0, s, lines, int(nx), D.rpiv[0].p, D.mult[0].p, b, nol, w);
  }
  { // y: lines (i_x, i_z); the last sweep in 2D
    const int64_t lines = nx * nz;
    const dim3 g(unsigned((lines + 63) / 64));
    if (dim == 2) hipLaunchKernelGGL(k_mpd_strided<true>, g, dim3(64), 0, s, lines, nx, nx * ny, int(ny), nx, D.rpiv[1].p, D.mult[1].p, w, x, nol);
    else hipLaunchKernelGGL(k_mpd_strided<false>, g, dim3(64), 0, s, lines, nx, nx * ny, int(ny), nx, D.rpiv[1].p, D.mult[1].p, w, w, nol);
  }
  if (dim == 3) { // z: lines (i_x, i_y), scatters x
    const int64_t lines = nx * ny;
    hipLaunchKernelGGL(k_mpd_strided<true>, dim3(unsigned((lines + 63) / 64)), dim3(64), 0, s, lines, lines, int64_t(0), int(nz), lines, D.rpiv[2].p, D.mult[2].p, w, x, nol);
  }
}

// the probe of the present M_p values: x = direct(e), then M_p x against e with the fp64 SpMV
static bool mp_direct_probe(ifem_ctx *ctx, double *err_out) {
  const int64_t n = ctx->nPo;
  const size_t un = size_t(n);
  std::vector<double> e(un), y(un);
  uint64_t st = 0x9E3779B97F4A7C15ull; // fixed seed: the same probe on every run
  double emax = 0;
  for (int64_t i = 0; i < n; ++i) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    e[i] = double(st >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    emax = std::max(emax, std::fabs(e[i]));
  }
  hipStream_t s = ctx->stream;
  DBuf<double> de, dx, dy;
  de.upload(e.data(), size_t(n), s);
  dx.alloc(size_t(n)); dy.alloc(size_t(n));
  mp_direct_apply(ctx, de.p, dx.p);
  spmv_mp(ctx, dx.p, dy.p, 0, /*use_f32=*/false);
  IFEM_HIP_CHECK(hipMemcpyAsync(y.data(), dy.p, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, s));
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  IFEM_HIP_CHECK(hipGetLastError());
  double err = 0;
  bool finite = true;
  for (int64_t i = 0; i < n; ++i) {
    const double d = std::fabs(y[i] - e[i]);
    finite = finite && std::isfinite(d);
    err = std::max(err, d);
  }
  if (err_out) *err_out = finite ? err / emax : INFINITY;
  return finite && err <= 1e-12 * emax;
}

bool mp_direct_ready(ifem_ctx *ctx, int verbose) {
  MpDirect &D = ctx->mp_direct;
  if (D.state < 0 || !D.mass_ready) return false;
  if (D.state == 0) {
    mp_direct_build(ctx);
    if (D.state < 0) {
      if (verbose) fprintf(stderr, "[ifem] M_p: not a full uniform lattice on one rank: CG\n");
      return false;
    }
  }
  if (D.checked == 1) return true;
  double err = 0;
  if (mp_direct_probe(ctx, &err)) {
    D.checked = 1;
    if (verbose) fprintf(stderr, "[ifem] M_p: line solves on the %d x %d x %d lattice, probe max |M_p x - e| / max |e| = %.2e\n", ctx->p_lattice.n[0], ctx->p_lattice.n[1], ctx->p_lattice.n[2], err);
    return true;
  }
  D.state = -1; // off for this context
  D.w.release(); // (the lattice map is shared: it stays)
  for (int d = 0; d < 3; ++d) { D.rpiv[d].release(); D.mult[d].release(); }
  if (verbose) fprintf(stderr, "[ifem] M_p: the line solves miss the assembled matrix (probe %.2e > 1e-12): CG from now on\n", err);
  return false;
}

} // namespace ifem
