// lattice_stencil.hpp -- the table build shared by the lattice stencil products of a uniform box level (sm_stencil.hip: S_m; bb_stencil.hip: B, B^T).
//
// On an axis-aligned uniform box the rows of these matrices with the same position signature hold the same numbers, so a product can read a dense
// row per class from a table instead of streaming (value, column) pairs.  An operator describes itself by a traits type OP:
//   DIM, W, NC, NR, G   space dimension | window width per axis | value components per block (planar: val[rs * NC + a * len + k]) | result
//                       components per row of the product with the probe vector (1: NC column components, NC: one column, NC row components) |
//                       lanes per row of k_stencil_classify
//   first_col(i)        first point of the column lattice, per axis, in the window of row point i
//   axis_classes        the signatures of the row lattice's axes (lattice.hpp)
//   table_name, ...     what the allocations are called in an error message
// The dense form of a row is [component][offset], x fastest, K = NC W^DIM doubles (StencilK); missing couplings are 0.
//
// Build (stencil_build, at set-up time only: it allocates and synchronises):
//   signature        the class of a row is the triple of its axes' signatures (OP::axis_classes numbers the ones that occur).
//   k_stencil_table     one block per class: the CSR row of the class's first lattice point in dense form, and max |entry| of it.
//   k_stencil_classify  G lanes per row: expands the row the same way and compares it entry by entry with its class, |v - T| <= 1e-12 max |T[class]|.
//                       A row that fails (or couples beyond the window) is irregular: class id 0xFFFF, appended to the row list (an integer atomic
//                       on the counter; the order of the list does not enter any sum); the planar CSR kernels produce these rows.  While it holds
//                       the row the group can also form the row's CSR product with a probe vector e, which spares the probe a CSR launch.
//   More than 1/8 irregular rows: the operator keeps the CSR product.
// Probe (stencil_probe_compare): the new product of a pseudo-random vector against a CSR product of the assembled values, max |diff| <= 1e-12
//   max |ref|, formed and compared on the device (three scalars come back).  stencil_decide: an operator that fails keeps the CSR product for
//   the life of the context.
#pragma once
#include <cmath>
#include <cstdio>
#include <vector>
#include "ctx.hpp"
#include "kernels.hpp"

namespace ifem {

constexpr int kStencilIrregular = 0xFFFF;

struct StencilDims { int n[3], m[3], nc0, nc1; }; // nodes per axis of the row lattice | of the column lattice; classes of the first two row axes
template <class OP> struct StencilK { static constexpr int KO = OP::DIM == 3 ? OP::W * OP::W * OP::W : OP::W * OP::W, K = KO * OP::NC; };

// The dense form of CSR row `node` (at point (ix, iy, iz) of the row lattice) into `dense` (K doubles, zeroed by the caller) by the LANES lanes of
// a group; returns whether this lane met a coupling beyond the window.  e (the probe vector, may be null): this lane's share of the row's product
// with it is added to ref[0 .. NR).  The caller separates the phases (zero | scatter | read).
template <class OP, int LANES>
__device__ inline bool stencil_expand(const StencilDims d, int ix, int iy, int iz, int64_t node, const int32_t *__restrict__ lon_col, const int64_t *__restrict__ rp,
                                      const int32_t *__restrict__ col, const double *__restrict__ val, double *dense, int lane, const double *__restrict__ e, double *ref) {
  constexpr int DIM = OP::DIM, W = OP::W, NC = OP::NC, KO = StencilK<OP>::KO;
  const int64_t rs = rp[node];
  const int len = int(rp[node + 1] - rs);
  const double *vb = val + rs * NC;
  bool beyond = false;
  for (int k = lane; k < len; k += LANES) {
    const int c = col[rs + k];
    double v[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) v[a] = vb[int64_t(a) * len + k];
    if (e) {
#pragma unroll
      for (int a = 0; a < NC; ++a) {
        if (OP::NR == 1) ref[0] += v[a] * e[int64_t(c) * NC + a];
        else ref[a] += v[a] * e[c];
      }
    }
    const int p = lon_col[c];
    const int jx = p % d.m[0], jy = (p / d.m[0]) % d.m[1], jz = p / (d.m[0] * d.m[1]);
    const int dx = jx - OP::first_col(ix), dy = jy - OP::first_col(iy), dz = DIM == 3 ? jz - OP::first_col(iz) : 0;
    if (dx < 0 || dx >= W || dy < 0 || dy >= W || dz < 0 || dz >= W) { beyond = true; continue; }
    const int o = DIM == 3 ? (dz * W + dy) * W + dx : dy * W + dx;
#pragma unroll
    for (int a = 0; a < NC; ++a) dense[a * KO + o] = v[a];
  }
  return beyond;
}

// table[c][K] and tmax[c] = table[classes * K + c] of class c = blockIdx.x from the row at its first lattice point; first: the per-axis first
// points of the axis classes, [nc0 | nc1 | nc2]
template <class OP>
__global__ __launch_bounds__(64) void k_stencil_table(StencilDims d, int classes, const int32_t *__restrict__ first, const int32_t *__restrict__ nol_row,
                                                      const int32_t *__restrict__ lon_col, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
                                                      const double *__restrict__ val, double *__restrict__ table) {
  constexpr int K = StencilK<OP>::K;
  __shared__ double dense[K];
  __shared__ double red[64];
  const int c = blockIdx.x, lane = threadIdx.x;
  const int ix = first[c % d.nc0], iy = first[d.nc0 + (c / d.nc0) % d.nc1], iz = OP::DIM == 3 ? first[d.nc0 + d.nc1 + c / (d.nc0 * d.nc1)] : 0;
  const int64_t node = nol_row[ix + d.n[0] * (iy + d.n[1] * iz)];
  for (int o = lane; o < K; o += 64) dense[o] = 0.0;
  __syncthreads();
  (void)stencil_expand<OP, 64>(d, ix, iy, iz, node, lon_col, rp, col, val, dense, lane, nullptr, nullptr); // (a coupling beyond the window: k_stencil_classify sends the row to the list)
  __syncthreads();
  double m = 0;
  for (int o = lane; o < K; o += 64) {
    table[int64_t(c) * K + o] = dense[o];
    m = fmax(m, fabs(dense[o]));
  }
  red[lane] = m;
  __syncthreads();
  if (lane == 0) {
    for (int l = 1; l < 64; ++l) m = fmax(m, red[l]);
    table[int64_t(classes) * K + c] = m;
  }
}

// G lanes per point of the row lattice (a wave for the 125 entries or blocks of an S_m or B row, 16 lanes for the at most 27 of a B^T row: with a
// wave per row the 17 M rows of B^T at 128^3 cells are as many waves that wait for four dependent loads each): class id or kStencilIrregular into
// cls, irregular rows into rows[< cap] (counter counts all of them) and, where e is given, the row's CSR product with it into ref[node * NR + a]
template <class OP>
__global__ __launch_bounds__(256) void k_stencil_classify(StencilDims d, int classes, int64_t N, const uint8_t *__restrict__ axcls, const int32_t *__restrict__ nol_row,
                                                          const int32_t *__restrict__ lon_col, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
                                                          const double *__restrict__ val, const double *__restrict__ table, uint16_t *__restrict__ cls,
                                                          int32_t *__restrict__ rows, int32_t cap, int32_t *__restrict__ counter, const double *__restrict__ e,
                                                          double *__restrict__ ref) {
  constexpr int K = StencilK<OP>::K, NR = OP::NR, G = OP::G, RPB = 256 / G;
  __shared__ double dense_all[RPB][K];
  const int w = threadIdx.x / G, lane = threadIdx.x % G;
  const int64_t p = int64_t(blockIdx.x) * RPB + w;
  const bool live = p < N;
  double *dense = dense_all[w];
  for (int o = lane; o < K; o += G) dense[o] = 0.0;
  __syncthreads();
  int c = 0;
  int64_t node = 0;
  bool bad = false;
  double r[NR];
#pragma unroll
  for (int a = 0; a < NR; ++a) r[a] = 0;
  if (live) {
    const int ix = int(p % d.n[0]), iy = int((p / d.n[0]) % d.n[1]), iz = int(p / (int64_t(d.n[0]) * d.n[1]));
    c = axcls[ix] + d.nc0 * (axcls[d.n[0] + iy] + d.nc1 * (OP::DIM == 3 ? axcls[d.n[0] + d.n[1] + iz] : 0));
    node = nol_row[p];
    bad = stencil_expand<OP, G>(d, ix, iy, iz, node, lon_col, rp, col, val, dense, lane, e, r);
  }
  __syncthreads();
  if (!live) return;
  if (e) {
#pragma unroll
    for (int a = 0; a < NR; ++a) {
#pragma unroll
      for (int off = G / 2; off > 0; off >>= 1) r[a] += __shfl_xor(r[a], off, 64); // (stays inside the aligned group)
    }
  }
  const double bound = 1e-12 * table[int64_t(classes) * K + c];
  for (int o = lane; o < K; o += G) bad = bad || !(fabs(dense[o] - table[int64_t(c) * K + o]) <= bound); // (a NaN fails)
  const unsigned long long group = (G == 64 ? ~0ull : (1ull << (G & 63)) - 1) << ((threadIdx.x & 63) / G * G);
  const bool irregular = (__ballot(bad) & group) != 0;
  if (lane == 0) {
    if (e) {
#pragma unroll
      for (int a = 0; a < NR; ++a) ref[node * NR + a] = r[a];
    }
    cls[p] = irregular ? uint16_t(kStencilIrregular) : uint16_t(c);
    if (irregular) {
      const int32_t at = atomicAdd(counter, 1);
      if (at < cap) rows[at] = int32_t(node);
    }
  }
}

// ---- host side

template <class RL, class CL> // PLattice / ULattice
inline StencilDims stencil_dims(const RL &R, const CL &C, const StencilClasses &T) {
  return {{R.n[0], R.n[1], R.n[2]}, {C.n[0], C.n[1], C.n[2]}, T.ncls[0], T.ncls[1]};
}

// tables and classes of the present values of M, whose rows are the nodes of lattice R and whose columns are those of lattice C, and (e given)
// the CSR product with e into ref; false: more than 1/8 of the rows are irregular
template <class OP, class RL, class CL>
bool stencil_build(ifem_ctx *ctx, StencilClasses &T, const RL &R, const CL &C, const PlanarCsr &M, const double *e, double *ref) {
  constexpr int K = StencilK<OP>::K, RPB = 256 / OP::G;
  const int64_t N = M.n_rows; // (the callers' eligibility: as many as the row lattice has points)
  hipStream_t s = ctx->stream;
  if (T.axcls.n == 0) { // the lattice part: once per context
    std::vector<uint8_t> ax, a;
    std::vector<int32_t> first, f;
    for (int d = 0; d < 3; ++d) {
      T.ncls[d] = OP::axis_classes(R.n[d], a, f);
      ax.insert(ax.end(), a.begin(), a.end());
      first.insert(first.end(), f.begin(), f.end());
    }
    T.classes = T.ncls[0] * T.ncls[1] * T.ncls[2];
    T.first.upload(first.data(), first.size(), s);
    T.axcls.upload(ax.data(), ax.size(), s);
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
    T.table.alloc(size_t(T.classes) * (K + 1), OP::table_name);
    T.cls.alloc(size_t(N), OP::cls_name);
    T.rows.alloc(size_t(N / 8 + 1), OP::rows_name);
    T.counter.alloc(1);
  }
  const StencilDims d = stencil_dims(R, C, T);
  const int32_t cap = int32_t(T.rows.n);
  IFEM_HIP_CHECK(hipMemsetAsync(T.counter.p, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL((k_stencil_table<OP>), dim3(unsigned(T.classes)), dim3(64), 0, s, d, T.classes, T.first.p, R.node_of_lattice.p, C.lattice_of_node.p, M.rowptr.p, M.col.p, M.val.p,
                     T.table.p);
  hipLaunchKernelGGL((k_stencil_classify<OP>), dim3(unsigned((N + RPB - 1) / RPB)), dim3(256), 0, s, d, T.classes, N, T.axcls.p, R.node_of_lattice.p, C.lattice_of_node.p, M.rowptr.p,
                     M.col.p, M.val.p, T.table.p, T.cls.p, T.rows.p, cap, T.counter.p, e, ref);
  int32_t count = 0;
  IFEM_HIP_CHECK(hipMemcpyAsync(&count, T.counter.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  IFEM_HIP_CHECK(hipGetLastError());
  T.n_irregular = count;
  return int64_t(count) * 8 <= N;
}

// the stencil product `got` of the probe vector against the CSR product `ref` (got: overwritten); *rel: max |got - ref| / max |ref|
inline bool stencil_probe_compare(ifem_ctx *ctx, int64_t n, const double *ref, double *got, double *rel) {
  double ymax = 0, err = 0;
  const bool finite = v_probe_diff(ctx, n, ref, got, &ymax, &err);
  *rel = !finite ? INFINITY : (ymax > 0 ? err / ymax : err);
  return finite && err <= 1e-12 * ymax;
}

// What a build (`few`: stencil_build's result) and its probe (`probe_ok`, `rel`; not made without `few`) mean for the record; the verbose line
// of an operator that keeps the CSR product is printed once.  `keeps`: who keeps it ("level", "context").  Returns T.ready.
inline bool stencil_decide(StencilClasses &T, bool few, bool probe_ok, double rel, const char *name, int64_t N, const char *keeps, int verbose) {
  const char *why = !few ? "more than 1/8 of the rows differ from their class" : !probe_ok ? "the stencil product misses the assembled matrix (1e-12)" : nullptr;
  if (few && !probe_ok) T.failed = true; // off for this context
  if (why) {
    if (verbose && !T.said) fprintf(stderr, "[ifem] %s: %s (%lld irregular rows of %lld, probe %.2e): this %s keeps the CSR product\n", name, why, (long long)T.n_irregular, (long long)N, rel, keeps);
    T.said = true;
    return false;
  }
  return T.ready = true;
}

} // namespace ifem
