// sm_stencil.hip -- y = S_m x from stencil tables over the pressure lattice of a uniform box level.
//
// S_m = B diag(M_u)^-1 B^T is formed from the masked B and B^T of an axis-aligned uniform box, so a pressure row that lies two or more nodes away
// from every face has the same 5 x 5 (x 5) stencil as every other such row, and a row near a face one of a few dozen others, fixed by its distance
// to each face and by the constrained velocity dofs there.  The stored-matrix product streams 125 (value, column) pairs per row -- 2.1 GB at
// 129^3 rows for a 17 MB vector; from a table the product reads x, the lattice map, a class id per row and writes y.
//
// Eligibility: the context's pressure nodes are a full lattice (setup.hip::p_lattice_ensure: one rank, no hanging-node line, uniform box cells,
// Q1 pressure in 2D / 3D, a bijection onto the box) and S_m is explicit on one rank.  Everything else keeps linalg.hip::spmv_sm.
//
// Build (sm_stencil_setup, whenever S_m was re-formed -- ifem_ctx::sm_version -- and only at set-up time: solver.hip::sm_ensure; never inside
// sm_apply, which runs inside captured V-cycles):
//   signature  of lattice point i on an axis of n nodes: (min(i, 2), min(n - 1 - i, 2)); the class of a row is the triple of its axes' signatures
//              (lattice.cpp::lattice_axis_classes numbers the signatures that occur; at most 5 per axis, correct for axes shorter than 5 nodes).
//   k_sms_table     one block per class: the CSR row of the class's first lattice point, expanded into the dense 5^dim vector in offset order
//                   (x fastest; missing couplings 0), and max |entry| of it.
//   k_sms_classify  one wave per row: expands the row the same way and compares it entry by entry with its class, |v - T| <= 1e-12 max |T[class]|.
//                   A row that fails (or couples beyond the window) is irregular: class id 0xFFFF, appended to the row list (an integer atomic
//                   on the counter; the order of the list does not enter any sum).  More than 1/8 irregular rows: the level keeps the CSR product.
//   probe           pseudo-random e, the new product against the fp64 spmv_sm of the assembled matrix, max |diff| <= 1e-12 max |S_m e|, formed and
//                   compared on the device; a level that fails keeps the CSR product from then on.
// Apply (sm_stencil_apply):
//   k_sms_apply     a block of 256 threads takes a lattice tile (3D 8 x 8 x 8, two outputs per thread; 2D 16 x 16), gathers x through
//                   node_of_lattice into LDS with a two-deep halo (12^3 doubles = 13.8 KB; 20^2), forms every output as the 5^dim-term sum in
//                   fixed offset order and stores it to y[node_of_lattice[.]].  A wave whose rows share one class reads the table row through
//                   wave-uniform loads, the others index it per lane.  A wave is an 8 x 8 x-y plane (2D: a 16 x 4 strip), so every tile that holds
//                   one of the first or last two nodes of the x or y axis mixes classes: at 129 nodes per axis tiles 0, 15 and 16 of 17, about
//                   a third of the waves; on a level of a few tiles all of them.
//                   Irregular rows are skipped; the planar CSR kernel over the row list produces them in a second launch on the same stream.
// fp64 throughout, plain stores, no floating-point atomics, no scratch; every sum has a fixed order.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
#include "ctx.hpp"
#include "kernels.hpp"

namespace ifem {

constexpr int kSmsIrregular = 0xFFFF;
template <int DIM> struct SmsGeo; // tile (outputs) and LDS box (tile + two-deep halo) of k_sms_apply
template <> struct SmsGeo<3> { static constexpr int TX = 8, TY = 8, TZ = 8, SX = 12, SY = 12, SZ = 12, K = 125; };
template <> struct SmsGeo<2> { static constexpr int TX = 16, TY = 16, TZ = 1, SX = 20, SY = 20, SZ = 1, K = 25; };

struct SmsDims { int n0, n1, n2, nc0, nc1; }; // lattice nodes per axis; classes of the first two axes

// the dense offset-ordered form of CSR row `node` at lattice point (ix, iy, iz) into `dense` (K doubles, zeroed here) by the 64 lanes of a wave
// or a one-wave block; returns whether this lane met a coupling beyond the window.  The caller separates the phases (zero | scatter | read).
template <int DIM>
__device__ inline void sms_zero(double *dense, int lane) {
  for (int o = lane; o < SmsGeo<DIM>::K; o += 64) dense[o] = 0.0;
}
template <int DIM>
__device__ inline bool sms_expand(const SmsDims d, int ix, int iy, int iz, int64_t node, const int32_t *__restrict__ lon, const int64_t *__restrict__ rp,
                                  const int32_t *__restrict__ col, const double *__restrict__ val, double *dense, int lane) {
  const int64_t rs = rp[node];
  const int len = int(rp[node + 1] - rs);
  bool beyond = false;
  for (int k = lane; k < len; k += 64) {
    const int p = lon[col[rs + k]];
    const int jx = p % d.n0, jy = (p / d.n0) % d.n1, jz = p / (d.n0 * d.n1);
    const int dx = jx - ix + 2, dy = jy - iy + 2, dz = DIM == 3 ? jz - iz + 2 : 2;
    if (dx < 0 || dx > 4 || dy < 0 || dy > 4 || dz < 0 || dz > 4) { beyond = true; continue; }
    dense[DIM == 3 ? (dz * 5 + dy) * 5 + dx : dy * 5 + dx] = val[rs + k];
  }
  return beyond;
}

// table[c][K] and tmax[c] = table[classes * K + c] of class c = blockIdx.x from the row at its first lattice point; first: the per-axis first
// points of the axis classes, [nc0 | nc1 | nc2]
template <int DIM>
__global__ __launch_bounds__(64) void k_sms_table(SmsDims d, int classes, const int32_t *__restrict__ first, const int32_t *__restrict__ nol,
                                                  const int32_t *__restrict__ lon, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
                                                  const double *__restrict__ val, double *__restrict__ table) {
  constexpr int K = SmsGeo<DIM>::K;
  __shared__ double dense[K];
  __shared__ double red[64];
  const int c = blockIdx.x, lane = threadIdx.x;
  const int ix = first[c % d.nc0], iy = first[d.nc0 + (c / d.nc0) % d.nc1], iz = DIM == 3 ? first[d.nc0 + d.nc1 + c / (d.nc0 * d.nc1)] : 0;
  const int64_t node = nol[ix + d.n0 * (iy + d.n1 * iz)];
  sms_zero<DIM>(dense, lane);
  __syncthreads();
  (void)sms_expand<DIM>(d, ix, iy, iz, node, lon, rp, col, val, dense, lane); // (a coupling beyond the window: k_sms_classify sends the row to the list)
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

// one wave per lattice point: class id or kSmsIrregular into cls, irregular rows into rows[< cap] (counter counts all of them)
template <int DIM>
__global__ __launch_bounds__(256) void k_sms_classify(SmsDims d, int classes, int64_t N, const uint8_t *__restrict__ axcls, const int32_t *__restrict__ nol,
                                                      const int32_t *__restrict__ lon, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
                                                      const double *__restrict__ val, const double *__restrict__ table, uint16_t *__restrict__ cls,
                                                      int32_t *__restrict__ rows, int32_t cap, int32_t *__restrict__ counter) {
  constexpr int K = SmsGeo<DIM>::K;
  __shared__ double dense_all[4][K];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = int64_t(blockIdx.x) * 4 + w;
  const bool live = p < N;
  double *dense = dense_all[w];
  sms_zero<DIM>(dense, lane);
  __syncthreads();
  int ix = 0, iy = 0, iz = 0, c = 0;
  int64_t node = 0;
  bool bad = false;
  if (live) {
    ix = int(p % d.n0); iy = int((p / d.n0) % d.n1); iz = int(p / (int64_t(d.n0) * d.n1));
    c = axcls[ix] + d.nc0 * (axcls[d.n0 + iy] + d.nc1 * (DIM == 3 ? axcls[d.n0 + d.n1 + iz] : 0));
    node = nol[p];
    bad = sms_expand<DIM>(d, ix, iy, iz, node, lon, rp, col, val, dense, lane);
  }
  __syncthreads();
  if (!live) return;
  const double bound = 1e-12 * table[int64_t(classes) * K + c];
  for (int o = lane; o < K; o += 64) bad = bad || !(fabs(dense[o] - table[int64_t(c) * K + o]) <= bound); // (a NaN fails)
  const bool irregular = __any(bad);
  if (lane == 0) {
    cls[p] = irregular ? uint16_t(kSmsIrregular) : uint16_t(c);
    if (irregular) {
      const int32_t at = atomicAdd(counter, 1);
      if (at < cap) rows[at] = int32_t(node);
    }
  }
}

// the 5^DIM-term sum of one output in fixed offset order; xs: the LDS entry of offset (-2, -2, -2)
template <int DIM, class TP>
__device__ __forceinline__ double sms_sum(TP T, const double *xs) {
  using G = SmsGeo<DIM>;
  double acc = 0;
#pragma unroll
  for (int dz = 0; dz < (DIM == 3 ? 5 : 1); ++dz)
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) acc = fma(T[(dz * 5 + dy) * 5 + dx], xs[(dz * G::SY + dy) * G::SX + dx], acc);
  return acc;
}

template <int DIM>
__global__ __launch_bounds__(256) void k_sms_apply(SmsDims d, int tiles_x, int tiles_y, const int32_t *__restrict__ nol, const uint16_t *__restrict__ cls,
                                                   const double *__restrict__ table, const double *__restrict__ x, double *__restrict__ y) {
  using G = SmsGeo<DIM>;
  constexpr int S = G::SX * G::SY * G::SZ, TILE = G::TX * G::TY * G::TZ, HZ = DIM == 3 ? 2 : 0;
  __shared__ double xs[S];
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, bz = blockIdx.x / (tiles_x * tiles_y);
  const int ox = bx * G::TX, oy = by * G::TY, oz = bz * G::TZ; // first output of the tile
  // The loads of every phase are issued together, so that the block waits for one memory round trip per phase instead of one per entry (the
  // kernel is bound by these latencies, not by traffic): the lattice map of the LDS entries, the class and the node of the outputs | the
  // entries of x | (barrier) the table rows and the sums.
  constexpr int NG = (S + 255) / 256, NO = TILE / 256;
  int src[NG], p_out[NO], c_out[NO], node_out[NO];
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const int s = tid + 256 * k;
    const int gx = ox - 2 + s % G::SX, gy = oy - 2 + (s / G::SX) % G::SY, gz = oz - HZ + s / (G::SX * G::SY);
    const bool in = s < S && gx >= 0 && gx < d.n0 && gy >= 0 && gy < d.n1 && gz >= 0 && gz < d.n2;
    src[k] = in ? nol[gx + d.n0 * (gy + d.n1 * gz)] : -1;
  }
#pragma unroll
  for (int k = 0; k < NO; ++k) {
    const int o = tid + 256 * k;
    const int gx = ox + o % G::TX, gy = oy + (o / G::TX) % G::TY, gz = oz + o / (G::TX * G::TY);
    const bool inside = gx < d.n0 && gy < d.n1 && gz < d.n2;
    p_out[k] = inside ? gx + d.n0 * (gy + d.n1 * gz) : -1;
    c_out[k] = inside ? int(cls[p_out[k]]) : kSmsIrregular;
    node_out[k] = inside ? nol[p_out[k]] : 0;
  }
  double v[NG];
#pragma unroll
  for (int k = 0; k < NG; ++k) v[k] = src[k] >= 0 ? x[src[k]] : 0.0; // beyond the lattice: the table holds no coupling there
#pragma unroll
  for (int k = 0; k < NG; ++k)
    if (tid + 256 * k < S) xs[tid + 256 * k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NO; ++k) {
    const int o = tid + 256 * k;
    const int lx = o % G::TX, ly = (o / G::TX) % G::TY, lz = o / (G::TX * G::TY);
    const int c = c_out[k];
    const bool valid = c != kSmsIrregular;
    const unsigned long long m = __ballot(valid);
    if (m == 0) continue; // (wave-uniform)
    const double *w = xs + (lz * G::SY + ly) * G::SX + lx;
    const int c0 = __builtin_amdgcn_readfirstlane(__shfl(c, __ffsll((long long)m) - 1));
    double acc;
    // one class in the wave: the table row through the constant address space, i.e. wave-uniform (scalar) loads -- the table is written by
    // an earlier kernel only.  (With the same pointer type in both branches the compiler merges them into one that loads the row per lane.)
    if (__all(!valid || c == c0)) acc = sms_sum<DIM>((const __attribute__((address_space(4))) double *)(table + c0 * G::K), w);
    else acc = sms_sum<DIM>(table + (valid ? c : c0) * G::K, w);
    if (valid) y[node_out[k]] = acc;
  }
}

// ---- host drivers

static SmsDims sms_dims(const ifem_ctx *ctx) {
  const PLattice &L = ctx->p_lattice;
  const SmStencil &T = ctx->sm_stencil;
  return {L.n[0], L.n[1], L.n[2], T.ncls[0], T.ncls[1]};
}

void sm_stencil_apply(ifem_ctx *ctx, const double *x, double *y) {
  const SmStencil &T = ctx->sm_stencil;
  const PLattice &L = ctx->p_lattice;
  const SmsDims d = sms_dims(ctx);
  const double N = double(ctx->nPo);
  hipStream_t s = ctx->stream;
  if (ctx->dim == 3) {
    using G = SmsGeo<3>;
    const int tx = (d.n0 + G::TX - 1) / G::TX, ty = (d.n1 + G::TY - 1) / G::TY, tz = (d.n2 + G::TZ - 1) / G::TZ;
    // the gather with its halo (index + value per LDS entry), class + index + result per row; the irregular rows as CSR rows
    KScope ks(ctx, IFEM_KC_SPMV_SM, double(tx) * ty * tz * (G::SX * G::SY * G::SZ) * 12.0 + N * 14.0 + double(T.n_irregular) * (G::K * 12.0 + 16.0));
    hipLaunchKernelGGL(k_sms_apply<3>, dim3(unsigned(tx * ty * tz)), dim3(256), 0, s, d, tx, ty, L.node_of_lattice.p, T.cls.p, T.table.p, x, y);
    spmv_sm_rows(ctx, x, y, T.n_irregular, T.rows.p);
  } else {
    using G = SmsGeo<2>;
    const int tx = (d.n0 + G::TX - 1) / G::TX, ty = (d.n1 + G::TY - 1) / G::TY;
    KScope ks(ctx, IFEM_KC_SPMV_SM, double(tx) * ty * (G::SX * G::SY) * 12.0 + N * 14.0 + double(T.n_irregular) * (G::K * 12.0 + 16.0));
    hipLaunchKernelGGL(k_sms_apply<2>, dim3(unsigned(tx * ty)), dim3(256), 0, s, d, tx, ty, L.node_of_lattice.p, T.cls.p, T.table.p, x, y);
    spmv_sm_rows(ctx, x, y, T.n_irregular, T.rows.p);
  }
}

// tables and classes of the present S_m values; false: more than 1/8 of the rows are irregular
static bool sm_stencil_build(ifem_ctx *ctx) {
  SmStencil &T = ctx->sm_stencil;
  const PLattice &L = ctx->p_lattice;
  const int dim = ctx->dim, K = dim == 3 ? 125 : 25;
  const int64_t N = ctx->nPo;
  hipStream_t s = ctx->stream;
  if (T.axcls.n == 0) { // the lattice part: once per context
    std::vector<uint8_t> ax, a;
    std::vector<int32_t> first, f;
    for (int d = 0; d < 3; ++d) {
      T.ncls[d] = lattice_axis_classes(L.n[d], a, f);
      ax.insert(ax.end(), a.begin(), a.end());
      first.insert(first.end(), f.begin(), f.end());
    }
    T.classes = T.ncls[0] * T.ncls[1] * T.ncls[2];
    T.first.upload(first.data(), first.size(), s);
    T.axcls.upload(ax.data(), ax.size(), s);
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
    T.table.alloc(size_t(T.classes) * (K + 1), "the stencil tables of S_m");
    T.cls.alloc(size_t(N), "the class ids of the S_m stencil product");
    T.rows.alloc(size_t(N / 8 + 1), "the irregular rows of the S_m stencil product");
    T.counter.alloc(1);
  }
  const SmsDims d = sms_dims(ctx);
  const int32_t cap = int32_t(T.rows.n);
  IFEM_HIP_CHECK(hipMemsetAsync(T.counter.p, 0, sizeof(int32_t), s));
  const PlanarCsr &M = ctx->Sm;
  if (dim == 3) {
    hipLaunchKernelGGL(k_sms_table<3>, dim3(unsigned(T.classes)), dim3(64), 0, s, d, T.classes, T.first.p, L.node_of_lattice.p, L.lattice_of_node.p, M.rowptr.p, M.col.p, M.val.p, T.table.p);
    hipLaunchKernelGGL(k_sms_classify<3>, dim3(unsigned((N + 3) / 4)), dim3(256), 0, s, d, T.classes, N, T.axcls.p, L.node_of_lattice.p, L.lattice_of_node.p, M.rowptr.p, M.col.p, M.val.p,
                       T.table.p, T.cls.p, T.rows.p, cap, T.counter.p);
  } else {
    hipLaunchKernelGGL(k_sms_table<2>, dim3(unsigned(T.classes)), dim3(64), 0, s, d, T.classes, T.first.p, L.node_of_lattice.p, L.lattice_of_node.p, M.rowptr.p, M.col.p, M.val.p, T.table.p);
    hipLaunchKernelGGL(k_sms_classify<2>, dim3(unsigned((N + 3) / 4)), dim3(256), 0, s, d, T.classes, N, T.axcls.p, L.node_of_lattice.p, L.lattice_of_node.p, M.rowptr.p, M.col.p, M.val.p,
                       T.table.p, T.cls.p, T.rows.p, cap, T.counter.p);
  }
  int32_t count = 0;
  IFEM_HIP_CHECK(hipMemcpyAsync(&count, T.counter.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  IFEM_HIP_CHECK(hipGetLastError());
  T.n_irregular = count;
  return int64_t(count) * 8 <= N;
}

// the new product against the fp64 CSR product of the assembled S_m on a pseudo-random vector, formed and compared on the device (three scalars
// come back: a re-formed S_m pays this on every level)
static bool sm_stencil_probe(ifem_ctx *ctx, double *err_out) {
  const int64_t n = ctx->nPo;
  const size_t un = size_t(n);
  hipStream_t s = ctx->stream;
  DBuf<double> de, d0, d1;
  de.alloc(un); d0.alloc(un); d1.alloc(un);
  vec_rough(ctx, n, 0x5EED, de.p); // a fixed hash of the index: the same probe on every run
  IFEM_HIP_CHECK(hipMemsetAsync(d1.p, 0xff, un * sizeof(double), s)); // NaN: a row nobody produced shows
  spmv_sm(ctx, de.p, d0.p, /*use_f32=*/false);
  sm_stencil_apply(ctx, de.p, d1.p);
  double lo = 0, hi = 0;
  v_minmax(ctx, n, d0.p, &lo, &hi);
  const double ymax = std::max(std::fabs(lo), std::fabs(hi));
  v_axpy(ctx, n, -1.0, d0.p, d1.p); // d1 = stencil - CSR
  v_minmax(ctx, n, d1.p, &lo, &hi);
  const double err = std::max(std::fabs(lo), std::fabs(hi));
  const double sq = v_dot(ctx, n, d1.p, d1.p); // (a NaN passes a minimum / maximum unseen, not a sum)
  IFEM_HIP_CHECK(hipGetLastError());
  const bool finite = std::isfinite(sq) && std::isfinite(err) && std::isfinite(ymax) && err < 1e299;
  if (err_out) *err_out = !finite ? INFINITY : (ymax > 0 ? err / ymax : err);
  return finite && err <= 1e-12 * ymax;
}

void sm_stencil_setup(ifem_ctx *ctx, int verbose) {
  SmStencil &T = ctx->sm_stencil;
  if (T.off || T.failed || T.version == ctx->sm_version) return;
  T.version = ctx->sm_version;
  T.ready = false;
  if (ctx->halo.nranks > 1 || !ctx->sm_valid || ctx->Sm.n_rows == 0 || ctx->Sm.n_rows != ctx->nPo || !p_lattice_ensure(ctx)) return;
  const char *why = nullptr;
  double err = 0;
  if (!sm_stencil_build(ctx)) why = "more than 1/8 of the rows differ from their class";
  else if (!sm_stencil_probe(ctx, &err)) { why = "the stencil product misses the assembled matrix (1e-12)"; T.failed = true; } // off for this context
  if (why) {
    if (verbose && !T.said) fprintf(stderr, "[ifem] S_m: %s (%lld irregular rows of %lld, probe %.2e): this level keeps the CSR product\n", why, (long long)T.n_irregular, (long long)ctx->nPo, err);
    T.said = true;
    return;
  }
  T.ready = true;
  // the single-precision copy of the values has no reader on this level any more
  ctx->Sm_f32.release();
  ctx->Sm_f32.stale();
  if (verbose) fprintf(stderr, "[ifem] S_m: stencil product on the %d x %d x %d lattice, %d classes, %lld irregular rows, probe %.2e\n", ctx->p_lattice.n[0], ctx->p_lattice.n[1],
                       ctx->p_lattice.n[2], T.classes, (long long)T.n_irregular, err);
}

} // namespace ifem
