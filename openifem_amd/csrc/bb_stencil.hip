// bb_stencil.hip -- y = B x and y = B^T x from stencil tables over the pressure and velocity lattices of a uniform box level.
//
// On an axis-aligned uniform box with Q2 velocity and Q1 pressure the velocity nodes are the lattice n_u = 2 cells + 1 per axis and pressure point
// j sits at velocity point 2 j.  A B row at pressure point j couples the velocity points within +-2 of 2 j per axis, times dim components
// (375 entries in 3D, 50 in 2D); a B^T row at velocity point i the pressure points j with |i - 2 j| <= 2, at most 3 per axis, times dim row
// components (81 / 18).  Rows with the same position signature hold the same numbers, so the stored-matrix products stream 7.5 GB of (value,
// column) pairs at 128^3 cells that are a few hundred distinct rows; from tables a product reads its vector, a lattice map, a class id per row
// and writes the result.
//
// Eligibility: one rank, no hanging-node line, uniform box cells, Q2 / Q1, both node sets full lattices (setup.hip::u_lattice_ensure), the
// blocks those of an INS assembly (an SCnsIM assembly leaves stabilised blocks: CSR).  Q1 velocity keeps CSR.  Everything else keeps
// linalg.hip::spmv_b / spmv_bt, and so do the products with other values on B's pattern, row parts and the single-precision copies.
//
// Tables (lattice_stencil.hpp; bb_stencil_setup, whenever an assembly wrote the blocks -- ifem_ctx::bb_version -- and only at solve set-up:
// solver.hip::ins_solve), for B and B^T separately, each from its own assembled values (with ifem_tuning::geo_cache = 2 both are masked copies;
// neither is assumed to be the transpose of the other):
//   signature  B row: that of its pressure point (lattice.cpp::lattice_axis_classes, distances capped at 2).  B^T row at point i of an axis of n
//              velocity nodes: (min(i, 4), min(n - 1 - i, 4)) and i mod 2 where both are capped (lattice_axis_classes_u).
//   window     B row at pressure point j: the 5 velocity points from 2 j - 2 per axis; B^T row at velocity point i: the 3 pressure points from
//              (i + 1) / 2 - 1 (the j with |i - 2 j| <= 2 are these without the last for odd i); dim values each.
//   probe      the new product against the CSR product that k_stencil_classify formed while it held the rows, so it needs no CSR launch.
// Apply:
//   k_bbs_apply_b   a block of 128 threads takes a tile of pressure points (3D 8 x 4 x 4, 2D 16 x 8), one output per thread, and gathers x
//                   through the velocity map into LDS one component at a time with a two-deep halo (19 x 11 x 11 doubles = 18.4 KB; 35 x 19); the
//                   loads of the next component are in flight while the present one is summed.  Every output is the window sum in the order
//                   component, offset.  A wave whose rows share a class reads the table row by wave-uniform loads, the others per lane.
//   k_bbs_apply_bt  a block of 256 threads takes a tile of velocity points (3D 16 x 8 x 4, 2D 32 x 16), two per thread, gathers the pressure
//                   values it needs (11 x 7 x 5; 19 x 11) into LDS and writes the dim components of each node through the velocity map.  The
//                   lanes of a wave take nodes of one parity (the class of an interior row is its parity), so that interior waves share a class.
//                   ADD: y += B^T x in the same pass (the second launch of the outer operator behind k_spmv_uu_pipe).
//   Irregular rows are skipped; the planar CSR kernels over the row list produce them in a second launch on the same stream.
// fp64 throughout, plain stores, no floating-point atomics, no scratch; every sum has a fixed order.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
#include "lattice_stencil.hpp"

namespace ifem {

constexpr int kBbsIrregular = kStencilIrregular;
constexpr int kBbsDeg = 2;
// B: tile of pressure points, LDS box of velocity points (2 T + 3 per axis), KO offsets per component
template <int DIM> struct BbsB;
template <> struct BbsB<3> { static constexpr int TX = 8, TY = 4, TZ = 4, SX = 19, SY = 11, SZ = 11, W = 5, KO = 125, K = 375; };
template <> struct BbsB<2> { static constexpr int TX = 16, TY = 8, TZ = 1, SX = 35, SY = 19, SZ = 1, W = 5, KO = 25, K = 50; };
// B^T: tile of velocity points (even origin), LDS box of pressure points (T / 2 + 3 per axis)
template <int DIM> struct BbsT;
template <> struct BbsT<3> { static constexpr int TX = 16, TY = 8, TZ = 4, SX = 11, SY = 7, SZ = 5, W = 3, KO = 27, K = 81; };
template <> struct BbsT<2> { static constexpr int TX = 32, TY = 16, TZ = 1, SX = 19, SY = 11, SZ = 1, W = 3, KO = 9, K = 18; };

// the operators for lattice_stencil.hpp: B rows over the pressure lattice, a wave per row (125 blocks); B^T rows over the velocity lattice, 16
// lanes per row (at most 27 blocks)
template <int D> struct BbsOpB {
  static constexpr int DIM = D, W = BbsB<D>::W, NC = D, NR = 1, G = 64;
  __host__ __device__ static constexpr int first_col(int j) { return kBbsDeg * j - kBbsDeg; }
  static int axis_classes(int n, std::vector<uint8_t> &cls, std::vector<int32_t> &first) { return lattice_axis_classes(n, cls, first); }
  static constexpr const char *table_name = "the stencil tables of B", *cls_name = "the class ids of a B / B^T stencil product",
                              *rows_name = "the irregular rows of a B / B^T stencil product";
};
template <int D> struct BbsOpT {
  static constexpr int DIM = D, W = BbsT<D>::W, NC = D, NR = D, G = 16;
  __host__ __device__ static constexpr int first_col(int i) { return (i + 1) / kBbsDeg - 1; }
  static int axis_classes(int n, std::vector<uint8_t> &cls, std::vector<int32_t> &first) { return lattice_axis_classes_u(n, kBbsDeg, cls, first); }
  static constexpr const char *table_name = "the stencil tables of B^T", *cls_name = BbsOpB<D>::cls_name, *rows_name = BbsOpB<D>::rows_name;
};

// acc + the window sum of one component in fixed offset order; xs: the LDS entry of the window's first offset, box rows of SX, planes of SX * SY
template <int DIM, int W, int SX, int SY, class TP>
__device__ __forceinline__ double bbs_sum(TP T, const double *xs, double acc) {
#pragma unroll
  for (int dz = 0; dz < (DIM == 3 ? W : 1); ++dz)
#pragma unroll
    for (int dy = 0; dy < W; ++dy)
#pragma unroll
      for (int dx = 0; dx < W; ++dx) acc = fma(T[(dz * W + dy) * W + dx], xs[(dz * SY + dy) * SX + dx], acc);
  return acc;
}

template <int DIM>
__global__ __launch_bounds__(128) void k_bbs_apply_b(StencilDims d, int tiles_x, int tiles_y, const int32_t *__restrict__ nol_p, const int32_t *__restrict__ nol_u,
                                                     const uint16_t *__restrict__ cls, const double *__restrict__ table, const double *__restrict__ x,
                                                     double *__restrict__ y) {
  using G = BbsB<DIM>;
  constexpr int S = G::SX * G::SY * G::SZ, NG = (S + 127) / 128, HZ = DIM == 3 ? kBbsDeg : 0;
  static_assert(G::TX * G::TY * G::TZ == 128, "one output per thread");
  __shared__ double xs[S];
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, bz = blockIdx.x / (tiles_x * tiles_y);
  const int ox = bx * G::TX, oy = by * G::TY, oz = bz * G::TZ; // first pressure point of the tile
  // The loads of every phase are issued together (the kernel is bound by these round trips, not by traffic): the velocity map of the LDS
  // entries, the class and the node of the output | component 0 of x | (barrier) the sums of component a while component a + 1 is in flight.
  int src[NG];
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const int s = tid + 128 * k;
    const int gx = kBbsDeg * ox - kBbsDeg + s % G::SX, gy = kBbsDeg * oy - kBbsDeg + (s / G::SX) % G::SY, gz = kBbsDeg * oz - HZ + s / (G::SX * G::SY);
    const bool in = s < S && gx >= 0 && gx < d.m[0] && gy >= 0 && gy < d.m[1] && gz >= 0 && gz < d.m[2];
    src[k] = in ? nol_u[gx + d.m[0] * (gy + d.m[1] * gz)] : -1;
  }
  const int lx = tid % G::TX, ly = (tid / G::TX) % G::TY, lz = tid / (G::TX * G::TY);
  const int gx = ox + lx, gy = oy + ly, gz = oz + lz;
  const bool inside = gx < d.n[0] && gy < d.n[1] && gz < d.n[2];
  const int p_out = inside ? gx + d.n[0] * (gy + d.n[1] * gz) : 0;
  const int c = inside ? int(cls[p_out]) : kBbsIrregular;
  const int node_out = inside ? nol_p[p_out] : 0;
  const bool valid = c != kBbsIrregular;
  const unsigned long long m = __ballot(valid);
  const int c0 = m ? __builtin_amdgcn_readfirstlane(__shfl(c, __ffsll((long long)m) - 1)) : 0;
  const bool uniform = __all(!valid || c == c0); // (wave-uniform)
  const double *w = xs + ((kBbsDeg * lz) * G::SY + kBbsDeg * ly) * G::SX + kBbsDeg * lx;
  double v[NG];
#pragma unroll
  for (int k = 0; k < NG; ++k) v[k] = src[k] >= 0 ? x[int64_t(src[k]) * DIM] : 0.0; // beyond the lattice: the table holds no coupling there
  double acc = 0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    if (a > 0) __syncthreads(); // the sums of the component before have read the box
#pragma unroll
    for (int k = 0; k < NG; ++k)
      if (tid + 128 * k < S) xs[tid + 128 * k] = v[k];
    __syncthreads();
    if (a + 1 < DIM) {
#pragma unroll
      for (int k = 0; k < NG; ++k) v[k] = src[k] >= 0 ? x[int64_t(src[k]) * DIM + (a + 1)] : 0.0;
    }
    if (m != 0) { // (wave-uniform)
      // one class in the wave: the table row through the constant address space, i.e. wave-uniform (scalar) loads -- the table is written by
      // an earlier kernel only.  (With the same pointer type in both branches the compiler merges them into one that loads the row per lane.)
      if (uniform) acc = bbs_sum<DIM, G::W, G::SX, G::SY>((const __attribute__((address_space(4))) double *)(table + c0 * G::K + a * G::KO), w, acc);
      else acc = bbs_sum<DIM, G::W, G::SX, G::SY>(table + (valid ? c : c0) * G::K + a * G::KO, w, acc);
    }
  }
  if (valid) y[node_out] = acc;
}

template <int DIM, bool ADD>
__global__ __launch_bounds__(256) void k_bbs_apply_bt(StencilDims d, int tiles_x, int tiles_y, const int32_t *__restrict__ nol_p, const int32_t *__restrict__ nol_u,
                                                      const uint16_t *__restrict__ cls, const double *__restrict__ table, const double *__restrict__ x,
                                                      double *__restrict__ y) {
  using G = BbsT<DIM>;
  constexpr int S = G::SX * G::SY * G::SZ, NG = (S + 255) / 256, NO = 2;
  static_assert(G::TX * G::TY * G::TZ == 256 * NO && G::TX % 2 == 0 && G::TY % 2 == 0 && (DIM == 2 || G::TZ % 2 == 0), "two outputs per thread, even tile origins");
  __shared__ double xs[S];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, bz = blockIdx.x / (tiles_x * tiles_y);
  const int ox = bx * G::TX, oy = by * G::TY, oz = bz * G::TZ; // first velocity point of the tile (even)
  // phases as in k_bbs_apply_b: the pressure map of the LDS entries, class and node of the outputs | x and, in add mode, y | (barrier) the sums
  int src[NG], c_out[NO], node_out[NO], lxyz[NO];
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const int s = tid + 256 * k;
    const int gx = ox / kBbsDeg - 1 + s % G::SX, gy = oy / kBbsDeg - 1 + (s / G::SX) % G::SY, gz = DIM == 3 ? oz / kBbsDeg - 1 + s / (G::SX * G::SY) : 0;
    const bool in = s < S && gx >= 0 && gx < d.m[0] && gy >= 0 && gy < d.m[1] && gz >= 0 && gz < d.m[2];
    src[k] = in ? nol_p[gx + d.m[0] * (gy + d.m[1] * gz)] : -1;
  }
#pragma unroll
  for (int k = 0; k < NO; ++k) {
    // the lanes of a wave take the nodes of one parity of the tile (3D: 8 parities of 64 nodes; 2D: 4 parities of 128 nodes in two halves)
    const int g = wave + 4 * k;
    int lx, ly, lz;
    if (DIM == 3) { lx = 2 * (lane & 7) + (g & 1); ly = 2 * ((lane >> 3) & 3) + ((g >> 1) & 1); lz = 2 * (lane >> 5) + (g >> 2); }
    else { lx = 2 * (lane & 15) + (g & 1); ly = 2 * ((lane >> 4) + 4 * (g >> 2)) + ((g >> 1) & 1); lz = 0; }
    const int gx = ox + lx, gy = oy + ly, gz = oz + lz;
    const bool inside = gx < d.n[0] && gy < d.n[1] && gz < d.n[2];
    const int p = inside ? gx + d.n[0] * (gy + d.n[1] * gz) : 0;
    c_out[k] = inside ? int(cls[p]) : kBbsIrregular;
    node_out[k] = inside ? nol_u[p] : 0;
    lxyz[k] = (((lz + 1) / 2) * G::SY + (ly + 1) / 2) * G::SX + (lx + 1) / 2; // the LDS entry of the window's first pressure point
  }
  double v[NG], yo[NO][DIM];
#pragma unroll
  for (int k = 0; k < NG; ++k) v[k] = src[k] >= 0 ? x[src[k]] : 0.0; // beyond the lattice: the table holds no coupling there
  if (ADD) {
#pragma unroll
    for (int k = 0; k < NO; ++k)
#pragma unroll
      for (int a = 0; a < DIM; ++a) yo[k][a] = c_out[k] != kBbsIrregular ? y[int64_t(node_out[k]) * DIM + a] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < NG; ++k)
    if (tid + 256 * k < S) xs[tid + 256 * k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NO; ++k) {
    const int c = c_out[k];
    const bool valid = c != kBbsIrregular;
    const unsigned long long m = __ballot(valid);
    if (m == 0) continue; // (wave-uniform)
    const double *w = xs + lxyz[k];
    const int c0 = __builtin_amdgcn_readfirstlane(__shfl(c, __ffsll((long long)m) - 1));
    double acc[DIM];
    if (__all(!valid || c == c0)) { // (the two pointer types: see k_bbs_apply_b)
#pragma unroll
      for (int a = 0; a < DIM; ++a) acc[a] = bbs_sum<DIM, G::W, G::SX, G::SY>((const __attribute__((address_space(4))) double *)(table + c0 * G::K + a * G::KO), w, 0.0);
    } else {
#pragma unroll
      for (int a = 0; a < DIM; ++a) acc[a] = bbs_sum<DIM, G::W, G::SX, G::SY>(table + (valid ? c : c0) * G::K + a * G::KO, w, 0.0);
    }
    if (valid) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) y[int64_t(node_out[k]) * DIM + a] = ADD ? yo[k][a] + acc[a] : acc[a];
    }
  }
}

// ---- host drivers

void bb_stencil_apply_b(ifem_ctx *ctx, const double *xu, double *yp) {
  const StencilClasses &T = ctx->bb_stencil.b;
  const StencilDims d = stencil_dims(ctx->p_lattice, ctx->u_lattice, T);
  const int dim = ctx->dim;
  hipStream_t s = ctx->stream;
  const int TX = dim == 3 ? BbsB<3>::TX : BbsB<2>::TX, TY = dim == 3 ? BbsB<3>::TY : BbsB<2>::TY, TZ = dim == 3 ? BbsB<3>::TZ : 1;
  const int box = dim == 3 ? BbsB<3>::SX * BbsB<3>::SY * BbsB<3>::SZ : BbsB<2>::SX * BbsB<2>::SY, K = dim == 3 ? BbsB<3>::K : BbsB<2>::K;
  const int tx = (d.n[0] + TX - 1) / TX, ty = (d.n[1] + TY - 1) / TY, tz = (d.n[2] + TZ - 1) / TZ;
  const unsigned blocks = unsigned(tx * ty * tz);
  // the gather with its halo (index once, one value per component and LDS entry), class + index + result per row; the irregular rows as CSR rows
  KScope ks(ctx, IFEM_KC_SPMV_BBT, double(blocks) * box * (4.0 + 8.0 * dim) + double(ctx->nPo) * 14.0 + double(T.n_irregular) * (K * 8.0 + K / dim * 4.0 + 16.0));
  if (dim == 3) hipLaunchKernelGGL(k_bbs_apply_b<3>, dim3(blocks), dim3(128), 0, s, d, tx, ty, ctx->p_lattice.node_of_lattice.p, ctx->u_lattice.node_of_lattice.p, T.cls.p, T.table.p, xu, yp);
  else hipLaunchKernelGGL(k_bbs_apply_b<2>, dim3(blocks), dim3(128), 0, s, d, tx, ty, ctx->p_lattice.node_of_lattice.p, ctx->u_lattice.node_of_lattice.p, T.cls.p, T.table.p, xu, yp);
  spmv_b_rows(ctx, xu, yp, T.n_irregular, T.rows.p);
}

void bb_stencil_apply_bt(ifem_ctx *ctx, const double *xp, double *yu, bool add) {
  const StencilClasses &T = ctx->bb_stencil.bt;
  const StencilDims d = stencil_dims(ctx->u_lattice, ctx->p_lattice, T);
  const int dim = ctx->dim;
  hipStream_t s = ctx->stream;
  const int TX = dim == 3 ? BbsT<3>::TX : BbsT<2>::TX, TY = dim == 3 ? BbsT<3>::TY : BbsT<2>::TY, TZ = dim == 3 ? BbsT<3>::TZ : 1;
  const int box = dim == 3 ? BbsT<3>::SX * BbsT<3>::SY * BbsT<3>::SZ : BbsT<2>::SX * BbsT<2>::SY, K = dim == 3 ? BbsT<3>::K : BbsT<2>::K;
  const int tx = (d.n[0] + TX - 1) / TX, ty = (d.n[1] + TY - 1) / TY, tz = (d.n[2] + TZ - 1) / TZ;
  const unsigned blocks = unsigned(tx * ty * tz);
  KScope ks(ctx, IFEM_KC_SPMV_BBT, double(blocks) * box * 12.0 + double(ctx->nUo) * (6.0 + 8.0 * dim * (add ? 2 : 1)) + double(T.n_irregular) * (K * 8.0 + K / dim * 4.0 + 16.0));
  const int32_t *np_ = ctx->p_lattice.node_of_lattice.p, *nu_ = ctx->u_lattice.node_of_lattice.p;
  if (dim == 3 && add) hipLaunchKernelGGL((k_bbs_apply_bt<3, true>), dim3(blocks), dim3(256), 0, s, d, tx, ty, np_, nu_, T.cls.p, T.table.p, xp, yu);
  else if (dim == 3) hipLaunchKernelGGL((k_bbs_apply_bt<3, false>), dim3(blocks), dim3(256), 0, s, d, tx, ty, np_, nu_, T.cls.p, T.table.p, xp, yu);
  else if (add) hipLaunchKernelGGL((k_bbs_apply_bt<2, true>), dim3(blocks), dim3(256), 0, s, d, tx, ty, np_, nu_, T.cls.p, T.table.p, xp, yu);
  else hipLaunchKernelGGL((k_bbs_apply_bt<2, false>), dim3(blocks), dim3(256), 0, s, d, tx, ty, np_, nu_, T.cls.p, T.table.p, xp, yu);
  spmv_bt_rows(ctx, xp, yu, T.n_irregular, T.rows.p, add);
}

// one block: tables, then the new product against the CSR product k_stencil_classify formed on a pseudo-random vector
static void bbs_setup_block(ifem_ctx *ctx, bool bt, int verbose, double *de, double *d0, double *d1) {
  StencilClasses &T = bt ? ctx->bb_stencil.bt : ctx->bb_stencil.b;
  T.ready = false;
  if (T.failed) return;
  const PLattice &P = ctx->p_lattice;
  const ULattice &U = ctx->u_lattice;
  const int dim = ctx->dim;
  const int64_t n_in = bt ? ctx->nPl : int64_t(dim) * ctx->nUl, n_out = bt ? int64_t(dim) * ctx->nUo : ctx->nPo;
  hipStream_t s = ctx->stream;
  vec_rough(ctx, n_in, bt ? 0xB7 : 0xB0, de); // a fixed hash of the index: the same probe on every run
  IFEM_HIP_CHECK(hipMemsetAsync(d1, 0xff, size_t(n_out) * sizeof(double), s)); // NaN: a row nobody produced shows
  const bool few = dim == 3 ? (bt ? stencil_build<BbsOpT<3>>(ctx, T, U, P, ctx->Bt, de, d0) : stencil_build<BbsOpB<3>>(ctx, T, P, U, ctx->B, de, d0))
                            : (bt ? stencil_build<BbsOpT<2>>(ctx, T, U, P, ctx->Bt, de, d0) : stencil_build<BbsOpB<2>>(ctx, T, P, U, ctx->B, de, d0));
  double err = 0;
  bool ok = false;
  if (few) {
    if (bt) bb_stencil_apply_bt(ctx, de, d1, false); else bb_stencil_apply_b(ctx, de, d1);
    ok = stencil_probe_compare(ctx, n_out, d0, d1, &err); // d1 = stencil - CSR
  }
  const char *name = bt ? "B^T" : "B";
  if (!stencil_decide(T, few, ok, err, name, bt ? ctx->nUo : ctx->nPo, "context", verbose)) return;
  if (verbose) fprintf(stderr, "[ifem] %s: stencil product, %d classes, %lld irregular rows, probe %.2e\n", name, T.classes, (long long)T.n_irregular, err);
}

void bb_stencil_setup(ifem_ctx *ctx, int verbose) {
  BbStencil &T = ctx->bb_stencil;
  if (T.off || T.version == ctx->bb_version) return;
  T.version = ctx->bb_version;
  T.b.ready = T.bt.ready = false;
  if (ctx->mg_fine) return; // a multigrid level uses B only to form its S_m
  if (T.scns || ctx->has_app || ctx->halo.nranks > 1 || ctx->kv != kBbsDeg || ctx->B.n_rows == 0 || ctx->B.n_rows != ctx->nPo || ctx->Bt.n_rows != ctx->nUo || !u_lattice_ensure(ctx)) return;
  T.builds++;
  // probe vector, reference and product of either block in one allocation: B (velocity, pressure, pressure), B^T (pressure, velocity, velocity)
  const size_t nu = size_t(ctx->dim) * size_t(ctx->nUl), np = size_t(ctx->nPl);
  DBuf<double> work;
  work.alloc(2 * (nu + np), "the probe vectors of the B / B^T stencil products");
  double *u0 = work.p, *u1 = u0 + nu, *p0 = u1 + nu, *p1 = p0 + np;
  bbs_setup_block(ctx, false, verbose, u0, p0, p1);
  bbs_setup_block(ctx, true, verbose, p0, u0, u1);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (`work` leaves scope)
}

} // namespace ifem
