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
// Build (bb_stencil_setup, whenever an assembly wrote the blocks -- ifem_ctx::bb_version -- and only at solve set-up: solver.hip::ins_solve), for
// B and B^T separately, each from its own assembled values (with ifem_tuning::geo_cache = 2 both are masked copies; neither is assumed to be the
// transpose of the other):
//   signature  B row: that of its pressure point (lattice.cpp::lattice_axis_classes, distances capped at 2).  B^T row at point i of an axis of n
//              velocity nodes: (min(i, 4), min(n - 1 - i, 4)) and i mod 2 where both are capped (lattice_axis_classes_u).
//   k_bbs_table     one block per class: the CSR row of the class's first lattice point expanded into the dense vector [component][offset]
//                   (x fastest; missing couplings 0), and max |entry| of it.
//   k_bbs_classify  a group of lanes per row (a wave for B, 16 lanes for B^T): expands the row the same way and compares it entry by entry with its class, |v - T| <= 1e-12 max |T[class]|.
//                   A row that fails (or couples beyond the window) is irregular: class id 0xFFFF, appended to the row list.  More than 1/8
//                   irregular rows: the block keeps the CSR product.  While it holds the row the group also forms the row's CSR product with the
//                   probe vector, so the probe needs no CSR launch of its own.
//   probe           pseudo-random e (a hash of the index), the new product against what k_bbs_classify formed, max |diff| <= 1e-12 max |ref|,
//                   compared on the device; a block that fails keeps the CSR product for the life of the context.
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
#include "ctx.hpp"
#include "kernels.hpp"

namespace ifem {

constexpr int kBbsIrregular = 0xFFFF;
constexpr int kBbsDeg = 2;
// B: tile of pressure points, LDS box of velocity points (2 T + 3 per axis), KO offsets per component
template <int DIM> struct BbsB;
template <> struct BbsB<3> { static constexpr int TX = 8, TY = 4, TZ = 4, SX = 19, SY = 11, SZ = 11, W = 5, KO = 125, K = 375; };
template <> struct BbsB<2> { static constexpr int TX = 16, TY = 8, TZ = 1, SX = 35, SY = 19, SZ = 1, W = 5, KO = 25, K = 50; };
// B^T: tile of velocity points (even origin), LDS box of pressure points (T / 2 + 3 per axis)
template <int DIM> struct BbsT;
template <> struct BbsT<3> { static constexpr int TX = 16, TY = 8, TZ = 4, SX = 11, SY = 7, SZ = 5, W = 3, KO = 27, K = 81; };
template <> struct BbsT<2> { static constexpr int TX = 32, TY = 16, TZ = 1, SX = 19, SY = 11, SZ = 1, W = 3, KO = 9, K = 18; };
template <int DIM, bool BT> struct BbsK { static constexpr int W = BT ? BbsT<DIM>::W : BbsB<DIM>::W, KO = BT ? BbsT<DIM>::KO : BbsB<DIM>::KO, K = KO * DIM; };

struct BbsDims { int np[3], nu[3], nc0, nc1; }; // pressure / velocity lattice nodes per axis; classes of the first two axes of the row lattice

// first pressure point of the window of velocity point i: the j with |i - 2 j| <= 2 are jb, jb + 1 and, for even i, jb + 2
__device__ __forceinline__ int bbs_jbase(int i) { return (i + 1) / kBbsDeg - 1; }

// The dense form of CSR row `node` (at point (ix, iy, iz) of its lattice) into `dense` (K doubles, zeroed by the caller) by the G lanes of a
// group; returns whether this lane met a coupling beyond the window.  e (the probe vector, may be null): this lane's share of the row's product
// with it is added to ref[0] (B) or ref[0 .. DIM) (B^T).  The caller separates the phases (zero | scatter | read).
template <int DIM, bool BT, int G>
__device__ inline bool bbs_expand(const BbsDims d, int ix, int iy, int iz, int64_t node, const int32_t *__restrict__ lon_col, const int64_t *__restrict__ rp,
                                  const int32_t *__restrict__ col, const double *__restrict__ val, double *dense, int lane, const double *__restrict__ e, double *ref) {
  constexpr int W = BbsK<DIM, BT>::W, KO = BbsK<DIM, BT>::KO;
  const int m0 = BT ? d.np[0] : d.nu[0], m1 = BT ? d.np[1] : d.nu[1]; // the column lattice
  const int64_t rs = rp[node];
  const int len = int(rp[node + 1] - rs);
  const double *vb = val + rs * DIM;
  bool beyond = false;
  for (int k = lane; k < len; k += G) {
    const int c = col[rs + k];
    double v[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) v[a] = vb[int64_t(a) * len + k];
    if (e) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        if (BT) ref[a] += v[a] * e[c];
        else ref[0] += v[a] * e[int64_t(c) * DIM + a];
      }
    }
    const int p = lon_col[c];
    const int jx = p % m0, jy = (p / m0) % m1, jz = p / (m0 * m1);
    int dx, dy, dz;
    if (BT) { dx = jx - bbs_jbase(ix); dy = jy - bbs_jbase(iy); dz = DIM == 3 ? jz - bbs_jbase(iz) : 0; }
    else { dx = jx - kBbsDeg * ix + kBbsDeg; dy = jy - kBbsDeg * iy + kBbsDeg; dz = DIM == 3 ? jz - kBbsDeg * iz + kBbsDeg : 0; }
    if (dx < 0 || dx >= W || dy < 0 || dy >= W || dz < 0 || dz >= W) { beyond = true; continue; }
    const int o = DIM == 3 ? (dz * W + dy) * W + dx : dy * W + dx;
#pragma unroll
    for (int a = 0; a < DIM; ++a) dense[a * KO + o] = v[a];
  }
  return beyond;
}

// table[c][K] and tmax[c] = table[classes * K + c] of class c = blockIdx.x from the row at its first lattice point; first: the per-axis first
// points of the axis classes, [nc0 | nc1 | nc2]
template <int DIM, bool BT>
__global__ __launch_bounds__(64) void k_bbs_table(BbsDims d, int classes, const int32_t *__restrict__ first, const int32_t *__restrict__ nol_row,
                                                  const int32_t *__restrict__ lon_col, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
                                                  const double *__restrict__ val, double *__restrict__ table) {
  constexpr int K = BbsK<DIM, BT>::K;
  __shared__ double dense[K];
  __shared__ double red[64];
  const int c = blockIdx.x, lane = threadIdx.x;
  const int n0 = BT ? d.nu[0] : d.np[0], n1 = BT ? d.nu[1] : d.np[1];
  const int ix = first[c % d.nc0], iy = first[d.nc0 + (c / d.nc0) % d.nc1], iz = DIM == 3 ? first[d.nc0 + d.nc1 + c / (d.nc0 * d.nc1)] : 0;
  const int64_t node = nol_row[ix + n0 * (iy + n1 * iz)];
  for (int o = lane; o < K; o += 64) dense[o] = 0.0;
  __syncthreads();
  (void)bbs_expand<DIM, BT, 64>(d, ix, iy, iz, node, lon_col, rp, col, val, dense, lane, nullptr, nullptr); // (a coupling beyond the window: k_bbs_classify sends the row to the list)
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

// G lanes per lattice point of the row lattice (a wave for the 125 blocks of a B row, 16 lanes for the at most 27 of a B^T row: with a wave
// per row the 17 M rows of B^T at 128^3 cells are as many waves that wait for four dependent loads each): class id or kBbsIrregular into cls,
// irregular rows into rows[< cap] (counter counts all of them), the row's CSR product with e into ref (B: ref[node], B^T: ref[node * DIM + a])
template <int DIM, bool BT, int G>
__global__ __launch_bounds__(256) void k_bbs_classify(BbsDims d, int classes, int64_t N, const uint8_t *__restrict__ axcls, const int32_t *__restrict__ nol_row,
                                                      const int32_t *__restrict__ lon_col, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
                                                      const double *__restrict__ val, const double *__restrict__ table, uint16_t *__restrict__ cls,
                                                      int32_t *__restrict__ rows, int32_t cap, int32_t *__restrict__ counter, const double *__restrict__ e,
                                                      double *__restrict__ ref) {
  constexpr int K = BbsK<DIM, BT>::K, NR = BT ? DIM : 1, RPB = 256 / G;
  __shared__ double dense_all[RPB][K];
  const int w = threadIdx.x / G, lane = threadIdx.x % G;
  const int64_t p = int64_t(blockIdx.x) * RPB + w;
  const bool live = p < N;
  const int n0 = BT ? d.nu[0] : d.np[0], n1 = BT ? d.nu[1] : d.np[1];
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
    const int ix = int(p % n0), iy = int((p / n0) % n1), iz = int(p / (int64_t(n0) * n1));
    c = axcls[ix] + d.nc0 * (axcls[n0 + iy] + d.nc1 * (DIM == 3 ? axcls[n0 + n1 + iz] : 0));
    node = nol_row[p];
    bad = bbs_expand<DIM, BT, G>(d, ix, iy, iz, node, lon_col, rp, col, val, dense, lane, e, r);
  }
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int a = 0; a < NR; ++a) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) r[a] += __shfl_xor(r[a], off, 64); // (stays inside the aligned group)
  }
  const double bound = 1e-12 * table[int64_t(classes) * K + c];
  for (int o = lane; o < K; o += G) bad = bad || !(fabs(dense[o] - table[int64_t(c) * K + o]) <= bound); // (a NaN fails)
  const unsigned long long group = (G == 64 ? ~0ull : (1ull << (G & 63)) - 1) << ((threadIdx.x & 63) / G * G);
  const bool irregular = (__ballot(bad) & group) != 0;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < NR; ++a) ref[node * NR + a] = r[a];
    cls[p] = irregular ? uint16_t(kBbsIrregular) : uint16_t(c);
    if (irregular) {
      const int32_t at = atomicAdd(counter, 1);
      if (at < cap) rows[at] = int32_t(node);
    }
  }
}

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
__global__ __launch_bounds__(128) void k_bbs_apply_b(BbsDims d, int tiles_x, int tiles_y, const int32_t *__restrict__ nol_p, const int32_t *__restrict__ nol_u,
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
    const bool in = s < S && gx >= 0 && gx < d.nu[0] && gy >= 0 && gy < d.nu[1] && gz >= 0 && gz < d.nu[2];
    src[k] = in ? nol_u[gx + d.nu[0] * (gy + d.nu[1] * gz)] : -1;
  }
  const int lx = tid % G::TX, ly = (tid / G::TX) % G::TY, lz = tid / (G::TX * G::TY);
  const int gx = ox + lx, gy = oy + ly, gz = oz + lz;
  const bool inside = gx < d.np[0] && gy < d.np[1] && gz < d.np[2];
  const int p_out = inside ? gx + d.np[0] * (gy + d.np[1] * gz) : 0;
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
__global__ __launch_bounds__(256) void k_bbs_apply_bt(BbsDims d, int tiles_x, int tiles_y, const int32_t *__restrict__ nol_p, const int32_t *__restrict__ nol_u,
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
    const bool in = s < S && gx >= 0 && gx < d.np[0] && gy >= 0 && gy < d.np[1] && gz >= 0 && gz < d.np[2];
    src[k] = in ? nol_p[gx + d.np[0] * (gy + d.np[1] * gz)] : -1;
  }
#pragma unroll
  for (int k = 0; k < NO; ++k) {
    // the lanes of a wave take the nodes of one parity of the tile (3D: 8 parities of 64 nodes; 2D: 4 parities of 128 nodes in two halves)
    const int g = wave + 4 * k;
    int lx, ly, lz;
    if (DIM == 3) { lx = 2 * (lane & 7) + (g & 1); ly = 2 * ((lane >> 3) & 3) + ((g >> 1) & 1); lz = 2 * (lane >> 5) + (g >> 2); }
    else { lx = 2 * (lane & 15) + (g & 1); ly = 2 * ((lane >> 4) + 4 * (g >> 2)) + ((g >> 1) & 1); lz = 0; }
    const int gx = ox + lx, gy = oy + ly, gz = oz + lz;
    const bool inside = gx < d.nu[0] && gy < d.nu[1] && gz < d.nu[2];
    const int p = inside ? gx + d.nu[0] * (gy + d.nu[1] * gz) : 0;
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

static BbsDims bbs_dims(const ifem_ctx *ctx, const BbStencil::Block &T) {
  const PLattice &P = ctx->p_lattice;
  const ULattice &U = ctx->u_lattice;
  return {{P.n[0], P.n[1], P.n[2]}, {U.n[0], U.n[1], U.n[2]}, T.ncls[0], T.ncls[1]};
}

void bb_stencil_apply_b(ifem_ctx *ctx, const double *xu, double *yp) {
  const BbStencil::Block &T = ctx->bb_stencil.b;
  const BbsDims d = bbs_dims(ctx, T);
  const int dim = ctx->dim;
  hipStream_t s = ctx->stream;
  const int TX = dim == 3 ? BbsB<3>::TX : BbsB<2>::TX, TY = dim == 3 ? BbsB<3>::TY : BbsB<2>::TY, TZ = dim == 3 ? BbsB<3>::TZ : 1;
  const int box = dim == 3 ? BbsB<3>::SX * BbsB<3>::SY * BbsB<3>::SZ : BbsB<2>::SX * BbsB<2>::SY, K = dim == 3 ? BbsB<3>::K : BbsB<2>::K;
  const int tx = (d.np[0] + TX - 1) / TX, ty = (d.np[1] + TY - 1) / TY, tz = (d.np[2] + TZ - 1) / TZ;
  const unsigned blocks = unsigned(tx * ty * tz);
  // the gather with its halo (index once, one value per component and LDS entry), class + index + result per row; the irregular rows as CSR rows
  KScope ks(ctx, IFEM_KC_SPMV_BBT, double(blocks) * box * (4.0 + 8.0 * dim) + double(ctx->nPo) * 14.0 + double(T.n_irregular) * (K * 8.0 + K / dim * 4.0 + 16.0));
  if (dim == 3) hipLaunchKernelGGL(k_bbs_apply_b<3>, dim3(blocks), dim3(128), 0, s, d, tx, ty, ctx->p_lattice.node_of_lattice.p, ctx->u_lattice.node_of_lattice.p, T.cls.p, T.table.p, xu, yp);
  else hipLaunchKernelGGL(k_bbs_apply_b<2>, dim3(blocks), dim3(128), 0, s, d, tx, ty, ctx->p_lattice.node_of_lattice.p, ctx->u_lattice.node_of_lattice.p, T.cls.p, T.table.p, xu, yp);
  spmv_b_rows(ctx, xu, yp, T.n_irregular, T.rows.p);
}

void bb_stencil_apply_bt(ifem_ctx *ctx, const double *xp, double *yu, bool add) {
  const BbStencil::Block &T = ctx->bb_stencil.bt;
  const BbsDims d = bbs_dims(ctx, T);
  const int dim = ctx->dim;
  hipStream_t s = ctx->stream;
  const int TX = dim == 3 ? BbsT<3>::TX : BbsT<2>::TX, TY = dim == 3 ? BbsT<3>::TY : BbsT<2>::TY, TZ = dim == 3 ? BbsT<3>::TZ : 1;
  const int box = dim == 3 ? BbsT<3>::SX * BbsT<3>::SY * BbsT<3>::SZ : BbsT<2>::SX * BbsT<2>::SY, K = dim == 3 ? BbsT<3>::K : BbsT<2>::K;
  const int tx = (d.nu[0] + TX - 1) / TX, ty = (d.nu[1] + TY - 1) / TY, tz = (d.nu[2] + TZ - 1) / TZ;
  const unsigned blocks = unsigned(tx * ty * tz);
  KScope ks(ctx, IFEM_KC_SPMV_BBT, double(blocks) * box * 12.0 + double(ctx->nUo) * (6.0 + 8.0 * dim * (add ? 2 : 1)) + double(T.n_irregular) * (K * 8.0 + K / dim * 4.0 + 16.0));
  const int32_t *np_ = ctx->p_lattice.node_of_lattice.p, *nu_ = ctx->u_lattice.node_of_lattice.p;
  if (dim == 3 && add) hipLaunchKernelGGL((k_bbs_apply_bt<3, true>), dim3(blocks), dim3(256), 0, s, d, tx, ty, np_, nu_, T.cls.p, T.table.p, xp, yu);
  else if (dim == 3) hipLaunchKernelGGL((k_bbs_apply_bt<3, false>), dim3(blocks), dim3(256), 0, s, d, tx, ty, np_, nu_, T.cls.p, T.table.p, xp, yu);
  else if (add) hipLaunchKernelGGL((k_bbs_apply_bt<2, true>), dim3(blocks), dim3(256), 0, s, d, tx, ty, np_, nu_, T.cls.p, T.table.p, xp, yu);
  else hipLaunchKernelGGL((k_bbs_apply_bt<2, false>), dim3(blocks), dim3(256), 0, s, d, tx, ty, np_, nu_, T.cls.p, T.table.p, xp, yu);
  spmv_bt_rows(ctx, xp, yu, T.n_irregular, T.rows.p, add);
}

// tables and classes of the present values of one block, and its CSR product with e into ref; false: more than 1/8 of the rows are irregular
template <int DIM, bool BT>
static bool bbs_build(ifem_ctx *ctx, BbStencil::Block &T, const double *e, double *ref) {
  const PLattice &P = ctx->p_lattice;
  const ULattice &U = ctx->u_lattice;
  constexpr int K = BbsK<DIM, BT>::K;
  const int64_t N = BT ? ctx->nUo : ctx->nPo;
  hipStream_t s = ctx->stream;
  if (T.axcls.n == 0) { // the lattice part: once per context
    std::vector<uint8_t> ax, a;
    std::vector<int32_t> first, f;
    for (int d = 0; d < 3; ++d) {
      T.ncls[d] = BT ? lattice_axis_classes_u(U.n[d], kBbsDeg, a, f) : lattice_axis_classes(P.n[d], a, f);
      ax.insert(ax.end(), a.begin(), a.end());
      first.insert(first.end(), f.begin(), f.end());
    }
    T.classes = T.ncls[0] * T.ncls[1] * T.ncls[2];
    T.first.upload(first.data(), first.size(), s);
    T.axcls.upload(ax.data(), ax.size(), s);
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
    T.table.alloc(size_t(T.classes) * (K + 1), BT ? "the stencil tables of B^T" : "the stencil tables of B");
    T.cls.alloc(size_t(N), "the class ids of a B / B^T stencil product");
    T.rows.alloc(size_t(N / 8 + 1), "the irregular rows of a B / B^T stencil product");
    T.counter.alloc(1);
  }
  const BbsDims d = bbs_dims(ctx, T);
  const int32_t cap = int32_t(T.rows.n);
  IFEM_HIP_CHECK(hipMemsetAsync(T.counter.p, 0, sizeof(int32_t), s));
  const PlanarCsr &M = BT ? ctx->Bt : ctx->B;
  const int32_t *nol_row = BT ? U.node_of_lattice.p : P.node_of_lattice.p, *lon_col = BT ? P.lattice_of_node.p : U.lattice_of_node.p;
  hipLaunchKernelGGL((k_bbs_table<DIM, BT>), dim3(unsigned(T.classes)), dim3(64), 0, s, d, T.classes, T.first.p, nol_row, lon_col, M.rowptr.p, M.col.p, M.val.p, T.table.p);
  constexpr int G = BT ? 16 : 64, RPB = 256 / G;
  hipLaunchKernelGGL((k_bbs_classify<DIM, BT, G>), dim3(unsigned((N + RPB - 1) / RPB)), dim3(256), 0, s, d, T.classes, N, T.axcls.p, nol_row, lon_col, M.rowptr.p, M.col.p, M.val.p, T.table.p,
                     T.cls.p, T.rows.p, cap, T.counter.p, e, ref);
  int32_t count = 0;
  IFEM_HIP_CHECK(hipMemcpyAsync(&count, T.counter.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  IFEM_HIP_CHECK(hipGetLastError());
  T.n_irregular = count;
  return int64_t(count) * 8 <= N;
}

// one block: tables, then the new product against the CSR product k_bbs_classify formed on a pseudo-random vector, compared on the device
// (three scalars come back)
static void bbs_setup_block(ifem_ctx *ctx, bool bt, int verbose, double *de, double *d0, double *d1) {
  BbStencil::Block &T = bt ? ctx->bb_stencil.bt : ctx->bb_stencil.b;
  T.ready = false;
  if (T.failed) return;
  const int dim = ctx->dim;
  const int64_t n_in = bt ? ctx->nPl : int64_t(dim) * ctx->nUl, n_out = bt ? int64_t(dim) * ctx->nUo : ctx->nPo;
  hipStream_t s = ctx->stream;
  vec_rough(ctx, n_in, bt ? 0xB7 : 0xB0, de); // a fixed hash of the index: the same probe on every run
  IFEM_HIP_CHECK(hipMemsetAsync(d1, 0xff, size_t(n_out) * sizeof(double), s)); // NaN: a row nobody produced shows
  const bool few = dim == 3 ? (bt ? bbs_build<3, true>(ctx, T, de, d0) : bbs_build<3, false>(ctx, T, de, d0))
                            : (bt ? bbs_build<2, true>(ctx, T, de, d0) : bbs_build<2, false>(ctx, T, de, d0));
  const char *why = nullptr;
  double err = 0;
  if (!few) why = "more than 1/8 of the rows differ from their class";
  else {
    if (bt) bb_stencil_apply_bt(ctx, de, d1, false); else bb_stencil_apply_b(ctx, de, d1);
    double lo = 0, hi = 0;
    v_minmax(ctx, n_out, d0, &lo, &hi);
    const double ymax = std::max(std::fabs(lo), std::fabs(hi));
    v_axpy(ctx, n_out, -1.0, d0, d1); // d1 = stencil - CSR
    v_minmax(ctx, n_out, d1, &lo, &hi);
    err = std::max(std::fabs(lo), std::fabs(hi));
    const double sq = v_dot(ctx, n_out, d1, d1); // (a NaN passes a minimum / maximum unseen, not a sum)
    IFEM_HIP_CHECK(hipGetLastError());
    const bool finite = std::isfinite(sq) && std::isfinite(err) && std::isfinite(ymax) && err < 1e299;
    const bool ok = finite && err <= 1e-12 * ymax;
    err = !finite ? INFINITY : (ymax > 0 ? err / ymax : err);
    if (!ok) { why = "the stencil product misses the assembled matrix (1e-12)"; T.failed = true; } // off for this context
  }
  const char *name = bt ? "B^T" : "B";
  if (why) {
    if (verbose && !T.said) fprintf(stderr, "[ifem] %s: %s (%lld irregular rows of %lld, probe %.2e): this context keeps the CSR product\n", name, why, (long long)T.n_irregular,
                                    (long long)(bt ? ctx->nUo : ctx->nPo), err);
    T.said = true;
    return;
  }
  T.ready = true;
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
