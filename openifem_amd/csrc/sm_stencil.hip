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
// Tables (lattice_stencil.hpp; sm_stencil_setup, whenever S_m was re-formed -- ifem_ctx::sm_version -- and only at set-up time:
// solver.hip::sm_ensure; never inside sm_apply, which runs inside captured V-cycles):
//   signature  of lattice point i on an axis of n nodes: (min(i, 2), min(n - 1 - i, 2)) (lattice.cpp::lattice_axis_classes: at most 5 per axis,
//              correct for axes shorter than 5 nodes); window: the 5 points from i - 2 per axis, one value each.
//   probe      the new product against the fp64 spmv_sm of the assembled matrix; a re-formed S_m pays it on every level.
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
#include "lattice_stencil.hpp"

namespace ifem {

constexpr int kSmsIrregular = kStencilIrregular;
template <int DIM> struct SmsGeo; // tile (outputs) and LDS box (tile + two-deep halo) of k_sms_apply
template <> struct SmsGeo<3> { static constexpr int TX = 8, TY = 8, TZ = 8, SX = 12, SY = 12, SZ = 12, K = 125; };
template <> struct SmsGeo<2> { static constexpr int TX = 16, TY = 16, TZ = 1, SX = 20, SY = 20, SZ = 1, K = 25; };

template <int D> struct SmsOp { // the operator for lattice_stencil.hpp: a wave per row
  static constexpr int DIM = D, W = 5, NC = 1, NR = 1, G = 64;
  __host__ __device__ static constexpr int first_col(int i) { return i - 2; }
  static int axis_classes(int n, std::vector<uint8_t> &cls, std::vector<int32_t> &first) { return lattice_axis_classes(n, cls, first); }
  static constexpr const char *table_name = "the stencil tables of S_m", *cls_name = "the class ids of the S_m stencil product",
                              *rows_name = "the irregular rows of the S_m stencil product";
};

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
__global__ __launch_bounds__(256) void k_sms_apply(StencilDims d, int tiles_x, int tiles_y, const int32_t *__restrict__ nol, const uint16_t *__restrict__ cls,
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
    const bool in = s < S && gx >= 0 && gx < d.n[0] && gy >= 0 && gy < d.n[1] && gz >= 0 && gz < d.n[2];
    src[k] = in ? nol[gx + d.n[0] * (gy + d.n[1] * gz)] : -1;
  }
#pragma unroll
  for (int k = 0; k < NO; ++k) {
    const int o = tid + 256 * k;
    const int gx = ox + o % G::TX, gy = oy + (o / G::TX) % G::TY, gz = oz + o / (G::TX * G::TY);
    const bool inside = gx < d.n[0] && gy < d.n[1] && gz < d.n[2];
    p_out[k] = inside ? gx + d.n[0] * (gy + d.n[1] * gz) : -1;
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

void sm_stencil_apply(ifem_ctx *ctx, const double *x, double *y) {
  const SmStencil &T = ctx->sm_stencil;
  const PLattice &L = ctx->p_lattice;
  const StencilDims d = stencil_dims(L, L, T);
  const double N = double(ctx->nPo);
  hipStream_t s = ctx->stream;
  if (ctx->dim == 3) {
    using G = SmsGeo<3>;
    const int tx = (d.n[0] + G::TX - 1) / G::TX, ty = (d.n[1] + G::TY - 1) / G::TY, tz = (d.n[2] + G::TZ - 1) / G::TZ;
    // the gather with its halo (index + value per LDS entry), class + index + result per row; the irregular rows as CSR rows
    KScope ks(ctx, IFEM_KC_SPMV_SM, double(tx) * ty * tz * (G::SX * G::SY * G::SZ) * 12.0 + N * 14.0 + double(T.n_irregular) * (G::K * 12.0 + 16.0));
    hipLaunchKernelGGL(k_sms_apply<3>, dim3(unsigned(tx * ty * tz)), dim3(256), 0, s, d, tx, ty, L.node_of_lattice.p, T.cls.p, T.table.p, x, y);
    spmv_sm_rows(ctx, x, y, T.n_irregular, T.rows.p);
  } else {
    using G = SmsGeo<2>;
    const int tx = (d.n[0] + G::TX - 1) / G::TX, ty = (d.n[1] + G::TY - 1) / G::TY;
    KScope ks(ctx, IFEM_KC_SPMV_SM, double(tx) * ty * (G::SX * G::SY) * 12.0 + N * 14.0 + double(T.n_irregular) * (G::K * 12.0 + 16.0));
    hipLaunchKernelGGL(k_sms_apply<2>, dim3(unsigned(tx * ty)), dim3(256), 0, s, d, tx, ty, L.node_of_lattice.p, T.cls.p, T.table.p, x, y);
    spmv_sm_rows(ctx, x, y, T.n_irregular, T.rows.p);
  }
}

// the new product against the fp64 CSR product of the assembled S_m on a pseudo-random vector, formed and compared on the device
static bool sm_stencil_probe(ifem_ctx *ctx, double *rel) {
  const int64_t n = ctx->nPo;
  const size_t un = size_t(n);
  hipStream_t s = ctx->stream;
  DBuf<double> de, d0, d1;
  de.alloc(un); d0.alloc(un); d1.alloc(un);
  vec_rough(ctx, n, 0x5EED, de.p); // a fixed hash of the index: the same probe on every run
  IFEM_HIP_CHECK(hipMemsetAsync(d1.p, 0xff, un * sizeof(double), s)); // NaN: a row nobody produced shows
  spmv_sm(ctx, de.p, d0.p, /*use_f32=*/false);
  sm_stencil_apply(ctx, de.p, d1.p);
  return stencil_probe_compare(ctx, n, d0.p, d1.p, rel); // d1 = stencil - CSR
}

void sm_stencil_setup(ifem_ctx *ctx, int verbose) {
  SmStencil &T = ctx->sm_stencil;
  if (T.off || T.failed || T.version == ctx->sm_version) return;
  T.version = ctx->sm_version;
  T.ready = false;
  if (ctx->halo.nranks > 1 || !ctx->sm_valid || ctx->Sm.n_rows == 0 || ctx->Sm.n_rows != ctx->nPo || !p_lattice_ensure(ctx)) return;
  const PLattice &L = ctx->p_lattice;
  double err = 0;
  const bool few = ctx->dim == 3 ? stencil_build<SmsOp<3>>(ctx, T, L, L, ctx->Sm, nullptr, nullptr) : stencil_build<SmsOp<2>>(ctx, T, L, L, ctx->Sm, nullptr, nullptr);
  const bool ok = few && sm_stencil_probe(ctx, &err);
  if (!stencil_decide(T, few, ok, err, "S_m", ctx->nPo, "level", verbose)) return;
  // the single-precision copy of the values has no reader on this level any more
  ctx->Sm_f32.release();
  ctx->Sm_f32.stale();
  if (verbose) fprintf(stderr, "[ifem] S_m: stencil product on the %d x %d x %d lattice, %d classes, %lld irregular rows, probe %.2e\n", L.n[0], L.n[1], L.n[2], T.classes, (long long)T.n_irregular, err);
}

} // namespace ifem
