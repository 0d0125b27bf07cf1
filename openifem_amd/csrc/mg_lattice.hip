// mg_lattice.hip -- the velocity transfers of the A_uu V-cycle between two uniform box levels without a table (ctx.hpp::MgLatticeU).
// Where both levels hold their Q2 velocity nodes as full lattices (ctx.hpp::ULattice) and every axis of the pair is either kept or halved,
// an entry of P_u or R_u is a function of the two lattice points alone (mg_lattice.hpp): the kernels below form the rows from the lattice
// maps, the weight formula and the Dirichlet flags of the two levels instead of streaming one packed 8-byte entry per weight
// (mg.hip::k_mg_csr_nodes).  One instantiation per set of halved axes: slots, tile and footprint sizes are compile-time constants.  The CSR tables of ifem_mg_attach stay: they are what the formula is checked against, entry by entry, once per
// attach (mg_lattice_u_setup), and the path of every pair that fails the check or is not eligible.
// Semantics are those of k_mg_csr_nodes: y[row][c] = flag_out ? 0 : float(sum_k w_k (flag_in[col_k][c] ? 0 : x[col_k][c])), the sum in double
// in a fixed order (z slots outermost, x slots innermost).
#include <hip/hip_runtime.h>
#include <cstdio>
#include "ctx.hpp"
#include "kernels.hpp"
#include "mg_lattice.hpp"

namespace ifem {

struct MglGeo {
  int nf[3], nc[3]; // lattice points per axis of the fine / coarse level (1 beyond dim)
  int halved[3];    // the pair halves the cells of this axis (nf = 2 nc - 1); 0: nf == nc
  double rnf[2];    // 1 / nf[0], 1 / nf[1]: the prolongation splits a lattice index without an integer division
};

static MglGeo mgl_geo(const MgLatticeU &L) {
  MglGeo g;
  for (int a = 0; a < 3; ++a) { g.nf[a] = L.n_f[a]; g.nc[a] = L.n_c[a]; g.halved[a] = L.halved[a] ? 1 : 0; }
  g.rnf[0] = 1.0 / g.nf[0]; g.rnf[1] = 1.0 / g.nf[1];
  return g;
}

// The kernels read a level through its FLAGGED lattice map (ifem_ctx::mgl_map, k_mgl_flag_map): node | drop bits << 29 per lattice point, bit c
// = component c of that node is a constrained dof of the constrained-dof set in use -- one 4-byte load gives the node and its flags, one
// 4-byte-aligned load of DIM floats its values: two loads per gathered node, where the map entry, DIM components and DIM flag bytes one by
// one are seven (measured at 128^3: 0.68 / 0.65 ms per finest prolongation / restriction that way, 0.18 / 0.19 ms this way; profiles/r16).
// Re-made at set-up when the set of the level changes (as the packed CSR entries are); nodes stay below 2^29 - 1, so ~0 never names one.
constexpr uint32_t kMglNodeMask = 0x1FFFFFFFu;
template <int DIM> struct MglVec { float v[DIM]; };

template <int DIM>
__global__ __launch_bounds__(256) void k_mgl_flag_map(int64_t n, const int32_t *__restrict__ node_of_lat, const uint8_t *__restrict__ flag,
                                                      uint32_t *__restrict__ map) {
  const int64_t p = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t nd = uint32_t(node_of_lat[p]);
  uint32_t bits = 0;
#pragma unroll
  for (int c = 0; c < DIM; ++c) bits |= (flag && flag[int64_t(nd) * DIM + c]) ? (1u << c) : 0u;
  map[p] = nd | (bits << 29);
}

// q = p / n, r = p % n for 0 <= p < 2^31 and n >= 1 from the double reciprocal: the rounded product is off by one at most
__device__ inline void mgl_divmod(int p, int n, double rn, int &q, int &r) {
  q = int(double(p) * rn);
  r = p - q * n;
  if (r < 0) { --q; r += n; }
  else if (r >= n) { ++q; r -= n; }
}

// ---- prolongation: one thread per fine node in node order (coalesced lattice_of_node and output).  HX / HY / HZ: the halved axes, compile-time,
// so that the 3 slots of a halved axis unroll: every slot's coarse node is loaded (an empty slot names a neighbour of the row's, in range, and
// carries weight 0, which selects its product away), all loads of a row in flight together.
template <int DIM, int HX, int HY, int HZ>
__global__ __launch_bounds__(256) void k_mgl_prolong(MglGeo g, int64_t n_fine, const int32_t *__restrict__ lat_of_node_f,
                                                     const uint32_t *__restrict__ map_c, const uint8_t *__restrict__ flag_f,
                                                     const float *__restrict__ x, float *__restrict__ y) {
  const int64_t node = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (node >= n_fine) return;
  constexpr int SX = HX ? kMglProlongSlots : 1, SY = HY ? kMglProlongSlots : 1, SZ = HZ ? kMglProlongSlots : 1;
  int ix, iy, iz, q;
  mgl_divmod(lat_of_node_f[node], g.nf[0], g.rnf[0], q, ix);
  mgl_divmod(q, g.nf[1], g.rnf[1], iz, iy);
  int jx[SX], jy[SY];
  double wx[SX], wy[SY];
#pragma unroll
  for (int k = 0; k < SX; ++k) if (!mgl_prolong_term(HX != 0, g.nc[0], ix, k, jx[k], wx[k])) wx[k] = 0.0;
#pragma unroll
  for (int k = 0; k < SY; ++k) if (!mgl_prolong_term(HY != 0, g.nc[1], iy, k, jy[k], wy[k])) wy[k] = 0.0;
  double s[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) s[c] = 0;
  // rows of up to 9 slots load everything at once; the 27 slots of three halved axes go plane by plane (registers)
  constexpr int UZ = SX * SY * SZ <= 9 ? SZ : 1;
#pragma unroll UZ
  for (int kz = 0; kz < SZ; ++kz) {
    int jz; double wz;
    if (!mgl_prolong_term(HZ != 0, g.nc[2], iz, kz, jz, wz)) wz = 0.0;
    uint32_t m[SY * SX];
#pragma unroll
    for (int ky = 0; ky < SY; ++ky)
#pragma unroll
      for (int kx = 0; kx < SX; ++kx) m[ky * SX + kx] = map_c[jx[kx] + g.nc[0] * (jy[ky] + g.nc[1] * jz)];
    MglVec<DIM> v[SY * SX];
#pragma unroll
    for (int t = 0; t < SY * SX; ++t) v[t] = *reinterpret_cast<const MglVec<DIM> *>(x + int64_t(m[t] & kMglNodeMask) * DIM);
#pragma unroll
    for (int ky = 0; ky < SY; ++ky)
#pragma unroll
      for (int kx = 0; kx < SX; ++kx) {
        const int t = ky * SX + kx;
        const double w = wz * wy[ky] * wx[kx];
#pragma unroll
        for (int c = 0; c < DIM; ++c) s[c] += (w != 0.0 && !((m[t] >> (29 + c)) & 1u)) ? w * double(v[t].v[c]) : 0.0;
      }
  }
  MglVec<DIM> out;
#pragma unroll
  for (int c = 0; c < DIM; ++c) out.v[c] = (flag_f && flag_f[node * DIM + c]) ? 0.0f : float(s[c]);
  *reinterpret_cast<MglVec<DIM> *>(y + node * DIM) = out;
}

// ---- restriction: a row holds up to 5 fine points per halved axis.  A block takes a tile of T coarse lattice points per axis, stages the
// tile's fine footprint (2T + 5 points on a halved axis, T on a kept one) through the fine map into LDS -- floats with the fine flags already
// applied, zeros outside the lattice -- sums from LDS and writes through the coarse map.
// Tile: 4 coarse points on every axis, 16 on the first kept axis (the flagship's x); with no kept axis 8 on x.  Footprints in 3D: 16 x 13 x 13
// = 2704 and 21 x 13 x 13 = 3549 points of 12 bytes: 32.4 and 42.6 KB of the CU's 160 KB (4 and 3 blocks per CU), 256 and 128 rows per block.
template <int DIM, int HX, int HY, int HZ>
struct MglTile {
  static constexpr int kWide = !HX ? 0 : ((DIM > 1 && !HY) ? 1 : ((DIM > 2 && !HZ) ? 2 : -1));
  static constexpr int t(int a) { return a >= DIM ? 1 : (a == kWide ? 16 : ((kWide < 0 && a == 0) ? 8 : 4)); }
  static constexpr int T0 = t(0), T1 = t(1), T2 = t(2);
  static constexpr int F0 = HX ? 2 * T0 + 5 : T0, F1 = HY ? 2 * T1 + 5 : T1, F2 = HZ ? 2 * T2 + 5 : T2;
  static constexpr int NF = F0 * F1 * F2, NT = T0 * T1 * T2;
};

template <int DIM, int HX, int HY, int HZ>
__global__ __launch_bounds__(256) void k_mgl_restrict(MglGeo g, int ntx, int nty, const uint32_t *__restrict__ map_f,
                                                      const uint32_t *__restrict__ map_c, const float *__restrict__ r, float *__restrict__ y) {
  using TL = MglTile<DIM, HX, HY, HZ>;
  __shared__ float sh[TL::NF * DIM]; // [F2][F1][F0][DIM]
  int b = blockIdx.x;
  const int j0x = (b % ntx) * TL::T0;
  b /= ntx;
  const int j0y = (b % nty) * TL::T1, j0z = (b / nty) * TL::T2;
  const int bx = HX ? 2 * j0x - 3 : j0x, by = HY ? 2 * j0y - 3 : j0y, bz = HZ ? 2 * j0z - 3 : j0z; // first fine point of the footprint
  constexpr int IT = (TL::NF + 255) / 256, BT = IT < 6 ? IT : 6; // footprint points per thread, staged BT at a time (registers)
  for (int i0 = 0; i0 < IT; i0 += BT) {
    uint32_t m[BT];
#pragma unroll
    for (int i = 0; i < BT; ++i) { // every load at a point inside the lattice (clamped); what lies outside is selected away below
      const int f = min(int(threadIdx.x) + 256 * (i0 + i), TL::NF - 1);
      const int gx = min(max(bx + f % TL::F0, 0), g.nf[0] - 1), gy = min(max(by + (f / TL::F0) % TL::F1, 0), g.nf[1] - 1),
                gz = min(max(bz + f / (TL::F0 * TL::F1), 0), g.nf[2] - 1);
      m[i] = map_f[gx + g.nf[0] * (gy + g.nf[1] * gz)];
    }
    MglVec<DIM> v[BT];
#pragma unroll
    for (int i = 0; i < BT; ++i) v[i] = *reinterpret_cast<const MglVec<DIM> *>(r + int64_t(m[i] & kMglNodeMask) * DIM);
#pragma unroll
    for (int i = 0; i < BT; ++i) {
      const int f = int(threadIdx.x) + 256 * (i0 + i);
      const int gx = bx + f % TL::F0, gy = by + (f / TL::F0) % TL::F1, gz = bz + f / (TL::F0 * TL::F1);
      const bool inside = gx >= 0 && gx < g.nf[0] && gy >= 0 && gy < g.nf[1] && gz >= 0 && gz < g.nf[2];
      if (f < TL::NF) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) sh[f * DIM + c] = (inside && !((m[i] >> (29 + c)) & 1u)) ? v[i].v[c] : 0.0f;
      }
    }
  }
  __syncthreads();
  constexpr int SX = HX ? kMglRestrictSlots : 1, SY = HY ? kMglRestrictSlots : 1, SZ = HZ ? kMglRestrictSlots : 1;
  for (int t = threadIdx.x; t < TL::NT; t += 256) {
    const int jx = j0x + t % TL::T0, jy = j0y + (t / TL::T0) % TL::T1, jz = j0z + t / (TL::T0 * TL::T1);
    if (jx >= g.nc[0] || jy >= g.nc[1] || jz >= g.nc[2]) continue;
    // per axis the local index of every slot inside the footprint (an empty slot: clamped, weight 0)
    int lx[SX], ly[SY];
    double wx[SX], wy[SY];
#pragma unroll
    for (int k = 0; k < SX; ++k) { int i; if (!mgl_restrict_term(HX != 0, g.nf[0], jx, k, i, wx[k])) wx[k] = 0.0; lx[k] = min(max(i - bx, 0), TL::F0 - 1); }
#pragma unroll
    for (int k = 0; k < SY; ++k) { int i; if (!mgl_restrict_term(HY != 0, g.nf[1], jy, k, i, wy[k])) wy[k] = 0.0; ly[k] = min(max(i - by, 0), TL::F1 - 1); }
    double s[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) s[c] = 0;
    constexpr int UZ = SX * SY * SZ <= 5 ? SZ : 1; // (rows of 25 and 125 slots go plane by plane: registers)
#pragma unroll UZ
    for (int kz = 0; kz < SZ; ++kz) {
      int iz; double wz;
      if (!mgl_restrict_term(HZ != 0, g.nf[2], jz, kz, iz, wz)) wz = 0.0;
      const int lz = min(max(iz - bz, 0), TL::F2 - 1);
#pragma unroll
      for (int ky = 0; ky < SY; ++ky) {
        const int row = TL::F0 * (ly[ky] + TL::F1 * lz);
        const double wzy = wz * wy[ky];
#pragma unroll
        for (int kx = 0; kx < SX; ++kx) {
          const float *pv = sh + (row + lx[kx]) * DIM;
          const double w = wzy * wx[kx];
#pragma unroll
          for (int c = 0; c < DIM; ++c) s[c] += w != 0.0 ? w * double(pv[c]) : 0.0;
        }
      }
    }
    const uint32_t mc = map_c[jx + g.nc[0] * (jy + g.nc[1] * jz)];
    MglVec<DIM> out;
#pragma unroll
    for (int c = 0; c < DIM; ++c) out.v[c] = ((mc >> (29 + c)) & 1u) ? 0.0f : float(s[c]);
    *reinterpret_cast<MglVec<DIM> *>(y + int64_t(mc & kMglNodeMask) * DIM) = out;
  }
}

// ---- the checks of a pair, once per attach.  counters: [0] rows of P_u, [1] rows of R_u whose entries are not exactly the formula's (another
// length, a column that is not the node at the formula's point, or a weight that differs), [2] coarse nodes whose injection partner is not
// the fine node at the coinciding point
template <bool PROLONG>
__global__ __launch_bounds__(256) void k_mgl_check(MglGeo g, int64_t n_rows, const int32_t *__restrict__ lat_of_row,
                                                   const int32_t *__restrict__ node_of_lat_col, const int64_t *__restrict__ ptr,
                                                   const int32_t *__restrict__ col, const double *__restrict__ w,
                                                   unsigned long long *__restrict__ bad) {
  const int64_t row = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (row >= n_rows) return;
  const int *nr = PROLONG ? g.nf : g.nc, *ncl = PROLONG ? g.nc : g.nf; // lattices of the rows / of the columns
  int p = lat_of_row[row];
  int i[3];
  i[0] = p % nr[0];
  p /= nr[0];
  i[1] = p % nr[1];
  i[2] = p / nr[1];
  const int64_t k0 = ptr[row], k1 = ptr[row + 1];
  int64_t terms = 0;
  bool ok = true;
  int s[3];
  for (int a = 0; a < 3; ++a) s[a] = PROLONG ? mgl_prolong_slots(g.halved[a]) : mgl_restrict_slots(g.halved[a]);
  for (int kz = 0; kz < s[2]; ++kz)
    for (int ky = 0; ky < s[1]; ++ky)
      for (int kx = 0; kx < s[0]; ++kx) {
        const int k[3] = {kx, ky, kz};
        int j[3];
        double wt = 1.0;
        bool term = true;
        for (int a = 0; a < 3; ++a) {
          double wa;
          const bool ta = PROLONG ? mgl_prolong_term(g.halved[a], g.nc[a], i[a], k[a], j[a], wa) : mgl_restrict_term(g.halved[a], g.nf[a], i[a], k[a], j[a], wa);
          term = term && ta;
          wt *= wa;
        }
        if (!term) continue;
        ++terms;
        const int32_t want = node_of_lat_col[j[0] + ncl[0] * (j[1] + ncl[1] * j[2])];
        bool found = false;
        for (int64_t e = k0; e < k1; ++e) found = found || (col[e] == want && w[e] == wt);
        ok = ok && found;
      }
  // the formula's columns are distinct nodes: as many entries as terms, every term found -> the row is the formula's
  if (!ok || terms != k1 - k0) atomicAdd(bad, 1ull);
}

__global__ __launch_bounds__(256) void k_mgl_check_inject(MglGeo g, int64_t n_coarse, const int32_t *__restrict__ lat_of_node_c,
                                                          const int32_t *__restrict__ node_of_lat_f, const int32_t *__restrict__ inj,
                                                          unsigned long long *__restrict__ bad) {
  const int64_t cn = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (cn >= n_coarse) return;
  int p = lat_of_node_c[cn];
  const int jx = p % g.nc[0];
  p /= g.nc[0];
  const int jy = p % g.nc[1], jz = p / g.nc[1];
  const int fx = mgl_inject_index(g.halved[0], jx), fy = mgl_inject_index(g.halved[1], jy), fz = mgl_inject_index(g.halved[2], jz);
  if (node_of_lat_f[fx + g.nf[0] * (fy + g.nf[1] * fz)] != inj[cn]) atomicAdd(bad, 1ull);
}

static inline unsigned blocks_for(int64_t n) { return unsigned((n + 255) / 256); }

// Decide the pair (c, c->mg_coarse) once per ifem_mg_attach: set-up time only (allocates, synchronises), from solver.hip::mg_uu_setup
void mg_lattice_u_setup(ifem_ctx *c, int verbose) {
  MgLatticeU &L = c->mg_lattice_u;
  if (L.state != 0) return;
  L.state = -1;
  L.bad_p = L.bad_r = L.bad_inj = -1;
  ifem_ctx *cc = c->mg_coarse;
  const char *why = nullptr;
  if (!cc) why = "no coarser level";
  else if (c->halo.nranks > 1 || cc->halo.nranks > 1 || c->mg_replica) why = "a partitioned or replicated level";
  else if (c->hang.active || c->hang.n > 0 || cc->hang.active || cc->hang.n > 0) why = "hanging-node lines";
  else if (c->kv != 2 || cc->kv != 2 || c->dim != cc->dim) why = "not Q2 velocity on both levels";
  else if (c->mg_Pu.n_rows != c->nUo || c->mg_Ru.n_rows != cc->nUl || c->nUo <= 0 || cc->nUl != cc->nUo || c->mg_inj_u.n != size_t(cc->nUo)) why = "no complete velocity tables";
  else if (!u_lattice_ensure(c) || !u_lattice_ensure(cc)) why = "a level is no full uniform lattice";
  else if (c->nUl >= int64_t(kMglNodeMask) || cc->nUl >= int64_t(kMglNodeMask)) why = "flagged map entries hold 29 node bits";
  if (!why) {
    for (int a = 0; a < 3; ++a) {
      const int nf = a < c->dim ? c->u_lattice.n[a] : 1, nc = a < c->dim ? cc->u_lattice.n[a] : 1;
      L.n_f[a] = nf; L.n_c[a] = nc;
      L.halved[a] = nf != nc;
      if (nf != nc && nf != 2 * nc - 1) why = "an axis is neither kept nor halved";
    }
  }
  if (!why) {
    hipStream_t s = c->stream;
    const MglGeo g = mgl_geo(L);
    DBuf<unsigned long long> bad;
    bad.alloc(3);
    IFEM_HIP_CHECK(hipMemsetAsync(bad.p, 0, 3 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_mgl_check<true>, dim3(blocks_for(c->nUo)), dim3(256), 0, s, g, c->nUo, c->u_lattice.lattice_of_node.p,
                       cc->u_lattice.node_of_lattice.p, c->mg_Pu.ptr.p, c->mg_Pu.col.p, c->mg_Pu.w.p, bad.p);
    hipLaunchKernelGGL(k_mgl_check<false>, dim3(blocks_for(cc->nUl)), dim3(256), 0, s, g, cc->nUl, cc->u_lattice.lattice_of_node.p,
                       c->u_lattice.node_of_lattice.p, c->mg_Ru.ptr.p, c->mg_Ru.col.p, c->mg_Ru.w.p, bad.p + 1);
    hipLaunchKernelGGL(k_mgl_check_inject, dim3(blocks_for(cc->nUo)), dim3(256), 0, s, g, cc->nUo, cc->u_lattice.lattice_of_node.p,
                       c->u_lattice.node_of_lattice.p, c->mg_inj_u.p, bad.p + 2);
    unsigned long long h[3] = {1, 1, 1};
    IFEM_HIP_CHECK(hipMemcpyAsync(h, bad.p, sizeof(h), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s)); // (`bad` leaves scope)
    IFEM_HIP_CHECK(hipGetLastError());
    L.bad_p = int64_t(h[0]); L.bad_r = int64_t(h[1]); L.bad_inj = int64_t(h[2]);
    if (h[2]) why = "the injection map is not the lattices'";
    else if (h[0] || h[1]) why = "table rows differ from the lattice formula";
  }
  if (!why) L.state = 1;
  if (verbose) {
    if (why) fprintf(stderr, "[ifem] A_uu V-cycle level of %lld cells: velocity transfers keep CSR (%s; rows off the formula: P %lld, R %lld)\n",
                     (long long)c->n_cells, why, (long long)L.bad_p, (long long)L.bad_r);
    else fprintf(stderr, "[ifem] A_uu V-cycle level of %lld cells: velocity transfers from the lattice formula (%d x %d x %d -> %d x %d x %d points)\n",
                 (long long)c->n_cells, L.n_f[0], L.n_f[1], L.n_f[2], L.n_c[0], L.n_c[1], L.n_c[2]);
  }
}

static const uint8_t *level_flags(const ifem_ctx *c, int cs) { return c->has_c[cs] ? c->is_c[cs].p : nullptr; }

// the flagged lattice map of a level for its constrained-dof set cs (set-up time: allocates), re-made when the set changes
static void mgl_flag_map_ensure(ifem_ctx *c, int cs) {
  const int64_t key = 2 * c->flag_id[cs] + (c->has_c[cs] ? 1 : 0);
  const size_t n = c->u_lattice.node_of_lattice.n;
  if (c->mgl_map.n == n && c->mgl_map_key == key) return;
  if (c->mgl_map.n != n) c->mgl_map.alloc(n);
  KScope ks(c, IFEM_KC_MG_TRANSFER, double(n) * (8.0 + c->dim));
  const dim3 grid(blocks_for(int64_t(n))), block(256);
  if (c->dim == 3) hipLaunchKernelGGL((k_mgl_flag_map<3>), grid, block, 0, c->stream, int64_t(n), c->u_lattice.node_of_lattice.p, level_flags(c, cs), c->mgl_map.p);
  else hipLaunchKernelGGL((k_mgl_flag_map<2>), grid, block, 0, c->stream, int64_t(n), c->u_lattice.node_of_lattice.p, level_flags(c, cs), c->mgl_map.p);
  c->mgl_map_key = key;
}

// the instantiation of the pair's halved axes
#define IFEM_MGL_PATTERN(K, DIM, ...)                                                                      \
  switch (g.halved[0] | (g.halved[1] << 1) | (g.halved[2] << 2)) {                                         \
    case 0: hipLaunchKernelGGL((K<DIM, 0, 0, 0>), __VA_ARGS__); break;                                     \
    case 1: hipLaunchKernelGGL((K<DIM, 1, 0, 0>), __VA_ARGS__); break;                                     \
    case 2: hipLaunchKernelGGL((K<DIM, 0, 1, 0>), __VA_ARGS__); break;                                     \
    case 3: hipLaunchKernelGGL((K<DIM, 1, 1, 0>), __VA_ARGS__); break;                                     \
    case 4: hipLaunchKernelGGL((K<DIM, 0, 0, DIM == 3>), __VA_ARGS__); break;                              \
    case 5: hipLaunchKernelGGL((K<DIM, 1, 0, DIM == 3>), __VA_ARGS__); break;                              \
    case 6: hipLaunchKernelGGL((K<DIM, 0, 1, DIM == 3>), __VA_ARGS__); break;                              \
    default: hipLaunchKernelGGL((K<DIM, 1, 1, DIM == 3>), __VA_ARGS__); break;                             \
  }

// coarse -> fine: y [dim nUo of c] from x [dim nUl of the coarse level]
static void mg_lattice_prolong(ifem_ctx *c, const float *x, float *y) {
  ifem_ctx *cc = c->mg_coarse;
  const int dim = c->dim;
  // per fine node its lattice point, flag bytes and outputs; per coarse node its flagged map entry and values (re-used from cache)
  KScope ks(c, IFEM_KC_MG_TRANSFER, double(c->nUo) * (4.0 + dim * 5.0) + double(cc->nUo) * (4.0 + dim * 4.0));
  const MglGeo g = mgl_geo(c->mg_lattice_u);
  const dim3 grid(blocks_for(c->nUo)), block(256);
  const uint8_t *ff = level_flags(c, c->asm_constraint_set);
  if (dim == 3) { IFEM_MGL_PATTERN(k_mgl_prolong, 3, grid, block, 0, c->stream, g, c->nUo, c->u_lattice.lattice_of_node.p, cc->mgl_map.p, ff, x, y) }
  else { IFEM_MGL_PATTERN(k_mgl_prolong, 2, grid, block, 0, c->stream, g, c->nUo, c->u_lattice.lattice_of_node.p, cc->mgl_map.p, ff, x, y) }
}

template <int DIM, int HX, int HY, int HZ>
static void launch_restrict(ifem_ctx *c, const MglGeo &g, const float *r, float *y) {
  using TL = MglTile<DIM, HX, HY, HZ>;
  const int ntx = (g.nc[0] + TL::T0 - 1) / TL::T0, nty = (g.nc[1] + TL::T1 - 1) / TL::T1, ntz = (g.nc[2] + TL::T2 - 1) / TL::T2;
  hipLaunchKernelGGL((k_mgl_restrict<DIM, HX, HY, HZ>), dim3(unsigned(ntx) * unsigned(nty) * unsigned(ntz)), dim3(256), 0, c->stream, g, ntx, nty,
                     c->mgl_map.p, c->mg_coarse->mgl_map.p, r, y);
}

// fine -> coarse: y [dim nUl of the coarse level] from r [dim nUo of c]
static void mg_lattice_restrict(ifem_ctx *c, const float *r, float *y) {
  ifem_ctx *cc = c->mg_coarse;
  const int dim = c->dim;
  // per fine node its flagged map entry and values (the tile seams re-read from cache); per coarse node its flagged map entry and outputs
  KScope ks(c, IFEM_KC_MG_TRANSFER, double(c->nUo) * (4.0 + dim * 4.0) + double(cc->nUo) * (4.0 + dim * 4.0));
  const MglGeo g = mgl_geo(c->mg_lattice_u);
  const int pat = g.halved[0] | (g.halved[1] << 1) | (g.halved[2] << 2);
#define IFEM_MGL_R(DIM, HX, HY, HZ) launch_restrict<DIM, HX, HY, HZ>(c, g, r, y)
  if (dim == 3) {
    switch (pat) {
      case 0: IFEM_MGL_R(3, 0, 0, 0); break; case 1: IFEM_MGL_R(3, 1, 0, 0); break; case 2: IFEM_MGL_R(3, 0, 1, 0); break; case 3: IFEM_MGL_R(3, 1, 1, 0); break;
      case 4: IFEM_MGL_R(3, 0, 0, 1); break; case 5: IFEM_MGL_R(3, 1, 0, 1); break; case 6: IFEM_MGL_R(3, 0, 1, 1); break; default: IFEM_MGL_R(3, 1, 1, 1); break;
    }
  } else {
    switch (pat & 3) {
      case 0: IFEM_MGL_R(2, 0, 0, 0); break; case 1: IFEM_MGL_R(2, 1, 0, 0); break; case 2: IFEM_MGL_R(2, 0, 1, 0); break; default: IFEM_MGL_R(2, 1, 1, 0); break;
    }
  }
#undef IFEM_MGL_R
}

// One velocity transfer of the pair (c, c->mg_coarse) as the cycle launches it: the lattice kernels where the pair passed its checks and
// ifem_tuning::mg_lattice_u is on, the CSR kernels elsewhere (csr_only: the CSR kernels whatever the pair is)
void mg_transfer_u(ifem_ctx *c, bool prolong, const float *x, float *y, bool csr_only) {
  if (csr_only || !mg_lattice_u_active(c)) {
    if (prolong) mg_csr_apply_nodes_f32(c, c->mg_Pu, x, c->mg_Pu_mask, y);
    else mg_csr_apply_nodes_f32(c, c->mg_Ru, x, c->mg_Ru_mask, y);
  } else if (prolong) mg_lattice_prolong(c, x, y);
  else mg_lattice_restrict(c, x, y);
}

// What both paths of the pair (c, c->mg_coarse) need before a cycle, at set-up time: the packed CSR entries with the drop bits of the constrained-dof
// set `cs` of the two levels (functions of the two sets: re-made when either changes), the decision about the lattice path, and its flagged maps
void mg_transfer_u_setup(ifem_ctx *c, int cs, int verbose) {
  ifem_ctx *cc = c->mg_coarse;
  const int64_t key[2] = {c->flag_id[cs], cc->flag_id[cs]};
  if (c->mg_Pu_mask.n != c->mg_Pu.col.n * 8 || c->mg_mask_key[0] != key[0] || c->mg_mask_key[1] != key[1]) {
    const uint8_t *ff = c->has_c[cs] ? c->is_c[cs].p : nullptr, *fc = cc->has_c[cs] ? cc->is_c[cs].p : nullptr;
    mg_csr_mask(c, c->mg_Ru, ff, fc, c->mg_Ru_mask); // rows: local coarse nodes, columns: owned fine nodes
    mg_csr_mask(c, c->mg_Pu, fc, ff, c->mg_Pu_mask); // rows: owned fine nodes, columns: local coarse nodes
    c->mg_mask_key[0] = key[0]; c->mg_mask_key[1] = key[1];
  }
  mg_lattice_u_setup(c, verbose);
  if (c->mg_lattice_u.state == 1) { // the flagged lattice maps of the two levels, for the same set
    mgl_flag_map_ensure(c, cs);
    mgl_flag_map_ensure(cc, cs);
  }
}

} // namespace ifem
