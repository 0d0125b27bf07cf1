// patch.hip -- vertex-patch smoother of the A_uu V-cycle (ifem_tuning::uu_smoother = 1): the shared-type form of uniform box levels, and
// (at the end of this file, ifem_tuning::uu_patch_levels = 1) the general form with one inverse per patch for every other level.
//
// The patch of mesh vertex v holds every Q2 velocity node n such that each cell containing n also contains v: on a box the lattice box
// of +-1 node around v, clipped at the domain (27 nodes in 3D, 9 in 2D; 18 / 12 / 8 on a face / edge / corner).  With A0 = mu K +
// (rho/dt) M + gamma rho GradDiv under the constraint rule of the assembly (a constrained dof is a decoupled 1 x 1 row, its column
// zero) and A_v = R_v A0 R_v^T, the smoother is the unweighted additive sum  B r = sum_v R_v^T A_v^-1 R_v r.  Convection is not part of
// A0; it stays in the residual the Chebyshev iteration works on.
//
// Setup (host, fp64, once per (mu, rho, gamma, dt, h, constrained-dof set)): the level is one axis-aligned cell repeated, so A_v
// depends only on which nodes of the patch exist and which of its dofs are constrained.  Patches are grouped into types by that
// signature (the 3D channel has a few dozen); every type's A_v is the sum of the box-cell matrix over its present cells, inverted by LU
// with partial pivoting and stored as float [N][N], N = dim 3^dim (26 kB in 3D).  A0 is symmetric, so is the inverse: the stored table
// is the symmetric part of the computed one, and the kernel may read it by row or by column.
//
// Kernel: d <- a d + b B r on single-precision level vectors, one launch per colour (parity of the vertex lattice index per axis: 8
// colours in 3D, 4 in 2D).  Patches of one colour share no node, so results go out with plain stores in a fixed order: no atomics, a
// deterministic sum.  The term a d is applied by the first colour that touches a node (the one whose vertex index is even along every
// axis in which the node lies between two vertices).  A workgroup of 256 threads takes a run of patches of one type: the inverse goes
// into LDS once, then per tile of 64 patches the N residual entries of each patch are gathered into LDS and the N x N by N x 64 product
// is formed.
//
// Arithmetic: plain FMAs, not MFMA.  gfx950's f32-input MFMA runs at the FP32 vector rate, so the choice is one of LDS traffic: a thread
// owns 12 rows x 2 patches (3D; 4 x 2 in 2D) and reads per column of the inverse three 16-byte broadcast words and two residual words
// for 24 FMAs -- 56 LDS bytes per 24 FMAs, which keeps the LDS pipe and the vector pipe about level.  The v_mfma_f32_16x16x4_f32 tiling
// would need the same operand bytes from LDS per flop (its A and B fragments are not reused across instructions at these sizes) plus
// padding of N = 81 to 96 in both directions.  Padding: rows 81..95 of the LDS copy are zero-filled (never neighbours' data), patches
// past the end of a tile and clipped nodes read r as 0 and store nothing.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>
#include "assemble_common.hpp"
#include "ctx.hpp"
#include "kernels.hpp"

namespace ifem {

constexpr int kPatchTile = 64;   // patches per tile of the product
constexpr int kPatchChunk = 128; // most patches per work item (workgroup)
constexpr int kPatchMaxTypes = 512;

template <int DIM>
struct PatchDims {
  static constexpr int NN = DIM == 3 ? 27 : 9; // nodes of a patch
  static constexpr int N = DIM * NN;           // dofs of a patch
  static constexpr int RI = DIM == 3 ? 12 : 4; // rows per thread (whole nodes: a multiple of DIM)
  static constexpr int NP = 8 * RI;            // rows of the LDS copy (8 row groups), >= N
  static constexpr int RS = kPatchTile + 1;    // row stride of the residual tile (odd: the gather's stores spread over the banks)
};

template <int DIM>
__global__ __launch_bounds__(256) void k_patch_apply(const int32_t *__restrict__ tab, const float *__restrict__ inv,
                                                     const int32_t *__restrict__ work, int colour, float a, float b,
                                                     const float *__restrict__ r, float *__restrict__ d) {
  using P = PatchDims<DIM>;
  constexpr int NN = P::NN, N = P::N, RI = P::RI, NP = P::NP, RS = P::RS;
  __shared__ float sInv[N * NP];            // [column j][row i], rows >= N zero
  __shared__ float sR[N * RS];              // [dof j][patch of the tile]
  __shared__ int32_t sNode[kPatchTile * NN]; // [patch of the tile][node of the patch]
  const int t = threadIdx.x;
  const int type = work[3 * blockIdx.x], p0 = work[3 * blockIdx.x + 1], cnt = work[3 * blockIdx.x + 2];
  const float *g = inv + size_t(type) * N * N;
  for (int e = t; e < N * NP; e += 256) {
    const int j = e / NP, i = e - j * NP;
    sInv[e] = i < N ? g[j * N + i] : 0.0f; // (symmetric table: column j read as row j)
  }
  const int pl = t & 31, ig = t >> 5;
  for (int tile0 = 0; tile0 < cnt; tile0 += kPatchTile) {
    const int np = min(kPatchTile, cnt - tile0);
    __syncthreads(); // the previous tile's readers are done
    for (int e = t; e < kPatchTile * NN; e += 256) {
      const int p = e / NN, nl = e - p * NN;
      const int32_t node = p < np ? tab[int64_t(p0 + tile0 + p) * NN + nl] : -1;
      sNode[e] = node;
#pragma unroll
      for (int c = 0; c < DIM; ++c) sR[(nl * DIM + c) * RS + p] = node >= 0 ? r[int64_t(node) * DIM + c] : 0.0f;
    }
    __syncthreads();
    float acc0[RI], acc1[RI];
#pragma unroll
    for (int k = 0; k < RI; ++k) { acc0[k] = 0.0f; acc1[k] = 0.0f; }
#pragma unroll 3
    for (int j = 0; j < N; ++j) {
      const float r0 = sR[j * RS + pl], r1 = sR[j * RS + pl + 32];
      const float *iv = &sInv[j * NP + ig * RI];
#pragma unroll
      for (int k = 0; k < RI; ++k) {
        const float v = iv[k];
        acc0[k] = fmaf(v, r0, acc0[k]);
        acc1[k] = fmaf(v, r1, acc1[k]);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int p = pl + 32 * h;
      if (p >= np) continue;
#pragma unroll
      for (int m = 0; m < RI / DIM; ++m) {
        const int nl = ig * (RI / DIM) + m;
        if (nl >= NN) continue;
        const int32_t node = sNode[p * NN + nl];
        if (node < 0) continue;
        // the first colour to touch this node: even vertex index along every axis in which the node sits between two vertices
        bool first = true;
        int q = nl;
#pragma unroll
        for (int ax = 0; ax < DIM; ++ax) {
          const int o = q % 3;
          q /= 3;
          first = first && (o == 1 || !((colour >> ax) & 1));
        }
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
          const int64_t idx = int64_t(node) * DIM + c;
          float v = b * (h == 0 ? acc0[m * DIM + c] : acc1[m * DIM + c]);
          if (!first) v += d[idx];
          else if (a != 0.0f) v += a * d[idx]; // a = 0: d holds nothing yet and is not read
          d[idx] = v;
        }
      }
    }
  }
}

// what every form needs: Q2 velocity on one rank without hanging-node lines
static bool patch_level_ok(const ifem_ctx *c) {
  return c->kv == 2 && c->halo.nranks == 1 && !c->hang.active && c->hang.n == 0 && c->n_cells > 0 && c->nUl == c->nUo;
}
// the form of the tables a level takes: 0 shared types (a uniform box level), 1 one inverse per patch (ifem_tuning::uu_patch_levels = 1), -1 none
static int patch_form(const ifem_ctx *c) {
  if (!patch_level_ok(c)) return -1;
  if (mf_takes_uniform(c)) return 0;
  return c->tune.uu_patch_levels == 1 && c->patch.gen_state >= 0 ? 1 : -1;
}
bool patch_eligible(const ifem_ctx *c) { return patch_form(c) >= 0; }

// dense inverse by LU with partial pivoting (fp64, n <= 81); false: singular
static bool invert_dense(int n, std::vector<double> &A, std::vector<double> &Ai) {
  Ai.assign(size_t(n) * n, 0.0);
  for (int i = 0; i < n; ++i) Ai[size_t(i) * n + i] = 1.0;
  for (int k = 0; k < n; ++k) {
    int piv = k;
    for (int i = k + 1; i < n; ++i)
      if (std::fabs(A[size_t(i) * n + k]) > std::fabs(A[size_t(piv) * n + k])) piv = i;
    if (!(std::fabs(A[size_t(piv) * n + k]) > 0)) return false;
    if (piv != k)
      for (int j = 0; j < n; ++j) { std::swap(A[size_t(k) * n + j], A[size_t(piv) * n + j]); std::swap(Ai[size_t(k) * n + j], Ai[size_t(piv) * n + j]); }
    const double ip = 1.0 / A[size_t(k) * n + k];
    for (int j = 0; j < n; ++j) { A[size_t(k) * n + j] *= ip; Ai[size_t(k) * n + j] *= ip; }
    for (int i = 0; i < n; ++i) {
      if (i == k) continue;
      const double f = A[size_t(i) * n + k];
      if (f == 0.0) continue;
      for (int j = 0; j < n; ++j) { A[size_t(i) * n + j] -= f * A[size_t(k) * n + j]; Ai[size_t(i) * n + j] -= f * Ai[size_t(k) * n + j]; }
    }
  }
  return true;
}

// the tables of one level, built on the host from its cell tables (cu [nc][nu] velocity nodes, cp [nc][np] vertices, vc [nc][np][dim]
// vertex coordinates, isc [nU][dim] constrained flags or empty).  false: more than kPatchMaxTypes patch types
struct PatchTables {
  std::vector<int32_t> tab, work;
  std::vector<float> inv;
  int work_ptr[9];
  int n_types = 0;
};
static bool patch_build(int dim, int64_t nc, int64_t nV, int64_t nU, const std::vector<int32_t> &cu, const std::vector<int32_t> &cp,
                        const std::vector<double> &vc, const std::vector<uint8_t> &isc, const double *h, const ifem_ins_params &Pm,
                        const FeTables &fe, PatchTables &T) {
  const int nu = dim == 3 ? 27 : 9, np = 1 << dim, NN = nu, N = dim * NN;
  // 1. lattice index of every cell (from its lowest corner and mf_h), patch -> node table, colour of every vertex
  double org[3] = {0, 0, 0};
  std::vector<double> lo(size_t(nc) * dim);
  for (int64_t c = 0; c < nc; ++c)
    for (int e = 0; e < dim; ++e) {
      double m = vc[(c * np) * dim + e];
      for (int b = 1; b < np; ++b) m = std::min(m, vc[(c * np + b) * dim + e]);
      lo[c * dim + e] = m;
      if (c == 0 || m < org[e]) org[e] = m;
    }
  std::vector<int32_t> tab(size_t(nV) * NN, -1);
  std::vector<int8_t> colour(size_t(nV), -1);
  for (int64_t c = 0; c < nc; ++c) {
    int64_t ci[3] = {0, 0, 0};
    for (int e = 0; e < dim; ++e) ci[e] = std::llround((lo[c * dim + e] - org[e]) / h[e]);
    for (int b = 0; b < np; ++b) {
      const int32_t v = cp[c * np + b];
      if (v < 0 || v >= nV) throw Error(IFEM_E_BADPARAM, "vertex-patch smoother: vertex id outside the level");
      int ib[3] = {b & 1, (b >> 1) & 1, (b >> 2) & 1}, col = 0;
      for (int e = 0; e < dim; ++e) col |= int((ci[e] + ib[e]) & 1) << e;
      colour[v] = int8_t(col);
      for (int a = 0; a < nu; ++a) {
        int ia[3] = {a % 3, (a / 3) % 3, a / 9}, slot = 0, mul = 1;
        bool in = true;
        for (int e = 0; e < dim; ++e) {
          const int o = ia[e] - 2 * ib[e]; // offset of the node from the vertex, in node spacings
          in = in && o >= -1 && o <= 1;
          slot += (o + 1) * mul;
          mul *= 3;
        }
        if (!in) continue;
        const int32_t node = cu[c * nu + a];
        if (node < 0 || node >= nU) throw Error(IFEM_E_BADPARAM, "vertex-patch smoother: node id outside the owned range");
        tab[size_t(v) * NN + slot] = node;
      }
    }
  }
  // 2. types: presence mask of the nodes + constrained bits of the dofs
  struct Sig {
    uint32_t mask; uint64_t c0, c1;
    bool operator<(const Sig &o) const { return mask != o.mask ? mask < o.mask : (c0 != o.c0 ? c0 < o.c0 : c1 < o.c1); }
  };
  std::map<Sig, int> types;
  std::vector<Sig> sigs;
  std::vector<int32_t> type_of(size_t(nV), 0);
  for (int64_t v = 0; v < nV; ++v) {
    Sig g{0u, 0ull, 0ull};
    for (int k = 0; k < NN; ++k) {
      const int32_t node = tab[size_t(v) * NN + k];
      if (node < 0) continue;
      g.mask |= 1u << k;
      for (int c = 0; c < dim; ++c)
        if (!isc.empty() && isc[size_t(node) * dim + c]) {
          const int bit = k * dim + c;
          if (bit < 64) g.c0 |= 1ull << bit; else g.c1 |= 1ull << (bit - 64);
        }
    }
    if (colour[v] < 0 || !(g.mask & (1u << (NN / 2)))) throw Error(IFEM_E_BADPARAM, "vertex-patch smoother: a vertex without a cell or without its own node");
    auto it = types.find(g);
    if (it == types.end()) {
      if ((int)sigs.size() >= kPatchMaxTypes) return false;
      it = types.emplace(g, (int)sigs.size()).first;
      sigs.push_back(g);
    }
    type_of[v] = it->second;
  }
  // 3. the Q2 box-cell matrix of A0 (fe_tables.cpp, J^-1 = diag(1 / h)), dof = node * dim + component
  const int nd = nu * dim;
  std::vector<double> Ac(size_t(nd) * nd, 0.0);
  double vol = 1, ih[3] = {0, 0, 0};
  for (int e = 0; e < dim; ++e) { vol *= h[e]; ih[e] = 1.0 / h[e]; }
  const double mu = Pm.viscosity, rho = Pm.rho, gam = Pm.grad_div, idt = 1.0 / Pm.dt;
  for (int q = 0; q < fe.nq; ++q) {
    const double w = fe.w[q] * vol;
    for (int a = 0; a < nu; ++a)
      for (int b2 = 0; b2 < nu; ++b2) {
        double gg = 0, ga[3], gb[3];
        for (int e = 0; e < dim; ++e) {
          ga[e] = fe.dphi[(q * nu + a) * dim + e] * ih[e];
          gb[e] = fe.dphi[(q * nu + b2) * dim + e] * ih[e];
          gg += ga[e] * gb[e];
        }
        const double sc = w * (mu * gg + rho * idt * fe.phi[q * nu + a] * fe.phi[q * nu + b2]);
        for (int c = 0; c < dim; ++c)
          for (int e = 0; e < dim; ++e)
            Ac[size_t(a * dim + c) * nd + (b2 * dim + e)] += (c == e ? sc : 0.0) + w * gam * rho * ga[c] * gb[e];
      }
  }
  // ... summed over the present cells of a type, constrained dofs eliminated, inverted
  const int ncorner = 1 << dim;
  std::vector<float> &inv = T.inv;
  inv.assign(size_t(sigs.size()) * N * N, 0.0f);
  std::vector<double> A, Ai;
  for (size_t ty = 0; ty < sigs.size(); ++ty) {
    const Sig &g = sigs[ty];
    A.assign(size_t(N) * N, 0.0);
    for (int oc = 0; oc < ncorner; ++oc) { // the cell in octant oc of the vertex: present iff its centre node is
      int sgn[3], cslot = 0, mul = 1;
      for (int e = 0; e < dim; ++e) { sgn[e] = ((oc >> e) & 1) ? 1 : -1; cslot += (sgn[e] + 1) * mul; mul *= 3; }
      if (!(g.mask & (1u << cslot))) continue;
      // local node a of that cell sits at offset ia - (sgn > 0 ? 0 : 2) from the vertex
      int loc[27];
      for (int a = 0; a < nu; ++a) {
        int ia[3] = {a % 3, (a / 3) % 3, a / 9}, slot = 0;
        bool in = true;
        mul = 1;
        for (int e = 0; e < dim; ++e) {
          const int o = ia[e] - (sgn[e] > 0 ? 0 : 2);
          in = in && o >= -1 && o <= 1;
          slot += (o + 1) * mul;
          mul *= 3;
        }
        loc[a] = in ? slot : -1;
      }
      for (int a = 0; a < nu; ++a) {
        if (loc[a] < 0) continue;
        for (int b2 = 0; b2 < nu; ++b2) {
          if (loc[b2] < 0) continue;
          for (int c = 0; c < dim; ++c)
            for (int e = 0; e < dim; ++e)
              A[size_t(loc[a] * dim + c) * N + (loc[b2] * dim + e)] += Ac[size_t(a * dim + c) * nd + (b2 * dim + e)];
        }
      }
    }
    for (int i = 0; i < N; ++i) {
      const int k = i / dim;
      const bool present = (g.mask >> k) & 1u;
      const bool con = i < 64 ? (g.c0 >> i) & 1ull : (g.c1 >> (i - 64)) & 1ull;
      if (present && !con) continue;
      const double dg = present ? std::fabs(A[size_t(i) * N + i]) : 1.0;
      for (int j = 0; j < N; ++j) { A[size_t(i) * N + j] = 0.0; A[size_t(j) * N + i] = 0.0; }
      A[size_t(i) * N + i] = dg > 0 ? dg : 1.0;
    }
    if (!invert_dense(N, A, Ai)) throw Error(IFEM_E_BADPARAM, "vertex-patch smoother: singular patch matrix");
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) inv[(ty * N + i) * N + j] = float(0.5 * (Ai[size_t(i) * N + j] + Ai[size_t(j) * N + i]));
  }
  // 4. patches sorted by (colour, type), work items of at most kPatchChunk patches of one colour and type
  std::vector<int32_t> order(static_cast<size_t>(nV));
  for (int64_t v = 0; v < nV; ++v) order[v] = int32_t(v);
  std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
    return colour[x] != colour[y] ? colour[x] < colour[y] : type_of[x] < type_of[y];
  });
  std::vector<int32_t> &stab = T.tab, &work = T.work;
  stab.assign(size_t(nV) * NN, 0);
  work.clear();
  for (int64_t k = 0; k < nV; ++k) std::memcpy(&stab[size_t(k) * NN], &tab[size_t(order[k]) * NN], NN * sizeof(int32_t));
  int *wp = T.work_ptr;
  for (int c = 0; c < 9; ++c) wp[c] = 0;
  for (int64_t k = 0; k < nV;) {
    const int col = colour[order[k]], ty = type_of[order[k]];
    int64_t e = k;
    while (e < nV && e - k < kPatchChunk && colour[order[e]] == col && type_of[order[e]] == ty) ++e;
    work.push_back(ty); work.push_back(int32_t(k)); work.push_back(int32_t(e - k));
    wp[col + 1] = int(work.size() / 3);
    k = e;
  }
  for (int c = 1; c <= ncorner; ++c) wp[c] = std::max(wp[c], wp[c - 1]); // a colour without a patch: an empty range
  T.n_types = int(sigs.size());
  return true;
}

static bool patch_gen_setup(ifem_ctx *ctx, const double key[9]);
static void patch_gen_apply(ifem_ctx *ctx, double a, double b, const float *r, float *d);

bool patch_setup(ifem_ctx *ctx) {
  PatchSmoother &S = ctx->patch;
  const int form = patch_form(ctx);
  S.eligible = form >= 0;
  if (!S.eligible) return false;
  if (!ctx->mf_valid) throw Error(IFEM_E_BADPARAM, "vertex-patch smoother: no operator state on this level");
  const int dim = ctx->dim, nu = ctx->nu, np = ctx->np;
  const int cs = ctx->asm_constraint_set;
  const ifem_ins_params &Pm = ctx->mf_params;
  const double key[9] = {Pm.viscosity, Pm.rho, Pm.grad_div, Pm.dt, form == 0 ? ctx->mf_h[0] : 0.0, form == 0 ? ctx->mf_h[1] : 0.0,
                         form == 0 ? ctx->mf_h[2] : 0.0, ctx->has_c[cs] ? double(ctx->flag_id[cs]) : -2.0, double(form)};
  if (S.valid && std::memcmp(key, S.key, sizeof(key)) == 0) return true;
  S.valid = false;
  if (form == 1) {
    S.eligible = patch_gen_setup(ctx, key);
    return S.eligible;
  }
  hipStream_t s = ctx->stream;
  const int64_t nc = ctx->n_cells, nV = ctx->nPl, nU = ctx->nUo;
  const std::vector<int32_t> cu = ctx->cell_unodes.download(s), cp = ctx->cell_pnodes.download(s);
  const std::vector<double> vc = ctx->vcoords.download(s);
  std::vector<uint8_t> isc;
  if (ctx->has_c[cs]) isc = ctx->is_c[cs].download(s);
  if ((int64_t)cu.size() != nc * nu || (int64_t)cp.size() != nc * np || (int64_t)vc.size() != nc * np * dim || (!isc.empty() && (int64_t)isc.size() < nU * dim))
    throw Error(IFEM_E_BADPARAM, "vertex-patch smoother: cell tables of unexpected size");
  PatchTables T;
  if (!patch_build(dim, nc, nV, nU, cu, cp, vc, isc, ctx->mf_h, Pm, ctx->fe, T)) { S.eligible = false; return false; }
  S.tab.upload(T.tab.data(), T.tab.size(), s);
  S.inv.upload(T.inv.data(), T.inv.size(), s);
  S.work.upload(T.work.data(), T.work.size(), s);
  IFEM_HIP_CHECK(hipStreamSynchronize(s)); // (the host arrays leave scope)
  std::memcpy(S.work_ptr, T.work_ptr, sizeof(S.work_ptr));
  S.n_patches = nV;
  S.n_types = T.n_types;
  S.inv_bytes = int64_t(T.inv.size() * sizeof(float));
  std::memcpy(S.key, key, sizeof(key));
  S.form = 0;
  S.valid = true;
  return true;
}

void patch_apply(ifem_ctx *ctx, double a, double b, const float *r, float *d) {
  const PatchSmoother &S = ctx->patch;
  if (!S.valid || !S.eligible) throw Error(IFEM_E_BADPARAM, "vertex-patch smoother applied without its tables (patch_setup)");
  if (S.form == 1) { patch_gen_apply(ctx, a, b, r, d); return; }
  const int dim = ctx->dim, ncol = 1 << dim, N = dim * (dim == 3 ? 27 : 9);
  // per patch: its node table, the gathered residual and the read-modify-write of d; 2 N^2 flops
  KScope ks(ctx, IFEM_KC_VECTOR, double(S.n_patches) * (N / dim) * (4.0 + 12.0 * dim), 2.0 * double(S.n_patches) * N * N);
  for (int c = 0; c < ncol; ++c) {
    const int nw = S.work_ptr[c + 1] - S.work_ptr[c];
    if (nw <= 0) continue;
    const int32_t *w = S.work.p + size_t(S.work_ptr[c]) * 3;
    if (dim == 3) hipLaunchKernelGGL((k_patch_apply<3>), dim3(unsigned(nw)), dim3(256), 0, ctx->stream, S.tab.p, S.inv.p, w, c, float(a), float(b), r, d);
    else hipLaunchKernelGGL((k_patch_apply<2>), dim3(unsigned(nw)), dim3(256), 0, ctx->stream, S.tab.p, S.inv.p, w, c, float(a), float(b), r, d);
  }
  IFEM_HIP_CHECK(hipGetLastError());
}


// ---------------------------------------------------------------------------------------------------------------------------------------
// The general form (ifem_tuning::uu_patch_levels = 1): levels whose cells differ -- curved or graded meshes, the cylinder.
//
// Same patch, stated without a lattice: for every cell that holds vertex v at its corner b, the 2^dim local nodes within one node spacing
// of b in the cell's reference lattice.  A vertex of valence 1, 2, 4, 5 in 2D gives 4 / 6 / 9 / 11 nodes; the extruded 3D cylinder 8 / 12 /
// 18 / 22 / 27 / 33 nodes (up to 99 dofs).  Every cell that holds a node of the patch holds v, so A_v = R_v A0 R_v^T is the sum of those cells'
// sub-blocks (the host checks that a cell's nodes inside the patch are exactly the 2^dim near its corner; a level where they are not is refused).
// Caps: at most 13 (2D) / 39 (3D) nodes per patch, at most 16 colours, fewer than 2^28 cells.  A level beyond a cap is not eligible and
// keeps its node blocks; nothing throws.
//
// Tables (host, topology only, once per context): per patch its node list, its (cell, corner) list and the 64-bit offset of its inverse;
// per (patch, node) one bit that says that this patch has the lowest colour among the patches holding the node -- it applies the term a d,
// which the box kernel derives from lattice parity.  Colours: greedy in vertex order under "no two vertices of one cell share a colour"
// (two patches share a node only if their vertices share a cell): deterministic, 5 colours on the 2D cylinder, 10 on the extruded one.
// Patches are sorted by colour, then by size.
//
// Setup kernel (fp64, once per (mu, rho, gamma, dt, constrained-dof set)): one workgroup per patch.  Per cell of the patch the
// (2^dim dim)^2 sub-block of A0 is integrated over the cell's quadrature points (J^-1 and JxW from the Q1 vertex map, the 1D tables of the
// matrix-free kernels) and added to the patch matrix, which lives in LDS as a packed lower triangle (117 x 118 / 2 doubles = 54 kB: the
// whole kernel stays below the 64 kB a workgroup gets without opt-in).  Constrained dofs become decoupled 1 x 1 rows with |a_ii|, then
// the matrix is inverted in place by symmetric Gauss-Jordan sweeps without pivoting (A_v is symmetric positive definite: the rho / dt mass
// term; condition number <= 41 on the cylinder at gamma rho / mu = 100).  A pivot that is not positive sets a flag: the level is refused.
// The inverse goes out as a full float [N_v][N_v] (symmetric by construction).
//
// Apply kernel (fp32): d <- a d + b B r, one launch per colour, plain stores in a fixed order.  Every patch streams its own inverse from
// memory once -- 2 flops per 4 bytes, bound by bandwidth -- so the layout serves the loads: a group of G lanes (64 in 3D, 32 in 2D; 4 / 8
// patches per workgroup) takes a patch, lane i accumulates row i (and i + 64 in 3D), and for each column j reads float j N + i: consecutive
// lanes, consecutive floats (the symmetric inverse read by column).  The patch's residual is gathered into LDS once.  Lanes beyond the patch's
// size read nothing and store nothing.
template <int DIM>
struct GenDims {
  static constexpr int CAPNN = DIM == 3 ? 39 : 13; // most nodes of a patch
  static constexpr int CAPN = DIM * CAPNN;         // most dofs: 117 / 26
  static constexpr int NK = 1 << DIM;              // nodes of a cell within one node spacing of a corner
  static constexpr int NQ = DIM == 3 ? 27 : 9;     // quadrature points = nodes of a Q2 cell
  static constexpr int G = DIM == 3 ? 64 : 32;     // apply: lanes per patch
  static constexpr int ROWS = DIM == 3 ? 2 : 1;    // apply: rows per lane, G ROWS >= CAPN
  static constexpr int PPB = 256 / G;              // apply: patches per workgroup
};
constexpr int kPatchMaxColours = 16;

struct PatchGenArgs {
  const int64_t *node_ptr, *cell_ptr, *inv_off;
  const int32_t *nodes, *cells;
  const double *vcoords;
  const int32_t *cell_unodes;
  const uint8_t *is_c;
  float *inv;
  int32_t *bad;
  double mu, rho, gamma, inv_dt;
  Tab1D t;
};

template <int DIM>
__global__ __launch_bounds__(256) void k_patch_gen_setup(PatchGenArgs A) {
  using D = GenDims<DIM>;
  constexpr int NK = D::NK, NQ = D::NQ, NV = 1 << DIM, M = NK * DIM;
  __shared__ double sA[D::CAPN * (D::CAPN + 1) / 2]; // packed lower triangle of the patch matrix: (i, j <= i) at i (i + 1) / 2 + j
  __shared__ double sCol[D::CAPN];
  __shared__ double sG[NQ * NK * DIM], sN[NQ * NK], sW[NQ], sX[NV * DIM]; // per cell: physical gradients / values of its near nodes, JxW, vertices
  __shared__ double tN[9], tD[9], tX[3], tW[3];
  __shared__ int32_t sNode[D::CAPNN], sSlot[NK];
  __shared__ uint8_t sCon[D::CAPN];
  const int t = threadIdx.x;
  const int64_t p = blockIdx.x, n0 = A.node_ptr[p];
  const int nn = min(int(A.node_ptr[p + 1] - n0), D::CAPNN), N = nn * DIM, NP = N * (N + 1) / 2;
  if (t < 9) { tN[t] = A.t.N[t]; tD[t] = A.t.dN[t]; }
  if (t < 3) { tX[t] = A.t.xi[t]; tW[t] = A.t.w[t]; }
  if (t < nn) sNode[t] = A.nodes[n0 + t] & 0x7fffffff;
  for (int e = t; e < NP; e += 256) sA[e] = 0.0;
  __syncthreads();
  if (t < N) sCon[t] = A.is_c ? A.is_c[int64_t(sNode[t / DIM]) * DIM + t % DIM] : uint8_t(0);
  for (int64_t k = A.cell_ptr[p]; k < A.cell_ptr[p + 1]; ++k) {
    const int32_t cb = A.cells[k];
    const int64_t cell = cb >> 3;
    const int b = cb & 7;
    __syncthreads(); // the previous cell's tables are consumed
    if (t < NV * DIM) sX[t] = A.vcoords[cell * NV * DIM + t];
    if (t < NK) { // the near node t of corner b and its place in the patch
      int a = 0, mul = 1;
#pragma unroll
      for (int e = 0; e < DIM; ++e) { a += (((b >> e) & 1) + ((t >> e) & 1)) * mul; mul *= 3; }
      const int32_t node = A.cell_unodes[cell * NQ + a];
      int slot = -1;
      for (int i = 0; i < nn; ++i) slot = sNode[i] == node ? i : slot;
      sSlot[t] = slot;
    }
    __syncthreads();
    if (t < NQ * NK) { // (quadrature point, near node): the d-linear map's Jacobian at the point, the node's shape value and physical gradient
      const int q = t / NK, kn = t - q * NK;
      int qi[DIM];
      double L[DIM][2], wq = 1.0;
#pragma unroll
      for (int e = 0, r = q; e < DIM; ++e) {
        qi[e] = r % 3; r /= 3;
        const double x_ = tX[qi[e]];
        L[e][1] = x_; L[e][0] = 1.0 - x_; wq *= tW[qi[e]];
      }
      double J[DIM * DIM], Ji[DIM * DIM];
#pragma unroll
      for (int i = 0; i < DIM * DIM; ++i) J[i] = 0.0;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
#pragma unroll
        for (int dd = 0; dd < DIM; ++dd) {
          double g = ((v >> dd) & 1) ? 1.0 : -1.0;
#pragma unroll
          for (int o = 0; o < DIM; ++o) if (o != dd) g *= L[o][(v >> o) & 1];
#pragma unroll
          for (int e = 0; e < DIM; ++e) J[e * DIM + dd] += sX[v * DIM + e] * g;
        }
      }
      const double det = inv_small<DIM, double>(J, Ji);
      if (kn == 0) sW[q] = fabs(det) * wq;
      double nv[DIM], dv[DIM], Nval = 1.0;
#pragma unroll
      for (int e = 0; e < DIM; ++e) {
        const int ia = ((b >> e) & 1) + ((kn >> e) & 1);
        nv[e] = tN[qi[e] * 3 + ia]; dv[e] = tD[qi[e] * 3 + ia];
        Nval *= nv[e];
      }
      double dr[DIM];
#pragma unroll
      for (int e = 0; e < DIM; ++e) {
        double g = dv[e];
#pragma unroll
        for (int o = 0; o < DIM; ++o) if (o != e) g *= nv[o];
        dr[e] = g;
      }
      sN[q * NK + kn] = Nval;
#pragma unroll
      for (int dd = 0; dd < DIM; ++dd) { // physical gradient d_dd N = sum_e (d^_e N) Ji[e][dd]
        double g = 0.0;
#pragma unroll
        for (int e = 0; e < DIM; ++e) g += dr[e] * Ji[e * DIM + dd];
        sG[(q * NK + kn) * DIM + dd] = g;
      }
    }
    __syncthreads();
    for (int e = t; e < M * M; e += 256) { // entry (near node ka, component c) x (kb, c2) of the cell's sub-block, lower triangle of the patch
      const int ra = e / M, rb = e - ra * M, ka = ra / DIM, c = ra - ka * DIM, kb = rb / DIM, c2 = rb - kb * DIM;
      const int sa = sSlot[ka], sb = sSlot[kb];
      const int I = sa * DIM + c, Jx = sb * DIM + c2;
      if (sa < 0 || sb < 0 || I < Jx) continue;
      double sum = 0.0;
      for (int q = 0; q < NQ; ++q) {
        const double *ga = &sG[(q * NK + ka) * DIM], *gb = &sG[(q * NK + kb) * DIM];
        double gg = 0.0;
#pragma unroll
        for (int dd = 0; dd < DIM; ++dd) gg += ga[dd] * gb[dd];
        const double sc = c == c2 ? A.mu * gg + A.rho * A.inv_dt * sN[q * NK + ka] * sN[q * NK + kb] : 0.0;
        sum += sW[q] * (sc + A.gamma * A.rho * ga[c] * gb[c2]);
      }
      sA[I * (I + 1) / 2 + Jx] += sum; // (one entry of this cell per place: no two threads meet)
    }
  }
  __syncthreads();
  // my entries of the packed triangle: t, t + 256, ...; (i, j) walks along with them
  int i0 = 0, j0 = t;
  while (j0 > i0) { j0 -= i0 + 1; ++i0; }
  // the constraint rule of the assembly: a constrained dof is a decoupled 1 x 1 row / column with |a_ii|
  for (int e = t, i = i0, j = j0; e < NP; e += 256) {
    if (sCon[i] || sCon[j]) {
      const double v = fabs(sA[e]);
      sA[e] = i == j ? (v > 0.0 ? v : 1.0) : 0.0;
    }
    j += 256;
    while (j > i) { j -= i + 1; ++i; }
  }
  // in-place inverse by symmetric Gauss-Jordan sweeps: after all of them the triangle holds -A^-1
  for (int k = 0; k < N; ++k) {
    __syncthreads();
    if (t < N) sCol[t] = t >= k ? sA[t * (t + 1) / 2 + k] : sA[k * (k + 1) / 2 + t];
    __syncthreads();
    const double dk = sCol[k];
    if (!(dk > 0.0) || !(dk < 1e300)) { // (the same value in every thread: the whole workgroup leaves)
      if (t == 0) atomicMax(A.bad, 1);
      return;
    }
    const double idk = 1.0 / dk;
    for (int e = t, i = i0, j = j0; e < NP; e += 256) {
      double v;
      if (i == k) v = j == k ? -idk : sCol[j] * idk;
      else if (j == k) v = sCol[i] * idk;
      else v = sA[e] - sCol[i] * sCol[j] * idk;
      sA[e] = v;
      j += 256;
      while (j > i) { j -= i + 1; ++i; }
    }
  }
  __syncthreads();
  float *out = A.inv + A.inv_off[p];
  for (int e = t; e < N * N; e += 256) {
    const int i = e / N, j = e - i * N, hi = max(i, j), lo = min(i, j);
    out[e] = float(-sA[hi * (hi + 1) / 2 + lo]);
  }
}

template <int DIM>
__global__ __launch_bounds__(256) void k_patch_gen_apply(const int64_t *__restrict__ node_ptr, const int32_t *__restrict__ nodes,
                                                         const int64_t *__restrict__ inv_off, const float *__restrict__ inv, int64_t p0,
                                                         int64_t cnt, float a, float b, const float *__restrict__ r, float *__restrict__ d) {
  using D = GenDims<DIM>;
  constexpr int G = D::G, ROWS = D::ROWS, PPB = D::PPB, LD = G * ROWS;
  __shared__ float sR[PPB * LD];
  __shared__ int32_t sNode[PPB * D::CAPNN];
  const int g = threadIdx.x / G, l = threadIdx.x - g * G;
  const int64_t pi = int64_t(blockIdx.x) * PPB + g;
  const bool live = pi < cnt;
  const int64_t p = p0 + (live ? pi : 0);
  const int64_t n0 = node_ptr[p];
  const int N = live ? DIM * min(int(node_ptr[p + 1] - n0), D::CAPNN) : 0;
  if (l * DIM < N && l < D::CAPNN) sNode[g * D::CAPNN + l] = nodes[n0 + l];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ROWS; ++k) {
    const int i = l + k * G;
    if (i < N) sR[g * LD + i] = r[int64_t(sNode[g * D::CAPNN + i / DIM] & 0x7fffffff) * DIM + i % DIM];
  }
  __syncthreads();
  const float *__restrict__ m = inv + inv_off[p];
  float acc[ROWS];
#pragma unroll
  for (int k = 0; k < ROWS; ++k) acc[k] = 0.0f;
#pragma unroll 4
  for (int j = 0; j < N; ++j) {
    const float rj = sR[g * LD + j];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
      const int i = l + k * G;
      if (i < N) acc[k] = fmaf(m[j * N + i], rj, acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < ROWS; ++k) {
    const int i = l + k * G;
    if (i >= N) continue;
    const int32_t e = sNode[g * D::CAPNN + i / DIM];
    const int64_t idx = int64_t(e & 0x7fffffff) * DIM + i % DIM;
    float v = b * acc[k];
    if (e >= 0) v += d[idx];                 // a patch of a lower colour has been here
    else if (a != 0.0f) v += a * d[idx];     // the first one applies a d (a = 0: d holds nothing yet and is not read)
    d[idx] = v;
  }
}

// topology of the general form, once per context (the mesh never changes).  false: the level is beyond a cap
static bool patch_gen_topology(ifem_ctx *ctx) {
  PatchSmoother &S = ctx->patch;
  if (S.gen_state) return S.gen_state > 0;
  S.gen_state = -1;
  const int dim = ctx->dim, nu = ctx->nu, np = ctx->np, nk = 1 << dim, cap = dim == 3 ? GenDims<3>::CAPNN : GenDims<2>::CAPNN;
  const int64_t nc = ctx->n_cells, nV = ctx->nPl, nU = ctx->nUo;
  if (nc >= (int64_t(1) << 28) || nV <= 0) return false;
  hipStream_t s = ctx->stream;
  const std::vector<int32_t> cu = ctx->cell_unodes.download(s), cp = ctx->cell_pnodes.download(s);
  if ((int64_t)cu.size() != nc * nu || (int64_t)cp.size() != nc * np) throw Error(IFEM_E_BADPARAM, "vertex-patch smoother: cell tables of unexpected size");
  for (int32_t v : cp) if (v < 0 || v >= nV) throw Error(IFEM_E_BADPARAM, "vertex-patch smoother: vertex id outside the level");
  for (int32_t n : cu) if (n < 0 || n >= nU) throw Error(IFEM_E_BADPARAM, "vertex-patch smoother: node id outside the owned range");
  // vertex -> (cell, corner)
  std::vector<int64_t> vptr(size_t(nV) + 1, 0);
  for (int32_t v : cp) ++vptr[size_t(v) + 1];
  for (int64_t v = 0; v < nV; ++v) vptr[v + 1] += vptr[v];
  std::vector<int32_t> vcell(size_t(nc) * np);
  {
    std::vector<int64_t> fill(vptr.begin(), vptr.end() - 1);
    for (int64_t c = 0; c < nc; ++c)
      for (int b = 0; b < np; ++b) vcell[size_t(fill[cp[c * np + b]]++)] = int32_t(c << 3 | b);
  }
  int near[8][8]; // local node k of the 2^dim within one node spacing of corner b
  for (int b = 0; b < np; ++b)
    for (int k = 0; k < nk; ++k) {
      int a = 0, mul = 1;
      for (int e = 0; e < dim; ++e) { a += (((b >> e) & 1) + ((k >> e) & 1)) * mul; mul *= 3; }
      near[b][k] = a;
    }
  // nodes of every patch in the order its cells bring them; greedy colours in vertex order
  std::vector<int64_t> nptr(size_t(nV) + 1, 0);
  std::vector<int32_t> pn;
  pn.reserve(size_t(nV) * (dim == 3 ? 27 : 9));
  std::vector<int32_t> stamp(size_t(nU), -1);
  std::vector<int8_t> colour(size_t(nV), -1);
  int n_colours = 0;
  for (int64_t v = 0; v < nV; ++v) {
    if (vptr[v + 1] == vptr[v]) return false; // a vertex without a cell
    uint32_t used = 0;
    for (int64_t k = vptr[v]; k < vptr[v + 1]; ++k) {
      const int64_t c = vcell[k] >> 3;
      const int b = vcell[k] & 7;
      for (int k2 = 0; k2 < nk; ++k2) {
        const int32_t node = cu[c * nu + near[b][k2]];
        if (stamp[node] != v) { stamp[node] = int32_t(v); pn.push_back(node); }
      }
      for (int b2 = 0; b2 < np; ++b2) {
        const int8_t cw = colour[cp[c * np + b2]];
        if (cw >= 0) used |= 1u << cw;
      }
    }
    nptr[v + 1] = int64_t(pn.size());
    if (nptr[v + 1] - nptr[v] > cap) return false;
    // every node of a cell of the patch that lies in the patch must be one of the 2^dim near its corner: then the cells' sub-blocks sum to A_v
    for (int64_t k = vptr[v]; k < vptr[v + 1]; ++k) {
      const int64_t c = vcell[k] >> 3;
      int inside = 0;
      for (int a = 0; a < nu; ++a) inside += stamp[cu[c * nu + a]] == v;
      if (inside != nk) return false;
    }
    int col = 0;
    while (col < kPatchMaxColours && ((used >> col) & 1u)) ++col;
    if (col >= kPatchMaxColours) return false;
    colour[v] = int8_t(col);
    n_colours = std::max(n_colours, col + 1);
  }
  // the patch of the lowest colour among those that hold a node applies a d there
  std::vector<int8_t> minc(static_cast<size_t>(nU), static_cast<int8_t>(kPatchMaxColours));
  for (int64_t v = 0; v < nV; ++v)
    for (int64_t k = nptr[v]; k < nptr[v + 1]; ++k) minc[pn[k]] = std::min(minc[pn[k]], colour[v]);
  for (int64_t n = 0; n < nU; ++n)
    if (minc[n] >= kPatchMaxColours) return false; // a node no patch covers
  // sorted by (colour, nodes)
  std::vector<int32_t> order(static_cast<size_t>(nV));
  for (int64_t v = 0; v < nV; ++v) order[v] = int32_t(v);
  std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
    if (colour[x] != colour[y]) return colour[x] < colour[y];
    return nptr[x + 1] - nptr[x] < nptr[y + 1] - nptr[y];
  });
  std::vector<int64_t> node_ptr(size_t(nV) + 1, 0), cell_ptr(size_t(nV) + 1, 0), inv_off(static_cast<size_t>(nV), 0);
  std::vector<int32_t> nodes(pn.size()), cells(vcell.size());
  int64_t floats = 0;
  for (int c = 0; c <= kPatchMaxColours; ++c) S.gen_col_ptr[c] = 0;
  for (int64_t k = 0; k < nV; ++k) {
    const int64_t v = order[k], nn = nptr[v + 1] - nptr[v], ncl = vptr[v + 1] - vptr[v];
    for (int64_t i = 0; i < nn; ++i) {
      const int32_t node = pn[nptr[v] + i];
      nodes[node_ptr[k] + i] = minc[node] == colour[v] ? int32_t(uint32_t(node) | 0x80000000u) : node;
    }
    std::memcpy(&cells[cell_ptr[k]], &vcell[vptr[v]], size_t(ncl) * sizeof(int32_t));
    node_ptr[k + 1] = node_ptr[k] + nn;
    cell_ptr[k + 1] = cell_ptr[k] + ncl;
    inv_off[k] = floats;
    floats += (nn * dim) * (nn * dim);
    S.gen_col_ptr[colour[v] + 1] = k + 1;
  }
  for (int c = 1; c <= kPatchMaxColours; ++c) S.gen_col_ptr[c] = std::max(S.gen_col_ptr[c], S.gen_col_ptr[c - 1]);
  S.gen_node_ptr.upload(node_ptr.data(), node_ptr.size(), s);
  S.gen_cell_ptr.upload(cell_ptr.data(), cell_ptr.size(), s);
  S.gen_inv_off.upload(inv_off.data(), inv_off.size(), s);
  S.gen_nodes.upload(nodes.data(), nodes.size(), s);
  S.gen_cells.upload(cells.data(), cells.size(), s);
  S.gen_bad.alloc(1);
  IFEM_HIP_CHECK(hipStreamSynchronize(s)); // (the host arrays leave scope)
  S.gen_colours = n_colours;
  S.gen_entries = int64_t(pn.size());
  S.gen_inv_floats = floats;
  S.gen_state = 1;
  return true;
}

// inverses of the general form for the level's operator state.  false: the level keeps its node blocks (a cap, the memory, a pivot)
static bool patch_gen_setup(ifem_ctx *ctx, const double key[9]) {
  PatchSmoother &S = ctx->patch;
  if (S.gen_rejected && std::memcmp(key, S.gen_rejected_key, sizeof(S.gen_rejected_key)) == 0) return false;
  if (!patch_gen_topology(ctx)) return false;
  hipStream_t s = ctx->stream;
  const int dim = ctx->dim, cs = ctx->asm_constraint_set;
  const int64_t nV = ctx->nPl;
  auto refuse = [&] {
    S.gen_rejected = true;
    std::memcpy(S.gen_rejected_key, key, sizeof(S.gen_rejected_key));
    return false;
  };
  if (S.form != 1 || (int64_t)S.inv.n != S.gen_inv_floats) { // the store of the other form, or none yet: does this one fit?
    S.inv.release();
    size_t fr = 0, tot = 0;
    IFEM_HIP_CHECK(hipMemGetInfo(&fr, &tot));
    if (double(S.gen_inv_floats) * sizeof(float) + double(256u << 20) > double(fr)) return refuse();
    S.inv.alloc(size_t(S.gen_inv_floats), "the inverse store of the vertex-patch smoother");
    S.tab.release(); S.work.release();
  }
  S.form = 1;
  PatchGenArgs a{};
  a.node_ptr = S.gen_node_ptr.p; a.cell_ptr = S.gen_cell_ptr.p; a.inv_off = S.gen_inv_off.p;
  a.nodes = S.gen_nodes.p; a.cells = S.gen_cells.p;
  a.vcoords = ctx->vcoords.p; a.cell_unodes = ctx->cell_unodes.p;
  a.is_c = ctx->has_c[cs] ? ctx->is_c[cs].p : nullptr;
  a.inv = S.inv.p; a.bad = S.gen_bad.p;
  a.mu = ctx->mf_params.viscosity; a.rho = ctx->mf_params.rho; a.gamma = ctx->mf_params.grad_div; a.inv_dt = 1.0 / ctx->mf_params.dt;
  tab1d(a.t, ctx->kv);
  int32_t bad = 0;
  {
    const double N = dim * (dim == 3 ? 27.0 : 9.0); // a typical patch: integration of its cells + N^3 of the sweeps
    KScope ks(ctx, IFEM_KC_SMOOTHER_SETUP, double(S.gen_inv_floats) * sizeof(float) + double(S.gen_cells.n) * (4.0 + 8.0 * ctx->np * dim + 4.0 * ctx->nu),
              double(nV) * N * N * N);
    IFEM_HIP_CHECK(hipMemsetAsync(S.gen_bad.p, 0, sizeof(int32_t), s));
    if (dim == 3) hipLaunchKernelGGL((k_patch_gen_setup<3>), dim3(unsigned(nV)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_patch_gen_setup<2>), dim3(unsigned(nV)), dim3(256), 0, s, a);
    IFEM_HIP_CHECK(hipGetLastError());
    IFEM_HIP_CHECK(hipMemcpyAsync(&bad, S.gen_bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
  }
  if (bad) return refuse(); // a patch matrix that is not positive definite
  S.n_patches = nV;
  S.n_types = 0;
  S.inv_bytes = S.gen_inv_floats * int64_t(sizeof(float));
  std::memcpy(S.key, key, sizeof(S.key));
  S.valid = true;
  return true;
}

static void patch_gen_apply(ifem_ctx *ctx, double a, double b, const float *r, float *d) {
  const PatchSmoother &S = ctx->patch;
  const int dim = ctx->dim;
  // every patch streams its inverse once; its node list; the gathered residual and the read-modify-write of d.  2 N_v^2 flops per patch
  KScope ks(ctx, IFEM_KC_VECTOR, double(S.inv_bytes) + double(S.gen_entries) * (4.0 + 12.0 * dim) + double(S.n_patches) * 24.0, 2.0 * double(S.gen_inv_floats));
  for (int c = 0; c < S.gen_colours; ++c) {
    const int64_t p0 = S.gen_col_ptr[c], cnt = S.gen_col_ptr[c + 1] - p0;
    if (cnt <= 0) continue;
    if (dim == 3)
      hipLaunchKernelGGL((k_patch_gen_apply<3>), dim3(unsigned((cnt + GenDims<3>::PPB - 1) / GenDims<3>::PPB)), dim3(256), 0, ctx->stream, S.gen_node_ptr.p,
                         S.gen_nodes.p, S.gen_inv_off.p, S.inv.p, p0, cnt, float(a), float(b), r, d);
    else
      hipLaunchKernelGGL((k_patch_gen_apply<2>), dim3(unsigned((cnt + GenDims<2>::PPB - 1) / GenDims<2>::PPB)), dim3(256), 0, ctx->stream, S.gen_node_ptr.p,
                         S.gen_nodes.p, S.gen_inv_off.p, S.inv.p, p0, cnt, float(a), float(b), r, d);
  }
  IFEM_HIP_CHECK(hipGetLastError());
}

} // namespace ifem
