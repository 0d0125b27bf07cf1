// patch.hip -- vertex-patch smoother of the A_uu V-cycle on uniform box levels (ifem_tuning::uu_smoother = 1).
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

bool patch_eligible(const ifem_ctx *c) {
  return mf_takes_uniform(c) && c->kv == 2 && c->halo.nranks == 1 && !c->hang.active && c->hang.n == 0 && c->n_cells > 0 && c->nUl == c->nUo;
}

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

bool patch_setup(ifem_ctx *ctx) {
  PatchSmoother &S = ctx->patch;
  S.eligible = patch_eligible(ctx);
  if (!S.eligible) return false;
  if (!ctx->mf_valid) throw Error(IFEM_E_BADPARAM, "vertex-patch smoother: no operator state on this level");
  const int dim = ctx->dim, nu = ctx->nu, np = ctx->np;
  const int cs = ctx->asm_constraint_set;
  const ifem_ins_params &Pm = ctx->mf_params;
  const double key[8] = {Pm.viscosity, Pm.rho, Pm.grad_div, Pm.dt, ctx->mf_h[0], ctx->mf_h[1], ctx->mf_h[2],
                         ctx->has_c[cs] ? double(ctx->flag_id[cs]) : -2.0};
  if (S.valid && std::memcmp(key, S.key, sizeof(key)) == 0) return true;
  S.valid = false;
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
  S.valid = true;
  return true;
}

void patch_apply(ifem_ctx *ctx, double a, double b, const float *r, float *d) {
  const PatchSmoother &S = ctx->patch;
  if (!S.valid || !S.eligible) throw Error(IFEM_E_BADPARAM, "vertex-patch smoother applied without its tables (patch_setup)");
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

} // namespace ifem
