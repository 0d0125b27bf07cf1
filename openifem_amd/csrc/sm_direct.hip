// sm_direct.hip -- x = S_m^-1 b on a uniform Q2/Q1 box level by fast diagonalisation (ifem_solver_opts::sm_mg = 2).
//
// On an axis-aligned uniform box whose constrained velocity dofs are whole faces per component, S_m = B diag(M_u)^-1 B^T is a sum of `dim`
// Kronecker products of 1D matrices, S_m = sum_c (x)_a F_{c,a}, F_{c,a} = X diag(d_{c,a} / m_a) X^T with X the 1D derivative coupling G_a for
// a = c and the 1D mass coupling N_a otherwise (sm_direct_host.cpp).  Where the mass-like factors of every axis coincide (no-slip, free and
// normal-only faces; not tangential-only ones) the generalised eigenvectors K_a q = lambda M~_a q, Q_a^T M~_a Q_a = I, diagonalise all terms:
//   S_m^-1 = (Q_z (x) Q_y (x) Q_x) diag(1 / (lambda_x[i] + lambda_y[j] + lambda_z[k])) (Q_z (x) Q_y (x) Q_x)^T,
// six contractions and one scale instead of the multigrid-preconditioned CG of solver.hip::solve_sm.
//
// The closed form is never trusted on its own.  sm_direct_setup (solver.hip::sm_ensure, set-up time only, never inside a captured region)
// decides the level, builds the factors of an axis whose key (cells, edge, masks) changed, and probes the present S_m whenever it was
// re-formed (ifem_ctx::sm_version): a pseudo-random e, x = direct(e), y = S_m x with the context's own fp64 product (stencil or CSR),
// max |y - e| <= 1e-7 max |e| on the device.  The CG this replaces stops at 1e-3; a structural mismatch (one stray constrained node) is an
// O(1) local error; the rounding floor eps cond(Lambda) is a few 1e-9 at 128^3.  A context that fails keeps CG from then on.
//
// Eligibility: one rank, no hanging-node line, ifem_ctx::mf_uniform, Q2 velocity and Q1 pressure on full lattices (setup.hip::u_lattice_ensure),
// explicit S_m, no SCnsIM blocks, not a multigrid coarse level, at most kSmdMaxAxis = 513 pressure nodes per axis, the constrained dofs of
// every component whole faces (the face-centre nodes give the masks, the constrained-dof counts must be what the masks imply:
// k_smd_masks), M~_a positive definite on every axis and min Lambda > 1e-12 max Lambda (the enclosed flow keeps CG).
//
// Kernels.  The work vectors are lattice-ordered, x fastest; the node order is folded into the first read (b[node_of_lattice[.]]) and the last
// store, there is no permutation pass.
//   k_smd_contract  out[.., i, ..] = sum_k A[i][k] in[.., k, ..] along one axis, A = Q_a^T (forward) or Q_a (backward), zero-padded to a
//                   multiple of 16 (129 -> 144), on v_mfma_f64_16x16x4_f64 (operand layout as in assemble3.hip: A operand row = lane & 15,
//                   k = lane >> 4; result row = (lane >> 4) + 4 r, column = lane & 15).  A block of 4 waves forms a 64 (i) x 64 (columns) tile of
//                   the result; per step of 32 in k it stages the A panel [64][32] (row pitch 34 doubles: the 16 x 2 fragment reads of a
//                   half-wave fall on 32 different banks) and the tile of the input [32][64] (pitch 80: the two k rows of a half-wave lie
//                   32 banks apart) through LDS, 37 KB; the loads of the next step are issued before the MFMAs of the present one.
//                   A strided axis (y, z): the columns are the faster lattice axes, neighbouring lanes on neighbouring x, wave w owns the
//                   16 rows i of its sub-tile.  The x axis: the columns are the lines, the k index is the contiguous one, the roles of the two
//                   MFMA operands are swapped so that the result again has 16 consecutive doubles per store row.  On a strided axis the 16-row
//                   sub-tiles beyond the padded axis are skipped, on the x axis they are staged as zeros.  The last forward contraction scales by 1 / (lambda_x[i] + lambda_y[j] + lambda_z[k]) from the three
//                   1D arrays in its store (no 3D table).  Passes: x (gather), y, z (scale) | z, y, x (scatter); 2D: x, y (scale) | y, x.
// Per application and node, 3D: 2 npad flops per contraction, 6 contractions (128^3: 144 x 2 x 6 x 129^3 = 3.7 GFLOP; 4.1 with the 64-row tail tile of the two x passes); bytes 8 read x
// ceil(npad / 64) + 8 written per contraction, + 4 for the index of the first and the last (128^3: 6 x 32 + 8 = 200 B per node, 0.43 GB, of
// which the re-reads of the input tile by the other i tiles are L2 hits).
// fp64 throughout, every sum has a fixed order (the k order of the MFMA chain, steps in sequence), plain stores, no floating-point atomics,
// no scratch.  Resource usage (-Rpass-analysis=kernel-resource-usage): 102 / 116 VGPRs (strided / x axis) + 32 AGPRs, 37 888 B LDS, no scratch,
// 3 waves per SIMD; measured 40 .. 68 us per contraction at 128^3, 284 us per application (profiles/r15_sm_direct.txt).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>
#include "ctx.hpp"
#include "kernels.hpp"
#include "sm_direct_host.hpp"

namespace ifem {

constexpr int kSmdTI = 64, kSmdTJ = 64, kSmdKC = 32, kSmdPitchA = kSmdKC + 2, kSmdPitchW = kSmdTJ + 16;
enum { SMD_GATHER = 1, SMD_SCATTER = 2, SMD_SCALE = 4 };
using smd_f64x4 = __attribute__((ext_vector_type(4))) double;

struct SmdPass {
  int n, npad;        // nodes of the contracted axis, rounded up to 16
  int64_t J;          // columns per batch
  int64_t sk, sj, so; // lattice strides of the contracted index, the column and the batch
  int nx, ny, dim;    // (the scale decodes a lattice position)
};

template <bool XAXIS, int FLAGS>
__global__ __launch_bounds__(256) void k_smd_contract(SmdPass P, const double *__restrict__ A, const double *__restrict__ in, double *__restrict__ out,
                                                      const int32_t *__restrict__ idx, const double *__restrict__ lx, const double *__restrict__ ly,
                                                      const double *__restrict__ lz) {
  __shared__ double As[kSmdTI * kSmdPitchA];
  __shared__ double Ws[kSmdKC * kSmdPitchW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t j0 = int64_t(blockIdx.x) * kSmdTJ, base = int64_t(blockIdx.z) * P.so;
  const int i0 = blockIdx.y * kSmdTI;
  // staging maps: the A panel by 32 consecutive k per row; the input tile along its contiguous lattice index
  const int a_k = tid & 31, a_i = tid >> 5;                      // rows a_i + 8 r
  const int w_k = XAXIS ? tid & 31 : tid >> 6, w_j = XAXIS ? tid >> 5 : tid & 63; // XAXIS: columns w_j + 8 r; else rows w_k + 4 r
  double ra[8], rw[8];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int i = i0 + a_i + 8 * r, k = k0 + a_k;
      ra[r] = (i < P.npad && k < P.npad) ? A[int64_t(i) * P.npad + k] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int k = k0 + (XAXIS ? w_k : w_k + 4 * r);
      const int64_t j = j0 + (XAXIS ? w_j + 8 * r : w_j);
      double v = 0.0;
      if (k < P.n && j < P.J) {
        const int64_t pos = base + int64_t(k) * P.sk + j * P.sj;
        v = (FLAGS & SMD_GATHER) ? in[idx[pos]] : in[pos];
      }
      rw[r] = v;
    }
  };
  smd_f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = smd_f64x4{0.0, 0.0, 0.0, 0.0};
  const int fr = lane & 15, fq = lane >> 4;
  const bool wave_on = XAXIS || i0 + 16 * w < P.npad; // (wave-uniform)
  fetch(0);
  for (int k0 = 0; k0 < P.npad; k0 += kSmdKC) {
#pragma unroll
    for (int r = 0; r < 8; ++r) As[(a_i + 8 * r) * kSmdPitchA + a_k] = ra[r];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (XAXIS) Ws[w_k * kSmdPitchW + w_j + 8 * r] = rw[r];
      else Ws[(w_k + 4 * r) * kSmdPitchW + w_j] = rw[r];
    }
    __syncthreads();
    if (k0 + kSmdKC < P.npad) fetch(k0 + kSmdKC);
    if (wave_on) {
      const int nk = min(kSmdKC, P.npad - k0) / 4; // 4 or 8: npad is a multiple of 16
      for (int kg = 0; kg < nk; kg += 4)
#pragma unroll
      for (int ku = 0; ku < 4; ++ku) {
        const int kq = 4 * (kg + ku) + fq;
        if (XAXIS) { // (the 16-row sub-tiles of A beyond the padded axis are staged as zeros)
          const double a = Ws[kq * kSmdPitchW + 16 * w + fr];
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, As[(16 * t + fr) * kSmdPitchA + kq], acc[t], 0, 0, 0);
        } else {
          const double a = As[(16 * w + fr) * kSmdPitchA + kq];
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ws[kq * kSmdPitchW + 16 * t + fr], acc[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  if (!wave_on) return;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = XAXIS ? i0 + 16 * t + fr : i0 + 16 * w + fq + 4 * r;
      const int64_t j = XAXIS ? j0 + 16 * w + fq + 4 * r : j0 + 16 * t + fr;
      if (i >= P.n || j >= P.J) continue;
      const int64_t pos = base + int64_t(i) * P.sk + j * P.sj;
      double v = acc[t][r];
      if (FLAGS & SMD_SCALE) {
        const int px = int(pos % P.nx), py = int((pos / P.nx) % P.ny);
        double l = lx[px] + ly[py];
        if (P.dim == 3) l += lz[pos / (int64_t(P.nx) * P.ny)];
        v *= 1.0 / l;
      }
      if (FLAGS & SMD_SCATTER) out[idx[pos]] = v; else out[pos] = v;
    }
}

// out[c] = constrained dofs of velocity component c (integer atomics: the order does not enter), out[3 + (c * 3 + a) * 2 + s] = the flag of
// component c at the centre node of face s of axis a (fc: their lattice points); the device form of sm_direct_host.cpp::smd_masks_scan
struct SmdFaces { int64_t p[18]; };
__global__ __launch_bounds__(256) void k_smd_masks(int dim, int64_t n_nodes, const uint8_t *__restrict__ is_c, const int32_t *__restrict__ nol, SmdFaces fc,
                                                   unsigned long long *__restrict__ out) {
  unsigned long long cnt[3] = {0, 0, 0};
  for (int64_t nd = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; nd < n_nodes; nd += int64_t(gridDim.x) * blockDim.x)
    for (int c = 0; c < dim; ++c) cnt[c] += is_c[nd * dim + c] ? 1 : 0;
  for (int c = 0; c < dim; ++c) {
    for (int off = 32; off > 0; off >>= 1) cnt[c] += __shfl_down(cnt[c], off);
    if ((threadIdx.x & 63) == 0 && cnt[c]) atomicAdd(out + c, cnt[c]);
  }
  if (blockIdx.x == 0 && threadIdx.x < 18) {
    const int c = threadIdx.x / 6, a = (threadIdx.x / 2) % 3;
    out[3 + threadIdx.x] = (c < dim && a < dim) ? (is_c[int64_t(nol[fc.p[threadIdx.x]]) * dim + c] ? 1 : 0) : 0;
  }
}

// ---- host drivers

template <bool XAXIS, int FLAGS>
static void smd_launch(ifem_ctx *ctx, const SmdPass &P, int64_t batches, const double *A, const double *in, double *out) {
  const SmDirect &D = ctx->sm_direct;
  const dim3 g(unsigned((P.J + kSmdTJ - 1) / kSmdTJ), unsigned((P.npad + kSmdTI - 1) / kSmdTI), unsigned(batches));
  hipLaunchKernelGGL((k_smd_contract<XAXIS, FLAGS>), g, dim3(256), 0, ctx->stream, P, A, in, out, ctx->p_lattice.node_of_lattice.p, D.lam[0].p, D.lam[1].p,
                     D.lam[2].p);
}

void sm_direct_apply(ifem_ctx *ctx, const double *b, double *x) {
  SmDirect &D = ctx->sm_direct;
  if (!D.w0.p || !D.Q[0].p) throw Error(IFEM_E_BADPARAM, "sm_direct_apply: the context has no fast-diagonalisation factors");
  const int dim = ctx->dim;
  const PLattice &L = ctx->p_lattice;
  const int nx = L.n[0], ny = L.n[1], nz = dim == 3 ? L.n[2] : 1;
  const int64_t N = int64_t(nx) * ny * nz;
  double flops = 0, bytes = 8.0 * double(N);
  for (int a = 0; a < dim; ++a) {
    flops += 4.0 * D.npad[a] * double(N);
    bytes += 2.0 * double(N) * 8.0 * ((D.npad[a] + kSmdTI - 1) / kSmdTI + 1);
  }
  KScope ks(ctx, IFEM_KC_SPMV_SM, bytes, flops);
  const SmdPass X{nx, D.npad[0], int64_t(ny) * nz, 1, nx, 0, nx, ny, dim};
  const SmdPass Y{ny, D.npad[1], nx, nx, 1, int64_t(nx) * ny, nx, ny, dim};
  const SmdPass Z{nz, D.npad[2], int64_t(nx) * ny, int64_t(nx) * ny, 1, 0, nx, ny, dim};
  double *w0 = D.w0.p, *w1 = D.w1.p;
  smd_launch<true, SMD_GATHER>(ctx, X, 1, D.Qt[0].p, b, w0);
  if (dim == 3) {
    smd_launch<false, 0>(ctx, Y, nz, D.Qt[1].p, w0, w1);
    smd_launch<false, SMD_SCALE>(ctx, Z, 1, D.Qt[2].p, w1, w0);
    smd_launch<false, 0>(ctx, Z, 1, D.Q[2].p, w0, w1);
    smd_launch<false, 0>(ctx, Y, nz, D.Q[1].p, w1, w0);
  } else {
    smd_launch<false, SMD_SCALE>(ctx, Y, 1, D.Qt[1].p, w0, w1);
    smd_launch<false, 0>(ctx, Y, 1, D.Q[1].p, w1, w0);
  }
  smd_launch<true, SMD_SCATTER>(ctx, X, 1, D.Q[0].p, w0, x);
}

// masks of the constraint set the assembly used; false: the constrained dofs are not whole faces, or a face constrains one tangential component only
static bool smd_read_masks(ifem_ctx *ctx, int mask[3][3]) {
  SmDirect &D = ctx->sm_direct;
  const ULattice &U = ctx->u_lattice;
  const int dim = ctx->dim, cs = ctx->asm_constraint_set;
  int face[3][3][2] = {};
  int64_t count[3] = {0, 0, 0};
  if (ctx->has_c[cs]) {
    hipStream_t s = ctx->stream;
    if (D.scan.n != 21) D.scan.alloc(21);
    IFEM_HIP_CHECK(hipMemsetAsync(D.scan.p, 0, 21 * sizeof(int64_t), s));
    SmdFaces fc{};
    for (int c = 0; c < 3; ++c)
      for (int a = 0; a < 3; ++a)
        for (int sd = 0; sd < 2; ++sd) fc.p[(c * 3 + a) * 2 + sd] = a < dim ? smd_face_centre(dim, U.n, a, sd) : 0;
    const int64_t nn = ctx->nUo;
    hipLaunchKernelGGL(k_smd_masks, dim3(unsigned(std::min<int64_t>((nn + 255) / 256, 2048))), dim3(256), 0, s, dim, nn, ctx->is_c[cs].p, U.node_of_lattice.p, fc,
                       (unsigned long long *)D.scan.p);
    int64_t h[21];
    IFEM_HIP_CHECK(hipMemcpyAsync(h, D.scan.p, sizeof(h), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
    IFEM_HIP_CHECK(hipGetLastError());
    for (int c = 0; c < 3; ++c) {
      count[c] = h[c];
      for (int a = 0; a < 3; ++a)
        for (int sd = 0; sd < 2; ++sd) face[c][a][sd] = int(h[3 + (c * 3 + a) * 2 + sd]);
    }
  }
  return smd_masks_decide(dim, U.n, face, count, mask);
}

// x = direct(e) against the context's own fp64 product of the present S_m, on the device
static bool smd_probe(ifem_ctx *ctx, double *err_out) {
  const int64_t n = ctx->nPo;
  const size_t un = size_t(n);
  DBuf<double> de, dx, dy;
  de.alloc(un); dx.alloc(un); dy.alloc(un);
  vec_rough(ctx, n, 0xFD5EED, de.p); // a fixed hash of the index: the same probe on every run
  IFEM_HIP_CHECK(hipMemsetAsync(dx.p, 0xff, un * sizeof(double), ctx->stream)); // NaN: an entry nobody produced shows
  sm_direct_apply(ctx, de.p, dx.p);
  if (sm_stencil_ready(ctx)) sm_stencil_apply(ctx, dx.p, dy.p);
  else spmv_sm(ctx, dx.p, dy.p, /*use_f32=*/false);
  double emax = 0, err = 0;
  const bool finite = v_probe_diff(ctx, n, de.p, dy.p, &emax, &err) && emax > 0; // dy = S_m x - e
  if (err_out) *err_out = finite ? err / emax : INFINITY;
  return finite && err <= 1e-7 * emax;
}

void sm_direct_setup(ifem_ctx *ctx, int verbose) {
  SmDirect &D = ctx->sm_direct;
  if (D.failed || D.version == ctx->sm_version) return;
  D.version = ctx->sm_version;
  D.ready = false;
  if (ctx->mg_fine) return; // a multigrid coarse level never builds factors
  const int dim = ctx->dim;
  const char *why = nullptr;
  int mask[3][3] = {};
  if (ctx->halo.nranks > 1) why = "several ranks";
  else if (!ctx->sm_valid || ctx->Sm.n_rows == 0 || ctx->Sm.n_rows != ctx->nPo) why = "no explicit S_m";
  else if (ctx->has_app || ctx->bb_stencil.scns) why = "SCnsIM blocks";
  else if (ctx->kv != 2) why = "Q1 velocity";
  else if (!u_lattice_ensure(ctx)) why = "not a full uniform lattice on one rank";
  else if (std::max(ctx->p_lattice.n[0], std::max(ctx->p_lattice.n[1], dim == 3 ? ctx->p_lattice.n[2] : 1)) > kSmdMaxAxis) why = "more than 513 pressure nodes on an axis";
  else if (!smd_read_masks(ctx, mask)) why = "the constrained velocity dofs are not whole faces with coinciding mass-like factors";
  hipStream_t s = ctx->stream;
  if (!why) {
    const PLattice &L = ctx->p_lattice;
    const auto t0 = std::chrono::steady_clock::now();
    bool built = false;
    for (int a = 0; a < dim && !why; ++a) {
      const int other = mask[a == 0 ? 1 : 0][a], nc = L.n[a] - 1;
      if (D.Q[a].p && D.key_n[a] == nc && D.key_h[a] == ctx->mf_h[a] && D.key_own[a] == mask[a][a] && D.key_other[a] == other) continue;
      D.Q[a].release(); // (the key below is valid only with the tables)
      SmdAxis A;
      const int rc = smd_axis_build(nc, ctx->mf_h[a], mask[a][a], other, A);
      if (rc != SMD_OK) { why = "a mass-like 1D factor is rank-deficient (an axis of one cell with both ends constrained)"; break; }
      D.builds++;
      built = true;
      const int np = A.np, npad = (np + 15) / 16 * 16;
      std::vector<double> q(size_t(npad) * npad, 0.0), qt(size_t(npad) * npad, 0.0);
      for (int i = 0; i < np; ++i)
        for (int j = 0; j < np; ++j) {
          q[size_t(i) * npad + j] = A.Q[size_t(i) * np + j];
          qt[size_t(j) * npad + i] = A.Q[size_t(i) * np + j];
        }
      D.npad[a] = npad;
      D.Qt[a].upload(qt.data(), qt.size(), s);
      D.lam[a].upload(A.lam.data(), A.lam.size(), s);
      D.Q[a].upload(q.data(), q.size(), s);
      IFEM_HIP_CHECK(hipStreamSynchronize(s)); // (q / qt leave scope)
      D.key_n[a] = nc; D.key_h[a] = ctx->mf_h[a]; D.key_own[a] = mask[a][a]; D.key_other[a] = other;
      D.lam_min[a] = *std::min_element(A.lam.begin(), A.lam.end());
      D.lam_max[a] = *std::max_element(A.lam.begin(), A.lam.end());
    }
    if (built) D.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!why) {
      double lo = 0, hi = 0;
      for (int a = 0; a < dim; ++a) { lo += D.lam_min[a]; hi += D.lam_max[a]; }
      if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo > 1e-12 * hi)) why = "the block is singular (enclosed flow)";
    }
    if (!why) {
      if (D.w0.n != size_t(ctx->nPo)) {
        D.w0.alloc(size_t(ctx->nPo), "a work vector of the direct S_m solve");
        D.w1.alloc(size_t(ctx->nPo), "a work vector of the direct S_m solve");
      }
      if (smd_probe(ctx, &D.probe)) D.ready = true;
      else { why = "the direct solve misses the assembled S_m (probe above 1e-7)"; D.failed = true; }
    }
  }
  if (!verbose) return;
  if (why) fprintf(stderr, "[ifem] S_m solve: %s%s: multigrid-preconditioned CG\n", why, D.failed ? " -- from now on" : "");
  else
    fprintf(stderr, "[ifem] S_m solve: fast diagonalisation on the %d x %d x %d lattice, %lld axis eigen-solves so far (last build %.1f ms host), probe max |S_m x - e| / max |e| = %.2e\n",
            ctx->p_lattice.n[0], ctx->p_lattice.n[1], ctx->p_lattice.n[2], (long long)D.builds, D.build_ms, D.probe);
}

} // namespace ifem
