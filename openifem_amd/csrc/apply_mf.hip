// apply_mf.hip -- matrix-free application of the velocity block A_uu of InsIM's Newton matrix:
//   y_(a,c) = sum_q JxW { mu gN_a.g x_c + rho N_a (u.g x_c) + rho/dt N_a x_c + rho N_a x.g u_c + gamma rho d_c N_a div x }
// which is row (a,c) of Ke x summed over the cells (reference: the u-u part of local_matrix, mpi_insim.cpp:263-289, after
// distribute_local_to_global).  Used as the operator of the inner (preconditioner-only) Krylov solve that stands in for
// MUMPS (mpi_insim.cpp:124-127): the assembled block matrix stays the operator of the outer FGMRES.
//
// One wavefront per cell, sum factorisation on the tensor-product element: nodal values -> Gauss points by one 1D
// interpolation per direction, reference gradients by the collocation derivative on the Gauss points (exact: the
// restriction of Q_k to a grid line has degree k and there are k+1 points), the weak form at the quadrature point
// (one lane per point, MappingQ1 Jacobian from the cell vertices), then the transposed passes.  ~10 kFLOP and ~2.3 kB of
// HBM traffic per 3D Q2 cell instead of 40 B per stored block entry (64 entries per row) of the assembled SpMV.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "ctx.hpp"
#include "kernels.hpp"

namespace ifem {

template <typename R>
struct MfTablesT {
  R N[9];  // [q][i]  1D Lagrange shape i (equidistant nodes) at Gauss point q
  R D[9];  // [q][q'] derivative at Gauss point q of the Lagrange polynomial of Gauss point q'
  R xi[3]; // Gauss points on [0,1]
  R w[3];
};
using MfTables = MfTablesT<double>;

// R = arithmetic type of the cell kernel: double for the operator of an outer solve, float for the preconditioner-only
// inner Krylov solve (tolerance 1e-2; its basis is single precision already).  Vectors in HBM stay double either way.
template <typename R, typename XT = double>
struct MfArgsT {
  int64_t n_cells, nUo; // n_cells: one past the last cell of this launch
  int64_t first_cell;   // first cell of this launch
  const double *vcoords;
  const int32_t *cell_unodes;
  const uint8_t *is_c; // constraint flags of the set the matrix was assembled with (local dofs) or nullptr
  const double *eval;  // evaluation point of the assembled matrix, velocity part, ghost-extended
  const XT *x;         // ghost-extended input (float: a level vector of the V-cycle)
  double *y;           // owned rows
  R mu, rho, gamma, inv_dt;
  int xcd;
  R *ycell; // per-cell results of the two-stage scatter
  MfTablesT<R> t;
  R ih[3], vol; // UNI kernels only: 1 / h_d and prod h_d of the level's one axis-aligned box cell (ifem_ctx::mf_h)
};

template <int DIM, int N1>
struct MfGeo {
  static constexpr int NN = (DIM == 2) ? N1 * N1 : N1 * N1 * N1;
  static constexpr int NV = 1 << DIM;
};

// ---------------------------------------------------------------------------------------------------------------
// Half a wavefront (32 lanes) per cell, two cells per wave.  Every 1D pass is an in-register "pencil" operation
// (one lane owns the N1 values of a grid line: N1 LDS reads, N1^2 FMAs against wave-uniform table entries that live in
// SGPRs, N1 LDS writes, in place), the quadrature-point stage runs on 27 of 32 lanes, the trilinear geometry comes
// from 8 monomial coefficients, and the only synchronisation is wave-local (LDS operations of one wave execute in
// order).  ~330 wave instructions per 3D Q2 cell (the first, item-per-lane version of round 1 needed ~1200).
// Round 4 measured a variant with TWO cells per lane in packed arithmetic (v_pk_fma_f32 by construction, four cells per wave trip;
// profiles/r04_valu_rate.txt, r04_mf_packed.txt): 1.97 against 1.75 ms per application at 128^3 -- v_pk_fma_f32 issues in 4.7
// cycles against 4.1 for v_fma_f32 (1.7 x per FMA), but packed multiplies / adds gain nothing (the two-operand forms issue in 2.5
// cycles), the pair needs 195 registers (two waves per SIMD, where every instruction issues ~15 % slower) and 8-byte LDS items.
__device__ inline void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS layout of the nodal / quadrature-point fields of a cell.  The pencil passes touch, per instruction, one entry of every
// (pencil, component) pair with one index fixed; the quadrature-point stage one entry per point with the component fixed.  On 3D
// Q2 the compact layout (component * 27 + i + 3 j + 9 k) puts two lanes of a 32-lane group on one bank in two of the three pass
// directions (29 % of the LDS cycles of rounds 1-3 were conflict cycles, and the LDS array is this kernel's busiest unit).  Entries
// that share a bank must differ in all four indices (i, j, k, component): the cosets of (1,1,1,1) in Z_3^4 are such sets, so entry
// (c; i,j,k) goes to row c (32 entries) at column (i-c) + 3 (j-c) + 9 (k-c), differences mod 3 -- every access pattern of the kernel
// is conflict-free.  Other element types keep the compact layout.
template <int DIM, int N1>
struct MfLay {
  static constexpr int NN = MfGeo<DIM, N1>::NN;
  static constexpr bool SWZ = DIM == 3 && N1 == 3;
  static constexpr int CS = SWZ ? 32 : NN; // entries per component
  static constexpr int SZ = DIM * CS;
  __device__ static int rot(int x) { return x < 0 ? x + N1 : x; }
  __device__ static int off(int c, int i0, int i1, int i2) {
    if constexpr (SWZ) return CS * c + rot(i0 - c) + 3 * rot(i1 - c) + 9 * rot(i2 - c);
    else return CS * c + i0 + N1 * i1 + N1 * N1 * i2;
  }
};

// NF fields per entry: the increment x and (CONV) the evaluation point u side by side, so that one ds_read_b64 (same LDS cycles as
// a ds_read_b32) fetches both
template <typename R, int NF>
struct alignas(sizeof(R) * NF) MfVal { R f[NF]; };

template <int DIM, int N1, typename R, int NF, bool UNI = false>
struct alignas(16) MfCell { // per-cell LDS scratch
  static constexpr int SZ = MfLay<DIM, N1>::SZ;
  MfVal<R, NF> V[SZ]; // nodal values -> values at the Gauss points; then, as R[SZ] over its head, integrand -> nodal result
  MfVal<R, NF> G[SZ]; // one reference-gradient direction at a time; R[SZ] over its head in the transposed passes
  R C[8 * DIM];       // [e][k]: monomial coefficients of the d-linear map
  R X[(1 << DIM) * DIM];
};
// UNI: the geometry is three constants of the launch, nothing of it passes through LDS
template <int DIM, int N1, typename R, int NF>
struct alignas(16) MfCell<DIM, N1, R, NF, true> {
  static constexpr int SZ = MfLay<DIM, N1>::SZ;
  MfVal<R, NF> V[SZ];
  MfVal<R, NF> G[SZ];
};
// what the prefetch carries of the cell's geometry: one vertex coordinate per lane, or nothing
template <bool UNI> struct MfPreGeo { double vc; };
template <> struct MfPreGeo<true> {};

// CONV = false: the evaluation point is zero (InsIMEX matrix: no convective / Newton terms) -- the second field is neither gathered
// nor interpolated
// LIFT = true (uu_lift_mf): the input mask is inverted -- A.x holds the constraint values and enters ONLY where A.is_c is set, so the
// cell results are the columns of the constrained dofs times their values (the K g that distribute_local_to_global moves into the
// right-hand side).  A wave whose two cells touch no constrained dof with a non-zero value stores zeros and moves on (wave-uniform).
// UNI = true (ifem_ctx::mf_uniform: every cell of the context is the same axis-aligned box of edges h): J = diag(h), so J^-1 =
// diag(A.ih) and JxW = A.vol wq are constants of the lane -- no vertex coordinates are loaded, the monomial coefficients, the
// Jacobian, its cofactors and the reciprocal are gone, and the two contractions with J^-1 keep their diagonal term only.  Chosen at
// launch for the whole grid.
template <int DIM, int KV, int WPB, bool CONV, typename R, typename XT, bool LIFT = false, bool UNI = false>
__global__ __launch_bounds__(64 * WPB) void k_apply_uu_mf2(MfArgsT<R, XT> A) {
  constexpr int N1 = KV + 1, NN = MfGeo<DIM, N1>::NN, NV = 1 << DIM, NF = CONV ? 2 : 1;
  constexpr int NP = NN / N1;        // pencils per field and direction
  constexpr int NPL = DIM * NP;      // pencil lanes (one per pencil and component)
  using Lay = MfLay<DIM, N1>;
  using Val = MfVal<R, NF>;
  __shared__ MfCell<DIM, N1, R, NF, UNI> SS[2 * WPB];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
  MfCell<DIM, N1, R, NF, UNI> &S = SS[2 * wave + half];
  R *const Vs = reinterpret_cast<R *>(S.V), *const Gs = reinterpret_cast<R *>(S.G); // single-field views (transposed passes)
  // ---- per-lane roles (fixed for the life of the wave)
  const bool pen_lane = hl < NPL;
  const int comp = pen_lane ? hl / NP : 0, pen = pen_lane ? hl % NP : 0;
  int padr[DIM][N1]; // entry of point i of this lane's pencil in direction d
  {
    const int a = pen % N1, b = pen / N1;
#pragma unroll
    for (int i = 0; i < N1; ++i) {
      if constexpr (DIM == 3) {
        padr[0][i] = Lay::off(comp, i, a, b); padr[1][i] = Lay::off(comp, a, i, b); padr[2][i] = Lay::off(comp, a, b, i);
      } else {
        padr[0][i] = Lay::off(comp, i, pen, 0); padr[1][i] = Lay::off(comp, pen, i, 0);
      }
    }
  }
  const bool q_lane = hl < NN;
  const int q = q_lane ? hl : 0;
  const int qi[3] = {q % N1, (q / N1) % N1, q / (N1 * N1)};
  int qoff[DIM]; // entry of node / quadrature point q, component c
#pragma unroll
  for (int c = 0; c < DIM; ++c) qoff[c] = Lay::off(c, qi[0], qi[1], DIM == 3 ? qi[2] : 0);
  R xi[3] = {0, 0, 0}, wq = 1;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    // select from the wave-uniform tables without dynamic indexing of kernel arguments
    R x_ = A.t.xi[0], w_ = A.t.w[0];
#pragma unroll
    for (int k = 1; k < N1; ++k) { x_ = qi[d] == k ? A.t.xi[k] : x_; w_ = qi[d] == k ? A.t.w[k] : w_; }
    xi[d] = x_; wq *= w_;
  }
  [[maybe_unused]] const R JxW_uni = A.vol * wq; // UNI: the same at this lane's point of every cell

  // every block owns one contiguous range of cell pairs (XCD-aware: neighbouring ranges run on the same XCD)
  const int64_t n_pairs = (A.n_cells - A.first_cell + 1) / 2;
  const int64_t per_block = (n_pairs + gridDim.x - 1) / gridDim.x;
  const int64_t vb = A.xcd ? xcd_swizzle(blockIdx.x, gridDim.x) : blockIdx.x;
  const int64_t p_end = (vb + 1) * per_block < n_pairs ? (vb + 1) * per_block : n_pairs;
  // The gather of a cell is a chain of two dependent HBM accesses (node id, then the nodal values): it is software-
  // pipelined over the cells of the wave -- ids two cells ahead (issued at the top of a cell), values, constraint flags and
  // vertex coordinates one cell ahead (issued after the quadrature-point stage, where few registers are live) -- and
  // everything is kept RAW (double / byte) until it is consumed, so that no conversion forces a wait next to a load.
  const int64_t p_first = vb * per_block + wave;
  // 32-bit index arithmetic in the prefetch (cells * nodes-per-cell and dim * nodes are below 2^31 by the int32 node ids)
  auto cell_of = [&](int64_t pr) { const int64_t c = A.first_cell + 2 * pr + half; return (pr < p_end && c < A.n_cells) ? uint32_t(c) : 0u; };
  struct Pre { XT x[DIM]; double u[DIM]; MfPreGeo<UNI> g; uint8_t f[DIM]; } pre;
  auto load_id = [&](int64_t pr) -> int32_t { return q_lane ? A.cell_unodes[cell_of(pr) * uint32_t(NN) + uint32_t(hl)] : 0; };
  auto load_vals = [&](int64_t pr, int32_t nd, Pre &o) {
    if (q_lane) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        const uint32_t dof = uint32_t(DIM) * uint32_t(nd) + uint32_t(c);
        o.x[c] = A.x[dof];
        if constexpr (CONV) o.u[c] = A.eval[dof];
        o.f[c] = A.is_c ? A.is_c[dof] : uint8_t(0); // one byte per dof: stays in L2
      }
    }
    if constexpr (!UNI) { if (hl < NV * DIM) o.g.vc = A.vcoords[int64_t(cell_of(pr)) * (NV * DIM) + hl]; }
  };
  int32_t nd_ahead = load_id(p_first + WPB);
  load_vals(p_first, load_id(p_first), pre);
  for (int64_t pair = p_first; pair < p_end; pair += WPB) {
    const int64_t cell = A.first_cell + 2 * pair + half;
    const bool active = cell < A.n_cells;
    // ---- gather: this cell's values are in registers; start the id load of the cell after the next
    const Pre cur = pre;
    const int32_t nd_next = nd_ahead;
    nd_ahead = load_id(pair + 2 * WPB);
    if constexpr (LIFT) {
      bool touched = false;
      if (q_lane) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) touched = touched || (cur.f[c] != 0 && cur.x[c] != XT(0));
      }
      if (!__any(touched)) { // no LDS traffic on this path: nothing to order
        load_vals(pair + WPB, nd_next, pre);
        if (active && q_lane) {
#pragma unroll
          for (int c = 0; c < DIM; ++c) A.ycell[cell * (DIM * NN) + hl * DIM + c] = R(0);
        }
        continue;
      }
    }
    if (q_lane) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        Val v;
        if constexpr (LIFT) v.f[0] = cur.f[c] != 0 ? R(cur.x[c]) : R(0);
        else v.f[0] = cur.f[c] != 0 ? R(0) : R(cur.x[c]);
        if constexpr (CONV) v.f[1] = R(cur.u[c]);
        S.V[qoff[c]] = v;
      }
    }
    if constexpr (!UNI) { if (hl < NV * DIM) S.X[hl] = R(cur.g.vc); }
    wsync();
    // monomial coefficients of x(xi) = sum_k C_k prod_{d in k} xi_d:  C_k = sum_{v subset of k} (-1)^{|k|-|v|} X_v
    if constexpr (!UNI) if (hl < NV * DIM) {
      const int k = hl / DIM, e = hl % DIM;
      R acc = 0;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const bool sub = (v & ~k) == 0;
        const int par = __builtin_popcount(k ^ v) & 1;
        const R xv = S.X[v * DIM + e];
        acc += sub ? (par ? -xv : xv) : R(0);
      }
      S.C[e * 8 + k] = acc;
    }
    // ---- nodal values -> Gauss points (both fields of an entry at once), in place
    if (pen_lane) {
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        Val in[N1];
#pragma unroll
        for (int i = 0; i < N1; ++i) in[i] = S.V[padr[d][i]];
#pragma unroll
        for (int o = 0; o < N1; ++o) {
          Val acc;
#pragma unroll
          for (int r = 0; r < NF; ++r) {
            R s = 0;
#pragma unroll
            for (int i = 0; i < N1; ++i) s += A.t.N[o * N1 + i] * in[i].f[r];
            acc.f[r] = s;
          }
          S.V[padr[d][o]] = acc;
        }
        wsync();
      }
    } else {
#pragma unroll
      for (int d = 0; d < DIM; ++d) wsync();
    }
    // ---- geometry at the quadrature point
    [[maybe_unused]] R Ji[DIM * DIM];
    R JxW = 0;
    if constexpr (UNI) JxW = JxW_uni;
    else {
      R J[DIM * DIM];
      if constexpr (DIM == 3) {
        const R e_ = xi[1], z_ = xi[2], x_ = xi[0];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          typedef R R4 __attribute__((ext_vector_type(4)));
          const R4 lo = *reinterpret_cast<const R4 *>(&S.C[e * 8]), hi = *reinterpret_cast<const R4 *>(&S.C[e * 8 + 4]); // wave-uniform addresses: wide broadcast reads
          J[e * 3 + 0] = lo[1] + lo[3] * e_ + hi[1] * z_ + hi[3] * (e_ * z_);
          J[e * 3 + 1] = lo[2] + lo[3] * x_ + hi[2] * z_ + hi[3] * (x_ * z_);
          J[e * 3 + 2] = hi[0] + hi[1] * x_ + hi[2] * e_ + hi[3] * (x_ * e_);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const R c1 = S.C[e * 8 + 1], c2 = S.C[e * 8 + 2], c3 = S.C[e * 8 + 3];
          J[e * 2 + 0] = c1 + c3 * xi[1];
          J[e * 2 + 1] = c2 + c3 * xi[0];
        }
      }
      R det;
      if constexpr (DIM == 2) {
        det = J[0] * J[3] - J[1] * J[2];
        const R r = R(1) / det;
        Ji[0] = J[3] * r; Ji[1] = -J[1] * r; Ji[2] = -J[2] * r; Ji[3] = J[0] * r;
      } else {
        const R c00 = J[4] * J[8] - J[5] * J[7], c01 = J[5] * J[6] - J[3] * J[8], c02 = J[3] * J[7] - J[4] * J[6];
        det = J[0] * c00 + J[1] * c01 + J[2] * c02;
        const R r = R(1) / det;
        Ji[0] = c00 * r; Ji[3] = c01 * r; Ji[6] = c02 * r;
        Ji[1] = (J[2] * J[7] - J[1] * J[8]) * r; Ji[4] = (J[0] * J[8] - J[2] * J[6]) * r; Ji[7] = (J[1] * J[6] - J[0] * J[7]) * r;
        Ji[2] = (J[1] * J[5] - J[2] * J[4]) * r; Ji[5] = (J[2] * J[3] - J[0] * J[5]) * r; Ji[8] = (J[0] * J[4] - J[1] * J[3]) * r;
      }
      JxW = fabs(det) * wq;
    }
    // ---- physical gradients: one reference direction at a time through G
    R gx[DIM][DIM], gu[DIM][DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c)
#pragma unroll
      for (int e = 0; e < DIM; ++e) { gx[c][e] = 0; gu[c][e] = 0; }
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      if (pen_lane) {
        Val in[N1];
#pragma unroll
        for (int i = 0; i < N1; ++i) in[i] = S.V[padr[d][i]];
#pragma unroll
        for (int o = 0; o < N1; ++o) {
          Val acc;
#pragma unroll
          for (int r = 0; r < NF; ++r) {
            R s = 0;
#pragma unroll
            for (int i = 0; i < N1; ++i) s += A.t.D[o * N1 + i] * in[i].f[r];
            acc.f[r] = s;
          }
          S.G[padr[d][o]] = acc;
        }
      }
      wsync();
      if (q_lane) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
          const Val g = S.G[qoff[c]];
          if constexpr (UNI) { // d/dx_d = (1 / h_d) d/dxi_d
            gx[c][d] = A.ih[d] * g.f[0];
            if constexpr (CONV) gu[c][d] = A.ih[d] * g.f[1];
          } else {
#pragma unroll
            for (int e = 0; e < DIM; ++e) gx[c][e] += Ji[d * DIM + e] * g.f[0];
            if constexpr (CONV) {
#pragma unroll
              for (int e = 0; e < DIM; ++e) gu[c][e] += Ji[d * DIM + e] * g.f[1];
            }
          }
        }
      }
      wsync();
    }
    // ---- weak form at the quadrature point
    R That[DIM][DIM]; // [comp][ref dir]
    if (q_lane) {
      R xq[DIM], uq[DIM];
#pragma unroll
      for (int c = 0; c < DIM; ++c) { const Val v = S.V[qoff[c]]; xq[c] = v.f[0]; uq[c] = CONV ? v.f[NF - 1] : R(0); }
      R divx = 0;
#pragma unroll
      for (int c = 0; c < DIM; ++c) divx += gx[c][c];
      R mass[DIM];
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        R conv = 0, newt = 0;
#pragma unroll
        for (int e = 0; e < DIM; ++e) { conv += uq[e] * gx[c][e]; newt += xq[e] * gu[c][e]; }
        mass[c] = JxW * A.rho * (conv + A.inv_dt * xq[c] + newt);
        R tp[DIM];
#pragma unroll
        for (int e = 0; e < DIM; ++e) tp[e] = JxW * (A.mu * gx[c][e] + (e == c ? A.gamma * A.rho * divx : R(0)));
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          if constexpr (UNI) That[c][d] = A.ih[d] * tp[d];
          else {
            R t = 0;
#pragma unroll
            for (int e = 0; e < DIM; ++e) t += Ji[d * DIM + e] * tp[e];
            That[c][d] = t;
          }
        }
      }
      // the integrand goes to the single-field view over the head of V: every paired value of the wave has been read above
      // (the LDS executes one wave's operations in order)
#pragma unroll
      for (int c = 0; c < DIM; ++c) Vs[qoff[c]] = mass[c];
    }
    // ---- the next cell's values: their latency hides behind the transposed passes below
    load_vals(pair + WPB, nd_next, pre);
    // ---- V_c += D_d^T T^_{c,d}, one direction at a time
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      if (q_lane) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) Gs[qoff[c]] = That[c][d];
      }
      wsync();
      if (pen_lane) {
        R t[N1];
#pragma unroll
        for (int i = 0; i < N1; ++i) t[i] = Gs[padr[d][i]];
#pragma unroll
        for (int o = 0; o < N1; ++o) {
          R acc = Vs[padr[d][o]];
#pragma unroll
          for (int i = 0; i < N1; ++i) acc += A.t.D[i * N1 + o] * t[i];
          Vs[padr[d][o]] = acc;
        }
      }
      wsync();
    }
    // ---- transposed interpolation back to the nodes, in place
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      if (pen_lane) {
        R in[N1];
#pragma unroll
        for (int i = 0; i < N1; ++i) in[i] = Vs[padr[d][i]];
#pragma unroll
        for (int o = 0; o < N1; ++o) {
          R acc = 0;
#pragma unroll
          for (int i = 0; i < N1; ++i) acc += A.t.N[i * N1 + o] * in[i];
          Vs[padr[d][o]] = acc;
        }
      }
      wsync();
    }
    // ---- two-stage scatter: plain stores of the cell's result ([node][component]), summed per node by k_mf_gather
    // (atomics-free, deterministic); the DIM stores of a wave fill the same lines
    if (active && q_lane) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) A.ycell[cell * (DIM * NN) + hl * DIM + c] = Vs[qoff[c]];
    }
    wsync();
  }
}

// Constrained rows of the assembled matrix carry only their diagonal: y_r = d_r x_r, d_r recovered from the
// inverse node block (row and column r of the block are zero apart from d_r, so its inverse has 1/d_r there).
// second stage of the atomics-free scatter: y_i = sum over the cells touching node(i) of the cell's local result (fixed
// order: deterministic), constrained rows y_r = d_r x_r as above
// FUSE (the multigrid smoother, solver.hip::mg_uu_smooth): the product t = (A x)_node is not stored but consumed on the
// spot -- fuse.mode 1: xs += x, r -= t (residual update after the coarse correction); mode 2: the Chebyshev step
// xs += x, r -= t, x <- a x + b B r with the inverse node block B (x is the smoother's direction vector and is updated in
// place: the cell kernel that read it has completed, and a thread only touches the entries of its own node).  fuse.first: xs = x
// is stored without reading xs (the first step of a sweep from zero: no memset of xs before it).
// LIFT (uu_lift_mf; x = the constraint values, y = the right-hand side): free rows y_i -= sum, constrained rows y_r = d_r x_r with
// the same d_r as above.
// The kernel: lanes walk the incidence entries FLAT, nodes sum from LDS.  A block is persistent (one resident round of blocks:
// apply_uu_mf_t) and takes every gridDim.x-th chunk of NT consecutive nodes, so that the nodes in flight on the device at any moment are
// neighbours and share the lines of the per-cell results.  The entries of a chunk are contiguous in `inc` (CSR), so its tile of up to
// TILE = NT * EPT entries is read with coalesced 4-byte loads, one DIM-value load of the cell result per LIVE entry (no slot is loaded
// that the sum does not use), and goes to LDS; the chunk's row pointers go to LDS as their low 32 bits (differences are exact below 2^32
// entries per chunk; inc_ptr stays 64-bit).  The vectors of the epilogue are requested between the entries and the cell results, so
// they arrive while the chain row pointer -> entry -> cell result runs.  Then lane t sums the entries of node t from LDS IN THE ORDER OF ITS INCIDENCE LIST, in
// double, and runs the epilogue -- the order (and for R = float every bit of the result) is that of the one-node-per-thread loop this
// replaces.  A chunk with more than TILE entries (any valence: a node's list may span tiles) takes further tiles; EPT = 6 fits the
// chunks of a lexicographically numbered Q2 box (a grid line alternates 8- and 4-cell nodes: 1536 entries).
// Measured and not kept (profiles/r11_mf_gather.txt): a software pipeline over the chunks of a block (cell results one chunk, entries two
// chunks ahead) at EPT = 8 and 6 -- no faster than this form at equal EPT, 30 VGPRs more; one contiguous chunk range per block.
template <typename R>
struct MfGatherGeo {
  static constexpr int NT = 256;                      // threads = nodes of a chunk
  static constexpr int EPT = sizeof(R) == 4 ? 6 : 3;  // entries per lane and tile
  static constexpr int TILE = NT * EPT;
};
inline unsigned mf_gather_chunks(int64_t n_nodes) { return unsigned((n_nodes + MfGatherGeo<float>::NT - 1) / MfGatherGeo<float>::NT); }

template <int DIM, typename R, bool FUSE, typename V, bool LIFT = false>
__global__ __launch_bounds__(MfGatherGeo<R>::NT) void k_mf_gather(int64_t n, int nn, const int64_t *__restrict__ inc_ptr, const int32_t *__restrict__ inc,
                            const R *__restrict__ ycell, const uint8_t *__restrict__ is_c,
                            const double *__restrict__ bjac, const float *__restrict__ bjf, const V *x, double *y, MfFuseT<V> fuse) {
  constexpr int NT = MfGatherGeo<R>::NT, EPT = MfGatherGeo<R>::EPT, TILE = MfGatherGeo<R>::TILE;
  __shared__ R vals[TILE * DIM];
  __shared__ uint32_t rpl[NT + 1];
  const int t = threadIdx.x;
  const int64_t n_nodes = n / DIM, n_chunks = (n_nodes + NT - 1) / NT;
  // entries ts .. ts + TILE of the list [k0, k1): lane t takes ts + j NT + t; -1 marks a slot past the end
  auto load_entries = [&](int64_t k0, int64_t k1, int64_t ts, int32_t (&e)[EPT]) {
    const int64_t m = k1 - k0 - ts;
#pragma unroll
    for (int j = 0; j < EPT; ++j) e[j] = j * NT + t < m ? inc[k0 + ts + j * NT + t] : int32_t(-1);
  };
  auto load_vals = [&](const int32_t (&e)[EPT], R (&v)[EPT][DIM]) {
#pragma unroll
    for (int j = 0; j < EPT; ++j)
      if (e[j] >= 0) {
        const R *src = ycell + int64_t(e[j] >> 5) * (DIM * nn) + (e[j] & 31) * DIM;
#pragma unroll
        for (int c = 0; c < DIM; ++c) v[j][c] = src[c];
      }
  };
  auto stage_vals = [&](const int32_t (&e)[EPT], const R (&v)[EPT][DIM]) {
#pragma unroll
    for (int j = 0; j < EPT; ++j)
      if (e[j] >= 0) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) vals[(j * NT + t) * DIM + c] = v[j][c];
      }
  };
  // entries [lo, hi) of this lane's node that lie in the staged tile [ts, ts + TILE), in list order
  auto sum_tile = [&](uint32_t lo, uint32_t hi, uint32_t ts, double (&s)[DIM]) {
    const uint32_t a = lo > ts ? lo : ts, b = hi < ts + TILE ? hi : ts + TILE;
    for (uint32_t k = a; k < b; ++k) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) s[c] += double(vals[(k - ts) * DIM + c]);
    }
  };

  for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const int64_t nd = ch * NT + t;
    const bool act = nd < n_nodes;
    const int64_t nds = act ? nd : 0; // (inactive lanes read node 0 and store nothing)
    // ---- the chunk's row pointers and its first tile of entries
    const int64_t last = (ch + 1) * NT, k0 = inc_ptr[ch * NT], k1 = inc_ptr[last < n_nodes ? last : n_nodes];
    const uint32_t rp_reg = uint32_t(inc_ptr[nd < n_nodes ? nd : n_nodes]);
    int32_t ent[EPT];
    R v[EPT][DIM];
    load_entries(k0, k1, 0, ent);
    // ---- this chunk's vectors: requested behind the entries, looked at after the sums
    uint8_t fl[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) fl[c] = is_c ? is_c[nds * DIM + c] : uint8_t(0);
    [[maybe_unused]] V xin[DIM], rin[DIM], xsin[DIM];
    [[maybe_unused]] float bjin[DIM * DIM];
    [[maybe_unused]] double yin[DIM];
    if constexpr (FUSE) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        xin[c] = x[nds * DIM + c];
        rin[c] = fuse.r[nds * DIM + c];
        xsin[c] = fuse.first ? V(0) : fuse.xs[nds * DIM + c]; // first: xs is not read (it holds nothing yet)
      }
      if (fuse.mode >= 2) {
#pragma unroll
        for (int e = 0; e < DIM * DIM; ++e) bjin[e] = bjf[nds * DIM * DIM + e];
      }
    } else if constexpr (LIFT) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) yin[c] = y[nds * DIM + c];
    }
    // ---- the cell results of the tile, staged with the row pointers
    load_vals(ent, v);
    stage_vals(ent, v);
    rpl[t] = rp_reg;
    if (t == 0) rpl[NT] = uint32_t(k1);
    __syncthreads();
    // ---- node sums
    double s[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) s[c] = 0;
    const uint32_t lo = rpl[t] - uint32_t(k0), hi = rpl[t + 1] - uint32_t(k0);
    sum_tile(lo, hi, 0, s);
    for (int64_t ts = TILE; ts < k1 - k0; ts += TILE) { // (block-uniform) further tiles of a chunk with more than TILE entries
      __syncthreads();
      int32_t e2[EPT];
      R v2[EPT][DIM];
      load_entries(k0, k1, ts, e2);
      load_vals(e2, v2);
      stage_vals(e2, v2);
      __syncthreads();
      sum_tile(lo, hi, uint32_t(ts), s);
    }
    // ---- epilogue
    if (act) {
      if constexpr (!FUSE) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
          const int64_t i = nd * DIM + c;
          if constexpr (LIFT) y[i] = fl[c] ? x[i] / bjac[nd * DIM * DIM + c * DIM + c] : yin[c] - s[c];
          else y[i] = fl[c] ? x[i] / bjac[nd * DIM * DIM + c * DIM + c] : s[c];
        }
      } else {
        double xv[DIM], rv[DIM], bj[DIM * DIM];
        if (fuse.mode >= 2) {
#pragma unroll
          for (int e = 0; e < DIM * DIM; ++e) bj[e] = double(bjin[e]);
        } else { // mode 1 applies no node block: only the diagonal entry of a constrained row is needed
#pragma unroll
          for (int c = 0; c < DIM; ++c) bj[c * DIM + c] = fl[c] ? double(bjf[nd * DIM * DIM + c * DIM + c]) : 1.0;
        }
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
          const int64_t i = nd * DIM + c;
          xv[c] = double(xin[c]);
          const double tt = fl[c] ? xv[c] / bj[c * DIM + c] : s[c];
          rv[c] = double(rin[c]) - tt;
          fuse.xs[i] = V(double(xsin[c]) + xv[c]);
          fuse.r[i] = V(rv[c]);
        }
        if (fuse.mode >= 2) {
          const double a = fuse.mode == 2 ? fuse.a : 0.0;
#pragma unroll
          for (int c = 0; c < DIM; ++c) {
            double z = 0;
#pragma unroll
            for (int j = 0; j < DIM; ++j) z += bj[c * DIM + j] * rv[j];
            fuse.d[nd * DIM + c] = V(a * xv[c] + fuse.b * z);
          }
        }
      }
    }
    __syncthreads(); // the next chunk overwrites vals and rpl
  }
}

template <typename R>
static void mf_tables_to(MfTablesT<R> &o, const MfTables &t) {
  for (int i = 0; i < 9; ++i) { o.N[i] = R(t.N[i]); o.D[i] = R(t.D[i]); }
  for (int i = 0; i < 3; ++i) { o.xi[i] = R(t.xi[i]); o.w[i] = R(t.w[i]); }
}

static void mf_tables(MfTables &t, int kv) {
  const int n1 = kv + 1;
  std::memset(&t, 0, sizeof(t));
  if (n1 == 2) {
    const double a = 0.5 / std::sqrt(3.0);
    t.xi[0] = 0.5 - a; t.xi[1] = 0.5 + a; t.w[0] = t.w[1] = 0.5;
  } else {
    const double a = 0.5 * std::sqrt(0.6);
    t.xi[0] = 0.5 - a; t.xi[1] = 0.5; t.xi[2] = 0.5 + a;
    t.w[0] = t.w[2] = 5.0 / 18.0; t.w[1] = 8.0 / 18.0;
  }
  for (int q = 0; q < n1; ++q)
    for (int i = 0; i < n1; ++i) {
      double v = 1; // Lagrange shape i on the equidistant nodes j/kv
      for (int j = 0; j < n1; ++j)
        if (j != i) v *= (t.xi[q] - double(j) / kv) / (double(i) / kv - double(j) / kv);
      t.N[q * n1 + i] = v;
      double d = 0; // derivative at xi_q of the Lagrange polynomial of Gauss point i
      for (int k = 0; k < n1; ++k) {
        if (k == i) continue;
        double p = 1.0 / (t.xi[i] - t.xi[k]);
        for (int j = 0; j < n1; ++j)
          if (j != i && j != k) p *= (t.xi[q] - t.xi[j]) / (t.xi[i] - t.xi[j]);
        d += p;
      }
      t.D[q * n1 + i] = d;
    }
}

template <typename R, typename XT, bool LIFT = false>
static void apply_uu_mf_t(ifem_ctx *ctx, const XT *xu, double *yu, const MfFuseT<XT> *fuse, int part) {
  if (!ctx->mf_valid) throw Error(IFEM_E_BADPARAM, "matrix-free A_uu: no assembled state (call ifem_ins_assemble first)");
  const int64_t n = int64_t(ctx->dim) * ctx->nUo;
  hipStream_t s = ctx->stream;
  MfArgsT<R, XT> a{};
  // cell range of this launch; with the interior-first tables (several ranks) every part uses them, part 0 included
  if (part != 0 && ctx->mf_n_interior < 0) throw Error(IFEM_E_BADPARAM, "matrix-free A_uu: cell split not built");
  const bool perm = ctx->mf_n_interior >= 0;
  a.first_cell = part == 2 ? ctx->mf_n_interior : 0;
  a.n_cells = part == 1 ? ctx->mf_n_interior : ctx->n_cells;
  a.nUo = ctx->nUo;
  a.vcoords = perm ? ctx->mf_vcoords.p : ctx->vcoords.p; a.cell_unodes = perm ? ctx->mf_cell_unodes.p : ctx->cell_unodes.p;
  a.is_c = ctx->has_c[ctx->asm_constraint_set] ? ctx->is_c[ctx->asm_constraint_set].p : nullptr;
  a.eval = ctx->mf_eval.p; a.x = xu; a.y = yu;
  a.mu = R(ctx->mf_params.viscosity); a.rho = R(ctx->mf_params.rho); a.gamma = R(ctx->mf_params.grad_div);
  a.inv_dt = R(1.0 / ctx->mf_params.dt);
  { MfTables t; mf_tables(t, ctx->kv); mf_tables_to(a.t, t); }
  a.xcd = ctx->tune.xcd_swizzle;
  const bool time_it = ctx->profile && !LIFT; // (the lift runs inside an assembly, whose own timing owns the two events)
  if (ctx->n_cells >= (int64_t(1) << 26) || ctx->nu > 32) throw Error(IFEM_E_BADPARAM, "matrix-free A_uu: incidence entries hold 26 cell bits and 5 node bits");
  if (ctx->uinc.n_rows == 0 && ctx->nUo) build_incidence(ctx);
  const size_t need = size_t(ctx->n_cells) * ctx->dim * ctx->nu; // in doubles: the float variant uses half of it
  if (ctx->mf_ycell.n < need) ctx->mf_ycell.alloc(need);
  a.ycell = reinterpret_cast<R *>(ctx->mf_ycell.p);
  if (time_it) IFEM_HIP_CHECK(hipEventRecord(ctx->ev0, s)); // the cell kernel alone (what rocprofv3 reports for it)
  constexpr int WPB = 4;
  const dim3 block(64 * WPB);
  const int64_t n_pairs = (a.n_cells - a.first_cell + 1) / 2;
  const bool conv = !ctx->mf_noconv;
  // one axis-aligned box cell on the whole context (setup.hip::detect_uniform_cells): the constant-geometry kernels
  const bool uni = mf_takes_uniform(ctx);
  if (uni) {
    double vol = 1;
    for (int d = 0; d < ctx->dim; ++d) { a.ih[d] = R(1.0 / ctx->mf_h[d]); vol *= ctx->mf_h[d]; }
    a.vol = R(vol);
  }
  // every block walks one contiguous range of cell pairs: the grid is a whole number of resident rounds (4 per CU slot)
  // so that no round runs partly empty
  auto grid_for_kernel = [&](const void *fn) {
    int per_cu = 0, dev = 0, cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * WPB, 0) != hipSuccess || per_cu < 1) per_cu = 6;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return unsigned(cus) * unsigned(per_cu) * 4u;
  };
  const unsigned g_all = unsigned(std::min<int64_t>((n_pairs + WPB - 1) / WPB, int64_t(1) << 30));
#define IFEM_MF2_(D, K, C, U)                                                                                          \
  { static const unsigned cap = grid_for_kernel(reinterpret_cast<const void *>(&k_apply_uu_mf2<D, K, WPB, C, R, XT, LIFT, U>)); \
    hipLaunchKernelGGL((k_apply_uu_mf2<D, K, WPB, C, R, XT, LIFT, U>), dim3(std::min(cap, g_all)), block, 0, s, a); }
#define IFEM_MF2(D, K)                                                                                                 \
  { if (conv) { if (uni) IFEM_MF2_(D, K, true, true) else IFEM_MF2_(D, K, true, false) }                                \
    else { if (uni) IFEM_MF2_(D, K, false, true) else IFEM_MF2_(D, K, false, false) } }
  if (n_pairs > 0) {
    // algorithmic traffic of the cell kernel: x, evaluation point (fp64 in HBM), constraint flags once per entry,
    // the per-cell results once, vertex coordinates (general kernels only) and node ids per cell; flops of the sum-factorised passes + the point stage
    const int64_t nc = a.n_cells - a.first_cell;
    const int d = ctx->dim, n1 = ctx->kv + 1, npc = 1 << d;
    const double share = ctx->n_cells > 0 ? double(nc) / double(ctx->n_cells) : 0.0;
    const double passes = double((2 * d) * d * ctx->nu * n1 * 2 * 2 + d * d * ctx->nu * n1 * 2 * 2);
    KScope ks(ctx, IFEM_KC_MF_CELL, share * double(n) * (sizeof(XT) + 8 + 1) + double(nc) * ((uni ? 0 : npc * d * 8) + ctx->nu * 4 + ctx->nu * d * sizeof(R)),
              double(nc) * (passes + ctx->nu * 190.0));
    if (ctx->dim == 3 && ctx->kv == 2) IFEM_MF2(3, 2)
    else if (ctx->dim == 3) IFEM_MF2(3, 1)
    else if (ctx->kv == 2) IFEM_MF2(2, 2)
    else IFEM_MF2(2, 1)
  }
#undef IFEM_MF2
#undef IFEM_MF2_
  if (part == 1) return; // the node gather follows the boundary cells
  if (time_it) IFEM_HIP_CHECK(hipEventRecord(ctx->ev1, s));
  const MfFuseT<XT> f0 = fuse ? *fuse : MfFuseT<XT>{};
  // node gather: the per-cell results and the incidence entries once, the node's row pointer; fused form: the inverse node block
  // (single precision) and the smoother's vectors (mode 1: xs, r read + written, x read; modes 2 / 3: d written too)
  // (fuse->first: xs is not read; mode 1 reads no node block)
  // (the row pointers are read once per node; the chunk bounds, one more 8-byte read per 256 nodes, are not counted)
  const double per_node = ctx->dim * double(sizeof(XT)) * (fuse ? (fuse->mode >= 2 ? 6.0 : 5.0) - (fuse->first ? 1.0 : 0.0) : 2.0) +
                          (fuse && fuse->mode >= 2 ? 4.0 * ctx->dim * ctx->dim : 0.0) + 8.0 + ctx->dim;
  KScope ksg(ctx, IFEM_KC_MF_GATHER, double(ctx->n_cells) * ctx->nu * (ctx->dim * sizeof(R) + 4.0) + double(ctx->nUo) * per_node);
  // persistent blocks: one resident round of the device, at most one block per chunk
  const unsigned g_chunks = std::max(1u, mf_gather_chunks(n / ctx->dim));
  const unsigned g_cap = ctx->mf_gather_block_cap ? std::min(ctx->mf_gather_block_cap, g_chunks) : g_chunks;
#define IFEM_MFG(D, F)                                                                                                 \
  { static const unsigned resident = grid_for_kernel(reinterpret_cast<const void *>(&k_mf_gather<D, R, F, XT, LIFT>)) / 4u; \
    const unsigned g = std::min(resident, g_cap);                                                                       \
    ctx->mf_gather_geo[0] = g_chunks; ctx->mf_gather_geo[1] = g;                                                        \
    hipLaunchKernelGGL((k_mf_gather<D, R, F, XT, LIFT>), dim3(g), dim3(MfGatherGeo<R>::NT), 0, s, n, ctx->nu, ctx->uinc.rowptr.p, \
                       ctx->uinc.col.p, a.ycell, a.is_c, ctx->bjac.p, fuse ? bjac_f32_ptr(ctx) : nullptr, xu, yu, f0); }
  if (ctx->dim == 3) { if (fuse) IFEM_MFG(3, true) else IFEM_MFG(3, false) }
  else { if (fuse) IFEM_MFG(2, true) else IFEM_MFG(2, false) }
#undef IFEM_MFG
  if (time_it) {
    IFEM_HIP_CHECK(hipEventSynchronize(ctx->ev1));
    float ms = 0;
    IFEM_HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->mf_ms_total += ms;
    ctx->timing.mf_calls++;
  }
}

// single = true: single-precision cell arithmetic (the inner, preconditioner-only solve); ifem_tuning::mf_f32 = 0 forces double
void apply_uu_mf(ifem_ctx *ctx, const double *xu, double *yu, bool single, const MfFuse *fuse, int part) {
  if (single && ctx->tune.mf_f32) apply_uu_mf_t<float, double>(ctx, xu, yu, fuse, part);
  else apply_uu_mf_t<double, double>(ctx, xu, yu, fuse, part);
}

// the lift vector g (ghost-extended): the constraint values on the constrained dofs of the set, zero elsewhere
__global__ void k_lift_vector(int64_t n, const uint8_t *__restrict__ is_c, const double *__restrict__ cval, double *__restrict__ g) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) g[i] = is_c[i] ? cval[i] : 0.0;
}

// Inhomogeneity lift of a stored_uu = 0 assembly (assemble.hip), on the state that assembly just recorded (mf_eval, mf_params,
// mf_noconv, asm_constraint_set) and after its uu_block_diag_mf: with g = the values of the active constraint set on its dofs,
//   velocity rows:  b_free -= (A_uu[free, constrained] g),   b_r = d_r g_r   (cell kernel + node gather with the mask inverted)
//   pressure rows:  b_p   -= B0[:, constrained u] g           (the unconstrained B of the geometry cache on the masked vector)
// which is what distribute_local_to_global leaves in the right-hand side of the stored assembly.  Pressure dofs cannot be
// constrained (ifem_set_constraints refuses them), so there is no B^T half.  The constraint arrays cover the local dofs, ghosts
// included: the lift vector needs no exchange.
void uu_lift_mf(ifem_ctx *ctx) {
  const int w = ctx->asm_constraint_set;
  if (!ctx->has_c[w]) return;
  const double *B0 = unconstrained_blocks(ctx).B0.p;
  double *rhs = ctx->vec[IFEM_VEC_RHS].p;
  apply_uu_mf_t<double, double, true>(ctx, ctx->cval[w].p, rhs, nullptr, 0);
  const int64_t nul = int64_t(ctx->dim) * ctx->nUl, npo = ctx->nPo;
  if (!npo) return;
  if ((int64_t)ctx->mf_lift.n != nul + npo) ctx->mf_lift.alloc(size_t(nul + npo));
  double *g = ctx->mf_lift.p, *bp = g + nul;
  if (nul) hipLaunchKernelGGL(k_lift_vector, dim3(unsigned(std::min<int64_t>((nul + 255) / 256, 4096))), dim3(256), 0, ctx->stream, nul, ctx->is_c[w].p, ctx->cval[w].p, g);
  spmv_b(ctx, g, bp, 0, B0);
  v_axpy(ctx, npo, -1.0, bp, rhs + int64_t(ctx->dim) * ctx->nUo);
}

void apply_uu_mf_f32in(ifem_ctx *ctx, const float *xu, double *yu, int part) {
  apply_uu_mf_t<float, float>(ctx, xu, yu, nullptr, part);
}

void apply_uu_mf_f32v(ifem_ctx *ctx, const float *xu, const MfFuseT<float> *fuse, int part) {
  if (!fuse) throw Error(IFEM_E_BADPARAM, "apply_uu_mf_f32v: the fused form only");
  apply_uu_mf_t<float, float>(ctx, xu, nullptr, fuse, part);
}

} // namespace ifem
