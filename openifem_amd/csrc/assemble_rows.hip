// assemble_rows.hip -- A_uu of the 3D Q2/Q1 element on uniform box meshes, assembled by ROW OWNERS: the transpose of assemble3.hip's loop.
//
// assemble3.hip lets one wavefront integrate one cell and add its 27 x 27 blocks to rows it shares with up to 7 other cells: 871 atomic
// requests per cell on an array that has to be zero before.  Here one wavefront owns the at most 8 lattice nodes of an owner
// (assemble_rows.hpp) and integrates, for each of their rows, the contribution of every cell that touches the row: 27 (row node, cell) pairs
// with the 27 column nodes of the pair's cell -- the shape of the one-cell contraction.  Nobody else writes these rows: each one is summed
// in an LDS image of its memory and leaves once, complete, as plain contiguous stores.  No atomics on A_uu, no zero fill, and the same
// bits on every run.
//
// What makes the 16 rows of one MFMA come from different cells: on a uniform box (ifem_ctx::mf_uniform) J^-1 = diag(1 / h) and
// JxW = prod(h) w_q are launch constants, so the B operand (gradient or value of the column node) is the same for every cell; only the
// point data rho JxW u (3) and rho JxW grad u + rho/dt JxW (9) differ per row.  The cell kernel computes them anyway in the launch that
// integrates the right-hand side (AsmArgs::pd, 27 x 12 doubles per cell, one definition of their scaling).
//
// For the same reason the viscous and the grad-div term (and the mass term of the IMEX matrix) are the same 27 x 27 x 9 numbers in every
// cell: a small kernel tabulates them ahead of every launch (k_rows_const, 64.5 KB, L2) and the accumulators of a contraction start
// from the table rows of their pairs.  What is left to contract is the convective and the Newton term: 336 of the 588 MFMAs of the
// one-cell contraction, and nothing at all for the IMEX matrix.
//
// The point data of a K-step (4 points of the owner's 8 cells, 3 KB) are loaded once by the wave, one K-step ahead, and handed to the
// lanes through LDS, in the room of the row image, which is dead while a contraction runs; the local right-hand sides of the owner's
// cells come into LDS with the block positions in the round of loads before the first contraction.  (Handing every XCD one contiguous
// range of owners, ctx.hpp::xcd_swizzle, measured 0.4 ms of 70 at 128^3, inside the run-to-run spread: the owners keep the block order.)
//
// Constraints: distribute_local_to_global(..., true) as assemble3.hip::row_tile applies it, per (row, cell) contribution BEFORE it is
// added to the image.  The right-hand side entries of an owned node belong to this wavefront: the terms of its constrained rows and
// columns are summed in a fixed order and added with a plain read-add-write, after the cell launch on the same stream.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "assemble_common.hpp"
#include "assemble_rows.hpp"

namespace ifem {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) double gdouble; // global address space: global_store, not the flat form
typedef __attribute__((address_space(1))) d2 gd2;

struct RowArgs {
  int64_t n_owners;
  int n[3];                       // cells per axis
  const int32_t *node_of_lattice; // ULattice
  const int32_t *cell_at;         // cell at i_x + n_x (i_y + n_y i_z)
  const uint16_t *posUU;          // [cell][row a][column b]: position of the block in its row
  const int64_t *rp_uu;
  double *v_uu, *rhs;
  const uint8_t *is_c;
  const double *cval;
  const double *pd, *fe;          // point data [cell][27][12] and local right-hand sides [cell][96] of the cell launch
  const int32_t *pnode_of_lattice; // PLattice: the pressure node of owner (i, j, k)
  int64_t p_off_c, p_off_rhs;     // first pressure entry of the constraint arrays / of rhs
  const Tabs3 *tabs3;
  const double *k0;               // the constant terms of the element matrix, [a 28][e 9][b 32] (k_rows_const)
  double ih[3], vol;
  double mu, rho, gamma, inv_dt;
  int use_inhom, imex;
};

// per-owner LDS of one wavefront
struct alignas(16) RowWave {
  static constexpr int IMG = 1128; // the longest row (125 blocks of 9) + its alignment double, rounded to 16 bytes
  // The staged point data of a contraction share the room of the row image: the image is dead while a contraction runs (every node_rows
  // ends behind a wsync2 after its stores have read the image, contract<1> starts after that, and contract<0> before the first image).
  // The other way round nothing stands between the last reads of pq in K-step 6 and the zeroing of the next image but program order:
  // the LDS operations of one wave execute in order, and both go through this union, so the compiler cannot tell them apart and move
  // one past the other.  Whoever gives the two members separate, restrict-qualified paths owes the end of contract a wsync2.
  union {
    double img[IMG];
    d2 pq[2][8][24];   // [K-step parity][cell slot = cell bits][points 4 ks .. 4 ks + 3][rwu 3 | gqs 9], in pairs of doubles
  };
  double fe[27 * 3 + 8]; // local right-hand sides of the pairs' cells: velocity [pair][c], then the vertex's pressure entry of cell slot 0..7
  double part[4 * 3];  // right-hand side terms of the row groups of one node
  int64_t rs[8];       // first block of the rows of the owner's nodes (index: node bits), and their lengths in blocks
  int32_t len[8];
  int32_t nb[125];     // nodes of the 5^3 lattice neighbourhood (rows::nb_point), -1 outside
  int32_t pcell[32];   // cell of pair p, -1: none (domain face, padding)
  uint8_t cm[128];     // constraint flags of the neighbourhood's nodes, bit c = component c
  uint16_t pos[27 * 27 + 7]; // [pair][column]: position of the block in its row (ifem_ctx::posUU of the pair's cell and local row)
  uint8_t pa[32];      // local index of the pair's row node in its cell, 27 (a zero row of the tile) without a cell
  uint8_t pcb[32];     // cell bits of pair p = its cell slot: the pair's cell is pcell[pcb[p]], the cell of the vertex pair with these bits
};

struct RowAcc {
  d4 acc0[9], acc1[9], sac0, sac1;
};

// The rows r in [R0, R0 + NR) of lanes g in [G0, G0 + NG) of row tile TI all belong to ONE node: sum them in the image, store the row.
template <int TI, int R0, int NR, int G0, int NG>
__device__ __forceinline__ void node_rows(const RowArgs &A, RowWave &S, const RowAcc &R, const int lane, const bool any_c) {
  constexpr rows::Pair P0 = rows::pair_of(16 * TI + G0 + 4 * R0);
  const int node = S.nb[rows::nb_of_node(P0.nd)]; // wave-uniform
  if (node < 0) return;                            // the last plane of an axis
  const int g = lane >> 4, l15 = lane & 15;
  const int64_t rs = S.rs[P0.nd];
  const int len = S.len[P0.nd];
  const int s = int(rs & 1), n = 9 * len; // 72 rs is a multiple of 8, not of 16: the image starts at double s of a 16-byte pair
  const int m = (s + n + 1) / 2;
  d2 *const img2 = reinterpret_cast<d2 *>(S.img);
  for (int i = lane; i < m; i += 64) img2[i] = d2{0, 0};
  wsync2();
  const unsigned rm = any_c ? S.cm[rows::nb_of_node(P0.nd)] : 0u;
  double rh[3] = {0, 0, 0};
  const bool mine = g >= G0 && g < G0 + NG;
#pragma unroll
  for (int r = R0; r < R0 + NR; ++r) {
    const int p = 16 * TI + g + 4 * r; // my row: a pair of this node if `mine`
    const int cell = S.pcell[p], a = S.pa[p];
    const bool on = mine && cell >= 0;
    // the pair's cell bits: the pairs of one node count through the node's free axes (rows::pair_of); the node's first pair is (R0, G0)
    int mycb = 0;
    {
      int k = p - (16 * TI + G0 + 4 * R0);
#pragma unroll
      for (int d = 0; d < 3; ++d)
        if (!((P0.nd >> d) & 1)) { mycb |= (k & 1) << d; k >>= 1; }
    }
    unsigned pos[2] = {0, 0};
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int b = 16 * tj + l15;
      if (on && b < 27) pos[tj] = S.pos[p * 27 + b];
    }
    // All row groups of the step add in the same instructions: ds_add_f64 is atomic, and where two cells of the node hold the same column
    // the LDS serialises the lanes of one instruction in its own fixed order -- one group after the other (16 live lanes per
    // instruction) costs four times the LDS instructions, which is what bounds the kernel then (profiles/r17_assemble_rows.txt).
    {
      if (on) {
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
          const int b = 16 * tj + l15;
          if (b >= 27) continue;
          const double sc = tj == 0 ? R.sac0[r] : R.sac1[r];
          double blk[9];
#pragma unroll
          for (int e = 0; e < 9; ++e) blk[e] = (tj == 0 ? R.acc0[e][r] : R.acc1[e][r]) + ((e == 0 || e == 4 || e == 8) ? sc : 0.0);
          if (any_c) { // rows / columns of constrained dofs, as assemble3.hip::row_tile
            const int tcol = rows::nb_of_column(mycb, b);
            const unsigned cmk = S.cm[tcol];
            if (rm | cmk) {
              const int64_t cnode = S.nb[tcol];
#pragma unroll
              for (int e = 0; e < 9; ++e) {
                const int c = e / 3, d = e - 3 * c;
                const bool rcn = (rm >> c) & 1u, ccn = (cmk >> d) & 1u;
                if (!rcn && !ccn) continue;
                const double v = blk[e];
                double w = 0.0;
                if (rcn) {
                  if (a == b && c == d) { // |Ke(r,r)| on the diagonal, rhs so that the update equals the inhomogeneity
                    w = fabs(v);
                    if (A.use_inhom) rh[c] += A.cval[int64_t(3) * node + c] * fabs(v);
                  }
                } else if (A.use_inhom) {
                  const double gi = A.cval[3 * cnode + d];
                  if (gi != 0.0) rh[c] -= v * gi;
                }
                blk[e] = w;
              }
            }
          }
          double *dst = S.img + s + 9 * int(pos[tj]);
#pragma unroll
          for (int e = 0; e < 9; ++e) unsafeAtomicAdd(dst + e, blk[e]); // ds_add_f64; the 27 columns of one pair are distinct blocks
        }
      }
      __builtin_amdgcn_wave_barrier(); // the steps of one node one after the other
    }
  }
  wsync2();
  { // the complete row: 16 bytes per lane, contiguous
    const uint64_t base = uint64_t(A.v_uu) + 72ull * uint64_t(rs) - 8ull * unsigned(s);
    gdouble *const G = reinterpret_cast<gdouble *>(base);
    for (int j = lane; j < m; j += 64) {
      const d2 v = img2[j];
      if (j == 0 && s) G[1] = v.y;
      else if (j == m - 1 && ((s + n) & 1)) G[2 * j] = v.x;
      else reinterpret_cast<gd2 *>(base)[j] = v;
    }
  }
  const bool inh = any_c && A.use_inhom; // wave-uniform
  if (inh) { // fixed order: tree over the 16 columns of a row group, then the groups in turn
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double v = rh[c];
      v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
      if (l15 == 0) S.part[g * 3 + c] = v;
    }
    wsync2();
  }
  // the node's right-hand side entries: the local right-hand sides of its cells in pair order (unconstrained components), then the
  // terms of its constrained rows and columns.  Stored: nobody else writes them.
  if (lane < 3) {
    double v = 0;
    if (!((rm >> lane) & 1u)) {
#pragma unroll
      for (int r = R0; r < R0 + NR; ++r)
#pragma unroll
        for (int gg = G0; gg < G0 + NG; ++gg) {
          const int p = 16 * TI + gg + 4 * r;
          const int cell = S.pcell[p];
          if (cell >= 0) v += S.fe[p * 3 + lane];
        }
    }
    if (inh)
#pragma unroll
      for (int gg = G0; gg < G0 + NG; ++gg) v += S.part[gg * 3 + lane];
    A.rhs[int64_t(3) * node + lane] = v;
  }
  wsync2();
}

// The terms of the element matrix that do not depend on the cell: on a uniform box the viscous term w mu ga . gb, the grad-div term
// gamma rho w ga_c gb_d and, in the IMEX matrix, the mass term rho/dt w N_a N_b are the same 27 x 27 x 9 numbers in every cell (in the
// Newton matrix the mass term stays in the point data, where the Newton MFMAs carry it).  One lane per entry sums them over the 27 points
// in point order, with the factors of the contraction (shape_ref4's products), into K0[a][e = 3 c + d][b]; row a = 27 and the columns
// b >= 27 are zero, so that the padding rows and columns of an MFMA tile need no branch.  Runs ahead of every row launch: no state
// (one workgroup of 1024 took 0.27 ms per launch, 32 of 256 take 0.012 ms: profiles/r18_assemble_rows.txt).
constexpr int kK0Rows = 28, kK0Cols = 32, kK0 = kK0Rows * 9 * kK0Cols;

__global__ __launch_bounds__(256) void k_rows_const(double *__restrict__ K0, Tab1D t, double ih0, double ih1, double ih2, double vol, double mu, double wgam,
                                                     double rdt, int imex) {
  const double ih[3] = {ih0, ih1, ih2};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kK0; i += gridDim.x * blockDim.x) {
    const int b = i % kK0Cols, e = (i / kK0Cols) % 9, a = i / (9 * kK0Cols);
    const int c = e / 3, d = e - 3 * c;
    double v = 0.0;
    if (a < 27 && b < 27) {
      const int ai[3] = {a % 3, (a / 3) % 3, a / 9}, bi[3] = {b % 3, (b / 3) % 3, b / 9};
      for (int q = 0; q < 27; ++q) {
        const int qi[3] = {q % 3, (q / 3) % 3, q / 9};
        double w = vol;
        for (int k = 0; k < 3; ++k) w *= t.w[qi[k]];
        double ga[3], gb[3];
        const double na2 = t.N[qi[0] * 3 + ai[0]] * t.N[qi[1] * 3 + ai[1]], nb2 = t.N[qi[0] * 3 + bi[0]] * t.N[qi[1] * 3 + bi[1]];
        const double naz = t.N[qi[2] * 3 + ai[2]], nbz = t.N[qi[2] * 3 + bi[2]];
        ga[0] = t.dN[qi[0] * 3 + ai[0]] * t.N[qi[1] * 3 + ai[1]] * naz * ih[0];
        ga[1] = t.N[qi[0] * 3 + ai[0]] * t.dN[qi[1] * 3 + ai[1]] * naz * ih[1];
        ga[2] = na2 * t.dN[qi[2] * 3 + ai[2]] * ih[2];
        gb[0] = t.dN[qi[0] * 3 + bi[0]] * t.N[qi[1] * 3 + bi[1]] * nbz * ih[0];
        gb[1] = t.N[qi[0] * 3 + bi[0]] * t.dN[qi[1] * 3 + bi[1]] * nbz * ih[1];
        gb[2] = nb2 * t.dN[qi[2] * 3 + bi[2]] * ih[2];
        double s = (w * wgam) * ga[c] * gb[d];
        if (c == d) {
          s += (w * mu) * (ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2]);
          if (imex) s += (rdt * w) * (na2 * naz) * (nb2 * nbz);
        }
        v += s;
      }
    }
    K0[i] = v;
  }
}

static void rows_const_ensure(ifem_ctx *ctx) {
  if (ctx->rows_k0.n != size_t(kK0)) ctx->rows_k0.alloc(size_t(kK0), "the constant terms of the row-owner assembly");
}

static void launch_rows_const(ifem_ctx *ctx, const double ih[3], double vol, double mu, double rho, double gamma, double inv_dt, int imex) {
  Tab1D t;
  tab1d(t, 2);
  hipLaunchKernelGGL(k_rows_const, dim3(grid_for(kK0)), dim3(256), 0, ctx->stream, ctx->rows_k0.p, t, ih[0], ih[1], ih[2], vol, mu, gamma * rho, rho * inv_dt, imex);
  IFEM_HIP_CHECK(hipGetLastError());
}

// The contraction of row tile TI over the 27 points for both column tiles (assemble3.hip::row_tile with constant geometry and per-row point
// data).  The accumulators start from the constant terms K0 of their rows' local nodes; the K-loop adds what depends on the cell: the
// convective term on the scalar part, the Newton term (with the mass term on its diagonal blocks) on the nine blocks.  The IMEX matrix has
// neither: its blocks are the table.
template <int TI>
__device__ __forceinline__ void contract(const RowArgs &A, const Tabs3 &T, RowWave &S, RowAcc &R, const int lane) {
  constexpr int BS = 9;
  const int l15 = lane & 15, g = lane >> 4;
  const int b9_0 = l15 % 9, b3_0 = l15 / 9, b9_1 = (16 + l15) % 9, b3_1 = (16 + l15) / 9; // my column nodes (27..31: zero through the z factor)
  const int al = S.pa[16 * TI + l15];
  const int a9 = al % 9, a3 = al / 9;
  R.sac0 = d4{0, 0, 0, 0}; R.sac1 = d4{0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r) { // rows g + 4 r of the tile: 128 contiguous bytes along l15
    const double *const k = A.k0 + int(S.pa[16 * TI + g + 4 * r]) * (9 * kK0Cols) + l15;
#pragma unroll
    for (int e = 0; e < BS; ++e) { R.acc0[e][r] = k[e * kK0Cols]; R.acc1[e][r] = k[e * kK0Cols + 16]; }
  }
  if (A.imex) return;
  // The point data of a K-step, 4 points of the owner's 8 cells, are loaded once by the wave: lane -> (cell slot, 48 of the slot's 384
  // contiguous bytes), requested one K-step ahead and handed over through LDS; lane (g, l15) reads point g of the slot of row l15's cell.
  // Cells the owner lacks and the padding point 27 give zeros (their rows / that point have N_a = 0: the values must only be finite).
  const int lslot = lane >> 3, lch = lane & 7;
  const int lcell = S.pcell[lslot]; // vertex pair s has cell bits s
  const d2 *const src = reinterpret_cast<const d2 *>(A.pd + int64_t(lcell < 0 ? 0 : lcell) * (27 * 12)) + 3 * lch;
  const int myslot = S.pcb[16 * TI + l15];
  d2 nx[3];
  auto request = [&](int ks) {
    const bool on = lcell >= 0 && (ks < 6 || lch < 6); // K-step 6 holds the points 24, 25, 26: 36 of the 48 doubles
#pragma unroll
    for (int i = 0; i < 3; ++i) nx[i] = on ? src[24 * ks + i] : d2{0, 0};
  };
  auto hand_over = [&](int half) {
    d2 *const dst = &S.pq[half][lslot][3 * lch];
#pragma unroll
    for (int i = 0; i < 3; ++i) dst[i] = nx[i];
    wsync2();
  };
  request(0);
  hand_over(0);
#pragma unroll 1
  for (int ks = 0; ks < 7; ++ks) {
    const int q = 4 * ks + g; // 27: the zero point
    const int q3 = q / 9, q9 = (q - q3 * 9) * 9, q4 = q3 * 4;
    if (ks < 6) request(ks + 1);
    double pq[12];
    {
      const d2 *const mine = &S.pq[ks & 1][myslot][6 * g];
#pragma unroll
      for (int i = 0; i < 6; ++i) { const d2 v = mine[i]; pq[2 * i] = v.x; pq[2 * i + 1] = v.y; }
    }
    double Nb0, Nb1, gb0[3], gb1[3];
    const double Na = T.N2[q9 + a9] * T.Nz[q4 + a3]; // zero for the padding point and the padding rows
    shape_ref4(T, q9, q4, b9_0, b3_0, Nb0, gb0);
    shape_ref4(T, q9, q4, b9_1, b3_1, Nb1, gb1);
#pragma unroll
    for (int d = 0; d < 3; ++d) { gb0[d] *= A.ih[d]; gb1[d] *= A.ih[d]; }
    // convective: sum_e rho w u_e N_a gb_e
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const double av = pq[e] * Na;
      R.sac0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, gb0[e], R.sac0, 0, 0, 0);
      R.sac1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, gb1[e], R.sac1, 0, 0, 0);
    }
    // Newton term rho N_a N_b d_d u_c with the mass term on its diagonal blocks
#pragma unroll
    for (int e = 0; e < BS; ++e) {
      const double an = Na * pq[3 + e];
      R.acc0[e] = __builtin_amdgcn_mfma_f64_16x16x4f64(an, Nb0, R.acc0[e], 0, 0, 0);
      R.acc1[e] = __builtin_amdgcn_mfma_f64_16x16x4f64(an, Nb1, R.acc1[e], 0, 0, 0);
    }
    if (ks < 6) hand_over((ks + 1) & 1); // the half that K-step ks - 1 read
  }
}

template <int WPB>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_ins_assemble_rows(RowArgs A) {
  __shared__ Tabs3 T;
  __shared__ __align__(16) RowWave SW[WPB];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  {
    const double *src = reinterpret_cast<const double *>(A.tabs3);
    double *dst = reinterpret_cast<double *>(&T);
    for (int i = threadIdx.x; i < int(sizeof(Tabs3) / 8); i += 64 * WPB) dst[i] = src[i];
  }
  __syncthreads(); // the only workgroup barrier: from here on every wave works on its own owner
  const int64_t owner = int64_t(blockIdx.x) * WPB + wave;
  if (owner >= A.n_owners) return;
  RowWave &S = SW[wave];
  int ijk[3];
  rows::owner_ijk(owner, A.n, ijk);
  // The set-up loads in batches: (1) the lattice nodes of the neighbourhood, the cells of the pairs, the pressure node; (2) what hangs
  // on them -- constraint flags and row starts of the nodes, then block positions and local right-hand sides of the cells (as compiled
  // the flags and row starts are waited for at the exchange of the cells through LDS: three rounds, where a loop per table made about 16).
  // Every load of a batch is requested before the first one is used: straight-line code, the addresses of absent nodes and cells are
  // clamped to entry 0 and the value is dropped.
  int64_t at[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) at[u] = lane + 64 * u < 125 ? rows::nb_point(ijk, A.n, lane + 64 * u) : -1;
  const rows::Pair P = rows::pair_of(lane < rows::kPairs ? lane : 0);
  const int64_t cat = lane < rows::kPairs && rows::row_point(ijk, A.n, P.nd) >= 0 ? rows::pair_cell(ijk, A.n, P) : -1;
  int32_t node[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) node[u] = A.node_of_lattice[at[u] < 0 ? 0 : at[u]];
  int32_t mycell = A.cell_at[cat < 0 ? 0 : cat];
  const int64_t pn = A.pnode_of_lattice[owner];
#pragma unroll
  for (int u = 0; u < 2; ++u) if (at[u] < 0) node[u] = -1;
  if (cat < 0) mycell = -1;
  if (lane < 32) {
    S.pcell[lane] = mycell;
    S.pa[lane] = uint8_t(mycell >= 0 ? P.a : 27);
    S.pcb[lane] = uint8_t(lane < rows::kPairs ? P.cb : 0);
  }
  uint8_t fl[2][3] = {{0, 0, 0}, {0, 0, 0}};
  uint8_t pfl = 0;
  int64_t r0[2], r1[2];
  if (A.is_c) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int c = 0; c < 3; ++c) fl[u][c] = A.is_c[int64_t(3) * (node[u] < 0 ? 0 : node[u]) + c];
    pfl = A.is_c[A.p_off_c + pn];
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) { r0[u] = A.rp_uu[node[u] < 0 ? 0 : node[u]]; r1[u] = A.rp_uu[(node[u] < 0 ? 0 : node[u]) + 1]; }
  wsync2();
  constexpr int NPOS = (rows::kPairs * 27 + 63) / 64;
  uint16_t pv[NPOS];
#pragma unroll
  for (int u = 0; u < NPOS; ++u) {
    const int i = lane + 64 * u < rows::kPairs * 27 ? lane + 64 * u : rows::kPairs * 27 - 1;
    const int p = i / 27;
    const int cell = S.pcell[p];
    pv[u] = A.posUU[(int64_t(cell < 0 ? 0 : cell) * 27 + (cell < 0 ? 0 : S.pa[p])) * 27 + (i - p * 27)];
  }
  double fv[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = lane + 64 * u < 27 * 3 + 8 ? lane + 64 * u : 27 * 3 + 7;
    const int p = i < 81 ? i / 3 : i - 81; // velocity [pair][c]; pressure: vertex i - 81 of the cell of vertex pair i - 81
    const int cell = S.pcell[p];
    const double v = A.fe[int64_t(cell < 0 ? 0 : cell) * 96 + (i < 81 ? (i - 3 * p) * 27 + (cell < 0 ? 0 : S.pa[p]) : i)];
    fv[u] = cell >= 0 ? v : 0.0;
  }
  bool cmine = false;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = lane + 64 * u;
    if (t >= 125) continue;
    const unsigned mk = node[u] < 0 ? 0u : unsigned(fl[u][0] != 0) | unsigned(fl[u][1] != 0) << 1 | unsigned(fl[u][2] != 0) << 2;
    S.nb[t] = node[u];
    S.cm[t] = uint8_t(mk);
    const int tx = t % 5 - 2, ty = (t / 5) % 5 - 2, tz = t / 25 - 2;
    if (node[u] >= 0 && (tx | ty | tz) >= 0 && tx < 2 && ty < 2 && tz < 2) { // one of the owner's own nodes: its row
      S.rs[tx | ty << 1 | tz << 2] = r0[u];
      S.len[tx | ty << 1 | tz << 2] = int32_t(r1[u] - r0[u]);
    }
    cmine = cmine || mk != 0;
  }
  const bool any_c = __any(cmine);
#pragma unroll
  for (int u = 0; u < NPOS; ++u)
    if (lane + 64 * u < rows::kPairs * 27) S.pos[lane + 64 * u] = pv[u]; // (of a pair without a cell: never read)
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (lane + 64 * u < 27 * 3 + 8) S.fe[lane + 64 * u] = fv[u];
  RowAcc R;
  contract<0>(A, T, S, R, lane);
  node_rows<0, 0, 2, 0, 4>(A, S, R, lane, any_c); // vertex node: 8 cells
  if (lane == 0) { // the pressure row of the owner's vertex: vertex b of cell pair p, b = the pair's cell bits = p
    if (!pfl) {
      double v = 0;
      for (int p = 0; p < 8; ++p) {
        const int cell = S.pcell[p];
        if (cell >= 0) v += S.fe[81 + p];
      }
      A.rhs[A.p_off_rhs + pn] = v;
    }
  }
  node_rows<0, 2, 1, 0, 4>(A, S, R, lane, any_c); // x edge
  node_rows<0, 3, 1, 0, 4>(A, S, R, lane, any_c); // y edge
  contract<1>(A, T, S, R, lane);
  node_rows<1, 0, 1, 0, 4>(A, S, R, lane, any_c); // z edge
  node_rows<1, 1, 1, 0, 2>(A, S, R, lane, any_c); // xy face
  node_rows<1, 1, 1, 2, 2>(A, S, R, lane, any_c); // xz face
  node_rows<1, 2, 1, 0, 2>(A, S, R, lane, any_c); // yz face
  node_rows<1, 2, 1, 2, 1>(A, S, R, lane, any_c); // cell interior
}

// cell at lattice position: the cell's interior node is lattice point (2 i_x + 1, 2 i_y + 1, 2 i_z + 1)
__global__ void k_rows_cell_at(int64_t n_cells, const int32_t *__restrict__ cell_unodes, const int32_t *__restrict__ lattice_of_node, int nl0, int nl1, int n0, int n1,
                               int32_t *__restrict__ cell_at) {
  const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= n_cells) return;
  const int64_t at = lattice_of_node[cell_unodes[c * 27 + 13]];
  const int x = int(at % nl0), y = int((at / nl0) % nl1), z = int(at / (int64_t(nl0) * nl1));
  cell_at[(x >> 1) + int64_t(n0) * ((y >> 1) + int64_t(n1) * (z >> 1))] = int32_t(c);
}

// Is the context one the row owners can assemble?  Reads only (plan_assembly); nullptr: yes, otherwise the reason.
const char *assemble_rows_refusal(const ifem_ctx &c) {
#if !IFEM_UU_INTERLEAVED
  return "the A_uu layout is not block-interleaved";
#else
  if (c.dim != 3 || c.kv != 2 || c.nu != 27) return "not 3D Q2 velocity";
  if (c.halo.nranks > 1 || c.nUo != c.nUl) return "several ranks";
  if (c.hang.active || c.hang.n > 0) return "hanging-node lines";
  if (!c.mf_uniform) return "the cells are not one axis-aligned box";
  if (c.want_shat) return "the scalar operator (Shat) is wanted";
  if (c.u_lattice.state < 0) return "the velocity nodes are no full lattice";
  return nullptr;
#endif
}

// The tables of the path, once per context: the lattice (setup.hip::u_lattice_ensure), the cell of every lattice cell and the room of the
// constant terms (filled by every launch).  false: no full lattice.
bool assemble_rows_ensure(ifem_ctx *ctx) {
  if (!u_lattice_ensure(ctx)) return false;
  const ULattice &L = ctx->u_lattice;
  int n[3];
  for (int d = 0; d < 3; ++d) n[d] = (L.n[d] - 1) / 2;
  if (int64_t(n[0]) * n[1] * n[2] != ctx->n_cells) return false;
  if (ctx->rows_cell_at.n != size_t(ctx->n_cells)) {
    ctx->rows_cell_at.alloc(size_t(ctx->n_cells));
    hipLaunchKernelGGL(k_rows_cell_at, dim3(grid_for(ctx->n_cells)), dim3(256), 0, ctx->stream, ctx->n_cells, ctx->cell_unodes.p, L.lattice_of_node.p, L.n[0], L.n[1], n[0], n[1],
                       ctx->rows_cell_at.p);
    IFEM_HIP_CHECK(hipGetLastError());
  }
  rows_const_ensure(ctx);
  return true;
}

// after the cell launch that wrote A.pd, on the same stream
void launch_ins_assemble_rows(ifem_ctx *ctx, const AsmArgs &C) {
  constexpr int WPB = 4;
  const ULattice &L = ctx->u_lattice;
  RowArgs A{};
  for (int d = 0; d < 3; ++d) { A.n[d] = (L.n[d] - 1) / 2; A.ih[d] = 1.0 / ctx->mf_h[d]; }
  A.n_owners = rows::n_owners(A.n);
  A.vol = ctx->mf_h[0] * ctx->mf_h[1] * ctx->mf_h[2];
  A.node_of_lattice = L.node_of_lattice.p; A.cell_at = ctx->rows_cell_at.p;
  A.posUU = ctx->posUU.p; A.rp_uu = ctx->Auu.rowptr.p; A.v_uu = ctx->Auu.val.p; A.rhs = C.rhs;
  A.is_c = C.is_c; A.cval = C.cval; A.use_inhom = C.cval ? C.use_inhom : 0;
  A.pd = C.pd; A.fe = C.fe_out; A.tabs3 = ctx->tabs3.p;
  A.pnode_of_lattice = ctx->p_lattice.node_of_lattice.p; A.p_off_c = int64_t(3) * ctx->nUl; A.p_off_rhs = int64_t(3) * ctx->nUo;
  A.mu = C.mu; A.rho = C.rho; A.gamma = C.gamma; A.inv_dt = C.inv_dt; A.imex = C.imex;
  if (!A.pd || !A.fe || !A.tabs3 || !A.cell_at || !A.pnode_of_lattice || !ctx->rows_k0.p) throw Error(IFEM_E_BADPARAM, "row-owner assembly before its cell launch");
  launch_rows_const(ctx, A.ih, A.vol, A.mu, A.rho, A.gamma, A.inv_dt, A.imex);
  A.k0 = ctx->rows_k0.p;
  hipLaunchKernelGGL((k_ins_assemble_rows<WPB>), dim3(unsigned((A.n_owners + WPB - 1) / WPB)), dim3(64 * WPB), 0, ctx->stream, A);
  IFEM_HIP_CHECK(hipGetLastError());
}

// test aid (ifem_test_rows_const): the table of the context's box for these parameters, without its padding, [a 27][b 27][e 9]
void rows_const_table(ifem_ctx *ctx, const ifem_ins_params *p, int imex, double *out) {
  if (ctx->dim != 3 || ctx->kv != 2 || !ctx->mf_uniform) throw Error(IFEM_E_BADPARAM, "ifem_test_rows_const: the context is no uniform 3D Q2 box");
  double ih[3];
  for (int d = 0; d < 3; ++d) ih[d] = 1.0 / ctx->mf_h[d];
  rows_const_ensure(ctx);
  launch_rows_const(ctx, ih, ctx->mf_h[0] * ctx->mf_h[1] * ctx->mf_h[2], p->viscosity, p->rho, p->grad_div, 1.0 / p->dt, imex);
  const std::vector<double> k = ctx->rows_k0.download(ctx->stream);
  for (int a = 0; a < 27; ++a)
    for (int b = 0; b < 27; ++b)
      for (int e = 0; e < 9; ++e) out[(a * 27 + b) * 9 + e] = k[(a * 9 + e) * kK0Cols + b];
}

} // namespace ifem
