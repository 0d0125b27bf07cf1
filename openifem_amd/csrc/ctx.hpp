// ctx.hpp -- device-side state of one ifem_ctx (one per GPU / process).
#pragma once
#include <array>
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <utility>
#include <string>
#include <vector>
#include "../../include/ifem_hip.h"

namespace ifem {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

#define IFEM_HIP_CHECK(expr)                                                                        \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess)                                                                           \
      throw ::ifem::Error(IFEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " at " + \
                                          __FILE__ + ":" + std::to_string(__LINE__));               \
  } while (0)

// ctx->scal / ctx->h_scal slots: [0,64) fused dot products, [64,128) multi-axpy coefficients, [128,256) recurrence scalars
// of the device-resident CG (linalg.hip), [kScalStageOff, +kScalStage) staging of the RCCL all-reduce (comm.hip)
constexpr int kScalSlots = 512, kScalStageOff = 256, kScalStage = 256;

template <class T>
struct DBuf { // owning device buffer
  T *p = nullptr;
  size_t n = 0;
  DBuf() = default;
  DBuf(const DBuf &) = delete;
  DBuf &operator=(const DBuf &) = delete;
  ~DBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void swap(DBuf &o) {
    std::swap(p, o.p);
    std::swap(n, o.n);
  }
  // `what` names the array in the error message of a failed allocation (an over-sized mesh must say which table did not fit)
  void alloc(size_t count, const char *what = nullptr) {
    release();
    if (!count) return;
    const hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError(); // the failed allocation must not poison the next call's error check
      size_t fr = 0, tot = 0;
      (void)hipMemGetInfo(&fr, &tot);
      throw ::ifem::Error(IFEM_E_HIP, std::string("hipMalloc of ") + std::to_string(count * sizeof(T)) + " bytes for " + (what ? what : "a device array") +
                                          " (" + std::to_string(count) + " x " + std::to_string(sizeof(T)) + " B): " + hipGetErrorString(e) + "; device memory free " +
                                          std::to_string(fr >> 20) + " of " + std::to_string(tot >> 20) + " MiB");
    }
    n = count;
  }
  void upload(const T *h, size_t count, hipStream_t s) {
    alloc(count);
    if (count) IFEM_HIP_CHECK(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s));
  }
  std::vector<T> download(hipStream_t s) const {
    std::vector<T> h(n);
    if (n) {
      IFEM_HIP_CHECK(hipMemcpyAsync(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost, s));
      IFEM_HIP_CHECK(hipStreamSynchronize(s));
    }
    return h;
  }
};

// Lazily refreshed single-precision copy of a double array (the preconditioner-only consumers stream it): `refresh` converts the
// source when the copy is stale; the invalidation events at the end of this file mark it stale when the source is rewritten
struct F32Copy : DBuf<float> {
  bool valid = false;
  void stale() { valid = false; }
  void refresh(const DBuf<double> &src, hipStream_t s, unsigned grid = 8192); // linalg.hip (k_to_f32)
};

// Row-planar block-CSR: row r owns blocks [rowptr[r], rowptr[r+1]); entry e (of BS per block) of the k-th
// block of the row lives at val[BS*rowptr[r] + e*len_r + k].  Consecutive lanes (k) read consecutive
// doubles for every e: fully coalesced without LDS staging.  BS = dim*dim (A_uu), dim (B, B^T) or 1.
// XCD-aware block index: MI355X dispatches block b to XCD b % 8 (observed, not a contract -- only speed depends on it);
// the remap hands every XCD one contiguous range of the Morton-ordered cells, so the nodes shared by neighbouring cells
// are fetched into ONE private L2 instead of eight.  Bijective for any grid size.
__device__ inline unsigned xcd_swizzle(unsigned bid, unsigned nwg) {
  constexpr unsigned NX = 8;
  const unsigned q = nwg / NX, r = nwg % NX, xcd = bid % NX, k = bid / NX;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// Value layout of A_uu (bs = dim*dim entries per block).  Block-interleaved: the bs entries of a block are contiguous,
// so the assembly scatters one node pair into one or two 64-byte segments (the f64 atomic unit retires ~24 G segments/s
// whatever the number of lanes that hit a segment) instead of into bs planes.  B, B^T, M_p, S_m stay row-planar
// (entry e of the k-th block of a row at val[bs*rowptr + e*len + k]).  IFEM_UU_INTERLEAVED=0 restores the planar A_uu.
#ifndef IFEM_UU_INTERLEAVED
#define IFEM_UU_INTERLEAVED 1
#endif
__host__ __device__ inline int64_t uu_base(int64_t rs, int64_t len, int64_t k, int bs) { // offset of entry 0 of block k
#if IFEM_UU_INTERLEAVED
  (void)len;
  return (rs + k) * bs;
#else
  (void)len;
  return rs * bs + k;
#endif
}
__host__ __device__ inline int64_t uu_estride(int64_t len) { // distance between consecutive entries of one block
#if IFEM_UU_INTERLEAVED
  (void)len;
  return 1;
#else
  return len;
#endif
}

struct PlanarCsr {
  int64_t n_rows = 0, nnzb = 0;
  int bs = 1, max_row = 0;
  DBuf<int64_t> rowptr;
  DBuf<int32_t> col;
  DBuf<double> val;
  // several ranks: rows whose columns are all owned (they can be multiplied while the halo is in flight) listed first,
  // then the rows that read a ghost column; built on first use (setup.hip::build_row_split)
  DBuf<int32_t> split_rows;
  int64_t n_interior = -1, n_boundary = 0;
  int64_t order_version = 0; // bumped when the blocks of the rows are re-ordered in place (setup.hip::reorder_uu_rows): positions taken before are stale
};

// FE tables for one (dim, kv): reference-cell shape values/gradients at the volume quadrature points.
struct FeTables {
  int dim, kv, nu, np, nq;
  double phi[27 * 27];       // [q][a]   Q_kv
  double dphi[27 * 27 * 3];  // [q][a][e]
  double psi[27 * 8];        // [q][b]   Q1 (pressure + geometry mapping)
  double dpsi[27 * 8 * 3];   // [q][b][e]
  double w[27];
  // face quadrature: per face f, nqf points: Q_kv values and Q1 gradients
  int nqf;
  double fphi[6 * 9 * 27];     // [f][qf][a]
  double fdpsi[6 * 9 * 8 * 3]; // [f][qf][v][e]
  double fw[9];
};
void build_fe_tables(FeTables &t, int dim, int kv);
// the 1D pieces the tables above are products of: the k + 1 Lagrange polynomials on the nodes j / k and their derivatives at x; QGauss(n) on [0, 1]
void fe_lagrange_1d(int k, double x, double *N, double *dN);
void fe_gauss01(int n, double *x, double *w);

struct Halo {
  int rank = 0, nranks = 1;
  std::vector<int> nbr;
  std::vector<int32_t> send_u_ptr, recv_u_ptr, send_p_ptr, recv_p_ptr;
  DBuf<int32_t> send_u_idx, send_p_idx;
  // 2-deep pressure halo of the distributed explicit S_m (empty: not available)
  std::vector<int32_t> send_s_ptr, recv_s_ptr;
  DBuf<int32_t> send_s_idx, sm_box_id;
  DBuf<int64_t> own_p_gid;
  int64_t p_lattice_n[3] = {1, 1, 1}, sm_box_lo[3] = {0, 0, 0}, sm_box_n[3] = {0, 0, 0};
  int64_t n_s_cols = 0; // nPo + far nodes
  bool has_s = false;
  DBuf<double> sendbuf;
  DBuf<double> nodal_buf; // staging of halo_refresh_nodal [nUl][dim], allocated by its first call
  void *comm = nullptr;  // ncclComm_t
  // overlapped exchanges (halo_start / halo_wait): a second communicator (ncclCommSplit of `comm`) whose send/recv groups
  // run on `hstream` (high priority) while the context stream works on the rows / cells that need no ghost value
  void *comm2 = nullptr;
  hipStream_t hstream = nullptr;
  bool owns_hstream = false;
  hipEvent_t ev_pack = nullptr, ev_done = nullptr;
  void *local = nullptr; // LocalWorld* (in-process virtual ranks, validation transport)
  const void *rev_src = nullptr; // local world only: the extended vector whose ghosts the peers fetch in a reverse exchange
  // counters since the last ifem_comm_stats(reset): halo exchanges (forward + reverse), all-reduces ordered on the stream,
  // all-reduces that made the host wait for the device
  uint64_t n_exchanges = 0, n_allreduce_dev = 0, n_allreduce_host = 0, n_allreduce_vec = 0;
};

} // namespace ifem

namespace ifem {
// ILU(0) of the explicit T_pp on its own pattern (tpp.hip): analysis once per pattern, numeric factors per Newton iteration
struct TppIlu {
  DBuf<int32_t> ent, n_low, diag, rows_f, rows_b;
  std::vector<int64_t> lvl_f, lvl_b; // level pointers into rows_f / rows_b (host: the launch plan)
  DBuf<int64_t> d_lvl_f, d_lvl_b;    // the same on the device (batched runs of small levels)
  std::vector<std::array<int32_t, 2>> plan_f, plan_b; // {level, -1}: one wide level; {l0, l1}: a run of small levels in one launch
  DBuf<double> LU, t0, t1; // factors; scratch of the Jacobi-sweep triangular solves
  bool analysed = false, factored = false;
  double pivot_min = 0, pivot_max = 0;
  bool broken = false; // the last factorisation met a zero / non-finite pivot: the caller falls back to Jacobi
  DBuf<unsigned long long> chk; // [3] device: min |pivot|, max |pivot| (bit patterns), non-finite entries
  int order_kind = 0, order_used = 0; // ifem_tuning::tpp_ilu_order the analysis was made for; the order it chose (0 natural, 1 multicolour)
};
// ILU(0) with dim x dim blocks in the natural row order (bilu.hip): the two Euclid factorisations of the SUPG block preconditioner
struct BIlu {
  int dim = 1, max_row = 0;
  int64_t n = 0, nnz = 0;
  DBuf<int64_t> rp, srcpos;          // the factor's own column-sorted CSR (owned x owned) and where each entry sits in the source values
  DBuf<int32_t> col, diag, rows_f, rows_b;
  std::vector<int64_t> lvl_f, lvl_b; // elimination levels (host: launch plan of the factorisation)
  DBuf<int64_t> d_lvl_f, d_lvl_b;
  DBuf<double> LU, dinv, t0, t1, t2; // factors (unit-lower L and U without its diagonal blocks), inverse pivot blocks, sweep scratch
  DBuf<unsigned long long> chk;
  bool analysed = false, factored = false, broken = false;
  double pivot_min = 0, pivot_max = 0;
};
// hanging-node constraint lines x[dof_i] = sum_k w_k x[master_k] (closed), see hanging.hip
struct Hanging {
  int32_t n = 0;
  DBuf<int32_t> dof, ptr, master; // local (ghost-extended) dof ids; lines of owned AND ghost hanging dofs
  DBuf<double> w, d, x, c0, y; // weights, diagonal of the hanging rows, extended scratch input / inhomogeneity / output
  DBuf<int> flag;
  std::vector<int32_t> host_dof;
  bool active = false; // some rank holds hanging lines: every rank takes part in their exchanges
};
} // namespace ifem

namespace ifem {
// the solid as MPI::FSI sees it on every rank and the scratch of the device-side FSI inputs (fsi.hip)
struct FsiState {
  int32_t nv = 0, nc = 0, nbf = 0;
  DBuf<double> vert;   // [nv][dim]
  DBuf<int32_t> cells; // [nc][2^dim]
  DBuf<double> rec;    // per solid cell: bounding box lo[dim], hi[dim], then the vertex coordinates [2^dim][dim]
  DBuf<double> bface;  // dim 2: per boundary face p1x p1y p2x p2y
  DBuf<double> vel, acc, stress;
  double box[6] = {0, 0, 0, 0, 0, 0}; // solid_box: lo, hi per direction
  DBuf<int32_t> bin_ptr, bin_cells;   // uniform grid over solid_box -> solid cells whose bounding box meets the bin
  int G[3] = {1, 1, 1};
  double inv_h[3] = {0, 0, 0};
  bool valid = false, has_fields = false, has_stress = false;
  DBuf<uint32_t> order_min, first; // first-touch cell of every local velocity node: (cell << 5 | local node) or 0xFFFFFFFF
  DBuf<int32_t> cand;              // velocity nodes whose support point lies in solid_box
  DBuf<uint8_t> taken;             // dofs that already carry a boundary or hanging line
  DBuf<uint8_t> prev[2];           // the flags of the two constraint sets before the merge (identity of the sets afterwards)
  DBuf<int64_t> counters;          // [8] device counters
  // uniform grid over the local fluid cells (point evaluation of the fluid solution, built on first use)
  DBuf<int32_t> fbin_ptr, fbin_cells;
  int fG[3] = {1, 1, 1};
  double fbox_lo[3] = {0, 0, 0}, finv_h[3] = {0, 0, 0};
  bool fbins_valid = false;
};
} // namespace ifem

namespace ifem {
// Per-kernel-family timing of one profiled step (ifem_kprof_begin / ifem_kprof_end): every launch wrapper opens a KScope, which
// records an event pair on the context stream around its launches -- nothing waits until ifem_kprof_end reads them all, so the
// queue keeps running ahead of the host as in a timed step.  One recorder per level chain: coarse multigrid levels log into
// the finest level's (they run on its stream).  The reference's counterpart: the TimerOutput sections of InsIM
// (mpi_insim.cpp:33,70,87,125,155,368).
struct KProf {
  bool on = false;
  int depth = 0; // a scope opened inside another one is part of the outer scope
  std::vector<hipEvent_t> ev;
  size_t used = 0;
  struct Rec { int cat; uint32_t e0, e1; double bytes, flops; };
  std::vector<Rec> recs;
  ~KProf() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};
struct KScope {
  KProf *k = nullptr;
  hipStream_t s = nullptr;
  uint32_t e1 = 0;
  inline KScope(ifem_ctx *ctx, int cat, double bytes = 0, double flops = 0);
  inline ~KScope();
  KScope(const KScope &) = delete;
  KScope &operator=(const KScope &) = delete;
};
} // namespace ifem

namespace ifem {
// one CSR transfer table of the multigrid hierarchy (row-parallel gather on the device)
struct MgCsr {
  int64_t n_rows = 0;
  DBuf<int64_t> ptr;
  DBuf<int32_t> col;
  DBuf<double> w;
};
} // namespace ifem

namespace ifem {
// Vertex-patch smoother of the A_uu V-cycle (patch.hip; ifem_tuning::uu_smoother = 1): the patch of a mesh vertex holds the velocity nodes
// within one node spacing of it in every cell that contains it.  Two forms of the tables, chosen per level:
// form 0, a uniform box level: the patch is the lattice box of +-1 node, clipped at the domain; all patches with the same present nodes and
//   the same constrained dofs (a "type") share one inverse.  Built on the host once per (mu, rho, gamma, dt, h, constrained-dof set).
// form 1, any other level (ifem_tuning::uu_patch_levels = 1): patches of 4..13 / 8..39 nodes (2D / 3D) from the cell tables alone, one stored
//   inverse per patch.  The topology (gen_*) is built on the host once per context, the inverses on the device once per
//   (mu, rho, gamma, dt, constrained-dof set).
struct PatchSmoother {
  bool eligible = false, valid = false; // the level can take the patch smoother / the tables below belong to `key`
  double key[9] = {0, 0, 0, 0, 0, 0, 0, -1, -1}; // mu, rho, gamma, dt, h[3], constrained-dof set, form
  int form = 0;
  int64_t n_patches = 0, inv_bytes = 0;
  int n_types = 0;
  DBuf<int32_t> tab;   // form 0: [n_patches][3^dim] velocity nodes of every patch (-1: clipped), patches sorted by (colour, type)
  DBuf<float> inv;     // form 0: [n_types][N][N] inverse patch matrices, N = dim 3^dim (symmetric; clipped nodes: identity rows)
                       // form 1: the [N_v][N_v] inverse of patch v at gen_inv_off[v], N_v = dim x its nodes (symmetric)
  DBuf<int32_t> work;  // form 0: [n_work][3] work items of the kernel: type, first patch, patches (one colour, one type each)
  int work_ptr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // form 0: work items of colour c: [work_ptr[c], work_ptr[c + 1])
  // form 1: patches sorted by (colour, nodes)
  int gen_state = 0;            // topology of this context: 0 not looked at, 1 built, -1 beyond a cap (the level keeps its node blocks)
  DBuf<int64_t> gen_node_ptr;   // [n_patches + 1] into gen_nodes
  DBuf<int32_t> gen_nodes;      // velocity node | 1 << 31 when this patch has the lowest colour among the patches that hold the node
  DBuf<int64_t> gen_cell_ptr;   // [n_patches + 1] into gen_cells
  DBuf<int32_t> gen_cells;      // cell << 3 | corner at which the patch's vertex sits in that cell
  DBuf<int64_t> gen_inv_off;    // [n_patches] offset of the patch's inverse in `inv`, in floats
  DBuf<int32_t> gen_bad;        // [1] set by the setup kernel: a non-positive pivot
  int64_t gen_col_ptr[17] = {0}; // patches of colour c: [gen_col_ptr[c], gen_col_ptr[c + 1])
  int gen_colours = 0;
  int64_t gen_entries = 0, gen_inv_floats = 0; // patch nodes over all patches; floats of the inverse store
  double gen_rejected_key[9] = {0, 0, 0, 0, 0, 0, 0, -1, -1}; // the last key the device setup refused (pivot / memory): not tried again
  bool gen_rejected = false;
};
} // namespace ifem

namespace ifem {
// reference tables of the 3D Q2/Q1 cell kernel (assemble3.hip), built on the host, copied into LDS by every workgroup
struct Tabs3 {
  double Nz[16], dNz[16];           // [q2 (4)][a2 (4)] 1D shape values / derivatives, zero for q2 = 3 or a2 = 3 (MFMA padding)
  double N2[81], DX2[81], DY2[81];  // [(q0 q1)][(a0 a1)]: N_x N_y, N'_x N_y, N_x N'_y
  double psi[27 * 8];               // [q][b] trilinear (pressure, geometry)
};
// per-cell records of that kernel (setup.hip::ensure_scat3): kAsm3Rec uint16 = [row tile 2][lane 64][column tile 2][r 4] holding
// (position of the block in its A_uu row - rank | rank << 9), rank = rank of that position among the row's 27 blocks of this cell,
// 0xFFFF = no block; kAsm3Hdr bytes = perm[32] (tile column -> local node, the cell's nodes in the order of their ids) | iperm[32] |
// permp[8] (the same for the pressure nodes) | srow[32] (position of the row's first block inside a 64-byte segment, in doubles) | padding
constexpr int kAsm3Rec = 1024, kAsm3Hdr = 128;

// B, B^T, M_p and diag(M_u) depend on the mesh and on WHICH dofs are constrained, nothing else (assemble.hip): the blocks of the last
// constrained-dof set stay until the set changes.  The same blocks integrated WITHOUT any constraint (functions of the mesh alone) are
// kept once built: the blocks of a new set are masked copies of them instead of a re-integration (M_p and diag(M_u) do not depend on
// the set), and S_m of a new set is the S_m of these copies with the rows that touch a constrained dof recomputed (linalg.hip::schur_numeric).
struct GeoCache {
  // assemblies with an unchanged (and never yet changed) constrained-dof set after which the unconstrained copies (19 + 4 GB at 128^3) are
  // given back: they only serve a CHANGE of the set.  A run whose set does change later (FSI: every time step) re-integrates them once and
  // keeps them from then on -- releasing them there would repeat a hipFree / hipMalloc / geometry launch every time step.
  static constexpr int kKeep = 2;
  bool valid = false; // B, B^T, M_p, diag(M_u) hold the blocks of constrained-dof set `key`
  int64_t key = -1;
  DBuf<double> B0, Bt0, Sm0; // unconstrained B / B^T, S_m of them
  bool b0_valid = false, sm0_valid = false;
  int unchanged = 0;       // consecutive assemblies that kept the cached blocks
  int set_changes = 0;     // times the constrained-dof set changed while blocks were cached
  uint64_t seen_asm = 0;   // a multigrid level: the finest level's asm_version its `unchanged` last counted
  int64_t refresh_stamp = -1; // a coarse multigrid level: the finest level's assembly its blocks were last refreshed for (geo_cache = 2)
  // An assembly asks for the blocks of set `k`: are the cached ones still those?  (Whether they may stay is the caller's caching mode.)
  bool holds(int64_t k) const { return valid && key == k; }
  // ... and tells what it does with them (assemble.hip::commit_assembly).  kept: they stay.  `count`: the request belongs to a new
  // assembly (a multigrid level is asked once per preconditioner application) -- the kKeep-th such hit of a run whose set never
  // changed gives the unconstrained copies back.
  bool hit_releases(bool count) const { return count && unchanged + 1 == kKeep && b0_valid && set_changes == 0; }
  void kept(bool count) {
    if (hit_releases(count)) {
      B0.release(); Bt0.release(); Sm0.release();
      b0_valid = sm0_valid = false;
    }
    if (count) ++unchanged;
  }
  // replaced: the assembly overwrites them with the blocks of set `k`; the driver sets `valid` again once they are written
  void replaced(int64_t k) {
    if (valid && key != k) ++set_changes;
    unchanged = 0;
    valid = false; key = k;
  }
};

} // namespace ifem

namespace ifem {
// Kelly error estimator (kelly.hip): 1D tables of the face integrals, the face table of the last call, the result
struct KellyTabs {
  double dn[2][3];    // [side][i]  derivative of the 1D Lagrange polynomial i at the cell's face 0 / 1
  double tv[3][3][3]; // [set][q][j] value of polynomial j at Gauss point g_q (set 0), at g_q / 2 (1), at (1 + g_q) / 2 (2): a whole face, its lower / upper subface
  double w[3];        // Gauss weights on [0, 1]
};
struct KellyState {
  int boxes = 0; // 0: not looked at yet, 1: every cell is an axis-aligned box, -1: some cell is not
  DBuf<KellyTabs> tabs;
  DBuf<int32_t> faces; // [n_cells][2 dim][IFEM_FACE_STRIDE(dim)]
  DBuf<double> eta;    // [n_cells]
};
} // namespace ifem

namespace ifem {
// Spalart-Allmaras turbulence model (sa.hip): the scalar Q_kv space is the velocity NODES, its matrix lives on the node pattern of A_uu
// (Auu.rowptr / col, one value per block, scattered through posUU).  Allocated by the first ifem_sa_* call.
struct SaState {
  DBuf<double> vec[IFEM_SA_N_VECS]; // nu~: present, evaluation point, Newton update, right-hand side, each [nUl]
  DBuf<double> val;                 // [Auu.nnzb] system matrix
  DBuf<uint8_t> is_c[2];            // constraint objects over the nodes (0 = zero, 1 = nonzero): flag ...
  DBuf<double> cval[2];             // ... and inhomogeneity, [nUl]
  bool has_c[2] = {false, false};
  DBuf<double> node_points;         // support points of the local nodes [nUl][dim] (d-linear map), built by the first ifem_sa_set_wall_points
  DBuf<double> wall_d;              // nodal distance to the nearest wall point [nUl] (DBL_MAX without wall points)
  BIlu ilu;                         // ILU(0) of the matrix (dim = 1)
  DBuf<double> dinv;                // diagonal of the matrix: the Jacobi fallback of a factorisation that broke down
  DBuf<double> V, Z, w;             // FGMRES bases (grown with the iteration count) and work vector
  DBuf<double> xext;                // several ranks: ghost-extended operator input [nUl]
  bool assembled = false, ilu_ok = false;
  int64_t val_order = -1, ilu_order = -1; // PlanarCsr::order_version of A_uu the values were scattered / the ILU(0) was analysed for
  // the wall function at a moving FSI wall (sa_wall.hip); everything below is empty until ifem_sa_set_moving_wall
  struct MovingWall {
    bool set = false, updated = false;  // a wall was given / ifem_sa_update_moving_wall_distance ran since (d_mov is "absent" before)
    int32_t nv = 0, ne = 0;             // wall vertices, wall edges (dim 2 only)
    int32_t max_vertex = -1;            // largest entry of `vertex`: a later, smaller solid must not be indexed with it
    double image_distance = 0, wall_function_distance = 0;
    int sample_at_image_point = 0;
    DBuf<int32_t> vertex;  // [nv] index into FsiState::vert
    DBuf<int32_t> by_id;   // [nv] the positions of `vertex` in ascending solid vertex id: the order of the reference's std::map
    DBuf<int32_t> edge;    // [ne][2] positions in `vertex`
    DBuf<double> normal;   // [nv][dim]
    DBuf<double> utau;     // [nv] shear_velocities
    DBuf<double> erec, vrec; // records streamed by k_sa_moving_wall: per edge v1 v2 utau1 utau2 |v2 - v1|^2, per vertex (by_id order) v utau
    DBuf<double> d_mov, yplus; // [nUl] (DBL_MAX = absent, 201 before the first update)
    DBuf<double> d_eff;    // [nUl] d_mov < d_fixed ? d_mov : d_fixed (:711-719): what SaArgs::wall_d reads once `updated`
    DBuf<double> pts, val; // [nv][dim] sample points, [nv][dim + 1] the fluid solution there
    DBuf<int32_t> cell;    // [nv] the fluid cell around each sample point or -1
    DBuf<uint32_t> order_min; // [nUl] smallest cell_order among the cells that touch the node
    DBuf<uint32_t> first_ind; // [nUl] bit 0: some indicator cell touches the node, bit 1: the first touching cell is an indicator cell
    DBuf<int64_t> count;   // [1]
    void clear() { // as if no moving wall had ever been set
      set = updated = false;
      nv = ne = 0;
      max_vertex = -1;
      for (DBuf<int32_t> *b : {&vertex, &by_id, &edge, &cell}) b->release();
      for (DBuf<double> *b : {&normal, &utau, &erec, &vrec, &d_mov, &yplus, &d_eff, &pts, &val}) b->release();
      order_min.release(); first_ind.release(); count.release();
    }
  } mw;
};
} // namespace ifem

namespace ifem {
// Fluid::MPI::SCnsEX, the explicit split solver (scnsex.hip): velocity and pressure live on the same nodes, both matrices are scalar and
// kept unconstrained on the node pattern of A_uu (one value per block, as SaState::val).  Allocated by the first ifem_scnsex_setup.
struct ExState {
  DBuf<double> av, ap;        // [Auu.nnzb] A_v = mu K + rho / dt M + rho M_sigma, A_p = (M / dt + M_sigma) / atm
  DBuf<double> dvn, dpn, dvs; // their diagonals over the nodes [nUl]; diag(A_v) once per component [dim * nUl]: the Jacobi diagonal of the stacked system
  DBuf<double> w[5];          // CG work vectors [dim * nUl]
  DBuf<double> last, red;     // last_solution of the outer loop [(dim + 1) nUl]; the two squared norms of an outer iteration
  double key[3] = {0, 0, 0};  // mu, rho, dt the matrices were integrated for
  int64_t fields_version = 0, key_fields = -1; // ifem_set_scns_fields calls that gave or released the PML field / the one the matrices belong to
  int64_t order = -1;         // PlanarCsr::order_version of A_uu the values were scattered for
  bool ready = false;
  int equal_order = 0;        // 0: not looked at yet, 1: pressure nodes == velocity nodes, -1: different counts (Taylor-Hood), -2: different tables
};
} // namespace ifem

namespace ifem {
// The pressure nodes of a uniform box level as the full lattice n[0] x n[1] (x n[2]) (setup.hip::p_lattice_ensure, host side lattice.cpp): one
// table for its readers, the direct M_p solve (mp_direct.hip) and the S_m stencil product (sm_stencil.hip).  Decided once per context: one rank,
// no hanging-node line, ifem_ctx::mf_uniform, Q1 pressure in 2D / 3D, the map node -> lattice point a bijection onto the whole box.
struct PLattice {
  int state = 0;        // 0: not looked at yet, 1: the maps below are built, -1: this context is no full lattice
  int n[3] = {1, 1, 1}; // lattice nodes per axis (cells + 1)
  DBuf<int32_t> node_of_lattice; // pressure node at lattice point i_x + n[0] (i_y + n[1] i_z)
  DBuf<int32_t> lattice_of_node; // its inverse
};

// Tensor-product direct solve of M_p on a uniform box level (mp_direct.hip): the pressure nodes form the full lattice (PLattice), so
// M_p = M_x (x) M_y (x) M_z and M_p^-1 is one sweep of tridiagonal line solves per axis.  Built lazily by the first solve_mp that could take it.
struct MpDirect {
  int state = 0;   // 0: not looked at yet, 1: the tables below are built, -1: this context keeps CG (not a full lattice, beyond a cap, or a failed check)
  int checked = 0; // 0: the present M_p values have not been probed yet, 1: they passed (ctx.hpp::geometry_written resets it when M_p is re-integrated)
  bool mass_ready = false; // an assembly has left M_p values behind
  DBuf<double> rpiv[3], mult[3]; // Thomas factors of the 1D mass matrices: reciprocal pivots, off-diagonal x reciprocal pivot, n[d] entries each
  DBuf<double> w;                // the lattice-ordered work vector of the sweeps
};

// The class tables of one lattice stencil product (lattice_stencil.hpp builds them; S_m: sm_stencil.hip, B and B^T: bb_stencil.hip): on a uniform
// box every row with the same position signature holds the same numbers.  Rows that differ from their class (`rows`) keep the CSR product.
struct StencilClasses {
  bool ready = false;  // the tables belong to the owner's `version` and passed the probe: the product takes the stencil path
  bool failed = false; // a probe failed: the context keeps the CSR product from then on
  bool said = false;   // the verbose line of an operator that keeps the CSR product has been printed
  int classes = 0, ncls[3] = {1, 1, 1};
  int64_t n_irregular = 0;
  DBuf<uint8_t> axcls;   // [n[0] + n[1] + n[2]] per-axis class of every coordinate of the row lattice
  DBuf<int32_t> first;   // [ncls[0] + ncls[1] + ncls[2]] first coordinate of every axis class
  DBuf<double> table;    // [classes][K] dense row of every class (component-major, then offset order), [classes] max |entry| behind it
  DBuf<uint16_t> cls;    // [row lattice] class of the row at that point, 0xFFFF: irregular
  DBuf<int32_t> rows;    // [n_irregular] the irregular rows (nodes); capacity lattice / 8 + 1
  DBuf<int32_t> counter; // [1] device count of the irregular rows
};

// y = S_m x from stencil tables over the pressure lattice (sm_stencil.hip): the signature of a row is, per axis, the distance to either face,
// capped at 2, and its stencil has 5^dim entries.  The tables are re-made and probed against the assembled S_m whenever S_m is re-formed
// (`version`), at set-up time.
struct SmStencil : StencilClasses {
  bool off = false;     // test aid (ifem_test_sm_apply): the context keeps the CSR product
  int64_t version = -1; // ifem_ctx::sm_version the tables (or the decision against them) belong to
};

// x = S_m^-1 b by fast diagonalisation on a uniform Q2/Q1 box level whose constrained velocity dofs are whole faces (sm_direct.hip;
// ifem_solver_opts::sm_mg = 2): S_m^-1 = (Q_z (x) Q_y (x) Q_x) diag(1 / (lambda_x + lambda_y + lambda_z)) (Q_z (x) Q_y (x) Q_x)^T.  Decided,
// and probed against the assembled S_m, whenever S_m is re-formed (`version`); the factors of an axis are kept while its key (cells, edge,
// masks) stays.
struct SmDirect {
  int64_t version = -1; // ifem_ctx::sm_version the decision belongs to
  bool ready = false;   // the factors stand and passed the probe of that version
  bool failed = false;  // a probe failed: the context keeps CG from then on
  int64_t builds = 0;   // axis eigen-solves this context has made (a re-formed S_m with the same keys adds none)
  double probe = 0;     // max |S_m x - e| / max |e| of the last probe
  double build_ms = 0;  // host time of the last factor build
  int npad[3] = {0, 0, 0}; // nodes per axis rounded up to the MFMA tile (16)
  // per axis: the key (cells, edge, masks of the own / the other components) of the tables below
  int key_n[3] = {0, 0, 0}, key_own[3] = {0, 0, 0}, key_other[3] = {0, 0, 0};
  double key_h[3] = {0, 0, 0}, lam_min[3] = {0, 0, 0}, lam_max[3] = {0, 0, 0};
  DBuf<double> Q[3], Qt[3]; // [npad][npad] row-major, zero-padded: Q and its transpose
  DBuf<double> lam[3];      // [n] eigenvalues of the axis
  DBuf<double> w0, w1;      // lattice-ordered work vectors of the contractions
  DBuf<int64_t> scan;       // [3 + 18] constrained dofs per component, face-centre flags (k_smd_masks)
  size_t bytes() const { size_t b = 0; for (int a = 0; a < 3; ++a) b += (Q[a].n + Qt[a].n + lam[a].n) * sizeof(double); return b; }
};

// The velocity nodes of the same level as the full lattice n[d] = deg cells_d + 1 (setup.hip::u_lattice_ensure, host side
// lattice.cpp::lattice_map_u): pressure point j sits at velocity point deg j.  Same eligibility and `state` protocol as PLattice.
struct ULattice {
  int state = 0;
  int n[3] = {1, 1, 1};
  int deg = 0;
  DBuf<int32_t> node_of_lattice; // velocity node at lattice point i_x + n[0] (i_y + n[1] i_z)
  DBuf<int32_t> lattice_of_node; // its inverse
};

// The velocity transfers towards the next coarser level from the lattice weight formula (mg_lattice.hip, mg_lattice.hpp) instead of the CSR
// tables, kept by the FINE level of the pair.  Decided once per ifem_mg_attach of the pair, at solve set-up (mg_lattice_u_setup): one rank, no
// replica, no hanging-node line, Q2 velocity, both levels full lattices (ULattice), every axis kept or halved, and the exact checks against
// mg_inj_u and against every row of mg_Pu / mg_Ru.  Same `state` protocol as PLattice; -1 keeps the CSR kernels.  The kernels read the two
// levels through ifem_ctx::mgl_map.
struct MgLatticeU {
  int state = 0;
  bool halved[3] = {false, false, false}; // the pair halves the cells of this axis (n_f = 2 n_c - 1); false: n_f == n_c
  int n_f[3] = {1, 1, 1}, n_c[3] = {1, 1, 1}; // velocity lattice points per axis of the two levels
  int64_t bad_p = -1, bad_r = -1, bad_inj = -1; // rows of P_u / R_u, coarse nodes of the injection that are not the formula's (-1: not looked at)
};

// y = B x and y = B^T x from stencil tables over the two lattices (bb_stencil.hip).  A B row at pressure point j couples the velocity points
// within +-deg of deg j (times dim components); a B^T row at velocity point i the at most 3^dim pressure points j with |i - deg j| <= deg.
// Each block has its own tables, read off its own assembled values (with ifem_tuning::geo_cache = 2 both are masked copies: neither is assumed
// to be the transpose of the other), re-made and probed whenever an assembly wrote the blocks (ifem_ctx::bb_version), at solve set-up.
struct BbStencil {
  StencilClasses b, bt;
  bool off = false;     // test aid (ifem_test_b_apply): the context keeps the CSR products
  bool scns = false;    // B / B^T hold the stabilised blocks of an SCnsIM assembly: ineligible until an INS assembly writes them again
  int64_t version = -1; // ifem_ctx::bb_version the tables (or the decision against them) belong to
  int64_t builds = 0;   // table builds so far (ifem_test_b_apply reports it: an assembly that kept the blocks adds none)
};
} // namespace ifem

struct ifem_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool owns_stream = true; // false: a coarse multigrid level running on the stream of the finest level (ifem_mg_attach)
  int dim = 0, kv = 0, nu = 0, np = 0, nq = 0;
  int64_t n_cells = 0;
  int64_t nUo = 0, nUl = 0, nPo = 0, nPl = 0; // velocity / pressure nodes owned / local
  int64_t n_local = 0;                        // dim*nUl + nPl
  int64_t n_global_u = 0, n_global_p = 0;     // owned counts summed over ranks (iteration limits must agree on all ranks)
  ifem::FeTables fe;
  ifem::DBuf<ifem::FeTables> d_fe;
  // mesh
  ifem::DBuf<double> vcoords;
  ifem::DBuf<int32_t> cell_unodes, cell_pnodes, cell_face_bid, indicator;
  // matrices
  ifem::PlanarCsr Auu; // rows: owned velocity nodes, cols: local velocity nodes, bs = dim*dim
  ifem::PlanarCsr Bt;  // rows: owned velocity nodes, cols: local pressure nodes, bs = dim   (block (0,1))
  ifem::PlanarCsr B;   // rows: owned pressure nodes, cols: local velocity nodes, bs = dim   (block (1,0))
  ifem::PlanarCsr Mp;  // rows: owned pressure nodes, cols: local pressure nodes, bs = 1     (mass (1,1))
  // SCnsIM (slightly compressible, SUPG): pressure-pressure block on the M_p pattern, nodal stress fields, cell fields
  ifem::DBuf<double> App, app_diag, stress, fsi_stress, sigma_pml, body_force, xinv, eddy_viscosity;
  bool has_app = false, stress_valid = false;
  ifem::PlanarCsr uinc;  // velocity node -> (cell << 5 | local index) incidence lists (gather stage of the matrix-free apply)
  // launch geometry of the last node gather {chunks, blocks} (apply_mf.hip::k_mf_gather), and a cap on its blocks (0: none) so that a small
  // mesh can give one block several chunks -- both for ifem_test_uu_fused_product only
  unsigned mf_gather_geo[2] = {0, 0}, mf_gather_block_cap = 0;
  // several ranks: the matrix-free apply keeps its own copy of the cell tables with the cells whose nodes are all owned
  // first (they are processed while the halo is in flight); the incidence lists then refer to this numbering
  ifem::DBuf<int32_t> mf_cell_unodes;
  ifem::DBuf<double> mf_vcoords;
  int64_t mf_n_interior = -1;
  // every local cell (ghost layer included) is the same axis-aligned box with edges mf_h: decided once at creation from vcoords
  // (setup.hip::detect_uniform_cells), which never change afterwards.  The matrix-free A_uu kernels then run their constant-geometry
  // variants (apply_mf.hip, mg.hip::k_uu_diag) unless ifem_tuning::mf_uniform = 0
  bool mf_uniform = false;
  double mf_h[3] = {0, 0, 0};
  ifem_tuning tune{};    // ifem_set_tuning
  ifem::PlanarCsr Sm;  // mass_schur(1,1) = B diag(M_u)^-1 B^T, explicit (single rank only; empty otherwise)
  bool sm_valid = false;
  int64_t sm_key = -1; // the constrained-dof set S_m was formed for
  ifem::F32Copy B_f32, Bt_f32; // single-precision copies for the matrix-free S_m of the approximate-preconditioner kinds
  ifem::DBuf<double> xs_ext; // [halo.n_s_cols] input of the distributed S_m SpMV: owned entries + 2-deep far nodes
  ifem::F32Copy Sm_f32; // single-precision copy of the S_m values for its SpMV (approximate-preconditioner kinds)
  ifem::F32Copy Mp_f32; // the same for M_p (CG(M_p) of the preconditioner)
  ifem::PLattice p_lattice; // the pressure nodes as a full lattice, where they are one (shared by the two readers below)
  ifem::MpDirect mp_direct; // M_p^-1 by line solves where the level is a full uniform lattice (mp_direct.hip; ifem_solver_opts::mp_solver)
  ifem::SmStencil sm_stencil; // S_m x from lattice stencil tables where the level is one (sm_stencil.hip)
  ifem::SmDirect sm_direct;   // S_m^-1 by fast diagonalisation where the level qualifies (sm_direct.hip; ifem_solver_opts::sm_mg = 2)
  ifem::ULattice u_lattice;   // the velocity nodes as a full lattice, where they are one
  ifem::BbStencil bb_stencil; // B x and B^T x from lattice stencil tables (bb_stencil.hip)
  int64_t bb_version = 0;     // B / B^T values were written (re-integrated, masked, or stabilised by an SCnsIM assembly)
  // identity of the constrained-dof SET of each AffineConstraints object (which dofs, not their values): B, B^T, M_p,
  // diag(M_u) and S_m depend on nothing else, so zero_ / nonzero_constraints with the same lines share one cache entry and
  // re-making identical constraints (time-dependent boundary values) keeps it
  // (decided by comparing the flag arrays on the device, api.hip::flags_differ)
  int64_t flag_id[2] = {0, 0}, flag_counter = 0;
  std::vector<uint8_t> seen_scratch; // api.hip::build_line_set: duplicate detection over the local dofs / nodes, all zero between calls
  // scalar velocity operator S^ = mu K + rho C(u) + rho/dt M on the A_uu block pattern (IFEM_AINV_SCALAR_*)
  ifem::DBuf<double> Shat, shat_dinv;
  ifem::F32Copy Shat_f32;
  bool want_shat = false, shat_valid = false, shat_dinv_valid = false;
  int asm_constraint_set = 0;
  ifem::GeoCache geo; // the geometry blocks of the last constrained-dof set and their unconstrained copies (assemble.hip)
  ifem::DBuf<int32_t> sm_rows;
  ifem::Hanging hang; // hanging-node lines (hanging.hip)
  ifem::FsiState fsi; // solid + scratch of the device-side FSI inputs (fsi.hip)
  ifem::SaState sa;   // Spalart-Allmaras turbulence model on the velocity nodes (sa.hip)
  ifem::ExState ex;   // Fluid::MPI::SCnsEX: scalar node matrices of the explicit split solver (scnsex.hip)
  ifem::KellyState kelly; // error estimator of refine_mesh (kelly.hip)
  // multigrid (ifem_mg_attach): the next coarser level (not owned) and the pressure transfers to it; per-level state of
  // the S_m V-cycle: 1/diag(S_m), largest eigenvalue of D^-1 S_m, scratch vectors [nPl]
  ifem_ctx *mg_coarse = nullptr;
  ifem_ctx *mg_fine = nullptr; // back link (not owned): the level this context hangs below, whose stream(s) it borrows
  bool mg_replica = false;     // mg_coarse is a REPLICATED single-rank context of the whole coarse mesh (several ranks here): restrictions are
                               // summed over the ranks by a vector all-reduce, nothing below this level exchanges anything
  ifem::MgCsr mg_Pp, mg_Rp, mg_Pu, mg_Ru;
  ifem::DBuf<int32_t> mg_inj_u; // [nUo of the coarse level] coincident owned velocity node of this level
  ifem::DBuf<uint8_t> mg_Pu_mask, mg_Ru_mask; // per weight 8 bytes: {column | components dropped by the Dirichlet flags of the two levels << 29, weight as float} (mg.hip::mg_csr_mask)
  ifem::DBuf<uint32_t> mgl_map;               // [velocity lattice] node | constrained components << 29 for the set mgl_map_key stands for: what the lattice transfer kernels read a level through (mg_lattice.hip)
  int64_t mgl_map_key = -1;
  ifem::MgLatticeU mg_lattice_u;              // the velocity transfers to mg_coarse from the lattice formula, where the pair is one (mg_lattice.hip)
  bool uu_is_stored = true;                   // the last full assembly scattered A_uu (false: ifem_tuning::stored_uu = 0, the matrix-free path)
  bool inhom_any[2] = {false, false};         // constraint object `which` carries a non-zero inhomogeneity somewhere (any rank)
  uint64_t graph_epoch = 0;                   // bumped by ifem_set_tuning / ifem_set_profiling / ifem_mg_attach: solver.hip::graph_run adds it to every replay key
  int64_t mg_mask_key[2] = {-1, -1};          // constrained-dof sets (flag ids of this level and the coarser one) of the masks
  ifem::DBuf<double> sm_dinv, mg_vec[6], mgu_vec[5];
  ifem::DBuf<float> mguf_vec[5]; // single-precision level vectors of the A_uu V-cycle (solver.hip)
  double sm_lmax = 0;
  double uu_evn = 0; // ||evaluation point|| of the current assembly (finest level)
  int64_t uu_evn_asm = -1;
  ifem::DBuf<double> sm_eig; // last iterate of the S_m power iteration: the next estimate (new constrained-dof set, same mesh) starts from it
  int64_t asm_version = 0, uu_mg_version = -1; // full assemblies done / the assembly the A_uu V-cycle data belong to
  // cached Chebyshev bound of the A_uu V-cycle's smoother.  It is a bound of B A_uu, so each smoother kind (0 node-block Jacobi, 1 vertex
  // patches) keeps its own; solver.hip::mg_uu_setup selects the level's kind, the cycle reads that entry
  struct UuBound {
    double lmax = 0, evn = -1, key[6] = {0, 0, 0, 0, 0, -1}; // estimate; ||evaluation point|| and (mu, rho, gamma, dt, noconv, constrained-dof set) it was taken at
    ifem::DBuf<double> eig; // last iterate of its power iteration: the next estimate (new constrained-dof set, same mesh) starts from it
    int64_t asm_stamp = -1; // ifem_tuning::geo_cache = 2: the finest level's assembly it was last checked for
  } uu_bound[2];
  int uu_bound_kind = 0;
  double uu_lmax() const { return uu_bound[uu_bound_kind].lmax; }
  ifem::PatchSmoother patch; // vertex-patch smoother of this level (patch.hip)
  int64_t sm_version = 0, sm_mg_version = -1; // S_m values rebuilt / the version the V-cycle data belong to
  // explicit T_pp = A_pp - A_pv Binv A_vp on the pattern of Sm and its dense LU (tpp.hip)
  ifem::DBuf<double> Tpp, tpp_diag;
  bool tpp_valid = false;
  ifem::TppIlu tpp_ilu; // level-scheduled ILU(0) of T_pp (tpp.hip)
  // the reference's structure (ifem_tuning::scns_pc = 2): ILU(0)(A_vv), B2pp = A_pp - A_pv rowsum(|A_vv|)^-1 A_vp and its ILU(0)
  ifem::BIlu pvv_ilu, b2_ilu;
  ifem::DBuf<double> B2pp, rsinv;
  bool b2_valid = false;
  ifem::PlanarCsr TppPat; // several ranks: pattern of the owned x owned block of T_pp (the per-rank ILU(0), tpp.hip)
  // matrix-free A_uu (IFEM_AINV_GMRES_BJACOBI_MF): state of the last ifem_ins_assemble
  ifem::DBuf<double> mf_ycell; // per-cell results of the matrix-free apply [n_cells][nu][dim] (two-stage scatter)
  ifem::DBuf<double> mf_eval;  // velocity part of the evaluation point, ghost-extended
  ifem::DBuf<double> mf_lift;  // inhomogeneity lift (apply_mf.hip::uu_lift_mf): lift vector [dim*nUl] and B0 times it [nPo]
  ifem_ins_params mf_params{};
  bool mf_valid = false;
  bool mf_noconv = false; // the assembled matrix has no convective terms (InsIMEX): the operator skips the second field group
  double mf_ms_total = 0;
  ifem::F32Copy Auu_f32;   // single-precision copy of Auu.val for the inner (preconditioner-only) solver
  bool last_spmv_f32 = false;
  ifem::DBuf<double> diagMu;   // diag of mass (0,0), per velocity dof (owned)
  ifem::DBuf<double> dinvMu;   // 1/diagMu
  ifem::DBuf<double> bjac;     // inverse diagonal node blocks of A_uu [nUo][dim*dim]
  ifem::F32Copy bjac_f32;  // single-precision copy for the inner solver (built on first use after bjac_setup)
  // scatter maps: position of the column inside the row, 0xFFFF = row not owned here
  ifem::DBuf<uint16_t> posUU, posUP, posPU, posPP;
  ifem::DBuf<int32_t> uu_diag_pos; // position of the diagonal block in every owned A_uu row (setup.hip::ensure_auu_values)
  // 3D Q2/Q1 cell kernel (assemble3.hip): per-cell scatter records and headers (setup.hip::ensure_scat3), reference tables
  ifem::DBuf<uint16_t> scat3;
  ifem::DBuf<uint8_t> hdr3;
  ifem::DBuf<ifem::Tabs3> tabs3;
  bool hdr3_rows = false; // the headers carry the row alignments of the present A_uu row order
  // row-owner assembly of A_uu (assemble_rows.hip): cell of every lattice cell (once per context); point data of the contraction,
  // [cell][27][12], written by the cell launch of every such assembly and held only while the path is taken; state of the last full
  // assembly (1: row owners ran, -1: refused, 0: none yet)
  ifem::DBuf<int32_t> rows_cell_at;
  ifem::DBuf<double> rows_pd, rows_fe; // (rows_fe: the cells' local right-hand sides [cell][96], summed by the owners in a fixed order)
  ifem::DBuf<double> rows_k0;          // the cell-independent terms of the element matrix, [a 28][e 9][b 32]; refilled by every row launch
  int rows_state = 0;
  const char *rows_why = nullptr; // the reason of a refusal
  // constraints (local dof numbering), sets 0 = zero, 1 = nonzero
  ifem::DBuf<uint8_t> is_c[2];
  ifem::DBuf<double> cval[2];
  bool has_c[2] = {false, false};
  // vectors
  ifem::DBuf<double> vec[IFEM_N_VECS];
  // Krylov workspace
  ifem::DBuf<double> krylovV, krylovZ, innerV, innerZ, work;
  ifem::DBuf<float> innerVf, innerZf; // bases of the single-precision flexible inner solver of IFEM_AINV_MG (ifem_tuning::inner_f32)
  ifem::DBuf<double> scal; // device scalars for reductions
  ifem::DBuf<double> partials; // per-block partial sums of the fused dot products [64][4096]
  double *h_scal = nullptr; // pinned host mirror
  ifem::Halo halo;
  bool assembled = false;
  bool profile = false; // HIP-event timing of every A_uu SpMV launch (bench only: adds a sync per launch)
  // timing
  ifem_timing timing{};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int tight_first_misses = 0, tight_first_backoff = 0; // ifem_solver_opts::inner_rel_first: consecutive misses, qualifying solves left to skip
  double spmv_uu_ms_total = 0;
  ifem::KProf kprof; // per-kernel-family event log of a profiled step (used on the finest level of a chain only)
  // The A_uu V-cycle as a hipGraph (finest level of a single-rank chain with at most ifem_tuning::vcycle_graph_cells cells): a fixed
  // sequence of ~100-200 short launches whose arguments (level vectors, tables, Chebyshev coefficients) do not change between
  // applications -- captured once per state (`key`: pointers, bounds, parameters, constraint set, sweep counts) and replayed.  `armed`:
  // the state has been seen once and ran eagerly (lazy buffers exist); the next application with the same key is captured.
  struct VcGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<uint64_t> key;
    bool armed = false;
    uint64_t launches = 0, captures = 0;
    void destroy() {
      if (exec) (void)hipGraphExecDestroy(exec);
      if (graph) (void)hipGraphDestroy(graph);
      exec = nullptr; graph = nullptr;
    }
  } vc_graph, sm_graph, pa_graph; // (pa_graph: the inner iteration's B2pp_inverse T_pp of the SCnsIM preconditioner)  // (sm_graph: the same for the V-cycle on S_m inside CG(S_m))
  // section marks of the preconditioner applications of one solve (start, after CG(M_p), after CG(S_m) + B^T, end): recorded on the
  // stream, read once when the solve has finished (ifem_solve_stats::t_cg_mp_ms / t_cg_sm_ms / t_ainv_ms) -- no host wait per section
  int test_restart_fits = 0; // test aid: stands in for the free-memory bound of the restart lengthening on this rank
  int inner_restart_eff = 0; // restart length of the inner GMRES of IFEM_AINV_MG once an application stagnated across restarts (solver.hip)
  std::vector<hipEvent_t> pc_ev;
  size_t pc_used = 0;
};

namespace ifem {
// the matrix-free A_uu kernels of this context take their constant-geometry variants
inline bool mf_takes_uniform(const ifem_ctx *c) { return c->mf_uniform && c->tune.mf_uniform != 0; }
} // namespace ifem

namespace ifem {
inline KProf &kprof_root(ifem_ctx *c) {
  while (c->mg_fine) c = c->mg_fine;
  return c->kprof;
}
inline KScope::KScope(ifem_ctx *ctx, int cat, double bytes, double flops) {
  KProf &r = kprof_root(ctx);
  if (!r.on) return;
  k = &r;
  if (r.depth++ > 0) return;
  s = ctx->stream;
  while (r.ev.size() < r.used + 2) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) { r.depth--; k = nullptr; return; }
    r.ev.push_back(e);
  }
  const uint32_t e0 = uint32_t(r.used);
  e1 = e0 + 1;
  r.used += 2;
  r.recs.push_back({cat, e0, e1, bytes, flops});
  (void)hipEventRecord(r.ev[e0], s);
}
inline KScope::~KScope() {
  if (!k) return;
  if (--k->depth > 0) return;
  (void)hipEventRecord(k->ev[e1], s);
}
} // namespace ifem

namespace ifem {
// The stored A_uu values, for every reader outside the assembly: refused when no assembly stored them or the last full assembly
// took the matrix-free path (ifem_tuning::stored_uu = 0) -- the array is then empty, or still holds the matrix of an assembly made
// before the tuning changed.
inline const DBuf<double> &stored_uu(const ifem_ctx *c) {
  if (c->Auu.val.n == 0 || !c->uu_is_stored)
    throw Error(IFEM_E_BADPARAM, "A_uu has no stored values (ifem_tuning::stored_uu = 0, or no assembly yet): this operation needs the block CSR");
  return c->Auu.val;
}

// The unconstrained B / B^T and the S_m of them (geometry cache), for their readers outside the assembly: the S_m of a new set
// (linalg.hip::schur_numeric) and the inhomogeneity lift (apply_mf.hip::uu_lift_mf).  Refused when the cache has given them back
// (GeoCache::kKeep) or never integrated them (ifem_tuning::geo_cache = 0).
inline bool has_unconstrained_blocks(const ifem_ctx *c) { return c->geo.b0_valid && c->geo.B0.n == c->B.val.n; }
// ... and B / B^T in place are masked copies of them, so S_m of the set differs from theirs only in the rows of constrained dofs
inline bool masked_from_unconstrained(const ifem_ctx *c) { return c->tune.geo_cache >= 1 && c->geo.valid && has_unconstrained_blocks(c); }
inline GeoCache &unconstrained_blocks(ifem_ctx *c) { // B0, Bt0; Sm0 / sm0_valid are schur_numeric's to form on first use
  if (!has_unconstrained_blocks(c)) throw Error(IFEM_E_BADPARAM, "the unconstrained B / B^T of the geometry cache are not there (released, or ifem_tuning::geo_cache = 0)");
  return c->geo;
}

// ---- Invalidation events: what goes stale when a writer rewrites device data.  Every writer names its write through one of these;
// the derived data they list are rebuilt by their readers (F32Copy::refresh, shat_refresh, schur_numeric / sm_ensure, ...).

// A_uu written: its stored values, or the matrix-free operator state of a stored_uu = 0 assembly.  The scalar operator S^ is
// integrated by the same cell kernel: its Jacobi scaling and single-precision copy go with it.
inline void uu_written(ifem_ctx *c) {
  c->Auu_f32.stale();
  c->Shat_f32.stale();
  c->shat_dinv_valid = false;
}
// the inverse node blocks `bjac` written
inline void bjac_written(ifem_ctx *c) { c->bjac_f32.stale(); }
// an assembly left B, B^T, M_p, diag(M_u) holding the blocks of constrained-dof set `key` (`blocks`: re-integrated or masked, i.e. their
// values were written -- the stencil tables of bb_stencil.hip belong to the values; false: kept; `mass`: M_p was re-integrated).  The
// single-precision copies of B / B^T are re-made once per assembly; S_m stays while the set stays
// (ifem_tuning::geo_cache = 1; the reference rebuilds it every solve(), same values).
inline void geometry_written(ifem_ctx *c, int64_t key, bool mass, bool blocks) {
  c->B_f32.stale(); c->Bt_f32.stale();
  if (blocks) { c->bb_version++; c->bb_stencil.scns = false; }
  if (mass) { c->Mp_f32.stale(); c->mp_direct.checked = 0; } // (the direct solve probes the new values before it trusts them again)
  c->mp_direct.mass_ready = true;
  if (key != c->sm_key || c->tune.geo_cache != 1) { c->sm_valid = false; c->sm_key = key; }
}
// S_m formed for the present blocks (explicit values, or the diagonal of its operator form)
inline void sm_written(ifem_ctx *c) {
  c->sm_valid = true;
  c->Sm_f32.stale();
  c->sm_version++;
}
// an SCnsIM assembly: A_uu, B and B^T hold the SUPG-stabilised blocks (the geometry cache no longer describes them), App is new.
// S_m, the matrix-free and scalar operators of the INS assembly, T_pp and the three ILU(0) factorisations are stale.
inline void scns_assembled(ifem_ctx *c) {
  uu_written(c);
  c->uu_is_stored = true;
  c->B_f32.stale(); c->Bt_f32.stale();
  c->bb_version++; c->bb_stencil.scns = true; // (stabilised blocks: the products keep CSR)
  c->sm_valid = false; c->sm_key = -1;
  c->geo.valid = false;
  c->mf_valid = false;
  c->shat_valid = false;
  c->tpp_valid = false; c->tpp_ilu.factored = false;
  c->b2_valid = false; c->pvv_ilu.factored = false; c->b2_ilu.factored = false;
}
} // namespace ifem
