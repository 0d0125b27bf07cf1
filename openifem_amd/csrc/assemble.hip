// assemble.hip -- host side of InsIM::assemble / InsIMEX::assemble (reference: source/mpi_insim.cpp:153-362,
// source/mpi_insimex.cpp:150-355): zeroing, argument block, kernel selection, epilogue.
//
// The cell kernels integrate the Newton-linearised INS weak form in component-block form:
//   Ke[(a,c),(b,d)] = sum_q JxW { d_cd [ mu gN_a.gN_b + rho N_a (u.gN_b) + rho/dt N_a N_b ]
//                                 + rho N_a N_b d_d u_c + gamma rho d_c N_a d_d N_b }
//   Ke[(a,c),p_b]   = -sum_q JxW d_c N_a  psi_b          (and its transpose)
// and scatter with AffineConstraints::distribute_local_to_global(..., true) semantics straight into the
// device block matrices:
//   assemble3.hip  3D Q2/Q1: contraction on the FP64 matrix cores, one wavefront per cell
//   assemble2.hip  every other (dim, kv): quadrature-point-outer vector kernel, one wavefront per cell
//
// The driver (launch_ins_assemble_ex) first DECIDES what the call does -- plan_assembly reads the context and returns an AsmPlan
// or throws, changing nothing -- then commits the context state, then runs the plan in one order: unconstrained geometry pass,
// masked copies, zero-fill, cell kernel, epilogue, inhomogeneity lift, hanging-node condensation.  Modes (kernels.hpp::AsmMode):
// a full assembly, a rhs-only one (InsIMEX), the geometry blocks of a multigrid level.  The geometry cache (ctx.hpp::GeoCache)
// is filled here and nowhere else.
#include <hip/hip_runtime.h>
#include "ctx.hpp"
#include "kernels.hpp"
#include "assemble_common.hpp"

namespace ifem {

void launch_ins_assemble2_kernel(ifem_ctx *ctx, const AsmArgs &A);
bool launch_ins_assemble3_kernel(ifem_ctx *ctx, const AsmArgs &A);

// B / B^T of a constrained-dof set from the unconstrained blocks: distribute_local_to_global(..., true) drops the rows and
// columns of constrained dofs, i.e. plane c of the B^T row of node a, and entry c of every B block in the
// column of node a, when velocity dof (a, c) is constrained -- the kept entries are the unconstrained sums unchanged.
template <int DIM>
__global__ void k_mask_bt(int64_t n_rows, const int64_t *__restrict__ rp, const uint8_t *__restrict__ is_c,
                          const double *__restrict__ src, double *__restrict__ dst) {
  const int64_t row = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 5; // 32 lanes per row
  const int lig = threadIdx.x & 31;
  if (row >= n_rows) return;
  const int64_t rs = rp[row];
  const int len = int(rp[row + 1] - rs);
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    const bool drop = is_c && is_c[row * DIM + c];
    for (int k = lig; k < len; k += 32) dst[rs * DIM + int64_t(c) * len + k] = drop ? 0.0 : src[rs * DIM + int64_t(c) * len + k];
  }
}
template <int DIM>
__global__ void k_mask_b(int64_t n_rows, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
                         const uint8_t *__restrict__ is_c, const double *__restrict__ src, double *__restrict__ dst) {
  const int64_t row = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 5;
  const int lig = threadIdx.x & 31;
  if (row >= n_rows) return;
  const int64_t rs = rp[row];
  const int len = int(rp[row + 1] - rs);
  for (int k = lig; k < len; k += 32) {
    const int64_t nd = col[rs + k];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const bool drop = is_c && is_c[nd * DIM + c];
      dst[rs * DIM + int64_t(c) * len + k] = drop ? 0.0 : src[rs * DIM + int64_t(c) * len + k];
    }
  }
}
template <int DIM>
static void masked_geometry_blocks(ifem_ctx *ctx, int w) {
  KScope ks(ctx, IFEM_KC_SCHUR_SETUP, 16.0 * double(ctx->B.val.n + ctx->Bt.val.n));
  const uint8_t *flags = ctx->has_c[w] ? ctx->is_c[w].p : nullptr;
  hipStream_t s = ctx->stream;
  const int64_t nu = ctx->Bt.n_rows, np = ctx->B.n_rows;
  if (nu) hipLaunchKernelGGL((k_mask_bt<DIM>), dim3(unsigned((nu * 32 + 255) / 256)), dim3(256), 0, s, nu, ctx->Bt.rowptr.p, flags, ctx->geo.Bt0.p, ctx->Bt.val.p);
  if (np) hipLaunchKernelGGL((k_mask_b<DIM>), dim3(unsigned((np * 32 + 255) / 256)), dim3(256), 0, s, np, ctx->B.rowptr.p, ctx->B.col.p, flags, ctx->geo.B0.p, ctx->B.val.p);
}

// ---- one launch of the cell kernel: what it integrates BESIDES the right-hand side, which it always integrates (the kernel has no
// switch for it: a geometry-only launch leaves a right-hand side nobody reads)
struct CellWork {
  bool uu;  // A_uu, into its stored values
  bool geo; // B, B^T, M_p, diag(M_u)
};

// One launch, in stream order: the zero-fill of what it integrates (`shat`: of the scalar operator too), the argument block, the kernel
// between ev0 and ev1 (the driver's last launch is the one timing.assemble_kernel_ms reports).
// `cset`: the constraint object the scatter applies (0 / 1), -1: none.
// imex = 1: InsIMEX::assemble (mpi_insimex.cpp:150-355): every field comes from the present solution, the matrix has no
// convective terms.
// rows_uu (with w.uu): A_uu is assembled by row owners (assemble_rows.hip) -- the cell kernel integrates what else there is, writes the
// point data of the contraction beside it, and the row kernel follows it between the same two events.  Its rows are stored, not added
// to: no fill of the values.
static void run_cell_kernel(ifem_ctx *ctx, const ifem_ins_params *p, CellWork w, bool shat, int cset, int imex, bool rows_uu = false) {
  hipStream_t s = ctx->stream;
  const int dim = ctx->dim;
  const bool scatter_uu = w.uu && !rows_uu;
  const double nuu = w.uu ? double(ctx->Auu.val.n) : 0.0;
  const double npd = rows_uu ? double(ctx->n_cells) * 27 * 12 : 0.0;
  if (rows_uu && ctx->rows_pd.n != size_t(npd)) ctx->rows_pd.alloc(size_t(npd), "the point data of the row-owner assembly");
  if (rows_uu && ctx->rows_fe.n != size_t(ctx->n_cells) * 96) ctx->rows_fe.alloc(size_t(ctx->n_cells) * 96, "the local right-hand sides of the row-owner assembly");
  const double ngeo = w.geo ? double(ctx->Bt.val.n + ctx->B.val.n + ctx->Mp.val.n + ctx->diagMu.n) : 0.0;
  { // system_matrix = 0; mass_matrix = 0; system_rhs = 0  (:163-165)
    KScope ks_fill(ctx, IFEM_KC_ZERO_FILL, 8.0 * ((scatter_uu ? nuu : 0.0) + ngeo + double(ctx->vec[IFEM_VEC_RHS].n)));
    // (a hand-written fill kernel with 16-byte non-temporal stores measures the same 15 ms for the 78 GB at 128^3)
    if (scatter_uu) IFEM_HIP_CHECK(hipMemsetAsync(ctx->Auu.val.p, 0, ctx->Auu.val.n * sizeof(double), s));
    if (w.geo) {
      IFEM_HIP_CHECK(hipMemsetAsync(ctx->Bt.val.p, 0, ctx->Bt.val.n * sizeof(double), s));
      IFEM_HIP_CHECK(hipMemsetAsync(ctx->B.val.p, 0, ctx->B.val.n * sizeof(double), s));
      IFEM_HIP_CHECK(hipMemsetAsync(ctx->Mp.val.p, 0, ctx->Mp.val.n * sizeof(double), s));
      IFEM_HIP_CHECK(hipMemsetAsync(ctx->diagMu.p, 0, ctx->diagMu.n * sizeof(double), s));
    }
    if (shat) {
      if (ctx->Shat.n != (size_t)ctx->Auu.nnzb) ctx->Shat.alloc((size_t)ctx->Auu.nnzb);
      IFEM_HIP_CHECK(hipMemsetAsync(ctx->Shat.p, 0, ctx->Shat.n * sizeof(double), s));
    }
    IFEM_HIP_CHECK(hipMemsetAsync(ctx->vec[IFEM_VEC_RHS].p, 0, ctx->vec[IFEM_VEC_RHS].n * sizeof(double), s));
  }
  AsmArgs A{};
  fill_cell_args(ctx, p, cset, A);
  A.v_mp = ctx->Mp.val.p; A.diagMu = ctx->diagMu.p;
  A.v_s = ctx->want_shat ? ctx->Shat.p : nullptr;
  A.rhs_only = !w.uu && !w.geo; // (the kernel reads the two skips only when this is 0; with row owners the launch still owes the
                                // right-hand side the terms of the constrained pressure / velocity dofs of B and B^T)
  A.skip_uu = !scatter_uu;
  A.pd = rows_uu ? ctx->rows_pd.p : nullptr;
  A.fe_out = rows_uu ? ctx->rows_fe.p : nullptr;
  A.skip_geo = !w.geo;
  A.debug_skip = ctx->tune.asm_skip;
  A.xcd_swizzle = ctx->tune.xcd_swizzle;
  A.eval = ctx->vec[imex ? IFEM_VEC_PRESENT : IFEM_VEC_EVAL].p; A.imex = imex;
  A.mu = p->viscosity; A.rho = p->rho; A.gamma = p->grad_div; A.inv_dt = 1.0 / p->dt;
  IFEM_HIP_CHECK(hipEventRecord(ctx->ev0, s));
  {
  // algorithmic traffic / work of the cell kernel: every stored value of the blocks it integrates
  // written once, the right-hand side, per cell the mesh tables and the three nodal vectors it gathers; flops of the
  // component-block form: per (node pair, point) dim^2 (2 FMA) + dim (2 FMA) + 5 products (53 flop in 3D), per (velocity
  // node, pressure node, point) 2 (1 + dim) when B / B^T / M_p are integrated.  MFMA padding is not counted.  Row owners: the same
  // values and flops from two launches, plus the point data written once by the cells and read once by its owners.  (The flops stay the
  // algorithmic ones: the row owners no longer execute the cell-independent terms, which they take from a table, assemble_rows.hip.)
  const int nd = ctx->nu * dim + ctx->np, npc = 1 << dim;
  const double pair = 2.0 * (2 * dim * dim + 2 * dim) + 5.0; // 24 FMA + 5 products in 3D
  KScope ks_asm(ctx, IFEM_KC_ASSEMBLE, 8.0 * (nuu + 2.0 * (npd + (rows_uu ? 96.0 * double(ctx->n_cells) : 0.0)) + ngeo + double(ctx->nUo) * dim + double(ctx->nPo)) + double(ctx->n_cells) * (npc * dim * 8.0 + (ctx->nu + ctx->np) * 4.0 + 3.0 * nd * 8.0),
                double(ctx->n_cells) * ctx->nq * ((nuu > 0 ? double(ctx->nu) * ctx->nu * pair : 0.0) + (ngeo > 0 ? double(ctx->nu) * ctx->np * 2.0 * (1 + dim) : 0.0)));
  if (!launch_ins_assemble3_kernel(ctx, A)) // assemble3.hip: 3D Q2/Q1 on the FP64 matrix cores
    launch_ins_assemble2_kernel(ctx, A);    // assemble2.hip (quadrature-point-outer, register accumulators)
  if (rows_uu) launch_ins_assemble_rows(ctx, A);
  }
  IFEM_HIP_CHECK(hipEventRecord(ctx->ev1, s));
}

// ---- filling the geometry cache (ctx.hpp::GeoCache)
// B, B^T, M_p, diag(M_u) of the mesh alone: one geometry-only launch with no constraint set, B / B^T copied away.  Touches neither
// geo.valid nor geo.key: which set the blocks in place belong to is the driver's bookkeeping (masked_geometry_blocks runs next).
static void integrate_unconstrained_geometry(ifem_ctx *ctx, const ifem_ins_params *p) {
  run_cell_kernel(ctx, p, CellWork{false, true}, ctx->want_shat, -1, 0);
  GeoCache &g = ctx->geo;
  if (g.B0.n != ctx->B.val.n) g.B0.alloc(ctx->B.val.n);
  if (g.Bt0.n != ctx->Bt.val.n) g.Bt0.alloc(ctx->Bt.val.n);
  if (ctx->B.val.n) IFEM_HIP_CHECK(hipMemcpyAsync(g.B0.p, ctx->B.val.p, ctx->B.val.n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  if (ctx->Bt.val.n) IFEM_HIP_CHECK(hipMemcpyAsync(g.Bt0.p, ctx->Bt.val.p, ctx->Bt.val.n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  g.b0_valid = true;
}

// ---- the driver
// Where B, B^T, M_p and diag(M_u) of an assembly come from (ctx.hpp::GeoCache).  An assembly whose constrained-dof set equals that of
// the previous one (zero_ and nonzero_constraints of make_constraints list the same dofs) keeps them (bit-identical to re-integrating
// them).  A NEW set (every FSI step): B / B^T are masked copies of the unconstrained ones, which are integrated once per mesh; M_p and
// diag(M_u) do not depend on the set at all.  Same values as re-integrating them under the new set (the kept entries are the same sums).
enum class GeoFrom { Kept, Masked, Cell };

struct AsmPlan {
  AsmMode mode;
  GeoFrom geo = GeoFrom::Kept;      // (a rhs-only assembly: kept, and the cache is not asked)
  bool cache_hit = false;           // the cache holds the blocks of the set and the caching mode lets them stay
  bool counted = false;             // the cache counts this request: it belongs to a new assembly of the finest level
  bool unconstrained_first = false; // the masked copies need the unconstrained pass first (M_p and diag(M_u) are then re-integrated too)
  bool stores_uu = false;           // a full assembly that scatters A_uu; a full one that does not is matrix-free (ifem_tuning::stored_uu = 0)
  bool lift = false;                // ... and owes the right-hand side the inhomogeneity lift (apply_mf.hip::uu_lift_mf)
  bool rows_uu = false;             // ... by row owners (assemble_rows.hip) instead of the cell kernel's atomic scatter
  const char *rows_refused = nullptr; // why not, when ifem_tuning::asm_rows asked for them
  bool matrix_free() const { return mode == AsmMode::Full && !stores_uu; }
};

static uint64_t finest_asm_version(const ifem_ctx *c) {
  while (c->mg_fine) c = c->mg_fine;
  return uint64_t(c->asm_version);
}

// The decision: reads the context, changes nothing, and throws every refusal of the driver.
static AsmPlan plan_assembly(const ifem_ctx &c, int w, AsmMode mode) {
  AsmPlan pl{mode};
  if (mode == AsmMode::Rhs) {
    if (!c.assembled) throw Error(IFEM_E_BADPARAM, "rhs-only assembly before any matrix assembly");
    return pl;
  }
  const bool full = mode == AsmMode::Full;
  // ifem_tuning::stored_uu = 0: the velocity-velocity block is never stored.  The cell kernel integrates the right-hand side only, the
  // geometry blocks come from the cache; A_uu is applied matrix-free in fp64 by the outer operator (the same operator to 1e-13,
  // test_matrix_free_uu_apply_equals_assembled_block) and its node-block diagonal comes from the cell integrals.
  // An assembly whose active constraint set carries non-zero values (the first Newton iteration of a step with inflow values, every
  // FSI step) owes the right-hand side the K g that distribute_local_to_global moves there: K g is the operator applied to a vector
  // that lives on the constrained dofs, so the matrix-free cell kernel computes it with its input mask inverted and the unconstrained
  // B of the geometry cache supplies the pressure rows.  Hanging-node lines are condensed around the operator afterwards
  // (hanging_condense_rhs), on the lifted right-hand side.
  pl.stores_uu = full && c.tune.stored_uu != 0;
  pl.lift = pl.matrix_free() && c.has_c[w] && c.inhom_any[w];
  // ifem_tuning::asm_rows: the stored block by row owners where the context is a uniform 3D Q2 box on a full lattice (a lattice not looked
  // at yet is decided by the launch, which falls back to the cell kernel's scatter).  InsIMEX matrices take the path as well.
  if (pl.stores_uu && c.tune.asm_rows != 0) {
    pl.rows_refused = c.tune.asm3_variant == 1 ? "asm3_variant = 1" : assemble_rows_refusal(c);
    pl.rows_uu = pl.rows_refused == nullptr;
  }
  // ifem_tuning::geo_cache = 0 switches the keeping off for full assemblies; a multigrid level keeps its blocks unless geo_cache = 2 and
  // counts ASSEMBLIES of the finest level (its version stamp), not the preconditioner applications that ask.
  const bool may_keep = full ? c.tune.geo_cache == 1 : c.tune.geo_cache != 2;
  pl.counted = full || finest_asm_version(&c) != c.geo.seen_asm;
  pl.cache_hit = may_keep && c.geo.holds(c.flag_id[w]);
  // are the unconstrained copies there once the cache has counted this request (the kKeep-th hit gives them back)?
  const bool copies = c.geo.b0_valid && !(pl.cache_hit && c.geo.hit_releases(pl.counted));
  if (!pl.cache_hit) pl.geo = c.tune.geo_cache ? GeoFrom::Masked : GeoFrom::Cell;
  // the lift applies the unconstrained B: a cache that gave its copies back (GeoCache::kKeep) integrates them once more and keeps them
  else if (pl.lift && !copies) pl.geo = GeoFrom::Masked;
  pl.unconstrained_first = pl.geo == GeoFrom::Masked && !copies;
  if (pl.matrix_free() && pl.geo == GeoFrom::Cell)
    throw Error(IFEM_E_BADPARAM, "stored_uu = 0 needs ifem_tuning::geo_cache >= 1 (the geometry blocks come from their own launch)");
  return pl;
}

// The context state an accepted assembly sets before anything runs.  A rhs-only assembly sets none: asm_constraint_set, the cache and
// the operator state stay those of the matrices in place.
static void commit_assembly(ifem_ctx *ctx, const ifem_ins_params *p, int cset, int imex, const AsmPlan &pl) {
  if (pl.mode == AsmMode::Rhs) return;
  if (pl.mode == AsmMode::Full) {
    if (pl.stores_uu) ensure_auu_values(ctx);
    ctx->uu_is_stored = pl.stores_uu;
    // state the matrix-free A_uu needs to reproduce this matrix (apply_mf.hip)
    const size_t nu = size_t(ctx->dim) * size_t(ctx->nUl);
    if (ctx->mf_eval.n != nu) ctx->mf_eval.alloc(nu);
    if (imex) IFEM_HIP_CHECK(hipMemsetAsync(ctx->mf_eval.p, 0, nu * sizeof(double), ctx->stream)); // no convection in the IMEX matrix
    else IFEM_HIP_CHECK(hipMemcpyAsync(ctx->mf_eval.p, ctx->vec[IFEM_VEC_EVAL].p, nu * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    ctx->mf_params = *p;
    ctx->mf_valid = true;
    ctx->mf_noconv = imex != 0;
    ctx->asm_version++; // before the cache counts this assembly
  } else
    ctx->geo.seen_asm = finest_asm_version(ctx);
  if (pl.cache_hit) ctx->geo.kept(pl.counted);
  else ctx->geo.replaced(ctx->flag_id[cset]);
}

// What follows the launches.  A multigrid level of S_m needs 1/diag(M_u) and the staleness of S_m (stale if the blocks are another
// set's); a rhs-only assembly reports its kernel time and nothing else.
static void assemble_epilogue(ifem_ctx *ctx, const AsmPlan &pl, int cset) {
  if (pl.mode != AsmMode::Rhs) {
    dinv_setup(ctx);
    ctx->asm_constraint_set = cset;
    // (M_p's single-precision copy goes stale only when M_p was re-integrated: with the unconstrained copies, or by the cell kernel)
    geometry_written(ctx, ctx->flag_id[cset], pl.unconstrained_first || pl.geo == GeoFrom::Cell, pl.geo != GeoFrom::Kept);
  }
  if (pl.mode == AsmMode::Full) {
    if (pl.stores_uu) bjac_setup(ctx);
    else uu_block_diag_mf(ctx);
    ctx->assembled = true;
    ctx->has_app = false;
    uu_written(ctx);
    ctx->shat_valid = ctx->want_shat;
  }
  if (pl.mode != AsmMode::LevelGeometry) { // the time of the launch between ev0 and ev1 (not of the unconstrained pass before it)
    IFEM_HIP_CHECK(hipEventSynchronize(ctx->ev1));
    float ms = 0;
    IFEM_HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->timing.assemble_kernel_ms = ms;
  }
}

void launch_ins_assemble_ex(ifem_ctx *ctx, const ifem_ins_params *p, int use_nonzero, int imex, AsmMode mode) {
  const int cset = use_nonzero ? 1 : 0;
  const auto mask = ctx->dim == 3 ? masked_geometry_blocks<3> : masked_geometry_blocks<2>;
  const AsmPlan pl = plan_assembly(*ctx, cset, mode);
  commit_assembly(ctx, p, cset, imex, pl);
  if (mode == AsmMode::LevelGeometry && pl.geo == GeoFrom::Kept) return; // the level's blocks and all that derives from them stand
  if (pl.unconstrained_first) integrate_unconstrained_geometry(ctx, p);
  if (pl.geo == GeoFrom::Masked) mask(ctx, cset);
  // (a multigrid level that took its blocks from the cache has nothing else for the cell kernel to integrate)
  bool rows_uu = pl.rows_uu;
  if (mode == AsmMode::Full) { // the tables of the row owners; without them (no full lattice) and without the path its point data goes
    if (rows_uu && !assemble_rows_ensure(ctx)) rows_uu = false;
    if (!rows_uu) { ctx->rows_pd.release(); ctx->rows_fe.release(); }
    ctx->rows_state = rows_uu ? 1 : (pl.stores_uu && ctx->tune.asm_rows != 0 ? -1 : 0);
    ctx->rows_why = rows_uu ? nullptr : (pl.rows_refused ? pl.rows_refused : "the velocity nodes are no full lattice");
  }
  if (mode != AsmMode::LevelGeometry || pl.geo == GeoFrom::Cell) run_cell_kernel(ctx, p, CellWork{pl.stores_uu, pl.geo == GeoFrom::Cell}, ctx->want_shat && mode != AsmMode::Rhs, cset, imex, rows_uu);
  if (pl.geo != GeoFrom::Kept) ctx->geo.valid = true; // (commit_assembly cleared it if the blocks were to be replaced: a launch that threw leaves no set's blocks behind)
  assemble_epilogue(ctx, pl, cset);
  if (pl.lift) uu_lift_mf(ctx);
  if (mode != AsmMode::LevelGeometry) hanging_condense_rhs(ctx, use_nonzero);
}

} // namespace ifem
