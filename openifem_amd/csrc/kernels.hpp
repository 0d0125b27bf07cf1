// kernels.hpp -- host-callable launchers implemented in the .hip translation units.
#pragma once
#include <functional>
#include <vector>
#include "ctx.hpp"
#include "lattice.hpp"

namespace ifem {

// setup.hip
void build_pattern(ifem_ctx *ctx, PlanarCsr &M, int bs, int64_t n_rows_owned, int R, const int32_t *d_rows, int C,
                   const int32_t *d_cols, DBuf<uint16_t> &pos);

void ensure_auu_values(ifem_ctx *ctx);
bool ensure_scat3(ifem_ctx *ctx, bool with_rows); // records of the 3D Q2/Q1 cell kernel (assemble3.hip); false: not applicable
void build_schur_pattern(ifem_ctx *ctx);
void build_schur_pattern_owned(ifem_ctx *ctx); // several ranks: owned x owned block, into ctx->TppPat
void build_incidence(ifem_ctx *ctx);
void detect_uniform_cells(ifem_ctx *ctx); // sets ifem_ctx::mf_uniform / mf_h from vcoords (once, at context creation)
int64_t compact_flagged_rows(ifem_ctx *ctx, const int64_t *flag, int64_t n, DBuf<int32_t> &rows); // ascending list of the flagged rows
void build_mf_cell_split(ifem_ctx *ctx); // several ranks: interior-first copy of the cell tables for the matrix-free apply

// assemble.hip
// what one call of the INS assembly driver assembles
enum class AsmMode {
  Rhs,           // the right-hand side only (the matrices stay as they are)
  Full,          // A_uu (or its matrix-free state), B, B^T, M_p, diag(M_u) and the right-hand side
  LevelGeometry, // B, B^T, M_p, diag(M_u) only: a multigrid level of the pressure Schur complement (no A_uu, no right-hand side state)
};
// row-owner assembly of A_uu on uniform 3D Q2 boxes (assemble_rows.hip): why a context cannot take it (nullptr: it can; reads only), its
// tables (false: no full lattice), the launch after the cell launch that wrote A.pd
struct AsmArgs;
const char *assemble_rows_refusal(const ifem_ctx &c);
bool assemble_rows_ensure(ifem_ctx *ctx);
void launch_ins_assemble_rows(ifem_ctx *ctx, const AsmArgs &A);
void rows_const_table(ifem_ctx *ctx, const ifem_ins_params *p, int imex, double *out); // test aid: the constant terms, [a 27][b 27][e 9]
void launch_ins_assemble_ex(ifem_ctx *ctx, const ifem_ins_params *p, int use_nonzero, int imex, AsmMode mode);
// the part of the argument block that the INS and the SCnsIM cell kernels share (AsmArgs, ScnsArgs: the same field names);
// `cset`: the constraint object the scatter applies (0 / 1), -1: none
template <class Args, class Params>
void fill_cell_args(const ifem_ctx *ctx, const Params *p, int cset, Args &A) {
  A.n_cells = ctx->n_cells; A.nUo = ctx->nUo; A.nUl = ctx->nUl; A.nPo = ctx->nPo;
  A.fe = ctx->d_fe.p;
  A.vcoords = ctx->vcoords.p; A.cell_unodes = ctx->cell_unodes.p; A.cell_pnodes = ctx->cell_pnodes.p;
  A.cell_face_bid = ctx->cell_face_bid.p; A.indicator = ctx->indicator.p;
  A.posUU = ctx->posUU.p; A.posUP = ctx->posUP.p; A.posPU = ctx->posPU.p; A.posPP = ctx->posPP.p;
  A.rp_uu = ctx->Auu.rowptr.p; A.rp_bt = ctx->Bt.rowptr.p; A.rp_b = ctx->B.rowptr.p; A.rp_mp = ctx->Mp.rowptr.p;
  A.v_uu = ctx->Auu.val.p; A.v_bt = ctx->Bt.val.p; A.v_b = ctx->B.val.p; A.rhs = ctx->vec[IFEM_VEC_RHS].p;
  const bool constrained = cset >= 0 && ctx->has_c[cset];
  A.is_c = constrained ? ctx->is_c[cset].p : nullptr;
  A.cval = constrained ? ctx->cval[cset].p : nullptr;
  A.use_inhom = (cset == 1 && constrained) ? 1 : 0;
  A.present = ctx->vec[IFEM_VEC_PRESENT].p;
  A.fsi_acc = ctx->indicator.p ? ctx->vec[IFEM_VEC_FSI_ACC].p : nullptr;
  for (int i = 0; i < 3; ++i) A.g[i] = p->gravity[i];
  A.n_neumann = p->n_neumann;
  for (int i = 0; i < 8; ++i) { A.neumann_id[i] = p->neumann_id[i]; A.neumann_p[i] = p->neumann_p[i]; }
}

// fsi.hip -- fluid-side inputs of MPI::FSI (source/mpi_fsi.cpp:96-127,142-223,291-663)
void fsi_set_solid(ifem_ctx *ctx, const ifem_fsi_solid *s);
void fsi_update_indicator(ifem_ctx *ctx, int32_t *host_out, int64_t *n_artificial);
void fsi_find_fluid_bc(ifem_ctx *ctx, double dt, int use_dirichlet_bc, const int32_t *cell_order, ifem_fsi_stats *stats);
void fsi_fluid_at_points(ifem_ctx *ctx, int32_t n, const double *points, double *values, double *stress, int32_t *cell);
void fsi_fluid_at_points_dev(ifem_ctx *ctx, int32_t n, const double *d_pts, double *d_val, double *d_st, int32_t *d_cell); // the same on device arrays, no sync
// api.hip: do the flag arrays of pair k differ (compared on the device); identity of the constrained-dof set `which` after
// its flags changed
void flags_differ(ifem_ctx *ctx, int npairs, const DBuf<uint8_t> *const *a, const DBuf<uint8_t> *const *b, double *out);
void constraint_set_identity(ifem_ctx *ctx, int which, bool differs_self, bool differs_other);
// api.hip: Dirichlet lines (index, value; val == nullptr: all zero) -> flag / value arrays over [0, N) in fresh buffers, zero where no line
// stands.  An index listed twice keeps its LAST line.  kept_*: the lines that stand, last first.  false: an index outside [0, N) -- the
// walk (from the back) stopped there, kept_* hold what it had passed and nothing was built
bool build_line_set(ifem_ctx *ctx, size_t N, int32_t n, const int32_t *idx, const double *val, std::vector<int32_t> &kept_idx,
                    std::vector<double> &kept_val, DBuf<uint8_t> &flag, DBuf<double> &cval);
// api.hip: the Newton loop of run_one_step.  `iteration(nz)` zeroes the update, assembles and solves with the constraint object nz,
// adds the update to the evaluation point and returns ||rhs|| with the two log columns of its system; the loop runs while
// ||rhs|| / ||rhs_0|| > tolerance and ||rhs|| > floor, throws IFEM_E_NEWTON_MAXIT at max_iterations, writes log[4 * outer + 0..3] =
// {||rhs||, relative, log2, log3} and returns the number of iterations.  nz = apply_nonzero in the first iteration, 0 afterwards
struct NewtonIter { double rhs_norm, log2, log3; };
int newton_loop(double floor, int apply_nonzero, double tolerance, int max_iterations, double *log, const std::function<NewtonIter(int)> &iteration);

// assemble_scns.hip
void launch_scns_assemble(ifem_ctx *ctx, const ifem_scns_params *p, int use_nonzero);
void launch_update_stress(ifem_ctx *ctx, double mu);

// sa.hip -- Fluid::MPI::SpalartAllmaras (mpi_spalart_allmaras.cpp) on the velocity nodes; state in ctx->sa
void sa_check(ifem_ctx *ctx);  // refuses what the model does not cover (hanging-node lines)
void sa_ensure(ifem_ctx *ctx); // allocates the state on first use
void sa_set_wall_points(ifem_ctx *ctx, int64_t n_pts, const double *pts);
void sa_set_constraints(ifem_ctx *ctx, int which, int32_t n, const int32_t *node, const double *inhom);
void sa_assemble(ifem_ctx *ctx, const ifem_sa_params *p, int use_nonzero);
void sa_solve(ifem_ctx *ctx, int use_nonzero, uint32_t *iters, double *res_out);
int sa_newton_step(ifem_ctx *ctx, const ifem_sa_params *p, int apply_nonzero, double tolerance, int max_iterations, double *log);
void sa_update_eddy_viscosity(ifem_ctx *ctx, const ifem_sa_params *p, double *host_out);
const double *sa_node_points(ifem_ctx *ctx); // support points of the local nodes [nUl][dim] on the device, built on first use
// sa_wall.hip -- the wall function at a moving FSI wall (mpi_spalart_allmaras.cpp:17-280, mpi_fsi.cpp:782-844); state in ctx->sa.mw
void sa_set_moving_wall(ifem_ctx *ctx, const ifem_sa_wall *w);
void sa_set_shear_velocities(ifem_ctx *ctx, const double *utau);
void sa_update_shear_velocity(ifem_ctx *ctx, const ifem_sa_params *p, double *host_out);
void sa_update_moving_wall_distance(ifem_ctx *ctx, const ifem_sa_params *p, double *host_d, double *host_yplus);
void sa_get_moving_wall(ifem_ctx *ctx, double *host_d, double *host_yplus);
void sa_update_boundary_condition(ifem_ctx *ctx, const ifem_sa_params *p, int first_step, const int32_t *cell_order, int64_t *n_lines);
void sa_get_constraints(ifem_ctx *ctx, int which, uint8_t *flags, double *inhom);
void sa_wall_refresh_d_eff(ifem_ctx *ctx); // d_eff = min(d_mov, d_fixed) again after the fixed distance changed

// scnsex.hip -- Fluid::MPI::SCnsEX (mpi_scnsex.cpp) on scalar node matrices; state in ctx->ex
void scnsex_check(ifem_ctx *ctx); // refuses what the solver does not cover (hanging-node lines, partitioned contexts, Taylor-Hood)
void scnsex_setup(ifem_ctx *ctx, const ifem_scns_params *p);
void scnsex_assemble_rhs(ifem_ctx *ctx, const ifem_scns_params *p, int velocity);
void scnsex_solve(ifem_ctx *ctx, int velocity, uint32_t *iters, double *res_out);
void scnsex_step(ifem_ctx *ctx, const ifem_scns_params *p, double tolerance, int max_iterations, ifem_scnsex_stats *stats);

// linalg.hip -- all on ctx->stream.  Block vectors are [u (dim*nUl) | p (nPl)]; "owned" ranges only.
struct VecLayout {
  int64_t n_u_owned; // dim*nUo
  int64_t p_off;     // dim*nUl
  int64_t n_p_owned; // nPo
};
inline VecLayout layout_of(const ifem_ctx *c) { return {c->dim * c->nUo, c->dim * c->nUl, c->nPo}; }

// y_u = A_uu x_u (+ B^T x_p when xp != nullptr)
void spmv_uu(ifem_ctx *ctx, const double *xu, const double *xp, double *yu, bool use_f32, int part = 0);
// apply_mf.hip: y_u = A_uu x_u without the stored matrix (sum-factorised cell kernel on the state of the last assemble)
// optional epilogue of the matrix-free product t = A_uu x (owned rows), see apply_mf.hip::k_mf_gather: t is consumed instead of
// stored.  mode 1: xs += x, r -= t; mode 2 additionally d = a x + b B r (B = inverse node block, single-precision copy) -- the
// Chebyshev step of the multigrid smoother, d being the owned part of x itself; mode 3: mode 1, then d = b B r into another
// vector d -- the first direction of the smoothing sweep that follows the coarse correction.  In mode 1 the node block is only
// read where a constraint flag needs its diagonal
template <typename V>
struct MfFuseT {
  int mode = 0;
  double a = 0, b = 0;
  V *xs = nullptr, *r = nullptr, *d = nullptr;
  int first = 0; // 1: xs holds nothing yet (the first step of a sweep that starts from zero): xs = x is stored, xs is not read
};
using MfFuse = MfFuseT<double>;
// part (several ranks, build_mf_cell_split): 0 every cell, then the node gather; 1 only the cells whose nodes are all owned
// (no ghost entry of xu is read: the halo may still be in flight); 2 the remaining cells, then the gather
void apply_uu_mf(ifem_ctx *ctx, const double *xu, double *yu, bool single = false, const MfFuse *fuse = nullptr, int part = 0);
// the same on SINGLE-PRECISION vectors, fused form only (the level vectors of the A_uu V-cycle, solver.hip): single-precision
// cell arithmetic, x and the vectors of `fuse` are float
void apply_uu_mf_f32v(ifem_ctx *ctx, const float *xu, const MfFuseT<float> *fuse, int part = 0);
// the plain product on a single-precision input (a Z column of the single-precision inner solver): same cell kernel, fp64 result
void apply_uu_mf_f32in(ifem_ctx *ctx, const float *xu, double *yu, int part = 0);
void uu_lift_mf(ifem_ctx *ctx); // apply_mf.hip: inhomogeneity lift of the right-hand side after a stored_uu = 0 assembly
// scalar velocity operator S^ (IFEM_AINV_SCALAR_GMRES): auxiliary data, SpMV on all components, Jacobi
void shat_refresh(ifem_ctx *ctx, bool f32);
void spmv_shat(ifem_ctx *ctx, const double *xu, double *yu, bool f32);
void shat_jacobi(ifem_ctx *ctx, const double *x, double *y);
// the same masked product for any scalar matrix `val` on the A_uu node pattern (sa.hip, scnsex.hip): ncomp in {1, dim}, flag may be nullptr
void spmv_node_scalar(ifem_ctx *ctx, int ncomp, const double *val, const uint8_t *flag, const double *diag, const double *x, double *y);
// y_p = B x_u
// `part` of the row-parallel products below: 0 all rows, 1 the rows that read owned columns only, 2 the others (several
// ranks: 1 runs while the halo of x is in flight, 2 after halo_wait; see PlanarCsr::split_rows)
void build_row_split(ifem_ctx *ctx, PlanarCsr &M, int64_t n_owned_cols, const PlanarCsr *M2 = nullptr, int64_t n_owned_cols2 = 0);
void spmv_b(ifem_ctx *ctx, const double *xu, double *yp, int part = 0, const double *val = nullptr); // val: other values on the pattern of B (the unconstrained block)
// y_u = B^T x_p
void spmv_bt(ifem_ctx *ctx, const double *xp, double *yu);
void spmv_b_f32(ifem_ctx *ctx, const double *xu, double *yp);  // same with single-precision copies of the values
void spmv_bt_f32(ifem_ctx *ctx, const double *xp, double *yu); // (matrix-free S_m inside the preconditioner only)
// y_p = A_pp x_p (SCnsIM pressure block on the M_p pattern); 1/diag(A_pp) for its Jacobi preconditioner
void spmv_app(ifem_ctx *ctx, const double *xp, double *yp);
void app_diag_setup(ifem_ctx *ctx);
void sm_diag_from_blocks(ifem_ctx *ctx, const double *dinv_mu_ext, double *d); // diag(B diag(M_u)^-1 B^T), owned pressure rows
void scalar_diag(ifem_ctx *ctx, const PlanarCsr &M, const double *val, double *d);
// y_p = M_p x_p
void spmv_mp(ifem_ctx *ctx, const double *xp, double *yp, int part = 0, bool use_f32 = false);
// mp_direct.hip: x = M_p^-1 b by tensor-product line solves on a uniform box level.  mp_direct_ready: the context qualifies, its tables are
// built and the present M_p values have passed the probe against the assembled matrix (decides, builds and probes on demand; false: CG).
// mp_direct_apply: the three sweeps on device vectors in the caller's node order (b and x may be the same vector)
bool mp_direct_ready(ifem_ctx *ctx, int verbose);
void mp_direct_apply(ifem_ctx *ctx, const double *b, double *x);
// its host-side setup, plain C++: the Thomas factors of h tridiag(1/6, 2/3, 1/6) with end diagonals 1/3
void mpd_thomas_factors(int n, double h, std::vector<double> &rpiv, std::vector<double> &mult);
// setup.hip: the pressure nodes of this context as a full lattice (ctx.hpp::PLattice; host side lattice.hpp), decided and built on first use
bool p_lattice_ensure(ifem_ctx *ctx);
// explicit S_m: numeric product B diag(1/diag M_u) B^T into ctx->Sm (pattern must exist), and y_p = S_m x_p
void schur_numeric(ifem_ctx *ctx);
void spmv_sm(ifem_ctx *ctx, const double *xp, double *yp, bool use_f32, int part = 0);
void spmv_sm_rows(ifem_ctx *ctx, const double *xp, double *yp, int64_t n_list, const int32_t *rows); // the listed rows only, fp64 values
// sm_stencil.hip: y = S_m x from stencil tables over the pressure lattice of a uniform box level.  sm_stencil_setup: set-up time only (allocates,
// synchronises): (re)builds and probes the tables when S_m was re-formed since it last looked.  sm_stencil_ready: sm_apply may take
// sm_stencil_apply (no allocation, capture-safe).
void sm_stencil_setup(ifem_ctx *ctx, int verbose);
inline bool sm_stencil_ready(const ifem_ctx *ctx) { return ctx->sm_stencil.ready && !ctx->sm_stencil.off && ctx->sm_stencil.version == ctx->sm_version; }
void sm_stencil_apply(ifem_ctx *ctx, const double *x, double *y);
// sm_direct.hip: x = S_m^-1 b by fast diagonalisation (ifem_solver_opts::sm_mg = 2).  sm_direct_setup: set-up time only, after sm_stencil_setup
// (allocates, synchronises): decides the level, builds the factors of a new key and probes them against the present S_m whenever S_m was
// re-formed since it last looked.  sm_direct_ready: solve_sm may take sm_direct_apply (seven launches, no allocation; b and x may not alias)
void sm_direct_setup(ifem_ctx *ctx, int verbose);
inline bool sm_direct_ready(const ifem_ctx *ctx) { return ctx->sm_direct.ready && ctx->sm_direct.version == ctx->sm_version; }
void sm_direct_apply(ifem_ctx *ctx, const double *b, double *x);
void sm_solve_probe(ifem_ctx *ctx, const ifem_solver_opts *o, const double *b, double *x, int64_t info[4]); // ifem_test_sm_solve on device vectors
// bb_stencil.hip: y = B x and y (+)= B^T x from stencil tables over the pressure and velocity lattices of a uniform box level.  bb_stencil_setup:
// solve set-up only (allocates, synchronises): (re)builds and probes the tables of both blocks when an assembly wrote them since it last looked
// (ifem_ctx::bb_version).  bb_stencil_ready(which: 0 B, 1 B^T): spmv_b / spmv_bt / the B^T arm of spmv_uu take the stencil product (no
// allocation, capture-safe).
bool u_lattice_ensure(ifem_ctx *ctx); // setup.hip: the velocity nodes as a full lattice (ctx.hpp::ULattice), decided and built on first use
void bb_stencil_setup(ifem_ctx *ctx, int verbose);
inline bool bb_stencil_ready(const ifem_ctx *ctx, int which) {
  const BbStencil &T = ctx->bb_stencil;
  return !T.off && T.version == ctx->bb_version && (which ? T.bt.ready : T.b.ready);
}
void bb_stencil_apply_b(ifem_ctx *ctx, const double *xu, double *yp);
void bb_stencil_apply_bt(ifem_ctx *ctx, const double *xp, double *yu, bool add);
void spmv_b_rows(ifem_ctx *ctx, const double *xu, double *yp, int64_t n_list, const int32_t *rows); // the listed rows only, fp64 values
void spmv_bt_rows(ifem_ctx *ctx, const double *xp, double *yu, int64_t n_list, const int32_t *rows, bool add);
// y_u = d .* x_u (diagonal scaling with 1/diag(M_u))
void vec_mul(ifem_ctx *ctx, int64_t n, const double *d, const double *x, double *y);
void vec_div(ifem_ctx *ctx, int64_t n, const double *d, const double *x, double *y); // y = x ./ d (d == 0 -> 1)
// y = bjac * x  (node-block Jacobi)
void bjac_apply(ifem_ctx *ctx, const double *x, double *y);
const float *bjac_f32_ptr(ifem_ctx *ctx); // single-precision copy of the inverse node blocks (refreshed on demand)
void bjac_setup(ifem_ctx *ctx);
void dinv_setup(ifem_ctx *ctx);

// generic vector kernels over one contiguous range
void v_axpy(ifem_ctx *ctx, int64_t n, double a, const double *x, double *y);            // y += a x
void v_axpby(ifem_ctx *ctx, int64_t n, double a, const double *x, double b, double *y); // y = a x + b y
void v_scale(ifem_ctx *ctx, int64_t n, double a, double *x);
void v_copy(ifem_ctx *ctx, int64_t n, const double *x, double *y);
void v_scale_to(ifem_ctx *ctx, int64_t n, double a, const double *x, double *y); // y = a x
void v_scale_to2(ifem_ctx *ctx, int64_t n, double a, const double *x, double *y, double *z); // y = z = a x
void v_zero(ifem_ctx *ctx, int64_t n, double *x);
double v_dot(ifem_ctx *ctx, int64_t n, const double *x, const double *y); // local (no all-reduce), syncs
// multi-dot: out[i] = <V_i, w> for i < k (V column-major with leading dimension ld), one pass, syncs
void v_mdot(ifem_ctx *ctx, int64_t n, int k, const double *V, int64_t ld, const double *w, double *out_host, bool all_ranks = false);
// w -= sum_i h[i] V_i
void v_maxpy(ifem_ctx *ctx, int64_t n, int k, const double *V, int64_t ld, const double *h_host, double *w, double *norm2_out = nullptr,
             bool all_ranks = false);
// single-precision Krylov basis (inner solver): V float, w / coefficients / accumulation double
void v_mdot_f32(ifem_ctx *ctx, int64_t n, int k, const float *V, int64_t ld, const double *w, double *out_host);
void v_maxpy_f32(ifem_ctx *ctx, int64_t n, int k, const float *V, int64_t ld, const double *h_host, double *w, double *norm2_out);
void v_scale_store_f32(ifem_ctx *ctx, int64_t n, double a, const double *w, float *v);
void bjac_apply_f32(ifem_ctx *ctx, const float *x, double *y);
// CG with device-resident recurrence scalars (single rank): init, alpha = rz / <p,q>, update of x, r, z, p; cgd_rr syncs
void cgd_init(ifem_ctx *ctx, int64_t n, const double *b, const double *diag, double *x, double *r, double *z, double *p);
void cgd_alpha(ifem_ctx *ctx, int64_t n, const double *p, const double *q);
void cgd_update(ifem_ctx *ctx, int64_t n, const double *diag, double *p, const double *q, double *x, double *r, double *z);
double cgd_rr(ifem_ctx *ctx);
// the same recurrence with one fused reduction per iteration (Chronopoulos / Gear): u = D^-1 r (u == r without diag), w = A u, s = A p
void cg1_init(ifem_ctx *ctx, int64_t n, const double *b, const double *diag, double *x, double *r, double *u, double *p, double *s);
void cg1_dots(ifem_ctx *ctx, int64_t n, const double *r, const double *u, const double *w, bool first);
void cg1_update(ifem_ctx *ctx, int64_t n, const double *diag, double *u, const double *w, double *p, double *s, double *x, double *r);
void v_minmax(ifem_ctx *ctx, int64_t n, const double *x, double *mn, double *mx);
// the comparison of a set-up probe on the device: got -= ref, *ref_max = max |ref|, *err = max |got - ref|; false: one of them is not finite
// (an entry nobody produced, a NaN in either vector).  Synchronises; three scalars come back.
bool v_probe_diff(ifem_ctx *ctx, int64_t n, const double *ref, double *got, double *ref_max, double *err);
// test aid (ifem_test_cg_device): solver.hip::cg_device on A = diag(a), host arrays in and out, exactly `iters` iterations
void test_cg_device(ifem_ctx *ctx, int64_t n, const double *a, const double *jac, const double *b, int iters, double *x);
// x[dof] = value for constrained dofs (AffineConstraints::distribute, Dirichlet lines) of the fluid set `which`; the launch itself on any
// flag / value arrays: x is compact [u (n_u_owned) | p (n_owned - n_u_owned)], the arrays hold the p part at p_off_ext
void apply_constraints(ifem_ctx *ctx, int which, double *x);
void distribute_lines(ifem_ctx *ctx, int64_t n_u_owned, int64_t n_owned, int64_t p_off_ext, const uint8_t *is_c, const double *cval, double *x);
void spmv_planar_scalar(ifem_ctx *ctx, const PlanarCsr &M, const double *val, const double *xp, double *yp);
// explicit pressure Schur complement of the SUPG block preconditioner (tpp.hip)
void tpp_numeric(ifem_ctx *ctx);
void spmv_tpp(ifem_ctx *ctx, const double *xp, double *yp);
bool tpp_ilu_factor(ifem_ctx *ctx); // false: zero / tiny / non-finite pivot (ctx->tpp_ilu.broken): do not apply the factors
void tpp_ilu_apply(ifem_ctx *ctx, const double *x, double *y);
int tpp_ilu_levels(const ifem_ctx *ctx);
void schur_pp_numeric(ifem_ctx *ctx, const double *binv, double *out); // out = A_pp - A_pv blockdiag(binv) A_vp on the pattern of T_pp
const PlanarCsr &tpp_pattern(ifem_ctx *ctx);                          // that pattern (built on first use)
// ILU(0) with dim x dim blocks, natural order, Jacobi-sweep application (bilu.hip)
void bilu_analyse(ifem_ctx *ctx, BIlu &I, int dim, int64_t n, const int64_t *rp_dev, const int32_t *col_dev);
bool bilu_factor(ifem_ctx *ctx, BIlu &I, const double *src);
void bilu_apply(ifem_ctx *ctx, BIlu &I, int sweeps, const double *x, double *y);
void rowsum_abs_inv(ifem_ctx *ctx, double *out);
void scns_refpc_setup(ifem_ctx *ctx, int verbose, bool *pvv_ok, bool *b2_ok);
void scns_pc_probe(ifem_ctx *ctx, int which, const double *x, double *y);
// kelly.hip, transfer.hip -- the two device passes of FluidSolver::refine_mesh (ifem_hip.h: ifem_kelly_estimate, ifem_transfer_solution)
void kelly_estimate(ifem_ctx *ctx, const double *x, const int32_t *face_table); // result in ctx->kelly.eta
void transfer_solution(ifem_ctx *src, ifem_ctx *dst, int vec, const int32_t *u_cell, const int32_t *u_pos, const int32_t *p_cell,
                       const int32_t *p_pos);
// hanging-node lines (hanging.hip): C x on a copy of x, C^T and the hanging rows on y, distribute, set-up
void hanging_set(ifem_ctx *ctx, int32_t n, const int32_t *dof, const int32_t *ptr, const int32_t *master, const double *weight);
const double *hanging_input(ifem_ctx *ctx, const double *x); // ghost-extended [u_l | p_l] copy of x with C applied
void hanging_output(ifem_ctx *ctx, const double *x, bool x_extended, double *y);
void hanging_distribute(ifem_ctx *ctx, double *x);
void hanging_refresh_diag(ifem_ctx *ctx);
bool hanging_offset(ifem_ctx *ctx, int use_nonzero);
void hanging_condense_rhs(ifem_ctx *ctx, int use_nonzero); // solver.hip: b = C^T (b^ - A^ c0), hanging rows d c0

// mg.hip: transfers and smoother updates of the multigrid inside the preconditioner
void mg_csr_apply(ifem_ctx *ctx, const MgCsr &M, const double *x, double *y);
void cheb_init(ifem_ctx *ctx, int64_t n, double c0, const double *dinv, const double *r, double *d);
void cheb_step(ifem_ctx *ctx, int64_t n, double a, double b, const double *dinv, const double *t, double *x, double *r, double *d);
void vec_recip(ifem_ctx *ctx, int64_t n, double *d);
void vec_rough(ifem_ctx *ctx, int64_t n, int64_t offset, double *x);
void uu_block_diag_mf(ifem_ctx *ctx); // ctx->bjac := inverse node blocks of the matrix-free A_uu (coarse multigrid levels)
void mg_csr_mask(ifem_ctx *ctx, const MgCsr &M, const uint8_t *flag_in, const uint8_t *flag_out, DBuf<uint8_t> &mask);
void mg_inject_nodes(ifem_ctx *ctx, int64_t n_nodes, const int32_t *inj, const double *fine, double *coarse);
void cheb_init_block_f32(ifem_ctx *ctx, double c0, const float *r, float *d);
void mg_csr_apply_nodes_f32(ifem_ctx *ctx, const MgCsr &M, const float *x, const DBuf<uint8_t> &mask, float *y);
// mg_lattice.hip: the velocity transfers of the pair (c, c->mg_coarse) of the A_uu V-cycle.  mg_transfer_u_setup: set-up time only (allocates,
// synchronises): the packed CSR entries for the constrained-dof set cs of the two levels, and (mg_lattice_u_setup, once per ifem_mg_attach) the
// decision whether the pair may take its weights from the lattice formula.  mg_transfer_u: what the cycle launches (prolong: coarse x -> fine y,
// else fine x -> coarse y; no allocation, capture-safe): the lattice kernels where the pair passed and ifem_tuning::mg_lattice_u is on,
// mg_csr_apply_nodes_f32 elsewhere or with csr_only
void mg_transfer_u_setup(ifem_ctx *c, int cs, int verbose);
void mg_lattice_u_setup(ifem_ctx *c, int verbose);
inline bool mg_lattice_u_active(const ifem_ctx *c) { return c->mg_lattice_u.state == 1 && c->tune.mg_lattice_u != 0; }
void mg_transfer_u(ifem_ctx *c, bool prolong, const float *x, float *y, bool csr_only = false);
void v_cvt_d2f(ifem_ctx *ctx, int64_t n, const double *x, float *y);
void v_cvt_f2d(ifem_ctx *ctx, int64_t n, const float *x, double *y);
void v_axpy_f32v(ifem_ctx *ctx, int64_t n, float a, const float *x, float *y);
// entry and exit of the A_uu V-cycle (ifem_tuning::inner_f32): r = float(src), d = c0 B r in one pass; out = x + d
void vc_entry(ifem_ctx *ctx, double c0, const double *src, float *r, float *d);
void vc_entry_f32(ifem_ctx *ctx, double c0, const float *src, float *r, float *d);
void vc_exit(ifem_ctx *ctx, int64_t n, const float *x, const float *d, double *out);
void vc_exit_f32(ifem_ctx *ctx, int64_t n, const float *x, const float *d, float *out);

// patch.hip: the vertex-patch smoother B = sum_v R_v^T A_v^-1 R_v of a level (ifem_tuning::uu_smoother = 1): shared inverses per patch type on a
// uniform box level, one inverse per patch on the others (ifem_tuning::uu_patch_levels = 1)
bool patch_eligible(const ifem_ctx *ctx);  // Q2 velocity, one rank, no hanging-node lines; a uniform box level, or uu_patch_levels = 1
bool patch_setup(ifem_ctx *ctx);           // tables for the level's operator state (cached on its key); false: not eligible (or beyond a cap of its form)
void patch_apply(ifem_ctx *ctx, double a, double b, const float *r, float *d); // d = a d + b B r, one launch per colour
inline bool patch_active(const ifem_ctx *c) { return c->tune.uu_smoother == 1 && c->patch.eligible && c->patch.valid; }

// all-reduce helpers (identity for a single rank)
void allreduce_sum(ifem_ctx *ctx, double *host_vals, int n);
void allreduce_max(ifem_ctx *ctx, double *host_vals, int n);
void allreduce_sum_dev(ifem_ctx *ctx, double *dev_vals, int n); // device scalars, in place, stream-ordered
// sum of a device VECTOR over the ranks, in place, stream-ordered (the hand-over to a replicated coarse level); scratch: n entries
void allreduce_sum_vec(ifem_ctx *ctx, double *dev, int64_t n, double *scratch);
void allreduce_sum_vec_f32(ifem_ctx *ctx, float *dev, int64_t n, float *scratch);
int comm_unique_id(uint8_t out[128]);
int comm_selftest(int device);
void comm_stats(ifem_ctx *ctx, ifem_comm_stats *out, bool reset, bool single_level = false);
void *local_world_create(int nranks);
void local_world_destroy(void *w);
// ghost refresh of a ghost-extended velocity buffer [dim*nUl] / pressure buffer [nPl] (RCCL send/recv over xGMI)
void halo_exchange(ifem_ctx *ctx, double *xu_ext);
void halo_exchange_p(ifem_ctx *ctx, double *xp_ext);
// ghost entries of nodal plane fields f[nplanes][nUl] := the owners' values, through the velocity halo plan (dim planes per exchange)
void halo_refresh_nodal(ifem_ctx *ctx, int nplanes, double *f);
// transpose: ghost entries are sent back to their owners and added there (C^T of hanging lines across ranks)
void halo_reverse_add(ifem_ctx *ctx, double *xu_ext);
// single-precision velocity vectors (level vectors of the A_uu V-cycle): same plans, half the bytes
void halo_exchange_f32(ifem_ctx *ctx, float *xu_ext);
void halo_reverse_add_f32(ifem_ctx *ctx, float *xu_ext);
void halo_start_f32(ifem_ctx *ctx, float *xu_ext);
void halo_reverse_add_p(ifem_ctx *ctx, double *xp_ext);
// overlapped form: halo_start (pack + transfers on the halo stream), work that reads no ghost entry, halo_wait
bool halo_overlap_ok(const ifem_ctx *ctx);
void halo_start(ifem_ctx *ctx, double *x_ext, int which); // which: 0 velocity, 1 pressure, 2 the 2-deep halo of S_m
void halo_wait(ifem_ctx *ctx);
void halo_exchange_s(ifem_ctx *ctx, double *xs_ext); // [n_s_cols]: owned pressure nodes, then the 2-deep far nodes
void build_schur_pattern_box(ifem_ctx *ctx);          // distributed explicit S_m on a structured pressure lattice
void schur_probe_fill(ifem_ctx *ctx, int color, const double *y); // S_m[i, j(color)] = y_i
void schur_probe_vector(ifem_ctx *ctx, int color, double *x);     // x_i = [color(i) == color]
void comm_init(ifem_ctx *ctx, const ifem_partition *part);
void comm_destroy(ifem_ctx *ctx);

// solver.hip
// (a Krylov solve that misses its tolerance throws IFEM_E_KRYLOV_NOCONV through throw_noconv: SolverControl::NoConvergence)
[[noreturn]] void throw_noconv(const char *solver, int it, double res, double tol);
void ins_solve(ifem_ctx *ctx, const ifem_ins_params *P, const ifem_solver_opts *o, int use_nonzero, ifem_solve_stats *stats);
void ins_precond_vmult(ifem_ctx *ctx, const ifem_ins_params *P, const ifem_solver_opts *o, const double *src, double *dst);
void ins_system_vmult(ifem_ctx *ctx, const double *src, double *dst);
// test aid (ifem_test_mp_solve): solve_mp under `o` on device vectors of nPo entries; info = {1 direct / 0 CG, CG iterations}
void mp_solve_probe(ifem_ctx *ctx, const ifem_solver_opts *o, const double *b, double *x, int32_t info[2]);
void sm_apply_probe(ifem_ctx *ctx, int path, const double *x, double *y, int64_t info[4]); // ifem_test_sm_apply on device vectors
void b_apply_probe(ifem_ctx *ctx, int which, int path, const double *x, double *y, int64_t info[4]); // ifem_test_b_apply on device vectors
void scns_solve(ifem_ctx *ctx, const ifem_solver_opts *o, int use_nonzero, ifem_solve_stats *stats);
// y = A_uu z on a compact owned SINGLE-PRECISION column (ghosts refreshed on a float copy), single-precision cell arithmetic, fp64 result
void uu_apply_f32col(ifem_ctx *ctx, const float *z, double *y);

// owned-range dot over a block vector (u range + p range), all-reduced
double bv_dot(ifem_ctx *ctx, const double *x, const double *y);
inline int64_t bv_len(const ifem_ctx *c) { return c->n_local; }

} // namespace ifem
