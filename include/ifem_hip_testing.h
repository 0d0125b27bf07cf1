/*
 * ifem_hip_testing.h -- TEST AIDS of libifem_hip.so.  Not part of the drop-in surface (include/ifem_hip.h): nothing here replaces
 * a member of the reference's FluidSolver hierarchy; the parity tests use these entry points to look at intermediate objects
 * of the SCnsIM block preconditioner (mpi_supg_solver.cpp:35-192) that the reference keeps private.
 */
#ifndef IFEM_HIP_TESTING_H
#define IFEM_HIP_TESTING_H
#include "ifem_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Test hook of the SCnsIM preconditioner (single-rank contexts, after ifem_scns_assemble): forms the explicit
 * T_pp = A_pp - A_pv P_vv^-1 A_vp and its ILU(0) (ifem_tuning::tpp_ilu_order) as ifem_scns_solve would.  Call with rowptr only
 * to size the arrays (n_p + 1 entries, nnz = rowptr[n_p]); with col / val it also returns the CSR of T_pp, and with x / y
 * (host, n_p entries) y = (LU)^-1 x.  *levels (may be NULL) receives the number of forward levels of the schedule. */
int ifem_tpp_ilu_probe(ifem_ctx *ctx, int64_t *rowptr, int32_t *col, double *val, const double *x, double *y, int32_t *levels);
/* Test aid: replace the values of the explicit T_pp (pattern and order as returned by ifem_tpp_ilu_probe) so that the next
 * factorisation sees them -- the breakdown path of the ILU(0) (zero / non-finite pivot -> IFEM_E_KRYLOV_NOCONV from the probe, Jacobi
 * in ifem_scns_solve) cannot be reached from an assembled fluid matrix at will. */
int ifem_tpp_override(ifem_ctx *ctx, const double *val); /* TEST AID ONLY: single rank, not part of the reference's interface */

/* The pieces of the reference-structure preconditioner (ifem_tuning::scns_pc = 2; single-rank contexts, after ifem_scns_assemble),
 * host vectors in the compact owned layout:
 *   which = 0: y = P_vv^-1 x, the ILU(0) of A_vv          (n = dim * n_unodes; mpi_supg_solver.cpp:49-51)
 *   which = 1: y = B2pp_inverse x, the ILU(0) of B2pp     (n = n_pnodes; :133)
 *   which = 2: y = B2pp x, B2pp = A_pp - A_pv rowsum(|A_vv|)^-1 A_vp   (:56-132)
 *   which = 3: y = T_pp x = A_pp x - A_pv P_vv^-1 A_vp x  (:19-32)
 * ifem_tuning::pvv_sweeps / b2pp_sweeps < 0 make the two ILU applications exact substitutions. */
int ifem_scns_pc_probe(ifem_ctx *ctx, int which, const double *x, double *y);

/* Stand-in for the free-memory bound of the self-lengthening inner restart (solver.hip::precond_vmult) on THIS rank: `columns` > 0 is
 * the number of basis column pairs this rank says it can afford, 0 restores the hipMemGetInfo estimate.  The decision itself is
 * collective (the smallest wish of all ranks wins): a test gives the ranks different bounds and checks that they agree. */
int ifem_test_restart_fits(ifem_ctx *ctx, int columns);

/* Which matrix-free A_uu kernels this context launches: returns 1 for the constant-geometry variants (every local cell is the same
 * axis-aligned box and ifem_tuning::mf_uniform is on), 0 for the general ones, < 0 on error.  h (may be NULL) receives the three edge
 * lengths the context detected (zeros: not a uniform box level; entries past dim are zero), whatever the tuning says. */
int ifem_test_mf_uniform(ifem_ctx *ctx, double *h);

/* How the last full assembly of the context wrote A_uu (ifem_tuning::asm_rows, csrc/assemble_rows.hip): *state = 1 the row owners ran, -1 they
 * were asked for and refused (the cell kernel scattered with atomics, as with asm_rows = 0), 0 not asked or no full assembly yet.  verbose != 0:
 * a refusal is named in one line on stderr. */
int ifem_test_asm_rows(ifem_ctx *ctx, int verbose, int32_t *state);

/* The cell-independent terms of the element matrix that the row owners take from a table instead of contracting them (csrc/assemble_rows.hip,
 * k_rows_const): runs the table kernel for the context's box and the parameters p and returns the table without its MFMA padding,
 *   out[(a * 27 + b) * 9 + 3 c + d] = sum_q w_q (gamma rho d_c N_a d_d N_b + delta_cd mu grad N_a . grad N_b), imex != 0: + delta_cd rho/dt N_a N_b,
 * a, b = local velocity nodes a_x + 3 a_y + 9 a_z.  Needs a created context of a uniform 3D Q2 box (IFEM_E_BADPARAM elsewhere), no assembly. */
int ifem_test_rows_const(ifem_ctx *ctx, const ifem_ins_params *p, int imex, double *out /* 27*27*9 */);

/* y_u = A_uu x_u on the velocity part of two context vectors as the single-precision inner solver of IFEM_AINV_MG forms the product
 * (ifem_tuning::inner_f32; solver.hip::uu_apply_f32col): x rounded to float, its ghost entries exchanged as float, single-precision
 * cell arithmetic, fp64 result.  After ifem_ins_assemble / ifem_imex_assemble.  Stages the column in a level vector of the A_uu V-cycle and
 * may (re)allocate it: a captured cycle of the context is then captured anew at its next use. */
int ifem_test_uu_vmult_f32col(ifem_ctx *ctx, int dst, int src);

/* The vertex-patch smoother of ifem_tuning::uu_smoother = 1 (patch.hip) for the operator state of the last ifem_ins_assemble /
 * ifem_imex_assemble, whatever uu_smoother says (a level that is not a uniform box takes part only with ifem_tuning::uu_patch_levels = 1; there
 * out[2] is the number of stored inverses, one per patch).  ifem_test_uu_patch_vmult: velocity part of the context vector dst = B times the velocity
 * part of src (src rounded to float, single-precision product, as inside the V-cycle); IFEM_E_BADPARAM on a level that is not eligible.
 * ifem_test_uu_patch_info: out = {eligible (0 / 1), patches, patch types, bytes of the inverse tables}; the last three are 0 before an assembly
 * or on a level that is not eligible.  Both build the tables when they are not there yet. */
int ifem_test_uu_patch_vmult(ifem_ctx *ctx, int dst, int src);
int ifem_test_uu_patch_info(ifem_ctx *ctx, int64_t out[4]);

/* ONE host launcher of the Krylov vector kernels (linalg.hip, as declared in kernels.hpp: the dispatch between the kernels is part of what
 * runs) on host data: device scratch, upload, the call, a stream synchronisation, download.  Needs a created context only (single rank; all_ranks
 * is passed as the solvers pass it and is the identity there).  n entries per vector, columns ld >= n entries apart; w: n doubles.
 *   IFEM_TVK_MDOT            out[i] = <V_i, w>, i < k                          V: k double columns
 *   IFEM_TVK_MDOT_SELF       out[0] = <w, w> through the aliased call v_mdot(n, 1, w, n, w)
 *   IFEM_TVK_MAXPY[_NORM]    w -= sum_i coef[i] V_i  [out[0] = ||w||^2 of the result]   V: k double columns
 *   IFEM_TVK_MDOT_F32        as MDOT                                            V: pad4(k) float columns, pad4(k) = (k + 3) & ~3
 *   IFEM_TVK_MAXPY_F32[_NORM]  as MAXPY[_NORM]                                  V: pad4(k) float columns
 *   IFEM_TVK_SCALE_STORE_F32 V (n floats) = float(coef[0] * w)
 *   IFEM_TVK_AXPY            w += coef[0] V_0                                   V: one double column
 *   IFEM_TVK_AXPBY           w = coef[0] V_0 + coef[1] w                        V: one double column
 *   IFEM_TVK_SCALE_TO2       V_0 = V_1 = coef[0] w                              V: two double columns (output)
 *   IFEM_TVK_DIV             w = w ./ V_0 (a zero divisor counts as 1)          V: one double column
 *   IFEM_TVK_MINMAX          out[0] = min w, out[1] = max w
 * Arguments an op does not use may be NULL. */
enum {
  IFEM_TVK_MDOT = 0, IFEM_TVK_MDOT_SELF, IFEM_TVK_MAXPY, IFEM_TVK_MAXPY_NORM, IFEM_TVK_MDOT_F32, IFEM_TVK_MAXPY_F32, IFEM_TVK_MAXPY_F32_NORM,
  IFEM_TVK_SCALE_STORE_F32, IFEM_TVK_AXPY, IFEM_TVK_AXPBY, IFEM_TVK_SCALE_TO2, IFEM_TVK_DIV, IFEM_TVK_MINMAX, IFEM_TVK_COUNT
};
int ifem_test_vec_kernel(ifem_ctx *ctx, int op, int64_t n, int k, int64_t ld, void *V, const double *coef, double *w, double *out);

/* The device-resident CG of the pressure solves (krylov.hip::cg_device; ifem_tuning::cg_single_reduction selects the form, as in production) on
 * A = diag(a) (applied through vec_mul), zero initial guess: x (n doubles, host) = the iterate after exactly `iters` iterations (tolerance 0, the
 * residual read every iteration, the work vector of the single-reduction form present).  jac (may be NULL): the Jacobi diagonal; a zero entry
 * counts as 1.  Single rank, a created context only. */
int ifem_test_cg_device(ifem_ctx *ctx, int64_t n, const double *a, const double *jac, const double *b, int iters, double *x);

/* ONE matrix-free product t = A_uu x with the epilogue of its node gather (apply_mf.hip::k_mf_gather, kernels.hpp::MfFuseT) on host vectors of
 * dim * n_unodes doubles, for the operator state of the last ifem_ins_assemble / ifem_imex_assemble.  Single rank.
 *   prec 0: double cell arithmetic, double vectors; 1: single-precision cell arithmetic and float vectors (the level vectors of the A_uu V-cycle;
 *   the host vectors are rounded to float and returned widened); 2: single-precision cell arithmetic, double vectors
 *   mode 0: d = t (the plain form; xs, r unused)     mode 1: xs += x, r -= t (d unused, may be NULL)
 *   mode 2: mode 1, then d = a x + b B r, formed in place in the device copy of x as the smoother does     mode 3: mode 1, then d = b B r
 *   first != 0: xs = x is stored and the incoming xs not read
 * block_cap > 0 caps the gather's blocks for this call, so that a small mesh gives one block several chunks of nodes; geo (may be NULL) receives
 * {chunks, blocks} of the gather launch. */
int ifem_test_uu_fused_product(ifem_ctx *ctx, int prec, int mode, int first, double a, double b, const double *x, double *xs, double *r, double *d,
                               int block_cap, int64_t geo[2]);

/* The host launchers of the multigrid kernels (mg.hip, as declared in kernels.hpp: the dispatch inside them is part of what runs), ONE per call, on
 * host data: device scratch, upload, the call, a stream synchronisation, download.  Single-rank contexts.  Every array an op WRITES has
 * IFEM_TMG_PAD more entries than the op may touch; on the device the whole array starts as 0xff bytes (NaN) and comes back whole: an entry the op
 * left out is NaN, and so is the padding unless the op wrote past its end.  Single-precision device vectors cross the interface as doubles, rounded
 * on the way in and widened on the way out.
 *
 * ifem_test_mg_transfer: a CSR transfer table of n_rows x n_cols (ptr: n_rows + 1, col / w: ptr[n_rows] entries), checked on the host as
 * ifem_mg_attach checks its tables (spanning, non-decreasing, columns in range, n_cols < 2^29); needs a created context only, whose dim selects the
 * node kernels.
 *   kind 0: y = W x by mg_csr_apply, the scalar transfer of the S_m cycle: x n_cols doubles, y n_rows (+ pad) doubles, fp64 weights
 *   kind 1: mg_csr_mask, then mg_csr_apply_nodes_f32, the node transfer of the A_uu cycle: x n_cols * dim, y n_rows * dim (+ pad), both float on the
 *           device; flag_in [n_cols * dim] / flag_out [n_rows * dim] (either may be NULL): non-zero drops that component of the column / row node */
enum { IFEM_TMG_PAD = 8 };
int ifem_test_mg_transfer(ifem_ctx *ctx, int kind, int64_t n_rows, int64_t n_cols, const int64_t *ptr, const int32_t *col, const double *w,
                          const uint8_t *flag_in, const uint8_t *flag_out, const double *x, double *y);

/* ifem_test_mg_lattice_transfer: one velocity transfer of the A_uu V-cycle between `fine` and the level attached below it (ifem_mg_attach with
 * velocity tables), on host vectors that are float on the device, with the Dirichlet flags of the two levels (the constraint object of the last
 * assembly of `fine`, object 0 before any; the coarse level is set to the same object, as the set-up of a cycle does).  No exchange is made: on
 * several ranks every rank multiplies what it is given.
 *   which 0: prolongation, x dim * local velocity nodes of the coarse level, y dim * owned velocity nodes of `fine` (+ IFEM_TMG_PAD)
 *   which 1: restriction, x dim * owned nodes of `fine`, y dim * local nodes of the coarse level (+ IFEM_TMG_PAD)
 *   path 0: the CSR kernels on the attached tables (mg_csr_mask + mg_csr_apply_nodes_f32)
 *   path 1: what a cycle launches: the lattice-formula kernels (csrc/mg_lattice.hip) where the pair passed its checks and
 *           ifem_tuning::mg_lattice_u is on, the CSR kernels elsewhere
 * Decides the pair when that has not happened since the attach, as the set-up of a solve would.
 * info = {state of the pair: 1 lattice formula / -1 keeps CSR, rows of P_u that differ from the formula, rows of R_u that do (-1 each: not
 * compared, the pair was not eligible), 1: this call ran the lattice kernels / 0} */
int ifem_test_mg_lattice_transfer(ifem_ctx *fine, int which, int path, const double *x, double *y, int64_t info[4]);

/* ifem_test_mg_vec_kernel: the vector kernels of the two V-cycles on n entries (outputs: n + IFEM_TMG_PAD).  [f]: float on the device.
 *   IFEM_TMG_CHEB_INIT            out0 = coef[0] in0 in1                                  in0 = D^-1, in1 = r
 *   IFEM_TMG_CHEB_STEP            out0 += out2, out1 -= in1, out2 = coef[0] out2 + coef[1] in0 out1      in0 = D^-1, in1 = t; out0 / out1 / out2 = x / r / d,
 *                                 in and out; in0 and in1 return what the device holds after the call (they must come back unchanged)
 *   IFEM_TMG_VEC_RECIP            out0 = 1 / out0, a zero gives 1 (in place)
 *   IFEM_TMG_VEC_ROUGH            out0 = the rough start vector of the power iteration, offset m
 *   IFEM_TMG_CVT_D2F              out0 [f] = in0                IFEM_TMG_CVT_F2D   out0 = in0 [f]
 *   IFEM_TMG_AXPY_F32V            out0 [f] += float(coef[0]) in0 [f] (in place)
 *   IFEM_TMG_VC_EXIT              out0 = in0 [f] + in1 [f]      IFEM_TMG_VC_EXIT_F32   the same with out0 [f]
 *   IFEM_TMG_INJECT_NODES         out0 [n * dim] = in0 [m * dim] at the nodes idx [n] (values in [-1, m); -1 gives zeros): n coarse, m fine nodes
 * the node-block ops read the inverse node blocks of the context (ifem_uu_block_diag(ctx, 0, .)): after an assembly, n = dim * n_unodes
 *   IFEM_TMG_VC_ENTRY             out0 [f] = in0, out1 [f] = coef[0] B out0               IFEM_TMG_VC_ENTRY_F32   the same with in0 [f]
 *   IFEM_TMG_CHEB_INIT_BLOCK_F32  out0 [f] = coef[0] B in0 [f]
 * Arguments an op does not use may be NULL. */
enum {
  IFEM_TMG_CHEB_INIT = 0, IFEM_TMG_CHEB_STEP, IFEM_TMG_VEC_RECIP, IFEM_TMG_VEC_ROUGH, IFEM_TMG_CVT_D2F, IFEM_TMG_CVT_F2D, IFEM_TMG_AXPY_F32V,
  IFEM_TMG_VC_EXIT, IFEM_TMG_VC_EXIT_F32, IFEM_TMG_INJECT_NODES, IFEM_TMG_VC_ENTRY, IFEM_TMG_VC_ENTRY_F32, IFEM_TMG_CHEB_INIT_BLOCK_F32, IFEM_TMG_COUNT
};
int ifem_test_mg_vec_kernel(ifem_ctx *ctx, int op, int64_t n, int64_t m, const double *coef, const int32_t *idx, double *in0, double *in1,
                            double *out0, double *out1, double *out2);

/* The M_p solve of the block preconditioner (solver.hip::solve_mp) on host vectors of n_pnodes (owned) doubles: x = what it produces for b under
 * the options o (NULL: the defaults), by the tensor-product line solves where the level qualifies and ifem_solver_opts::mp_solver = 0, by CG to
 * max(mp_abs, mp_rel ||b||) elsewhere.  info = {1 direct / 0 CG, CG iterations}.  After an assembly that integrated M_p (a multigrid level: after
 * the first solve of its chain).  The direct path is single-rank; on several ranks the call is collective like the solve itself. */
int ifem_test_mp_solve(ifem_ctx *ctx, const ifem_solver_opts *o, const double *b, double *x, int32_t info[2]);

/* y = S_m x, the pressure Schur block S_m = B diag(M_u)^-1 B^T of the block preconditioner, on host vectors of n_pnodes (owned) doubles.  After
 * an assembly (a multigrid level: after the first solve of its chain); forms S_m and its stencil tables when they are not there yet, as a solve
 * would.  Path 0 needs one rank and the explicit S_m; on several ranks path 1 is collective like the solve itself (every rank calls it with its
 * owned entries) and is the distributed product, which never takes the stencil path.
 *   path 0: the fp64 CSR product of the assembled matrix     path 1: what the solves of the default options use (solver.hip::sm_apply): the
 *   lattice stencil product (sm_stencil.hip) where the level is a full uniform lattice and its tables passed their probe, the CSR product elsewhere
 *   path 2: switch the stencil product of this context off from now on     path 3: on again (the default).  Both only switch (x, y unused, may be
 *   NULL) and make a captured V-cycle of the context be captured anew; path 3 also builds and probes the tables of an S_m that was re-formed
 *   while the path was off.
 * info = {1 the stencil product is in use / 0, its classes, its irregular rows (produced by the CSR kernel), bytes of its table}. */
int ifem_test_sm_apply(ifem_ctx *ctx, int path, const double *x, double *y, int64_t info[4]);

/* The S_m solve of the block preconditioner (solver.hip::solve_sm) on host vectors of n_pnodes (owned) doubles: x = what it produces for b under
 * the options o (NULL: the defaults), by fast diagonalisation (sm_direct.hip) where ifem_solver_opts::sm_mg = 2, the level qualifies and its
 * factors passed the probe against the present S_m, by (multigrid-preconditioned) CG to max(sm_abs, sm_rel ||b||) elsewhere.  Forms S_m, and
 * with sm_mg = 2 the factors, when they are not there yet, as a solve would.  After an assembly.
 * info = {1 direct / 0 CG, CG iterations, the probe value max |S_m x - e| / max |e| of the factors x 1e18 as an integer (0: CG), bytes of the
 * factor tables}. */
int ifem_test_sm_solve(ifem_ctx *ctx, const ifem_solver_opts *o, const double *b, double *x, int64_t info[4]);

/* The products with the off-diagonal blocks on host vectors.  which 0: y = B x (x: dim * n_unodes_local doubles, node-interleaved, ghost entries
 * filled by the caller; y: n_pnodes_owned), 1: y = B^T x (x: n_pnodes_local; y: dim * n_unodes_owned), 2: y += B^T x (y in and out).  After an
 * assembly that left the blocks behind.  No exchange is made: on several ranks every rank multiplies what it is given.
 *   path 0: the fp64 CSR product of the assembled block     path 1: what the solves launch (linalg.hip::spmv_b / spmv_bt / the B^T arm of
 *   spmv_uu): the lattice stencil product (bb_stencil.hip) where the context is a full uniform Q2/Q1 lattice on one rank and the block's tables
 *   passed their probe, the CSR product elsewhere; makes the tables of blocks an assembly wrote since the last look, as a solve's set-up does
 *   path 2: switch the stencil products of this context off from now on     path 3: on again (the default).  Both only switch (x, y unused, may
 *   be NULL); path 3 also builds and probes the tables when the blocks were written while the path was off.
 * info = {0: the product of `which` is the CSR one / otherwise the number of table builds this context has made so far (an assembly that keeps
 * the blocks adds none), classes of the block, its irregular rows (produced by the CSR kernel), bytes of its table}. */
int ifem_test_b_apply(ifem_ctx *ctx, int which, int path, const double *x, double *y, int64_t info[4]);

#ifdef __cplusplus
}
#endif
#endif
