// solver.hip -- host drivers of the linear solves; every vector/matrix operation is a HIP kernel on ctx->stream.
//   precond_vmult()     InsIM::BlockSchurPreconditioner::vmult                  (mpi_insim.cpp:57-128): solve_mp(), solve_sm(), ainv_apply()
//   ins_solve()         InsIM::solve                                            (mpi_insim.cpp:365-395)
// The Krylov drivers themselves are krylov.hip: gmres(flexible) is deal.II's SolverFGMRES as used by InsIM::solve (mpi_insim.cpp:379-388),
// cg() PETSc's KSPCG + PreconditionNone (mpi_insim.cpp:73-82,88-108).
// A~^-1 (MUMPS in the reference, ainv_apply() here) is an inner right-preconditioned GMRES(m): on the BSR A_uu with node-block Jacobi, or
// (IFEM_AINV_MG, the type MgUu) on the matrix-free A_uu with a multigrid V-cycle; the outer solver is *flexible* GMRES precisely so that
// such an inexact inner solve is admissible.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <vector>
#include "ctx.hpp"
#include "kernels.hpp"
#include "krylov.hpp"

namespace ifem {

// all-reduced multi-dot over the n owned entries, summed over the ranks
static MdotFn mdot_over(ifem_ctx *c, int64_t n) {
  return [c, n](int k, const double *V, int64_t ld, const double *w, double *out) { v_mdot(c, n, k, V, ld, w, out, /*all_ranks=*/true); };
}

struct Clock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

struct SolveState {
  ifem_ctx *ctx;
  const ifem_ins_params *P;
  const ifem_solver_opts *o;
  ifem_solve_stats st{};
  int64_t nuo, npo, n;
  double p_src_norm = 0, u_src_norm = 0; // norms of the pressure / velocity parts of the vector the preconditioner is applied to
  bool tight_candidate = false, tight_used = false; // inner_rel_first: the solve qualified for it / its first application ran with it
  // workspace carved out of ctx->work
  double *xu_ext, *xp_ext, *tu, *tp[7], *utmp, *inner_w, *inner_z, *outer_w;
};

// ghost-extended views of a compact owned vector [u_o | p_o]
static void extend_u(SolveState &S, const double *xu, const double **out) {
  ifem_ctx *c = S.ctx;
  if (c->halo.nranks == 1) { *out = xu; return; }
  v_copy(c, S.nuo, xu, S.xu_ext);
  halo_exchange(c, S.xu_ext); // exchanges the u part only when given a u-extended buffer (see comm.hip)
  *out = S.xu_ext;
}
static void extend_p(SolveState &S, const double *xp, const double **out) {
  ifem_ctx *c = S.ctx;
  if (c->halo.nranks == 1) { *out = xp; return; }
  v_copy(c, S.npo, xp, S.xp_ext);
  halo_exchange_p(c, S.xp_ext);
  *out = S.xp_ext;
}

// the assembled operator A^ = [A_uu B^T; B A_pp]: ghost-extended input (xu [dim*nUl], xp [nPl]), compact owned output
static void system_apply_ext(SolveState &S, const double *xu, const double *xp, double *y, bool time_it);

// The halo protocol of an operator on a compact owned vector, written once.  Overlapped (several ranks, comm.hip::halo_start / halo_wait, and
// the site's own condition `overlap`): `start` copies into the ghost-extended buffer and sends the halo off on the halo stream, op(1) is the
// part that reads no ghost entry, op(2) the rest once the halo has arrived.  Otherwise `refresh` makes the ghost-extended view (extend_* /
// halo_exchange*: on one rank the caller's own vector, no copy) and op(0) is the whole operator.
template <typename Start, typename Refresh, typename Op>
static void halo_apply(ifem_ctx *c, bool overlap, const Start &start, const Refresh &refresh, const Op &op) {
  if (overlap && halo_overlap_ok(c)) { start(); op(1); halo_wait(c); op(2); return; }
  refresh(); op(0);
}

// the same on a compact owned vector (ghosts refreshed here).  Several ranks: both halos travel on the halo stream while the
// rows without a ghost column are multiplied (PlanarCsr::split_rows)
static void system_apply_raw(SolveState &S, const double *x, double *y, bool time_it) {
  ifem_ctx *c = S.ctx;
  const double *xu = S.xu_ext, *xp = S.xp_ext;
  halo_apply(c, !c->has_app && !((S.o->outer_matrix_free || !c->uu_is_stored) && c->mf_valid),
    [&] {
      build_row_split(c, c->Auu, c->nUo, &c->Bt, c->nPo); build_row_split(c, c->B, c->nUo);
      v_copy(c, S.nuo, x, S.xu_ext); v_copy(c, S.npo, x + S.nuo, S.xp_ext);
      halo_start(c, S.xu_ext, 0); halo_start(c, S.xp_ext, 1);
    },
    [&] { extend_u(S, x, &xu); extend_p(S, x + S.nuo, &xp); },
    [&](int part) {
      if (part == 0) { system_apply_ext(S, xu, xp, y, time_it); return; }
      spmv_uu(c, xu, xp, y, false, part); spmv_b(c, xu, y + S.nuo, part);
    });
}

// operator of the outer Krylov solver: A^, or C^T A^ C with the hanging rows replaced by their diagonal (hanging.hip)
static void system_apply(SolveState &S, const double *x, double *y, bool time_it) {
  ifem_ctx *c = S.ctx;
  if (!c->hang.active) { system_apply_raw(S, x, y, time_it); return; }
  const double *xe = hanging_input(c, x); // ghost-extended, hanging entries interpolated
  system_apply_ext(S, xe, xe + int64_t(c->dim) * c->nUl, y, time_it);
  hanging_output(c, x, false, y);
}

static void system_apply_ext(SolveState &S, const double *xu, const double *xp, double *y, bool time_it) {
  ifem_ctx *c = S.ctx;
  if ((S.o->outer_matrix_free || !c->uu_is_stored) && c->mf_valid && !c->has_app) { // A_uu x_u without the stored matrix (fp64 cell arithmetic)
    apply_uu_mf(c, xu, y);
    spmv_bt(c, xp, S.tu);
    v_axpy(c, S.nuo, 1.0, S.tu, y);
  } else
    spmv_uu(c, xu, xp, y, false);
  spmv_b(c, xu, y + S.nuo);
  if (c->has_app) { // SCnsIM: y_p += A_pp x_p
    spmv_app(c, xp, S.tp[5]);
    v_axpy(c, S.npo, 1.0, S.tp[5], y + S.nuo);
  }
}

static double dot_all(SolveState &S, int64_t n, const double *a, const double *b) {
  double d = v_dot(S.ctx, n, a, b);
  allreduce_sum(S.ctx, &d, 1);
  return d;
}

// ---- the pressure Schur complement S_m = B diag(M_u)^-1 B^T of one level (mass_schur(1,1), mpi_insim.cpp:44-49)
// S_m applied with two SpMVs (ghost refreshes in between): several ranks without the 2-deep halo plan, and the probing
static void sm_matrix_free(SolveState &S, const double *x, double *y, bool lowp) {
  ifem_ctx *c = S.ctx;
  const double *xe; extend_p(S, x, &xe);
  if (lowp) spmv_bt_f32(c, xe, S.tu); else spmv_bt(c, xe, S.tu);
  vec_mul(c, S.nuo, c->dinvMu.p, S.tu, S.tu);
  const double *te; extend_u(S, S.tu, &te);
  if (lowp) spmv_b_f32(c, te, y); else spmv_b(c, te, y);
}

static bool sm_is_explicit(const SolveState &S) {
  const ifem_ctx *c = S.ctx;
  return S.o->explicit_schur && (c->halo.nranks == 1 || c->halo.has_s);
}

// BlockSchurPreconditioner ctor (:44-49): S_m formed explicitly, once per constrained-dof set
static void sm_ensure(SolveState &S) {
  ifem_ctx *c = S.ctx;
  if (!sm_is_explicit(S)) return;
  if (c->halo.nranks == 1) {
    if (c->Sm.n_rows == 0) build_schur_pattern(c);
    schur_numeric(c);
    sm_stencil_setup(c, S.o->verbose); // (re)builds and probes the lattice stencil tables when S_m was re-formed: set-up time, never inside sm_apply
    if (S.o->sm_mg == 2) sm_direct_setup(c, S.o->verbose); // the fast-diagonalisation factors and their probe (sm_direct.hip), with the product above
    return;
  }
  // same matrix, distributed: pattern from the pressure lattice, values by probing
  if (c->Sm.n_rows == 0 && c->nPo) build_schur_pattern_box(c);
  if ((int64_t)c->xs_ext.n < c->halo.n_s_cols) c->xs_ext.alloc(c->halo.n_s_cols);
  if (!c->sm_valid) {
    const int ncol = c->dim == 3 ? 125 : 25;
    for (int col = 0; col < ncol; ++col) {
      schur_probe_vector(c, col, S.tp[1]);
      sm_matrix_free(S, S.tp[1], S.tp[3], false);
      schur_probe_fill(c, col, S.tp[3]);
    }
    sm_written(c);
  }
}

// y = S_m x on compact owned pressure vectors
static void sm_apply(SolveState &S, const double *x, double *y, bool lowp) {
  ifem_ctx *c = S.ctx;
  if (sm_is_explicit(S) && c->halo.nranks > 1) {
    v_copy(c, S.npo, x, c->xs_ext.p);
    // (rows of S_m without a far column while the 2-deep halo travels)
    halo_apply(c, true, [&] { build_row_split(c, c->Sm, c->nPo); halo_start(c, c->xs_ext.p, 2); }, [&] { halo_exchange_s(c, c->xs_ext.p); },
               [&](int part) { spmv_sm(c, c->xs_ext.p, y, lowp, part); });
    return;
  }
  // the approximate-preconditioner kinds (1, 3) also stream S_m in single precision: it only ever acts inside CG to
  // 1e-3 ||v|| and the rounding (6e-8 relative) is far below the eigenvalue ratio of this Laplacian-like operator
  // ... unless the level applies S_m from its lattice stencil tables (sm_stencil.hip: fp64 tables of a few KB, `lowp` has nothing to save there)
  if (sm_is_explicit(S)) {
    if (sm_stencil_ready(c)) sm_stencil_apply(c, x, y);
    else spmv_sm(c, x, y, lowp);
    return;
  }
  sm_matrix_free(S, x, y, lowp);
}

// ---- multigrid V-cycle for S_m over the levels attached with ifem_mg_attach (geometric, rediscretised coarse operators).
// Smoother: Chebyshev iteration on D^-1 S_m (D = diag S_m) over [lambda_max / ratio, 1.1 lambda_max]: no inner products, a
// fixed polynomial, so the V-cycle (same polynomial before and after the coarse correction) is a fixed SPD operator and
// CG may use it as its preconditioner.  Level vectors (ctx->mg_vec, nPl + 8 each): 0 right-hand side / residual,
// 1 solution, 2 Chebyshev direction, 3 operator product, 4 prolongated correction.  Compact owned entries come first, so
// the same buffers serve as ghost-extended pressure vectors for the transfers.
// A fixed launch sequence on fixed buffers as a hipGraph (ctx.hpp::VcGraph): replayed while `key` -- every pointer, bound, parameter and count the
// sequence's kernel arguments are made of -- stays what it was when the graph was captured.  A new key runs `body` eagerly once (whatever is
// allocated or converted lazily inside exists afterwards) and is captured at its next occurrence.  The context's graph_epoch (a tuning or
// profiling change) is part of every key.  Returns false when the runtime refused the capture: the caller stops asking (body has run eagerly
// by then).
static bool graph_run(ifem_ctx *c, ifem_ctx::VcGraph &G, std::vector<uint64_t> &key, const std::function<void()> &body) {
  key.push_back(c->graph_epoch);
  if (G.exec && key == G.key) {
    if (hipGraphLaunch(G.exec, c->stream) == hipSuccess) { ++G.launches; return true; }
    (void)hipGetLastError(); // a replay the runtime refuses: give the graph up and run the sequence eagerly
    G.destroy();
    G.armed = false;
    body();
    return false;
  }
  if (!(G.armed && key == G.key)) {
    G.destroy();
    G.key = key; G.armed = true;
    body();
    return true;
  }
  bool captured = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
  if (captured) {
    bool threw = false;
    try { body(); }
    catch (...) { threw = true; } // e.g. a call that is illegal during capture on a path the eager warm-up did not reach
    if (threw) { // end and discard the capture, clear the error, and run the sequence eagerly: an eager run may well succeed
      hipGraph_t dead = nullptr;
      (void)hipStreamEndCapture(c->stream, &dead);
      if (dead) (void)hipGraphDestroy(dead);
      (void)hipGetLastError();
      G.destroy();
      G.armed = false;
      body();
      return false;
    }
    captured = hipStreamEndCapture(c->stream, &G.graph) == hipSuccess && G.graph != nullptr;
    captured = captured && hipGraphInstantiate(&G.exec, G.graph, nullptr, nullptr, 0) == hipSuccess;
    captured = captured && hipGraphLaunch(G.exec, c->stream) == hipSuccess;
  }
  if (captured) { ++G.captures; ++G.launches; return true; }
  (void)hipGetLastError();
  G.destroy();
  G.armed = false;
  body();
  return false;
}
// rocprofv3 (rocprofiler-sdk 7.2) dies with a segmentation fault inside hipGraphLaunch when kernel tracing is on: under a profiler the cycles are
// launched eagerly.  Detected once per process by the tool library being loaded (or announced: rocprofv3 exports ROCP_TOOL_LIBRARIES for its
// child) -- the one place where this library looks at its environment.
static bool profiler_attached() {
  static const bool on = [] {
    if (std::getenv("ROCP_TOOL_LIBRARIES") || std::getenv("ROCPROFILER_REGISTER_FORCE_LOAD")) return true;
    for (const char *lib : {"librocprofiler-sdk-tool.so", "librocprofiler-sdk-tool.so.1", "librocprofiler-sdk-tool.so.0"}) {
      if (void *h = dlopen(lib, RTLD_NOLOAD | RTLD_LAZY)) { dlclose(h); return true; }
    }
    return false;
  }();
  return on;
}
static inline void key_ptr(std::vector<uint64_t> &key, const void *p) { key.push_back(uint64_t(reinterpret_cast<uintptr_t>(p))); }
static inline void key_f64(std::vector<uint64_t> &key, double v) { uint64_t b; std::memcpy(&b, &v, 8); key.push_back(b); }

// May the cycle over `levels` (level 0 = c) be replayed as a hipGraph (ctx.hpp::VcGraph)?  Small single-rank chains outside of any profiling;
// what else a level must satisfy is its caller's (S_m: the explicit matrix; A_uu: no per-level profiling)
static bool cycle_graph_ok(ifem_ctx *c, const std::vector<SolveState> &levels) {
  bool ok = c->tune.vcycle_graph_cells > 0 && c->n_cells <= c->tune.vcycle_graph_cells && !c->profile && !kprof_root(c).on && !profiler_attached();
  for (const SolveState &L : levels) ok = ok && L.ctx->halo.nranks == 1 && !L.ctx->mg_replica;
  return ok;
}
// the smoother's B of a level of the A_uu V-cycle: 0 inverse node blocks, 1 the vertex-patch sum of patch.hip (chosen by mg_uu_setup)
static int smoother_kind(const ifem_ctx *c) { return patch_active(c) ? 1 : 0; }
// per-level part of the replay keys: every pointer, count, bound and parameter the level's launches of the cycle are made of
static void sm_level_key(ifem_ctx *lc, std::vector<uint64_t> &key) {
  for (auto &v : lc->mg_vec) key_ptr(key, v.p);
  key_ptr(key, lc->sm_dinv.p); key_ptr(key, lc->Sm.val.p); key_ptr(key, lc->Sm_f32.p); key_ptr(key, lc->Sm.rowptr.p);
  key_ptr(key, lc->mg_Rp.col.p); key_ptr(key, lc->mg_Pp.col.p);
  key.push_back(uint64_t(lc->nPo)); key.push_back(uint64_t(lc->sm_version)); key.push_back(uint64_t(lc->tune.sm_lanes)); key.push_back(uint64_t(lc->Sm_f32.valid));
  key_f64(key, lc->sm_lmax);
  // which product the level launches, and the tables of the stencil one
  const SmStencil &T = lc->sm_stencil;
  key.push_back(uint64_t(sm_stencil_ready(lc))); key.push_back(uint64_t(T.n_irregular));
  key_ptr(key, T.table.p); key_ptr(key, T.cls.p); key_ptr(key, T.rows.p); key_ptr(key, lc->p_lattice.node_of_lattice.p);
  // S_m in operator form launches the B^T and B products: which ones, and the tables of the stencil ones (bb_stencil.hip)
  const BbStencil &Q = lc->bb_stencil;
  for (int which = 0; which < 2; ++which) {
    const StencilClasses &K = which ? Q.bt : Q.b;
    key.push_back(uint64_t(bb_stencil_ready(lc, which))); key.push_back(uint64_t(K.n_irregular));
    key_ptr(key, K.table.p); key_ptr(key, K.cls.p); key_ptr(key, K.rows.p);
  }
  key_ptr(key, lc->u_lattice.node_of_lattice.p); key_ptr(key, lc->B.val.p); key_ptr(key, lc->Bt.val.p);
}
static void uu_level_key(ifem_ctx *lc, std::vector<uint64_t> &key) {
  (void)bjac_f32_ptr(lc); // lazy state (the single-precision copy of the inverse node blocks) stays outside the graph
  for (auto &v : lc->mguf_vec) key_ptr(key, v.p);
  key_ptr(key, lc->bjac_f32.p); key_ptr(key, lc->mf_eval.p); key_ptr(key, lc->mf_ycell.p); key_ptr(key, lc->mg_Ru_mask.p); key_ptr(key, lc->mg_Pu_mask.p);
  key_ptr(key, lc->has_c[lc->asm_constraint_set] ? lc->is_c[lc->asm_constraint_set].p : nullptr);
  key.push_back(uint64_t(lc->nUo)); key.push_back(uint64_t(lc->n_cells)); key.push_back(uint64_t(lc->mf_noconv)); key.push_back(uint64_t(lc->tune.xcd_swizzle));
  // which transfer kernels the level launches towards the next one, and the maps of the lattice ones (mg_lattice.hip)
  key.push_back(uint64_t(mg_lattice_u_active(lc))); key_ptr(key, lc->mgl_map.p); key_ptr(key, lc->u_lattice.lattice_of_node.p);
  // everything else the captured launches are made of: the epoch moves with ifem_set_tuning / ifem_set_profiling / ifem_mg_attach
  key.push_back(lc->graph_epoch); key.push_back(uint64_t(lc->tune.mf_f32));
  key.push_back(uint64_t(mf_takes_uniform(lc))); for (double hd : lc->mf_h) key_f64(key, hd); // which cell kernels, and their constants
  key_ptr(key, lc->bjac.p); key_ptr(key, lc->vcoords.p); key_ptr(key, lc->cell_unodes.p); key_ptr(key, lc->uinc.col.p);
  key.push_back(uint64_t(smoother_kind(lc))); key_ptr(key, lc->patch.tab.p); key_ptr(key, lc->patch.inv.p); key_ptr(key, lc->patch.work.p); // the level's smoother and its tables
  key.push_back(uint64_t(lc->patch.form)); key_ptr(key, lc->patch.gen_nodes.p); key_ptr(key, lc->patch.gen_node_ptr.p); key_ptr(key, lc->patch.gen_inv_off.p); key.push_back(uint64_t(lc->patch.gen_colours)); // (the per-patch form)
  key_f64(key, lc->uu_lmax()); key_f64(key, lc->mf_params.viscosity); key_f64(key, lc->mf_params.rho); key_f64(key, lc->mf_params.grad_div); key_f64(key, lc->mf_params.dt);
}

// A replicated coarse level (a single-rank context of the whole coarse mesh below a partitioned level) is computed by every rank
// on its own device: its operators carry float / double atomics whose order differs between devices, so the replicas agree to
// rounding only, and replica-local decisions (the 1 % early exit of a power iteration) may differ.  Quantities that steer the
// smoother -- the Chebyshev bounds -- are therefore agreed on over the partitioned level's communicator (maximum over the ranks):
// every rank then applies the SAME polynomial, and the level stays one (symmetric) preconditioner for all of them.
static ifem_ctx *replica_world(ifem_ctx *c) {
  if (c->halo.nranks > 1) return nullptr;
  for (ifem_ctx *p = c->mg_fine; p; p = p->mg_fine)
    if (p->halo.nranks > 1) return p;
  return nullptr;
}

// a level vector of at least n entries: (re)allocated and zero-filled when it is too short (set-up: never inside a captured cycle)
template <typename T>
static void ensure_zeroed(ifem_ctx *c, DBuf<T> &v, int64_t n) {
  if ((int64_t)v.n >= n) return;
  v.alloc((size_t)n);
  IFEM_HIP_CHECK(hipMemsetAsync(v.p, 0, v.n * sizeof(T), c->stream));
}

// Largest eigenvalue of a smoothed operator B A over n owned entries: power iteration (set-up only: host-synchronised norms), BA(x, y) writes
// y = B A x.  Cold -- no estimate yet (lmax_prev <= 0) or no stored iterate of this length -- it starts from a fixed rough vector (seed) and
// runs all `steps`; warm -- the operator was re-formed for another constrained-dof set of the same mesh -- it starts from the previous run's last
// iterate `eig` and stops once the estimate moves by less than 1 %.  Returns the raw estimate (0 or non-finite ones are the caller's to replace).
template <typename Op>
static double estimate_lmax(ifem_ctx *c, int64_t n, int steps, int64_t seed, double lmax_prev, DBuf<double> &eig, double *x, double *y, const Op &BA,
                            bool *was_warm = nullptr) {
  const bool warm = lmax_prev > 0 && (int64_t)eig.n == n && n > 0;
  if (was_warm) *was_warm = warm;
  if (warm) v_copy(c, n, eig.p, x);
  else vec_rough(c, n, seed, x);
  double lam = 0;
  for (int it = 0; it < steps; ++it) {
    double nx = v_dot(c, n, x, x);
    allreduce_sum(c, &nx, 1);
    if (!(nx > 0)) break;
    v_scale(c, n, 1.0 / std::sqrt(nx), x);
    BA(x, y);
    double ny = v_dot(c, n, y, y);
    allreduce_sum(c, &ny, 1);
    const double prev = lam;
    lam = std::sqrt(ny);
    v_copy(c, n, y, x);
    if (warm && it >= 1 && std::fabs(lam - prev) <= 0.01 * lam) break;
  }
  if (n > 0) {
    if ((int64_t)eig.n != n) eig.alloc((size_t)n);
    v_copy(c, n, x, eig.p);
  }
  return lam;
}

// One Chebyshev sweep of a level's smoother: `steps` steps over the target interval [lo, hi] of B A (mg_sm_sweep, mg_uu_sweep: the one place
// where each multigrid chooses them), and its recurrence: the first direction is d = c0() B r, step k makes d = a d + b B r with next(a, b).
struct ChebSweep { double lo, hi; int steps; };
struct Cheb {
  double theta, delta, sigma, rho;
  Cheb(double lo, double hi) : theta(0.5 * (hi + lo)), delta(0.5 * (hi - lo)), sigma(theta / delta), rho(1.0 / sigma) {}
  explicit Cheb(const ChebSweep &w) : Cheb(w.lo, w.hi) {}
  double c0() const { return 1.0 / theta; }
  void next(double &a, double &b) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    a = rho_new * rho; b = 2.0 * rho_new / delta; rho = rho_new;
  }
};

struct MgSm {
  std::vector<SolveState> L; // level 0 = the context being solved
  bool lowp = false;
  int nu = 2;
  double ratio = 4.0;
};

// geometry blocks, S_m, its diagonal and the eigenvalue bound of every level; cheap when nothing changed
static void mg_sm_setup(MgSm &M, int use_nonzero) {
  for (size_t l = 0; l < M.L.size(); ++l) {
    SolveState &S = M.L[l];
    ifem_ctx *c = S.ctx;
    if (l > 0) { // coarse levels are rediscretised: B, B^T, M_p, diag(M_u) of the level's own mesh and constraint set
      // (ifem_tuning::geo_cache = 2, "every assembly is a new constrained-dof set": once per assembly of the finest level,
      // not once per preconditioner application)
      ifem_ctx *f0 = M.L[0].ctx;
      if (!(c->tune.geo_cache == 2 && c->geo.refresh_stamp == f0->asm_version)) {
        launch_ins_assemble_ex(c, S.P, use_nonzero, 0, AsmMode::LevelGeometry);
        c->geo.refresh_stamp = f0->asm_version;
      }
      sm_ensure(S);
    }
    for (auto &v : c->mg_vec) ensure_zeroed(c, v, c->nPl + 8);
    // S_m in operator form (the finest level of a partition without the 2-deep pressure halo: unstructured strips): the smoother
    // needs its diagonal only, which the rows of B give; "valid" = the diagonal belongs to the present blocks
    const bool opform = !sm_is_explicit(S);
    if (opform && !c->sm_valid) sm_written(c);
    if (c->sm_mg_version == c->sm_version && c->sm_lmax > 0) continue;
    if ((int64_t)c->sm_dinv.n != c->nPo) c->sm_dinv.alloc((size_t)c->nPo);
    if (opform) {
      const double *de; extend_u(S, c->dinvMu.p, &de);
      sm_diag_from_blocks(c, de, c->sm_dinv.p);
    } else
    scalar_diag(c, c->Sm, c->Sm.val.p, c->sm_dinv.p); // owned rows; the diagonal entry has a local column id on every layout
    vec_recip(c, S.npo, c->sm_dinv.p);
    // largest eigenvalue of D^-1 S_m (estimate_lmax: 14 steps when cold)
    double lam = estimate_lmax(c, S.npo, c->tune.eig_steps > 0 ? c->tune.eig_steps : 14, int64_t(c->halo.rank) * 1000003, c->sm_lmax, c->sm_eig, c->mg_vec[1].p,
                               c->mg_vec[3].p, [&](const double *x, double *y) { sm_apply(S, x, y, false); vec_mul(c, S.npo, c->sm_dinv.p, y, y); });
    if (ifem_ctx *w = replica_world(c)) allreduce_max(w, &lam, 1);
    c->sm_lmax = lam > 0 ? lam : 1.0;
    c->sm_mg_version = c->sm_version;
  }
}

// the sweep of level l over the target interval of D^-1 S_m: the coarsest level's longer polynomial over a wide interval stands in for a direct solve
static ChebSweep mg_sm_sweep(const MgSm &M, size_t l) {
  const double hi = 1.1 * M.L[l].ctx->sm_lmax;
  if (l + 1 == M.L.size()) return {hi / 900.0, hi, 30};
  return {hi / M.ratio, hi, M.nu};
}
// the Chebyshev sweep of level l on S x = b from the pair (x, r = b - S x); with keep_r the residual is kept up to date on exit
// (one operator product per step), without it the last product is skipped
static void mg_sm_smooth(MgSm &M, size_t l, double *x, double *r, bool keep_r) {
  SolveState &S = M.L[l];
  ifem_ctx *c = S.ctx;
  double *d = c->mg_vec[2].p, *t = c->mg_vec[3].p;
  const ChebSweep w = mg_sm_sweep(M, l);
  Cheb ch(w);
  cheb_init(c, S.npo, ch.c0(), c->sm_dinv.p, r, d);
  for (int k = 0; k < w.steps; ++k) {
    const bool last = k == w.steps - 1;
    if (last && !keep_r) { v_axpy(c, S.npo, 1.0, d, x); break; }
    sm_apply(S, d, t, M.lowp);
    double a, b; ch.next(a, b);
    // x += d; r -= S d; d = rho_new rho_old d + (2 rho_new / delta) D^-1 r   (the new d is unused after the last step)
    cheb_step(c, S.npo, a, b, c->sm_dinv.p, t, x, r, d);
  }
}

// level l: mg_vec[1] = V(mg_vec[0]); mg_vec[0] is overwritten by the residual
static void mg_sm_vcycle(MgSm &M, size_t l) {
  SolveState &S = M.L[l];
  ifem_ctx *c = S.ctx;
  double *r = c->mg_vec[0].p, *x = c->mg_vec[1].p;
  v_zero(c, S.npo, x);
  if (l + 1 == M.L.size()) { mg_sm_smooth(M, l, x, r, false); return; } // coarsest level
  mg_sm_smooth(M, l, x, r, true);
  // restriction r_c = P^T r: gather per LOCAL coarse node from the owned fine nodes, ghost rows travel to their owners
  SolveState &Sc = M.L[l + 1];
  ifem_ctx *cc = Sc.ctx;
  mg_csr_apply(c, c->mg_Rp, r, cc->mg_vec[0].p);
  if (c->mg_replica) allreduce_sum_vec(c, cc->mg_vec[0].p, cc->nPo, cc->mg_vec[4].p); // replicated coarse level: sum of the ranks' partial rows
  else halo_reverse_add_p(cc, cc->mg_vec[0].p);
  mg_sm_vcycle(M, l + 1);
  // prolongation e = P x_c from the ghost-extended coarse correction, then x += e, r -= S e
  halo_exchange_p(cc, cc->mg_vec[1].p);
  double *e = c->mg_vec[4].p, *t = c->mg_vec[3].p;
  mg_csr_apply(c, c->mg_Pp, cc->mg_vec[1].p, e);
  sm_apply(S, e, t, M.lowp);
  v_axpy(c, S.npo, 1.0, e, x);
  v_axpy(c, S.npo, -1.0, t, r);
  mg_sm_smooth(M, l, x, r, false);
}

// CG preconditioned by one V-cycle, zero initial guess, absolute tolerance on the true residual ||b - S x||_2 (the
// reference's stopping rule for CG(S_m), mpi_insim.cpp:88-89)
static int pcg_mg_sm(MgSm &M, const double *b, double *x, double tol, int maxit, double *r, double *p, double *q, double *sv = nullptr) {
  SolveState &S = M.L[0];
  ifem_ctx *c = S.ctx;
  auto dot2 = [&](const double *a1, const double *b1, const double *a2, const double *b2, double *out) {
    out[0] = v_dot(c, S.npo, a1, b1);
    out[1] = (a1 == a2 && b1 == b2) ? out[0] : v_dot(c, S.npo, a2, b2);
    allreduce_sum(c, out, 2);
  };
  double *zin = c->mg_vec[0].p, *z = c->mg_vec[1].p;
  // the cycle: eagerly, or replayed as a hipGraph on small single-rank chains (as the A_uu V-cycle, precond_vmult)
  bool graph_ok = cycle_graph_ok(c, M.L);
  for (const SolveState &L : M.L) graph_ok = graph_ok && sm_is_explicit(L);
  auto sm_cycle = [&]() {
    if (!graph_ok) { mg_sm_vcycle(M, 0); return; }
    std::vector<uint64_t> key;
    key.push_back(M.L.size()); key.push_back(uint64_t(M.nu)); key_f64(key, M.ratio); key.push_back(uint64_t(M.lowp));
    for (const SolveState &L : M.L) sm_level_key(L.ctx, key);
    if (!graph_run(c, c->sm_graph, key, [&]() { mg_sm_vcycle(M, 0); })) { c->tune.vcycle_graph_cells = 0; graph_ok = false; }
  };
  if (sv && c->tune.cg_single_reduction) {
    // the recurrence of linalg.hip::cg1_* with the V-cycle as its preconditioner: u = V r, w = S u, the two inner products of the step in one
    // pass with alpha / beta formed on the device (several ranks: one all-reduce on the stream), the vectors updated in one pass; the host
    // waits once per iteration, for ||r||^2 of the stopping rule (it waited six times: three pairs of separate dot products)
    auto norm2 = [&](const double *v) { double t = v_dot(c, S.npo, v, v); allreduce_sum(c, &t, 1); return t; };
    cg1_init(c, S.npo, b, nullptr, x, r, r, p, sv);
    double rr = norm2(r);
    int it = 0;
    while (std::sqrt(rr) > tol && it < maxit) {
      v_copy(c, S.npo, r, zin);
      sm_cycle();                      // z = V r
      sm_apply(S, z, q, M.lowp);       // w = S z
      cg1_dots(c, S.npo, r, z, q, it == 0);
      cg1_update(c, S.npo, nullptr, z, q, p, sv, x, r);
      rr = norm2(r);
      ++it;
      if (!(rr == rr)) break; // NaN guard
    }
    return it;
  }
  v_zero(c, S.npo, x);
  v_copy(c, S.npo, b, r);
  double d2[2];
  dot2(r, r, r, r, d2);
  double rr = d2[0], rz = 0;
  int it = 0;
  while (std::sqrt(rr) > tol && it < maxit) {
    v_copy(c, S.npo, r, zin);
    sm_cycle();
    double rz_new[2];
    dot2(r, z, r, z, rz_new);
    if (it == 0) v_copy(c, S.npo, z, p);
    else v_axpby(c, S.npo, 1.0, z, rz_new[0] / rz, p);
    rz = rz_new[0];
    sm_apply(S, p, q, M.lowp);
    double pq[2];
    dot2(p, q, p, q, pq);
    const double al = rz / pq[0];
    v_axpy(c, S.npo, al, p, x);
    v_axpy(c, S.npo, -al, q, r);
    dot2(r, r, r, r, d2);
    rr = d2[0];
    ++it;
    if (!(rr == rr)) break; // NaN guard
  }
  return it;
}

static void carve_workspace(SolveState &S, bool krylov = true);

// ---- multigrid V-cycle for A_uu (IFEM_AINV_MG): stands where the reference has MUMPS (mpi_insim.cpp:124-127).  Every level
// applies its own matrix-free A_uu (apply_mf.hip, single-precision cell arithmetic) at the evaluation point injected from
// the level above; smoother = Chebyshev iteration on (node-block diagonal)^-1 A_uu.  The coarse block diagonals are
// integrated matrix-free (mg.hip::k_uu_diag), the finest level uses the blocks of the assembled matrix.  Level vectors
// (ctx->mguf_vec, SINGLE precision since round 3 -- the cell arithmetic of the level operators, the node blocks of the smoother
// and the basis of the Krylov solver around the cycle are single precision already -- dim * nUl + 8 each): 0 right-hand side /
// residual, 1 solution, 2 direction, 3 (unused: the operator product is consumed inside the fused gather), 4 prolongated
// correction; compact owned entries first, so the buffers double as ghost-extended velocity vectors.  The double vectors
// ctx->mgu_vec[1..3] remain as scratch of the eigenvalue estimates.
// One application of A~^-1 is one MgUu: the level chain below the context being solved, the cycle on it (eager or replayed as a hipGraph),
// and the inner solve around the cycle with its retry and fallback ladder.
struct MgUu {
  SolveState &S;             // the context being solved (statistics and workspace of the application)
  ifem_ctx *const c;
  const ifem_solver_opts *const o;
  std::vector<SolveState> L; // level 0 = a copy of S, then the attached coarser levels with velocity transfers
  int nu = 3, nu_post = 3;
  double ratio = 8.0;
  bool trim = false;     // ifem_tuning::inner_f32: single-precision bases around the cycle, and the cycle without the passes nothing reads
  bool graph_ok = false; // the cycle may be replayed as a hipGraph (decided by solve(), withdrawn when the runtime refuses a capture)
  double res = 0;        // residual estimate of the last Krylov attempt
  OpFn Amf;              // the matrix-free A_uu of level 0 on a compact owned vector
  MdotFn mdot;           // all-reduced multi-dot over the owned velocity entries

  explicit MgUu(SolveState &S);
  void cycle();                               // mguf_vec[1] = V(mguf_vec[0]) of level 0
  void apply(const double *x, double *y);     // y = V x on whatever vectors: they only appear in the entry and exit kernels around cycle()
  void apply(const float *x, float *y);       // column j of V -> column j of Z (trim only)
  bool solve_once(const double *b, double *x, double tol);
  void lengthen_restart(int its, int mi);
  void solve(const double *b, double *x, double tol);
};

// matrix-free A_uu of one level on a compact owned vector.  Several ranks: the cells whose nodes are all owned are
// processed while the velocity halo travels, the cells of the ghost layer and the node gather after it has arrived
static void uu_apply_level(SolveState &S, const double *x, double *y, const MfFuse *fuse = nullptr) {
  ifem_ctx *c = S.ctx;
  const double *xe = S.xu_ext;
  halo_apply(c, true, [&] { build_mf_cell_split(c); v_copy(c, S.nuo, x, S.xu_ext); halo_start(c, S.xu_ext, 0); },
             [&] { extend_u(S, x, &xe); }, [&](int part) { apply_uu_mf(c, xe, y, true, fuse, part); });
}

// the same on a level vector of the V-cycle (single precision, ghost-extended in place: owned entries first), fused form
static void uu_apply_level_f32(SolveState &S, float *x_ext, const MfFuseT<float> *fuse) {
  ifem_ctx *c = S.ctx;
  halo_apply(c, true, [&] { build_mf_cell_split(c); halo_start_f32(c, x_ext); }, [&] { halo_exchange_f32(c, x_ext); },
             [&](int part) { apply_uu_mf_f32v(c, x_ext, fuse, part); });
}

// the plain product on a compact owned single-precision column (a Z column of fgmres_f32), fp64 result: one rank reads the column in
// place; several ranks extend a copy by the ghost entries (level vector 3: the cycle does not use it), the interior cells running
// while the halo travels
void uu_apply_f32col(ifem_ctx *c, const float *z, double *y) {
  if (c->halo.nranks == 1) { apply_uu_mf_f32in(c, z, y); return; }
  const int64_t nuo = int64_t(c->dim) * c->nUo, nv = int64_t(c->dim) * c->nUl + 8;
  auto &ext = c->mguf_vec[3]; ensure_zeroed(c, ext, nv);
  if (nuo) IFEM_HIP_CHECK(hipMemcpyAsync(ext.p, z, size_t(nuo) * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  halo_apply(c, true, [&] { build_mf_cell_split(c); halo_start_f32(c, ext.p); }, [&] { halo_exchange_f32(c, ext.p); },
             [&](int part) { apply_uu_mf_f32in(c, ext.p, y, part); });
}

// ---- the smoother's B of a level, as the cycle sees it (the kind itself: smoother_kind above).
// d = a d + b B r.  The node blocks are only asked for a == 0: their other directions ride in the fused gather of the product
static void smoother_dir(ifem_ctx *c, double a, double b, const float *r, float *d) {
  if (smoother_kind(c) == 1) patch_apply(c, a, b, r, d);
  else cheb_init_block_f32(c, b, r, d);
}
// the fused epilogue (MfFuseT::mode) the level's B supports for a wanted one.  The node blocks ride in the gather of the product: the mode stays.
// The patch sum cannot: modes 2 and 3 become mode 1 (x and r only), and the return value says that the direction pass smoother_dir must follow
static bool smoother_fuse_mode(const ifem_ctx *c, int &mode) {
  if (smoother_kind(c) == 0 || mode == 1) return false;
  mode = 1;
  return true;
}
// entry of the trimmed cycle: r = float(src) and the first direction d = c0 B r (node blocks: one pass, mg.hip::k_vc_entry)
static void smoother_entry(ifem_ctx *c, double c0, const double *src, float *r, float *d) {
  if (smoother_kind(c) == 0) { vc_entry(c, c0, src, r, d); return; }
  v_cvt_d2f(c, int64_t(c->dim) * c->nUo, src, r);
  smoother_dir(c, 0.0, c0, r, d);
}
static void smoother_entry(ifem_ctx *c, double c0, const float *src, float *r, float *d) {
  if (smoother_kind(c) == 0) { vc_entry_f32(c, c0, src, r, d); return; }
  const int64_t nuo = int64_t(c->dim) * c->nUo;
  if (nuo) IFEM_HIP_CHECK(hipMemcpyAsync(r, src, size_t(nuo) * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  smoother_dir(c, 0.0, c0, r, d);
}

static void mg_uu_setup(MgUu &M, bool force_bounds = false) {
  ifem_ctx *f0 = M.L[0].ctx;
  // size of the evaluation point the bounds below were estimated at: A_uu carries rho C(u), so a bound taken at a small
  // velocity must not outlive a grown convective part.  One norm per assembly on the finest level (all levels see the same
  // field by injection); a change of more than 10 % refreshes the estimates (warm: 2-3 power steps per level)
  if (f0->uu_evn_asm != f0->asm_version) {
    double e2 = v_dot(f0, int64_t(f0->dim) * f0->nUo, f0->mf_eval.p, f0->mf_eval.p);
    allreduce_sum(f0, &e2, 1);
    f0->uu_evn = std::sqrt(e2);
    f0->uu_evn_asm = f0->asm_version;
  }
  for (size_t l = 0; l < M.L.size(); ++l) {
    SolveState &S = M.L[l];
    ifem_ctx *c = S.ctx;
    const int64_t nv = int64_t(c->dim) * c->nUl + 8;
    for (int k = 1; k <= 3; ++k) ensure_zeroed(c, c->mgu_vec[k], nv);
    for (auto &v : c->mguf_vec) ensure_zeroed(c, v, nv);
    if (l > 0 && c->uu_mg_version != f0->asm_version) { // operator state of a coarse level: rediscretisation at the injected point
      ifem_ctx *p = M.L[l - 1].ctx;
      c->mf_params = f0->mf_params;
      c->mf_noconv = f0->mf_noconv;
      c->asm_constraint_set = f0->asm_constraint_set;
      const size_t ne = size_t(c->dim) * size_t(c->nUl);
      if (c->mf_eval.n != ne) c->mf_eval.alloc(ne);
      mg_inject_nodes(c, c->nUo, p->mg_inj_u.p, p->mf_eval.p, c->mf_eval.p);
      if (p->mg_replica) allreduce_sum_vec(p, c->mf_eval.p, int64_t(c->dim) * c->nUo, c->mgu_vec[1].p); // every rank injects the nodes it owns
      else halo_exchange(c, c->mf_eval.p);
      c->mf_valid = true;
      uu_block_diag_mf(c);
      c->uu_mg_version = f0->asm_version;
    }
    // transfers towards the next level: the packed entries (functions of the two constrained-dof sets) and the choice of the lattice kernels
    if (l + 1 < M.L.size()) mg_transfer_u_setup(c, f0->asm_constraint_set, S.o->verbose);
    // the smoother's B of this level: the inverse node blocks, or (ifem_tuning::uu_smoother = 1 on an eligible level) the vertex-patch
    // sum of patch.hip, whose tables are made here, outside of any captured cycle.  The bound below is one of B A_uu: each kind keeps its own
    // (ctx.hpp::UuBound)
    const int kind = (c->tune.uu_smoother == 1 && patch_setup(c)) ? 1 : 0;
    c->uu_bound_kind = kind;
    ifem_ctx::UuBound &B = c->uu_bound[kind];
    // eigenvalue bound of (block D)^-1 A_uu: depends on the parameters and the constrained-dof set, hardly on the evaluation
    // point (the viscous and mass terms carry the top of the spectrum): estimated once per such state
    const double key[6] = {f0->mf_params.viscosity, f0->mf_params.rho, f0->mf_params.grad_div, f0->mf_params.dt,
                           double(f0->mf_noconv), double(c->flag_id[c->asm_constraint_set])};
    bool same = B.lmax > 0 && !force_bounds;
    for (int i = 0; i < 6; ++i) same = same && key[i] == B.key[i];
    same = same && std::fabs(f0->uu_evn - B.evn) <= 0.1 * std::max(B.evn, 1e-300);
    // measurement mode: a new set per assembly.  The stamp is the entry's own: a kind that sat out an assembly has a bound of the set before
    if (c->tune.geo_cache == 2 && B.asm_stamp != f0->asm_version) same = false;
    B.asm_stamp = f0->asm_version;
    if (same) continue;
    if (force_bounds) B.lmax = 0; // cold estimate: all 12 steps from a rough vector
    // power iteration on B A_uu (estimate_lmax: 12 steps when cold; warm across constrained-dof sets: the top of this spectrum belongs to the mesh)
    double *y = c->mgu_vec[3].p; bool warm;
    double lam = estimate_lmax(c, S.nuo, c->tune.eig_steps > 0 ? c->tune.eig_steps : 12, int64_t(c->halo.rank) * 7000003, B.lmax, B.eig, c->mgu_vec[1].p,
                               c->mgu_vec[2].p, [&](const double *x, double *z) {
      uu_apply_level(S, x, y);
      if (kind == 1) { // the patch B acts on the single-precision level vectors (3 and 4 are idle outside of a cycle)
        v_cvt_d2f(c, S.nuo, y, c->mguf_vec[3].p);
        smoother_dir(c, 0.0, 1.0, c->mguf_vec[3].p, c->mguf_vec[4].p);
        v_cvt_f2d(c, S.nuo, c->mguf_vec[4].p, z);
      } else
      bjac_apply(c, y, z);
    }, &warm);
    if (ifem_ctx *w = replica_world(c)) allreduce_max(w, &lam, 1);
    B.lmax = lam > 0 && std::isfinite(lam) ? lam : 1.0;
    if (S.o->verbose) fprintf(stderr, "[ifem] A_uu V-cycle level %zu (%lld cells): lambda_max estimate %.4f (%s)\n", l, (long long)c->n_cells, c->uu_lmax(), warm ? "warm" : "cold");
    B.evn = f0->uu_evn;
    for (int i = 0; i < 6; ++i) B.key[i] = key[i];
  }
}

// One Chebyshev sweep of mg_uu_smooth.  keep_r: the residual is kept up to date on exit (one operator product per step), without it the
// last product is skipped.  d_ready: the first direction d = (1/theta) B r is already in place (written by the fused residual update, MfFuse
// mode 3, or by the entry of the cycle).
// trim (ifem_tuning::inner_f32): the passes nothing reads are left out -- x_fresh: x holds nothing yet, the first fused step stores xs = x
// instead of adding to a zeroed vector; the last step of a keep_r sweep updates x and r only (mode 1: its new direction would be
// overwritten by the residual update after the coarse correction); no_exit: the closing x += d is the caller's (it delivers x + d elsewhere)
struct SmoothOpts {
  bool keep_r = false, d_ready = false, trim = false, x_fresh = false, no_exit = false;
};
// the sweeps of level l over the target interval of B A_uu (post: the one after the coarse correction); the coarsest level runs one longer sweep
static ChebSweep mg_uu_sweep(const MgUu &M, size_t l, bool post = false) {
  const double hi = 1.1 * M.L[l].ctx->uu_lmax();
  if (l + 1 == M.L.size()) return {hi / 400.0, hi, 24};
  return {hi / M.ratio, hi, post ? M.nu_post : M.nu};
}
static void mg_uu_smooth(MgUu &M, size_t l, const ChebSweep &w, float *x, float *r, const SmoothOpts &o) {
  SolveState &S = M.L[l];
  ifem_ctx *c = S.ctx;
  float *d = c->mguf_vec[2].p;
  Cheb ch(w);
  if (!o.d_ready) smoother_dir(c, 0.0, ch.c0(), r, d);
  for (int k = 0; k < w.steps; ++k) {
    const bool last = k == w.steps - 1;
    if (last && !o.keep_r) {
      if (o.no_exit) break;
      if (k == 0 && o.x_fresh) IFEM_HIP_CHECK(hipMemsetAsync(x, 0, size_t(S.nuo) * sizeof(float), c->stream)); // (a one-step sweep from zero)
      v_axpy_f32v(c, S.nuo, 1.0f, d, x);
      break;
    }
    // x += d; r -= A d; d = rho_new rho_old d + (2 rho_new / delta) B r: fused into the node gather of the product as far as B allows
    MfFuseT<float> f;
    f.mode = (o.trim && last) ? 1 : 2; ch.next(f.a, f.b); f.xs = x; f.r = r; f.d = d;
    f.first = (k == 0 && o.x_fresh) ? 1 : 0;
    const bool dir_follows = smoother_fuse_mode(c, f.mode);
    uu_apply_level_f32(S, d, &f);
    // (the direction of the last step of a keep_r sweep is never read: the residual update after the coarse correction writes a new one)
    if (dir_follows && !last) smoother_dir(c, f.a, f.b, r, d);
  }
}

// level l: mguf_vec[1] = V(mguf_vec[0]); mguf_vec[0] is overwritten by the residual
// M.trim = false: every pass of the cycle as it was written first (ifem_tuning::inner_f32 = 0).  M.trim = true: level 0 starts from r AND the
// first direction d (smoother_entry) and ends BEFORE its last update x += d (vc_exit delivers x + d); no level zeroes its x (see SmoothOpts)
static void mg_uu_vcycle(MgUu &M, size_t l) {
  SolveState &S = M.L[l];
  ifem_ctx *c = S.ctx;
  float *r = c->mguf_vec[0].p, *x = c->mguf_vec[1].p;
  const bool trim = M.trim, top = trim && l == 0;
  if (!trim) IFEM_HIP_CHECK(hipMemsetAsync(x, 0, size_t(S.nuo) * sizeof(float), c->stream));
  if (l + 1 == M.L.size()) {
    SmoothOpts coarsest;
    coarsest.d_ready = top; coarsest.trim = trim; coarsest.x_fresh = trim; coarsest.no_exit = top;
    mg_uu_smooth(M, l, mg_uu_sweep(M, l), x, r, coarsest);
    return;
  }
  SmoothOpts pre;
  pre.keep_r = true; pre.d_ready = top; pre.trim = trim; pre.x_fresh = trim;
  mg_uu_smooth(M, l, mg_uu_sweep(M, l), x, r, pre);
  SolveState &Sc = M.L[l + 1];
  ifem_ctx *cc = Sc.ctx;
  mg_transfer_u(c, /*prolong=*/false, r, cc->mguf_vec[0].p);
  // partial restrictions -> the coarse residual: ghost rows to their owners, or (replicated coarse level: every rank holds all rows) the
  // sum over the ranks; from there down nothing is exchanged and the prolongation reads the replica directly
  if (c->mg_replica) allreduce_sum_vec_f32(c, cc->mguf_vec[0].p, int64_t(cc->dim) * cc->nUo, cc->mguf_vec[4].p);
  else halo_reverse_add_f32(cc, cc->mguf_vec[0].p);
  mg_uu_vcycle(M, l + 1);
  halo_exchange_f32(cc, cc->mguf_vec[1].p);
  float *e = c->mguf_vec[4].p;
  mg_transfer_u(c, /*prolong=*/true, cc->mguf_vec[1].p, e);
  MfFuseT<float> f; // x += e; r -= A e; d = (1/theta) B r: the first direction of the post-smoothing sweep
  f.mode = 3; f.xs = x; f.r = r; f.d = c->mguf_vec[2].p; f.b = Cheb(mg_uu_sweep(M, l, true)).c0();
  const bool dir_follows = smoother_fuse_mode(c, f.mode);
  uu_apply_level_f32(S, e, &f);
  if (dir_follows) smoother_dir(c, 0.0, f.b, r, f.d);
  SmoothOpts post;
  post.d_ready = true; post.trim = trim; post.no_exit = top;
  mg_uu_smooth(M, l, mg_uu_sweep(M, l, true), x, r, post);
}
// the first direction of level 0 is (1 / theta) B r with the theta of the sweep the cycle starts with
static double mg_uu_entry_c0(const MgUu &M) { return Cheb(mg_uu_sweep(M, 0)).c0(); }

// the level chain of this application: every attached coarser level that has velocity transfers from the one above
MgUu::MgUu(SolveState &S_) : S(S_), c(S_.ctx), o(S_.o) {
  nu = std::max(1, o->mg_smooth_u); nu_post = o->mg_smooth_u_post > 0 ? o->mg_smooth_u_post : nu; ratio = std::max(1.5, o->mg_cheb_ratio_u);
  L.push_back(S);
  for (ifem_ctx *p = c; p->mg_coarse && p->mg_Pu.n_rows == p->nUo && p->nUo > 0; p = p->mg_coarse) {
    SolveState Sc{p->mg_coarse, S.P, o};
    carve_workspace(Sc, false);
    L.push_back(Sc);
  }
  if (!c->mf_valid) throw Error(IFEM_E_BADPARAM, "IFEM_AINV_MG needs the operator state of ifem_ins_assemble / ifem_imex_assemble");
  trim = c->tune.inner_f32 != 0;
  Amf = [this](const double *x, double *y) { uu_apply_level(S, x, y); };
  mdot = mdot_over(c, S.nuo);
}

// the cycle itself: eagerly, or as a captured hipGraph (ctx.hpp::VcGraph) on small single-rank chains
void MgUu::cycle() {
  if (!graph_ok) { mg_uu_vcycle(*this, 0); return; }
  std::vector<uint64_t> key;
  key.push_back(L.size()); key.push_back(uint64_t(nu)); key.push_back(uint64_t(nu_post)); key_f64(key, ratio);
  key.push_back(uint64_t(trim)); // which passes the captured cycle consists of
  for (const SolveState &l : L) uu_level_key(l.ctx, key);
  if (!graph_run(c, c->vc_graph, key, [&]() { mg_uu_vcycle(*this, 0); })) {
    c->tune.vcycle_graph_cells = 0;
    graph_ok = false;
    if (o->verbose) fprintf(stderr, "[ifem] hipGraph capture of the A_uu V-cycle failed: eager launches from now on\n");
  }
}

// the cycle between its entry and exit runs on the fixed level vectors (and is what a hipGraph captures): whatever vector it is
// applied to only appears as an argument of the entry and exit kernels outside of it
void MgUu::apply(const double *x, double *y) {
  if (!trim) {
    v_cvt_d2f(c, S.nuo, x, c->mguf_vec[0].p);
    cycle();
    v_cvt_f2d(c, S.nuo, c->mguf_vec[1].p, y);
    return;
  }
  smoother_entry(c, mg_uu_entry_c0(*this), x, c->mguf_vec[0].p, c->mguf_vec[2].p);
  cycle();
  vc_exit(c, S.nuo, c->mguf_vec[1].p, c->mguf_vec[2].p, y);
}
void MgUu::apply(const float *x, float *y) {
  smoother_entry(c, mg_uu_entry_c0(*this), x, c->mguf_vec[0].p, c->mguf_vec[2].p);
  cycle();
  vc_exit_f32(c, S.nuo, c->mguf_vec[1].p, c->mguf_vec[2].p, y);
}

// one attempt of A~^-1 with the V-cycle; returns false when the result is not finite (a Chebyshev bound below the
// spectral radius turns the smoothers into amplifiers)
bool MgUu::solve_once(const double *b, double *x, double tol) {
  const OpFn Vc = [this](const double *u, double *y) { apply(u, y); };
  if (o->inner_maxit == 0) { // A~^-1 := one V-cycle, no inner Krylov iteration (the outer solver is flexible)
    apply(b, x);
    S.st.inner_iters += 1;
  } else if (o->inner_maxit < 0) { // -k: k stationary V-cycle sweeps x += V(b - A x): no Arnoldi process, k - 1 operator products
    const int k = -o->inner_maxit;
    apply(b, x);
    for (int it = 1; it < k; ++it) {
      Amf(x, S.inner_w);
      v_axpby(c, S.nuo, 1.0, b, -1.0, S.inner_w); // r = b - A x
      apply(S.inner_w, S.inner_z);
      v_axpy(c, S.nuo, 1.0, S.inner_z, x);
    }
    S.st.inner_iters += k;
  } else { // flexible GMRES: the preconditioned directions are kept, so the update needs no extra V-cycle
    const int64_t ld = basis_ld(c, S.nuo);
    // restart length: the caller's, lengthened by the context when an application needed more than two restart cycles (lengthen_restart)
    const int mi = std::max(std::max(1, o->inner_restart), c->inner_restart_eff);
    int its;
    // one pair of bases per context: a change of ifem_tuning::inner_f32 gives the other pair back (a no-op when it is empty).  The fp64
    // basis the node-block-Jacobi fallback of solve() grows under inner_f32 = 1 is deliberately temporary: the next application frees it here
    if (trim) {
      c->innerV.release(); c->innerZ.release();
      grow_basis(c, c->innerVf, ld, std::min(mi + 1, kBasisStart), mi + 1);
      grow_basis(c, c->innerZf, ld, std::min(mi, kBasisStart), mi);
      const auto grow = basis_grower(c, c->innerVf, c->innerZf, ld, mi + 1);
      const OpF32 Amf32 = [this](const float *z, double *y) { uu_apply_f32col(c, z, y); }; // the product on a Z column of fgmres_f32
      const OpF32F32 Vcf = [this](const float *u, float *y) { apply(u, y); };
      its = fgmres_f32(c, S.nuo, ld, Amf, Amf32, Vcf, b, x, mi, o->inner_maxit, tol, c->innerVf.p, c->innerZf.p,
                       S.inner_w, &res, [this](double *v, int k) { allreduce_sum(c, v, k); }, grow);
    } else {
      c->innerVf.release(); c->innerZf.release();
      grow_basis(c, c->innerV, ld, std::min(mi + 1, kBasisStart), mi + 1);
      grow_basis(c, c->innerZ, ld, std::min(mi, kBasisStart), mi);
      const auto grow = basis_grower(c, c->innerV, c->innerZ, ld, mi + 1);
      its = gmres(c, S.nuo, ld, /*reorth=*/false, Amf, Vc, true, b, x, mi, o->inner_maxit, tol,
                  c->innerV.p, c->innerZ.p, S.inner_w, &res, mdot, nullptr, &grow);
    }
    S.st.inner_iters += its;
    lengthen_restart(its, mi);
  }
  if (o->inner_maxit > 0) return std::isfinite(res); // the Arnoldi recurrence carries any NaN / Inf of the V-cycle
  double dn;
  mdot(1, x, S.nuo, x, &dn);
  return std::isfinite(dn);
}

// An application that needed more than two restart cycles of GMRES(mi) lengthens the context's restart -- a V-cycle that has lost its mesh
// independence (the refined cylinder, DESIGN section 6: 147 inner iterations with GMRES(16), 75 with GMRES(40), 59 with GMRES(100))
// stagnates across restarts; the bases grow on demand, so the longer cycle costs memory only where it is used.  Capped at 128 columns and
// at a quarter of the free device memory.
void MgUu::lengthen_restart(int its, int mi) {
  if (!(its > 2 * mi && mi < 128)) return;
  size_t fr = 0, tot = 0;
  (void)hipMemGetInfo(&fr, &tot);
  int want = std::min(128, 2 * mi);
  const double per_col = 2.0 * double(basis_ld(c, S.nuo)) * (trim ? sizeof(float) : sizeof(double));
  int fits = int(std::min<double>(128.0, 0.25 * double(fr) / std::max(per_col, 1.0)));
  if (c->test_restart_fits > 0) fits = c->test_restart_fits; // test aid (ifem_test_restart_fits): a rank that is short of memory
  want = std::min(want, std::max(fits, mi));
  // `its` and `mi` are the same on every rank, free memory and `ld` are not: the restart length must be (the ranks restart
  // together -- their all-reduces and halo exchanges pair up), so the smallest wish of all ranks wins
  if (c->halo.nranks > 1) { double w = -double(want); allreduce_max(c, &w, 1); want = int(-w); }
  if (want > mi) {
    if (o->verbose) fprintf(stderr, "[ifem] inner GMRES(%d) needed %d iterations: restart length %d from now on\n", mi, its, want);
    c->inner_restart_eff = want;
  }
}

// x = A~^-1 b: inner GMRES on the matrix-free operator with one V-cycle as its preconditioner, to the absolute tolerance tol
void MgUu::solve(const double *b, double *x, double tol) {
  mg_uu_setup(*this);
  graph_ok = cycle_graph_ok(c, L);
  for (const SolveState &l : L) graph_ok = graph_ok && !l.ctx->profile;
  if (solve_once(b, x, tol)) return;
  // re-estimate every level's bound from scratch and try once more; if that fails too, this application falls back to
  // the node-block Jacobi preconditioned inner solve (the preconditioner degrades, the outer solver stays correct)
  if (o->verbose) fprintf(stderr, "[ifem] A_uu V-cycle returned non-finite values: re-estimating the Chebyshev bounds\n");
  mg_uu_setup(*this, /*force_bounds=*/true);
  res = 0;
  // the fused single-precision kernels read, with zero coefficients, up to 3 columns past the ones in use: none may keep a NaN
  if (c->innerVf.n) IFEM_HIP_CHECK(hipMemsetAsync(c->innerVf.p, 0, c->innerVf.n * sizeof(float), c->stream));
  if (c->innerZf.n) IFEM_HIP_CHECK(hipMemsetAsync(c->innerZf.p, 0, c->innerZf.n * sizeof(float), c->stream));
  if (solve_once(b, x, tol)) return;
  if (o->verbose) fprintf(stderr, "[ifem] A_uu V-cycle still non-finite: node-block Jacobi for this application\n");
  const OpFn Pbj = [this](const double *u, double *y) { bjac_apply(c, u, y); };
  res = 0;
  const int64_t ldj = basis_ld(c, S.nuo);
  const int mj = std::max(1, o->inner_restart);
  const std::function<void(int, double *&, double *&)> growv = [&](int cols, double *&V, double *&) {
    grow_basis(c, c->innerV, ldj, std::min(cols, mj + 1), mj + 1); // (not flexible: one z vector)
    V = c->innerV.p;
  };
  // gmres() stores its first basis vector before it asks `growv` for columns: the fp64 basis must exist here (with
  // ifem_tuning::inner_f32 the context has not allocated it before this fallback)
  grow_basis(c, c->innerV, ldj, std::min(mj + 1, kBasisStart), mj + 1);
  if (S.nuo > 0 && !c->innerV.p) throw Error(IFEM_E_BADPARAM, "inner GMRES: no basis storage");
  S.st.inner_iters += gmres(c, S.nuo, ldj, /*reorth=*/false, Amf, Pbj, false, b, x, mj,
                            std::max(o->inner_maxit, 50), tol, c->innerV.p, S.inner_z, S.inner_w, &res, mdot, nullptr, &growv);
}

// ---- the statements of InsIM::BlockSchurPreconditioner::vmult (mpi_insim.cpp:57-128), one function each.
// approx_kind: the approximate-preconditioner kinds, which stream M_p and S_m in single precision
static bool approx_kind(const ifem_solver_opts *o) {
  return o->ainv_kind == IFEM_AINV_GMRES_BJACOBI_F32 || o->ainv_kind == IFEM_AINV_GMRES_BJACOBI_MF || o->ainv_kind == IFEM_AINV_MG;
}
static int p_maxit(const ifem_ctx *c) { return (int)std::min<int64_t>(std::max<int64_t>(c->n_global_p, 1), 1 << 30); }

// CG for Mp (:69-84): x = M_p^-1 b to max(mp_abs, mp_rel ||b||)
// ... or, on a uniform box level whose pressure nodes fill the lattice (mp_direct.hip; ifem_solver_opts::mp_solver = 0), three sweeps of
// tridiagonal line solves: the solution to rounding, which meets mp_rel / mp_abs trivially; cg_mp_iters stays as it is.  Returns whether
// the direct path ran
static bool solve_mp(SolveState &S, const double *b, double *x) {
  ifem_ctx *c = S.ctx;
  const ifem_solver_opts *o = S.o;
  if (o->mp_solver == 0 && mp_direct_ready(c, o->verbose)) {
    mp_direct_apply(c, b, x);
    return true;
  }
  // the approximate-preconditioner kinds stream M_p in single precision like S_m (the solve is to 1e-6, the rounding of the
  // values 6e-8).  (p.q fused into this SpMV was measured: a block reduction in each of its 67 k small blocks costs more
  // than the separate pass over the two vectors.)
  const bool approx = approx_kind(o);
  const OpFn mp = [&](const double *u, double *y) {
    const double *ue = S.xp_ext;
    halo_apply(c, true, [&] { build_row_split(c, c->Mp, c->nPo); v_copy(c, S.npo, u, S.xp_ext); halo_start(c, S.xp_ext, 1); },
               [&] { extend_p(S, u, &ue); }, [&](int part) { spmv_mp(c, ue, y, part, approx); });
  };
  // ... and put a Jacobi preconditioner on this solve: same stopping rule on the true residual, fewer iterations (the reference uses
  // PreconditionNone; counts are no parity target)
  const bool pjac = approx;
  const double tol = std::max(o->mp_abs, o->mp_rel * S.p_src_norm);
  // device-resident recurrences on any number of ranks: the dot products are all-reduced on the stream (comm.hip::allreduce_sum_dev)
  if (pjac) scalar_diag(c, c->Mp, c->Mp.val.p, S.tp[5]);
  if (o->device_cg != 0)
    S.st.cg_mp_iters += cg_device(c, S.npo, mp, pjac ? S.tp[5] : nullptr, b, x, tol, p_maxit(c), S.tp[1], S.tp[2], S.tp[3], S.tp[4], 4, S.tp[6]);
  else if (pjac)
    S.st.cg_mp_iters += pcg_jacobi(c, S.npo, mp, S.tp[5], b, x, tol, p_maxit(c), S.tp[1], c->nPl, S.tp[3], S.tp[4], mdot_over(c, S.npo)); // r = tp[1], z = tp[2]
  else
    S.st.cg_mp_iters += cg(c, S.npo, mp, b, x, tol, p_maxit(c), S.tp[1], S.tp[2], S.tp[3], [&](const double *u, const double *v) { return dot_all(S, S.npo, u, v); });
  return false;
}

// CG for Sm (:86-112): x = S_m^-1 b to max(sm_abs, sm_rel ||b||)
static void solve_sm(SolveState &S, const double *b, double *x) {
  ifem_ctx *c = S.ctx;
  const ifem_solver_opts *o = S.o;
  const bool lowp = approx_kind(o);
  const double tol = std::max(o->sm_abs, o->sm_rel * S.p_src_norm);
  sm_ensure(S);
  // ifem_solver_opts::sm_mg = 2, a uniform box level whose factors passed the probe of the present S_m (sm_direct.hip): six contractions and a
  // scale, the solution to rounding; the coarser levels are not touched, cg_sm_iters stays as it is, sm_mg_levels stays 0
  if (o->sm_mg == 2 && sm_direct_ready(c)) {
    sm_direct_apply(c, b, x);
    return;
  }
  const OpFn sm = [&](const double *u, double *y) { sm_apply(S, u, y, lowp); };
  // multigrid-preconditioned CG when coarser levels are attached (every level needs its S_m explicitly: Jacobi smoothing)
  // (the finest level may apply S_m as two SpMVs -- several ranks without the 2-deep pressure halo, e.g. the strips of an unstructured
  // mesh above replicated coarse levels: the V-cycle needs the operator and its diagonal there, not the matrix)
  bool use_mg = o->sm_mg && c->mg_coarse && (sm_is_explicit(S) || (o->explicit_schur && c->halo.nranks > 1));
  MgSm M;
  if (use_mg) {
    M.lowp = lowp; M.nu = std::max(1, o->mg_smooth); M.ratio = std::max(1.5, o->mg_cheb_ratio);
    M.L.push_back(S);
    for (ifem_ctx *cc = c->mg_coarse; cc; cc = cc->mg_coarse) {
      SolveState Sc{cc, S.P, o};
      carve_workspace(Sc, false);
      if (!sm_is_explicit(Sc)) { use_mg = false; break; }
      M.L.push_back(Sc);
    }
  }
  if (use_mg) {
    mg_sm_setup(M, c->asm_constraint_set);
    S.st.cg_sm_iters += pcg_mg_sm(M, b, x, tol, p_maxit(c), S.tp[1], S.tp[2], S.tp[3], S.tp[4]);
    S.st.sm_mg_levels = (uint32_t)M.L.size();
  } else if (o->device_cg != 0) // (Jacobi on S_m was measured too: 176 instead of 172 iterations -- its diagonal is nearly constant)
    S.st.cg_sm_iters += cg_device(c, S.npo, sm, nullptr, b, x, tol, p_maxit(c), S.tp[1], S.tp[2], S.tp[3], S.tp[4], 4, S.tp[6]);
  else
    S.st.cg_sm_iters += cg(c, S.npo, sm, b, x, tol, p_maxit(c), S.tp[1], S.tp[2], S.tp[3], [&](const double *u, const double *v) { return dot_all(S, S.npo, u, v); });
}

// The relative tolerance of this application's inner solve: the first application of a solve may ask for a tighter one
// (ifem_solver_opts::inner_rel_first)
// ... when the residual it is applied to is velocity-dominated.  The block-triangular preconditioner leaves O(0.1) of the
// pressure part of a residual behind per outer iteration (the pressure Schur complement is only approximated, mpi_insim.cpp:
// 57-112), so a first Krylov vector whose pressure share exceeds ~10 fgmres_rel cannot be finished in one iteration by
// a better velocity solve -- the later Newton iterations, whose residual is almost all continuity equation (shares
// 0.996 / 0.66 against 7e-5 in the first one at 128^3): there the cheap setting is the better one (time_step leg of
// bench.py: 1.16 s against 1.27 s with the tight first application everywhere)
// ... and while it pays: a solve whose tight first application did NOT end the outer iteration at its first check has spent
// the extra inner iterations for nothing (64^3 channel: 2 outer iterations either way, 29.8 instead of 24.5 ms).  After such a
// miss the context leaves the option off for its next 8 / 16 / 32 / 64 qualifying solves (ins_solve keeps the count), then tries again.
static double inner_rel_now(SolveState &S) {
  const ifem_solver_opts *o = S.o;
  const double pshare_max = o->inner_first_pshare > 0 ? o->inner_first_pshare : 10.0 * o->fgmres_rel;
  const bool pressure_dominated = S.p_src_norm > pshare_max * std::hypot(S.u_src_norm, S.p_src_norm);
  bool tight = false;
  if (S.st.precond_applies == 0 && o->inner_rel_first > 0 && !pressure_dominated) {
    S.tight_candidate = true;
    tight = S.tight_used = S.ctx->tight_first_backoff == 0;
  }
  const double rel = tight ? o->inner_rel_first : o->inner_rel;
  if (o->verbose && S.st.precond_applies == 0)
    fprintf(stderr, "[ifem] first preconditioner application: pressure share of the residual %.3e, inner tolerance %.1e\n",
            S.p_src_norm / std::max(std::hypot(S.u_src_norm, S.p_src_norm), 1e-300), rel);
  return rel;
}

// A~^-1 (:124-127): x = A~^-1 b to rel ||b||, by the inner solver of ifem_solver_opts::ainv_kind
static void ainv_apply(SolveState &S, const double *b, double *x, double rel) {
  ifem_ctx *c = S.ctx;
  const ifem_solver_opts *o = S.o;
  if (!c->uu_is_stored && o->ainv_kind != IFEM_AINV_GMRES_BJACOBI_MF && o->ainv_kind != IFEM_AINV_MG)
    throw Error(IFEM_E_BADPARAM, "ifem_tuning::stored_uu = 0 keeps no A_uu values: use IFEM_AINV_MG or IFEM_AINV_GMRES_BJACOBI_MF (the matrix-free inner operators)");
  const bool scalar_op = o->ainv_kind == IFEM_AINV_SCALAR_GMRES;
  if (scalar_op) shat_refresh(c, true);
  const MdotFn mdot = mdot_over(c, S.nuo);
  double bn;
  mdot(1, b, S.nuo, b, &bn);
  const double tol = rel * std::sqrt(bn);
  if (o->ainv_kind == IFEM_AINV_MG) { // inner GMRES on the matrix-free operator, one V-cycle as its preconditioner
    MgUu(S).solve(b, x, tol);
    return;
  }
  const bool f32 = o->ainv_kind == IFEM_AINV_GMRES_BJACOBI_F32;
  OpFn Auu = [&](const double *u, double *y) { const double *ue; extend_u(S, u, &ue); spmv_uu(c, ue, nullptr, y, f32); };
  if (o->ainv_kind == IFEM_AINV_GMRES_BJACOBI_MF) Auu = [&](const double *u, double *y) { uu_apply_level(S, u, y); };
  if (scalar_op) Auu = [&](const double *u, double *y) { const double *ue; extend_u(S, u, &ue); spmv_shat(c, ue, y, true); };
  const OpFn Pj = [&](const double *u, double *y) { if (scalar_op) shat_jacobi(c, u, y); else bjac_apply(c, u, y); };
  // inner_maxit <= 0 means "one V-cycle / stationary sweeps" to IFEM_AINV_MG only; for the Krylov kinds it is the library default cap
  const int inner_cap = o->inner_maxit > 0 ? o->inner_maxit : 400;
  const bool f32_basis = (f32 || o->ainv_kind == IFEM_AINV_GMRES_BJACOBI_MF) && o->inner_restart + 6 <= 64;
  double res = 0;
  if (f32_basis) { // columns 0..m: basis, m+1: scratch for V y, up to the next multiple of 4: padding read by the fused kernels
    const OpF32 Pf = [&](const float *u, double *y) { bjac_apply_f32(c, u, y); };
    S.st.inner_iters += gmres_f32basis(c, S.nuo, basis_ld(c, S.nuo), Auu, Pf, b, x, o->inner_restart, inner_cap, tol,
                                       reinterpret_cast<float *>(c->innerV.p), S.inner_z, S.inner_w, &res,
                                       [&](double *v, int k) { allreduce_sum(c, v, k); });
  } else
    S.st.inner_iters += gmres(c, S.nuo, basis_ld(c, S.nuo), /*reorth=*/false, Auu, Pj, false, b, x, o->inner_restart,
                              inner_cap, tol, c->innerV.p, S.inner_z, S.inner_w, &res, mdot);
}

static void precond_vmult(SolveState &S, const double *src, double *dst) {
  ifem_ctx *c = S.ctx;
  const ifem_ins_params *P = S.P;
  const double *src0 = src, *src1 = src + S.nuo;
  double *dst0 = dst, *dst1 = dst + S.nuo;
  double *tmp = S.tp[0];
  S.p_src_norm = std::sqrt(dot_all(S, S.npo, src1, src1));
  if (S.st.precond_applies == 0 && S.o->inner_rel_first > 0) { // pressure share of the first Krylov vector (see inner_rel_now)
    double uu = 0;
    v_mdot(S.ctx, S.nuo, 1, src0, S.nuo, src0, &uu);
    allreduce_sum(S.ctx, &uu, 1);
    S.u_src_norm = std::sqrt(uu);
  }
  // section marks on the stream (read by precond_section_times once the solve is over)
  auto mark = [&]() {
    if (c->pc_ev.size() <= c->pc_used) {
      hipEvent_t e = nullptr;
      IFEM_HIP_CHECK(hipEventCreate(&e));
      c->pc_ev.push_back(e);
    }
    IFEM_HIP_CHECK(hipEventRecord(c->pc_ev[c->pc_used++], c->stream));
  };
  mark();
  // CG for Mp (:69-84)
  solve_mp(S, src1, tmp);
  v_scale(c, S.npo, -(P->viscosity + P->grad_div * P->rho), tmp);
  mark();
  // CG for Sm (:86-112)
  solve_sm(S, src1, dst1);
  v_axpby(c, S.npo, 1.0, tmp, -P->rho / P->dt, dst1);
  // utmp = src0 - B^T dst1 (:116-120)
  const double *xe; extend_p(S, dst1, &xe);
  spmv_bt(c, xe, S.utmp);
  v_axpby(c, S.nuo, 1.0, src0, -1.0, S.utmp);
  mark();
  // A~^-1 utmp (:124-127)
  ainv_apply(S, S.utmp, dst0, inner_rel_now(S));
  mark();
  S.st.precond_applies++;
}

// device time of the three sections of every preconditioner application since pc_used was reset; the stream must be idle
static void precond_section_times(ifem_ctx *c, ifem_solve_stats &st) {
  for (size_t k = 0; k + 3 < c->pc_used; k += 4) {
    float a = 0, b = 0, d = 0;
    if (hipEventElapsedTime(&a, c->pc_ev[k], c->pc_ev[k + 1]) == hipSuccess && hipEventElapsedTime(&b, c->pc_ev[k + 1], c->pc_ev[k + 2]) == hipSuccess &&
        hipEventElapsedTime(&d, c->pc_ev[k + 2], c->pc_ev[k + 3]) == hipSuccess) {
      st.t_cg_mp_ms += a; st.t_cg_sm_ms += b; st.t_ainv_ms += d;
    }
  }
  c->pc_used = 0;
}

// The inner Krylov basis is shared by every solver of the context.  The single-precision-basis kernels read (with zero
// coefficients) up to 3 columns past the ones in use, so the buffer is zero-filled whenever it is (re)allocated: 0 * NaN
// from uninitialised memory would poison the preconditioner.
static void grow_inner_basis(ifem_ctx *c, int64_t need) { ensure_zeroed(c, c->innerV, need); }

static void carve_workspace(SolveState &S, bool krylov) {
  ifem_ctx *c = S.ctx;
  const int64_t nul = c->dim * c->nUl, npl = c->nPl;
  S.nuo = c->dim * c->nUo; S.npo = c->nPo; S.n = S.nuo + S.npo;
  const int64_t need = nul + npl + 4 * nul + 7 * npl + S.n + 64;
  if ((int64_t)c->work.n < need) c->work.alloc(need);
  double *p = c->work.p;
  S.xu_ext = p; p += nul;
  S.xp_ext = p; p += npl;
  S.tu = p; p += nul;
  S.utmp = p; p += nul;
  S.inner_w = p; p += nul;
  S.inner_z = p; p += nul;
  for (int i = 0; i < 7; ++i) { S.tp[i] = p; p += npl; }
  S.outer_w = p;
  if (!krylov) return; // a coarse multigrid level: vector scratch only
  const int m = S.o->fgmres_restart, mi = S.o->inner_restart;
  grow_basis(c, c->krylovV, basis_ld(S.ctx, S.n), std::min(m + 1, kBasisStart), m + 1); // the rest on demand (basis_grower)
  grow_basis(c, c->krylovZ, basis_ld(S.ctx, S.n), std::min(m, kBasisStart), m);
  // the inner solve of IFEM_AINV_MG is flexible too and grows its bases the same way; the other kinds' kernels want theirs whole
  // (its single-precision bases, ifem_tuning::inner_f32, are the solver's own: MgUu::solve_once allocates them where it runs that solver)
  if (!(S.o->ainv_kind == IFEM_AINV_MG && c->tune.inner_f32 && S.o->inner_maxit > 0))
    grow_inner_basis(c, (int64_t)(S.o->ainv_kind == IFEM_AINV_MG ? std::min(mi + 1, kBasisStart) : mi + 1) * basis_ld(S.ctx, S.nuo));
}

// a SolveState on the library's default options, for the entry points that are no solve.  The options it points to are this function's and outlive it
static SolveState default_state(ifem_ctx *ctx) {
  static const ifem_solver_opts o = [] { ifem_solver_opts d; ifem_default_solver_opts(&d); return d; }();
  SolveState S{ctx, nullptr, &o}; carve_workspace(S);
  return S;
}

void ins_precond_vmult(ifem_ctx *ctx, const ifem_ins_params *P, const ifem_solver_opts *o, const double *src, double *dst) {
  SolveState S{ctx, P, o};
  carve_workspace(S);
  ctx->pc_used = 0;
  precond_vmult(S, src, dst);
  ctx->pc_used = 0;
}

void mp_solve_probe(ifem_ctx *ctx, const ifem_solver_opts *o, const double *b, double *x, int32_t info[2]) {
  SolveState S{ctx, nullptr, o};
  carve_workspace(S);
  S.p_src_norm = std::sqrt(dot_all(S, S.npo, b, b));
  info[0] = solve_mp(S, b, x) ? 1 : 0;
  info[1] = int32_t(S.st.cg_mp_iters);
}

// ifem_test_sm_solve: x = what solve_sm produces for b under o; info = {1 direct / 0 CG, CG iterations, probe value x 1e18 (0: no direct path),
// bytes of the factor tables}
void sm_solve_probe(ifem_ctx *ctx, const ifem_solver_opts *o, const double *b, double *x, int64_t info[4]) {
  SolveState S{ctx, nullptr, o};
  carve_workspace(S);
  S.p_src_norm = std::sqrt(dot_all(S, S.npo, b, b));
  solve_sm(S, b, x);
  const bool direct = o->sm_mg == 2 && sm_direct_ready(ctx);
  info[0] = direct ? 1 : 0;
  info[1] = int64_t(S.st.cg_sm_iters);
  info[2] = direct ? int64_t(std::llround(std::min(ctx->sm_direct.probe, 9.0) * 1e18)) : 0;
  info[3] = direct ? int64_t(ctx->sm_direct.bytes()) : 0;
}

// what the two test aids below report of a lattice stencil product: `first` | classes | irregular rows | table bytes, zeros while it is off
static void stencil_info(const StencilClasses &T, bool on, int64_t first, int64_t info[4]) {
  info[0] = on ? first : 0;
  info[1] = on ? T.classes : 0;
  info[2] = on ? T.n_irregular : 0;
  info[3] = on ? int64_t(T.table.n * sizeof(double)) : 0;
}

// ifem_test_sm_apply: y = S_m x on device vectors of owned pressure nodes.  path 0: the fp64 CSR product of the assembled matrix (one rank); 1: sm_apply
// as the solves of the default options call it (several ranks: collective, the distributed explicit product or the two SpMVs); 2 / 3: switch the
// stencil path of this context off / on again (x, y unused; 3 also makes the tables of the present S_m when that is formed already)
void sm_apply_probe(ifem_ctx *ctx, int path, const double *x, double *y, int64_t info[4]) {
  SmStencil &T = ctx->sm_stencil;
  if (path == 2 || path == 3) {
    T.off = path == 2;
    ctx->graph_epoch++; // captured cycles are keyed on the product they launch
    if (path == 3 && ctx->halo.nranks == 1 && ctx->sm_valid && ctx->Sm.n_rows > 0) sm_stencil_setup(ctx, 0); // S_m re-formed while the path was off
  } else {
    SolveState S = default_state(ctx);
    if (path == 0 && !sm_is_explicit(S)) throw Error(IFEM_E_BADPARAM, "ifem_test_sm_apply: this context keeps no explicit S_m");
    sm_ensure(S);
    if (path == 0) spmv_sm(ctx, x, y, false);
    else sm_apply(S, x, y, approx_kind(S.o));
  }
  stencil_info(T, sm_stencil_ready(ctx), 1, info);
}

// ifem_test_b_apply: y = B x (which 0), y = B^T x (1) or y += B^T x (2) on device vectors, x ghost-extended, y owned.  path 0: the fp64 CSR
// product of the assembled block; 1: what the solves launch (the tables are made first, as a solve's set-up makes them); 2 / 3: switch the stencil
// products of this context off / on again (x, y unused; 3 also makes the tables of the present blocks).  info: 0 when the product of `which` is the
// CSR one, otherwise the number of table builds this context has made so far | classes | irregular rows | table bytes
void b_apply_probe(ifem_ctx *ctx, int which, int path, const double *x, double *y, int64_t info[4]) {
  BbStencil &T = ctx->bb_stencil;
  const int blk = which ? 1 : 0;
  if (path == 2 || path == 3) {
    T.off = path == 2;
    ctx->graph_epoch++; // captured cycles are keyed on the products they launch
    if (path == 3) bb_stencil_setup(ctx, 0);
  } else {
    if (path == 1) bb_stencil_setup(ctx, 0);
    const bool stencil = path == 1 && bb_stencil_ready(ctx, blk);
    if (which == 0) {
      if (stencil) bb_stencil_apply_b(ctx, x, y);
      else spmv_b_rows(ctx, x, y, ctx->B.n_rows, nullptr);
    } else if (stencil) bb_stencil_apply_bt(ctx, x, y, which == 2);
    else spmv_bt_rows(ctx, x, y, ctx->Bt.n_rows, nullptr, which == 2);
  }
  stencil_info(blk ? T.bt : T.b, bb_stencil_ready(ctx, blk), T.builds, info);
}

// right-hand side of the condensed system after an assembly that treated the hanging dofs as ordinary ones:
// b = C^T (b^ - A^ c0) on the regular rows, d_h c0_h on the hanging rows (distribute_local_to_global semantics)
void hanging_condense_rhs(ifem_ctx *ctx, int use_nonzero) {
  if (!ctx->hang.active) return;
  SolveState S = default_state(ctx);
  hanging_refresh_diag(ctx);
  double *rhs = ctx->vec[IFEM_VEC_RHS].p;
  const bool inhom = hanging_offset(ctx, use_nonzero); // c0: ghost-extended, zero away from the hanging entries
  if (inhom) {
    system_apply_ext(S, ctx->hang.c0.p, ctx->hang.c0.p + int64_t(ctx->dim) * ctx->nUl, S.outer_w, false);
    v_axpy(ctx, S.n, -1.0, S.outer_w, rhs);
  }
  hanging_output(ctx, ctx->hang.c0.p, true, rhs);
}

void ins_system_vmult(ifem_ctx *ctx, const double *src, double *dst) {
  SolveState S = default_state(ctx);
  system_apply(S, src, dst, false);
}

// SUPGFluidSolver::solve + BlockIncompSchurPreconditioner::vmult (mpi_supg_solver.cpp:35-192, 297-328).
//   P_vv^-1  : node-block Jacobi of A_vv            (reference: Hypre-Euclid ILU(0))
//   T_pp     : A_pp - A_pv P_vv^-1 A_vp, solved by GMRES(200) to 1e-3 ||.|| with the ILU(0) of the explicit T_pp
//                                                   (reference: ILU(0) of B2pp = A_pp - A_pv rowsum|A_vv|^-1 A_vp)
// what deal.II's SolverControl::NoConvergence carries: the last step and the last residual
void throw_noconv(const char *solver, int it, double res, double tol) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s did not converge (SolverControl::NoConvergence): residual %.6e after %d iteration%s, tolerance %.6e%s", solver, res, it,
           it == 1 ? "" : "s", tol, std::isfinite(res) ? "" : " -- the system holds non-finite values (check the state vectors)");
  throw Error(IFEM_E_KRYLOV_NOCONV, msg);
}

// constructor of BlockIncompSchurPreconditioner (mpi_supg_solver.cpp:35-134) in the reference's structure: ILU(0)(A_vv), B2pp and its
// ILU(0); cached until the next assembly
void scns_refpc_setup(ifem_ctx *ctx, int verbose, bool *pvv_ok, bool *b2_ok) {
  BIlu &Iv = ctx->pvv_ilu, &Ip = ctx->b2_ilu;
#if !IFEM_UU_INTERLEAVED
  throw Error(IFEM_E_BADPARAM, "scns_pc = 2 needs the block-interleaved A_uu layout");
#endif
  if (!Iv.analysed) bilu_analyse(ctx, Iv, ctx->dim, ctx->nUo, ctx->Auu.rowptr.p, ctx->Auu.col.p);
  *pvv_ok = Iv.factored ? !Iv.broken : bilu_factor(ctx, Iv, stored_uu(ctx).p);
  if (!*pvv_ok && verbose) fprintf(stderr, "[ifem] scns solve: ILU(0) of A_vv broke down: node-block Jacobi instead\n");
  const PlanarCsr &Pt = tpp_pattern(ctx);
  if (!ctx->b2_valid) {
    const size_t nb = (size_t)ctx->nUo * ctx->dim * ctx->dim;
    if (ctx->rsinv.n != nb) ctx->rsinv.alloc(nb);
    if (ctx->B2pp.n != (size_t)Pt.nnzb) ctx->B2pp.alloc((size_t)Pt.nnzb);
    rowsum_abs_inv(ctx, ctx->rsinv.p);
    schur_pp_numeric(ctx, ctx->rsinv.p, ctx->B2pp.p);
    ctx->b2_valid = true; Ip.factored = false;
  }
  if (!Ip.analysed) bilu_analyse(ctx, Ip, 1, Pt.n_rows, Pt.rowptr.p, Pt.col.p);
  *b2_ok = Ip.factored ? !Ip.broken : bilu_factor(ctx, Ip, ctx->B2pp.p);
  if (!*b2_ok && verbose) fprintf(stderr, "[ifem] scns solve: ILU(0) of B2pp broke down: Jacobi instead\n");
}

// test hook (ifem_scns_pc_probe, single rank): the pieces of the preconditioner on device vectors
void scns_pc_probe(ifem_ctx *ctx, int which, const double *x, double *y) {
  SolveState S = default_state(ctx);
  bool pvv_ok = false, b2_ok = false;
  scns_refpc_setup(ctx, 0, &pvv_ok, &b2_ok);
  if (!pvv_ok || !b2_ok) throw Error(IFEM_E_KRYLOV_NOCONV, "ILU(0) broke down");
  switch (which) {
  case 0: bilu_apply(ctx, ctx->pvv_ilu, ctx->tune.pvv_sweeps, x, y); break;
  case 1: bilu_apply(ctx, ctx->b2_ilu, ctx->tune.b2pp_sweeps, x, y); break;
  case 2: spmv_planar_scalar(ctx, tpp_pattern(ctx), ctx->B2pp.p, x, y); break;
  case 3: {
    spmv_bt(ctx, x, S.tu);
    bilu_apply(ctx, ctx->pvv_ilu, ctx->tune.pvv_sweeps, S.tu, S.utmp);
    spmv_b(ctx, S.utmp, S.tp[4]);
    spmv_app(ctx, x, y);
    v_axpy(ctx, S.npo, -1.0, S.tp[4], y);
    break;
  }
  default: throw Error(IFEM_E_BADPARAM, "ifem_scns_pc_probe: which must be 0..3");
  }
}

void scns_solve(ifem_ctx *ctx, const ifem_solver_opts *o, int use_nonzero, ifem_solve_stats *stats) {
  if (!ctx->assembled || !ctx->has_app) throw Error(IFEM_E_BADPARAM, "ifem_scns_solve called before ifem_scns_assemble");
  SolveState S{ctx, nullptr, o};
  carve_workspace(S);
  Clock total;
  app_diag_setup(ctx);
  const int mt = 200;
  grow_inner_basis(ctx, (int64_t)(mt + 1) * basis_ld(S.ctx, S.npo));
  double *rhs = ctx->vec[IFEM_VEC_RHS].p, *upd = ctx->vec[IFEM_VEC_UPDATE].p;
  const MdotFn mdot = mdot_over(ctx, S.n);
  const MdotFn mdot_p = mdot_over(ctx, S.npo);
  double bn;
  mdot(1, rhs, S.n, rhs, &bn);
  bn = std::sqrt(bn);
  const double tol = 1e-6 * bn; // mpi_supg_solver.cpp:311-312
  const int64_t n_glob = ctx->n_global_u + ctx->n_global_p; // identical on all ranks
  const int maxit = o->fgmres_maxit > 0 ? o->fgmres_maxit : (int)std::min<int64_t>(n_glob, 1 << 30);
  OpFn Aop = [&](const double *x, double *y) { system_apply(S, x, y, false); };
  // y_u = A_vp x_p and y_p = A_pv x_u on compact owned vectors (ghosts refreshed first on several ranks)
  auto bt_apply = [&](const double *xp, double *yu) { const double *xe; extend_p(S, xp, &xe); spmv_bt(ctx, xe, yu); };
  auto b_apply = [&](const double *xu, double *yp) { const double *xe; extend_u(S, xu, &xe); spmv_b(ctx, xe, yp); };
  OpFn Tpp = [&](const double *x, double *y) {
    const double *xe; extend_p(S, x, &xe);
    spmv_bt(ctx, xe, S.tu);
    bjac_apply(ctx, S.tu, S.utmp);
    b_apply(S.utmp, S.tp[4]);
    spmv_app(ctx, xe, y);
    v_axpy(ctx, S.npo, -1.0, S.tp[4], y);
  };
  OpFn Jpp = [&](const double *x, double *y) { vec_div(ctx, S.npo, ctx->app_diag.p, x, y); };
  // one rank: T_pp as an explicit matrix (tpp.hip): one SpMV per inner iteration, and the inner GMRES preconditioned by the
  // ILU(0) of that matrix (the reference: Euclid ILU(0) of B2pp, mpi_supg_solver.cpp:141-192, preconditioner_pilut.cpp:124-138),
  // factorised once per Newton iteration and applied by level-scheduled triangular solves.  Several ranks: the operator stays
  // distributed, the preconditioner is the ILU(0) of the owned x owned block of T_pp on every rank (block-Jacobi ILU: what
  // Euclid does across ranks, mpi_supg_solver.cpp:49-53,120-133).  ifem_tuning::tpp_operator keeps the operator form with
  // Jacobi, tpp_ilu_order = -1 the explicit matrix with Jacobi.  A factorisation that breaks down (zero / tiny / non-finite
  // pivot) is not applied: Jacobi instead.
  // ifem_tuning::scns_pc = 2 (default): the reference's structure.  P_vv^-1 = ILU(0) of A_vv (mpi_supg_solver.cpp:49-51), T_pp the
  // operator A_pp - A_pv P_vv^-1 A_vp (:19-32), the inner GMRES(200) preconditioned by the ILU(0) of the assembled
  // B2pp = A_pp - A_pv rowsum(|A_vv|)^-1 A_vp (:56-133); both factorisations once per Newton iteration, applied by Jacobi sweeps on
  // the triangular systems (bilu.hip).  A factorisation that breaks down falls back to (node-block) Jacobi.
  const bool refpc = ctx->tune.scns_pc == 2;
  bool pvv_ok = false;
  OpFn Pvv = [&](const double *x, double *y) {
    if (pvv_ok) bilu_apply(ctx, ctx->pvv_ilu, ctx->tune.pvv_sweeps, x, y);
    else bjac_apply(ctx, x, y);
  };
  bool b2_ok = false;
  if (refpc) {
    scns_refpc_setup(ctx, o->verbose, &pvv_ok, &b2_ok);
    Tpp = [&](const double *x, double *y) { // SchurComplementTpp::vmult
      const double *xe; extend_p(S, x, &xe);
      spmv_bt(ctx, xe, S.tu);
      Pvv(S.tu, S.utmp);
      b_apply(S.utmp, S.tp[4]);
      spmv_app(ctx, xe, y);
      v_axpy(ctx, S.npo, -1.0, S.tp[4], y);
    };
    if (b2_ok) Jpp = [&](const double *x, double *y) { bilu_apply(ctx, ctx->b2_ilu, ctx->tune.b2pp_sweeps, x, y); };
  }
  // w = B2pp_inverse (T_pp stage) of the inner iteration: ~20 short launches with constant arguments (the Jacobi sweeps of the two ILU(0)
  // applications, three SpMVs) whose cost is the host's launch rate -- one captured hipGraph on a single rank (ifem_tuning::scns_graph)
  bool pa_graph_ok = refpc && ctx->tune.scns_graph != 0 && ctx->halo.nranks == 1 && !ctx->profile && !ctx->kprof.on && !profiler_attached();
  OpFn PAg = [&](const double *x, double *y) {
    auto body = [&]() { Tpp(x, S.tp[1]); Jpp(S.tp[1], y); };
    if (!pa_graph_ok) { body(); return; }
    std::vector<uint64_t> key;
    for (const void *p : {(const void *)x, (const void *)y, (const void *)S.tp[1], (const void *)S.tp[4], (const void *)S.tu, (const void *)S.utmp,
                          (const void *)ctx->App.p, (const void *)ctx->B.val.p, (const void *)ctx->Bt.val.p})
      key_ptr(key, p);
    for (const BIlu *I : {&ctx->pvv_ilu, &ctx->b2_ilu})
      for (const void *p : {(const void *)I->rp.p, (const void *)I->col.p, (const void *)I->diag.p, (const void *)I->LU.p, (const void *)I->dinv.p,
                            (const void *)I->t0.p, (const void *)I->t1.p, (const void *)I->t2.p})
        key_ptr(key, p);
    key.push_back(uint64_t(ctx->tune.pvv_sweeps)); key.push_back(uint64_t(ctx->tune.b2pp_sweeps)); key.push_back(uint64_t(pvv_ok)); key.push_back(uint64_t(b2_ok));
    key.push_back(uint64_t(ctx->pvv_ilu.nnz)); key.push_back(uint64_t(ctx->b2_ilu.nnz));
    if (!graph_run(ctx, ctx->pa_graph, key, body)) pa_graph_ok = false;
  };
  const bool tpp_explicit = !refpc && ctx->halo.nranks == 1 && !ctx->tune.tpp_operator;
  auto ilu_or_warn = [&]() {
    const bool ok = tpp_ilu_factor(ctx);
    if (!ok && o->verbose)
      fprintf(stderr, "[ifem] scns solve: ILU(0) of T_pp broke down (|pivot| in [%.3e, %.3e]): Jacobi instead\n", ctx->tpp_ilu.pivot_min,
              ctx->tpp_ilu.pivot_max);
    return ok;
  };
  if (tpp_explicit) {
    tpp_numeric(ctx);
    Tpp = [&](const double *x, double *y) { spmv_tpp(ctx, x, y); };
    if (ctx->tune.tpp_ilu_order >= 0 && ilu_or_warn())
      Jpp = [&](const double *x, double *y) { tpp_ilu_apply(ctx, x, y); };
    else
      Jpp = [&](const double *x, double *y) { vec_div(ctx, S.npo, ctx->tpp_diag.p, x, y); };
  } else if (!refpc && ctx->halo.nranks > 1 && !ctx->tune.tpp_operator && ctx->tune.tpp_ilu_order >= 0) {
    tpp_numeric(ctx); // the owned x owned block
    if (ilu_or_warn()) Jpp = [&](const double *x, double *y) { tpp_ilu_apply(ctx, x, y); };
  }
  OpFn Pop = [&](const double *src, double *dst) {
    const double *src0 = src, *src1 = src + S.nuo;
    double *dst0 = dst, *dst1 = dst + S.nuo;
    Pvv(src0, S.inner_w);                          // ptmp1 = P_vv^-1 src0
    b_apply(S.inner_w, S.tp[0]);                   // A_pv ptmp1
    v_axpby(ctx, S.npo, 1.0, src1, -1.0, S.tp[0]); // ptmp = src1 - A_pv ptmp1
    double pn;
    mdot_p(1, S.tp[0], S.npo, S.tp[0], &pn);
    double res = 0;
    const double inner_tol = 1e-3 * std::sqrt(pn);
    if (refpc && pn > 0) {
      // initial guess alpha ptmp with alpha = (ptmp . ptmp) / (T_pp ptmp . ptmp) (:165-171); the Krylov solve runs on the correction
      // with the same ABSOLUTE tolerance 1e-3 ||ptmp|| (:174-175)
      Tpp(S.tp[0], S.tp[6]);
      double sc;
      mdot_p(1, S.tp[6], S.npo, S.tp[0], &sc);
      const double alpha = sc != 0 && std::isfinite(sc) ? pn / sc : 0.0;
      v_axpby(ctx, S.npo, 1.0, S.tp[0], -alpha, S.tp[6]); // r0 = ptmp - alpha T_pp ptmp
      const LeftPrecond left_pc{S.tp[5], pa_graph_ok ? &PAg : nullptr};
      S.st.inner_iters += gmres(ctx, S.npo, basis_ld(S.ctx, S.npo), ctx->tune.scns_inner_reorth != 0, Tpp, Jpp, false, S.tp[6], dst1, mt, 100000,
                                inner_tol, ctx->innerV.p, S.tp[1], S.tp[2], &res, mdot_p, nullptr, nullptr, ctx->tune.scns_inner_left != 0 ? &left_pc : nullptr);
      v_axpy(ctx, S.npo, alpha, S.tp[0], dst1);
    } else
      S.st.inner_iters += gmres(ctx, S.npo, basis_ld(S.ctx, S.npo), /*reorth=*/true, Tpp, Jpp, false, S.tp[0], dst1, mt, 100000, inner_tol,
                                ctx->innerV.p, S.tp[1], S.tp[2], &res, mdot_p);
    bt_apply(dst1, S.tu);                          // A_vp dst1
    Pvv(S.tu, S.utmp);
    v_copy(ctx, S.nuo, S.inner_w, dst0);
    v_axpy(ctx, S.nuo, -1.0, S.utmp, dst0);        // dst0 = P_vv^-1 src0 - P_vv^-1 A_vp dst1
    S.st.precond_applies++;
  };
  double res = 0;
  const auto grow = basis_grower(ctx, ctx->krylovV, ctx->krylovZ, basis_ld(S.ctx, S.n), o->fgmres_restart + 1);
  const int it = gmres(ctx, S.n, basis_ld(S.ctx, S.n), true, Aop, Pop, true, rhs, upd, o->fgmres_restart, maxit, tol, ctx->krylovV.p,
                       ctx->krylovZ.p, S.outer_w, &res, mdot, nullptr, &grow);
  apply_constraints(ctx, use_nonzero ? 1 : 0, upd);
  hanging_distribute(ctx, upd);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  S.st.fgmres_iters = it; S.st.fgmres_res = res; S.st.t_total_ms = total.ms();
  if (stats) *stats = S.st;
  if (o->verbose)
    fprintf(stderr, "[ifem] scns solve: fgmres %d its res %.3e (tol %.3e) | inner Tpp its %u | %.1f ms\n", it, res, tol,
            S.st.inner_iters, S.st.t_total_ms);
  if (!(res <= tol)) throw_noconv("FGMRES", it, res, tol);
}

void ins_solve(ifem_ctx *ctx, const ifem_ins_params *P, const ifem_solver_opts *o, int use_nonzero,
               ifem_solve_stats *stats) {
  if (!ctx->assembled) throw Error(IFEM_E_BADPARAM, "ifem_solve called before ifem_ins_assemble");
  SolveState S{ctx, P, o};
  carve_workspace(S);
  Clock total;
  bb_stencil_setup(ctx, o->verbose); // (re)builds and probes the lattice tables of B and B^T when an assembly wrote the blocks: set-up time only
  ctx->pc_used = 0;
  ctx->spmv_uu_ms_total = 0;
  ctx->timing.spmv_uu_calls = 0;
  ctx->mf_ms_total = 0;
  ctx->timing.mf_calls = 0;
  double *rhs = ctx->vec[IFEM_VEC_RHS].p, *upd = ctx->vec[IFEM_VEC_UPDATE].p;
  const MdotFn mdot = mdot_over(ctx, S.n);
  double bn;
  mdot(1, rhs, S.n, rhs, &bn);
  bn = std::sqrt(bn);
  const double tol = std::max(o->fgmres_abs, o->fgmres_rel * bn);
  const int64_t n_glob = ctx->n_global_u + ctx->n_global_p; // SolverControl(system_matrix.m(), ...): identical on all ranks
  const int maxit = o->fgmres_maxit > 0 ? o->fgmres_maxit : (int)std::min<int64_t>(n_glob, 1 << 30);
  OpFn Aop = [&](const double *x, double *y) { system_apply(S, x, y, true); };
  OpFn Pop = [&](const double *x, double *y) { precond_vmult(S, x, y); };
  double res = 0;
  std::vector<double> hist;
  const auto grow = basis_grower(ctx, ctx->krylovV, ctx->krylovZ, basis_ld(S.ctx, S.n), o->fgmres_restart + 1);
  const int it = gmres(ctx, S.n, basis_ld(S.ctx, S.n), /*reorth=*/true, Aop, Pop, true, rhs, upd, o->fgmres_restart, maxit, tol, ctx->krylovV.p, ctx->krylovZ.p,
                       S.outer_w, &res, mdot, o->verbose ? &hist : nullptr, &grow);
  apply_constraints(ctx, use_nonzero ? 1 : 0, upd); // constraints_used.distribute(newton_update)
  hanging_distribute(ctx, upd);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  // inner_rel_first pays only when it ends the outer iteration at its first check (inner_rel_now); `it` is the same on all ranks
  if (S.tight_used) {
    if (it <= 1) ctx->tight_first_misses = 0;
    else { ctx->tight_first_misses = std::min(ctx->tight_first_misses + 1, 4); ctx->tight_first_backoff = 4 << ctx->tight_first_misses; }
  } else if (S.tight_candidate && ctx->tight_first_backoff > 0)
    ctx->tight_first_backoff--;
  S.st.inner_first_tight = S.tight_used ? 1u : 0u;
  precond_section_times(ctx, S.st); // (the stream was synchronised above)
  S.st.fgmres_iters = it;
  S.st.fgmres_res = res;
  S.st.t_total_ms = total.ms();
  S.st.t_spmv_ms = ctx->spmv_uu_ms_total;
  ctx->timing.mf_ms_avg = ctx->timing.mf_calls ? ctx->mf_ms_total / ctx->timing.mf_calls : 0;
  ctx->timing.spmv_uu_ms_avg = ctx->timing.spmv_uu_calls ? ctx->spmv_uu_ms_total / ctx->timing.spmv_uu_calls : 0;
  if (stats) *stats = S.st;
  if (o->verbose)
    fprintf(stderr, "[ifem] solve: fgmres %d its res %.3e (tol %.3e) | P applies %u CG(Mp) %u (%.1f ms) CG(Sm) %u (%.1f ms) inner %u (%.1f ms) | %.1f ms\n",
            it, res, tol, S.st.precond_applies, S.st.cg_mp_iters, S.st.t_cg_mp_ms, S.st.cg_sm_iters, S.st.t_cg_sm_ms, S.st.inner_iters, S.st.t_ainv_ms, S.st.t_total_ms);
  if (o->verbose) {
    fprintf(stderr, "[ifem] solve: ||rhs|| %.3e, relative residual per FGMRES iteration:", bn);
    for (double r : hist) fprintf(stderr, " %.2e", r / bn);
    fprintf(stderr, "\n");
  }
  if (!(res <= tol)) throw_noconv("FGMRES", it, res, tol);
}

} // namespace ifem
