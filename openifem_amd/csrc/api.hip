// api.hip -- the extern "C" surface declared in include/ifem_hip.h.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/ifem_hip_testing.h"
#include "ctx.hpp"
#include "kernels.hpp"
#include "sa_wall_function.hpp"

using namespace ifem;

static thread_local std::string g_err;

#define IFEM_API_BEGIN try {
#define IFEM_API_END                                           \
  }                                                            \
  catch (const ifem::Error &e) { g_err = e.what(); return e.code; } \
  catch (const std::exception &e) { g_err = e.what(); return IFEM_E_HIP; } \
  return IFEM_OK;

namespace ifem {
__global__ void k_flags_diff(int64_t n, const uint8_t *a, const uint8_t *b, unsigned long long *out) {
  unsigned long long d = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d += a[i] != b[i];
  if (d) atomicAdd(out, d);
}
__global__ void k_constraint_scatter(int32_t n, const int32_t *dof, const double *val, uint8_t *flag, double *cval) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flag[dof[i]] = 1;
  cval[dof[i]] = val[i];
}

// Only the n lines cross the bus; flags and inhomogeneities over [0, N) are built on the device (FSI re-makes the constraints every
// time step, mpi_fsi.cpp:1191: at 128^3 the dense host arrays were 480 MB per call).  See kernels.hpp.
bool build_line_set(ifem_ctx *ctx, size_t N, int32_t n, const int32_t *idx, const double *val, std::vector<int32_t> &kept_idx,
                    std::vector<double> &kept_val, DBuf<uint8_t> &flag, DBuf<double> &cval) {
  kept_idx.clear(); kept_val.clear();
  kept_idx.reserve((size_t)n); kept_val.reserve((size_t)n);
  std::vector<uint8_t> &seen = ctx->seen_scratch; // all zero between calls
  if (seen.size() < N) seen.assign(N, 0);
  bool in_range = true;
  for (int32_t i = n - 1; i >= 0; --i) {
    const int32_t d = idx[i];
    if (d < 0 || (size_t)d >= N) { in_range = false; break; }
    if (seen[d]) continue;
    seen[d] = 1;
    kept_idx.push_back(d);
    kept_val.push_back(val ? val[i] : 0.0);
  }
  for (int32_t d : kept_idx) seen[d] = 0;
  if (!in_range) return false;
  hipStream_t s = ctx->stream;
  flag.alloc(N);
  cval.alloc(N);
  if (N) {
    IFEM_HIP_CHECK(hipMemsetAsync(flag.p, 0, N, s));
    IFEM_HIP_CHECK(hipMemsetAsync(cval.p, 0, N * sizeof(double), s));
  }
  if (!kept_idx.empty()) {
    DBuf<int32_t> d_idx;
    DBuf<double> d_val;
    d_idx.upload(kept_idx.data(), kept_idx.size(), s);
    d_val.upload(kept_val.data(), kept_val.size(), s);
    hipLaunchKernelGGL(k_constraint_scatter, dim3((unsigned)((kept_idx.size() + 255) / 256)), dim3(256), 0, s, (int32_t)kept_idx.size(), d_idx.p, d_val.p, flag.p, cval.p);
    IFEM_HIP_CHECK(hipGetLastError());
    IFEM_HIP_CHECK(hipStreamSynchronize(s)); // d_idx, d_val are released on return
  }
  return true;
}

// the loop of run_one_step in the three solvers (its head: mpi_insim.cpp:420-427, mpi_supg_solver.cpp:354-355, mpi_spalart_allmaras.cpp:296-297).
// See kernels.hpp.
int newton_loop(double floor, int apply_nonzero, double tolerance, int max_iterations, double *log, const std::function<NewtonIter(int)> &iteration) {
  int outer = 0;
  double cur = 1.0, init = 1.0, rel = 1.0;
  while (rel > tolerance && cur > floor) {
    if (outer >= max_iterations) throw Error(IFEM_E_NEWTON_MAXIT, "Too many Newton iterations!");
    const NewtonIter it = iteration(apply_nonzero && outer == 0);
    cur = it.rhs_norm;
    if (outer == 0) init = cur;
    rel = cur / init;
    if (log) { log[outer * 4 + 0] = cur; log[outer * 4 + 1] = rel; log[outer * 4 + 2] = it.log2; log[outer * 4 + 3] = it.log3; }
    ++outer;
  }
  return outer;
}

// out[k] = 1 when the flag arrays of pair k differ somewhere (a never-set array differs from everything), compared on the
// device: the flags of a 128^3 mesh are 53 MB, the answer is a word
void flags_differ(ifem_ctx *ctx, int npairs, const DBuf<uint8_t> *const *a, const DBuf<uint8_t> *const *b, double *out) {
  const size_t N = (size_t)ctx->n_local;
  unsigned long long *cnt = reinterpret_cast<unsigned long long *>(ctx->scal.p + kScalStageOff); // staging slots, idle here
  IFEM_HIP_CHECK(hipMemsetAsync(cnt, 0, npairs * sizeof(unsigned long long), ctx->stream));
  for (int k = 0; k < npairs; ++k)
    if (a[k]->n == N && b[k]->n == N && N)
      hipLaunchKernelGGL(k_flags_diff, dim3(1024), dim3(256), 0, ctx->stream, (int64_t)N, a[k]->p, b[k]->p, cnt + k);
  unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  IFEM_HIP_CHECK(hipMemcpyAsync(h, cnt, npairs * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < npairs; ++k) out[k] = (a[k]->n != N || b[k]->n != N || h[k] != 0) ? 1.0 : 0.0;
}

// identity of the constrained-dof set (ctx.hpp) after the flags of set `which` changed: differs_self = they are not what
// they were, differs_other = they are not the other set's either.  Decided over ALL ranks, since a stale cache triggers
// collective work.
void constraint_set_identity(ifem_ctx *ctx, int which, bool differs_self, bool differs_other) {
  const int other = 1 - which;
  double differs[2] = {differs_self ? 1.0 : 0.0, differs_other ? 1.0 : 0.0};
  allreduce_max(ctx, differs, 2);
  if (differs[0] != 0.0) ctx->flag_id[which] = differs[1] == 0.0 ? ctx->flag_id[other] : ++ctx->flag_counter;
}
} // namespace ifem

namespace {
template <typename T>
std::vector<T> download_range(const ifem::DBuf<T> &b, int64_t off, int64_t count, hipStream_t s) {
  if (off < 0 || count < 0 || size_t(off + count) > b.n) throw ifem::Error(IFEM_E_BADPARAM, "ifem_export_rows: slice outside its array");
  std::vector<T> h((size_t)count);
  if (count) {
    IFEM_HIP_CHECK(hipMemcpyAsync(h.data(), b.p + off, size_t(count) * sizeof(T), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
  }
  return h;
}

// the caller's options, or the defaults
ifem_solver_opts opts_or_default(const ifem_solver_opts *o) {
  ifem_solver_opts d;
  if (o) d = *o; else ifem_default_solver_opts(&d);
  return d;
}

// entry points that return a count (>= 0) instead of IFEM_OK
template <class Body>
int api_count(Body &&body) {
  try { return body(); }
  catch (const ifem::Error &e) { g_err = e.what(); return e.code; }
  catch (const std::exception &e) { g_err = e.what(); return IFEM_E_HIP; }
}
} // namespace

extern "C" {

const char *ifem_last_error(void) { return g_err.c_str(); }

int64_t ifem_abi_sizeof(int which) {
  switch (which) {
  case 0: return sizeof(ifem_mesh_desc);
  case 1: return sizeof(ifem_partition);
  case 2: return sizeof(ifem_ins_params);
  case 3: return sizeof(ifem_solver_opts);
  case 4: return sizeof(ifem_solve_stats);
  case 5: return sizeof(ifem_scns_params);
  case 6: return sizeof(ifem_timing);
  case 7: return sizeof(ifem_tuning);
  case 8: return sizeof(ifem_mg_transfer);
  case 9: return sizeof(ifem_fsi_solid);
  case 10: return sizeof(ifem_fsi_stats);
  case 11: return sizeof(ifem_comm_stats);
  case 12: return sizeof(ifem_kprof_entry);
  case 13: return sizeof(ifem_sa_params);
  case 64: return sizeof(ifem_scnsex_stats);
  case 65: return sizeof(ifem_sa_wall);
  default: return -1;
  }
}

int ifem_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void ifem_default_solver_opts(ifem_solver_opts *o) {
  o->fgmres_restart = 30; o->fgmres_maxit = 0; o->fgmres_rel = 1e-4; o->fgmres_abs = 1e-12;
  o->mp_rel = 1e-6; o->mp_abs = 1e-10; o->sm_rel = 1e-3; o->sm_abs = 1e-10;
  o->ainv_kind = IFEM_AINV_GMRES_BJACOBI; o->inner_restart = 30; o->inner_maxit = 400; o->inner_rel = 1e-2;
  o->explicit_schur = 1;
  o->outer_matrix_free = 0;
  o->device_cg = 1;
  o->verbose = 0;
  o->sm_mg = 1; o->mg_smooth = 2; o->mg_cheb_ratio = 4.0;
  o->mg_smooth_u = 2; o->mg_smooth_u_post = 0; o->mg_cheb_ratio_u = 4.0;
  o->inner_rel_first = 0.0;
  o->inner_first_pshare = 0.0;
  o->mp_solver = 0;
}

void ifem_default_tuning(ifem_tuning *t) {
  t->geo_cache = 1; t->xcd_swizzle = 1; t->asm_skip = 0; t->spmv_lanes = 32; t->sm_lanes = 32; t->mf_f32 = 1;
  t->tpp_operator = 0; t->spmv_pipe = 1; t->halo_overlap = 1; t->asm3_variant = 0; t->cg_single_reduction = 1; t->asm3_cpb = 2; t->tpp_milu_permille = 950; t->tpp_ilu_order = 2; t->basis_pad = 32 * 33; t->tpp_tri_sweeps = 0; t->uu_row_order = 1; t->eig_steps = 0; t->vcycle_graph_cells = 262144;
  t->scns_pc = 2; t->pvv_sweeps = 4; t->b2pp_sweeps = 6; t->scns_inner_reorth = 0; t->scns_inner_left = 1; t->scns_graph = 0; t->stored_uu = 1; t->mf_uniform = 1; t->inner_f32 = 1; t->mg_lattice_u = 1; t->uu_smoother = 0; t->uu_patch_levels = 0; t->asm_rows = 1;
}

int ifem_set_tuning(ifem_ctx *ctx, const ifem_tuning *t) {
  IFEM_API_BEGIN
  if (!t) throw Error(IFEM_E_BADPARAM, "null tuning");
  const int g[2] = {t->spmv_lanes, t->sm_lanes};
  for (int v : g)
    if (v != 8 && v != 16 && v != 32 && v != 64) throw Error(IFEM_E_BADPARAM, "lanes per row must be 8, 16, 32 or 64");
  if (t->basis_pad < 0) throw Error(IFEM_E_BADPARAM, "negative size in ifem_tuning");
  if (t->asm3_cpb > 0 && t->asm3_cpb != 2 && t->asm3_cpb != 4 && t->asm3_cpb != 8) throw Error(IFEM_E_BADPARAM, "asm3_cpb must be 2, 4 or 8 (cells per workgroup of the 3D Q2/Q1 cell kernel)");
  if (t->tpp_ilu_order < -1 || t->tpp_ilu_order > 2) throw Error(IFEM_E_BADPARAM, "tpp_ilu_order must be -1, 0, 1 or 2");
  if (t->scns_pc != 0 && t->scns_pc != 1 && t->scns_pc != 2) throw Error(IFEM_E_BADPARAM, "scns_pc must be 1 (explicit T_pp) or 2 (the reference's structure); 0 = default");
  if (t->uu_smoother != 0 && t->uu_smoother != 1) throw Error(IFEM_E_BADPARAM, "uu_smoother must be 0 (node-block Jacobi) or 1 (vertex patches on uniform box levels)");
  if (t->uu_patch_levels != 0 && t->uu_patch_levels != 1) throw Error(IFEM_E_BADPARAM, "uu_patch_levels must be 0 (uniform box levels only) or 1 (per-patch inverses on all other eligible levels)");
  ctx->tune = *t;
  ++ctx->graph_epoch;
  ++ctx->bb_version; // the lattice tables of B / B^T are re-made and probed by the next solve's set-up (CSR until then)
  if (ctx->tune.asm3_cpb <= 0) ctx->tune.asm3_cpb = 2; // a zero-initialised struct: the defaults of the fields added after round 4
  if (ctx->tune.scns_pc == 0) { ctx->tune.scns_pc = 2; if (!ctx->tune.pvv_sweeps) ctx->tune.pvv_sweeps = 4; if (!ctx->tune.b2pp_sweeps) ctx->tune.b2pp_sweeps = 6; ctx->tune.scns_inner_left = 1; ctx->tune.stored_uu = 1; }
  IFEM_API_END
}

int ifem_ctx_create(const ifem_mesh_desc *m, const ifem_partition *part, int device, ifem_ctx **out) {
  ifem_ctx *ctx = nullptr;
  IFEM_API_BEGIN
  if (!m || !out) throw Error(IFEM_E_BADPARAM, "null argument");
  if ((m->dim != 2 && m->dim != 3) || (m->kv != 1 && m->kv != 2)) throw Error(IFEM_E_BADPARAM, "dim must be 2|3, kv 1|2");
  if (ifem_device_count() <= device) throw Error(IFEM_E_NODEVICE, "no HIP device: libifem_hip has no CPU fallback");
  IFEM_HIP_CHECK(hipSetDevice(device));
  ctx = new ifem_ctx();
  ctx->device = device;
  ifem_default_tuning(&ctx->tune);
  IFEM_HIP_CHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  IFEM_HIP_CHECK(hipEventCreate(&ctx->ev0));
  IFEM_HIP_CHECK(hipEventCreate(&ctx->ev1));
  hipStream_t s = ctx->stream;
  ctx->dim = m->dim; ctx->kv = m->kv;
  build_fe_tables(ctx->fe, m->dim, m->kv);
  ctx->nu = ctx->fe.nu; ctx->np = ctx->fe.np; ctx->nq = ctx->fe.nq;
  ctx->d_fe.upload(&ctx->fe, 1, s);
  ctx->n_cells = m->n_cells;
  ctx->nUo = m->n_unodes_owned; ctx->nUl = m->n_unodes_local;
  ctx->nPo = m->n_pnodes_owned; ctx->nPl = m->n_pnodes_local;
  ctx->n_local = ctx->dim * ctx->nUl + ctx->nPl;
  const int dim = ctx->dim, nu = ctx->nu, np = ctx->np;
  ctx->vcoords.upload(m->vcoords, (size_t)m->n_cells * np * dim, s);
  ctx->cell_unodes.upload(m->cell_unodes, (size_t)m->n_cells * nu, s);
  ctx->cell_pnodes.upload(m->cell_pnodes, (size_t)m->n_cells * np, s);
  if (m->cell_face_bid) ctx->cell_face_bid.upload(m->cell_face_bid, (size_t)m->n_cells * 2 * dim, s);
  else {
    std::vector<int32_t> none((size_t)m->n_cells * 2 * dim, -1);
    ctx->cell_face_bid.upload(none.data(), none.size(), s);
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
  }
  detect_uniform_cells(ctx);
  IFEM_HIP_CHECK(hipHostMalloc((void **)&ctx->h_scal, kScalSlots * sizeof(double)));
  ctx->scal.alloc(kScalSlots);
  comm_init(ctx, part);
  {
    double g[2] = {double(ctx->dim * ctx->nUo), double(ctx->nPo)};
    allreduce_sum(ctx, g, 2);
    ctx->n_global_u = (int64_t)g[0]; ctx->n_global_p = (int64_t)g[1];
  }
  // block sparsity + scatter maps (make_sparsity_pattern / matrix.reinit, mpi_fluid_solver.cpp:311-322)
  build_pattern(ctx, ctx->Auu, dim * dim, ctx->nUo, nu, ctx->cell_unodes.p, nu, ctx->cell_unodes.p, ctx->posUU);
  build_pattern(ctx, ctx->Bt, dim, ctx->nUo, nu, ctx->cell_unodes.p, np, ctx->cell_pnodes.p, ctx->posUP);
  build_pattern(ctx, ctx->B, dim, ctx->nPo, np, ctx->cell_pnodes.p, nu, ctx->cell_unodes.p, ctx->posPU);
  build_pattern(ctx, ctx->Mp, 1, ctx->nPo, np, ctx->cell_pnodes.p, np, ctx->cell_pnodes.p, ctx->posPP);
  ctx->diagMu.alloc((size_t)dim * ctx->nUo);
  ctx->dinvMu.alloc((size_t)dim * ctx->nUo);
  ctx->bjac.alloc((size_t)dim * dim * ctx->nUo);
  for (int v = 0; v < IFEM_N_VECS; ++v) {
    ctx->vec[v].alloc((size_t)ctx->n_local);
    IFEM_HIP_CHECK(hipMemsetAsync(ctx->vec[v].p, 0, ctx->n_local * sizeof(double), s));
  }
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  *out = ctx;
  }
  catch (const ifem::Error &e) { g_err = e.what(); if (ctx) ifem_ctx_destroy(ctx); return e.code; }
  catch (const std::exception &e) { g_err = e.what(); if (ctx) ifem_ctx_destroy(ctx); return IFEM_E_HIP; }
  return IFEM_OK;
}

void ifem_ctx_destroy(ifem_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  // unhook from a multigrid chain.  The level above forgets this one; the levels below ran on this context's stream(s) (or
  // on those of a level further up) and stay usable by themselves: the chain below gets streams of its own.
  if (ctx->mg_fine && ctx->mg_fine->mg_coarse == ctx) {
    ctx->mg_fine->mg_coarse = nullptr;
    ctx->mg_fine->mg_replica = false;
    ctx->mg_fine->sm_mg_version = -1;
    ctx->mg_fine->uu_mg_version = -1;
  }
  if (ifem_ctx *below = ctx->mg_coarse) {
    below->mg_fine = nullptr;
    hipStream_t ns = nullptr, nh = nullptr;
    if (!below->owns_stream && hipStreamCreateWithFlags(&ns, hipStreamNonBlocking) == hipSuccess) {
      for (ifem_ctx *c = below; c; c = c->mg_coarse) { c->stream = ns; c->owns_stream = c == below; }
    }
    if (below->halo.hstream && !below->halo.owns_hstream) {
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
      if (hipStreamCreateWithPriority(&nh, hipStreamNonBlocking, hi) == hipSuccess)
        for (ifem_ctx *c = below; c; c = c->mg_coarse) { c->halo.hstream = nh; c->halo.owns_hstream = c == below; }
    }
  }
  comm_destroy(ctx);
  if (ctx->h_scal) (void)hipHostFree(ctx->h_scal);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  for (hipEvent_t e : ctx->pc_ev) (void)hipEventDestroy(e);
  ctx->vc_graph.destroy();
  ctx->sm_graph.destroy();
  ctx->pa_graph.destroy();
  hipStream_t s = ctx->owns_stream ? ctx->stream : nullptr;
  delete ctx;
  if (s) (void)hipStreamDestroy(s);
}

int64_t ifem_n_local_dofs(const ifem_ctx *ctx) { return ctx->n_local; }
int64_t ifem_uu_stored_bytes(const ifem_ctx *ctx) { return ctx ? int64_t(ctx->Auu.val.n * sizeof(double)) : 0; }
int64_t ifem_nnz(const ifem_ctx *ctx, int block) {
  switch (block) {
  case 0: return ctx->Auu.nnzb;
  case 1: return ctx->B.nnzb;
  case 2: return ctx->Mp.nnzb;
  default: return 0;
  }
}

int ifem_set_constraints(ifem_ctx *ctx, int which, int32_t n, const int32_t *dof, const double *inhom) {
  IFEM_API_BEGIN
  if (which < 0 || which > 1) throw Error(IFEM_E_BADPARAM, "which must be 0 or 1");
  if (n < 0 || (n > 0 && !dof)) throw Error(IFEM_E_BADPARAM, "bad constraint list");
  // A dof listed twice keeps its LAST line, as the sequential host loop did.
  const size_t N = (size_t)ctx->n_local;
  std::vector<int32_t> kd;
  std::vector<double> kv;
  DBuf<uint8_t> nf;
  DBuf<double> nv;
  {
    int bad = build_line_set(ctx, N, n, dof, inhom, kd, kv, nf, nv) ? 0 : 1;
    for (int32_t d : kd) if (d >= ctx->dim * ctx->nUl) { bad = 2; break; } // (seen before the line that left the range: the walk runs from the back)
    // the call is collective on partitioned contexts (constraint_set_identity all-reduces): every rank must fail together,
    // or the ranks with good lists would wait in that all-reduce for the one that threw
    double worst = bad;
    allreduce_max(ctx, &worst, 1);
    if (worst == 1.0) throw Error(IFEM_E_BADPARAM, bad == 1 ? "constraint dof out of range" : "constraint dof out of range on another rank");
    if (worst == 2.0) throw Error(IFEM_E_BADPARAM, "pressure Dirichlet constraints are not supported");
  }
  const DBuf<uint8_t> *pa[2] = {&nf, &nf}, *pb[2] = {&ctx->is_c[which], &ctx->is_c[1 - which]};
  double differs[2];
  flags_differ(ctx, 2, pa, pb, differs);
  ctx->is_c[which].swap(nf);
  ctx->cval[which].swap(nv);
  ctx->has_c[which] = !kd.empty();
  {
    double any = 0; // (collective on partitioned contexts: a rank without inhomogeneous lines must agree with one that has them)
    for (double v : kv) if (v != 0.0) { any = 1; break; }
    allreduce_max(ctx, &any, 1);
    ctx->inhom_any[which] = any != 0.0;
  }
  constraint_set_identity(ctx, which, differs[0] != 0.0, differs[1] != 0.0);
  IFEM_API_END
}

int ifem_fsi_set_solid(ifem_ctx *ctx, const ifem_fsi_solid *solid) {
  IFEM_API_BEGIN
  ifem::fsi_set_solid(ctx, solid);
  IFEM_API_END
}
int ifem_fsi_update_indicator(ifem_ctx *ctx, int32_t *host_out, int64_t *n_artificial) {
  IFEM_API_BEGIN
  ifem::fsi_update_indicator(ctx, host_out, n_artificial);
  IFEM_API_END
}
int ifem_fsi_find_fluid_bc(ifem_ctx *ctx, double dt, int use_dirichlet_bc, const int32_t *cell_order, ifem_fsi_stats *stats) {
  IFEM_API_BEGIN
  if (!(dt > 0)) throw Error(IFEM_E_BADPARAM, "ifem_fsi_find_fluid_bc: dt must be positive");
  ifem::fsi_find_fluid_bc(ctx, dt, use_dirichlet_bc, cell_order, stats);
  IFEM_API_END
}
int ifem_fsi_fluid_at_points(ifem_ctx *ctx, int32_t n, const double *points, double *values, double *stress, int32_t *cell) {
  IFEM_API_BEGIN
  ifem::fsi_fluid_at_points(ctx, n, points, values, stress, cell);
  IFEM_API_END
}
int ifem_fsi_get_stress(ifem_ctx *ctx, double *host_out) {
  IFEM_API_BEGIN
  const size_t n = (size_t)(ctx->dim * (ctx->dim + 1) / 2) * ctx->nUl;
  if (!host_out) throw Error(IFEM_E_BADPARAM, "null output");
  if (ctx->fsi_stress.n != n) throw Error(IFEM_E_BADPARAM, "the context holds no nodal fsi_stress");
  IFEM_HIP_CHECK(hipMemcpyAsync(host_out, ctx->fsi_stress.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}
int ifem_get_constraints(ifem_ctx *ctx, int which, uint8_t *flags, double *inhom) {
  IFEM_API_BEGIN
  if (which < 0 || which > 1) throw Error(IFEM_E_BADPARAM, "which must be 0 or 1");
  const size_t n = (size_t)ctx->n_local;
  if (ctx->is_c[which].n != n) { // never set: no line
    if (flags) std::fill(flags, flags + n, uint8_t(0));
    if (inhom) std::fill(inhom, inhom + n, 0.0);
  } else {
    if (flags) IFEM_HIP_CHECK(hipMemcpyAsync(flags, ctx->is_c[which].p, n, hipMemcpyDeviceToHost, ctx->stream));
    if (inhom) IFEM_HIP_CHECK(hipMemcpyAsync(inhom, ctx->cval[which].p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  IFEM_API_END
}

int ifem_set_hanging_constraints(ifem_ctx *ctx, int32_t n, const int32_t *dof, const int32_t *ptr, const int32_t *master,
                                 const double *weight) {
  IFEM_API_BEGIN
  ifem::hanging_set(ctx, n, dof, ptr, master, weight);
  IFEM_API_END
}

int ifem_kelly_estimate(ifem_ctx *ctx, int vec, const int32_t *face_table, double *eta_host, const double **eta_device) {
  IFEM_API_BEGIN
  if (!ctx) throw Error(IFEM_E_BADPARAM, "ifem_kelly_estimate: null context");
  if (vec < 0 || vec >= IFEM_N_VECS) throw Error(IFEM_E_BADPARAM, "bad vector id");
  IFEM_HIP_CHECK(hipSetDevice(ctx->device));
  ifem::kelly_estimate(ctx, ctx->vec[vec].p, face_table);
  if (eta_host && ctx->n_cells) {
    IFEM_HIP_CHECK(hipMemcpyAsync(eta_host, ctx->kelly.eta.p, size_t(ctx->n_cells) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  if (eta_device) *eta_device = ctx->kelly.eta.p;
  IFEM_API_END
}

int ifem_transfer_solution(ifem_ctx *src, ifem_ctx *dst, int vec, const int32_t *u_cell, const int32_t *u_pos, const int32_t *p_cell,
                           const int32_t *p_pos) {
  IFEM_API_BEGIN
  if (vec < 0 || vec >= IFEM_N_VECS) throw Error(IFEM_E_BADPARAM, "bad vector id");
  if (dst) IFEM_HIP_CHECK(hipSetDevice(dst->device));
  ifem::transfer_solution(src, dst, vec, u_cell, u_pos, p_cell, p_pos);
  IFEM_API_END
}

int ifem_mg_attach(ifem_ctx *fine, ifem_ctx *coarse, const ifem_mg_transfer *t) {
  IFEM_API_BEGIN
  if (!fine || !coarse || !t || fine == coarse) throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: two contexts and a transfer table");
  // a single-rank coarse context below a partitioned fine one: the REPLICATED coarse level (see ifem_hip.h)
  const bool replica = fine->halo.nranks > 1 && coarse->halo.nranks == 1;
  if (fine->dim != coarse->dim || fine->kv != coarse->kv || fine->device != coarse->device ||
      (!replica && (fine->halo.nranks != coarse->halo.nranks || fine->halo.rank != coarse->halo.rank)))
    throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: the levels must share dimension, velocity degree, device, rank and rank count "
                                 "(or the coarse context is a single-rank replica of the whole coarse mesh)");
  if (coarse->mg_fine && coarse->mg_fine != fine)
    throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: the coarse context already hangs below another level");
  for (const ifem_ctx *c = coarse; c; c = c->mg_coarse)
    if (c == fine) throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: the fine context is a level below the coarse one");
  // row pointers non-decreasing and closed: a malformed table would send the transfer kernels out of bounds
  auto monotone = [](const int64_t *ptr, int64_t n_rows, int64_t nnz_, const char *what) {
    if (ptr[0] != 0 || ptr[n_rows] != nnz_) throw Error(IFEM_E_BADPARAM, std::string("ifem_mg_attach: ") + what + " row pointers do not span the table");
    for (int64_t r = 0; r < n_rows; ++r)
      if (ptr[r + 1] < ptr[r]) throw Error(IFEM_E_BADPARAM, std::string("ifem_mg_attach: ") + what + " row pointers decrease");
  };
  if (t->n_fine_p_owned != fine->nPo || t->n_coarse_p_local != coarse->nPl)
    throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: P_p needs one row per owned fine pressure node, R_p one per local coarse pressure node");
  if (!t->pp_ptr || !t->pp_col || !t->pp_w || !t->rp_ptr || !t->rp_col || !t->rp_w) throw Error(IFEM_E_BADPARAM, "null transfer table");
  const int64_t nnz = t->pp_ptr[fine->nPo];
  if (nnz < 0 || t->rp_ptr[coarse->nPl] != nnz) throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: R_p is not the transpose of P_p");
  monotone(t->pp_ptr, fine->nPo, nnz, "P_p");
  monotone(t->rp_ptr, coarse->nPl, nnz, "R_p");
  for (int64_t k = 0; k < nnz; ++k) {
    if (t->pp_col[k] < 0 || t->pp_col[k] >= coarse->nPl) throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: P_p column out of range");
    if (t->rp_col[k] < 0 || t->rp_col[k] >= fine->nPo) throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: R_p column out of range");
  }
  hipStream_t s = fine->stream;
  fine->mg_Pp.n_rows = fine->nPo;
  fine->mg_Pp.ptr.upload(t->pp_ptr, (size_t)fine->nPo + 1, s);
  fine->mg_Pp.col.upload(t->pp_col, (size_t)nnz, s);
  fine->mg_Pp.w.upload(t->pp_w, (size_t)nnz, s);
  fine->mg_Rp.n_rows = coarse->nPl;
  fine->mg_Rp.ptr.upload(t->rp_ptr, (size_t)coarse->nPl + 1, s);
  fine->mg_Rp.col.upload(t->rp_col, (size_t)nnz, s);
  fine->mg_Rp.w.upload(t->rp_w, (size_t)nnz, s);
  fine->mg_Pu.n_rows = fine->mg_Ru.n_rows = 0;
  // the packed transfer entries (columns, weights and drop bits baked in) and the captured cycles belong to the tables that are replaced
  fine->mg_mask_key[0] = fine->mg_mask_key[1] = -1;
  fine->mg_lattice_u = MgLatticeU(); // decided anew for the new tables (mg_lattice.hip::mg_lattice_u_setup)
  ++fine->graph_epoch; ++coarse->graph_epoch;
  fine->vc_graph.destroy(); fine->sm_graph.destroy();
  fine->vc_graph.armed = fine->sm_graph.armed = false; fine->vc_graph.key.clear(); fine->sm_graph.key.clear();
  if (t->pu_ptr) { // velocity-node transfers: optional
    if (!t->pu_col || !t->pu_w || !t->ru_ptr || !t->ru_col || !t->ru_w || !t->inj_u) throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: incomplete velocity transfer tables");
    if (t->n_fine_u_owned != fine->nUo || t->n_coarse_u_local != coarse->nUl)
      throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: P_u needs one row per owned fine velocity node, R_u one per local coarse velocity node");
    const int64_t nu = t->pu_ptr[fine->nUo];
    if (nu < 0 || t->ru_ptr[coarse->nUl] != nu) throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: R_u is not the transpose of P_u");
    monotone(t->pu_ptr, fine->nUo, nu, "P_u");
    monotone(t->ru_ptr, coarse->nUl, nu, "R_u");
    for (int64_t k = 0; k < nu; ++k) {
      if (t->pu_col[k] < 0 || t->pu_col[k] >= coarse->nUl) throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: P_u column out of range");
      if (t->ru_col[k] < 0 || t->ru_col[k] >= fine->nUo) throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: R_u column out of range");
      // the node transfers read their weights as float (mg.hip::mg_csr_mask): a weight that single precision cannot hold would be rounded silently
      if (double(float(t->pu_w[k])) != t->pu_w[k]) throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: a P_u weight (pu_w) is not exact in single precision");
      if (double(float(t->ru_w[k])) != t->ru_w[k]) throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: an R_u weight (ru_w) is not exact in single precision");
    }
    for (int64_t i = 0; i < coarse->nUo; ++i)
      if ((t->inj_u[i] < 0 && !(replica && t->inj_u[i] == -1)) || t->inj_u[i] >= fine->nUo)
        throw Error(IFEM_E_BADPARAM, "ifem_mg_attach: inj_u must name owned fine nodes (-1 below a replicated level: another rank owns the fine node)");
    fine->mg_Pu.n_rows = fine->nUo;
    fine->mg_Pu.ptr.upload(t->pu_ptr, (size_t)fine->nUo + 1, s);
    fine->mg_Pu.col.upload(t->pu_col, (size_t)nu, s);
    fine->mg_Pu.w.upload(t->pu_w, (size_t)nu, s);
    fine->mg_Ru.n_rows = coarse->nUl;
    fine->mg_Ru.ptr.upload(t->ru_ptr, (size_t)coarse->nUl + 1, s);
    fine->mg_Ru.col.upload(t->ru_col, (size_t)nu, s);
    fine->mg_Ru.w.upload(t->ru_w, (size_t)nu, s);
    fine->mg_inj_u.upload(t->inj_u, (size_t)coarse->nUo, s);
  }
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  if (fine->mg_coarse && fine->mg_coarse != coarse) fine->mg_coarse->mg_fine = nullptr; // re-attach: the old level is on its own
  fine->mg_coarse = coarse;
  fine->mg_replica = replica;
  coarse->mg_fine = fine;
  fine->sm_mg_version = -1;
  fine->uu_mg_version = -1;
  // one stream for the whole chain: the V-cycle walks up and down the levels and every launch must stay in order
  for (ifem_ctx *c = coarse; c; c = c->mg_coarse) {
    if (c->stream == s) continue;
    IFEM_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->owns_stream) (void)hipStreamDestroy(c->stream);
    c->stream = s;
    c->owns_stream = false;
    // likewise one halo stream (the levels share the communicators, comm.hip)
    if (fine->halo.hstream && c->halo.hstream && c->halo.hstream != fine->halo.hstream) {
      IFEM_HIP_CHECK(hipStreamSynchronize(c->halo.hstream));
      if (c->halo.owns_hstream) (void)hipStreamDestroy(c->halo.hstream);
      c->halo.hstream = fine->halo.hstream;
      c->halo.owns_hstream = false;
    }
  }
  IFEM_API_END
}

int ifem_mg_depth(const ifem_ctx *ctx) {
  int d = 0;
  for (const ifem_ctx *c = ctx ? ctx->mg_coarse : nullptr; c; c = c->mg_coarse) ++d;
  return d;
}

int ifem_set_cell_fields(ifem_ctx *ctx, const int32_t *indicator) {
  IFEM_API_BEGIN
  if (indicator) {
    ctx->indicator.upload(indicator, (size_t)ctx->n_cells, ctx->stream);
    IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  } else
    ctx->indicator.release();
  IFEM_API_END
}

static inline bool vec_ok(int v) { return v >= 0 && v < IFEM_N_VECS; }
// PRESENT / EVAL / FSI_ACC / INCREMENT are ghosted (extended) vectors, the others hold owned entries only
static inline bool is_ext(int v) { return v == IFEM_VEC_PRESENT || v == IFEM_VEC_EVAL || v == IFEM_VEC_FSI_ACC || v == IFEM_VEC_INCREMENT; }
static inline int64_t vec_len(const ifem_ctx *c, int v) { return is_ext(v) ? c->n_local : c->dim * c->nUo + c->nPo; }
static inline int64_t p_off(const ifem_ctx *c, int v) { return c->dim * (is_ext(v) ? c->nUl : c->nUo); }

int ifem_vec_set(ifem_ctx *ctx, int vec, const double *host) {
  IFEM_API_BEGIN
  if (!vec_ok(vec)) throw Error(IFEM_E_BADPARAM, "bad vector id");
  IFEM_HIP_CHECK(hipMemcpyAsync(ctx->vec[vec].p, host, vec_len(ctx, vec) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}
int ifem_vec_get(ifem_ctx *ctx, int vec, double *host) {
  IFEM_API_BEGIN
  if (!vec_ok(vec)) throw Error(IFEM_E_BADPARAM, "bad vector id");
  IFEM_HIP_CHECK(hipMemcpyAsync(host, ctx->vec[vec].p, vec_len(ctx, vec) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}
int ifem_vec_zero(ifem_ctx *ctx, int vec) {
  IFEM_API_BEGIN
  if (!vec_ok(vec)) throw Error(IFEM_E_BADPARAM, "bad vector id");
  v_zero(ctx, ctx->n_local, ctx->vec[vec].p);
  IFEM_API_END
}
// owned entries of src -> dst (layouts may differ); ghosts of an extended dst are refreshed
static void copy_owned(ifem_ctx *ctx, int dst, int src, double a_src, double b_dst) {
  const int64_t nuo = ctx->dim * ctx->nUo;
  v_axpby(ctx, nuo, a_src, ctx->vec[src].p, b_dst, ctx->vec[dst].p);
  v_axpby(ctx, ctx->nPo, a_src, ctx->vec[src].p + p_off(ctx, src), b_dst, ctx->vec[dst].p + p_off(ctx, dst));
  if (is_ext(dst)) {
    halo_exchange(ctx, ctx->vec[dst].p);
    halo_exchange_p(ctx, ctx->vec[dst].p + p_off(ctx, dst));
  }
}
int ifem_vec_copy(ifem_ctx *ctx, int dst, int src) {
  IFEM_API_BEGIN
  if (!vec_ok(dst) || !vec_ok(src)) throw Error(IFEM_E_BADPARAM, "bad vector id");
  copy_owned(ctx, dst, src, 1.0, 0.0);
  IFEM_API_END
}
int ifem_vec_axpy(ifem_ctx *ctx, double a, int x, int y) {
  IFEM_API_BEGIN
  if (!vec_ok(x) || !vec_ok(y)) throw Error(IFEM_E_BADPARAM, "bad vector id");
  copy_owned(ctx, y, x, a, 1.0);
  IFEM_API_END
}
static double norm2_owned(ifem_ctx *ctx, int vec) {
  const int64_t nuo = ctx->dim * ctx->nUo;
  double d[2];
  d[0] = v_dot(ctx, nuo, ctx->vec[vec].p, ctx->vec[vec].p);
  d[1] = v_dot(ctx, ctx->nPo, ctx->vec[vec].p + p_off(ctx, vec), ctx->vec[vec].p + p_off(ctx, vec));
  double s = d[0] + d[1];
  allreduce_sum(ctx, &s, 1);
  return std::sqrt(s);
}
int ifem_vec_norm2(ifem_ctx *ctx, int vec, double *out) {
  IFEM_API_BEGIN
  if (!vec_ok(vec)) throw Error(IFEM_E_BADPARAM, "bad vector id");
  *out = norm2_owned(ctx, vec);
  IFEM_API_END
}
int ifem_vec_minmax(ifem_ctx *ctx, int vec, int block, double *vmin, double *vmax) {
  IFEM_API_BEGIN
  if (!vec_ok(vec)) throw Error(IFEM_E_BADPARAM, "bad vector id");
  double mn, mx;
  if (block == 0) v_minmax(ctx, ctx->dim * ctx->nUo, ctx->vec[vec].p, &mn, &mx);
  else v_minmax(ctx, ctx->nPo, ctx->vec[vec].p + p_off(ctx, vec), &mn, &mx);
  if (ctx->halo.nranks > 1) { // max = -min(-x): reuse the sum all-reduce on {mn, -mx} is wrong; do two max-reductions
    double t[2] = {-mn, mx};
    allreduce_max(ctx, t, 2);
    mn = -t[0]; mx = t[1];
  }
  if (vmin) *vmin = mn;
  if (vmax) *vmax = mx;
  IFEM_API_END
}
int ifem_halo_exchange(ifem_ctx *ctx, int vec) {
  IFEM_API_BEGIN
  if (!vec_ok(vec) || !is_ext(vec)) throw Error(IFEM_E_BADPARAM, "not a ghosted vector");
  halo_exchange(ctx, ctx->vec[vec].p);
  halo_exchange_p(ctx, ctx->vec[vec].p + p_off(ctx, vec));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

// one assembly through the driver, waited for; timing.assemble_ms is its wall time
static void timed_assemble(ifem_ctx *ctx, const ifem_ins_params *p, int use_nonzero, int imex, AsmMode mode) {
  if (!p || p->dt <= 0) throw Error(IFEM_E_BADPARAM, "bad ifem_ins_params");
  auto t0 = std::chrono::steady_clock::now();
  launch_ins_assemble_ex(ctx, p, use_nonzero, imex, mode);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->timing.assemble_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int ifem_ins_assemble(ifem_ctx *ctx, const ifem_ins_params *p, int use_nonzero) {
  IFEM_API_BEGIN
  timed_assemble(ctx, p, use_nonzero, 0, AsmMode::Full);
  IFEM_API_END
}

int ifem_imex_assemble(ifem_ctx *ctx, const ifem_ins_params *p, int use_nonzero, int assemble_system) {
  IFEM_API_BEGIN
  timed_assemble(ctx, p, use_nonzero, 1, assemble_system ? AsmMode::Full : AsmMode::Rhs);
  IFEM_API_END
}

static void imex_solve_impl(ifem_ctx *ctx, const ifem_ins_params *p, const ifem_solver_opts *o, int use_nonzero, ifem_solve_stats *stats) {
  ifem_solver_opts oo = opts_or_default(o);
  if (!o) oo.inner_rel = 1e-4;
  const double bn = norm2_owned(ctx, IFEM_VEC_RHS);
  oo.fgmres_rel = 0.0;
  oo.fgmres_abs = std::min(1e-9, 1e-8 * bn); // mpi_insimex.cpp:369-370
  ins_solve(ctx, p, &oo, use_nonzero, stats);
}

int ifem_imex_solve(ifem_ctx *ctx, const ifem_ins_params *p, const ifem_solver_opts *o, int use_nonzero, ifem_solve_stats *stats) {
  IFEM_API_BEGIN
  if (!p) throw Error(IFEM_E_BADPARAM, "null params");
  imex_solve_impl(ctx, p, o, use_nonzero, stats);
  IFEM_API_END
}

int ifem_imex_step(ifem_ctx *ctx, const ifem_ins_params *p, const ifem_solver_opts *o, int apply_nonzero, int assemble_system,
                   ifem_solve_stats *stats) {
  IFEM_API_BEGIN
  if (!p || p->dt <= 0) throw Error(IFEM_E_BADPARAM, "bad ifem_ins_params");
  v_zero(ctx, ctx->n_local, ctx->vec[IFEM_VEC_UPDATE].p); // solution_time_increment = 0
  launch_ins_assemble_ex(ctx, p, apply_nonzero, 1, assemble_system ? AsmMode::Full : AsmMode::Rhs);
  imex_solve_impl(ctx, p, o, apply_nonzero, stats);
  copy_owned(ctx, IFEM_VEC_PRESENT, IFEM_VEC_UPDATE, 1.0, 1.0); // present_solution += solution_time_increment
  launch_update_stress(ctx, p->viscosity);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_solve(ifem_ctx *ctx, const ifem_ins_params *p, const ifem_solver_opts *o, int use_nonzero, ifem_solve_stats *stats) {
  IFEM_API_BEGIN
  const ifem_solver_opts oo = opts_or_default(o);
  ins_solve(ctx, p, &oo, use_nonzero, stats);
  IFEM_API_END
}

int ifem_rhs_norm(ifem_ctx *ctx, double *l2) { return ifem_vec_norm2(ctx, IFEM_VEC_RHS, l2); }

// solution_increment = present - evaluation; present = evaluation (:465-473)
static void fluid_newton_accept(ifem_ctx *ctx) {
  copy_owned(ctx, IFEM_VEC_INCREMENT, IFEM_VEC_PRESENT, 1.0, 0.0);
  copy_owned(ctx, IFEM_VEC_INCREMENT, IFEM_VEC_EVAL, -1.0, 1.0);
  copy_owned(ctx, IFEM_VEC_PRESENT, IFEM_VEC_EVAL, 1.0, 0.0);
}

int ifem_ins_newton_step(ifem_ctx *ctx, const ifem_ins_params *p, const ifem_solver_opts *o, int apply_nonzero,
                         double tolerance, int max_iterations, double *log) {
  return api_count([&] {
    const ifem_solver_opts oo = opts_or_default(o);
    copy_owned(ctx, IFEM_VEC_EVAL, IFEM_VEC_PRESENT, 1.0, 0.0); // evaluation_point = present_solution (:420)
    const int outer = newton_loop(1e-11, apply_nonzero, tolerance, max_iterations, log, [&](int nz) {
      ifem_solve_stats st{};
      v_zero(ctx, ctx->n_local, ctx->vec[IFEM_VEC_UPDATE].p); // newton_update = 0 (:427)
      launch_ins_assemble_ex(ctx, p, nz, 0, AsmMode::Full);
      ins_solve(ctx, p, &oo, nz, &st);
      const double cur = norm2_owned(ctx, IFEM_VEC_RHS);         // system_rhs.l2_norm() (:438)
      copy_owned(ctx, IFEM_VEC_EVAL, IFEM_VEC_UPDATE, 1.0, 1.0); // evaluation_point += newton_update (:444-448)
      return NewtonIter{cur, double(st.fgmres_iters), st.fgmres_res};
    });
    fluid_newton_accept(ctx);
    IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return outer;
  });
}

int ifem_set_scns_fields(ifem_ctx *ctx, const double *sigma_pml, const double *body_force, const double *fsi_stress) {
  IFEM_API_BEGIN
  hipStream_t s = ctx->stream;
  const size_t ncq = (size_t)ctx->n_cells * ctx->nq;
  if (sigma_pml || ctx->sigma_pml.n) ctx->ex.fields_version++; // the PML field is given or released: the matrices of the explicit solver hold it
  if (sigma_pml) ctx->sigma_pml.upload(sigma_pml, ncq, s); else ctx->sigma_pml.release();
  if (body_force) ctx->body_force.upload(body_force, ncq * ctx->dim, s); else ctx->body_force.release();
  if (fsi_stress) ctx->fsi_stress.upload(fsi_stress, (size_t)(ctx->dim * (ctx->dim + 1) / 2) * ctx->nUl, s); else ctx->fsi_stress.release();
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  IFEM_API_END
}

int ifem_set_eddy_viscosity(ifem_ctx *ctx, const double *nodal) {
  IFEM_API_BEGIN
  if (nodal) ctx->eddy_viscosity.upload(nodal, (size_t)ctx->nUl, ctx->stream); else ctx->eddy_viscosity.release();
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_update_stress(ifem_ctx *ctx, double viscosity, double *host_out) {
  IFEM_API_BEGIN
  launch_update_stress(ctx, viscosity);
  if (host_out) {
    IFEM_HIP_CHECK(hipMemcpyAsync(host_out, ctx->stress.p, ctx->stress.n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  IFEM_API_END
}

int ifem_scns_assemble(ifem_ctx *ctx, const ifem_scns_params *p, int use_nonzero) {
  IFEM_API_BEGIN
  if (!p || p->dt <= 0 || p->viscosity <= 0) throw Error(IFEM_E_BADPARAM, "bad ifem_scns_params");
  launch_scns_assemble(ctx, p, use_nonzero);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_scns_solve(ifem_ctx *ctx, const ifem_solver_opts *o, int use_nonzero, ifem_solve_stats *stats) {
  IFEM_API_BEGIN
  const ifem_solver_opts oo = opts_or_default(o);
  scns_solve(ctx, &oo, use_nonzero, stats);
  IFEM_API_END
}

int ifem_scns_newton_step(ifem_ctx *ctx, const ifem_scns_params *p, const ifem_solver_opts *o, int apply_nonzero,
                          double tolerance, int max_iterations, double *log) {
  return api_count([&] {
    const ifem_solver_opts oo = opts_or_default(o);
    copy_owned(ctx, IFEM_VEC_EVAL, IFEM_VEC_PRESENT, 1.0, 0.0);
    const int outer = newton_loop(1e-14, apply_nonzero, tolerance, max_iterations, log, [&](int nz) { // mpi_supg_solver.cpp:354-355
      ifem_solve_stats st{};
      v_zero(ctx, ctx->n_local, ctx->vec[IFEM_VEC_UPDATE].p);
      launch_scns_assemble(ctx, p, nz);
      scns_solve(ctx, &oo, nz, &st);
      const double cur = norm2_owned(ctx, IFEM_VEC_RHS);
      copy_owned(ctx, IFEM_VEC_EVAL, IFEM_VEC_UPDATE, 1.0, 1.0);
      return NewtonIter{cur, double(st.fgmres_iters), double(st.inner_iters)};
    });
    fluid_newton_accept(ctx);
    launch_update_stress(ctx, p->viscosity); // update_stress() (:396), feeds the next assemble
    IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return outer;
  });
}

// ---- the models on scalar node matrices (sa.hip, scnsex.hip).  A context only exists where a device does: without one the caller has none to
// pass.  prefix: "ifem_sa_*" or "ifem_scnsex_*"
static void need_ctx(const ifem_ctx *ctx, const char *prefix) {
  if (ctx) return;
  if (ifem_device_count() <= 0) throw Error(IFEM_E_NODEVICE, "no HIP device: libifem_hip has no CPU fallback");
  throw Error(IFEM_E_BADPARAM, std::string(prefix) + ": no context");
}
// owned rows of a scalar matrix on the A_uu node pattern: the row pointers alone while col or val is missing, else all three
static void export_node_csr(ifem_ctx *ctx, const DBuf<double> &values, bool ready, const char *not_ready_msg, int64_t *rowptr, int32_t *col, double *val) {
  hipStream_t s = ctx->stream;
  const auto rp = ctx->Auu.rowptr.download(s);
  for (int64_t i = 0; i <= ctx->nUo; ++i) rowptr[i] = rp[i] - rp[0];
  if (!col || !val) return;
  if (!ready) throw Error(IFEM_E_BADPARAM, not_ready_msg);
  const auto c = ctx->Auu.col.download(s);
  const auto v = values.download(s);
  for (int64_t k = 0; k < rowptr[ctx->nUo]; ++k) { col[k] = c[rp[0] + k]; val[k] = v[rp[0] + k]; }
}

// ---- Fluid::MPI::SpalartAllmaras (sa.hip)
static inline bool sa_vec_ok(int v) { return v >= 0 && v < IFEM_SA_N_VECS; }

int ifem_sa_set_wall_points(ifem_ctx *ctx, int64_t n, const double *pts) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_set_wall_points(ctx, n, pts);
  IFEM_API_END
}

int ifem_sa_get_wall_distance(ifem_ctx *ctx, double *host_out) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_check(ctx);
  if (!host_out) throw Error(IFEM_E_BADPARAM, "ifem_sa_get_wall_distance: no output array");
  sa_ensure(ctx);
  IFEM_HIP_CHECK(hipMemcpyAsync(host_out, ctx->sa.wall_d.p, ctx->sa.wall_d.n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_sa_set_constraints(ifem_ctx *ctx, int which, int32_t n, const int32_t *node, const double *inhom) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_set_constraints(ctx, which, n, node, inhom);
  IFEM_API_END
}

int ifem_sa_vec_set(ifem_ctx *ctx, int vec, const double *host) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_check(ctx);
  if (!sa_vec_ok(vec) || !host) throw Error(IFEM_E_BADPARAM, "ifem_sa_vec_set: bad vector id or no data");
  sa_ensure(ctx);
  IFEM_HIP_CHECK(hipMemcpyAsync(ctx->sa.vec[vec].p, host, ctx->sa.vec[vec].n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_sa_vec_get(ifem_ctx *ctx, int vec, double *host) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_check(ctx);
  if (!sa_vec_ok(vec) || !host) throw Error(IFEM_E_BADPARAM, "ifem_sa_vec_get: bad vector id or no output array");
  sa_ensure(ctx);
  IFEM_HIP_CHECK(hipMemcpyAsync(host, ctx->sa.vec[vec].p, ctx->sa.vec[vec].n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_sa_assemble(ifem_ctx *ctx, const ifem_sa_params *p, int use_nonzero) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_assemble(ctx, p, use_nonzero);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_sa_solve(ifem_ctx *ctx, int use_nonzero, uint32_t *iters, double *res) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_solve(ctx, use_nonzero, iters, res);
  IFEM_API_END
}

int ifem_sa_newton_step(ifem_ctx *ctx, const ifem_sa_params *p, int apply_nonzero, double tolerance, int max_iterations, double *log) {
  return api_count([&] {
    need_ctx(ctx, "ifem_sa_*");
    return sa_newton_step(ctx, p, apply_nonzero, tolerance, max_iterations, log);
  });
}

int ifem_sa_update_eddy_viscosity(ifem_ctx *ctx, const ifem_sa_params *p, double *host_out) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_update_eddy_viscosity(ctx, p, host_out);
  IFEM_API_END
}

int ifem_sa_export_csr(ifem_ctx *ctx, int64_t *rowptr, int32_t *col, double *val) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_check(ctx);
  if (!rowptr) throw Error(IFEM_E_BADPARAM, "ifem_sa_export_csr: no rowptr array");
  export_node_csr(ctx, ctx->sa.val, ctx->sa.assembled, "ifem_sa_export_csr called before ifem_sa_assemble", rowptr, col, val);
  IFEM_API_END
}

// ---- the wall function at a moving FSI wall (sa_wall.hip)
int ifem_sa_set_moving_wall(ifem_ctx *ctx, const ifem_sa_wall *wall) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_set_moving_wall(ctx, wall);
  IFEM_API_END
}

int ifem_sa_update_shear_velocity(ifem_ctx *ctx, const ifem_sa_params *p, double *host_out) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_update_shear_velocity(ctx, p, host_out);
  IFEM_API_END
}

int ifem_sa_get_shear_velocity(const ifem_sa_params *p, double image_distance, double vel, double init_guess, double *out) {
  IFEM_API_BEGIN
  if (!p || !out || !(p->viscosity > 0) || !(p->rho > 0)) throw Error(IFEM_E_BADPARAM, "ifem_sa_get_shear_velocity: bad ifem_sa_params or no output");
  *out = sa_shear_velocity(p->viscosity / p->rho, image_distance, vel, init_guess);
  IFEM_API_END
}

int ifem_sa_update_moving_wall_distance(ifem_ctx *ctx, const ifem_sa_params *p, double *host_d, double *host_yplus) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_update_moving_wall_distance(ctx, p, host_d, host_yplus);
  IFEM_API_END
}

int ifem_sa_get_moving_wall(ifem_ctx *ctx, double *host_d, double *host_yplus) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_get_moving_wall(ctx, host_d, host_yplus);
  IFEM_API_END
}

int ifem_sa_update_boundary_condition(ifem_ctx *ctx, const ifem_sa_params *p, int first_step, const int32_t *cell_order, int64_t *n_lines) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_update_boundary_condition(ctx, p, first_step, cell_order, n_lines);
  IFEM_API_END
}

int ifem_sa_get_constraints(ifem_ctx *ctx, int which, uint8_t *flags, double *inhom) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_get_constraints(ctx, which, flags, inhom);
  IFEM_API_END
}

int ifem_sa_set_shear_velocities(ifem_ctx *ctx, const double *utau) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_sa_*");
  sa_set_shear_velocities(ctx, utau);
  IFEM_API_END
}

// ---- Fluid::MPI::SCnsEX (scnsex.hip)
int ifem_scnsex_setup(ifem_ctx *ctx, const ifem_scns_params *p) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_scnsex_*");
  scnsex_setup(ctx, p);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_scnsex_assemble_rhs(ifem_ctx *ctx, const ifem_scns_params *p, int velocity) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_scnsex_*");
  scnsex_assemble_rhs(ctx, p, velocity);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_scnsex_solve(ifem_ctx *ctx, int velocity, uint32_t *iters, double *res) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_scnsex_*");
  scnsex_solve(ctx, velocity, iters, res);
  IFEM_API_END
}

int ifem_scnsex_step(ifem_ctx *ctx, const ifem_scns_params *p, double tolerance, int max_iterations, ifem_scnsex_stats *stats) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_scnsex_*");
  if (stats) *stats = ifem_scnsex_stats{};
  scnsex_step(ctx, p, tolerance, max_iterations, stats);
  IFEM_API_END
}

int ifem_scnsex_export_csr(ifem_ctx *ctx, int which, int64_t *rowptr, int32_t *col, double *val) {
  IFEM_API_BEGIN
  need_ctx(ctx, "ifem_scnsex_*");
  scnsex_check(ctx);
  if (which < 0 || which > 1 || !rowptr) throw Error(IFEM_E_BADPARAM, "ifem_scnsex_export_csr: which must be 0 or 1, rowptr an array");
  export_node_csr(ctx, which == 0 ? ctx->ex.av : ctx->ex.ap, ctx->ex.ready, "ifem_scnsex_export_csr called before ifem_scnsex_setup", rowptr, col, val);
  IFEM_API_END
}

int ifem_system_vmult(ifem_ctx *ctx, int dst, int src) {
  IFEM_API_BEGIN
  if (!vec_ok(dst) || !vec_ok(src) || is_ext(dst) || is_ext(src)) throw Error(IFEM_E_BADPARAM, "use non-ghosted vectors");
  ins_system_vmult(ctx, ctx->vec[src].p, ctx->vec[dst].p);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_true_residual(ifem_ctx *ctx, double *residual_l2, double *rhs_l2) {
  IFEM_API_BEGIN
  if (!ctx->assembled || !residual_l2) throw Error(IFEM_E_BADPARAM, "ifem_true_residual after an assembly and a solve");
  const int64_t n = int64_t(ctx->dim) * ctx->nUo + ctx->nPo;
  DBuf<double> r;
  r.alloc((size_t)n + 8);
  ins_system_vmult(ctx, ctx->vec[IFEM_VEC_UPDATE].p, r.p);
  v_axpby(ctx, n, 1.0, ctx->vec[IFEM_VEC_RHS].p, -1.0, r.p); // r = b - A x
  apply_constraints(ctx, 0, r.p); // zero_constraints: the constrained rows are set to 0 and drop out of the norm
  *residual_l2 = std::sqrt(bv_dot(ctx, r.p, r.p));
  if (rhs_l2) *rhs_l2 = std::sqrt(bv_dot(ctx, ctx->vec[IFEM_VEC_RHS].p, ctx->vec[IFEM_VEC_RHS].p));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_mass_vmult(ifem_ctx *ctx, int dst, int src) {
  IFEM_API_BEGIN
  if (!vec_ok(dst) || !vec_ok(src) || is_ext(dst) || is_ext(src) || dst == src) throw Error(IFEM_E_BADPARAM, "use two non-ghosted vectors");
  if (!ctx->assembled) throw Error(IFEM_E_BADPARAM, "ifem_mass_vmult called before an assembly");
  const int64_t nuo = int64_t(ctx->dim) * ctx->nUo;
  vec_mul(ctx, nuo, ctx->diagMu.p, ctx->vec[src].p, ctx->vec[dst].p);
  if ((int64_t)ctx->work.n < ctx->nPl) ctx->work.alloc(ctx->nPl);
  double *xe = ctx->work.p; // ghost-extended copy of the pressure part
  v_copy(ctx, ctx->nPo, ctx->vec[src].p + nuo, xe);
  if (ctx->halo.nranks > 1) halo_exchange_p(ctx, xe);
  spmv_mp(ctx, xe, ctx->vec[dst].p + nuo);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_uu_block_diag(ifem_ctx *ctx, int which, double *host_out) {
  IFEM_API_BEGIN
  if (!ctx->assembled || !host_out) throw Error(IFEM_E_BADPARAM, "ifem_uu_block_diag after an assembly, with an output buffer");
  const size_t n = (size_t)ctx->nUo * ctx->dim * ctx->dim;
  if (which == 1) {
    std::vector<double> keep(n);
    IFEM_HIP_CHECK(hipMemcpyAsync(keep.data(), ctx->bjac.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    uu_block_diag_mf(ctx);
    IFEM_HIP_CHECK(hipMemcpyAsync(host_out, ctx->bjac.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    IFEM_HIP_CHECK(hipMemcpyAsync(ctx->bjac.p, keep.data(), n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    bjac_written(ctx);
  } else {
    IFEM_HIP_CHECK(hipMemcpyAsync(host_out, ctx->bjac.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  IFEM_API_END
}

int ifem_uu_vmult(ifem_ctx *ctx, int dst, int src, int variant) {
  IFEM_API_BEGIN
  if (!vec_ok(dst) || !vec_ok(src) || is_ext(dst) || is_ext(src) || dst == src) throw Error(IFEM_E_BADPARAM, "use two non-ghosted vectors");
  if (!ctx->assembled) throw Error(IFEM_E_BADPARAM, "ifem_uu_vmult called before ifem_ins_assemble");
  const int64_t nul = int64_t(ctx->dim) * ctx->nUl, nuo = int64_t(ctx->dim) * ctx->nUo;
  if ((int64_t)ctx->work.n < nul) ctx->work.alloc(nul);
  double *xe = ctx->work.p; // ghost-extended copy of the velocity part
  v_copy(ctx, nuo, ctx->vec[src].p, xe);
  if (ctx->halo.nranks > 1) halo_exchange(ctx, xe);
  if (variant == IFEM_AINV_GMRES_BJACOBI_MF) apply_uu_mf(ctx, xe, ctx->vec[dst].p);
  else if (variant == IFEM_AINV_MG) apply_uu_mf(ctx, xe, ctx->vec[dst].p, /*single=*/true); // the inner solve's single-precision operator
  else if (variant == IFEM_AINV_GMRES_BJACOBI || variant == IFEM_AINV_GMRES_BJACOBI_F32)
    spmv_uu(ctx, xe, nullptr, ctx->vec[dst].p, variant == IFEM_AINV_GMRES_BJACOBI_F32);
  else throw Error(IFEM_E_BADPARAM, "variant: IFEM_AINV_GMRES_BJACOBI, _F32, _MF or IFEM_AINV_MG (single-precision matrix-free)");
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_test_uu_vmult_f32col(ifem_ctx *ctx, int dst, int src) {
  IFEM_API_BEGIN
  if (!vec_ok(dst) || !vec_ok(src) || is_ext(dst) || is_ext(src) || dst == src) throw Error(IFEM_E_BADPARAM, "use two non-ghosted vectors");
  if (!ctx->assembled) throw Error(IFEM_E_BADPARAM, "ifem_test_uu_vmult_f32col called before ifem_ins_assemble");
  const int64_t nuo = int64_t(ctx->dim) * ctx->nUo, nv = int64_t(ctx->dim) * ctx->nUl + 8;
  auto &col = ctx->mguf_vec[4]; // (a level vector of the V-cycle, idle outside of it)
  if ((int64_t)col.n < nv) { col.alloc((size_t)nv); IFEM_HIP_CHECK(hipMemsetAsync(col.p, 0, col.n * sizeof(float), ctx->stream)); }
  v_cvt_d2f(ctx, nuo, ctx->vec[src].p, col.p);
  uu_apply_f32col(ctx, col.p, ctx->vec[dst].p);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_test_uu_patch_vmult(ifem_ctx *ctx, int dst, int src) {
  IFEM_API_BEGIN
  if (!vec_ok(dst) || !vec_ok(src) || is_ext(dst) || is_ext(src) || dst == src) throw Error(IFEM_E_BADPARAM, "use two non-ghosted vectors");
  if (!ctx->assembled || !ctx->mf_valid) throw Error(IFEM_E_BADPARAM, "ifem_test_uu_patch_vmult called before ifem_ins_assemble");
  if (!patch_setup(ctx)) throw Error(IFEM_E_BADPARAM, "ifem_test_uu_patch_vmult: this level cannot take the vertex-patch smoother (ifem_test_uu_patch_info)");
  const int64_t nuo = int64_t(ctx->dim) * ctx->nUo, nv = int64_t(ctx->dim) * ctx->nUl + 8;
  for (int k = 3; k <= 4; ++k) { // (level vectors of the V-cycle, idle outside of it)
    auto &v = ctx->mguf_vec[k];
    if ((int64_t)v.n < nv) { v.alloc((size_t)nv); IFEM_HIP_CHECK(hipMemsetAsync(v.p, 0, v.n * sizeof(float), ctx->stream)); }
  }
  v_cvt_d2f(ctx, nuo, ctx->vec[src].p, ctx->mguf_vec[3].p);
  patch_apply(ctx, 0.0, 1.0, ctx->mguf_vec[3].p, ctx->mguf_vec[4].p);
  v_cvt_f2d(ctx, nuo, ctx->mguf_vec[4].p, ctx->vec[dst].p);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_test_uu_patch_info(ifem_ctx *ctx, int64_t out[4]) {
  IFEM_API_BEGIN
  if (!out) throw Error(IFEM_E_BADPARAM, "ifem_test_uu_patch_info: null output");
  const bool ok = ctx->mf_valid ? patch_setup(ctx) : patch_eligible(ctx);
  const bool tables = ok && ctx->patch.valid;
  out[0] = ok ? 1 : 0;
  out[1] = tables ? ctx->patch.n_patches : 0;
  out[2] = tables ? (ctx->patch.form == 1 ? ctx->patch.n_patches : ctx->patch.n_types) : 0; // stored inverses
  out[3] = tables ? ctx->patch.inv_bytes : 0;
  IFEM_API_END
}

extern "C++" {
// one product on host vectors with device vectors of type V (see ifem_test_uu_fused_product)
template <typename V>
static void fused_product_on(ifem_ctx *ctx, int prec, int mode, int first, double a, double b, const double *x, double *xs, double *r, double *d) {
  const size_t n = size_t(ctx->dim) * ctx->nUo, nv = size_t(ctx->dim) * ctx->nUl + 8;
  hipStream_t s = ctx->stream;
  ifem::DBuf<V> dx, dxs, dr, dd;
  ifem::DBuf<double> dy;
  std::vector<V> h(nv, V(0));
  auto up = [&](ifem::DBuf<V> &buf, const double *src, size_t len) {
    buf.alloc(len);
    for (size_t i = 0; i < n; ++i) h[i] = V(src[i]);
    IFEM_HIP_CHECK(hipMemcpyAsync(buf.p, h.data(), len * sizeof(V), hipMemcpyHostToDevice, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
  };
  auto down = [&](const V *src, double *dst) {
    IFEM_HIP_CHECK(hipMemcpyAsync(h.data(), src, n * sizeof(V), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i) dst[i] = double(h[i]);
  };
  up(dx, x, nv);
  if (mode == 0) {
    dy.alloc(n);
    if constexpr (std::is_same<V, float>::value) ifem::apply_uu_mf_f32in(ctx, dx.p, dy.p);
    else ifem::apply_uu_mf(ctx, dx.p, dy.p, prec == 2);
    IFEM_HIP_CHECK(hipMemcpyAsync(d, dy.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
    return;
  }
  up(dxs, xs, n);
  up(dr, r, n);
  if (mode == 3) { dd.alloc(n); IFEM_HIP_CHECK(hipMemsetAsync(dd.p, 0, n * sizeof(V), s)); }
  ifem::MfFuseT<V> f;
  f.mode = mode; f.a = a; f.b = b; f.first = first;
  f.xs = dxs.p; f.r = dr.p; f.d = mode == 2 ? dx.p : dd.p; // mode 2 updates the direction in place, as the smoother does
  if constexpr (std::is_same<V, float>::value) ifem::apply_uu_mf_f32v(ctx, dx.p, &f);
  else ifem::apply_uu_mf(ctx, dx.p, nullptr, prec == 2, &f);
  down(dxs.p, xs);
  down(dr.p, r);
  if (mode >= 2) down(f.d, d);
}
} // extern "C++"

int ifem_test_uu_fused_product(ifem_ctx *ctx, int prec, int mode, int first, double a, double b, const double *x, double *xs, double *r, double *d,
                               int block_cap, int64_t geo[2]) {
  IFEM_API_BEGIN
  if (!ctx->assembled || !ctx->mf_valid) throw Error(IFEM_E_BADPARAM, "ifem_test_uu_fused_product called before ifem_ins_assemble");
  if (ctx->halo.nranks > 1) throw Error(IFEM_E_BADPARAM, "ifem_test_uu_fused_product: single-rank contexts");
  if (prec < 0 || prec > 2 || mode < 0 || mode > 3 || block_cap < 0 || !x || (mode != 1 && !d) || (mode && (!xs || !r)))
    throw Error(IFEM_E_BADPARAM, "ifem_test_uu_fused_product: prec 0..2, mode 0..3, block_cap >= 0, and the vectors the mode uses");
  ctx->mf_gather_block_cap = unsigned(block_cap);
  try {
    if (prec == 1) fused_product_on<float>(ctx, prec, mode, first ? 1 : 0, a, b, x, xs, r, d);
    else fused_product_on<double>(ctx, prec, mode, first ? 1 : 0, a, b, x, xs, r, d);
  } catch (...) { ctx->mf_gather_block_cap = 0; throw; }
  ctx->mf_gather_block_cap = 0;
  if (geo) { geo[0] = ctx->mf_gather_geo[0]; geo[1] = ctx->mf_gather_geo[1]; }
  IFEM_API_END
}

int ifem_test_vec_kernel(ifem_ctx *ctx, int op, int64_t n, int k, int64_t ld, void *V, const double *coef, double *w, double *out) {
  IFEM_API_BEGIN
  if (op < 0 || op >= IFEM_TVK_COUNT || n < 0 || k < 0 || ld < n) throw Error(IFEM_E_BADPARAM, "ifem_test_vec_kernel: op, n >= 0, k >= 0, ld >= n");
  if (ctx->halo.nranks > 1) throw Error(IFEM_E_BADPARAM, "ifem_test_vec_kernel: single-rank contexts");
  const bool f32 = op == IFEM_TVK_MDOT_F32 || op == IFEM_TVK_MAXPY_F32 || op == IFEM_TVK_MAXPY_F32_NORM || op == IFEM_TVK_SCALE_STORE_F32;
  const bool multi = op == IFEM_TVK_MDOT || op == IFEM_TVK_MAXPY || op == IFEM_TVK_MAXPY_NORM;
  const bool multi32 = op == IFEM_TVK_MDOT_F32 || op == IFEM_TVK_MAXPY_F32 || op == IFEM_TVK_MAXPY_F32_NORM;
  const bool v_out = op == IFEM_TVK_SCALE_STORE_F32 || op == IFEM_TVK_SCALE_TO2; // V is written, not read
  const bool w_out = op == IFEM_TVK_MAXPY || op == IFEM_TVK_MAXPY_NORM || op == IFEM_TVK_MAXPY_F32 || op == IFEM_TVK_MAXPY_F32_NORM ||
                     op == IFEM_TVK_AXPY || op == IFEM_TVK_AXPBY || op == IFEM_TVK_DIV;
  const int64_t ncols = multi ? k : multi32 ? ((k + 3) & ~3) : op == IFEM_TVK_SCALE_TO2 ? 2 : (op == IFEM_TVK_MDOT_SELF || op == IFEM_TVK_MINMAX) ? 0 : 1;
  const bool maxpy = op == IFEM_TVK_MAXPY || op == IFEM_TVK_MAXPY_NORM || op == IFEM_TVK_MAXPY_F32 || op == IFEM_TVK_MAXPY_F32_NORM;
  const bool scalars = op == IFEM_TVK_MDOT || op == IFEM_TVK_MDOT_SELF || op == IFEM_TVK_MDOT_F32 || op == IFEM_TVK_MAXPY_NORM ||
                       op == IFEM_TVK_MAXPY_F32_NORM || op == IFEM_TVK_MINMAX;
  const size_t nV = size_t(ld) * size_t(ncols);
  if ((op == IFEM_TVK_MDOT || op == IFEM_TVK_MDOT_F32) && k < 1) throw Error(IFEM_E_BADPARAM, "ifem_test_vec_kernel: a multi-dot of at least one column");
  if ((n > 0 && !w) || (nV && !V) || (scalars && !out) || (maxpy && k > 0 && !coef) ||
      ((op == IFEM_TVK_SCALE_STORE_F32 || op == IFEM_TVK_AXPY || op == IFEM_TVK_AXPBY || op == IFEM_TVK_SCALE_TO2) && !coef))
    throw Error(IFEM_E_BADPARAM, "ifem_test_vec_kernel: a null array this op uses");
  hipStream_t s = ctx->stream;
  DBuf<double> dV, dw, dy;
  DBuf<float> dVf;
  if (f32) dVf.alloc(nV); else dV.alloc(nV);
  dw.alloc((size_t)n);
  if (nV && !v_out) IFEM_HIP_CHECK(hipMemcpyAsync(f32 ? (void *)dVf.p : (void *)dV.p, V, nV * (f32 ? sizeof(float) : sizeof(double)), hipMemcpyHostToDevice, s));
  if (nV && v_out) IFEM_HIP_CHECK(hipMemsetAsync(f32 ? (void *)dVf.p : (void *)dV.p, 0xff, nV * (f32 ? sizeof(float) : sizeof(double)), s)); // NaN: an entry left out shows
  if (n) IFEM_HIP_CHECK(hipMemcpyAsync(dw.p, w, size_t(n) * sizeof(double), hipMemcpyHostToDevice, s));
  const bool all_ranks = true; // as the Krylov solvers pass it: the identity on one rank
  switch (op) {
  case IFEM_TVK_MDOT: v_mdot(ctx, n, k, dV.p, ld, dw.p, out, all_ranks); break;
  case IFEM_TVK_MDOT_SELF: v_mdot(ctx, n, 1, dw.p, n, dw.p, out, all_ranks); break;
  case IFEM_TVK_MAXPY: v_maxpy(ctx, n, k, dV.p, ld, coef, dw.p, nullptr, all_ranks); break;
  case IFEM_TVK_MAXPY_NORM: v_maxpy(ctx, n, k, dV.p, ld, coef, dw.p, out, all_ranks); break;
  case IFEM_TVK_MDOT_F32: v_mdot_f32(ctx, n, k, dVf.p, ld, dw.p, out); break;
  case IFEM_TVK_MAXPY_F32: v_maxpy_f32(ctx, n, k, dVf.p, ld, coef, dw.p, nullptr); break;
  case IFEM_TVK_MAXPY_F32_NORM: v_maxpy_f32(ctx, n, k, dVf.p, ld, coef, dw.p, out); break;
  case IFEM_TVK_SCALE_STORE_F32: v_scale_store_f32(ctx, n, coef[0], dw.p, dVf.p); break;
  case IFEM_TVK_AXPY: v_axpy(ctx, n, coef[0], dV.p, dw.p); break;
  case IFEM_TVK_AXPBY: v_axpby(ctx, n, coef[0], dV.p, coef[1], dw.p); break;
  case IFEM_TVK_SCALE_TO2: v_scale_to2(ctx, n, coef[0], dw.p, dV.p, dV.p + ld); break;
  case IFEM_TVK_DIV:
    dy.alloc((size_t)n);
    vec_div(ctx, n, dV.p, dw.p, dy.p);
    dw.swap(dy);
    break;
  default: v_minmax(ctx, n, dw.p, &out[0], &out[1]); break;
  }
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  if (n && w_out) IFEM_HIP_CHECK(hipMemcpyAsync(w, dw.p, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, s));
  if (nV && v_out) IFEM_HIP_CHECK(hipMemcpyAsync(V, f32 ? (void *)dVf.p : (void *)dV.p, nV * (f32 ? sizeof(float) : sizeof(double)), hipMemcpyDeviceToHost, s));
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  IFEM_API_END
}

int ifem_test_cg_device(ifem_ctx *ctx, int64_t n, const double *a, const double *jac, const double *b, int iters, double *x) {
  IFEM_API_BEGIN
  if (n <= 0 || iters < 0 || !a || !b || !x) throw Error(IFEM_E_BADPARAM, "ifem_test_cg_device: n > 0, iters >= 0, a, b and x");
  if (ctx->halo.nranks > 1) throw Error(IFEM_E_BADPARAM, "ifem_test_cg_device: single-rank contexts");
  test_cg_device(ctx, n, a, jac, b, iters, x);
  IFEM_API_END
}

// ---- test aids of the multigrid kernels (mg.hip).  Every device array an op writes has IFEM_TMG_PAD entries behind what the op may write and starts
// as 0xff bytes (NaN): the host gets the whole array back, so an entry left out and a write past the end both show.
extern "C++" {
namespace {
template <typename T>
struct GuardedOut { // device output of n + IFEM_TMG_PAD entries of T, exchanged with a host array of as many doubles
  DBuf<T> d;
  size_t n = 0;
  // NaN everywhere; in_out: the first n entries are the host's (rounded to T)
  void open(const double *host, size_t n_, bool in_out, hipStream_t s) {
    n = n_;
    d.alloc(n + IFEM_TMG_PAD);
    IFEM_HIP_CHECK(hipMemsetAsync(d.p, 0xff, (n + IFEM_TMG_PAD) * sizeof(T), s));
    if (in_out && n) {
      std::vector<T> h(host, host + n);
      IFEM_HIP_CHECK(hipMemcpyAsync(d.p, h.data(), n * sizeof(T), hipMemcpyHostToDevice, s));
      IFEM_HIP_CHECK(hipStreamSynchronize(s)); // h leaves scope
    }
  }
  void close(double *host, hipStream_t s) {
    std::vector<T> h(n + IFEM_TMG_PAD);
    IFEM_HIP_CHECK(hipMemcpyAsync(h.data(), d.p, h.size() * sizeof(T), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = 0; i < h.size(); ++i) host[i] = double(h[i]);
  }
};
// device input of n entries of T from a host array of doubles (rounded to T)
template <typename T>
void upload_as(DBuf<T> &d, const double *host, size_t n, hipStream_t s) {
  std::vector<T> h(host, host + n);
  d.upload(h.data(), n, s);
  IFEM_HIP_CHECK(hipStreamSynchronize(s)); // h leaves scope
}
} // namespace
} // extern "C++"

int ifem_test_mg_transfer(ifem_ctx *ctx, int kind, int64_t n_rows, int64_t n_cols, const int64_t *ptr, const int32_t *col, const double *w,
                          const uint8_t *flag_in, const uint8_t *flag_out, const double *x, double *y) {
  IFEM_API_BEGIN
  if (kind < 0 || kind > 1 || n_rows < 0 || n_cols < 0 || !ptr || !y) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_transfer: kind 0 / 1, n_rows >= 0, n_cols >= 0, ptr and y");
  if (ctx->halo.nranks > 1) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_transfer: single-rank contexts");
  if (n_cols >= (int64_t(1) << 29)) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_transfer: packed entries hold 29 column bits");
  // the table as ifem_mg_attach checks it: a malformed one would send the kernels out of bounds
  const int64_t nnz = ptr[n_rows];
  if (ptr[0] != 0 || nnz < 0) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_transfer: row pointers do not span the table");
  for (int64_t r = 0; r < n_rows; ++r)
    if (ptr[r + 1] < ptr[r]) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_transfer: row pointers decrease");
  if ((nnz && (!col || !w)) || (n_cols && !x)) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_transfer: col, w and x");
  for (int64_t k = 0; k < nnz; ++k)
    if (col[k] < 0 || col[k] >= n_cols) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_transfer: column out of range");
  hipStream_t s = ctx->stream;
  const size_t dim = size_t(ctx->dim);
  MgCsr M;
  M.n_rows = n_rows;
  M.ptr.upload(ptr, size_t(n_rows) + 1, s);
  M.col.upload(col, size_t(nnz), s);
  M.w.upload(w, size_t(nnz), s);
  if (kind == 0) {
    DBuf<double> dx;
    dx.upload(x, size_t(n_cols), s);
    GuardedOut<double> dy;
    dy.open(nullptr, size_t(n_rows), false, s);
    mg_csr_apply(ctx, M, dx.p, dy.d.p);
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
    dy.close(y, s);
  } else {
    DBuf<uint8_t> fi, fo, mask;
    if (flag_in) fi.upload(flag_in, size_t(n_cols) * dim, s);
    if (flag_out) fo.upload(flag_out, size_t(n_rows) * dim, s);
    DBuf<float> dx;
    upload_as(dx, x, size_t(n_cols) * dim, s);
    GuardedOut<float> dy;
    dy.open(nullptr, size_t(n_rows) * dim, false, s);
    mg_csr_mask(ctx, M, fi.p, fo.p, mask);
    mg_csr_apply_nodes_f32(ctx, M, dx.p, mask, dy.d.p);
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
    dy.close(y, s);
  }
  IFEM_HIP_CHECK(hipGetLastError());
  IFEM_API_END
}

int ifem_test_mg_lattice_transfer(ifem_ctx *fine, int which, int path, const double *x, double *y, int64_t info[4]) {
  IFEM_API_BEGIN
  if (!fine || which < 0 || which > 1 || path < 0 || path > 1 || !x || !y || !info) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_lattice_transfer: which 0 / 1, path 0 / 1, x, y and info");
  ifem_ctx *cc = fine->mg_coarse;
  if (!cc || fine->mg_Pu.n_rows != fine->nUo || fine->nUo <= 0 || fine->mg_Ru.n_rows != cc->nUl)
    throw Error(IFEM_E_BADPARAM, "ifem_test_mg_lattice_transfer: a level with velocity transfers to an attached coarser level");
  hipStream_t s = fine->stream;
  const size_t dim = size_t(fine->dim);
  cc->asm_constraint_set = fine->asm_constraint_set; // as the set-up of a cycle leaves the chain
  mg_transfer_u_setup(fine, fine->asm_constraint_set, 0);
  const bool prolong = which == 0;
  const size_t n_in = (prolong ? size_t(cc->nUl) : size_t(fine->nUo)) * dim, n_out = (prolong ? size_t(fine->nUo) : size_t(cc->nUl)) * dim;
  DBuf<float> dx;
  upload_as(dx, x, n_in, s);
  GuardedOut<float> dy;
  dy.open(nullptr, n_out, false, s);
  mg_transfer_u(fine, prolong, dx.p, dy.d.p, /*csr_only=*/path == 0);
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  dy.close(y, s);
  IFEM_HIP_CHECK(hipGetLastError());
  info[0] = fine->mg_lattice_u.state; info[1] = fine->mg_lattice_u.bad_p; info[2] = fine->mg_lattice_u.bad_r;
  info[3] = (path == 1 && mg_lattice_u_active(fine)) ? 1 : 0;
  IFEM_API_END
}

int ifem_test_mg_vec_kernel(ifem_ctx *ctx, int op, int64_t n, int64_t m, const double *coef, const int32_t *idx, double *in0, double *in1,
                            double *out0, double *out1, double *out2) {
  IFEM_API_BEGIN
  if (op < 0 || op >= IFEM_TMG_COUNT || n < 0 || !out0) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_vec_kernel: op, n >= 0 and out0");
  if (ctx->halo.nranks > 1) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_vec_kernel: single-rank contexts");
  const bool block = op == IFEM_TMG_VC_ENTRY || op == IFEM_TMG_VC_ENTRY_F32 || op == IFEM_TMG_CHEB_INIT_BLOCK_F32;
  const bool need_in0 = op != IFEM_TMG_VEC_RECIP && op != IFEM_TMG_VEC_ROUGH;
  const bool need_in1 = op == IFEM_TMG_CHEB_INIT || op == IFEM_TMG_CHEB_STEP || op == IFEM_TMG_VC_EXIT || op == IFEM_TMG_VC_EXIT_F32;
  const bool need_coef = op == IFEM_TMG_CHEB_INIT || op == IFEM_TMG_CHEB_STEP || op == IFEM_TMG_AXPY_F32V || block;
  const bool need_out1 = op == IFEM_TMG_CHEB_STEP || op == IFEM_TMG_VC_ENTRY || op == IFEM_TMG_VC_ENTRY_F32;
  if ((need_in0 && !in0) || (need_in1 && !in1) || (need_coef && !coef) || (need_out1 && !out1) || (op == IFEM_TMG_CHEB_STEP && !out2))
    throw Error(IFEM_E_BADPARAM, "ifem_test_mg_vec_kernel: a null array this op uses");
  const size_t dim = size_t(ctx->dim), N = size_t(n);
  if (block && (!ctx->assembled || n != int64_t(dim) * ctx->nUo || ctx->bjac.n != size_t(ctx->nUo) * dim * dim))
    throw Error(IFEM_E_BADPARAM, "ifem_test_mg_vec_kernel: the node-block ops run after an assembly, n = dim * n_unodes");
  if (op == IFEM_TMG_INJECT_NODES) {
    if (m < 0 || (n && !idx)) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_vec_kernel: the injection needs m >= 0 fine nodes and idx");
    for (int64_t i = 0; i < n; ++i)
      if (idx[i] < -1 || idx[i] >= m) throw Error(IFEM_E_BADPARAM, "ifem_test_mg_vec_kernel: injection index out of range");
  }
  hipStream_t s = ctx->stream;
  DBuf<double> a0, a1;
  DBuf<float> f0, f1;
  DBuf<int32_t> di;
  GuardedOut<double> o0, o1, o2;
  GuardedOut<float> g0, g1;
  switch (op) {
  case IFEM_TMG_CHEB_INIT:
    a0.upload(in0, N, s); a1.upload(in1, N, s);
    o0.open(nullptr, N, false, s);
    cheb_init(ctx, n, coef[0], a0.p, a1.p, o0.d.p);
    break;
  case IFEM_TMG_CHEB_STEP:
    a0.upload(in0, N, s); a1.upload(in1, N, s);
    o0.open(out0, N, true, s); o1.open(out1, N, true, s); o2.open(out2, N, true, s);
    cheb_step(ctx, n, coef[0], coef[1], a0.p, a1.p, o0.d.p, o1.d.p, o2.d.p);
    break;
  case IFEM_TMG_VEC_RECIP:
    o0.open(out0, N, true, s);
    vec_recip(ctx, n, o0.d.p);
    break;
  case IFEM_TMG_VEC_ROUGH:
    o0.open(nullptr, N, false, s);
    vec_rough(ctx, n, m, o0.d.p);
    break;
  case IFEM_TMG_CVT_D2F:
    a0.upload(in0, N, s);
    g0.open(nullptr, N, false, s);
    v_cvt_d2f(ctx, n, a0.p, g0.d.p);
    break;
  case IFEM_TMG_CVT_F2D:
    upload_as(f0, in0, N, s);
    o0.open(nullptr, N, false, s);
    v_cvt_f2d(ctx, n, f0.p, o0.d.p);
    break;
  case IFEM_TMG_AXPY_F32V:
    upload_as(f0, in0, N, s);
    g0.open(out0, N, true, s);
    v_axpy_f32v(ctx, n, float(coef[0]), f0.p, g0.d.p);
    break;
  case IFEM_TMG_VC_EXIT:
    upload_as(f0, in0, N, s); upload_as(f1, in1, N, s);
    o0.open(nullptr, N, false, s);
    vc_exit(ctx, n, f0.p, f1.p, o0.d.p);
    break;
  case IFEM_TMG_VC_EXIT_F32:
    upload_as(f0, in0, N, s); upload_as(f1, in1, N, s);
    g0.open(nullptr, N, false, s);
    vc_exit_f32(ctx, n, f0.p, f1.p, g0.d.p);
    break;
  case IFEM_TMG_INJECT_NODES:
    a0.upload(in0, size_t(m) * dim, s);
    di.upload(idx, N, s);
    o0.open(nullptr, N * dim, false, s);
    mg_inject_nodes(ctx, n, di.p, a0.p, o0.d.p);
    break;
  case IFEM_TMG_VC_ENTRY:
    a0.upload(in0, N, s);
    g0.open(nullptr, N, false, s); g1.open(nullptr, N, false, s);
    vc_entry(ctx, coef[0], a0.p, g0.d.p, g1.d.p);
    break;
  case IFEM_TMG_VC_ENTRY_F32:
    upload_as(f0, in0, N, s);
    g0.open(nullptr, N, false, s); g1.open(nullptr, N, false, s);
    vc_entry_f32(ctx, coef[0], f0.p, g0.d.p, g1.d.p);
    break;
  default: // IFEM_TMG_CHEB_INIT_BLOCK_F32
    upload_as(f0, in0, N, s);
    g0.open(nullptr, N, false, s);
    cheb_init_block_f32(ctx, coef[0], f0.p, g0.d.p);
    break;
  }
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  IFEM_HIP_CHECK(hipGetLastError());
  if (o0.d.p) o0.close(out0, s);
  if (g0.d.p) g0.close(out0, s);
  if (o1.d.p) o1.close(out1, s);
  if (g1.d.p) g1.close(out1, s);
  if (o2.d.p) o2.close(out2, s);
  if (op == IFEM_TMG_CHEB_STEP && n) { // the two read-only inputs as the device holds them after the call
    IFEM_HIP_CHECK(hipMemcpyAsync(in0, a0.p, N * sizeof(double), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipMemcpyAsync(in1, a1.p, N * sizeof(double), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
  }
  IFEM_API_END
}

int ifem_test_mp_solve(ifem_ctx *ctx, const ifem_solver_opts *o, const double *b, double *x, int32_t info[2]) {
  IFEM_API_BEGIN
  if (!b || !x || !info) throw Error(IFEM_E_BADPARAM, "ifem_test_mp_solve: b, x and info");
  if (!ctx->mp_direct.mass_ready) throw Error(IFEM_E_BADPARAM, "ifem_test_mp_solve called before an assembly that integrated M_p");
  const ifem_solver_opts oo = opts_or_default(o);
  const size_t n = size_t(ctx->nPo);
  DBuf<double> db, dx;
  db.upload(b, n, ctx->stream);
  dx.alloc(n);
  mp_solve_probe(ctx, &oo, db.p, dx.p, info);
  if (n) IFEM_HIP_CHECK(hipMemcpyAsync(x, dx.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_test_sm_solve(ifem_ctx *ctx, const ifem_solver_opts *o, const double *b, double *x, int64_t info[4]) {
  IFEM_API_BEGIN
  if (!b || !x || !info) throw Error(IFEM_E_BADPARAM, "ifem_test_sm_solve: b, x and info");
  if (!ctx->assembled && !ctx->geo.valid) throw Error(IFEM_E_BADPARAM, "ifem_test_sm_solve called before an assembly that left B, B^T and diag(M_u) behind");
  const ifem_solver_opts oo = opts_or_default(o);
  const size_t n = size_t(ctx->nPo);
  DBuf<double> db, dx;
  db.upload(b, n, ctx->stream);
  dx.alloc(n);
  if (n) IFEM_HIP_CHECK(hipMemsetAsync(dx.p, 0, n * sizeof(double), ctx->stream));
  sm_solve_probe(ctx, &oo, db.p, dx.p, info);
  if (n) IFEM_HIP_CHECK(hipMemcpyAsync(x, dx.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_test_sm_apply(ifem_ctx *ctx, int path, const double *x, double *y, int64_t info[4]) {
  IFEM_API_BEGIN
  if (path < 0 || path > 3 || !info) throw Error(IFEM_E_BADPARAM, "ifem_test_sm_apply: path 0..3 and info");
  if (path >= 2) { sm_apply_probe(ctx, path, nullptr, nullptr, info); return IFEM_OK; }
  if (!x || !y) throw Error(IFEM_E_BADPARAM, "ifem_test_sm_apply: x and y");
  if (!ctx->geo.valid) throw Error(IFEM_E_BADPARAM, "ifem_test_sm_apply called before an assembly that left B, B^T and diag(M_u) behind");
  if (ctx->halo.nranks > 1 && path == 0) throw Error(IFEM_E_BADPARAM, "ifem_test_sm_apply: path 0 is single-rank (several ranks: path 1, collective)");
  const size_t n = size_t(ctx->nPo);
  DBuf<double> dx, dy;
  dx.upload(x, n, ctx->stream);
  dy.alloc(n);
  sm_apply_probe(ctx, path, dx.p, dy.p, info);
  if (n) IFEM_HIP_CHECK(hipMemcpyAsync(y, dy.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_test_b_apply(ifem_ctx *ctx, int which, int path, const double *x, double *y, int64_t info[4]) {
  IFEM_API_BEGIN
  if (which < 0 || which > 2 || path < 0 || path > 3 || !info) throw Error(IFEM_E_BADPARAM, "ifem_test_b_apply: which 0..2, path 0..3 and info");
  if (path >= 2) { b_apply_probe(ctx, which, path, nullptr, nullptr, info); return IFEM_OK; }
  if (!x || !y) throw Error(IFEM_E_BADPARAM, "ifem_test_b_apply: x and y");
  if (!ctx->assembled && !ctx->geo.valid) throw Error(IFEM_E_BADPARAM, "ifem_test_b_apply called before an assembly that left B and B^T behind");
  const size_t nu = size_t(ctx->dim) * size_t(ctx->nUl), np = size_t(ctx->nPl), nuo = size_t(ctx->dim) * size_t(ctx->nUo), npo = size_t(ctx->nPo);
  const size_t n_in = which == 0 ? nu : np, n_out = which == 0 ? npo : nuo;
  DBuf<double> dx, dy;
  dx.upload(x, n_in, ctx->stream);
  if (which == 2) dy.upload(y, n_out, ctx->stream); else dy.alloc(n_out);
  b_apply_probe(ctx, which, path, dx.p, dy.p, info);
  if (n_out) IFEM_HIP_CHECK(hipMemcpyAsync(y, dy.p, n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_precond_vmult(ifem_ctx *ctx, const ifem_ins_params *p, const ifem_solver_opts *o, int dst, int src) {
  IFEM_API_BEGIN
  if (!vec_ok(dst) || !vec_ok(src) || is_ext(dst) || is_ext(src)) throw Error(IFEM_E_BADPARAM, "use non-ghosted vectors");
  const ifem_solver_opts oo = opts_or_default(o);
  ins_precond_vmult(ctx, p, &oo, ctx->vec[src].p, ctx->vec[dst].p);
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  IFEM_API_END
}

int ifem_tpp_ilu_probe(ifem_ctx *ctx, int64_t *rowptr, int32_t *col, double *val, const double *x, double *y, int32_t *levels) {
  IFEM_API_BEGIN
  if (!ctx->assembled || !ctx->has_app) throw Error(IFEM_E_BADPARAM, "ifem_tpp_ilu_probe after ifem_scns_assemble");
  if (ctx->halo.nranks > 1) throw Error(IFEM_E_BADPARAM, "ifem_tpp_ilu_probe: single-rank contexts only");
  if (!rowptr) throw Error(IFEM_E_BADPARAM, "ifem_tpp_ilu_probe: rowptr is required");
  hipStream_t s = ctx->stream;
  bjac_setup(ctx);
  ifem::tpp_numeric(ctx);
  const int64_t n = ctx->Sm.n_rows;
  IFEM_HIP_CHECK(hipMemcpyAsync(rowptr, ctx->Sm.rowptr.p, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  if (col && val) {
    IFEM_HIP_CHECK(hipMemcpyAsync(col, ctx->Sm.col.p, (size_t)rowptr[n] * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipMemcpyAsync(val, ctx->Tpp.p, (size_t)rowptr[n] * sizeof(double), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
  }
  if (x && y) {
    if (ctx->tune.tpp_ilu_order < 0) throw Error(IFEM_E_BADPARAM, "ifem_tpp_ilu_probe: tpp_ilu_order = -1 keeps no ILU");
    if (!ifem::tpp_ilu_factor(ctx))
      throw Error(IFEM_E_KRYLOV_NOCONV, "ILU(0) of T_pp broke down: zero, tiny or non-finite pivot (|pivot| in [" + std::to_string(ctx->tpp_ilu.pivot_min) +
                                            ", " + std::to_string(ctx->tpp_ilu.pivot_max) + "])");
    DBuf<double> dx, dy;
    dx.upload(x, (size_t)n, s);
    dy.alloc((size_t)n);
    ifem::tpp_ilu_apply(ctx, dx.p, dy.p);
    IFEM_HIP_CHECK(hipMemcpyAsync(y, dy.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    IFEM_HIP_CHECK(hipStreamSynchronize(s));
    if (levels) *levels = ifem::tpp_ilu_levels(ctx);
  }
  IFEM_API_END
}

int ifem_scns_pc_probe(ifem_ctx *ctx, int which, const double *x, double *y) {
  IFEM_API_BEGIN
  if (!ctx->assembled || !ctx->has_app) throw Error(IFEM_E_BADPARAM, "ifem_scns_pc_probe after ifem_scns_assemble");
  if (ctx->halo.nranks > 1) throw Error(IFEM_E_BADPARAM, "ifem_scns_pc_probe: single-rank contexts only");
  if (!x || !y) throw Error(IFEM_E_BADPARAM, "ifem_scns_pc_probe: null vector");
  hipStream_t s = ctx->stream;
  const size_t n = which == 0 ? (size_t)ctx->dim * ctx->nUo : (size_t)ctx->nPo;
  DBuf<double> dx, dy;
  dx.upload(x, n, s);
  dy.alloc(n);
  ifem::scns_pc_probe(ctx, which, dx.p, dy.p);
  IFEM_HIP_CHECK(hipMemcpyAsync(y, dy.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
  IFEM_API_END
}

int ifem_tpp_override(ifem_ctx *ctx, const double *val) {
  IFEM_API_BEGIN
  if (!ctx) throw Error(IFEM_E_BADPARAM, "ifem_tpp_override: null context");
  if (ctx->halo.nranks > 1) throw Error(IFEM_E_BADPARAM, "ifem_tpp_override is a single-rank test aid");
  if (!ctx->tpp_valid || !val) throw Error(IFEM_E_BADPARAM, "ifem_tpp_override after ifem_tpp_ilu_probe, with values");
  IFEM_HIP_CHECK(hipMemcpyAsync(ctx->Tpp.p, val, ctx->Tpp.n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  scalar_diag(ctx, ctx->Sm, ctx->Tpp.p, ctx->tpp_diag.p); // (single rank: T_pp lives on the pattern of S_m) the Jacobi fallback of a broken-down ILU divides by THIS matrix's diagonal
  IFEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->tpp_ilu.factored = false;
  IFEM_API_END
}

// rows [row0, row0 + nrows) of the local system as CSR, pattern [A_uu | B^T ; B | M_p-pattern] (explicit zeros kept so that both `which`
// share one pattern), downloading only the slices of the device arrays those rows own (the whole A_uu of the 128^3 channel is 78 GB:
// ifem_export_csr cannot be called there)
static void export_rows(ifem_ctx *ctx, int which, int64_t row0, int64_t nrows, int64_t *rowptr, int32_t *col, double *val) {
  hipStream_t s = ctx->stream;
  const int dim = ctx->dim, bs = dim * dim;
  const int64_t nuo = dim * ctx->nUo, npo = ctx->nPo, n = nuo + npo, poff = dim * ctx->nUl;
  if (!rowptr || row0 < 0 || nrows < 0 || row0 + nrows > n) throw Error(IFEM_E_BADPARAM, "ifem_export_rows: row range outside the local system");
  rowptr[0] = 0;
  // ---- velocity rows: nodes A0 .. A1-1 cover them
  const int64_t u0 = std::min(row0, nuo), u1 = std::min(row0 + nrows, nuo);
  if (u1 > u0) {
    const int64_t A0 = u0 / dim, A1 = (u1 + dim - 1) / dim;
    auto rpA = download_range(ctx->Auu.rowptr, A0, A1 - A0 + 1, s), rpT = download_range(ctx->Bt.rowptr, A0, A1 - A0 + 1, s);
    for (int64_t r = u0; r < u1; ++r) {
      const int64_t a = r / dim - A0;
      rowptr[r - row0 + 1] = rowptr[r - row0] + (rpA[a + 1] - rpA[a]) * dim + (rpT[a + 1] - rpT[a]);
    }
    if (col && val) {
      const int64_t b0 = rpA[0], b1 = rpA[A1 - A0], t0 = rpT[0], t1 = rpT[A1 - A0];
      auto cA = download_range(ctx->Auu.col, b0, b1 - b0, s);
      std::vector<double> vA;
      if (which == 0) vA = download_range(stored_uu(ctx), b0 * bs, (b1 - b0) * bs, s);
      auto cT = download_range(ctx->Bt.col, t0, t1 - t0, s);
      auto vT = download_range(ctx->Bt.val, t0 * dim, (t1 - t0) * dim, s);
      auto dM = download_range(ctx->diagMu, A0 * dim, (A1 - A0) * dim, s);
      for (int64_t r = u0; r < u1; ++r) {
        const int64_t A = r / dim, a = A - A0;
        const int c = int(r % dim);
        const int64_t rs = rpA[a], len = rpA[a + 1] - rs, ts = rpT[a], tlen = rpT[a + 1] - ts;
        int64_t o = rowptr[r - row0];
        for (int64_t k = 0; k < len; ++k)
          for (int d = 0; d < dim; ++d) {
            col[o] = cA[rs - b0 + k] * dim + d;
            if (which == 0) val[o] = vA[uu_base(rs, len, k, bs) + (c * dim + d) * uu_estride(len) - b0 * bs];
            else val[o] = (cA[rs - b0 + k] == A && c == d) ? dM[a * dim + c] : 0.0;
            ++o;
          }
        for (int64_t k = 0; k < tlen; ++k) {
          col[o] = int32_t(poff + cT[ts - t0 + k]);
          val[o] = (which == 0) ? vT[ts * dim + c * tlen + k - t0 * dim] : 0.0;
          ++o;
        }
      }
    }
  }
  // ---- pressure rows
  const int64_t p0 = std::max(row0, nuo) - nuo, p1 = row0 + nrows - nuo;
  if (p1 > p0) {
    auto rpB = download_range(ctx->B.rowptr, p0, p1 - p0 + 1, s), rpM = download_range(ctx->Mp.rowptr, p0, p1 - p0 + 1, s);
    for (int64_t i = p0; i < p1; ++i) {
      const int64_t j = i - p0, r = nuo + i - row0;
      rowptr[r + 1] = rowptr[r] + (rpB[j + 1] - rpB[j]) * dim + (rpM[j + 1] - rpM[j]);
    }
    if (col && val) {
      const int64_t b0 = rpB[0], b1 = rpB[p1 - p0], m0 = rpM[0], m1 = rpM[p1 - p0];
      auto cB = download_range(ctx->B.col, b0, b1 - b0, s);
      auto vB = download_range(ctx->B.val, b0 * dim, (b1 - b0) * dim, s);
      auto cM = download_range(ctx->Mp.col, m0, m1 - m0, s);
      auto vM = download_range(ctx->Mp.val, m0, m1 - m0, s);
      std::vector<double> vApp;
      if (ctx->has_app) vApp = download_range(ctx->App, m0, m1 - m0, s);
      for (int64_t i = p0; i < p1; ++i) {
        const int64_t j = i - p0;
        const int64_t rs = rpB[j], len = rpB[j + 1] - rs, ms = rpM[j], mlen = rpM[j + 1] - ms;
        int64_t o = rowptr[nuo + i - row0];
        for (int64_t k = 0; k < len; ++k)
          for (int d = 0; d < dim; ++d) {
            col[o] = cB[rs - b0 + k] * dim + d;
            val[o] = (which == 0) ? vB[rs * dim + d * len + k - b0 * dim] : 0.0;
            ++o;
          }
        for (int64_t k = 0; k < mlen; ++k) {
          col[o] = int32_t(poff + cM[ms - m0 + k]);
          val[o] = (which == 0) ? (ctx->has_app ? vApp[ms - m0 + k] : 0.0) : vM[ms - m0 + k];
          ++o;
        }
      }
    }
  }
}

int ifem_export_rows(ifem_ctx *ctx, int which, int64_t row0, int64_t nrows, int64_t *rowptr, int32_t *col, double *val) {
  IFEM_API_BEGIN
  export_rows(ctx, which, row0, nrows, rowptr, col, val);
  IFEM_API_END
}

// the whole local system: the slab [0, n)
int ifem_export_csr(ifem_ctx *ctx, int which, int64_t *rowptr, int32_t *col, double *val) {
  IFEM_API_BEGIN
  export_rows(ctx, which, 0, int64_t(ctx->dim) * ctx->nUo + ctx->nPo, rowptr, col, val);
  IFEM_API_END
}

// the stored block pattern of A_uu for the nodes [node0, node0 + n_nodes): ABSOLUTE block offsets (block k of the array holds the
// values [k * dim^2, (k + 1) * dim^2)) and block columns in storage order -- what the scatter of the cell kernel addresses
int ifem_export_uu_pattern(ifem_ctx *ctx, int64_t node0, int64_t n_nodes, int64_t *rowptr, int32_t *col) {
  IFEM_API_BEGIN
  if (!rowptr || node0 < 0 || n_nodes < 0 || node0 + n_nodes > ctx->Auu.n_rows) throw Error(IFEM_E_BADPARAM, "ifem_export_uu_pattern: node range outside the owned rows");
  hipStream_t s = ctx->stream;
  auto rp = download_range(ctx->Auu.rowptr, node0, n_nodes + 1, s);
  std::copy(rp.begin(), rp.end(), rowptr);
  if (col) {
    auto c = download_range(ctx->Auu.col, rp.front(), rp.back() - rp.front(), s);
    std::copy(c.begin(), c.end(), col);
  }
  IFEM_API_END
}

int ifem_get_timing(ifem_ctx *ctx, ifem_timing *t) {
  IFEM_API_BEGIN
  *t = ctx->timing; // spmv_uu_bytes is set by the profiled launches themselves (linalg.hip::spmv_uu)
  IFEM_API_END
}

int ifem_comm_stats_get(ifem_ctx *ctx, ifem_comm_stats *out, int reset) {
  IFEM_API_BEGIN
  if (!out) throw Error(IFEM_E_BADPARAM, "ifem_comm_stats_get: null output");
  ifem::comm_stats(ctx, out, reset != 0);
  IFEM_API_END
}

int ifem_comm_stats_level(ifem_ctx *ctx, int level, ifem_comm_stats *out) {
  IFEM_API_BEGIN
  if (!out || level < 0) throw Error(IFEM_E_BADPARAM, "ifem_comm_stats_level: an output and a level >= 0");
  ifem_ctx *c = ctx;
  for (int k = 0; k < level && c; ++k) c = c->mg_coarse;
  if (!c) throw Error(IFEM_E_BADPARAM, "ifem_comm_stats_level: the chain has fewer levels");
  ifem::comm_stats(c, out, false, /*single_level=*/true);
  IFEM_API_END
}

int ifem_test_restart_fits(ifem_ctx *ctx, int columns) {
  if (!ctx || columns < 0) return IFEM_E_BADPARAM;
  ctx->test_restart_fits = columns;
  return IFEM_OK;
}

int ifem_test_mf_uniform(ifem_ctx *ctx, double *h) {
  if (!ctx) return IFEM_E_BADPARAM;
  if (h) for (int d = 0; d < 3; ++d) h[d] = ctx->mf_uniform ? ctx->mf_h[d] : 0.0;
  return ifem::mf_takes_uniform(ctx) ? 1 : 0;
}

int ifem_test_asm_rows(ifem_ctx *ctx, int verbose, int32_t *state) {
  if (!ctx || !state) return IFEM_E_BADPARAM;
  *state = ctx->rows_state;
  if (verbose && ctx->rows_state < 0) fprintf(stderr, "[ifem] A_uu row owners refused: %s\n", ctx->rows_why ? ctx->rows_why : "?");
  return IFEM_OK;
}

int ifem_test_rows_const(ifem_ctx *ctx, const ifem_ins_params *p, int imex, double *out) {
  IFEM_API_BEGIN
  if (!p || !out) throw Error(IFEM_E_BADPARAM, "ifem_test_rows_const: null argument");
  ifem::rows_const_table(ctx, p, imex, out);
  IFEM_API_END
}

int ifem_inner_restart_length(ifem_ctx *ctx) { return ctx ? ctx->inner_restart_eff : IFEM_E_BADPARAM; }

int ifem_vcycle_graph_stats(ifem_ctx *ctx, uint64_t *captures, uint64_t *launches) {
  IFEM_API_BEGIN
  if (captures) *captures = ctx->vc_graph.captures + ctx->sm_graph.captures + ctx->pa_graph.captures;
  if (launches) *launches = ctx->vc_graph.launches + ctx->sm_graph.launches + ctx->pa_graph.launches;
  IFEM_API_END
}

int ifem_kprof_begin(ifem_ctx *ctx) {
  IFEM_API_BEGIN
  ifem::KProf &k = ifem::kprof_root(ctx);
  k.recs.clear();
  k.used = 0;
  k.depth = 0;
  k.on = true;
  IFEM_API_END
}

int ifem_kprof_end(ifem_ctx *ctx, ifem_kprof_entry *out, int32_t max_entries) {
  int written = 0;
  IFEM_API_BEGIN
  ifem::KProf &k = ifem::kprof_root(ctx);
  k.on = false;
  IFEM_HIP_CHECK(hipSetDevice(ctx->device));
  IFEM_HIP_CHECK(hipDeviceSynchronize());
  ifem_kprof_entry acc[IFEM_KC_COUNT];
  for (int f = 0; f < IFEM_KC_COUNT; ++f) acc[f] = {f, 0u, 0.0, 0.0, 0.0};
  for (const auto &r : k.recs) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, k.ev[r.e0], k.ev[r.e1]) != hipSuccess) continue; // a scope cut short by an exception
    ifem_kprof_entry &a = acc[r.cat >= 0 && r.cat < IFEM_KC_COUNT ? r.cat : IFEM_KC_OTHER];
    a.scopes++; a.ms += ms; a.bytes += r.bytes; a.flops += r.flops;
  }
  k.recs.clear();
  k.used = 0;
  for (int f = 0; f < IFEM_KC_COUNT && out && written < max_entries; ++f)
    if (acc[f].scopes) out[written++] = acc[f];
  return written;
  IFEM_API_END
}

const char *ifem_kprof_family_name(int32_t family) {
  static const char *names[IFEM_KC_COUNT] = {"assemble_cells", "zero_fill", "spmv_uu", "spmv_b_bt", "mf_cell", "mf_gather", "spmv_sm", "spmv_mp",
                                             "mdot", "maxpy", "vector_ops", "mg_transfer", "smoother_setup", "cg_recurrence", "schur_setup", "other", "tpp_ilu", "refine"};
  return family >= 0 && family < IFEM_KC_COUNT ? names[family] : "?";
}

int ifem_set_ainv_kind(ifem_ctx *ctx, int kind) { ctx->want_shat = kind == IFEM_AINV_SCALAR_GMRES; return IFEM_OK; }
int ifem_set_profiling(ifem_ctx *ctx, int on) { ctx->profile = on != 0; ++ctx->graph_epoch; return IFEM_OK; }
int ifem_synchronize(ifem_ctx *ctx) {
  IFEM_API_BEGIN
  IFEM_HIP_CHECK(hipSetDevice(ctx->device));
  IFEM_HIP_CHECK(hipDeviceSynchronize());
  IFEM_API_END
}

int ifem_comm_unique_id(uint8_t out[128]) { return ifem::comm_unique_id(out); }
int ifem_comm_selftest(int device) {
  IFEM_API_BEGIN
  ifem::comm_selftest(device);
  IFEM_API_END
}
void *ifem_local_world_create(int nranks) { return ifem::local_world_create(nranks); }
void ifem_local_world_destroy(void *w) { ifem::local_world_destroy(w); }

} // extern "C"
