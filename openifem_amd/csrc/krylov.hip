// krylov.hip -- the Krylov drivers: restarted GMRES in its three forms (fp64 bases; single-precision basis; flexible with both bases in single precision)
// around one host-side Arnoldi recurrence, and CG in its host- and device-scalar forms.  They know operators and preconditioners as callables and vectors
// as device pointers -- nothing of the PDE, the context's matrices or the multigrids (solver.hip); every vector operation is a launcher of linalg.hip.
#include <cmath>
#include "krylov.hpp"

namespace ifem {

// Host arithmetic of one restart cycle, shared by the three GMRES drivers below: the Hessenberg matrix H (row-major, (m+1) x m), the Givens
// rotations (cs, sn) that keep it triangular, the rotated right-hand side g and the solution y of the small triangular system.
struct Arnoldi {
  const int m;
  std::vector<double> H, cs, sn, g, y;
  explicit Arnoldi(int m_) : m(m_), H((size_t)(m_ + 1) * m_, 0.0), cs(m_), sn(m_), g(m_ + 1), y(m_) {}
  void start(double beta) { std::fill(g.begin(), g.end(), 0.0); g[0] = beta; }
  // column j = (h[0..j], hn): stored, rotated by the earlier rotations, annihilated by a new one; returns the residual estimate |g[j+1]|
  double column(int j, const double *h, double hn) {
    for (int i = 0; i <= j; ++i) H[(size_t)i * m + j] = h[i];
    H[(size_t)(j + 1) * m + j] = hn;
    for (int i = 0; i < j; ++i) {
      const double t = cs[i] * H[(size_t)i * m + j] + sn[i] * H[(size_t)(i + 1) * m + j];
      H[(size_t)(i + 1) * m + j] = -sn[i] * H[(size_t)i * m + j] + cs[i] * H[(size_t)(i + 1) * m + j];
      H[(size_t)i * m + j] = t;
    }
    const double a = H[(size_t)j * m + j], c = H[(size_t)(j + 1) * m + j], r = std::hypot(a, c);
    cs[j] = a / r; sn[j] = c / r;
    H[(size_t)j * m + j] = r; H[(size_t)(j + 1) * m + j] = 0;
    g[j + 1] = -sn[j] * g[j]; g[j] = cs[j] * g[j];
    return std::fabs(g[j + 1]);
  }
  // y[0..j) = H(0..j, 0..j)^-1 g[0..j): back substitution
  void solve(int j) {
    for (int i = j - 1; i >= 0; --i) {
      double t = g[i];
      for (int k = i + 1; k < j; ++k) t -= H[(size_t)i * m + k] * y[k];
      y[i] = t / H[(size_t)i * m + i];
    }
  }
};

// (flexible) right-preconditioned restarted GMRES, x0 = 0.  V: (m+1) x n, Z: m x n (flexible) or 1 x n.
// Orthogonalisation: classical Gram-Schmidt with one re-orthogonalisation pass (two fused multi-dot /
// multi-axpy sweeps instead of deal.II's j+1 sequential dots; same Krylov space, fewer host round trips).
int gmres(ifem_ctx *ctx, int64_t n, int64_t ld, bool reorth, const OpFn &A, const OpFn &Pinv, bool flexible,
                 const double *b, double *x, int m, int maxit, double tol, double *V, double *Z, double *w,
                 double *res_out,
                 const MdotFn &mdot,
                 std::vector<double> *history, // residual norm after every iteration (verbose runs)
                 const std::function<void(int, double *&, double *&)> *ensure, // bases that grow with the iteration count: called
                                                                                        // with the V columns the next iteration needs
                 const LeftPrecond *left_pc) {
  const bool left = left_pc != nullptr;
  double *stage = left ? left_pc->stage : nullptr;
  const OpFn *PA = left ? left_pc->PA : nullptr;
  Arnoldi K(m);
  std::vector<double> h(m + 1), h2(m + 1);
  v_zero(ctx, n, x);
  int it = 0;
  double res = 0;
  bool first = true;
  while (true) {
    const double *r0 = w; // the residual the cycle starts from: b itself in the first cycle (x = 0), b - A x after a restart
    if (first) { r0 = b; first = false; }
    else { A(x, w); v_axpby(ctx, n, 1.0, b, -1.0, w); }
    if (left) { Pinv(r0, Z); r0 = Z; }
    double bb;
    mdot(1, r0, n, r0, &bb);
    const double beta = std::sqrt(bb);
    res = beta;
    if (res <= tol || it >= maxit || !std::isfinite(res)) break; // (deal.II's SolverControl::check fails on a NaN as well)
    if (left && stage) v_scale_to2(ctx, n, 1.0 / beta, r0, V, stage);
    else v_scale_to(ctx, n, 1.0 / beta, r0, V);
    K.start(beta);
    int j = 0;
    bool done = false;
    for (; j < m && it < maxit; ++j) {
      if (ensure) (*ensure)(j + 2, V, Z); // columns 0 .. j + 1 of V, 0 .. j of Z
      double *vj = V + (int64_t)j * ld;
      double *zj = flexible ? Z + (int64_t)j * ld : Z;
      if (left && stage && PA) (*PA)(stage, w);
      else if (left) { A(stage ? stage : vj, zj); Pinv(zj, w); }
      else { Pinv(vj, zj); A(zj, w); }
      // classical Gram-Schmidt (twice with reorth); ||w||^2 comes out of the last multi-axpy pass (summed over the ranks like the
      // dot products of `mdot`): per iteration the host waits for the device once per pass, not three / five times
      double ww = 0;
      mdot(j + 1, V, ld, w, h.data());
      if (reorth) {
        v_maxpy(ctx, n, j + 1, V, ld, h.data(), w);
        mdot(j + 1, V, ld, w, h2.data());
        v_maxpy(ctx, n, j + 1, V, ld, h2.data(), w, &ww, true);
      } else {
        v_maxpy(ctx, n, j + 1, V, ld, h.data(), w, &ww, true);
        std::fill(h2.begin(), h2.end(), 0.0);
      }
      for (int i = 0; i <= j; ++i) h[i] += h2[i]; // column j of H: the coefficients of both passes
      const double hn = std::sqrt(ww);
      if (hn > 0) {
        if (left && stage) v_scale_to2(ctx, n, 1.0 / hn, w, V + (int64_t)(j + 1) * ld, stage);
        else v_scale_to(ctx, n, 1.0 / hn, w, V + (int64_t)(j + 1) * ld);
      }
      res = K.column(j, h.data(), hn);
      ++it;
      if (history) history->push_back(res);
      if (res <= tol || hn == 0 || !std::isfinite(res)) { ++j; done = true; break; }
    }
    K.solve(j);
    if (flexible || left) {
      for (int i = 0; i < j; ++i) h[i] = -K.y[i];
      v_maxpy(ctx, n, j, left ? V : Z, ld, h.data(), x); // x += sum y_i z_i   (left preconditioning: x += V y)
    } else {
      // x += P^-1 (V y): one preconditioner application instead of storing every z_j
      v_zero(ctx, n, w);
      for (int i = 0; i < j; ++i) h[i] = -K.y[i];
      v_maxpy(ctx, n, j, V, ld, h.data(), w);
      Pinv(w, Z);
      v_axpy(ctx, n, 1.0, Z, x);
    }
    if (done || it >= maxit) break;
  }
  if (res_out) *res_out = res;
  return it;
}

// Inner solver of the preconditioner: right-preconditioned restarted GMRES, x0 = 0, Krylov basis stored in single
// precision (half the Gram-Schmidt traffic; everything else fp64), single-pass classical Gram-Schmidt with the norm of
// the orthogonalised vector fused into the multi-axpy sweep.  Only used where an approximate A^-1 is admissible.
int gmres_f32basis(ifem_ctx *ctx, int64_t n, int64_t ld, const OpFn &A, const OpF32 &Pinv, const double *b, double *x,
                          int m, int maxit, double tol, float *V, double *z, double *w, double *res_out,
                          const std::function<void(double *, int)> &allreduce) {
  Arnoldi K(m);
  std::vector<double> h(m + 4);
  v_zero(ctx, n, x);
  int it = 0;
  double res = 0;
  bool first = true;
  while (true) {
    if (first) { v_copy(ctx, n, b, w); first = false; }
    else { A(x, w); v_axpby(ctx, n, 1.0, b, -1.0, w); }
    double bb = v_dot(ctx, n, w, w);
    allreduce(&bb, 1);
    const double beta = std::sqrt(bb);
    res = beta;
    if (res <= tol || it >= maxit || !std::isfinite(res)) break;
    v_scale_store_f32(ctx, n, 1.0 / beta, w, V);
    K.start(beta);
    int j = 0;
    bool done = false;
    for (; j < m && it < maxit; ++j) {
      Pinv(V + (int64_t)j * ld, z);
      A(z, w);
      v_mdot_f32(ctx, n, j + 1, V, ld, w, h.data());
      allreduce(h.data(), j + 1);
      double ww;
      v_maxpy_f32(ctx, n, j + 1, V, ld, h.data(), w, &ww);
      allreduce(&ww, 1);
      const double hn = std::sqrt(ww);
      if (hn > 0) v_scale_store_f32(ctx, n, 1.0 / hn, w, V + (int64_t)(j + 1) * ld);
      res = K.column(j, h.data(), hn);
      ++it;
      if (res <= tol || hn == 0 || !std::isfinite(res)) { ++j; done = true; break; }
    }
    K.solve(j);
    // x += P^-1 (V y): round V y to the basis precision (column m+1 of the basis is free at this point)
    v_zero(ctx, n, w);
    for (int i = 0; i < j; ++i) h[i] = -K.y[i];
    v_maxpy_f32(ctx, n, j, V, ld, h.data(), w, nullptr);
    float *vy = V + (int64_t)(m + 1) * ld;
    v_scale_store_f32(ctx, n, 1.0, w, vy);
    Pinv(vy, z);
    v_axpy(ctx, n, 1.0, z, x);
    if (done || it >= maxit) break;
  }
  if (res_out) *res_out = res;
  return it;
}

// Flexible inner solver of IFEM_AINV_MG (ifem_tuning::inner_f32): right-preconditioned restarted FGMRES, x0 = 0, with BOTH bases in single
// precision -- the preconditioner (a single-precision V-cycle) reads column j of V and writes column j of Z, the operator (single-precision
// cell arithmetic) reads that Z column and writes the fp64 w.  w, b, x, the Hessenberg arithmetic, the stopping test and the restart residual
// b - A x are fp64; Gram-Schmidt is the single fused pass of gmres(reorth = false).  Same iteration as gmres(flexible = true) up to the rounding
// of the stored columns.  The fused kernels take at most 64 columns per call: longer bases (the self-lengthening restart) go in chunks.
int fgmres_f32(ifem_ctx *ctx, int64_t n, int64_t ld, const OpFn &A, const OpF32 &Af, const OpF32F32 &Pinv, const double *b, double *x,
                      int m, int maxit, double tol, float *V, float *Z, double *w, double *res_out,
                      const std::function<void(double *, int)> &allreduce, const std::function<void(int, float *&, float *&)> &ensure) {
  Arnoldi K(m);
  std::vector<double> h(m + 4);
  constexpr int kChunk = 64;
  auto mdot = [&](int k, const float *B, double *out) {
    for (int k0 = 0; k0 < k; k0 += kChunk) v_mdot_f32(ctx, n, std::min(kChunk, k - k0), B + int64_t(k0) * ld, ld, w, out + k0);
    allreduce(out, k);
  };
  auto maxpy = [&](int k, const float *B, const double *coef, double *dst, double *norm2) { // dst -= sum coef_i B_i
    for (int k0 = 0; k0 < k; k0 += kChunk) {
      const bool last = k0 + kChunk >= k;
      v_maxpy_f32(ctx, n, std::min(kChunk, k - k0), B + int64_t(k0) * ld, ld, coef + k0, dst, last ? norm2 : nullptr);
    }
    if (norm2) allreduce(norm2, 1);
  };
  v_zero(ctx, n, x);
  int it = 0;
  double res = 0;
  bool first = true;
  while (true) {
    const double *r0 = w;
    if (first) { r0 = b; first = false; }
    else { A(x, w); v_axpby(ctx, n, 1.0, b, -1.0, w); }
    double bb = v_dot(ctx, n, r0, r0);
    allreduce(&bb, 1);
    const double beta = std::sqrt(bb);
    res = beta;
    if (res <= tol || it >= maxit || !std::isfinite(res)) break;
    v_scale_store_f32(ctx, n, 1.0 / beta, r0, V);
    K.start(beta);
    int j = 0;
    bool done = false;
    for (; j < m && it < maxit; ++j) {
      ensure(j + 2, V, Z); // columns 0 .. j + 1 of V, 0 .. j of Z
      float *zj = Z + (int64_t)j * ld;
      Pinv(V + (int64_t)j * ld, zj);
      Af(zj, w);
      mdot(j + 1, V, h.data());
      double ww = 0;
      maxpy(j + 1, V, h.data(), w, &ww);
      const double hn = std::sqrt(ww);
      if (hn > 0) v_scale_store_f32(ctx, n, 1.0 / hn, w, V + (int64_t)(j + 1) * ld);
      res = K.column(j, h.data(), hn);
      ++it;
      if (res <= tol || hn == 0 || !std::isfinite(res)) { ++j; done = true; break; }
    }
    K.solve(j);
    for (int i = 0; i < j; ++i) h[i] = -K.y[i];
    maxpy(j, Z, h.data(), x, nullptr); // x += sum y_i z_i
    if (done || it >= maxit) break;
  }
  if (res_out) *res_out = res;
  return it;
}

// plain CG, zero initial guess, absolute tolerance on ||r||_2
int cg(ifem_ctx *ctx, int64_t n, const OpFn &A, const double *b, double *x, double tol, int maxit, double *r,
              double *p, double *q, const std::function<double(const double *, const double *)> &dot) {
  v_zero(ctx, n, x);
  v_copy(ctx, n, b, r);
  v_copy(ctx, n, b, p);
  double rr = dot(r, r);
  int it = 0;
  while (std::sqrt(rr) > tol && it < maxit) {
    A(p, q);
    const double al = rr / dot(p, q);
    v_axpy(ctx, n, al, p, x);
    v_axpy(ctx, n, -al, q, r);
    const double rn = dot(r, r);
    v_axpby(ctx, n, 1.0, r, rn / rr, p);
    rr = rn;
    ++it;
  }
  return it;
}

// CG / Jacobi-PCG whose recurrence scalars stay on the device: five launches and no host round trip per iteration; the
// host reads ||r||^2 every `chk` iterations, so up to chk - 1 iterations run beyond the tolerance (harmless: they only
// tighten the solve).  Same iterates as cg() / pcg_jacobi() up to that point.  On several ranks the partial sums are
// all-reduced on the stream (RCCL) between the reduction and the scalar update: still no host round trip per iteration.
int cg_device(ifem_ctx *ctx, int64_t n, const OpFn &A, const double *diag, const double *b, double *x, double tol,
                     int maxit, double *r, double *z, double *p, double *q, int chk, double *s) {
  if (s && ctx->tune.cg_single_reduction) {
    // one reduction per iteration (linalg.hip::cg1_*): u = D^-1 r lives in z (or IS r), w = A u in q, s = A p
    double *u = diag ? z : r, *w = q;
    cg1_init(ctx, n, b, diag, x, r, u, p, s);
    A(u, w);
    cg1_dots(ctx, n, r, u, w, true);
    int it = 0;
    double rr = cgd_rr(ctx);
    while (std::sqrt(rr) > tol && it < maxit) {
      const int burst = std::min(chk, maxit - it);
      for (int k = 0; k < burst; ++k) {
        cg1_update(ctx, n, diag, u, w, p, s, x, r);
        A(u, w);
        cg1_dots(ctx, n, r, u, w, false);
      }
      it += burst;
      rr = cgd_rr(ctx);
      if (!(rr == rr)) break; // NaN guard
    }
    return it;
  }
  cgd_init(ctx, n, b, diag, x, r, z, p);
  int it = 0;
  double rr = cgd_rr(ctx);
  while (std::sqrt(rr) > tol && it < maxit) {
    const int burst = std::min(chk, maxit - it);
    for (int k = 0; k < burst; ++k) {
      A(p, q);
      cgd_alpha(ctx, n, p, q);
      cgd_update(ctx, n, diag, p, q, x, r, z);
    }
    it += burst;
    rr = cgd_rr(ctx);
    if (!(rr == rr)) break; // NaN guard
  }
  return it;
}

// test aid (ifem_test_cg_device): cg_device as the pressure solves call it -- the s work vector present, the form chosen by
// ifem_tuning::cg_single_reduction -- on A = diag(a), host data in and out; tol = 0 and chk = 1: exactly `iters` iterations
void test_cg_device(ifem_ctx *ctx, int64_t n, const double *a, const double *jac, const double *b, int iters, double *x) {
  hipStream_t s = ctx->stream;
  DBuf<double> da, dj, db, dx, w[5];
  auto up = [&](DBuf<double> &d, const double *h) {
    d.alloc((size_t)n);
    IFEM_HIP_CHECK(hipMemcpyAsync(d.p, h, size_t(n) * sizeof(double), hipMemcpyHostToDevice, s));
  };
  up(da, a);
  up(db, b);
  if (jac) up(dj, jac);
  dx.alloc((size_t)n);
  for (auto &v : w) v.alloc((size_t)n);
  const OpFn A = [&](const double *in, double *out) { vec_mul(ctx, n, da.p, in, out); };
  cg_device(ctx, n, A, jac ? dj.p : nullptr, db.p, dx.p, 0.0, iters, w[0].p, w[1].p, w[2].p, w[3].p, 1, w[4].p);
  IFEM_HIP_CHECK(hipMemcpyAsync(x, dx.p, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, s));
  IFEM_HIP_CHECK(hipStreamSynchronize(s));
}

// Jacobi-preconditioned CG, zero initial guess, same stopping rule (absolute tolerance on the TRUE residual ||r||_2).
// r and z must be adjacent (z = r + ld) so that <r,r> and <z,r> come out of one fused reduction.
int pcg_jacobi(ifem_ctx *ctx, int64_t n, const OpFn &A, const double *diag, const double *b, double *x, double tol,
                      int maxit, double *r, int64_t ld, double *p, double *q,
                      const MdotFn &mdot) {
  double *z = r + ld;
  v_zero(ctx, n, x);
  v_copy(ctx, n, b, r);
  vec_div(ctx, n, diag, r, z);
  v_copy(ctx, n, z, p);
  double d2[2];
  mdot(2, r, ld, r, d2);
  double rr = d2[0], rz = d2[1];
  int it = 0;
  while (std::sqrt(rr) > tol && it < maxit) {
    A(p, q);
    double pq;
    mdot(1, p, n, q, &pq);
    const double al = rz / pq;
    v_axpy(ctx, n, al, p, x);
    v_axpy(ctx, n, -al, q, r);
    vec_div(ctx, n, diag, r, z);
    mdot(2, r, ld, r, d2);
    v_axpby(ctx, n, 1.0, z, d2[1] / rz, p);
    rr = d2[0]; rz = d2[1];
    ++it;
  }
  return it;
}

// leading dimension of a Krylov basis: a multiple of 64 doubles plus an odd number of 256-byte lines, so that the
// K+1 streams of a fused multi-dot do not start on the same HBM channel
int64_t basis_ld(const ifem_ctx *ctx, int64_t n) { return ((n + 63) / 64) * 64 + ctx->tune.basis_pad; }

} // namespace ifem
