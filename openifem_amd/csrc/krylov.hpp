// krylov.hpp -- what solver.hip needs of the Krylov drivers in krylov.hip, and the storage of their bases
#pragma once
#include <algorithm>
#include <functional>
#include <vector>
#include "ctx.hpp"
#include "kernels.hpp"

namespace ifem {

using OpFn = std::function<void(const double *, double *)>;
using MdotFn = std::function<void(int, const double *, int64_t, const double *, double *)>; // out[i] = <V_i, w>, i < k, columns ld apart
using OpF32 = std::function<void(const float *, double *)>;
using OpF32F32 = std::function<void(const float *, float *)>;

// LEFT preconditioning of gmres() (not flexible): the Krylov space of P^-1 A, the stopping test reads the PRECONDITIONED residual --
// deal.II's SolverGMRES with its defaults (mpi_supg_solver.cpp:176-182)
struct LeftPrecond {
  double *stage = nullptr;  // every new basis vector is also written here and the operators read IT, so that
  const OpFn *PA = nullptr; // ... the fused w = P^-1 A stage (a sequence with constant kernel arguments: a hipGraph) can replace the pair
};

// the drivers (krylov.hip); gmres: `history` gets the residual norm after every iteration, `ensure` grows the bases with the iteration count (basis_grower)
int gmres(ifem_ctx *ctx, int64_t n, int64_t ld, bool reorth, const OpFn &A, const OpFn &Pinv, bool flexible, const double *b, double *x, int m, int maxit,
          double tol, double *V, double *Z, double *w, double *res_out, const MdotFn &mdot, std::vector<double> *history = nullptr,
          const std::function<void(int, double *&, double *&)> *ensure = nullptr, const LeftPrecond *left_pc = nullptr);
int gmres_f32basis(ifem_ctx *ctx, int64_t n, int64_t ld, const OpFn &A, const OpF32 &Pinv, const double *b, double *x, int m, int maxit, double tol, float *V,
                   double *z, double *w, double *res_out, const std::function<void(double *, int)> &allreduce);
int fgmres_f32(ifem_ctx *ctx, int64_t n, int64_t ld, const OpFn &A, const OpF32 &Af, const OpF32F32 &Pinv, const double *b, double *x, int m, int maxit,
               double tol, float *V, float *Z, double *w, double *res_out, const std::function<void(double *, int)> &allreduce,
               const std::function<void(int, float *&, float *&)> &ensure);
int cg(ifem_ctx *ctx, int64_t n, const OpFn &A, const double *b, double *x, double tol, int maxit, double *r, double *p, double *q,
       const std::function<double(const double *, const double *)> &dot);
int cg_device(ifem_ctx *ctx, int64_t n, const OpFn &A, const double *diag, const double *b, double *x, double tol, int maxit, double *r, double *z, double *p,
              double *q, int chk, double *s = nullptr);
int pcg_jacobi(ifem_ctx *ctx, int64_t n, const OpFn &A, const double *diag, const double *b, double *x, double tol, int maxit, double *r, int64_t ld, double *p,
               double *q, const MdotFn &mdot);
int64_t basis_ld(const ifem_ctx *ctx, int64_t n); // leading dimension of a Krylov basis over n entries

// Krylov bases of the flexible solvers grow with the iteration count instead of being sized for the restart length: FGMRES(30) at
// 128^3 would hold 61 vectors of 425 MB where the bench's solves use 2 to 14.  Contents are kept; new columns are zero.
// max_cols: the most columns the solver can ever ask for (restart length + 1): growth never goes beyond it (rounded up to the
// multiple of 4 the fused kernels read), so FGMRES(30) ends at 32 columns, not at 36
template <typename T>
void grow_basis(ifem_ctx *c, DBuf<T> &B, int64_t ld, int64_t cols, int64_t max_cols) {
  const int64_t have = ld > 0 ? int64_t(B.n) / ld : 0;
  if (have >= cols || ld <= 0) return;
  const int64_t cap = std::max<int64_t>((std::max(max_cols, cols) + 3) / 4 * 4, cols);
  const int64_t want = std::min(cap, std::max<int64_t>((cols + 7) / 8 * 8, have + have / 2));
  DBuf<T> nb;
  nb.alloc(size_t(want) * size_t(ld));
  if (have > 0) IFEM_HIP_CHECK(hipMemcpyAsync(nb.p, B.p, size_t(have) * size_t(ld) * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
  IFEM_HIP_CHECK(hipMemsetAsync(nb.p + size_t(have) * size_t(ld), 0, size_t(want - have) * size_t(ld) * sizeof(T), c->stream));
  IFEM_HIP_CHECK(hipStreamSynchronize(c->stream));
  B.swap(nb);
}
// the callback gmres() gets for the pair (V: up to max_v columns, Z: up to max_v - 1)
template <typename T>
std::function<void(int, T *&, T *&)> basis_grower(ifem_ctx *c, DBuf<T> &Vb, DBuf<T> &Zb, int64_t ld, int max_v) {
  return [c, &Vb, &Zb, ld, max_v](int cols, T *&V, T *&Z) {
    grow_basis(c, Vb, ld, std::min(cols, max_v), max_v);
    grow_basis(c, Zb, ld, std::min(cols - 1, max_v - 1), max_v - 1);
    V = Vb.p; Z = Zb.p;
  };
}
constexpr int kBasisStart = 8; // columns a basis starts with

} // namespace ifem
