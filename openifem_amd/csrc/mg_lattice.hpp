// The velocity transfers of the A_uu V-cycle between two uniform box levels as a closed formula (mg_lattice.hip; checked by
// tests/cpp/mg_lattice_check.cpp on the host).  Both levels hold their Q2 velocity nodes as full lattices (ctx.hpp::ULattice); per axis the pair
// either keeps the axis (n_f == n_c: weight 1 at the same index) or halves its cells (n_f == 2 n_c - 1).  On a halved axis the coarse cell K
// spans the coarse points 2K, 2K + 1, 2K + 2 and the fine points 4K .. 4K + 4; the quadratic Lagrange polynomials through the coarse points,
// taken at the quarter points t / 4, are
//     t = 0 (1, 0, 0)    t = 1 (3/8, 3/4, -1/8)    t = 2 (0, 1, 0)    t = 3 (-1/8, 3/4, 3/8)    t = 4 (0, 0, 1)
// A row of P or R is the tensor product over the axes: products of exact dyadic rationals, formed in double.  Terms are addressed by a slot
// number so that a kernel can walk them without keeping a table: a slot either holds a term (true) or nothing (false).
#ifndef IFEM_MG_LATTICE_HPP
#define IFEM_MG_LATTICE_HPP

#if defined(__HIPCC__)
#define IFEM_MGL_HD __host__ __device__
#else
#define IFEM_MGL_HD
#endif

namespace ifem {

enum { kMglProlongSlots = 3, kMglRestrictSlots = 5 };

// slots an axis uses: the loops of a row run over mgl_slots(...) per axis
IFEM_MGL_HD inline int mgl_prolong_slots(bool halved) { return halved ? kMglProlongSlots : 1; }
IFEM_MGL_HD inline int mgl_restrict_slots(bool halved) { return halved ? kMglRestrictSlots : 1; }

// prolongation along one axis, fine index i, slot k: coarse index j and weight w.  n_c: coarse points of the axis (2 cells_c + 1 when halved).
// A zero weight is no term.
IFEM_MGL_HD inline bool mgl_prolong_term(bool halved, int n_c, int i, int k, int &j, double &w) {
  if (!halved) { j = i; w = 1.0; return k == 0; }
  const int cells_c = (n_c - 1) / 2;
  int K = i >> 2;
  if (K > cells_c - 1) K = cells_c - 1; // the last fine point belongs to the last coarse cell
  const int t = i - 4 * K;              // 0 .. 4
  j = 2 * K + k;
  if (!(t & 1)) { w = 1.0; return 2 * k == t; }
  if (k == 1) w = 0.75;
  else w = ((k == 0) == (t == 1)) ? 0.375 : -0.125;
  return true;
}

// restriction along one axis (the transpose), coarse index j, slot k: fine index i and weight w.  n_f: fine points of the axis.
//   j odd  (a coarse cell's mid point): fine 2j - 1, 2j, 2j + 1 with 3/4, 1, 3/4
//   j even (a coarse cell's end point): fine 2j - 3, 2j - 1, 2j, 2j + 1, 2j + 3 with -1/8, 3/8, 1, 3/8, -1/8
// fine indices outside [0, n_f) are no terms
IFEM_MGL_HD inline bool mgl_restrict_term(bool halved, int n_f, int j, int k, int &i, double &w) {
  if (!halved) { i = j; w = 1.0; return k == 0; }
  if (j & 1) {
    i = 2 * j - 1 + k;
    w = k == 1 ? 1.0 : 0.75;
    if (k > 2) return false;
  } else {
    const int off = k < 2 ? 2 * k - 3 : (k == 2 ? 0 : 2 * k - 5); // -3, -1, 0, 1, 3
    i = 2 * j + off;
    w = k == 2 ? 1.0 : ((k == 1 || k == 3) ? 0.375 : -0.125);
  }
  return i >= 0 && i < n_f;
}

// terms of a whole 1D row (the entry-by-entry check compares this with the CSR row length)
IFEM_MGL_HD inline int mgl_prolong_count(bool halved, int n_c, int i) {
  int n = 0, j; double w;
  for (int k = 0; k < mgl_prolong_slots(halved); ++k) n += mgl_prolong_term(halved, n_c, i, k, j, w) ? 1 : 0;
  return n;
}
IFEM_MGL_HD inline int mgl_restrict_count(bool halved, int n_f, int j) {
  int n = 0, i; double w;
  for (int k = 0; k < mgl_restrict_slots(halved); ++k) n += mgl_restrict_term(halved, n_f, j, k, i, w) ? 1 : 0;
  return n;
}

// the fine point a coarse point coincides with (the injection of the evaluation point)
IFEM_MGL_HD inline int mgl_inject_index(bool halved, int j) { return halved ? 2 * j : j; }

} // namespace ifem
#endif
