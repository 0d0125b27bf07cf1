// assemble_rows.hpp -- index arithmetic of the row-owner assembly of A_uu (assemble_rows.hip), host and device: nothing here touches the
// GPU, so a stand-alone program can include it (tests/test_assemble_rows_host.py).
//
// 3D Q2 velocity on a full lattice of 2 n_d + 1 points per axis (n_d cells).  OWNER (i, j, k), 0 <= i <= n_x and likewise j, k, owns the at
// most 8 lattice points (2i + d_x, 2j + d_y, 2k + d_z), d in {0, 1}^3, that exist: d_x = 1 needs i < n_x.  A point with d_d = 0 on an axis
// is a cell boundary there, touched by the cells i_d - 1 and i_d; with d_d = 1 it is the midpoint of cell i_d.  That gives
// 8 + 3 * 4 + 3 * 2 + 1 = 27 (row node, cell) PAIRS per owner, in an order that keeps the pairs of one node adjacent and fills the two
// 16-row tiles of the contraction as vertex (8) + x edge (4) + y edge (4) | z edge (4) + xy face (2) + xz face (2) + yz face (2) + interior (1).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define IFEM_ROWS_HD __host__ __device__
#else
#define IFEM_ROWS_HD
#endif

namespace ifem {
namespace rows {

constexpr int kPairs = 27;
constexpr int kNodeSeq[8] = {0, 1, 2, 4, 3, 5, 6, 7};          // node bits d_x | d_y << 1 | d_z << 2 in the order of their pairs
constexpr int kNodeFirst[9] = {0, 8, 12, 16, 20, 22, 24, 26, 27}; // first pair of the s-th node of that order

struct Pair {
  int nd; // the row node: d_x | d_y << 1 | d_z << 2
  int cb; // the cell: bit d set = the cell BELOW the node on axis d (i_d - 1), only where d_d = 0
  int a;  // local index of the node in that cell, a_x + 3 a_y + 9 a_z
};

IFEM_ROWS_HD constexpr Pair pair_of(int p) {
  int s = 0;
  while (p >= kNodeFirst[s + 1]) ++s;
  const int nd = kNodeSeq[s];
  int k = p - kNodeFirst[s], cb = 0;
  for (int d = 0; d < 3; ++d)
    if (!((nd >> d) & 1)) { cb |= (k & 1) << d; k >>= 1; }
  int a = 0, st = 1;
  for (int d = 0; d < 3; ++d, st *= 3) a += st * (((nd >> d) & 1) ? 1 : (((cb >> d) & 1) ? 2 : 0));
  return Pair{nd, cb, a};
}

IFEM_ROWS_HD inline int64_t n_owners(const int n[3]) { return int64_t(n[0] + 1) * (n[1] + 1) * (n[2] + 1); }
IFEM_ROWS_HD inline void owner_ijk(int64_t o, const int n[3], int ijk[3]) {
  ijk[0] = int(o % (n[0] + 1));
  ijk[1] = int((o / (n[0] + 1)) % (n[1] + 1));
  ijk[2] = int(o / (int64_t(n[0] + 1) * (n[1] + 1)));
}

// lattice point of the row node of a pair, x fastest over 2 n_d + 1 points per axis; -1: the owner has no such node
IFEM_ROWS_HD inline int64_t row_point(const int ijk[3], const int n[3], int nd) {
  int64_t at = 0, st = 1;
  for (int d = 0; d < 3; ++d) {
    const int x = 2 * ijk[d] + ((nd >> d) & 1);
    if (x > 2 * n[d]) return -1;
    at += st * x; st *= 2 * n[d] + 1;
  }
  return at;
}
// cell of a pair as i_x + n_x (i_y + n_y i_z); -1: outside the mesh (the node lies on a face of the domain, or does not exist)
IFEM_ROWS_HD inline int64_t pair_cell(const int ijk[3], const int n[3], const Pair &P) {
  int64_t at = 0, st = 1;
  for (int d = 0; d < 3; ++d) {
    const int c = ijk[d] - ((P.cb >> d) & 1);
    if (c < 0 || c >= n[d]) return -1;
    at += st * c; st *= n[d];
  }
  return at;
}
// The 5^3 lattice neighbourhood of an owner: point t = t_x + 5 t_y + 25 t_z is lattice point 2 i_d - 2 + t_d.  Every row node of the owner
// (t_d = 2 + d_d) and every column node of its pairs lies inside: column b = b_x + 3 b_y + 9 b_z of a pair's cell sits at t_d = 2 - 2 cb_d + b_d.
IFEM_ROWS_HD constexpr int nb_of_node(int nd) { return (2 + (nd & 1)) + 5 * (2 + ((nd >> 1) & 1)) + 25 * (2 + ((nd >> 2) & 1)); }
IFEM_ROWS_HD inline int nb_of_column(int cb, int b) {
  const int bx = b % 3, by = (b / 3) % 3, bz = b / 9;
  return (2 - 2 * (cb & 1) + bx) + 5 * (2 - 2 * ((cb >> 1) & 1) + by) + 25 * (2 - 2 * ((cb >> 2) & 1) + bz);
}
// lattice point of neighbourhood entry t; -1: outside the lattice
IFEM_ROWS_HD inline int64_t nb_point(const int ijk[3], const int n[3], int t) {
  const int td[3] = {t % 5, (t / 5) % 5, t / 25};
  int64_t at = 0, st = 1;
  for (int d = 0; d < 3; ++d) {
    const int x = 2 * ijk[d] - 2 + td[d];
    if (x < 0 || x > 2 * n[d]) return -1;
    at += st * x; st *= 2 * n[d] + 1;
  }
  return at;
}

} // namespace rows
} // namespace ifem
