// lattice.hpp -- the pressure and velocity nodes of a uniform box level as full lattices (plain C++, no device call: lattice.cpp).
#pragma once
#include <cstdint>
#include <vector>

namespace ifem {

constexpr int kLatticeMaxLine = 65536; // nodes per axis (the 32-bit position along a line, the per-axis tables of the readers)

// node_of_lattice [n[0] n[1] n[2]] (point i_x + n[0] (i_y + n[1] i_z) -> node) and its inverse lattice_of_node [n_nodes] from the cell tables
// (vc [nc][2^dim][dim], cp [nc][2^dim]) of a level whose cells all have the edges h; false: the nodes are not the full lattice of a uniform
// box (holes, L-shapes, duplicate nodes, a vertex off its lattice point by more than 8 eps max|x|, more than kLatticeMaxLine nodes on an axis
// or 2^31 nodes).  The outputs are unspecified then.
bool lattice_map(int dim, int64_t nc, int64_t n_nodes, const double *vc, const int32_t *cp, const double *h, int n[3],
                 std::vector<int32_t> &node_of_lattice, std::vector<int32_t> &lattice_of_node);

// The same for the velocity nodes of degree deg (1 or 2; cu [nc][(deg + 1)^dim], local index x fastest): the lattice point of local node t
// of cell (c_x, c_y, c_z) is deg c + t per axis, n[d] = deg cells_d + 1, so pressure point j sits at velocity point deg j.  Refuses the same
// inputs, and a cell whose vertices are not its own box of edges h.
bool lattice_map_u(int dim, int deg, int64_t nc, int64_t n_nodes, const double *vc, const int32_t *cu, const double *h, int n[3],
                   std::vector<int32_t> &node_of_lattice, std::vector<int32_t> &lattice_of_node);

// Position signature of point i on an axis of n nodes: (min(i, 2), min(n - 1 - i, 2)) as one code 3 a + b, and the compact numbering of the
// codes that occur on the axis in the order of their first point: cls [n] (compact id of every point), first [ids] (first point of every
// id).  Returns the number of ids (at most 5; fewer than 5 nodes: one id per node).
int lattice_axis_classes(int n, std::vector<uint8_t> &cls, std::vector<int32_t> &first);

// The signature of a velocity point, whose B^T row couples the pressure points j with |i - deg j| <= deg: (min(i, 2 deg), min(n - 1 - i, 2 deg))
// and, where both distances are capped, i mod deg.  Same outputs (at most 4 deg + 2 ids per axis).
int lattice_axis_classes_u(int n, int deg, std::vector<uint8_t> &cls, std::vector<int32_t> &first);

} // namespace ifem
