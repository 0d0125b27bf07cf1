// refine.hpp -- the host side of FluidSolver::refine_mesh (source/mpi_fluid_solver.cpp:416-488) on box triangulations with at most one
// level of local refinement: the face table of the error estimator (ifem_kelly_estimate), the marking rule standing in for
// parallel::distributed::GridRefinement::refine_and_coarsen_fixed_fraction, the level caps, and the table of the solution transfer
// (ifem_transfer_solution).  Nothing here needs a device.
#pragma once
#include <array>
#include <cstdint>
#include <vector>
#include "grid.hpp"

namespace ifem_host {

// The cells of a DoFTables of a box triangulation on the half-cell lattice (one coarse cell = 2 units per direction): origin and
// size (2: coarse cell, 1: child), read off vcoords -- whatever order the tables keep their cells in (Morton on a uniform box) -- and
// the position of every cell among the ACTIVE cells of the triangulation (coarse cells x fastest, children in place).
struct BoxCells {
  std::vector<std::array<int, 3>> org;
  std::vector<int> size;
  std::vector<int32_t> active_index; // [cell of the tables] -> active cell of the triangulation
  std::vector<int32_t> owner;        // [half-cell lattice, x fastest] -> cell of the tables
  std::array<int, 3> n_half{1, 1, 1};
};
template <int dim>
void box_cells(const Triangulation<dim> &tria, const DoFTables<dim> &dofs, BoxCells &out);

// int32 [n_cells][2 dim][1 + 2^(dim-1)] in the layout of ifem_hip.h (ifem_kelly_estimate): boundary, equal neighbour, coarser neighbour
// plus the subface this face is of its face, or the 2^(dim-1) finer neighbours in tangential-lexicographic order
template <int dim>
std::vector<int32_t> make_face_table(const Triangulation<dim> &tria, const DoFTables<dim> &dofs);

// Marking rule on the indicators ROUNDED TO float (the reference keeps them in a Vector<float>, mpi_fluid_solver.cpp:422).  The
// reference calls p4est's refine_and_coarsen_fixed_fraction(0.6, 0.4), whose threshold bisection cannot be restated bit for bit; this
// is the rule it approximates, and the rule of this project:
//   total = sum of eta_K (double accumulation of the float values, in cell order);
//   sort by eta descending, ties by ascending cell index;
//   the refine set is the shortest prefix whose sum reaches top * total, the coarsen set the shortest suffix whose sum reaches
//   bottom * total (running sums in double, in sorted order from the respective end; "reaches": sum >= fraction * total);
//   a cell in both sets is refined; total = 0 flags nothing.
void mark_fixed_fraction(const std::vector<float> &criteria, double top, double bottom, std::vector<uint8_t> &refine,
                         std::vector<uint8_t> &coarsen);

// The caps of mpi_fluid_solver.cpp:433-447 on flags per ACTIVE cell: coarse box cells count as level `base_level`
// (global_refinements[0]), their children as one more.  Refine flags go on cells of level >= max_level, coarsen flags on cells of
// level min_level, and -- the mirror's own cap, one level of local refinement -- refine flags go on children.
template <int dim>
void apply_level_caps(const Triangulation<dim> &tria, int base_level, int min_level, int max_level, std::vector<uint8_t> &refine,
                      std::vector<uint8_t> &coarsen);

// per node of `fresh`: the cell of `old` whose closure holds it (lowest cell index) and its position there in units of 1 / (2 deg),
// packed x | y << 8 | z << 16 (ifem_hip.h, ifem_transfer_solution); both tables belong to the same box
struct TransferTable {
  std::vector<int32_t> u_cell, u_pos, p_cell, p_pos;
};
template <int dim>
void make_transfer_table(const Triangulation<dim> &box, const DoFTables<dim> &old, const DoFTables<dim> &fresh, TransferTable &out);

} // namespace ifem_host
