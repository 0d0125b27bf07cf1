// refine.cpp -- see refine.hpp; FluidSolver<dim>::refine_mesh at the end.
#include "refine.hpp"
#include <algorithm>
#include <cmath>
#include <numeric>
#include "../../../include/ifem_hip.h"
#include "insim.hpp"

namespace ifem_host {

template <int dim>
void box_cells(const Triangulation<dim> &tria, const DoFTables<dim> &dofs, BoxCells &out) {
  if (!tria.is_box) throw std::invalid_argument("box_cells: box triangulations only");
  constexpr int NV = 1 << dim;
  const size_t nc = dofs.vcoords.size() / (size_t)(NV * dim);
  double half[3] = {1, 1, 1};
  out = BoxCells();
  for (int d = 0; d < dim; ++d) {
    half[d] = (tria.p1[d] - tria.p0[d]) / tria.reps[d] / 2;
    out.n_half[d] = 2 * tria.reps[d];
  }
  out.org.resize(nc);
  out.size.resize(nc);
  out.owner.assign((size_t)out.n_half[0] * out.n_half[1] * out.n_half[2], -1);
  for (size_t c = 0; c < nc; ++c) {
    const double *v = &dofs.vcoords[c * NV * dim];
    std::array<int, 3> o{0, 0, 0};
    int size = 0;
    for (int d = 0; d < dim; ++d) {
      o[d] = (int)std::llround((v[d] - tria.p0[d]) / half[d]);
      const int s = (int)std::llround((v[(NV - 1) * dim + d] - v[d]) / half[d]);
      if (d == 0) size = s;
      if (s != size || (s != 1 && s != 2) || o[d] < 0 || o[d] + s > out.n_half[d] || (s == 2 && o[d] % 2 != 0))
        throw std::invalid_argument("box_cells: a cell is neither a coarse cell of the box nor one of its children");
    }
    out.org[c] = o;
    out.size[c] = size;
    for (int k = 0; k < (dim == 3 ? size : 1); ++k)
      for (int j = 0; j < size; ++j)
        for (int i = 0; i < size; ++i) {
          int32_t &w = out.owner[((size_t)(o[2] + k) * out.n_half[1] + (o[1] + j)) * out.n_half[0] + (o[0] + i)];
          if (w >= 0) throw std::invalid_argument("box_cells: two cells overlap");
          w = (int32_t)c;
        }
  }
  for (int32_t w : out.owner)
    if (w < 0) throw std::invalid_argument("box_cells: the cells do not cover the box (a partitioned mesh?)");
  // active order: coarse cells x fastest, a refined one replaced by its children (x fastest)
  const size_t n_coarse = (size_t)tria.reps[0] * tria.reps[1] * tria.reps[2];
  std::vector<int32_t> first(n_coarse + 1, 0);
  for (size_t ci = 0; ci < n_coarse; ++ci) {
    const int i = int(ci % tria.reps[0]), j = int((ci / tria.reps[0]) % tria.reps[1]), k = int(ci / ((size_t)tria.reps[0] * tria.reps[1]));
    const int32_t w = out.owner[((size_t)(2 * k) * out.n_half[1] + 2 * j) * out.n_half[0] + 2 * i];
    first[ci + 1] = first[ci] + (out.size[(size_t)w] == 2 ? 1 : NV);
  }
  out.active_index.resize(nc);
  for (size_t c = 0; c < nc; ++c) {
    const auto &o = out.org[c];
    const size_t ci = ((size_t)(o[2] / 2) * tria.reps[1] + o[1] / 2) * tria.reps[0] + o[0] / 2;
    int child = 0;
    if (out.size[c] == 1)
      for (int d = 0; d < dim; ++d) child |= (o[d] & 1) << d;
    out.active_index[c] = first[ci] + child;
  }
}
template void box_cells<2>(const Triangulation<2> &, const DoFTables<2> &, BoxCells &);
template void box_cells<3>(const Triangulation<3> &, const DoFTables<3> &, BoxCells &);

template <int dim>
std::vector<int32_t> make_face_table(const Triangulation<dim> &tria, const DoFTables<dim> &dofs) {
  BoxCells B;
  box_cells<dim>(tria, dofs, B);
  constexpr int NS = 1 << (dim - 1), FS = 1 + NS, NF = 2 * dim;
  const size_t nc = B.org.size();
  std::vector<int32_t> tab(nc * NF * FS, -1);
  auto owner = [&](const int *p) { return B.owner[((size_t)p[2] * B.n_half[1] + p[1]) * B.n_half[0] + p[0]]; };
  for (size_t c = 0; c < nc; ++c)
    for (int f = 0; f < NF; ++f) {
      const int d = f >> 1, side = f & 1, size = B.size[c];
      int32_t *r = &tab[(c * NF + f) * FS];
      int p[3] = {B.org[c][0], B.org[c][1], B.org[c][2]};
      p[d] = side ? p[d] + size : p[d] - 1; // the half cell just behind the face, at the cell's lower corner
      if (p[d] < 0 || p[d] >= B.n_half[d]) { r[0] = IFEM_FACE_BOUNDARY; continue; }
      int tdir[2] = {0, 0}, nt = 0;
      for (int t = 0; t < dim; ++t) if (t != d) tdir[nt++] = t;
      const int32_t nb = owner(p);
      const int nsize = B.size[(size_t)nb];
      if (nsize == size) { r[0] = IFEM_FACE_EQUAL; r[1] = nb; }
      else if (nsize > size) { // which subface of the coarse cell's face this is
        int sub = 0;
        for (int t = 0; t < nt; ++t) sub |= (B.org[c][tdir[t]] - B.org[(size_t)nb][tdir[t]]) << t;
        r[0] = IFEM_FACE_COARSER | (sub << 8);
        r[1] = nb;
      } else {
        r[0] = IFEM_FACE_FINER;
        for (int s = 0; s < NS; ++s) {
          int q[3] = {p[0], p[1], p[2]};
          for (int t = 0; t < nt; ++t) q[tdir[t]] += (s >> t) & 1;
          r[1 + s] = owner(q);
        }
      }
    }
  return tab;
}
template std::vector<int32_t> make_face_table<2>(const Triangulation<2> &, const DoFTables<2> &);
template std::vector<int32_t> make_face_table<3>(const Triangulation<3> &, const DoFTables<3> &);

void mark_fixed_fraction(const std::vector<float> &criteria, double top, double bottom, std::vector<uint8_t> &refine,
                         std::vector<uint8_t> &coarsen) {
  // The rule (refine.hpp; the reference's refine_and_coarsen_fixed_fraction(0.6, 0.4) bisects a threshold inside p4est, which cannot be
  // restated bit for bit): total = sum eta_K; sort by eta descending, ties by ascending cell index; refine = the shortest prefix whose sum
  // reaches top * total; coarsen = the shortest suffix whose sum reaches bottom * total; a cell in both sets is refined; total = 0 flags nothing.
  const size_t n = criteria.size();
  refine.assign(n, 0);
  coarsen.assign(n, 0);
  double total = 0;
  for (float v : criteria) total += double(v);
  if (!(total > 0)) return;
  std::vector<size_t> order(n);
  std::iota(order.begin(), order.end(), size_t(0));
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return criteria[a] > criteria[b]; });
  double s = 0;
  for (size_t k = 0; k < n; ++k) {
    refine[order[k]] = 1;
    s += double(criteria[order[k]]);
    if (s >= top * total) break;
  }
  s = 0;
  for (size_t k = n; k-- > 0;) {
    coarsen[order[k]] = 1;
    s += double(criteria[order[k]]);
    if (s >= bottom * total) break;
  }
  for (size_t i = 0; i < n; ++i)
    if (refine[i]) coarsen[i] = 0;
}

template <int dim>
void apply_level_caps(const Triangulation<dim> &tria, int base_level, int min_level, int max_level, std::vector<uint8_t> &refine,
                      std::vector<uint8_t> &coarsen) {
  constexpr int NV = 1 << dim;
  const size_t n_coarse = tria.n_active_cells();
  const bool was = tria.locally_refined && tria.refine_flags.size() == n_coarse;
  if (refine.size() != tria.n_active_cells_with_children() || coarsen.size() != refine.size())
    throw std::invalid_argument("apply_level_caps: one flag per active cell");
  size_t a = 0;
  for (size_t c = 0; c < n_coarse; ++c) {
    const bool children = was && tria.refine_flags[c];
    const int level = base_level + (children ? 1 : 0);
    for (int k = 0; k < (children ? NV : 1); ++k, ++a) {
      if (level >= max_level) refine[a] = 0;  // (:433-441)
      if (level == min_level) coarsen[a] = 0; // (:442-447)
      if (children) refine[a] = 0;            // one level of local refinement
    }
  }
}
template void apply_level_caps<2>(const Triangulation<2> &, int, int, int, std::vector<uint8_t> &, std::vector<uint8_t> &);
template void apply_level_caps<3>(const Triangulation<3> &, int, int, int, std::vector<uint8_t> &, std::vector<uint8_t> &);

template <int dim>
void make_transfer_table(const Triangulation<dim> &box, const DoFTables<dim> &old, const DoFTables<dim> &fresh, TransferTable &out) {
  if (old.kv != fresh.kv) throw std::invalid_argument("make_transfer_table: the two meshes must share the velocity degree");
  BoxCells O, F;
  box_cells<dim>(box, old, O);
  box_cells<dim>(box, fresh, F);
  constexpr int NV = 1 << dim;
  out.u_cell.assign((size_t)fresh.n_unodes, -1); out.u_pos.assign((size_t)fresh.n_unodes, 0);
  out.p_cell.assign((size_t)fresh.n_pnodes, -1); out.p_pos.assign((size_t)fresh.n_pnodes, 0);
  const size_t nc = F.org.size();
  for (int space = 0; space < 2; ++space) {
    const int deg = space == 0 ? fresh.kv : 1, n1 = deg + 1, nn = space == 0 ? fresh.nu : NV;
    const std::vector<int32_t> &cell_nodes = space == 0 ? fresh.cell_unodes : fresh.cell_pnodes;
    std::vector<int32_t> &t_cell = space == 0 ? out.u_cell : out.p_cell, &t_pos = space == 0 ? out.u_pos : out.p_pos;
    for (size_t c = 0; c < nc; ++c)
      for (int a = 0; a < nn; ++a) {
        const int32_t nd = cell_nodes[c * nn + a];
        if (t_cell[(size_t)nd] >= 0) continue; // (the answer depends on the node alone)
        int l[3] = {a % n1, (a / n1) % n1, a / (n1 * n1)}, key[3] = {0, 0, 0}, lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        for (int d = 0; d < dim; ++d) { // node on the lattice of deg units per half cell; half cells whose closure holds it
          key[d] = F.org[c][d] * deg + l[d] * F.size[c];
          lo[d] = std::max((key[d] + deg - 1) / deg - 1, 0);
          hi[d] = std::min(key[d] / deg, O.n_half[d] - 1);
        }
        int32_t best = -1;
        for (int k = lo[2]; k <= hi[2]; ++k)
          for (int j = lo[1]; j <= hi[1]; ++j)
            for (int i = lo[0]; i <= hi[0]; ++i) {
              const int32_t w = O.owner[((size_t)k * O.n_half[1] + j) * O.n_half[0] + i];
              if (best < 0 || w < best) best = w;
            }
        int pos = 0;
        for (int d = 0; d < dim; ++d) {
          const int u = key[d] - O.org[(size_t)best][d] * deg; // 0 ... size * deg
          pos |= (O.size[(size_t)best] == 2 ? u : 2 * u) << (8 * d);
        }
        t_cell[(size_t)nd] = best;
        t_pos[(size_t)nd] = pos;
      }
  }
}
template void make_transfer_table<2>(const Triangulation<2> &, const DoFTables<2> &, const DoFTables<2> &, TransferTable &);
template void make_transfer_table<3>(const Triangulation<3> &, const DoFTables<3> &, const DoFTables<3> &, TransferTable &);

namespace Fluid {
namespace MPI {

// FluidSolver::refine_mesh (mpi_fluid_solver.cpp:416-488): estimator, marking, caps, re-flag, setup_dofs / make_constraints /
// initialize_system on the new mesh, transfer of present_solution.  The old context stays alive until the transfer has read it.
template <int dim>
void FluidSolver<dim>::refine_mesh(const unsigned int min_grid_level, const unsigned int max_grid_level) {
  if (const char *why = refine_mesh_refusal()) throw std::runtime_error(std::string("refine_mesh: ") + why);
  if (!ctx) throw std::runtime_error("refine_mesh: initialize_system first");
  RefineReport &R = last_refine;
  R = RefineReport();
  // 1. KellyErrorEstimator on the velocity of present_solution (:422-430), on the device
  BoxCells cells;
  box_cells<dim>(triangulation, dofs, cells);
  const std::vector<int32_t> faces = make_face_table<dim>(triangulation, dofs);
  const size_t n_active = cells.org.size();
  std::vector<double> eta(n_active);
  check(ifem_kelly_estimate(ctx, IFEM_VEC_PRESENT, faces.data(), eta.data(), nullptr), "refine_mesh");
  R.indicators.assign(n_active, 0.0);
  std::vector<float> criteria(n_active); // Vector<float> estimated_error_per_cell, in the order of the active cells
  for (size_t c = 0; c < n_active; ++c) {
    R.indicators[(size_t)cells.active_index[c]] = eta[c];
    criteria[(size_t)cells.active_index[c]] = float(eta[c]);
  }
  // 2. refine_and_coarsen_fixed_fraction(0.6, 0.4) (:431-432) and the level caps (:433-447)
  mark_fixed_fraction(criteria, 0.6, 0.4, R.refine_flags, R.coarsen_flags);
  apply_level_caps<dim>(triangulation, (int)parameters.global_refinements[0], (int)min_grid_level, (int)max_grid_level, R.refine_flags, R.coarsen_flags);
  // 3. prepare_ / execute_coarsening_and_refinement (:454,468)
  const std::vector<uint8_t> before = triangulation.locally_refined ? triangulation.refine_flags : std::vector<uint8_t>(triangulation.n_active_cells(), 0);
  triangulation.set_active_flags(R.refine_flags, R.coarsen_flags);
  triangulation.execute_coarsening_and_refinement();
  const std::vector<uint8_t> after = triangulation.locally_refined ? triangulation.refine_flags : std::vector<uint8_t>(triangulation.n_active_cells(), 0);
  for (size_t c = 0; c < before.size(); ++c) {
    R.n_refined += (!before[c] && after[c]) ? 1 : 0;
    R.n_coarsened += (before[c] && !after[c]) ? 1 : 0;
  }
  R.n_active_cells = (int64_t)triangulation.n_active_cells_with_children();
  R.changed = before != after;
  if (pcout)
    *pcout << "Refine mesh" << std::endl
           << "   Refined cells: " << R.n_refined << ", coarsened parents: " << R.n_coarsened << ", active cells: " << R.n_active_cells << std::endl;
  if (!R.changed) return; // the same mesh: the context stays as it is
  // 4.-6. setup_dofs, make_constraints, initialize_system (:471-473) beside the old context
  struct OldContext { // destroyed after the transfer, or when something on the way throws
    ifem_ctx *c;
    ~OldContext() { if (c) ifem_ctx_destroy(c); }
  } old{ctx};
  const DoFTables<dim> old_dofs = dofs;
  mg_coarse.reset(); // the levels borrow the old context's stream: they go first
  mg_tria.reset();
  ctx = nullptr;
  setup_dofs();
  make_constraints();
  initialize_system();
  // 7. trans.interpolate (:477-481); no constraints.distribute afterwards, as in the reference
  TransferTable T;
  make_transfer_table<dim>(triangulation, old_dofs, dofs, T);
  check(ifem_transfer_solution(old.c, ctx, IFEM_VEC_PRESENT, T.u_cell.data(), T.u_pos.data(), T.p_cell.data(), T.p_pos.data()), "refine_mesh");
}

// what keeps the refusal: the message of the case, or nullptr when this solver refines
template <int dim>
const char *FluidSolver<dim>::refine_mesh_refusal() const {
  if (!triangulation.is_box) return "the triangulation is not a box (subdivided_hyper_rectangle)";
  if (proc_grid[0] * proc_grid[1] * proc_grid[2] > 1) return "the solver is partitioned over several ranks";
  if (turbulence_model) return "a turbulence model is attached (the Spalart-Allmaras entry points refuse hanging nodes)";
  return nullptr;
}

template void FluidSolver<2>::refine_mesh(const unsigned int, const unsigned int);
template void FluidSolver<3>::refine_mesh(const unsigned int, const unsigned int);
template const char *FluidSolver<2>::refine_mesh_refusal() const;
template const char *FluidSolver<3>::refine_mesh_refusal() const;

} // namespace MPI
} // namespace Fluid
} // namespace ifem_host
