// turbulence.cpp -- host mirror of Fluid::MPI::SpalartAllmaras<dim> (source/mpi_spalart_allmaras.cpp) over the ifem_sa_* entry points.
#include "turbulence.hpp"
#include <algorithm>
#include <iomanip>
#include <map>
#include "insim.hpp"

namespace ifem_host {
namespace Fluid {
namespace MPI {

template <int dim>
TurbulenceModel<dim> *TurbulenceModel<dim>::create(FluidSolver<dim> &fluid, const std::string &model_name) {
  if (model_name == "Spalart-Allmaras") return new SpalartAllmaras<dim>(fluid);
  throw std::logic_error("ExcNotImplemented: turbulence model '" + model_name + "' (available: Spalart-Allmaras)");
}

namespace {
// local nodes of face f = 2 d + side of a Q_kv cell (lexicographic, x fastest)
template <int dim, class F>
void for_face_nodes(int kv, int f, F fn) {
  const int n1 = kv + 1, d = f / 2, side = f % 2;
  int nu = 1;
  for (int k = 0; k < dim; ++k) nu *= n1;
  for (int a = 0; a < nu; ++a) {
    int r = a;
    for (int k = 0; k < d; ++k) r /= n1;
    if (r % n1 == (side ? kv : 0)) fn(a);
  }
}
} // namespace

// The wall points must be those of the WHOLE mesh on every rank (the reference all-reduces them, :478-491) and a partitioned solver only
// holds its own cells: rather than compute a wall distance from a rank's share, the mirror refuses.  (The device entry points themselves
// take partitioned contexts: a caller that has all wall points passes them to every rank.)
template <int dim>
void SpalartAllmaras<dim>::refuse_partitioned() const {
  if (fluid.proc_grid[0] * fluid.proc_grid[1] * fluid.proc_grid[2] > 1)
    throw std::invalid_argument("SpalartAllmaras: a partitioned fluid solver (set_partition with more than one rank) is not supported by the host mirror "
                                "of the turbulence model: the wall points of the whole mesh are not gathered");
}

template <int dim>
void SpalartAllmaras<dim>::make_constraints() {
  refuse_partitioned();
  const auto &dofs = fluid.dofs;
  const auto &par = fluid.parameters;
  const size_t n_cells = dofs.cell_unodes.size() / dofs.nu;
  std::vector<uint8_t> seen((size_t)dofs.n_unodes, 0);
  nodes.clear(); values.clear();
  for (const auto &bc : par.spalart_allmaras_model_bcs) { // std::map: ascending boundary id (:367-402)
    double augmented_value = 0.0;
    if (bc.second == 1) augmented_value = 5.0 * par.viscosity / par.fluid_rho;
    else if (bc.second != 0) throw std::invalid_argument("Unrecogonized Spalart-Allmaras BC type!");
    for (size_t c = 0; c < n_cells; ++c)
      for (int f = 0; f < 2 * dim; ++f) {
        if (dofs.cell_face_bid[c * 2 * dim + f] != (int32_t)bc.first) continue;
        for_face_nodes<dim>(dofs.kv, f, [&](int a) {
          const int32_t nd = dofs.cell_unodes[c * dofs.nu + a];
          if (seen[nd]) return;
          seen[nd] = 1;
          nodes.push_back(nd); values.push_back(augmented_value);
        });
      }
  }
  if (fluid.ctx) {
    fluid.check(ifem_sa_set_constraints(fluid.ctx, 1, (int32_t)nodes.size(), nodes.data(), values.data()), "SpalartAllmaras::make_constraints");
    fluid.check(ifem_sa_set_constraints(fluid.ctx, 0, (int32_t)nodes.size(), nodes.data(), nullptr), "SpalartAllmaras::make_constraints");
  }
}

template <int dim>
void SpalartAllmaras<dim>::initialize_system() {
  refuse_partitioned();
  const auto &dofs = fluid.dofs;
  const auto &par = fluid.parameters;
  constexpr int NV = 1 << dim;
  const size_t n_cells = dofs.cell_unodes.size() / dofs.nu;
  // setup_cell_property (:436-477): the distinct vertices of the boundary faces whose S-A type is 0
  std::map<int32_t, std::array<double, dim>> boundary_points;
  for (size_t c = 0; c < n_cells; ++c)
    for (int f = 0; f < 2 * dim; ++f) {
      const int32_t bid = dofs.cell_face_bid[c * 2 * dim + f];
      if (bid < 0) continue;
      const auto bc = par.spalart_allmaras_model_bcs.find((unsigned)bid);
      if (bc == par.spalart_allmaras_model_bcs.end() || bc->second != 0) continue;
      const int d = f / 2, side = f % 2;
      for (int v = 0; v < NV; ++v) {
        if (((v >> d) & 1) != side) continue;
        int a = 0, stride = 1;
        for (int k = 0; k < dim; ++k) { a += ((v >> k) & 1) * dofs.kv * stride; stride *= dofs.kv + 1; }
        std::array<double, dim> x;
        for (int k = 0; k < dim; ++k) x[k] = dofs.vcoords[(c * NV + v) * dim + k];
        boundary_points.insert({dofs.cell_unodes[c * dofs.nu + a], x});
      }
    }
  wall.clear();
  for (const auto &p : boundary_points)
    for (int k = 0; k < dim; ++k) wall.push_back(p.second[k]);
  if (nodes.empty() && !par.spalart_allmaras_model_bcs.empty()) make_constraints();
  fluid.check(ifem_sa_set_constraints(fluid.ctx, 1, (int32_t)nodes.size(), nodes.data(), values.data()), "SpalartAllmaras::initialize_system");
  fluid.check(ifem_sa_set_constraints(fluid.ctx, 0, (int32_t)nodes.size(), nodes.data(), nullptr), "SpalartAllmaras::initialize_system");
  // the initial condition (:561-565): coefficient x laminar kinematic viscosity, zero_constraints.distribute
  std::vector<double> nu((size_t)dofs.n_unodes, par.spalart_allmaras_initial_condition_coefficient * par.viscosity / par.fluid_rho);
  for (int32_t nd : nodes) nu[nd] = 0.0;
  fluid.check(ifem_sa_vec_set(fluid.ctx, IFEM_SA_PRESENT, nu.data()), "SpalartAllmaras::initialize_system");
  fluid.check(ifem_sa_set_wall_points(fluid.ctx, (int64_t)(wall.size() / dim), wall.data()), "SpalartAllmaras::setup_cell_property");
  eddy_viscosity.assign((size_t)dofs.n_unodes, 0.0); // zero until the first step, as the reference's vector
}

template <int dim>
void SpalartAllmaras<dim>::run_one_step(bool apply_nonzero_constraints) {
  const auto &par = fluid.parameters;
  if (fluid.pcout) *fluid.pcout << std::string(96, '*') << std::endl << "Solving for S-A turbulence model..." << std::endl;
  const ifem_sa_params p{par.viscosity, par.fluid_rho, fluid.time.get_delta_t()};
  std::vector<double> log((size_t)4 * (par.fluid_max_iterations + 1), 0.0);
  const int rc = ifem_sa_newton_step(fluid.ctx, &p, apply_nonzero_constraints, par.fluid_tolerance, (int)par.fluid_max_iterations, log.data());
  if (rc < 0) throw SolverFailure(rc, std::string("SpalartAllmaras::run_one_step: ") + ifem_last_error());
  last_newton_iterations = (unsigned)rc;
  // the step ended with update_eddy_viscosity (:344) on the device; the mirror keeps the host copy the reference's get_eddy_viscosity returns
  eddy_viscosity.resize((size_t)fluid.dofs.n_unodes);
  fluid.check(ifem_sa_update_eddy_viscosity(fluid.ctx, &p, eddy_viscosity.data()), "SpalartAllmaras::update_eddy_viscosity");
  if (fluid.pcout)
    for (int it = 0; it < rc; ++it)
      *fluid.pcout << std::scientific << std::left << " ITR = " << std::setw(2) << it << " ABS_RES = " << log[it * 4] << " REL_RES = " << log[it * 4 + 1]
                   << " GMRES_ITR = " << std::setw(3) << (unsigned)log[it * 4 + 2] << " GMRES_RES = " << log[it * 4 + 3] << std::endl;
}

template <int dim>
void SpalartAllmaras<dim>::connect_indicator_field(const std::vector<int32_t> &indicator) {
  if (!indicator.empty()) {
    if (indicator.size() != fluid.dofs.cell_unodes.size() / fluid.dofs.nu) throw std::invalid_argument("connect_indicator_field: one entry per cell");
    fluid.check(ifem_set_cell_fields(fluid.ctx, indicator.data()), "SpalartAllmaras::connect_indicator_field");
  }
  has_indicator = true;
}

template <int dim>
void SpalartAllmaras<dim>::update_moving_wall_distance(const ifem_fsi_solid &solid, const ifem_sa_wall &w, const std::vector<double> &shear_velocities) {
  refuse_partitioned();
  if (w.n_vertices <= 0 || !w.vertex || !w.normal || (int64_t)shear_velocities.size() != w.n_vertices)
    throw std::invalid_argument("update_moving_wall_distance: wall vertices, normals and one shear velocity per wall vertex");
  fluid.check(ifem_fsi_set_solid(fluid.ctx, &solid), "SpalartAllmaras::update_moving_wall_distance");
  const std::vector<int32_t> v(w.vertex, w.vertex + w.n_vertices), e(w.edge ? w.edge : nullptr, w.edge ? w.edge + 2 * (size_t)w.n_edges : nullptr);
  const std::vector<double> nrm(w.normal, w.normal + (size_t)w.n_vertices * dim);
  const double key[3] = {w.image_distance, w.wall_function_distance, double(w.sample_at_image_point != 0)};
  if (v != wall_vertex || e != wall_edge || nrm != wall_normal || !std::equal(key, key + 3, wall_key)) {
    fluid.check(ifem_sa_set_moving_wall(fluid.ctx, &w), "SpalartAllmaras::update_moving_wall_distance");
    wall_vertex = v; wall_edge = e; wall_normal = nrm;
    std::copy(key, key + 3, wall_key);
  }
  const auto &par = fluid.parameters;
  const ifem_sa_params p{par.viscosity, par.fluid_rho, fluid.time.get_delta_t()};
  fluid.check(ifem_sa_set_shear_velocities(fluid.ctx, shear_velocities.data()), "SpalartAllmaras::update_moving_wall_distance");
  fluid.check(ifem_sa_update_moving_wall_distance(fluid.ctx, &p, nullptr, nullptr), "SpalartAllmaras::update_moving_wall_distance");
}

template <int dim>
void SpalartAllmaras<dim>::update_boundary_condition(bool first_step) {
  refuse_partitioned();
  if (!has_indicator) throw std::logic_error("No available indicator function for SA model!");
  const auto &par = fluid.parameters;
  const ifem_sa_params p{par.viscosity, par.fluid_rho, fluid.time.get_delta_t()};
  fluid.check(ifem_sa_update_boundary_condition(fluid.ctx, &p, first_step, nullptr, &last_boundary_lines), "SpalartAllmaras::update_boundary_condition");
  // the lines of nonzero_constraints after the merge, as constraint_nodes() / constraint_values() report them
  const size_t n = (size_t)fluid.dofs.n_unodes;
  std::vector<uint8_t> flags(n);
  std::vector<double> inhom(n);
  fluid.check(ifem_sa_get_constraints(fluid.ctx, 1, flags.data(), inhom.data()), "SpalartAllmaras::update_boundary_condition");
  nodes.clear(); values.clear();
  for (size_t i = 0; i < n; ++i)
    if (flags[i]) { nodes.push_back((int32_t)i); values.push_back(inhom[i]); }
}

template <int dim>
double SpalartAllmaras<dim>::get_shear_velocity(double vel, double init_guess) {
  const auto &par = fluid.parameters;
  const ifem_sa_params p{par.viscosity, par.fluid_rho, fluid.time.get_delta_t()};
  double out = 0;
  fluid.check(ifem_sa_get_shear_velocity(&p, par.spalart_allmaras_image_distance, vel, init_guess, &out), "SpalartAllmaras::get_shear_velocity");
  return out;
}

template <int dim>
std::vector<double> SpalartAllmaras<dim>::get_present_solution() const {
  std::vector<double> x((size_t)fluid.dofs.n_unodes);
  fluid.check(ifem_sa_vec_get(fluid.ctx, IFEM_SA_PRESENT, x.data()), "SpalartAllmaras::get_present_solution");
  return x;
}

template <int dim>
std::vector<double> SpalartAllmaras<dim>::get_eddy_viscosity() const {
  return eddy_viscosity;
}

template class TurbulenceModel<2>;
template class TurbulenceModel<3>;
template class SpalartAllmaras<2>;
template class SpalartAllmaras<3>;

} // namespace MPI
} // namespace Fluid
} // namespace ifem_host
