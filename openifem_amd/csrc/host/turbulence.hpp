// turbulence.hpp -- host-side mirror of Fluid::MPI::TurbulenceModel<dim> / SpalartAllmaras<dim> (include/mpi_turbulence_model.h,
// include/mpi_spalart_allmaras.h, source/mpi_spalart_allmaras.cpp): the model attached to a fluid solver with
// FluidSolver::attach_turbulence_model("Spalart-Allmaras").  Same member names and call points as the reference; the transport
// equation itself runs on the device of the solver's context through the ifem_sa_* entry points of ifem_hip.h.
// Not mirrored: the FSI wall function (update_moving_wall_distance, update_boundary_condition, get_shear_velocity), mesh refinement
// transfer, the checkpoint payload (save_checkpoint of a solver with a model attached throws), the serial class family, and PARTITIONED
// fluid solvers: the model needs the wall points of the whole mesh on every rank (the reference all-reduces them) and the mirror does not
// gather them, so make_constraints / initialize_system throw when set_partition named more than one rank.
#pragma once
#include <string>
#include <vector>
#include "grid.hpp"
#include "parameters.hpp"

namespace ifem_host {
namespace Fluid {
namespace MPI {

template <int dim>
class FluidSolver;

template <int dim>
class TurbulenceModel {
public:
  virtual ~TurbulenceModel() = default;
  virtual void make_constraints() = 0;
  virtual void initialize_system() = 0;
  virtual void run_one_step(bool apply_nonzero_constraints) = 0;
  virtual std::vector<double> get_present_solution() const = 0; // nu~ on the scalar Q_kv space [n_unodes]
  virtual std::vector<double> get_eddy_viscosity() const = 0;   // mu_t [n_unodes]
  // TurbulenceModelFactory<dim>::create: anything but "Spalart-Allmaras" is ExcNotImplemented
  static TurbulenceModel<dim> *create(FluidSolver<dim> &, const std::string &model_name);
};

template <int dim>
class SpalartAllmaras : public TurbulenceModel<dim> {
public:
  explicit SpalartAllmaras(FluidSolver<dim> &fluid) : fluid(fluid) {}
  // :348-406: type 0 (wall) gives 0, type 1 (inflow) 5 mu / rho on the nonzero object, both give 0 on the zero object; boundary ids in
  // ascending order, the first line of a node stays
  void make_constraints() override;
  // :542-567: nu~ = coefficient mu / rho, constrained nodes 0, then setup_cell_property (wall points = the vertices of the type-0 faces)
  void initialize_system() override;
  void run_one_step(bool apply_nonzero_constraints) override; // :283-345
  std::vector<double> get_present_solution() const override;
  std::vector<double> get_eddy_viscosity() const override; // the host copy taken at the end of the last run_one_step (zero before the first)
  // the lines of nonzero_constraints (node, inhomogeneity) and the wall points [n][dim] as handed to the device
  const std::vector<int32_t> &constraint_nodes() const { return nodes; }
  const std::vector<double> &constraint_values() const { return values; }
  const std::vector<double> &wall_points() const { return wall; }
  unsigned int last_newton_iterations = 0;

private:
  void refuse_partitioned() const;
  FluidSolver<dim> &fluid;
  std::vector<int32_t> nodes;
  std::vector<double> values, wall, eddy_viscosity;
};

} // namespace MPI
} // namespace Fluid
} // namespace ifem_host
