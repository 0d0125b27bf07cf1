// turbulence.hpp -- host-side mirror of Fluid::MPI::TurbulenceModel<dim> / SpalartAllmaras<dim> (include/mpi_turbulence_model.h,
// include/mpi_spalart_allmaras.h, source/mpi_spalart_allmaras.cpp): the model attached to a fluid solver with
// FluidSolver::attach_turbulence_model("Spalart-Allmaras").  Same member names and call points as the reference; the transport
// equation itself runs on the device of the solver's context through the ifem_sa_* entry points of ifem_hip.h.
// The FSI wall function (update_moving_wall_distance, update_boundary_condition, get_shear_velocity) takes the plain solid description of the
// C ABI (ifem_fsi_solid + ifem_sa_wall) where the reference takes iterator containers; the FSI driver loop itself is not mirrored.
// Not mirrored: mesh refinement transfer, the checkpoint payload (save_checkpoint of a solver with a model attached throws), the serial class family, and PARTITIONED
// fluid solvers: the model needs the wall points of the whole mesh on every rank (the reference all-reduces them) and the mirror does not
// gather them, so make_constraints / initialize_system throw when set_partition named more than one rank.
#pragma once
#include <string>
#include <vector>
#include "../../../include/ifem_hip.h"
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
  // TurbulenceModel::connect_indicator_field (mpi_turbulence_model.cpp:92-98) with the cell indicator as a plain array [n_cells], which it
  // hands to the device; an indicator the caller produced on the device (ifem_fsi_update_indicator) is announced with an empty vector
  void connect_indicator_field(const std::vector<int32_t> &indicator);
  // :17-127.  Hands the solid at its current position to the device, (re)sets the wall when its lists changed since the last call (which
  // resets the device's moving distance), uploads shear_velocities [wall.n_vertices] and measures every node
  void update_moving_wall_distance(const ifem_fsi_solid &solid, const ifem_sa_wall &wall, const std::vector<double> &shear_velocities);
  // :130-215 on the two constraint objects, which make_constraints re-made first; throws "No available indicator function for SA model!"
  // until connect_indicator_field was called
  void update_boundary_condition(bool first_step);
  double get_shear_velocity(double vel, double init_guess); // :218-280
  int64_t last_boundary_lines = 0; // lines the last update_boundary_condition merged into each object
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
  bool has_indicator = false;
  std::vector<int32_t> wall_vertex, wall_edge; // the lists of the last ifem_sa_set_moving_wall
  std::vector<double> wall_normal;
  double wall_key[3] = {0, 0, 0};              // image distance, wall-function distance, sample_at_image_point
};

} // namespace MPI
} // namespace Fluid
} // namespace ifem_host
