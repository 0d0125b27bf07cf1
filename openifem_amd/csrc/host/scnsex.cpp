// scnsex.cpp -- host mirror of Fluid::MPI::SCnsEX<dim> (include/mpi_scnsex.h, source/mpi_scnsex.cpp) over the C ABI of ifem_hip.h.
// assemble() and solve() of the reference are the device's (ifem_scnsex_setup / _assemble_rhs / _solve); the outer loop of
// run_one_step (:448-503) runs inside ifem_scnsex_step, so the console shows the line of the LAST outer iteration of a step
// (ITR, ABS_RES, REL_RES, VEL_ITR, PRE_ITR, VEL_RES, PRE_RES; :492-498) instead of one line per iteration.
// ONE deliberate difference from the reference's text: its loop over boundary_condition_time_limits (:554-566) skips the entry that
// follows an erased one; run() removes EVERY expired entry.
// The preconditioner of the two CG solves is Jacobi where the reference uses BoomerAMG (see scnsex.hip); partitioned runs, hanging
// nodes and refinement are refused (by the device entry points and by refine_mesh_not_supported), the turbulence model is not attached.
#include <cmath>
#include <iomanip>
#include "insim.hpp"

namespace ifem_host {
namespace Fluid {
namespace MPI {

template <int dim>
SCnsEX<dim>::SCnsEX(Triangulation<dim> &tria, const Parameters::AllParameters &parameters, int device)
    : FluidSolver<dim>(tria, parameters, device) {
  // mpi_scnsex.cpp:12-14
  if (parameters.fluid_velocity_degree != parameters.fluid_pressure_degree) throw std::invalid_argument("Velocity degree must the same as pressure!");
}

template <int dim>
void SCnsEX<dim>::initialize_system() {
  FluidSolver<dim>::initialize_system();
  this->upload_fields();
}

template <int dim>
void SCnsEX<dim>::set_hard_coded_boundary_condition_time(const unsigned int id, const double limit) {
  if (parameters.fluid_dirichlet_bcs.find(id) == parameters.fluid_dirichlet_bcs.end())
    throw std::invalid_argument("Hard coded BC ID not included in parameters file!");
  if (this->hard_coded_boundary_values.find((int)id) == this->hard_coded_boundary_values.end())
    throw std::invalid_argument("Bundary condition is not hard coded!");
  boundary_condition_time_limits[id] = limit;
}

template <int dim>
ifem_scns_params SCnsEX<dim>::scns_params() const {
  ifem_scns_params p{};
  p.viscosity = parameters.viscosity; p.rho = parameters.fluid_rho; p.dt = time.get_delta_t();
  p.solid_rho = parameters.solid_rho;
  p.formulation = IFEM_FORM_SCNSIM;
  for (int i = 0; i < dim; ++i) p.gravity[i] = parameters.gravity[i];
  p.n_neumann = 0;
  if (parameters.n_fluid_neumann_bcs != 0)
    for (auto &kv : parameters.fluid_neumann_bcs) {
      if (p.n_neumann >= 8) throw std::invalid_argument("at most 8 Neumann boundaries are supported");
      p.neumann_id[p.n_neumann] = (int32_t)kv.first;
      p.neumann_p[p.n_neumann++] = kv.second;
    }
  return p;
}

template <int dim>
void SCnsEX<dim>::run_one_step(bool apply_nonzero_constraints, bool assemble_system) {
  static_cast<void>(apply_nonzero_constraints); // Dirichlet values are always applied as non-zero constraints (mpi_scnsex.h:77-80)
  const ifem_scns_params p = scns_params();
  if (this->output_enabled && time.get_timestep() == 0) this->output_results(0);
  time.increment();
  if (this->pcout)
    *this->pcout << std::string(96, '*') << std::endl
                 << "Time step = " << time.get_timestep() << ", at t = " << std::scientific << time.current() << std::endl;
  // the matrices depend on mu, rho, dt and the PML field alone: the device re-integrates them when one of those changed, so
  // assemble_system only states the reference's intent (first step, or the step after a restart)
  if (assemble_system) check(ifem_scnsex_setup(ctx, &p), "assemble");
  this->last_newton_iterations = this->last_fgmres_iterations = 0;
  const int rc = ifem_scnsex_step(ctx, &p, parameters.fluid_tolerance, (int)parameters.fluid_max_iterations, &last_step);
  if (rc == IFEM_E_NEWTON_MAXIT) throw SolverFailure(rc, "Too many iterations!");
  check(rc, "run_one_step");
  this->last_newton_iterations = last_step.outer_iterations;
  this->last_fgmres_iterations = last_step.vel_iters + last_step.pre_iters;
  if (this->pcout)
    *this->pcout << std::scientific << std::left << " ITR = " << std::setw(2) << last_step.outer_iterations - 1
                 << " ABS_RES = " << last_step.abs_res << " REL_RES = " << last_step.rel_res << " VEL_ITR = " << std::setw(3)
                 << last_step.vel_iters << " PRE_ITR = " << std::setw(3) << last_step.pre_iters << " VEL_RES = " << last_step.vel_res
                 << " PRE_RES = " << last_step.pre_res << std::endl;
  check(ifem_update_stress(ctx, parameters.viscosity, nullptr), "update_stress"); // (:505)
  if (this->output_enabled && time.time_to_output()) this->output_results(time.get_timestep());                      // (:507-510)
  if (parameters.simulation_type == "Fluid" && time.time_to_save()) this->save_checkpoint((int)time.get_timestep()); // (:512-515)
  this->refine_mesh_on_schedule(); // (:516-520; SCnsEX keeps the refusal: refine_mesh_refusal)
}

template <int dim>
const char *SCnsEX<dim>::refine_mesh_refusal() const { return "the SCnsEX entry points refuse hanging nodes"; }

template <int dim>
void SCnsEX<dim>::run() {
  if (this->pcout) *this->pcout << "Running with HIP on 1 MI355X rank(s)..." << std::endl;
  bool success_load = this->load_checkpoint(); // (:531)
  if (!success_load) {
    if (!this->hard_coded_boundary_values.empty()) this->field_time += time.get_delta_t(); // (:534-540)
    this->triangulation.refine_global(parameters.global_refinements[0]);
    this->setup_dofs();
    this->make_constraints();
    this->initialize_system();
  }
  while (time.end() - time.current() > 1e-12) {
    for (auto b = boundary_condition_time_limits.begin(); b != boundary_condition_time_limits.end();) {
      if (b->second < time.current()) {
        this->hard_coded_boundary_values.erase((int)b->first);
        b = boundary_condition_time_limits.erase(b);
      } else
        ++b;
    }
    if (!this->hard_coded_boundary_values.empty()) { // time dependent values: advance the fields by dt and make the constraints again
      this->field_time += time.get_delta_t();
      this->make_constraints();
    }
    run_one_step(true, time.get_timestep() < 1 || success_load);
    success_load = false;
  }
}

template class SCnsEX<2>;
template class SCnsEX<3>;

} // namespace MPI
} // namespace Fluid
} // namespace ifem_host
