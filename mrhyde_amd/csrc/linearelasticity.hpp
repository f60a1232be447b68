// linearelasticity.hpp -- the linearelasticity module of the MI355X path.
#pragma once
#include "physics.hpp"

namespace mha {

// linearelasticity: -div sigma(u) = source, sigma = lambda tr(grad u) I + mu (grad u + grad u^T)
// (reference: src/physics/linearelasticity.hpp, src/physics/linearelasticity.cpp:20-672, computeStress :913-1099);
// myvars {dx, dy[, dz]} (:28-39), 2-D and 3-D.  Volume terms on the point engine (linearelasticity_point), traction and
// weak-Dirichlet groups in kernels/linearelasticity_boundary.hip.  Not built, and refused: "use crystal elasticity",
// "Biot", "use Lame parameters" = 0, an "e" variable on the block (that is linearelasticityThermal below), the interface
// condition, computeFlux.  The stress output (getDerivedNames / getDerivedValues, :1289-1360) is
// AssemblyManager::getDerivedValues with kernels/linearelasticity_stress.hip.
class linearelasticity : public PhysicsBase {
 public:
  explicit linearelasticity(int dim);
  void checkBoundaryGroup(const GroupQuery &g) const override;
  bool stressSettings(LeStressDev &a) const override { a.plane_stress = incplanestress; return false; }
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void boundaryResidual() override;
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  std::vector<std::string> getDerivedNames() const override { return {"VM stress", "MAG stress"}; }  // :1289-1295
  bool incplanestress = false;                // linearelasticity.cpp:47
  double formparam = 1.0, penalty = 10.0;     // modelparams(0), (1) (:54-55)
};

// linearelasticity + thermal on one block: the reference's `modules: thermal, linearelasticity` (thermoelastic coupling).
// linearelasticity::setWorkset (linearelasticity.cpp:860-906) finds e_num when the block holds "e"; computeStress
// (:913-1276) then subtracts alpha_T (e - T_ambient) c from the normal stresses, c = 3 lambda + 2 mu, and 5 mu under
// incplanestress in 2-D.  thermal sees no "ux" on the block, so its row is the plain one (thermal.cpp:125-163).
// myvars {dx, dy[, dz], e}: the displacements first, so that variable d is component d as on the plain block (the
// reference finds the variables by name).  Volume terms on the point engine (linearelasticity_thermal_point), traction
// groups through kernels/linearelasticity_boundary.hip.  Refused: weak-Dirichlet and interface groups (their side stress
// needs the thermoelastic term at the side points), thermal's boundary groups on e, computeFlux, and what the plain
// block refuses.
class linearelasticityThermal : public PhysicsBase {
 public:
  explicit linearelasticityThermal(int dim);
  void checkVariables(int dim, const std::vector<VarInfo> &vars) const override;
  void checkBoundaryGroup(const GroupQuery &g) const override;
  bool stressSettings(LeStressDev &a) const override {
    a.plane_stress = incplanestress;
    a.alpha_T = alpha_T;
    a.T_ambient = T_ambient;
    return true;
  }
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void boundaryResidual() override;
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  std::vector<std::string> getDerivedNames() const override { return {"VM stress", "MAG stress"}; }  // :1289-1295
  bool incplanestress = false;                // linearelasticity.cpp:47
  double formparam = 1.0, penalty = 10.0;     // modelparams(0), (1) (:54-55): accepted, no term of this block reads them
  double T_ambient = 0.0, alpha_T = 1.0e-6;   // modelparams(3), (4) (:57-58)
  bool have_advection = false;                // thermal.cpp:39
};

}  // namespace mha
