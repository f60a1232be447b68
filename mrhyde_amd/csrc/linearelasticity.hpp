// linearelasticity.hpp -- the linearelasticity module of the MI355X path.
#pragma once
#include "physics.hpp"

namespace mha {

// linearelasticity: -div sigma(u) = source, sigma = lambda tr(grad u) I + mu (grad u + grad u^T)
// (reference: src/physics/linearelasticity.hpp, src/physics/linearelasticity.cpp:20-672, computeStress :913-1099);
// myvars {dx, dy[, dz]} (:28-39), 2-D and 3-D.  Volume terms on the point engine (linearelasticity_point), traction and
// weak-Dirichlet groups in kernels/linearelasticity_boundary.hip.  Not built, and refused: "use crystal elasticity",
// "Biot", "use Lame parameters" = 0, the thermoelastic term of an "e" variable, the interface condition, computeFlux,
// the stress output.
class linearelasticity : public PhysicsBase {
 public:
  explicit linearelasticity(int dim);
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void boundaryResidual() override;
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  bool incplanestress = false;                // linearelasticity.cpp:47
  double formparam = 1.0, penalty = 10.0;     // modelparams(0), (1) (:54-55)
};

}  // namespace mha
