// stokes.hpp -- the stokes module of the MI355X path.
#pragma once
#include "physics.hpp"

namespace mha {

// stokes: -div(viscosity grad u) + grad pr = source, div u = 0, with optional PSPG and LSIC stabilisation
// (reference: src/physics/stokes.hpp, src/physics/stokes.cpp:17-456); myvars {ux, pr, uy[, uz]} (:25-41), each variable
// with its own order (Q1/Q1 with PSPG, Q2/Q1 without), 2-D and 3-D.  Volume terms on the point engine (stokes_point), on
// navierstokes' variable layout.  "source pr" is registered because the reference registers it (:59); the reference
// evaluates it (:78) and no term reads it: it is not passed to the device.  boundaryResidual and computeFlux are empty in
// the reference (:444-456): groups add nothing -- no kernel runs, so no limit on the element size applies to them -- and
// the flux view stays zero.
class stokes : public PhysicsBase {
 public:
  explicit stokes(int dim);
  void checkBoundaryGroup(const GroupQuery &) const override {}
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void boundaryResidual() override {}
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  bool usePSPG = false, useLSIC = false;  // stokes.cpp:44-45
};

}  // namespace mha
