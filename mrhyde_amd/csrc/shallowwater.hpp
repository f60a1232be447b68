// shallowwater.hpp -- the continuous-Galerkin shallow water module of the MI355X path.
#pragma once
#include "physics.hpp"

namespace mha {

// shallowwater: xi_t + div(Hu, Hv) = source H and the two momentum equations in conservative form, D = xi + bathymetry
// (reference: src/physics/shallowwater.hpp, src/physics/shallowwater.cpp:17-174); myvars {H, Hu, Hv} (:24-29), 2-D only.
// Volume terms on the point engine (shallowwater_point).  Functions read by the volume terms: bathymetry, bathymetry_x,
// bathymetry_y, source H, source Hu, source Hv.  "viscosity" and "Coriolis" are evaluated by the reference (:79-80) and no
// term reads them: registered, not passed to the device.  "bottom friction", the "flux <side>" and "Neumann source"
// side functions and "bathymetry side" (:50, :56-62) are registered by the reference and never evaluated: accepted and
// unread, as cdr's "SUPG tau".  boundaryResidual and computeFlux are empty in the reference (:161-174): groups add nothing
// (no kernel runs, so no limit on the element size applies to them), the flux view stays zero.
class shallowwater : public PhysicsBase {
 public:
  shallowwater();
  void checkVariables(int dim, const std::vector<VarInfo> &vars) const override;
  void checkBoundaryGroup(const GroupQuery &) const override {}
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void boundaryResidual() override {}
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  double gravity = 9.8;    // settings "gravity" (shallowwater.cpp:32); shallowwaterHybridized's "g" is 9.81
  double formparam = 1.0;  // settings "form_param" (:34): read by no term
};

}  // namespace mha
