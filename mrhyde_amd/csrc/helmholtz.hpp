// helmholtz.hpp -- the helmholtz (frequency-domain wave) module of the MI355X path.
#pragma once
#include "physics.hpp"

namespace mha {

// helmholtz: the complex field u = ureal + i uimag of -div(c^2 grad u) - omega^2 u = source, carried as two HGRAD
// variables (reference: src/physics/helmholtz.hpp, src/physics/helmholtz.cpp:16-450); myvars {ureal, uimag} (:24-27),
// both of ONE order (the reference indexes uimag's basis with ureal's loop index, :155-159; checkVariables refuses two),
// 2-D and 3-D.  Volume terms on the point engine (helmholtz_point, :175-193), the Robin condition of a Neumann group in
// kernels/helmholtz_boundary.hip (:254-419).  The operator is indefinite and non-symmetric, every row couples to both
// variables; it has no time-derivative term.  Not built, and refused: "fractional" (:22; its volume form names 13
// functions where the device table holds 12), weak-Dirichlet and interface groups, functions that read the solution
// fields.  computeFlux is empty in the reference (:430-433): the flux view stays zero.
class helmholtz : public PhysicsBase {
 public:
  helmholtz();
  void checkVariables(int dim, const std::vector<VarInfo> &vars) const override;
  void checkBoundaryGroup(const GroupQuery &g) const override;
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void boundaryResidual() override;
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  // the ten functions of the volume form in the device table's order; refuses the field-reading ones by name
  void volumeFunctions(PhysParamsDev &pp, int dim) const;
  void checkVolumeFunctions(int dim) const override { PhysParamsDev pp; volumeFunctions(pp, dim); }
};

}  // namespace mha
