// cdr.hpp -- the cdr (convection-diffusion-reaction) module of the MI355X path, alone and beside navierstokes.
#pragma once
#include "physics.hpp"

namespace mha {

// computeFlux of a module whose flux is empty in the reference: zeros in the workset's flux views
void zero_flux(Workset &w);

// cdr: c_t + v . grad c - div(diffusion / (density specific heat) grad c) + reaction = source
// (reference: src/physics/cdr.hpp, src/physics/cdr.cpp:15-142); myvars {c} (:22-23), 2-D and 3-D.  Volume terms on the
// point engine (cdr_point).  Every function may read the solution fields ("reaction: 0.5*c*c"): the engine then runs the
// instantiation whose functions are Dual numbers.  "SUPG tau" is registered because the reference registers it (:48); the
// reference evaluates it (:82) and no term reads it, and computeTau (:186-207) has no caller: neither is built.
// boundaryResidual and computeFlux are empty in the reference (:147-164): groups add nothing, the flux view stays zero.
class cdr : public PhysicsBase {
 public:
  cdr();
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void boundaryResidual() override {}
  void computeFlux() override;
};

// navierstokes + cdr on one block: the reference's `modules: navier stokes, cdr`.  Neither module looks for the other's
// variables (navierstokes::setWorkset finds only "e", cdr::setWorkset only "c", cdr.cpp:169-180): the coupling is what
// cdr's functions read from the block's fields (xvel: 'ux').  They share the function "density"
// (FunctionManager::addFunction keeps the first tree of a name, functionManager.cpp:48-68).  myvars {ux, pr, uy[, uz], c}:
// the variable list when navierstokes is imported before cdr.  Volume terms only: boundary groups of the modules and
// computeFlux are refused, as on navierstokes+thermal.
class navierstokesCdr : public PhysicsBase {
 public:
  explicit navierstokesCdr(int dim);
  void checkBoundaryGroup(const GroupQuery &g) const override;
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  bool useSUPG = false, usePSPG = false;  // navierstokes.cpp:45-46
  bool fix_uz_offsets = false;            // false reproduces navierstokes.cpp:688
};

}  // namespace mha
