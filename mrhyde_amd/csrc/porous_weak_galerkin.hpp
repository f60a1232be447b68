// porous_weak_galerkin.hpp -- the porousWeakGalerkin (weak Galerkin Darcy) module of the MI355X path.
#pragma once
#include "physics.hpp"

namespace mha {

// porousWeakGalerkin: u = weak gradient of (pint, pbndry), t = -perm u, div t = source, with pint in HVOL, pbndry in
// HFACE, u and t in HDIV-DG (reference: src/physics/porousWeakGalerkin.hpp, src/physics/porousWeakGalerkin.cpp:13-609).
// myvars of the BLOCK {pint (HVOL 0), u (HDIV 1), t (HDIV 1)} (:14-64 without pbndry); pbndry (HFACE 0, one constant
// per face) is no block variable: it arrives as data per element, and its rows live in the caller's trace system.  The
// block's LIDs are DG (check_dg_lids of porous_hybrid.hpp, asked by the element step once per mesh).  volumeResidual
// (:94-323) runs on the point function porous_wg_point; faceResidual (:424-505) on all faces of every element is the
// element step (kernels/porous_wg_blocks.hip, kernels/porous_wg_fused.hip).  Functions "source" (0), "perm" (1) (:69-88);
// "use permeability data" (:58, updatePerm :601-609) takes perm = data(elem, 0), the value itself.  Refused by name:
// "useAC" other than 0 (:20, the HDIV_AC basis is not built), the KL options and any parameter vector (the reference
// module has none), deck strings that read solution fields, boundary groups of the module (the weak "Dirichlet pbndry"
// and "interface" branches of boundaryResidual :329-417), computeFlux (:511-554), 1-D, orders above lowest.
class porousWeakGalerkin : public PhysicsBase {
 public:
  porousWeakGalerkin();
  void checkVariables(int dim, const std::vector<VarInfo> &vars) const override;
  void checkBoundaryGroup(const GroupQuery &g) const override;
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  void setParameterVector(const std::string &name, const double *v, int n) override;
  bool heterogeneous() const override { return usePermData; }
  // source, perm in the device table's order (slots 0, 1 of porous_wg_point); refuses the field-reading ones by name
  void volumeFunctions(FuncDesc f[2]) const;
  void checkVolumeFunctions(int /*dim*/) const override { FuncDesc f[2]; volumeFunctions(f); }
  // the kernels' arguments of the element step: functions and element data (the caller adds state and outputs)
  PwgElementDev elementArgs();
  bool usePermData = false;

 private:
  // the block's element data when "use permeability data" is set (column 0 is perm), else null
  void permData(const double *&edata, int &ecols) const;
};

}  // namespace mha
