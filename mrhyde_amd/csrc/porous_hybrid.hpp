// porous_hybrid.hpp -- the porousMixedHybridized (hybridized mixed Darcy) module of the MI355X path.
#pragma once
#include "physics.hpp"

namespace mha {

// porousMixedHybridized: K^-1 u + grad p = 0, div u = source with p in HVOL, u in HDIV-DG and the trace lambda in HFACE
// (reference: src/physics/porousMixedHybridized.hpp, src/physics/porousMixedHybridized.cpp:12-464; its label there is
// "porousMixedHybrid").  myvars of the BLOCK {p (HVOL 0), u (HDIV 1)} (:20-41); lambda (HFACE 0, one constant per face)
// is no block variable: it arrives as data per element, and its rows live in the caller's trace system.  The block's
// LIDs are DG -- every LID belongs to one element (check_dg_lids, asked by the element step once per mesh).
// volumeResidual (:72-189) is porousMixed's with total_mobility == 1 and runs on porousMixed's point function with
// function slot 4 pinned to the constant 1; faceResidual (:287-362) on all faces of every element is the element step
// (kernels/porous_hybrid_blocks.hip, kernels/porous_hybrid_fused.hip).  Functions "source" (0), "Kinv_xx|yy|zz" (1)
// (:54-66); "use permeability data" (:42) takes Kinv_dd = 1 / data(elem, 0) as porousMixed does.  Refused by name: the KL
// options (the reference module has none), deck strings that read solution fields, boundary groups of the module (the
// weak "Dirichlet p" and "interface" branches of boundaryResidual :196-280), computeFlux (:369-408), 1-D.
class porousMixedHybridized : public porousMixed {
 public:
  porousMixedHybridized();
  void checkVariables(int dim, const std::vector<VarInfo> &vars) const override;
  void checkBoundaryGroup(const GroupQuery &g) const override;
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  void setParameterVector(const std::string &name, const double *v, int n) override;
  int pointModuleId() const override { return MHA_PHYSICS_POROUS_MIXED; }
  // source, Kinv_xx, Kinv_yy, Kinv_zz in the device table's order (slots 0..3 of porous_point); refuses the
  // field-reading ones by name
  void volumeFunctions(FuncDesc f[4], int dim) const;
  void checkVolumeFunctions(int dim) const override { FuncDesc f[4]; volumeFunctions(f, dim); }
  // the kernels' arguments of the element step: functions and element data (the caller adds state and outputs)
  PmhElementDev elementArgs(int dim);
};

// every LID of lids[nelem][n] lies in [0, nrows) and belongs to exactly one (element, position); MHA_ERR_INVALID names
// the first row that two elements share (a conforming HDIV map) and the module that asks (porousWeakGalerkin shares the check)
void check_dg_lids(int nelem, int n, int nrows, const int32_t *lids, const char *module = "porousMixedHybridized");

}  // namespace mha
