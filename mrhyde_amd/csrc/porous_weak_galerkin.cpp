#include "porous_weak_galerkin.hpp"

namespace mha {

namespace {

const char *const kVolumeFuncs[2] = {"source", "perm"};

}  // namespace

porousWeakGalerkin::porousWeakGalerkin() {
  label = "porousWeakGalerkin";
  myvars = {"pint", "u", "t"};              // reference: porousWeakGalerkin.cpp:40-55; pbndry (HFACE) is data, not a block variable
  mybasistypes = {"HVOL", "HDIV", "HDIV"};  // HDIV-DG: the same basis on an element-local LID map
  needs = "the variables pint (HVOL, order 0), u and t (HDIV-DG, order 1), in that order, on 2-D quads or 3-D hexes; the "
          "trace pbndry (HFACE) is no block variable";
}

void porousWeakGalerkin::checkVariables(int dim, const std::vector<VarInfo> &vars) const {
  MHA_REQUIRE(dim == 2 || dim == 3, MHA_ERR_INVALID, label << ": 1-D is not built; the module needs " << needs);
  PhysicsBase::checkVariables(dim, vars);
  MHA_REQUIRE(vars[0].order == 0 && vars[1].order == 1 && vars[2].order == 1, MHA_ERR_INVALID,
              label << " needs " << needs << " (HVOL, HDIV or HFACE above lowest order is not built)");
}

// reference: porousWeakGalerkin::boundaryResidual (:329-417): the weak "Dirichlet pbndry" and the multiscale "interface"
// branch.  Neither is built: the decks give the condition on the trace (`Dirichlet conditions: pbndry`)
void porousWeakGalerkin::checkBoundaryGroup(const GroupQuery &) const {
  throw Error(MHA_ERR_INVALID,
              "porousWeakGalerkin: boundary groups of the module (the weak 'Dirichlet pbndry' and 'interface' branches of "
              "boundaryResidual) are not built; Dirichlet data goes on the trace: fix the trace rows and put the values into lambda");
}

// reference: porousWeakGalerkin::defineFunctions (:69-88): source 0, perm 1
void porousWeakGalerkin::defineFunctions(FunctionManager &fm) {
  functionManager = &fm;
  auto constant = [](double v) { FuncDesc f; f.kind = MHA_FUNC_CONSTANT; f.amp = v; return f; };
  if (!fm.has("source")) fm.addFunction("source", constant(0.0));
  if (!fm.has("perm")) fm.addFunction("perm", constant(1.0));
}

// reference: the constructor's settings (:19-20, 58): "use permeability data"; "useAC" picks the HDIV_AC basis, which is
// not built ("Include face terms" is the caller's choice of running the element step)
void porousWeakGalerkin::setParameter(const std::string &name, double value) {
  if (name == "use permeability data") { usePermData = value != 0.0; return; }
  if (name == "useAC") {
    MHA_REQUIRE(value == 0.0, MHA_ERR_INVALID, "porousWeakGalerkin: 'useAC' asks for the HDIV_AC basis, which is not built");
    return;
  }
  MHA_REQUIRE(name != "use KL expansion" && name != "fix_KL_3d" && name.compare(0, 3, "KL ") != 0, MHA_ERR_INVALID,
              "porousWeakGalerkin has no KL expansion ('" << name << "'): the reference module reads 'use permeability data' and 'useAC' only");
  PhysicsBase::setParameter(name, value);
}

void porousWeakGalerkin::setParameterVector(const std::string &name, const double *, int) {
  throw Error(MHA_ERR_INVALID, "porousWeakGalerkin has no KL expansion and no parameter vector '" + name + "'");
}

void porousWeakGalerkin::volumeFunctions(FuncDesc f[2]) const {
  for (int k = 0; k < 2; ++k) {
    f[k] = functionManager->evaluate(kVolumeFuncs[k]);
    MHA_REQUIRE(!(f[k].kind == MHA_FUNC_EXPRESSION && f[k].uses_fields), MHA_ERR_INVALID,
                "porousWeakGalerkin: '" << kVolumeFuncs[k] << "' reads solution fields: functions of the fields are not "
                "built for this module (the form is linear in pint, u, t, pbndry)");
  }
}

void porousWeakGalerkin::permData(const double *&edata, int &ecols) const {
  edata = nullptr;
  ecols = 0;
  if (!usePermData) return;
  MHA_REQUIRE(wkset != nullptr && wkset->elem_data != nullptr, MHA_ERR_STATE,
              "porousWeakGalerkin: 'use permeability data' is set but the block has no element data (mha_set_element_data / mha_import_mesh_data)");
  edata = wkset->elem_data;
  ecols = wkset->elem_data_cols;
}

// reference: porousWeakGalerkin::volumeResidual (:94-323) as the point function porous_wg_point
void porousWeakGalerkin::volumeResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "porousWeakGalerkin::volumeResidual called without a workset");
  Workset &w = *wkset;
  BlockDev b = w.dev;
  b.e_begin = w.first_elem;
  b.e_count = w.numElem;
  PhysParamsDev pp;
  pp.physics = MHA_PHYSICS_POROUS_WEAK_GALERKIN;
  volumeFunctions(pp.f);
  permData(pp.het.edata, pp.het.ecols);
  launch_volume_points(w, b, pp);
}

// reference: porousWeakGalerkin::computeFlux (:511-554), t . n for the multiscale coupling: not built
void porousWeakGalerkin::computeFlux() {
  throw Error(MHA_ERR_INVALID, "porousWeakGalerkin: computeFlux (the flux of the multiscale 'aux pbndry' coupling) is not built");
}

PwgElementDev porousWeakGalerkin::elementArgs() {
  PwgElementDev a;
  volumeFunctions(a.f);
  permData(a.edata, a.ecols);
  return a;
}

}  // namespace mha
