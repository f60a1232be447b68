#include "shallowwater.hpp"

#include "cdr.hpp"

namespace mha {

shallowwater::shallowwater() {
  label = "shallowwater";
  myvars = {"H", "Hu", "Hv"};                  // reference: shallowwater.cpp:24-26
  mybasistypes = {"HGRAD", "HGRAD", "HGRAD"};  // reference: shallowwater.cpp:27-29
  needs = "H, Hu, Hv in 2-D";
}

void shallowwater::checkVariables(int dim, const std::vector<VarInfo> &vars) const {
  MHA_REQUIRE(dim == 2, MHA_ERR_INVALID, label << " needs " << needs);
  PhysicsBase::checkVariables(dim, vars);
}

// reference: shallowwater::defineFunctions (shallowwater.cpp:47-62): bathymetry and bottom friction 1, the rest 0;
// "bathymetry side" is the deck's "bathymetry" string again (:62), default 1
void shallowwater::defineFunctions(FunctionManager &fm) {
  functionManager = &fm;
  auto constant = [](double v) { FuncDesc f; f.kind = MHA_FUNC_CONSTANT; f.amp = v; return f; };
  for (const char *k : {"bathymetry", "bottom friction", "bathymetry side"})
    if (!fm.has(k)) fm.addFunction(k, constant(1.0));
  for (const char *k : {"bathymetry_x", "bathymetry_y", "viscosity", "Coriolis", "source H", "source Hu", "source Hv",
                        "flux left", "flux right", "flux top", "flux bottom", "Neumann source Hu", "Neumann source Hv"})
    if (!fm.has(k)) fm.addFunction(k, constant(0.0));
}

void shallowwater::setParameter(const std::string &name, double value) {
  if (name == "gravity") gravity = value;
  else if (name == "form_param") formparam = value;
  else PhysicsBase::setParameter(name, value);
}

// reference: shallowwater::volumeResidual (shallowwater.cpp:118-153) as the point function shallowwater_point.
// "viscosity" and "Coriolis" are not passed: no term reads them.
void shallowwater::volumeResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "shallowwater::volumeResidual called without a workset");
  Workset &w = *wkset;
  BlockDev b = w.dev;
  b.e_begin = w.first_elem;
  b.e_count = w.numElem;
  PhysParamsDev pp;
  pp.physics = MHA_PHYSICS_SHALLOWWATER;
  const char *names[6] = {"bathymetry", "bathymetry_x", "bathymetry_y", "source H", "source Hu", "source Hv"};
  for (int k = 0; k < 6; ++k) pp.f[k] = functionManager->evaluate(names[k]);
  pp.p[0] = gravity;
  launch_volume_points(w, b, pp);
}

void shallowwater::computeFlux() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "shallowwater::computeFlux called without a workset");
  zero_flux(*wkset);
}

}  // namespace mha
