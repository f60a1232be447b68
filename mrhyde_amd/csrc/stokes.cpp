#include "stokes.hpp"

#include "cdr.hpp"

namespace mha {

stokes::stokes(int dim) {
  label = "stokes";
  if (dim == 3) myvars = {"ux", "pr", "uy", "uz"};  // reference: stokes.cpp:25-32
  else myvars = {"ux", "pr", "uy"};
  mybasistypes.assign(myvars.size(), "HGRAD");  // reference: stokes.cpp:34-41
  needs = dim == 3 ? "ux, pr, uy, uz, in that order" : "ux, pr, uy, in that order";
}

// reference: stokes::defineFunctions (stokes.cpp:58-62): sources 0, viscosity 1
void stokes::defineFunctions(FunctionManager &fm) {
  functionManager = &fm;
  auto constant = [](double v) { FuncDesc f; f.kind = MHA_FUNC_CONSTANT; f.amp = v; return f; };
  for (const char *k : {"source ux", "source pr", "source uy", "source uz"})
    if (!fm.has(k)) fm.addFunction(k, constant(0.0));
  if (!fm.has("viscosity")) fm.addFunction("viscosity", constant(1.0));
}

void stokes::setParameter(const std::string &name, double value) {
  if (name == "usePSPG") usePSPG = value != 0.0;
  else if (name == "useLSIC") useLSIC = value != 0.0;
  else PhysicsBase::setParameter(name, value);
}

// reference: stokes::volumeResidual (stokes.cpp:178-438) as the point function stokes_point.  "source pr" is not passed:
// no term reads it.  Table: source ux, source uy[, source uz], viscosity.
void stokes::volumeResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "stokes::volumeResidual called without a workset");
  Workset &w = *wkset;
  BlockDev b = w.dev;
  b.e_begin = w.first_elem;
  b.e_count = w.numElem;
  PhysParamsDev pp;
  pp.physics = MHA_PHYSICS_STOKES;
  const char *sources[3] = {"source ux", "source uy", "source uz"};
  for (int d = 0; d < w.dimension; ++d) pp.f[d] = functionManager->evaluate(sources[d]);
  pp.f[w.dimension] = functionManager->evaluate("viscosity");
  pp.p[0] = usePSPG ? 1.0 : 0.0;
  pp.p[1] = useLSIC ? 1.0 : 0.0;
  launch_volume_points(w, b, pp);
}

void stokes::computeFlux() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "stokes::computeFlux called without a workset");
  zero_flux(*wkset);
}

}  // namespace mha
