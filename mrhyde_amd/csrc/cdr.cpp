#include "cdr.hpp"

namespace mha {

namespace {

FuncDesc constant(double v) {
  FuncDesc f;
  f.kind = MHA_FUNC_CONSTANT;
  f.amp = v;
  return f;
}

// reference: cdr::defineFunctions (cdr.cpp:40-48): source 0, diffusion 1, specific heat 1, density 1, reaction 1,
// xvel / yvel / zvel 1, SUPG tau 0
void define_cdr_functions(FunctionManager &fm) {
  for (const char *k : {"source", "SUPG tau"})
    if (!fm.has(k)) fm.addFunction(k, constant(0.0));
  for (const char *k : {"diffusion", "specific heat", "density", "reaction", "xvel", "yvel", "zvel"})
    if (!fm.has(k)) fm.addFunction(k, constant(1.0));
}

}  // namespace

// navierstokes::computeFlux and cdr::computeFlux are empty (navierstokes.cpp:1016-1018, cdr.cpp:161-164), as are those of
// stokes and shallowwater: the flux view keeps the zeros the workset reset left in it
void zero_flux(Workset &w) {
  MHA_REQUIRE(w.bnd.flux != nullptr, MHA_ERR_INVALID, "computeFlux: no flux array on the workset");
  const size_t npt = static_cast<size_t>(w.bnd.num) * w.side_tables.nqs;
  MHA_HIP(hipMemsetAsync(w.bnd.flux, 0, sizeof(double) * npt, w.stream));
  if (w.bnd.dflux_du) MHA_HIP(hipMemsetAsync(w.bnd.dflux_du, 0, sizeof(double) * npt * w.dev.n, w.stream));
  if (w.bnd.dflux_daux) MHA_HIP(hipMemsetAsync(w.bnd.dflux_daux, 0, sizeof(double) * npt, w.stream));
}

cdr::cdr() {
  label = "cdr";
  myvars = {"c"};            // reference: cdr.cpp:22
  mybasistypes = {"HGRAD"};  // reference: cdr.cpp:23
  needs = "one HGRAD variable (c) in 2-D or 3-D";
}

void cdr::defineFunctions(FunctionManager &fm) {
  functionManager = &fm;
  define_cdr_functions(fm);
}

// reference: cdr::volumeResidual (cdr.cpp:62-142) as the point function cdr_point.  "SUPG tau" is not passed: no term
// reads it.
void cdr::volumeResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "cdr::volumeResidual called without a workset");
  Workset &w = *wkset;
  BlockDev b = w.dev;
  b.e_begin = w.first_elem;
  b.e_count = w.numElem;
  PhysParamsDev pp;
  pp.physics = MHA_PHYSICS_CDR;
  const char *names[8] = {"source", "diffusion", "specific heat", "density", "reaction", "xvel", "yvel", "zvel"};
  for (int k = 0; k < 5 + w.dimension; ++k) pp.f[k] = functionManager->evaluate(names[k]);
  launch_volume_points(w, b, pp);
}

void cdr::computeFlux() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "cdr::computeFlux called without a workset");
  zero_flux(*wkset);
}

// ---- navierstokes + cdr on one block -----------------------------------------------------------------------------
navierstokesCdr::navierstokesCdr(int dim) {
  label = "navierstokes+cdr";
  if (dim == 2) myvars = {"ux", "pr", "uy", "c"};  // navierstokes.cpp:27-34 followed by cdr.cpp:22
  else myvars = {"ux", "pr", "uy", "uz", "c"};
  mybasistypes.assign(myvars.size(), "HGRAD");
  needs = dim == 3 ? "the 5 HGRAD variables ux, pr, uy, uz, c, in that order" : "the 4 HGRAD variables ux, pr, uy, c, in that order";
}

// both modules' defineFunctions (navierstokes.cpp:62-76, cdr.cpp:40-48) on one function manager: "density" is registered
// once and read by both
void navierstokesCdr::defineFunctions(FunctionManager &fm) {
  functionManager = &fm;
  for (const char *k : {"source ux", "source pr", "source uy", "source uz"})
    if (!fm.has(k)) fm.addFunction(k, constant(0.0));
  for (const char *k : {"density", "viscosity"})
    if (!fm.has(k)) fm.addFunction(k, constant(1.0));
  define_cdr_functions(fm);
}

void navierstokesCdr::setParameter(const std::string &name, double value) {
  if (name == "useSUPG") useSUPG = value != 0.0;
  else if (name == "usePSPG") usePSPG = value != 0.0;
  else if (name == "fix_uz_offsets") fix_uz_offsets = value != 0.0;
  else PhysicsBase::setParameter(name, value);
}

// navierstokes::volumeResidual and cdr::volumeResidual as ONE point function (navierstokes_cdr_point).  The device table
// holds kMaxFuncs = 12 functions and the two modules name 13 in 3-D: "source pr", which no term of navierstokes reads, is
// left out and cdr's "source" takes its place (physics_points.hpp).
void navierstokesCdr::volumeResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "navierstokes+cdr::volumeResidual called without a workset");
  Workset &w = *wkset;
  BlockDev b = w.dev;
  b.e_begin = w.first_elem;
  b.e_count = w.numElem;
  PhysParamsDev pp;
  pp.physics = MHA_PHYSICS_NAVIERSTOKES_CDR;
  const char *names[12] = {"source ux", "source", "source uy", "source uz", "density", "viscosity",
                           "diffusion", "specific heat", "reaction", "xvel", "yvel", "zvel"};
  static_assert(kMaxFuncs == 12, "the coupled module fills the table: source pr is left out to fit");
  for (int k = 0; k < 12; ++k) {
    if ((k == 3 || k == 11) && w.dimension == 2) continue;  // source uz, zvel
    pp.f[k] = functionManager->evaluate(names[k]);
  }
  // in the field-reading instantiation only cdr's functions are Dual numbers
  for (int k : {0, 2, 3, 4, 5})
    MHA_REQUIRE(!(pp.f[k].kind == MHA_FUNC_EXPRESSION && pp.f[k].uses_fields), MHA_ERR_INVALID,
                "navierstokes+cdr: '" << names[k] << "' reads solution fields: functions of the fields are built for cdr's "
                "functions (source, diffusion, specific heat, reaction, xvel, yvel, zvel), not for navierstokes' own"
                << (k == 4 ? " or the shared density" : ""));
  pp.p[0] = useSUPG ? 1.0 : 0.0;
  pp.p[1] = usePSPG ? 1.0 : 0.0;
  pp.p[2] = fix_uz_offsets ? 1.0 : 0.0;
  launch_volume_points(w, b, pp);
}

// neither module has a boundary term here (navierstokes' are not built, cdr's are empty in the reference): a group of the
// modules on this block is refused rather than passed over
void navierstokesCdr::checkBoundaryGroup(const GroupQuery &) const {
  throw Error(MHA_ERR_INVALID,
              "navierstokes+cdr: boundary groups of the modules (Neumann, weak Dirichlet, interface) are not built for the "
              "coupled block; strong Dirichlet rows and the generic Flux condition are");
}

void navierstokesCdr::computeFlux() {
  throw Error(MHA_ERR_INVALID, "navierstokes+cdr: computeFlux is not built for the coupled block");
}

}  // namespace mha
