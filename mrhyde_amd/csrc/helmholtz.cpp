#include "helmholtz.hpp"

namespace mha {

namespace {

// the volume form's functions in the device table's order (helmholtz_point) and the side form's (HelmholtzBoundaryDev)
const char *const kVolumeFuncs[10] = {"c2r_x", "c2i_x", "c2r_y", "c2i_y", "c2r_z", "c2i_z", "omega2r", "omega2i",
                                      "source_r", "source_i"};
const char *const kSideFuncs[10] = {"c2r_x", "c2i_x", "c2r_y", "c2i_y", "c2r_z", "c2i_z", "robin_alpha_r", "robin_alpha_i",
                                    "source_r_side", "source_i_side"};

}  // namespace

helmholtz::helmholtz() {
  label = "helmholtz";
  myvars = {"ureal", "uimag"};        // reference: helmholtz.cpp:24-25
  mybasistypes = {"HGRAD", "HGRAD"};  // reference: helmholtz.cpp:26-27
  needs = "the two HGRAD variables ureal, uimag in 2-D or 3-D";
}

void helmholtz::checkVariables(int dim, const std::vector<VarInfo> &vars) const {
  PhysicsBase::checkVariables(dim, vars);
  // the reference indexes uimag's basis with ureal's loop index (helmholtz.cpp:155-159)
  MHA_REQUIRE(vars[0].order == vars[1].order, MHA_ERR_INVALID, "helmholtz needs the same order on ureal and uimag");
}

// reference: helmholtz::boundaryResidual (helmholtz.cpp:254-419): a side whose condition on ureal is "Neumann" gets the
// Robin terms on both rows (:320); every other type adds nothing there.  Weak-Dirichlet and interface groups, which the
// reference passes over, are refused rather than silently dropped.
void helmholtz::checkBoundaryGroup(const GroupQuery &g) const {
  MHA_REQUIRE(g.bc_type == MHA_BC_NEUMANN, MHA_ERR_INVALID,
              "helmholtz: boundary groups are MHA_BC_NEUMANN (the Robin condition of helmholtz.cpp:320-375); "
              "weak-Dirichlet and interface groups are not built");
  MHA_REQUIRE(helmholtz_boundary_supported(g.dim, g.n, g.nqs), MHA_ERR_INVALID,
              "helmholtz boundary terms are not available for " << g.n << " dofs per element with " << g.nqs
                                                                << " side integration points");
}

// reference: helmholtz::defineFunctions (helmholtz.cpp:41-70): every function defaults to "0.0".  omegar, omegai, the
// alphaH* / alphaT* pairs and freqExp are registered because the reference registers them; only its fractional branch
// (not built) reads them
void helmholtz::defineFunctions(FunctionManager &fm) {
  functionManager = &fm;
  FuncDesc zero;
  zero.kind = MHA_FUNC_CONSTANT;
  zero.amp = 0.0;
  for (const char *k : kVolumeFuncs)
    if (!fm.has(k)) fm.addFunction(k, zero);
  for (const char *k : {"robin_alpha_r", "robin_alpha_i", "source_r_side", "source_i_side", "omegar", "omegai", "alphaHr",
                        "alphaHi", "alphaTr", "alphaTi", "freqExp"})
    if (!fm.has(k)) fm.addFunction(k, zero);
}

// reference: the constructor's settings (helmholtz.cpp:22)
void helmholtz::setParameter(const std::string &name, double value) {
  if (name == "fractional")
    MHA_REQUIRE(value == 0.0, MHA_ERR_INVALID,
                "helmholtz: 'fractional' is not built (its volume form names 13 functions, the device table holds "
                    << kMaxFuncs << ")");
  else PhysicsBase::setParameter(name, value);
}

void helmholtz::volumeFunctions(PhysParamsDev &pp, int dim) const {
  pp.physics = MHA_PHYSICS_HELMHOLTZ;
  static_assert(kMaxFuncs >= 10, "the helmholtz volume form names ten functions");
  for (int k = 0; k < 10; ++k) {
    if (dim == 2 && (k == 4 || k == 5)) continue;  // c2r_z, c2i_z
    pp.f[k] = functionManager->evaluate(kVolumeFuncs[k]);
    MHA_REQUIRE(!(pp.f[k].kind == MHA_FUNC_EXPRESSION && pp.f[k].uses_fields), MHA_ERR_INVALID,
                "helmholtz: '" << kVolumeFuncs[k] << "' reads solution fields: functions of the fields are not built for "
                "this module (the form is linear in ureal, uimag)");
  }
}

// reference: helmholtz::volumeResidual (helmholtz.cpp:77-248, the non-fractional branch) as the point function
// helmholtz_point
void helmholtz::volumeResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "helmholtz::volumeResidual called without a workset");
  Workset &w = *wkset;
  BlockDev b = w.dev;
  b.e_begin = w.first_elem;
  b.e_count = w.numElem;
  PhysParamsDev pp;
  volumeFunctions(pp, w.dimension);
  launch_volume_points(w, b, pp);
}

// the Robin terms of a Neumann group (checkBoundaryGroup has refused every other type)
void helmholtz::boundaryResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "helmholtz::boundaryResidual called without a workset");
  Workset &w = *wkset;
  HelmholtzBoundaryDev hb;
  for (int k = 0; k < 10; ++k) {
    if (w.dimension == 2 && (k == 4 || k == 5)) continue;
    hb.f[k] = functionManager->evaluate(kSideFuncs[k]);
    // an array of a volume function is [E][numip]: not the side points' shape.  The reference evaluates each of these
    // names a second time at the side points (:49-64); constants, closed forms and deck strings do that here
    MHA_REQUIRE(hb.f[k].kind != MHA_FUNC_IP_ARRAY, MHA_ERR_INVALID,
                "helmholtz: '" << kSideFuncs[k] << "' is an integration-point array; a boundary group needs it at the side "
                "points: give it as a constant, a closed form or a deck string");
    MHA_REQUIRE(!hb.f[k].uses_fields, MHA_ERR_INVALID,
                "helmholtz: '" << kSideFuncs[k] << "' reads solution fields: not built");
  }
  BoundaryDev bd = w.bnd;
  bd.bc_type = w.current_bc;
  if (w.apply.mode) launch_boundary_apply(w.dev, w.side_tables, bd, hb, w.time_dev, w.boundaryRequest(), w.stream);
  else launch_helmholtz_boundary(w.dev, w.side_tables, bd, hb, w.time_dev, w.res, w.stream);
}

// helmholtz::computeFlux is empty (helmholtz.cpp:430-433): the flux view keeps the zeros the workset reset left in it
void helmholtz::computeFlux() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "helmholtz::computeFlux called without a workset");
  Workset &w = *wkset;
  MHA_REQUIRE(w.bnd.flux != nullptr, MHA_ERR_INVALID, "computeFlux: no flux array on the workset");
  const size_t npt = static_cast<size_t>(w.bnd.num) * w.side_tables.nqs;
  MHA_HIP(hipMemsetAsync(w.bnd.flux, 0, sizeof(double) * npt, w.stream));
  if (w.bnd.dflux_du) MHA_HIP(hipMemsetAsync(w.bnd.dflux_du, 0, sizeof(double) * npt * w.dev.n, w.stream));
  if (w.bnd.dflux_daux) MHA_HIP(hipMemsetAsync(w.bnd.dflux_daux, 0, sizeof(double) * npt, w.stream));
}

}  // namespace mha
