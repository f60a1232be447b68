#include "linearelasticity.hpp"

namespace mha {

namespace {

// The constructor's options (linearelasticity.cpp:42-58) whose terms are not built, on both elasticity modules: accepted
// at the value that leaves them off and refused otherwise.  false: `name` is none of them.
bool unbuilt_option(const std::string &label, const std::string &name, double value) {
  if (name == "use crystal elasticity")
    MHA_REQUIRE(value == 0.0, MHA_ERR_INVALID, label << ": 'use crystal elasticity' is not built (CrystalElastic::computeStress)");
  else if (name == "Biot")
    MHA_REQUIRE(value == 0.0, MHA_ERR_INVALID, label << ": 'Biot' (the pressure term of a poroelastic block) is not built");
  else if (name == "use Lame parameters")
    MHA_REQUIRE(value != 0.0, MHA_ERR_INVALID, label << ": 'use Lame parameters' = 0 is not built; give 'lambda' and 'mu'");
  else return false;
  return true;
}

}  // namespace

linearelasticity::linearelasticity(int dim) {
  label = "linearelasticity";
  if (dim == 2) myvars = {"dx", "dy"};  // reference: linearelasticity.cpp:33-40
  else myvars = {"dx", "dy", "dz"};
  mybasistypes.assign(myvars.size(), "HGRAD");
  needs = std::string(dim == 2 ? "the 2 HGRAD variables dx, dy" : "the 3 HGRAD variables dx, dy, dz") +
          ", in that order (the thermoelastic term of an 'e' variable on the block is the module linearelasticity+thermal, "
          "MHA_PHYSICS_LINEARELASTICITY_THERMAL)";
}

void linearelasticity::checkBoundaryGroup(const GroupQuery &g) const {
  MHA_REQUIRE(g.bc_type == MHA_BC_NEUMANN || g.bc_type == MHA_BC_WEAK_DIRICHLET, MHA_ERR_INVALID,
              "linearelasticity: boundary groups are MHA_BC_NEUMANN (traction) or MHA_BC_WEAK_DIRICHLET; the interface "
              "condition (MHA_BC_INTERFACE) is not built");
  MHA_REQUIRE(linearelasticity_boundary_supported(g.dim, g.n, g.nqs), MHA_ERR_INVALID,
              "linearelasticity boundary terms are not available for " << g.n << " dofs per element with " << g.nqs
                                                                       << " side integration points");
}

// reference: linearelasticity::defineFunctions (linearelasticity.cpp:72-76): lambda 1, mu 0.5, sources 0
void linearelasticity::defineFunctions(FunctionManager &fm) {
  functionManager = &fm;
  auto constant = [](double v) { FuncDesc f; f.kind = MHA_FUNC_CONSTANT; f.amp = v; return f; };
  if (!fm.has("lambda")) fm.addFunction("lambda", constant(1.0));
  if (!fm.has("mu")) fm.addFunction("mu", constant(0.5));
  for (const char *k : {"source dx", "source dy", "source dz"})
    if (!fm.has(k)) fm.addFunction(k, constant(0.0));
}

// reference: the constructor's settings (linearelasticity.cpp:42-58)
void linearelasticity::setParameter(const std::string &name, double value) {
  if (name == "incplanestress") incplanestress = value != 0.0;
  else if (name == "form_param") formparam = value;
  else if (name == "penalty") penalty = value;
  else if (!unbuilt_option(label, name, value)) PhysicsBase::setParameter(name, value);
}

// reference: linearelasticity::volumeResidual (linearelasticity.cpp:92-240) as the point function linearelasticity_point
void linearelasticity::volumeResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "linearelasticity::volumeResidual called without a workset");
  Workset &w = *wkset;
  BlockDev b = w.dev;
  b.e_begin = w.first_elem;
  b.e_count = w.numElem;
  PhysParamsDev pp;
  pp.physics = MHA_PHYSICS_LINEARELASTICITY;
  const char *names[5] = {"lambda", "mu", "source dx", "source dy", "source dz"};
  for (int k = 0; k < 5; ++k) pp.f[k] = functionManager->evaluate(names[k]);
  pp.p[0] = incplanestress ? 1.0 : 0.0;
  launch_volume_points(w, b, pp);
}

// reference: linearelasticity::boundaryResidual (linearelasticity.cpp:244-672).  The group's type holds for every
// component of the side; the data of component d is "Neumann d<x|y|z> <side>" (default 0) or "Dirichlet d<x|y|z> <side>".
void linearelasticity::boundaryResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "linearelasticity::boundaryResidual called without a workset");
  Workset &w = *wkset;
  const bool weak = w.current_bc == MHA_BC_WEAK_DIRICHLET;  // or MHA_BC_NEUMANN: checkBoundaryGroup has refused the rest
  for (int v = 1; v < w.layout.nvars; ++v)
    MHA_REQUIRE(w.layout.card[v] == w.layout.card[0], MHA_ERR_INVALID,
                "linearelasticity boundary terms need the same order on every component");
  LeBoundaryDev le;
  const int dim = w.dimension;
  for (int d = 0; d < dim; ++d) {
    const std::string name = std::string(weak ? "Dirichlet " : "Neumann ") + myvars[d] + " " + w.sidename;
    if (weak) {
      le.f[d] = functionManager->evaluate(name);
    } else if (functionManager->has(name)) {
      le.f[d] = functionManager->evaluate(name);
    } else {
      le.f[d].kind = MHA_FUNC_CONSTANT;  // a component without traction data (linearelasticity.cpp:267-284 evaluates
      le.f[d].amp = 0.0;                 // only what the deck names)
    }
    MHA_REQUIRE(!le.f[d].uses_fields, MHA_ERR_INVALID, "boundary data '" << name << "' reads solution fields: not built");
  }
  if (weak) {
    le.f[3] = functionManager->evaluate("lambda");
    le.f[4] = functionManager->evaluate("mu");
    MHA_REQUIRE(le.f[3].kind != MHA_FUNC_IP_ARRAY && le.f[4].kind != MHA_FUNC_IP_ARRAY, MHA_ERR_INVALID,
                "weak Dirichlet needs 'lambda' and 'mu' at the side points: give them as constants, closed forms or deck strings");
    MHA_REQUIRE(!le.f[3].uses_fields && !le.f[4].uses_fields, MHA_ERR_INVALID,
                "linearelasticity: 'lambda' and 'mu' that read solution fields are not built");
  }
  le.penalty = penalty;
  le.form_param = formparam;
  le.plane_stress = incplanestress && dim == 2 ? 1 : 0;
  BoundaryDev bd = w.bnd;
  bd.bc_type = w.current_bc;
  if (w.apply.mode) launch_boundary_apply(w.dev, w.side_tables, bd, le, w.time_dev, w.boundaryRequest(), w.stream);
  else launch_linearelasticity_boundary(w.dev, w.side_tables, bd, le, w.time_dev, w.res, w.stream);
}

void linearelasticity::computeFlux() {
  throw Error(MHA_ERR_INVALID, "linearelasticity: computeFlux is not built");
}

// ---- linearelasticity + thermal on one block ---------------------------------------------------------------------
linearelasticityThermal::linearelasticityThermal(int dim) {
  label = "linearelasticity+thermal";
  if (dim == 2) myvars = {"dx", "dy", "e"};  // linearelasticity.cpp:33-40 and thermal.cpp:31
  else myvars = {"dx", "dy", "dz", "e"};
  mybasistypes.assign(myvars.size(), "HGRAD");
  needs = dim == 2 ? "the 3 HGRAD variables dx, dy, e, in that order" : "the 4 HGRAD variables dx, dy, dz, e, in that order";
}

void linearelasticityThermal::checkVariables(int dim, const std::vector<VarInfo> &vars) const {
  PhysicsBase::checkVariables(dim, vars);
  for (int d = 1; d < dim; ++d)
    MHA_REQUIRE(vars[d].order == vars[0].order, MHA_ERR_INVALID,
                "linearelasticity+thermal needs the same order on every displacement component (e may have its own)");
}

// Traction reads no stress: the plain block's kernel on the displacement rows of the coupled element.  Everything else on
// a side is refused.
void linearelasticityThermal::checkBoundaryGroup(const GroupQuery &g) const {
  MHA_REQUIRE(g.bc_type == MHA_BC_NEUMANN, MHA_ERR_INVALID,
              "linearelasticity+thermal: boundary groups are MHA_BC_NEUMANN (traction on the displacements); weak-Dirichlet "
              "and interface groups (MHA_BC_WEAK_DIRICHLET, MHA_BC_INTERFACE: their side stress needs the thermoelastic "
              "term at the side points) and thermal's groups on e are not built for the coupled block");
  // a Neumann side with data for e is thermal's own condition (thermal.cpp:188-216): not run, and not passed over
  MHA_REQUIRE(!g.functions.has("Neumann e " + g.sidename), MHA_ERR_INVALID,
              "linearelasticity+thermal: thermal's boundary groups on e are not built for the coupled block ('Neumann e "
                  << g.sidename << "' is set); a Neumann group is traction on the displacements");
  MHA_REQUIRE(g.vars[0].order == g.order, MHA_ERR_INVALID,
              "linearelasticity+thermal: traction groups need the order of e not above the displacements'");
  MHA_REQUIRE(linearelasticity_boundary_supported(g.dim, g.dim * g.vars[0].card, g.nqs), MHA_ERR_INVALID,
              "linearelasticity boundary terms are not available for " << g.vars[0].card << " dofs per component with "
                                                                       << g.nqs << " side integration points");
}

// both modules' defineFunctions (linearelasticity.cpp:72-76, thermal.cpp:52-63) on one function manager
void linearelasticityThermal::defineFunctions(FunctionManager &fm) {
  functionManager = &fm;
  auto constant = [](double v) { FuncDesc f; f.kind = MHA_FUNC_CONSTANT; f.amp = v; return f; };
  if (!fm.has("mu")) fm.addFunction("mu", constant(0.5));
  for (const char *k : {"source dx", "source dy", "source dz", "thermal source", "bx", "by", "bz"})
    if (!fm.has(k)) fm.addFunction(k, constant(0.0));
  for (const char *k : {"lambda", "thermal diffusion", "specific heat", "density"})
    if (!fm.has(k)) fm.addFunction(k, constant(1.0));
}

void linearelasticityThermal::setParameter(const std::string &name, double value) {
  if (name == "incplanestress") incplanestress = value != 0.0;
  else if (name == "form_param") formparam = value;
  else if (name == "penalty") penalty = value;
  else if (name == "T_ambient") T_ambient = value;
  else if (name == "alpha_T") alpha_T = value;
  else if (name == "include advection") have_advection = value != 0.0;
  else if (!unbuilt_option(label, name, value)) PhysicsBase::setParameter(name, value);
}

// linearelasticity::volumeResidual with e_num >= 0 and thermal::volumeResidual as ONE point function
// (linearelasticity_thermal_point): the e-columns of the displacement rows come out of the same forward-AD pass
void linearelasticityThermal::volumeResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "linearelasticity+thermal::volumeResidual called without a workset");
  Workset &w = *wkset;
  BlockDev b = w.dev;
  b.e_begin = w.first_elem;
  b.e_count = w.numElem;
  PhysParamsDev pp;
  pp.physics = MHA_PHYSICS_LINEARELASTICITY_THERMAL;
  const char *names[12] = {"lambda", "mu", "source dx", "source dy", "source dz", "thermal source",
                           "thermal diffusion", "specific heat", "density", "bx", "by", "bz"};
  static_assert(kMaxFuncs >= 12, "the coupled module names twelve functions");
  for (int k = 0; k < 12; ++k) pp.f[k] = functionManager->evaluate(names[k]);
  pp.p[0] = incplanestress ? 1.0 : 0.0;
  pp.p[1] = T_ambient;
  pp.p[2] = alpha_T;
  pp.p[3] = have_advection ? 1.0 : 0.0;
  launch_volume_points(w, b, pp);
}

// Traction (linearelasticity.cpp:361-371, 419-429, 482-492, 546-556, 609-619), the one group checkBoundaryGroup takes
void linearelasticityThermal::boundaryResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "linearelasticity+thermal::boundaryResidual called without a workset");
  Workset &w = *wkset;
  const int dim = w.dimension;
  LeBoundaryDev le;
  for (int d = 0; d < dim; ++d) {
    const std::string name = std::string("Neumann ") + myvars[d] + " " + w.sidename;
    if (functionManager->has(name)) {
      le.f[d] = functionManager->evaluate(name);
    } else {
      le.f[d].kind = MHA_FUNC_CONSTANT;
      le.f[d].amp = 0.0;
    }
    MHA_REQUIRE(!le.f[d].uses_fields, MHA_ERR_INVALID, "boundary data '" << name << "' reads solution fields: not built");
  }
  le.disp_card = w.layout.card[0];
  BoundaryDev bd = w.bnd;
  bd.bc_type = w.current_bc;
  if (w.apply.mode) launch_boundary_apply(w.dev, w.side_tables, bd, le, w.time_dev, w.boundaryRequest(), w.stream);
  else launch_linearelasticity_boundary(w.dev, w.side_tables, bd, le, w.time_dev, w.res, w.stream);
}

void linearelasticityThermal::computeFlux() {
  throw Error(MHA_ERR_INVALID, "linearelasticity+thermal: computeFlux is not built for the coupled block");
}

}  // namespace mha
