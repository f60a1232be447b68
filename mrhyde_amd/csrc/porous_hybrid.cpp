#include "porous_hybrid.hpp"

namespace mha {

namespace {

const char *const kVolumeFuncs[4] = {"source", "Kinv_xx", "Kinv_yy", "Kinv_zz"};

}  // namespace

porousMixedHybridized::porousMixedHybridized() {
  label = "porousMixedHybridized";
  myvars = {"p", "u"};              // reference: porousMixedHybridized.cpp:20-41; lambda (HFACE) is data, not a block variable
  mybasistypes = {"HVOL", "HDIV"};  // HDIV-DG: the same basis on an element-local LID map
  needs = "the variables p (HVOL, order 0) and u (HDIV-DG, order 1), in that order, on 2-D quads or 3-D hexes; the trace "
          "lambda (HFACE) is no block variable";
}

void porousMixedHybridized::checkVariables(int dim, const std::vector<VarInfo> &vars) const {
  MHA_REQUIRE(dim == 2 || dim == 3, MHA_ERR_INVALID, label << ": 1-D is not built; the module needs " << needs);
  PhysicsBase::checkVariables(dim, vars);
  MHA_REQUIRE(vars[0].order == 0 && vars[1].order == 1, MHA_ERR_INVALID,
              label << " needs " << needs << " (HDIV or HFACE above lowest order is not built)");
}

// reference: porousMixedHybrid::boundaryResidual (:196-280): the weak "Dirichlet p" and the multiscale "interface"
// branch.  Neither is built: the decks give the condition on the trace (`Dirichlet conditions: lambda`)
void porousMixedHybridized::checkBoundaryGroup(const GroupQuery &) const {
  throw Error(MHA_ERR_INVALID,
              "porousMixedHybridized: boundary groups of the module (the weak 'Dirichlet p' and 'interface' branches of "
              "boundaryResidual) are not built; Dirichlet data goes on the trace: fix the trace rows and put the values into lambda");
}

// reference: porousMixedHybrid::defineFunctions (:54-66): source 0, Kinv_* 1; no total_mobility
void porousMixedHybridized::defineFunctions(FunctionManager &fm) {
  functionManager = &fm;
  auto constant = [](double v) { FuncDesc f; f.kind = MHA_FUNC_CONSTANT; f.amp = v; return f; };
  if (!fm.has("source")) fm.addFunction("source", constant(0.0));
  for (const char *k : {"Kinv_xx", "Kinv_yy", "Kinv_zz"})
    if (!fm.has(k)) fm.addFunction(k, constant(1.0));
}

// reference: the constructor's settings (:42): "use permeability data" alone
void porousMixedHybridized::setParameter(const std::string &name, double value) {
  if (name == "use permeability data") { usePermData = value != 0.0; return; }
  MHA_REQUIRE(name != "use KL expansion" && name != "fix_KL_3d" && name.compare(0, 3, "KL ") != 0, MHA_ERR_INVALID,
              "porousMixedHybridized has no KL expansion ('" << name << "'): the reference module reads 'use permeability data' only");
  PhysicsBase::setParameter(name, value);
}

void porousMixedHybridized::setParameterVector(const std::string &name, const double *, int) {
  throw Error(MHA_ERR_INVALID, "porousMixedHybridized has no KL expansion and no parameter vector '" + name + "'");
}

void porousMixedHybridized::volumeFunctions(FuncDesc f[4], int dim) const {
  for (int k = 0; k < 4; ++k) {
    if (k == 3 && dim == 2) { f[k] = FuncDesc(); f[k].amp = 1.0; continue; }  // Kinv_zz
    f[k] = functionManager->evaluate(kVolumeFuncs[k]);
    MHA_REQUIRE(!(f[k].kind == MHA_FUNC_EXPRESSION && f[k].uses_fields), MHA_ERR_INVALID,
                "porousMixedHybridized: '" << kVolumeFuncs[k] << "' reads solution fields: functions of the fields are not "
                "built for this module (the form is linear in p, u, lambda)");
  }
}

// reference: porousMixedHybrid::volumeResidual (:72-189) = porousMixed::volumeResidual with total_mobility == 1: the
// point function porous_point under porousMixed's id, function slot 4 the constant 1
void porousMixedHybridized::volumeResidual() {
  MHA_REQUIRE(wkset != nullptr, MHA_ERR_STATE, "porousMixedHybridized::volumeResidual called without a workset");
  Workset &w = *wkset;
  BlockDev b = w.dev;
  b.e_begin = w.first_elem;
  b.e_count = w.numElem;
  PhysParamsDev pp;
  pp.physics = pointModuleId();
  volumeFunctions(pp.f, w.dimension);
  pp.f[4] = FuncDesc();
  pp.f[4].amp = 1.0;
  pp.het = hetParams();
  if (!w.apply.mode && w.res.res == nullptr && w.res.crs_vals == nullptr) launch_porous_element(b, w.layout, pp, w.time_dev, w.res, w.stream);
  else launch_volume_points(w, b, pp);
}

// reference: porousMixedHybrid::computeFlux (:369-408), u . n for the multiscale coupling: not built
void porousMixedHybridized::computeFlux() {
  throw Error(MHA_ERR_INVALID, "porousMixedHybridized: computeFlux (the flux of the multiscale 'aux p' coupling) is not built");
}

PmhElementDev porousMixedHybridized::elementArgs(int dim) {
  PmhElementDev a;
  volumeFunctions(a.f, dim);
  const PorousHetDev h = hetParams();
  a.edata = h.edata;
  a.ecols = h.ecols;
  return a;
}

void check_dg_lids(int nelem, int n, int nrows, const int32_t *lids, const char *module) {
  MHA_REQUIRE(nelem > 0 && n > 0 && nrows > 0 && lids, MHA_ERR_INVALID, "DG check: null or empty LID map");
  std::vector<int32_t> owner(static_cast<size_t>(nrows), -1);
  for (int e = 0; e < nelem; ++e)
    for (int k = 0; k < n; ++k) {
      const int32_t row = lids[static_cast<size_t>(e) * n + k];
      MHA_REQUIRE(row >= 0 && row < nrows, MHA_ERR_INVALID, "DG check: LID out of range: " << row);
      MHA_REQUIRE(owner[row] < 0, MHA_ERR_INVALID,
                  module << ": row " << row << " belongs to elements " << owner[row] << " and " << e
                      << ": the block's LIDs must be DG (every LID in exactly one element); a conforming HDIV map is porousMixed's");
      owner[row] = e;
    }
}

}  // namespace mha
