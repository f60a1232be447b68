// physics.hpp -- physics-module operator API of the MI355X path.
//
// Mirrors template<class EvalT> class PhysicsBase (reference: src/physics/physicsBase.hpp:30-205):
// modules are created by name, get a FunctionManager-like table of named coefficient functions
// through defineFunctions(), are pointed at a Workset with setWorkset(), and expose
// volumeResidual() / boundaryResidual() / faceResidual() / computeFlux() with no arguments and
// no return value -- all I/O goes through the workset.  There is one instance per block instead of
// one per EvalT: the derivative array (EvalT = SFad<W>) is produced inside the kernel.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "workset.hpp"

namespace mha {

// The slice of FunctionManager<EvalT> the functors use: evaluate(name,"ip")
// (reference: src/managers/functionManager.cpp:543-760).  A function is a constant, per-ip data,
// or a member of a small closed family evaluated at the physical integration points.
class FunctionManager {
 public:
  void addFunction(const std::string &name, const FuncDesc &f) { funcs_[name] = f; programs_.erase(name); texts_.erase(name); dirty_ = true; }
  // a deck string: compiled to a postfix program kept on the device for the life of the function (expression.hpp).
  // Compilation is deferred to the first evaluate(): a string may name solution fields of the block (setFieldSlots)
  // and functions of the deck that are defined later, as FunctionManager::decomposeFunctions allows
  // (functionManager.cpp:95-540).
  void addExpression(const std::string &name, const std::string &text);
  // names of Workset::getSolutionField -> slot of the point engine's field array; `_t` names -> time-derivative slots
  void setFieldSlots(const std::map<std::string, int> &fields, const std::map<std::string, int> &fields_t) {
    field_slot_ = fields;
    field_t_slot_ = fields_t;
    dirty_ = true;
  }
  bool has(const std::string &name) const { return funcs_.count(name) != 0 || texts_.count(name) != 0; }
  void setTime(double t) { time_ = t; }
  FuncDesc evaluate(const std::string &name) const {
    if (dirty_) compileAll();
    auto it = funcs_.find(name);
    // reference: TEUCHOS_TEST_FOR_EXCEPTION "function manager could not evaluate" (functionManager.cpp:573)
    MHA_REQUIRE(it != funcs_.end(), MHA_ERR_INVALID, "function manager could not evaluate: " << name);
    FuncDesc f = it->second;
    f.t = time_;
    return f;
  }

 private:
  struct Program { DeviceBuffer<int32_t> code; DeviceBuffer<double> consts; };
  void compileAll() const;
  void compileOne(const std::string &name, std::vector<std::string> &open, std::vector<int32_t> &code, std::vector<double> &consts,
                  bool &fields) const;
  mutable std::map<std::string, FuncDesc> funcs_;
  mutable std::map<std::string, std::shared_ptr<Program>> programs_;
  std::map<std::string, std::string> texts_;
  std::map<std::string, int> field_slot_, field_t_slot_;
  mutable bool dirty_ = false;
  double time_ = 0.0;
};

// one variable of a block: basis type (MHA_BASIS_*), order, dofs per element
struct VarInfo { int type, order, card; };

// a boundary group of the modules as its rule sees it: type, side, and of the block the dofs per element over all
// variables, its order, the integration points of one side, the variables and the function table
struct GroupQuery {
  int bc_type;
  const std::string &sidename;
  int dim, n, order, nqs;
  const std::vector<VarInfo> &vars;
  const FunctionManager &functions;
};

class PhysicsBase {
 public:
  virtual ~PhysicsBase() = default;
  // the module's mybasistypes must be what the block was created with, in that order (physicsInterface.cpp:537-610):
  // any other variable list is refused with "<label> needs <needs>"; a module with a rule on the orders adds it
  virtual void checkVariables(int dim, const std::vector<VarInfo> &vars) const;
  // refuses a boundary group of the module (every type but MHA_BC_DIRICHLET / MHA_BC_FLUX) that boundaryResidual has no
  // term for; asked when the group is added and again before an assembly writes anything.  The default -- any valid
  // type, within the sizes kernels/thermal_boundary.hip is built for -- is also the rule of a block without a module.
  virtual void checkBoundaryGroup(const GroupQuery &g) const { defaultBoundaryGroupRule(g); }
  static void defaultBoundaryGroupRule(const GroupQuery &g);
  virtual void defineFunctions(FunctionManager &fm) { functionManager = &fm; }
  virtual void volumeResidual() { notImplemented("volumeResidual"); }
  virtual void boundaryResidual() { notImplemented("boundaryResidual"); }
  virtual void faceResidual() { notImplemented("faceResidual"); }
  virtual void computeFlux() { notImplemented("computeFlux"); }
  virtual void setWorkset(Workset *w) { wkset = w; }
  // the volume term exists as a point function only; thermal has element kernels beside it
  virtual bool pointEngineOnly() const { return true; }
  // refusals of the module's volume functions that an assembly states before it writes anything
  virtual void checkVolumeFunctions(int /*dim*/) const {}
  // scalar settings a module reads from its parameter list in the reference constructor
  virtual void setParameter(const std::string &name, double) {
    throw Error(MHA_ERR_INVALID, "physics module '" + label + "' has no parameter '" + name + "'");
  }
  // vector-valued parameters the reference module reads from the workset (wkset->getParameter)
  virtual void setParameterVector(const std::string &name, const double *, int) {
    throw Error(MHA_ERR_INVALID, "physics module '" + label + "' has no parameter vector '" + name + "'");
  }
  // reference: getDerivedNames (physicsBase.hpp); the values are AssemblyManager::getDerivedValues
  virtual std::vector<std::string> getDerivedNames() const { return {}; }
  // the module's settings of the stress output (plane stress; with an "e" variable after the displacements alpha_T and
  // T_ambient, and true returned); a module without a stress output refuses
  virtual bool stressSettings(LeStressDev &a) const {
    MHA_REQUIRE(!getDerivedNames().empty(), MHA_ERR_INVALID,
                "physics module '" << label << "' has no derived quantities (the stress output is linearelasticity's)");
    throw Error(MHA_ERR_INVALID, "physics module '" + label + "' has no stress output");
  }
  // true when the coefficients differ from element to element in a way the geometry database cannot see
  virtual bool heterogeneous() const { return false; }

  int id = 0;  // MHA_PHYSICS_*, set by import_physics
  // the module whose point function and variable layout the volume term runs on (engine_dispatch.hpp): its own, unless
  // the volume form is another module's (porousMixedHybridized: porousMixed's)
  virtual int pointModuleId() const { return id; }
  std::string label;
  Workset *wkset = nullptr;
  FunctionManager *functionManager = nullptr;
  std::vector<std::string> myvars, mybasistypes;
  std::string needs;  // the variable list in words

 protected:
  // the reference prints a message for un-overridden hooks (physicsBase.cpp); we raise
  void notImplemented(const char *what) const {
    throw Error(MHA_ERR_INVALID, "physics module '" + label + "' does not implement " + what);
  }
};

// thermal: rho*cp*de/dt - div(kappa grad e) = source
// (reference: src/physics/thermal.hpp, src/physics/thermal.cpp:24-165)
class thermal : public PhysicsBase {
 public:
  thermal();
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void boundaryResidual() override;
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  ThermalDev device_params() const;
  double formparam = 1.0;  // settings "form_param" (reference: thermal.cpp:35)
  bool have_advection = false;  // settings "include advection" (reference: thermal.cpp:39): adds (b . grad e, v)
  // the advection term and coefficients that depend on the solution ("1+e*e") exist in the point-engine form only
  bool pointEngineOnly() const override;
};

// porousMixed: mixed Darcy, (K mobility)^-1 u + grad p = 0, div u = source
// (reference: src/physics/porousMixed.hpp, src/physics/porousMixed.cpp:24-432); myvars {p (HVOL), u (HDIV)}
// Heterogeneous permeability (porousMixed.cpp:46-120, 550-714): "use permeability data" takes Kinv_xx = Kinv_yy = Kinv_zz
// = 1 / data(elem, 0) from the element data of the block (Workset::elem_data); "use KL expansion" divides Kinv_dd by
// exp(KL_dd), a Karhunen-Loeve field with one 1-D expansion per direction ("KL N x", "KL L x", "KL sigma x", "KL eta x",
// ...) and the coefficient vectors "KLUQcoeffs" / "KLStochcoeffs".  The device tables (PorousHetDev) are rebuilt when a
// setting or a vector changes, at the next assembly.
class porousMixed : public PhysicsBase {
 public:
  porousMixed();
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void boundaryResidual() override;
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  void setParameterVector(const std::string &name, const double *v, int n) override;
  bool heterogeneous() const override { return usePermData || useKL; }
  bool usePermData = false, useKL = false;
  // false reproduces the 3-D KLUQcoeffs branch of updateKLPerm (porousMixed.cpp:614-637): lambda_z from the y expansion,
  // the term added twice to KL_xx, once to KL_yy, never to KL_zz
  bool fix_KL_3d = false;

 protected:
  PorousHetDev hetParams();  // (also the element data of porousMixedHybridized, porous_hybrid.hpp)

 private:
  void buildKLTables(int dim);
  int klN_[3] = {-1, -1, -1};
  double klL_[3] = {0, 0, 0}, klSigma_[3] = {0, 0, 0}, klEta_[3] = {0, 0, 0};
  bool klSet_[3][3] = {};  // L, sigma, eta given per direction
  std::vector<double> uq_, stoch_;
  bool hasUQ_ = false, hasStoch_ = false, klDirty_ = true;
  DeviceBuffer<double> klTab_;
};

// navierstokes: incompressible Navier-Stokes with optional SUPG / PSPG
// (reference: src/physics/navierstokes.hpp, src/physics/navierstokes.cpp:20-849, 1054-1079); myvars {ux, pr, uy[, uz]}
class navierstokes : public PhysicsBase {
 public:
  explicit navierstokes(int dim);
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  bool useSUPG = false, usePSPG = false;  // navierstokes.cpp:45-46
  bool fix_uz_offsets = false;            // false reproduces navierstokes.cpp:688
};

// navierstokes + thermal on one block: the reference's `modules: navierstokes, thermal` (Boussinesq coupling).  The two
// modules find each other through the block's variable list -- navierstokes::setWorkset (navierstokes.cpp:1026-1046) sets
// have_energy when it holds "e", thermal::setWorkset (thermal.cpp:359-379) sets have_nsvel when it holds "ux" -- and share
// the function "density" (FunctionManager::addFunction keeps the first tree of a name, functionManager.cpp:48-68).
// myvars {ux, pr, uy[, uz], e}: the variable list when navierstokes is imported before thermal.  Volume terms only: thermal
// boundary groups and computeFlux on this block are refused (kernels/thermal_boundary.hip is written for a one-variable
// block).
class navierstokesThermal : public PhysicsBase {
 public:
  explicit navierstokesThermal(int dim);
  void checkBoundaryGroup(const GroupQuery &g) const override;
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void computeFlux() override;
  void setParameter(const std::string &name, double value) override;
  bool useSUPG = false, usePSPG = false;  // navierstokes.cpp:45-46
  bool fix_uz_offsets = false;            // false reproduces navierstokes.cpp:688
  double T_ambient = 0.0, beta = 1.0;     // navierstokes.cpp:48-53 (model_params)
  bool have_advection = false;            // thermal.cpp:39: adds (b . grad e, v) on top of (u . grad e, v)
};

// shallowwaterHybridized: HDG shallow water, interior unknowns H, Hux, Huy; the trace unknowns are the module's "aux"
// variables (reference: src/physics/shallowwaterHybridized.hpp, .cpp:24-844).  volumeResidual runs on the point engine;
// the side terms (computeFlux, boundaryResidual's fluxes) are the stateless batch entry point mha_swhdg_side_terms:
// the workset-level aux-variable plumbing of the subgrid solver that feeds them is not built.
class shallowwaterHybridized : public PhysicsBase {
 public:
  shallowwaterHybridized();
  void checkVariables(int dim, const std::vector<VarInfo> &vars) const override;
  void defineFunctions(FunctionManager &fm) override;
  void volumeResidual() override;
  void boundaryResidual() override;
  bool roestab = true;    // settings "Roe-like stabilization" / "max EV stabilization" (shallowwaterHybridized.cpp:60-66)
  void setParameter(const std::string &name, double value) override;
  double gravity = 9.81;  // settings "g" (shallowwaterHybridized.cpp:72)
};

// PhysicsImporter::import equivalent (reference: src/physics/physicsImporter.cpp:48-204)
// (dim: the coupled module's variable list depends on it)
std::unique_ptr<PhysicsBase> import_physics(int physics_id, int dim = 3);

}  // namespace mha
