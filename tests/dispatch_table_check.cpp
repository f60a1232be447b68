// dispatch_table_check.cpp -- host-only check of kernels/engine_dispatch.hpp: which (dimension, module) pairs
// dispatch_module reaches, which EXPR variant dispatch_expr hands each module in each situation, and the texts of the
// refusals, against the table written out below.  No HIP runtime call: built host-only and run by
// tests/test_dispatch_table.py on a machine without a GPU.  Prints "ok" and returns 0, or one line per mismatch and 1.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../mrhyde_amd/csrc/kernels/engine_dispatch.hpp"

using namespace mha;

namespace {

const char *kFieldsRefusal = "functions of the solution fields are built for the thermal module";
const char *kHetRefusal =
    "porousMixed: heterogeneous permeability with deck-string functions is not built; give source / mobility as constants or closed forms";
constexpr int FIELDS_REFUSED = -1, HET_REFUSED = -2;

// per module: the dimensions it exists in and EXPR (or the refusal) for
//   plain | a deck string | a deck string that reads the fields | heterogeneous data | heterogeneous data + a deck string
struct Row {
  int physics;
  const char *name;
  bool in2d, in3d;
  int plain, deck, fields, het, het_deck;
};
const Row kTable[] = {
    {MHA_PHYSICS_THERMAL, "thermal", true, true, 0, 1, 2, 0, 1},
    {MHA_PHYSICS_POROUS_MIXED, "porousMixed", true, true, 0, 1, FIELDS_REFUSED, 3, HET_REFUSED},
    {MHA_PHYSICS_NAVIERSTOKES, "navierstokes", true, true, 0, 1, FIELDS_REFUSED, 0, 1},
    {MHA_PHYSICS_SHALLOWWATER_HYBRIDIZED, "shallowwaterHybridized", true, false, 0, 1, FIELDS_REFUSED, 0, 1},
    {MHA_PHYSICS_NAVIERSTOKES_THERMAL, "navierstokes+thermal", true, true, 0, 1, FIELDS_REFUSED, 0, 1},
    {MHA_PHYSICS_LINEARELASTICITY, "linearelasticity", true, true, 0, 1, FIELDS_REFUSED, 0, 1},
    {MHA_PHYSICS_LINEARELASTICITY_THERMAL, "linearelasticity+thermal", true, true, 0, 1, FIELDS_REFUSED, 0, 1},
    {MHA_PHYSICS_CDR, "cdr", true, true, 0, 1, 2, 0, 1},
    {MHA_PHYSICS_NAVIERSTOKES_CDR, "navierstokes+cdr", true, true, 0, 1, 2, 0, 1},
    {MHA_PHYSICS_HELMHOLTZ, "helmholtz", true, true, 0, 1, FIELDS_REFUSED, 0, 1},
};

int failures = 0;
void fail(const std::string &what) {
  std::printf("MISMATCH: %s\n", what.c_str());
  ++failures;
}

// the pair dispatch_module hands over, or (0, 0) and the refusal's text
std::pair<int, int> module_of(int dim, int physics, const char *what, std::string *refusal) {
  std::pair<int, int> got(0, 0);
  refusal->clear();
  try {
    dispatch_module(dim, physics, what, [&](auto d, auto p) { got = {decltype(d)::value, decltype(p)::value}; });
  } catch (const Error &e) {
    if (e.code != MHA_ERR_INVALID) fail("refusal with code " + std::to_string(e.code));
    *refusal = e.what();
  }
  return got;
}

// EXPR for module `physics` (2-D) with these parameters, FIELDS_REFUSED / HET_REFUSED for the two refusals; also checks
// the layout of the pair against itself and against one with a variable more
int expr_of(const PhysParamsDev &pp) {
  int got = -99;
  std::string refusal;
  try {
    dispatch_module(2, pp.physics, "point-engine", [&](auto d, auto p) {
      constexpr int DIM = decltype(d)::value, PHYS = decltype(p)::value;
      dispatch_expr<PHYS>(pp, [&](auto e) { got = decltype(e)::value; });
      using L = Layout<PHYS, DIM>;
      VarLayoutDev vl;
      vl.nvars = L::nvars;
      vl.ns_tot = L::NS;
      for (int v = 0; v < L::nvars; ++v) vl.type[v] = L::type(v);
      require_layout<PHYS, DIM>(vl);
      vl.nvars += 1;
      try {
        require_layout<PHYS, DIM>(vl);
        fail("a layout with a variable too many passes");
      } catch (const Error &) {
      }
    });
  } catch (const Error &e) {
    if (e.code != MHA_ERR_INVALID) fail("refusal with code " + std::to_string(e.code));
    refusal = e.what();
    if (refusal == kFieldsRefusal) return FIELDS_REFUSED;
    if (refusal == kHetRefusal) return HET_REFUSED;
    fail("unknown refusal: " + refusal);
  }
  return got;
}

PhysParamsDev params(int physics, bool deck, bool fields, bool het) {
  PhysParamsDev pp;
  pp.physics = physics;
  if (deck) {
    pp.f[3].kind = MHA_FUNC_EXPRESSION;
    pp.f[3].uses_fields = fields ? 1 : 0;
  }
  if (het) pp.het.kl = 1;
  return pp;
}

void expect_expr(const Row &r, const char *situation, const PhysParamsDev &pp, int want) {
  const int got = expr_of(pp);
  if (got != want)
    fail(std::string(r.name) + ", " + situation + ": EXPR " + std::to_string(got) + ", table " + std::to_string(want));
}

}  // namespace

int main() {
  std::string refusal;
  int pairs = 0;
  for (const Row &r : kTable) {
    for (int dim = 2; dim <= 3; ++dim) {
      const bool exists = dim == 2 ? r.in2d : r.in3d;
      pairs += exists;
      for (const char *what : {"Jacobian-product", "Jacobian-diagonal", "point-engine"}) {
        const std::pair<int, int> got = module_of(dim, r.physics, what, &refusal);
        const std::string text = std::string("no ") + what + " kernel for physics " + std::to_string(r.physics) + " in " +
                                 std::to_string(dim) + "-D";
        if (exists && (got.first != dim || got.second != r.physics))
          fail(std::string(r.name) + " in " + std::to_string(dim) + "-D reaches (" + std::to_string(got.first) + ", " +
               std::to_string(got.second) + ")" + refusal);
        if (!exists && (got.first != 0 || refusal != text)) fail(std::string(r.name) + ": refusal '" + refusal + "'");
      }
      // the engine's mass mode: module -physics, the refusal names the id as given
      const std::pair<int, int> mass = module_of(dim, -r.physics, "point-engine", &refusal);
      if (exists && (mass.first != dim || mass.second != r.physics)) fail(std::string(r.name) + ": mass mode");
      if (!exists && refusal != "no point-engine kernel for physics " + std::to_string(-r.physics) + " in " +
                                    std::to_string(dim) + "-D")
        fail(std::string(r.name) + ": mass-mode refusal '" + refusal + "'");
    }
    expect_expr(r, "plain", params(r.physics, false, false, false), r.plain);
    expect_expr(r, "deck string", params(r.physics, true, false, false), r.deck);
    expect_expr(r, "deck string reading the fields", params(r.physics, true, true, false), r.fields);
    expect_expr(r, "heterogeneous", params(r.physics, false, false, true), r.het);
    expect_expr(r, "heterogeneous + deck string", params(r.physics, true, false, true), r.het_deck);
    {  // element data in place of the KL field: the same two answers
      PhysParamsDev pp = params(r.physics, false, false, false);
      static const double one = 1.0;
      pp.het.edata = &one;
      expect_expr(r, "element data", pp, r.het);
      pp.f[0].kind = MHA_FUNC_EXPRESSION;
      expect_expr(r, "element data + deck string", pp, r.het_deck);
    }
    // mass mode evaluates no function: deck strings, field-reading ones included, do not choose the variant
    expect_expr(r, "mass mode + deck string reading the fields", params(-r.physics, true, true, false), r.plain);
  }
  if (pairs != 19) fail("the table holds " + std::to_string(pairs) + " pairs, not 19");
  // ids and dimensions outside the table
  for (const std::pair<int, int> &dp : std::vector<std::pair<int, int>>{{2, 0}, {2, 11}, {3, 99}, {1, 1}, {4, 1}}) {
    const std::pair<int, int> got = module_of(dp.first, dp.second, "Jacobian-product", &refusal);
    if (got.first != 0 || refusal != "no Jacobian-product kernel for physics " + std::to_string(dp.second) + " in " +
                                         std::to_string(dp.first) + "-D")
      fail("(" + std::to_string(dp.first) + ", " + std::to_string(dp.second) + ") reaches a kernel or refuses with '" +
           refusal + "'");
  }
  if (!failures) std::printf("ok\n");
  return failures ? 1 : 0;
}
