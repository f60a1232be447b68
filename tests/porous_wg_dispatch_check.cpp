// porous_wg_dispatch_check.cpp -- host-only check of kernels/engine_dispatch.hpp for porousWeakGalerkin, beside
// dispatch_table_check.cpp (which pins the ten earlier modules): the pairs (2, 13) and (3, 13) reach their kernels under
// every launcher's name and in mass mode, the module's layout is pint (HVOL), u, t (HDIV) with 3 + 2 dim slots, and
// dispatch_expr hands it variant 0 without and 1 with deck strings -- element data chooses no variant of its own and may
// stand beside deck strings --, and refuses deck strings that read the solution fields.  No HIP runtime call.  Prints "ok"
// and returns 0, or one line per mismatch and 1.
#include <cstdio>
#include <string>

#include "../mrhyde_amd/csrc/kernels/engine_dispatch.hpp"

using namespace mha;

namespace {

int failures = 0;
void fail(const std::string &what) {
  std::printf("MISMATCH: %s\n", what.c_str());
  ++failures;
}

constexpr int FIELDS_REFUSED = -1;

int expr_of(int dim, const PhysParamsDev &pp) {
  int got = -99;
  try {
    dispatch_module(dim, pp.physics, "point-engine", [&](auto d, auto p) {
      constexpr int DIM = decltype(d)::value, PHYS = decltype(p)::value;
      if (DIM != dim || PHYS != MHA_PHYSICS_POROUS_WEAK_GALERKIN) fail("the pair reaches another kernel");
      dispatch_expr<PHYS>(pp, [&](auto e) { got = decltype(e)::value; });
    });
  } catch (const Error &e) {
    if (e.code != MHA_ERR_INVALID) fail("refusal with code " + std::to_string(e.code));
    if (std::string(e.what()) == "functions of the solution fields are built for the thermal module") return FIELDS_REFUSED;
    fail(std::string("unknown refusal: ") + e.what());
  }
  return got;
}

void expect(int dim, const char *situation, const PhysParamsDev &pp, int want) {
  const int got = expr_of(dim, pp);
  if (got != want)
    fail(std::to_string(dim) + "-D, " + situation + ": EXPR " + std::to_string(got) + ", expected " + std::to_string(want));
}

template <int DIM>
void check_layout() {
  using L = Layout<MHA_PHYSICS_POROUS_WEAK_GALERKIN, DIM>;
  static_assert(L::nvars == 3 && L::NS == 3 + 2 * DIM, "pint, u, t: 1 + 2 (dim + 1) slots");
  static_assert(L::type(0) == MHA_BASIS_HVOL && L::type(1) == MHA_BASIS_HDIV && L::type(2) == MHA_BASIS_HDIV, "");
  static_assert(slotptr_of<L, DIM>(1) == 1 && slotptr_of<L, DIM>(2) == 2 + DIM, "slots pint, u_x.., div u, t_x.., div t");
  VarLayoutDev vl;
  vl.nvars = 3;
  vl.ns_tot = 3 + 2 * DIM;
  vl.type[0] = MHA_BASIS_HVOL;
  vl.type[1] = vl.type[2] = MHA_BASIS_HDIV;
  require_layout<MHA_PHYSICS_POROUS_WEAK_GALERKIN, DIM>(vl);
  vl.type[2] = MHA_BASIS_HGRAD;
  try {
    require_layout<MHA_PHYSICS_POROUS_WEAK_GALERKIN, DIM>(vl);
    fail("a layout with t in HGRAD passes");
  } catch (const Error &) {
  }
}

}  // namespace

int main() {
  static_assert(MHA_PHYSICS_POROUS_WEAK_GALERKIN == 13, "the module's id");
  static const double one = 1.0;
  for (int dim = 2; dim <= 3; ++dim) {
    for (const char *what : {"Jacobian-product", "Jacobian-diagonal", "point-engine"})
      for (int sign : {1, -1}) {
        int d_got = 0, p_got = 0;
        try {
          dispatch_module(dim, sign * MHA_PHYSICS_POROUS_WEAK_GALERKIN, what, [&](auto d, auto p) {
            d_got = decltype(d)::value;
            p_got = decltype(p)::value;
          });
        } catch (const Error &e) {
          fail(std::string("refused: ") + e.what());
        }
        if (d_got != dim || p_got != MHA_PHYSICS_POROUS_WEAK_GALERKIN)
          fail(std::string(what) + " in " + std::to_string(dim) + "-D reaches (" + std::to_string(d_got) + ", " + std::to_string(p_got) + ")");
      }
    PhysParamsDev pp;
    pp.physics = MHA_PHYSICS_POROUS_WEAK_GALERKIN;
    expect(dim, "plain", pp, 0);
    pp.het.edata = &one;
    expect(dim, "element data", pp, 0);
    pp.f[0].kind = MHA_FUNC_EXPRESSION;
    expect(dim, "element data + deck string", pp, 1);
    pp.het.edata = nullptr;
    expect(dim, "deck string", pp, 1);
    pp.f[0].uses_fields = 1;
    expect(dim, "deck string reading the fields", pp, FIELDS_REFUSED);
    pp.physics = -MHA_PHYSICS_POROUS_WEAK_GALERKIN;
    expect(dim, "mass mode + deck string reading the fields", pp, 0);
  }
  check_layout<2>();
  check_layout<3>();
  // 1-D has no kernel
  try {
    dispatch_module(1, MHA_PHYSICS_POROUS_WEAK_GALERKIN, "point-engine", [&](auto, auto) { fail("1-D reaches a kernel"); });
    fail("1-D is not refused");
  } catch (const Error &e) {
    if (std::string(e.what()) != "no point-engine kernel for physics 13 in 1-D") fail(std::string("1-D refusal: ") + e.what());
  }
  if (!failures) std::printf("ok\n");
  return failures ? 1 : 0;
}
