// stokes_shallowwater_dispatch_check.cpp -- host-only check of kernels/engine_dispatch.hpp for stokes and shallowwater,
// beside dispatch_table_check.cpp (which pins the ten earlier modules): the pairs (2, 14), (3, 14) and (2, 15) reach their
// kernels under every launcher's name and in mass mode, (3, 15) and (1, 14) are refused with the standing text, stokes has
// navierstokes' layout and shallowwater three HGRAD variables, dispatch_expr hands both variant 0 without and 1 with deck
// strings and refuses deck strings that read the solution fields.  No HIP runtime call.  Prints "ok" and returns 0, or one
// line per mismatch and 1.
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
  const int id = pp.physics < 0 ? -pp.physics : pp.physics;
  try {
    dispatch_module(dim, pp.physics, "point-engine", [&](auto d, auto p) {
      constexpr int DIM = decltype(d)::value, PHYS = decltype(p)::value;
      if (DIM != dim || PHYS != id) fail("the pair reaches another kernel");
      dispatch_expr<PHYS>(pp, [&](auto e) { got = decltype(e)::value; });
    });
  } catch (const Error &e) {
    if (e.code != MHA_ERR_INVALID) fail("refusal with code " + std::to_string(e.code));
    if (std::string(e.what()) == "functions of the solution fields are built for the thermal module") return FIELDS_REFUSED;
    fail(std::string("unknown refusal: ") + e.what());
  }
  return got;
}

void expect(int dim, int physics, const char *situation, const PhysParamsDev &pp, int want) {
  const int got = expr_of(dim, pp);
  if (got != want)
    fail("module " + std::to_string(physics) + " in " + std::to_string(dim) + "-D, " + situation + ": EXPR " +
         std::to_string(got) + ", expected " + std::to_string(want));
}

template <int PHYS, int DIM>
void check_layout(int nvars) {
  using L = Layout<PHYS, DIM>;
  if (L::nvars != nvars || L::NS != nvars * (1 + DIM)) fail("layout of module " + std::to_string(PHYS));
  VarLayoutDev vl;
  vl.nvars = nvars;
  vl.ns_tot = nvars * (1 + DIM);
  for (int v = 0; v < nvars; ++v) vl.type[v] = MHA_BASIS_HGRAD;
  require_layout<PHYS, DIM>(vl);
  vl.type[nvars - 1] = MHA_BASIS_HVOL;
  try {
    require_layout<PHYS, DIM>(vl);
    fail("a layout with an HVOL variable passes");
  } catch (const Error &) {
  }
}

void expect_refused(int dim, int physics, const char *what) {
  try {
    dispatch_module(dim, physics, what, [&](auto, auto) { fail("a pair outside the table reaches a kernel"); });
    fail("(" + std::to_string(dim) + ", " + std::to_string(physics) + ") is not refused");
  } catch (const Error &e) {
    const std::string text =
        std::string("no ") + what + " kernel for physics " + std::to_string(physics) + " in " + std::to_string(dim) + "-D";
    if (e.code != MHA_ERR_INVALID || text != e.what()) fail(std::string("refusal: ") + e.what());
  }
}

}  // namespace

int main() {
  static_assert(MHA_PHYSICS_STOKES == 14 && MHA_PHYSICS_SHALLOWWATER == 15, "the modules' ids");
  static_assert(Layout<MHA_PHYSICS_STOKES, 2>::NS == Layout<MHA_PHYSICS_NAVIERSTOKES, 2>::NS &&
                    Layout<MHA_PHYSICS_STOKES, 3>::NS == Layout<MHA_PHYSICS_NAVIERSTOKES, 3>::NS &&
                    Layout<MHA_PHYSICS_STOKES, 3>::nvars == Layout<MHA_PHYSICS_NAVIERSTOKES, 3>::nvars,
                "stokes runs on navierstokes' layout");
  const int pairs[3][2] = {{2, MHA_PHYSICS_STOKES}, {3, MHA_PHYSICS_STOKES}, {2, MHA_PHYSICS_SHALLOWWATER}};
  for (const auto &dp : pairs) {
    const int dim = dp[0], physics = dp[1];
    for (const char *what : {"Jacobian-product", "Jacobian-diagonal", "point-engine"})
      for (int sign : {1, -1}) {
        int d_got = 0, p_got = 0;
        try {
          dispatch_module(dim, sign * physics, what, [&](auto d, auto p) {
            d_got = decltype(d)::value;
            p_got = decltype(p)::value;
          });
        } catch (const Error &e) {
          fail(std::string("refused: ") + e.what());
        }
        if (d_got != dim || p_got != physics)
          fail(std::string(what) + " in " + std::to_string(dim) + "-D reaches (" + std::to_string(d_got) + ", " +
               std::to_string(p_got) + ")");
      }
    PhysParamsDev pp;
    pp.physics = physics;
    expect(dim, physics, "plain", pp, 0);
    pp.f[1].kind = MHA_FUNC_EXPRESSION;
    expect(dim, physics, "deck string", pp, 1);
    pp.f[1].uses_fields = 1;
    expect(dim, physics, "deck string reading the fields", pp, FIELDS_REFUSED);
    pp.physics = -physics;
    expect(dim, physics, "mass mode + deck string reading the fields", pp, 0);
  }
  check_layout<MHA_PHYSICS_STOKES, 2>(3);
  check_layout<MHA_PHYSICS_STOKES, 3>(4);
  check_layout<MHA_PHYSICS_SHALLOWWATER, 2>(3);
  for (const char *what : {"Jacobian-product", "Jacobian-diagonal", "point-engine"}) {
    expect_refused(3, MHA_PHYSICS_SHALLOWWATER, what);
    expect_refused(3, -MHA_PHYSICS_SHALLOWWATER, what);
    expect_refused(1, MHA_PHYSICS_STOKES, what);
    expect_refused(1, MHA_PHYSICS_SHALLOWWATER, what);
  }
  if (!failures) std::printf("ok\n");
  return failures ? 1 : 0;
}
