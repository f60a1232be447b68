// engine_dispatch.hpp -- the host side that the launchers of the point-function kernels share (point_engine.hip,
// jacobian_apply.hip, jacobian_apply_multi.hip, jacobian_diagonal.hip): the list of (dimension, module) pairs that have
// a point function, the check of the host's variable layout against the module's, the choice of the EXPR variant, the
// preparation of a kernel that may spill and wants the large LDS, and the launch geometry of the one-wavefront-per-
// element kernels.  dispatch_module, require_layout and dispatch_expr call nothing of the HIP runtime: the table they
// state is checked on the host alone (tests/dispatch_table_check.cpp).
//
// A new module with a point function: its Layout (engine_points.hpp), its line in MHA_MODULE_POINT (same file), its
// lines in MHA_POINT_MODULES below and, if its point function has a form for deck strings that read the solution
// fields, its entry in has_field_form.
#pragma once
#include <algorithm>
#include <type_traits>

#include "../common.hpp"
#include "device_math.hpp"
#include "engine_points.hpp"

namespace mha {
namespace {

// LDS a workgroup of these kernels may ask for, and the wavefronts (= elements) a workgroup of the product kernels holds
// at most
constexpr size_t kPointLdsLimit = 160 * 1024;
constexpr int kProductMaxWaves = 8;

// every (dimension, module) pair with a point function; shallowwaterHybridized and shallowwater are 2-D only
#define MHA_POINT_MODULES(X)                  \
  X(2, MHA_PHYSICS_THERMAL)                   \
  X(3, MHA_PHYSICS_THERMAL)                   \
  X(2, MHA_PHYSICS_POROUS_MIXED)              \
  X(3, MHA_PHYSICS_POROUS_MIXED)              \
  X(2, MHA_PHYSICS_NAVIERSTOKES)              \
  X(3, MHA_PHYSICS_NAVIERSTOKES)              \
  X(2, MHA_PHYSICS_NAVIERSTOKES_THERMAL)      \
  X(3, MHA_PHYSICS_NAVIERSTOKES_THERMAL)      \
  X(2, MHA_PHYSICS_LINEARELASTICITY)          \
  X(3, MHA_PHYSICS_LINEARELASTICITY)          \
  X(2, MHA_PHYSICS_LINEARELASTICITY_THERMAL)  \
  X(3, MHA_PHYSICS_LINEARELASTICITY_THERMAL)  \
  X(2, MHA_PHYSICS_CDR)                       \
  X(3, MHA_PHYSICS_CDR)                       \
  X(2, MHA_PHYSICS_NAVIERSTOKES_CDR)          \
  X(3, MHA_PHYSICS_NAVIERSTOKES_CDR)          \
  X(2, MHA_PHYSICS_HELMHOLTZ)                 \
  X(3, MHA_PHYSICS_HELMHOLTZ)                 \
  X(2, MHA_PHYSICS_POROUS_WEAK_GALERKIN)      \
  X(3, MHA_PHYSICS_POROUS_WEAK_GALERKIN)      \
  X(2, MHA_PHYSICS_SHALLOWWATER_HYBRIDIZED)   \
  X(2, MHA_PHYSICS_STOKES)                    \
  X(3, MHA_PHYSICS_STOKES)                    \
  X(2, MHA_PHYSICS_SHALLOWWATER)

// f(integral_constant<int, DIM>, integral_constant<int, PHYS>) for the pair (dim, |physics|); refuses any other pair
// with "no <what> kernel for physics ...".  physics < 0 is the engine's mass mode of module -physics.
template <class F>
void dispatch_module(int dim, int physics, const char *what, F &&f) {
  static_assert(MHA_PHYSICS_HELMHOLTZ < 100 && MHA_PHYSICS_POROUS_WEAK_GALERKIN < 100 && MHA_PHYSICS_STOKES < 100 &&
                    MHA_PHYSICS_SHALLOWWATER < 100,
                "the switch key holds two decimal digits of module id");
#define MHA_MODULE_CASE(D, P) \
  case D * 100 + P: f(std::integral_constant<int, D>{}, std::integral_constant<int, P>{}); break;
  switch (dim * 100 + (physics < 0 ? -physics : physics)) {
    MHA_POINT_MODULES(MHA_MODULE_CASE)
    default: MHA_REQUIRE(false, MHA_ERR_INVALID, "no " << what << " kernel for physics " << physics << " in " << dim << "-D");
  }
#undef MHA_MODULE_CASE
}

// the host's variable layout is the module's
template <int PHYS, int DIM>
void require_layout(const VarLayoutDev &vl) {
  using L = Layout<PHYS, DIM>;
  MHA_REQUIRE(vl.nvars == L::nvars && vl.ns_tot == L::NS, MHA_ERR_INVALID,
              "variable layout does not match the physics module (" << vl.nvars << " variables, " << vl.ns_tot
                                                                    << " slots)");
  for (int v = 0; v < L::nvars; ++v)
    MHA_REQUIRE(vl.type[v] == L::type(v), MHA_ERR_INVALID, "basis type of variable " << v << " does not match the module");
}

// the modules whose point function has an EXPR = 2 form (deck strings that read the solution fields)
template <int PHYS>
constexpr bool has_field_form() {
  return PHYS == MHA_PHYSICS_THERMAL || PHYS == MHA_PHYSICS_CDR || PHYS == MHA_PHYSICS_NAVIERSTOKES_CDR;
}

// f(integral_constant<int, EXPR>) with the variant of the point function that pp asks for: 2 deck strings that read
// the solution fields / 3 porousMixed with heterogeneous permeability / 1 deck strings / 0 plain.  Deck strings count
// for a module only (physics > 0): the engine's mass mode evaluates none.  f is instantiated with the variants the
// module has, no others.  porousWeakGalerkin reads its element data at run time inside variants 0 and 1 (one test of a
// kernel argument per point), so it carries element data and deck strings together and has no variant of its own.
template <int PHYS, class F>
void dispatch_expr(const PhysParamsDev &pp, F &&f) {
  const bool module = pp.physics > 0;
  if (module && uses_fields(pp)) {
    if constexpr (has_field_form<PHYS>()) {
      f(std::integral_constant<int, 2>{});
    } else {
      MHA_REQUIRE(false, MHA_ERR_INVALID, "functions of the solution fields are built for the thermal module");
    }
  } else if (PHYS == MHA_PHYSICS_POROUS_MIXED && (pp.het.edata || pp.het.kl)) {
    if constexpr (PHYS == MHA_PHYSICS_POROUS_MIXED) {
      MHA_REQUIRE(!has_expression(pp), MHA_ERR_INVALID,
                  "porousMixed: heterogeneous permeability with deck-string functions is not built; give source / mobility as constants or closed forms");
      f(std::integral_constant<int, 3>{});
    }
  } else if (module && has_expression(pp)) {
    // deck-string functions: the interpreter costs registers and scratch, so only these instantiations carry it
    f(std::integral_constant<int, 1>{});
  } else {
    f(std::integral_constant<int, 0>{});
  }
}

// before the launch of a kernel that can spill and takes its LDS dynamically: the scratch it needs is one the runtime
// can back, and it may ask for the whole limit
template <class Kernel>
void prepare_kernel(Kernel kern, const char *what) {
  require_modest_scratch(kern, what);
  MHA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              static_cast<int>(kPointLdsLimit)));
}

// wavefronts (= elements) a workgroup holds when each needs per_wave bytes of LDS beside the tables; 0: not one
inline int waves_that_fit(size_t tables, size_t per_wave) {
  if (tables + per_wave > kPointLdsLimit) return 0;
  return static_cast<int>(std::min<size_t>(kProductMaxWaves, (kPointLdsLimit - tables) / per_wave));
}

inline void require_wave_fits(size_t tables, size_t per_wave) {
  MHA_REQUIRE(tables + per_wave <= kPointLdsLimit, MHA_ERR_INVALID,
              "element needs " << tables + per_wave << " B of LDS (limit 160 KB)");
}

// launch geometry of the one-wavefront-per-element kernels: as many wavefronts per workgroup as the LDS holds beside
// the tables, eight at most; a persistent grid of up to four workgroups per CU
struct WaveLaunch {
  int nw;      // wavefronts per workgroup
  size_t lds;  // bytes per workgroup
  int grid;
};
inline WaveLaunch wave_launch(size_t tables, size_t per_wave, int e_count) {
  require_wave_fits(tables, per_wave);
  WaveLaunch g;
  g.nw = waves_that_fit(tables, per_wave);
  g.lds = tables + g.nw * per_wave;
  const int per_cu = static_cast<int>(std::max<size_t>(1, std::min<size_t>(size_t(4), kPointLdsLimit / g.lds)));
  g.grid = std::max(1, std::min((e_count + g.nw - 1) / g.nw, current_device_num_cus() * per_cu));
  return g;
}

}  // namespace
}  // namespace mha
