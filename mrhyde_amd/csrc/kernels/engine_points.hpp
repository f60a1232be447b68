// engine_points.hpp -- what the kernels that run the modules' point functions share (point_engine.hip: element matrix
// and residual; jacobian_apply.hip: matrix-free products with the same Jacobian): the static variable layout of every
// module, the geometric block G between reference and physical slots, the geometry of an integration point, and the
// dispatch to the point functions of physics_points.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "physics_points.hpp"

namespace mha {
namespace {

// static variable layout of a module (must agree with the host's VarLayoutDev; checked in the launcher)
template <int PHYS, int DIM>
struct Layout;
template <int DIM>
struct Layout<MHA_PHYSICS_THERMAL, DIM> {
  static constexpr int nvars = 1, NS = 1 + DIM;
  __host__ __device__ static constexpr int type(int) { return MHA_BASIS_HGRAD; }
};
template <int DIM>
struct Layout<MHA_PHYSICS_POROUS_MIXED, DIM> {
  static constexpr int nvars = 2, NS = 2 + DIM;
  __host__ __device__ static constexpr int type(int v) { return v == 0 ? MHA_BASIS_HVOL : MHA_BASIS_HDIV; }
};
template <int DIM>
struct Layout<MHA_PHYSICS_NAVIERSTOKES, DIM> {
  static constexpr int nvars = 1 + DIM, NS = (1 + DIM) * (1 + DIM);
  __host__ __device__ static constexpr int type(int) { return MHA_BASIS_HGRAD; }
};

// navierstokes + thermal on one block: ux, pr, uy[, uz], e
template <int DIM>
struct Layout<MHA_PHYSICS_NAVIERSTOKES_THERMAL, DIM> {
  static constexpr int nvars = 2 + DIM, NS = (2 + DIM) * (1 + DIM);
  __host__ __device__ static constexpr int type(int) { return MHA_BASIS_HGRAD; }
};

// linearelasticity: dx, dy[, dz]
template <int DIM>
struct Layout<MHA_PHYSICS_LINEARELASTICITY, DIM> {
  static constexpr int nvars = DIM, NS = DIM * (1 + DIM);
  __host__ __device__ static constexpr int type(int) { return MHA_BASIS_HGRAD; }
};

// linearelasticity + thermal: dx, dy[, dz], e
template <int DIM>
struct Layout<MHA_PHYSICS_LINEARELASTICITY_THERMAL, DIM> {
  static constexpr int nvars = DIM + 1, NS = (DIM + 1) * (1 + DIM);
  static_assert(NS <= kMaxSlots, "");
  __host__ __device__ static constexpr int type(int) { return MHA_BASIS_HGRAD; }
};

// cdr: c
template <int DIM>
struct Layout<MHA_PHYSICS_CDR, DIM> {
  static constexpr int nvars = 1, NS = 1 + DIM;
  __host__ __device__ static constexpr int type(int) { return MHA_BASIS_HGRAD; }
};

// navierstokes + cdr on one block: ux, pr, uy[, uz], c
template <int DIM>
struct Layout<MHA_PHYSICS_NAVIERSTOKES_CDR, DIM> {
  static constexpr int nvars = 2 + DIM, NS = (2 + DIM) * (1 + DIM);
  static_assert(NS <= kMaxSlots, "");
  __host__ __device__ static constexpr int type(int) { return MHA_BASIS_HGRAD; }
};

// helmholtz: ureal, uimag
template <int DIM>
struct Layout<MHA_PHYSICS_HELMHOLTZ, DIM> {
  static constexpr int nvars = 2, NS = 2 * (1 + DIM);
  __host__ __device__ static constexpr int type(int) { return MHA_BASIS_HGRAD; }
};

template <int DIM>
struct Layout<MHA_PHYSICS_SHALLOWWATER_HYBRIDIZED, DIM> {
  static constexpr int nvars = 3, NS = 3 * (1 + DIM);
  __host__ __device__ static constexpr int type(int) { return MHA_BASIS_HGRAD; }
};

__host__ __device__ constexpr int slots_of(int type, int dim) { return type == MHA_BASIS_HVOL ? 1 : 1 + dim; }
// slots that carry a time derivative: every value, not gradients / divergence
__host__ __device__ constexpr bool value_like(int type, int s, int dim) {
  return type == MHA_BASIS_HDIV ? s < dim : s == 0;
}

template <class L, int DIM>
__host__ __device__ constexpr int slotptr_of(int v) {
  int p = 0;
  for (int k = 0; k < v; ++k) p += slots_of(L::type(k), DIM);
  return p;
}

// physical slot values from reference slot values (one variable): G ref
template <int DIM>
__device__ __forceinline__ void to_phys(int type, const double *ref, const double *J, const double *Ji, double det,
                                        double *phys) {
  if (type == MHA_BASIS_HVOL) {
    phys[0] = ref[0];
  } else if (type == MHA_BASIS_HGRAD) {
    phys[0] = ref[0];
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; ++c) s += Ji[c * DIM + d] * ref[1 + c];
      phys[1 + d] = s;
    }
  } else {
    const double r = 1.0 / det;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; ++c) s += J[d * DIM + c] * ref[c];
      phys[d] = s * r;
    }
    phys[DIM] = ref[DIM] * r;
  }
}

// reference-slot coefficients from physical-slot coefficients: G^T phys
template <int DIM>
__device__ __forceinline__ void to_ref_T(int type, const double *phys, const double *J, const double *Ji, double det,
                                         double *ref) {
  if (type == MHA_BASIS_HVOL) {
    ref[0] = phys[0];
  } else if (type == MHA_BASIS_HGRAD) {
    ref[0] = phys[0];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < DIM; ++d) s += Ji[c * DIM + d] * phys[1 + d];
      ref[1 + c] = s;
    }
  } else {
    const double r = 1.0 / det;
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < DIM; ++d) s += J[d * DIM + c] * phys[d];
      ref[c] = s * r;
    }
    ref[DIM] = phys[DIM] * r;
  }
}

// orders a wave's LDS writes before its later LDS reads (data private to the wave: no workgroup barrier needed)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int DIM>
constexpr int geo_size() { return 2 * DIM * DIM + 2 + DIM; }  // J, Ji, det, w, x

// geometry of integration point q of element e, stored at g: J, Ji, det, w = reference weight x det, x (geo_size<DIM>()
// doubles).  A macro, expanded inside the kernels' point loops: as an inlined function the same statements left every
// point_engine_kernel with other register counts (thermal 2-D, 128 threads per element: 181 VGPRs against 201), and the
// engine's kernels are to stay what they were.  Needs DIM in scope.
#define MHA_POINT_GEOMETRY(b, e, q, NQ, g_out)                                                              \
  do {                                                                                                      \
    const double *xn = (b).nodes + (size_t)(e) * (1 << DIM) * DIM;                                          \
    double J[DIM * DIM], Ji[DIM * DIM], det, x[DIM];                                                        \
    _Pragma("unroll") for (int r = 0; r < DIM; ++r) {                                                       \
      _Pragma("unroll") for (int c = 0; c < DIM; ++c) {                                                     \
        double sum = 0.0;                                                                                   \
        for (int k = 0; k < (1 << DIM); ++k) sum += xn[k * DIM + r] * (b).nodegrad[(k * (NQ) + (q)) * DIM + c]; \
        J[r * DIM + c] = sum;                                                                               \
      }                                                                                                     \
      double sum = 0.0;                                                                                     \
      for (int k = 0; k < (1 << DIM); ++k) sum += xn[k * DIM + r] * (b).nodeval[k * (NQ) + (q)];            \
      x[r] = sum;                                                                                           \
    }                                                                                                       \
    invert<DIM>(J, Ji, det);                                                                                \
    double *g = (g_out);                                                                                    \
    _Pragma("unroll") for (int k = 0; k < DIM * DIM; ++k) { g[k] = J[k]; g[DIM * DIM + k] = Ji[k]; }        \
    g[2 * DIM * DIM] = det;                                                                                 \
    g[2 * DIM * DIM + 1] = (b).ref_wts[q] * det;                                                            \
    _Pragma("unroll") for (int d = 0; d < DIM; ++d) g[2 * DIM * DIM + 2 + d] = x[d];                        \
  } while (0)

}  // namespace
}  // namespace mha

// the module's point function.  EXPR: 0 / 1 deck strings / 2 deck strings that read the solution fields (thermal, cdr,
// navierstokes+cdr) / 3 porousMixed with heterogeneous permeability (no deck strings).  A macro for the same reason as
// the geometry: behind one more inlined function the deck-string instantiations of navierstokes + cdr came out with
// other spills.  Needs DIM, PHYS and EXPR in scope.
#define MHA_MODULE_POINT(pa, F)                                                                                          \
  do {                                                                                                                   \
    if constexpr (PHYS == MHA_PHYSICS_THERMAL) thermal_point<DIM, EXPR>(pa, F);                                          \
    else if constexpr (PHYS == MHA_PHYSICS_POROUS_MIXED) porous_point<DIM, (EXPR == 1), (EXPR == 3)>(pa, F);             \
    else if constexpr (PHYS == MHA_PHYSICS_SHALLOWWATER_HYBRIDIZED) swhdg_point<DIM, (EXPR != 0)>(pa, F);                \
    else if constexpr (PHYS == MHA_PHYSICS_NAVIERSTOKES_THERMAL) navierstokes_thermal_point<DIM, (EXPR != 0)>(pa, F);    \
    else if constexpr (PHYS == MHA_PHYSICS_LINEARELASTICITY) linearelasticity_point<DIM, (EXPR != 0)>(pa, F);            \
    else if constexpr (PHYS == MHA_PHYSICS_LINEARELASTICITY_THERMAL) linearelasticity_thermal_point<DIM, (EXPR != 0)>(pa, F); \
    else if constexpr (PHYS == MHA_PHYSICS_CDR) cdr_point<DIM, EXPR>(pa, F);                                             \
    else if constexpr (PHYS == MHA_PHYSICS_NAVIERSTOKES_CDR) navierstokes_cdr_point<DIM, EXPR>(pa, F);                   \
    else if constexpr (PHYS == MHA_PHYSICS_HELMHOLTZ) helmholtz_point<DIM, (EXPR != 0)>(pa, F);                          \
    else navierstokes_point<DIM, (EXPR != 0)>(pa, F);                                                                    \
  } while (0)
