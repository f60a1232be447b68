// engine_points.hpp -- the device side that the kernels running the modules' point functions share (point_engine.hip:
// element matrix and residual; jacobian_apply.hip, jacobian_apply_multi.hip: matrix-free products with the same
// Jacobian; jacobian_diagonal.hip: its diagonal): the static variable layout of every module, the geometric block G
// between reference and physical slots, the geometry of an integration point, the dispatch to the point functions of
// physics_points.hpp, and -- as macros, see below -- the statements the four element loops have in common: var_at, the
// element range of a wave, the dof gather's row and sign, the reference-slot fields, the element size, the phase-3
// seeding, the point function's arguments and the back-transform.  The host side of the same kernels is
// engine_dispatch.hpp.
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

// porousWeakGalerkin: pint, u, t (pbndry, the HFACE trace, is data of the element step)
template <int DIM>
struct Layout<MHA_PHYSICS_POROUS_WEAK_GALERKIN, DIM> {
  static constexpr int nvars = 3, NS = 3 + 2 * DIM;
  __host__ __device__ static constexpr int type(int v) { return v == 0 ? MHA_BASIS_HVOL : MHA_BASIS_HDIV; }
};

// stokes: ux, pr, uy[, uz] -- navierstokes' layout
template <int DIM>
struct Layout<MHA_PHYSICS_STOKES, DIM> {
  static constexpr int nvars = 1 + DIM, NS = (1 + DIM) * (1 + DIM);
  __host__ __device__ static constexpr int type(int) { return MHA_BASIS_HGRAD; }
};

// shallowwater: H, Hu, Hv
template <int DIM>
struct Layout<MHA_PHYSICS_SHALLOWWATER, DIM> {
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

// ---- statements the four kernels share, as text ----
// Macros, not functions, and with the index expressions the kernels had (s_Uh[q * NS + sp + sl], not a pointer advanced
// to the point first): moved into an inlined function template the seeding loop changed the resource usage of 17 of
// jacobian_diagonal.hip's kernels; as these macros every kernel of the four files compiles to the instructions it had
// before they were shared.  Each names what it needs in scope; all need L, DIM and NS.

// layout of the variable that holds slot m / dof f: declares VarAt and var_at(key, by_slot).  The loop runs over the
// module's compile-time variable count, so the layout arrays are indexed statically (kernel arguments in scalar
// registers); indexed by a run-time variable number they are memory loads, one dependent on the other, in every phase
// of every element.  Needs vl.
#define MHA_VAR_AT()                                                                                                     \
  struct VarAt { int sp, nsl, card, cp, vp, to; };                                                                       \
  auto var_at = [&](int key, bool by_slot) {                                                                             \
    VarAt r = {vl.slotptr[0], vl.nslot[0], vl.card[0], vl.cardpad[0], vl.varptr[0], vl.table_off[0]};                    \
    _Pragma("unroll") for (int k = 1; k < L::nvars; ++k)                                                                 \
      if (key >= (by_slot ? vl.slotptr[k] : vl.varptr[k]))                                                               \
        r = {vl.slotptr[k], vl.nslot[k], vl.card[k], vl.cardpad[k], vl.varptr[k], vl.table_off[k]};                      \
    return r;                                                                                                            \
  }

// blocked element ranges per wave (wave `wave` of NW in the workgroup): waves running at the same time work far apart
// in the mesh.  Declares el_begin, el_end.  Needs b.
#define MHA_WAVE_ELEMENT_RANGE(NW, wave)                                                                                 \
  const int nwaves = gridDim.x * (NW), gid = blockIdx.x * (NW) + (wave);                                                 \
  const int chunk = (b.e_count + nwaves - 1) / nwaves;                                                                   \
  const int el_begin = gid * chunk, el_end = min(b.e_count, el_begin + chunk)

// dof f of element e: declares pos, row and the orientation sign sg.  Needs b, vl, e, n.
#define MHA_DOF_ROW(f)                                                                                                   \
  const int pos = b.offsets[f], row = b.lids[(size_t)e * n + pos];                                                       \
  const double sg = vl.orient ? (double)vl.orient[(size_t)e * n + f] : 1.0

// work item idx = (point q, slot m) of phase 2: declares q, m, va, sl, card and T, the table row of (q, m).  Needs tab,
// var_at.
#define MHA_REF_SLOT(idx)                                                                                                \
  const int q = (idx) / NS, m = (idx) - q * NS;                                                                          \
  const VarAt va = var_at(m, true);                                                                                      \
  const int sl = m - va.sp, card = va.card;                                                                              \
  const double *T = tab + va.to + (q * va.nsl + sl) * va.cp

// U^(q,m), Udot^(q,m) of the item MHA_REF_SLOT(idx) opened.  Needs s_u, s_ud, s_Uh, s_Udh, tm.
#define MHA_REF_FIELDS(idx)                                                                                              \
  do {                                                                                                                   \
    const double *uu = s_u + va.vp, *ud = s_ud + va.vp;                                                                  \
    double a = 0.0, ad = 0.0;                                                                                            \
    if (tm.transient) {                                                                                                  \
      _Pragma("unroll 4") for (int dof = 0; dof < card; ++dof) {                                                         \
        a += uu[dof] * T[dof];                                                                                           \
        ad += ud[dof] * T[dof];                                                                                          \
      }                                                                                                                  \
    } else { /* steady: the time-derivative coefficients are zero */                                                     \
      _Pragma("unroll 4") for (int dof = 0; dof < card; ++dof) a += uu[dof] * T[dof];                                    \
    }                                                                                                                    \
    s_Uh[idx] = a;                                                                                                       \
    s_Udh[idx] = ad;                                                                                                     \
  } while (0)

// element size: declares h.  Workset::getElementSize (workset.cpp:2666-2679).  Needs s_geo, NQ, GEO.
#define MHA_ELEMENT_SIZE()                                                                                               \
  double vol = 0.0;                                                                                                      \
  for (int q = 0; q < NQ; ++q) vol += s_geo[q * GEO + 2 * DIM * DIM + 1];                                                \
  const double h = (DIM == 2) ? sqrt(vol) : cbrt(vol)

// geometry of point q as phase 3 reads it: declares g, J, Ji, det, w.  Needs s_geo, GEO, q.
#define MHA_POINT_GEO()                                                                                                  \
  const double *g = s_geo + q * GEO;                                                                                     \
  const double *J = g, *Ji = g + DIM * DIM;                                                                              \
  const double det = g[2 * DIM * DIM], w = g[2 * DIM * DIM + 1]

// seeding of phase 3: fills U, Ud (Dual[NS], in scope) with the physical fields at point q, derivative parts along the
// direction whose reference slot sp + sl is DIR -- an expression in q, m, sp, sl (the unit direction m:
// (m == sp + sl) ? 1.0 : 0.0).
// Needs s_Uh, s_Udh, q, tm and MHA_POINT_GEO.
#define MHA_SEED_POINT(DIR)                                                                                              \
  _Pragma("unroll") for (int v = 0; v < L::nvars; ++v) {                                                                 \
    const int type = L::type(v), sp = slotptr_of<L, DIM>(v), ns = slots_of(type, DIM);                                   \
    double ref[1 + DIM], phys[1 + DIM], refd[1 + DIM], physd[1 + DIM], dir[1 + DIM], pdir[1 + DIM];                      \
    _Pragma("unroll") for (int sl = 0; sl < ns; ++sl) {                                                                  \
      ref[sl] = s_Uh[q * NS + sp + sl];                                                                                  \
      refd[sl] = s_Udh[q * NS + sp + sl];                                                                                \
      dir[sl] = DIR;                                                                                                     \
    }                                                                                                                    \
    to_phys<DIM>(type, ref, J, Ji, det, phys);                                                                           \
    to_phys<DIM>(type, refd, J, Ji, det, physd);                                                                         \
    to_phys<DIM>(type, dir, J, Ji, det, pdir);                                                                           \
    _Pragma("unroll") for (int sl = 0; sl < ns; ++sl) {                                                                  \
      U[sp + sl] = mk(phys[sl], tm.alpha_u * pdir[sl]);                                                                  \
      Ud[sp + sl] = value_like(type, sl, DIM) ? mk(physd[sl], tm.alpha_t * pdir[sl]) : mk(0.0);                          \
    }                                                                                                                    \
  }

// declares pa, the point function's arguments at point q of element e.  Needs U, Ud, g, h, tm, e, q, NQ, pp.
#define MHA_POINT_ARGS(pa)                                                                                               \
  PointArgs<DIM> pa;                                                                                                     \
  pa.U = U; pa.Ud = Ud; pa.x = g + 2 * DIM * DIM + 2; pa.h = h; pa.dt = tm.dt;                                           \
  pa.transient = tm.transient; pa.e = e; pa.q = q; pa.nq = NQ; pa.pp = &pp

// back-transform w G^T F.d, variable by variable: STORE is a statement that takes w * ref[sl], the coefficient of
// reference slot sp + sl.  Needs MHA_POINT_GEO.
#define MHA_BACK_TRANSFORM(F, STORE)                                                                                     \
  _Pragma("unroll") for (int v = 0; v < L::nvars; ++v) {                                                                 \
    const int type = L::type(v), sp = slotptr_of<L, DIM>(v), ns = slots_of(type, DIM);                                   \
    double phys[1 + DIM], ref[1 + DIM];                                                                                  \
    _Pragma("unroll") for (int sl = 0; sl < ns; ++sl) phys[sl] = F[sp + sl].d;                                           \
    to_ref_T<DIM>(type, phys, J, Ji, det, ref);                                                                          \
    _Pragma("unroll") for (int sl = 0; sl < ns; ++sl) { STORE; }                                                         \
  }

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
    else if constexpr (PHYS == MHA_PHYSICS_POROUS_WEAK_GALERKIN) porous_wg_point<DIM, (EXPR != 0)>(pa, F);               \
    else if constexpr (PHYS == MHA_PHYSICS_STOKES) stokes_point<DIM, (EXPR != 0)>(pa, F);                                \
    else if constexpr (PHYS == MHA_PHYSICS_SHALLOWWATER) shallowwater_point<DIM, (EXPR != 0)>(pa, F);                    \
    else navierstokes_point<DIM, (EXPR != 0)>(pa, F);                                                                    \
  } while (0)
