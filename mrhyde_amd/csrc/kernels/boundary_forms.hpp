// boundary_forms.hpp -- the Jacobian of each module's boundary terms as a point form at a side integration point.
//
// The boundary-group Jacobian of every module that has one is  A_b = sum_q S_a(q)^T C(q) S_b(q)  with
// S_a(q) = (N_a, d_1 N_a, ..., d_DIM N_a) per variable (value and physical gradient of a basis function at the side
// point) and C(q) a small matrix between (variable, slot) pairs.  A module states C(q) ONCE, as its action
//     G = C(q) F,     F = the trial fields at the point, laid out [variable][slot], slot 0 = value, 1 + d = d_d,
// i.e. as the derivative of the integrand of its boundaryResidual in the direction F, weight and alpha_u seeding
// included.  kernels/boundary_apply.hip takes the forward product from apply(F), the transposed one from
// G_c = apply(e_c) . F and the diagonal from the columns apply(e_c) of the row's own variable: no second formula.
//
// A form names:  Dev -- the module's device record; NV(dim) variables of NS(dim) slots each (P = NV NS <= 12);
// NF functions of the record evaluated at the side points into coefficients 0 .. NF-1 of the point record; NC
// coefficients in all (NF evaluated, the rest derived by finish()); kNeedsU -- C depends on the state; kHas3D;
// has_jacobian(bc_type) -- the group types with a Jacobian.  A point record is  p[0] = w, p[1 .. DIM] = n, then the
// coefficients at p[1 + DIM + k].
#pragma once
#include "../../../include/mrhyde_amd.h"
#include "device_types.hpp"
#include "dual.hpp"
#include "swhdg_side.hpp"

namespace mha {

// sum_q w to the power 1 / (dim - 1): Workset::getSideElementSize (src/tools/workset.cpp:2682-2696)
template <int DIM>
__device__ __forceinline__ double side_element_size(const double *s_pt, int PT, int nqs) {
  double vol = 0.0;
  for (int q = 0; q < nqs; ++q) vol += s_pt[q * PT];
  return DIM == 2 ? vol : sqrt(vol);
}

// thermal, weak Dirichlet / interface (src/physics/thermal.cpp:227-243): the integrand
//   kappa w [ (epen / h)(T - g) v - (grad T . n) v - sf (T - g)(grad v . n) ],  epen = 10, sf = form_param
// is affine in T; its derivative in the direction (T, grad T) = F, tested with (v, grad v):
//   C = kappa w alpha_u [[epen / h, -n^T], [-sf n, 0]]
struct ThermalSideForm {
  using Dev = BoundaryDev;
  static constexpr bool kNeedsU = false, kHas3D = true;
  static constexpr int NF = 1, NC = 2;  // kappa | epen / h
  __host__ __device__ static constexpr int NV(int) { return 1; }
  __host__ __device__ static constexpr int NS(int dim) { return 1 + dim; }
  __host__ __device__ static bool has_jacobian(int bc) { return bc == MHA_BC_WEAK_DIRICHLET || bc == MHA_BC_INTERFACE; }
  __device__ static const FuncDesc &func(const Dev &d, int) { return d.diff; }
  template <int DIM>
  __device__ static void finish(const Dev &, double *s_pt, int PT, int nqs, int q, const double *, const double *, int) {
    s_pt[q * PT + 1 + DIM + 1] = 10.0 / side_element_size<DIM>(s_pt, PT, nqs);
  }
  template <int DIM>
  __device__ static void apply(const Dev &d, const double *p, double alpha_u, const double *F, double *G) {
    const double *nrm = p + 1, kwa = p[1 + DIM] * p[0] * alpha_u;
    double gn = 0.0;
#pragma unroll
    for (int j = 0; j < DIM; ++j) gn += F[1 + j] * nrm[j];
    G[0] = kwa * (p[1 + DIM + 1] * F[0] - gn);
#pragma unroll
    for (int j = 0; j < DIM; ++j) G[1 + j] = -kwa * d.form_param * nrm[j] * F[0];
  }
};

// helmholtz, the Robin condition of a Neumann group (src/physics/helmholtz.cpp:357-375).  With the side fields ur, ui and
//   c2durdn = sum_d (c2r_d d_d ur - c2i_d d_d ui) n_d          c2duidn = sum_d (c2r_d d_d ui + c2i_d d_d ur) n_d
// the rows of ureal and uimag test  w Br  and  w Bi  with their values,
//   Br = ar (ur + ui) - ai (ui - ur) + (durdn + duidn) - (sources) - (c2durdn + c2duidn)
//   Bi = ar (ui - ur) + ai (ur + ui) + (duidn - durdn) - (sources) - (c2duidn - c2durdn)
// linear in (ur, grad ur, ui, grad ui) = F up to the sources: the form is the two brackets at F without them.
struct HelmholtzSideForm {
  using Dev = HelmholtzBoundaryDev;
  static constexpr bool kNeedsU = false, kHas3D = true;
  static constexpr int NF = 8, NC = 8;  // c2r_x, c2i_x, c2r_y, c2i_y, c2r_z, c2i_z, alpha_r, alpha_i (the sources drop out)
  __host__ __device__ static constexpr int NV(int) { return 2; }
  __host__ __device__ static constexpr int NS(int dim) { return 1 + dim; }
  __host__ __device__ static bool has_jacobian(int bc) { return bc == MHA_BC_NEUMANN; }
  __device__ static const FuncDesc &func(const Dev &d, int kf) { return d.f[kf]; }
  template <int DIM>
  __device__ static void finish(const Dev &, double *, int, int, int, const double *, const double *, int) {}
  template <int DIM>
  __device__ static void apply(const Dev &, const double *p, double alpha_u, const double *F, double *G) {
    constexpr int NS1 = 1 + DIM;
    const double *nrm = p + 1, *c = p + 1 + DIM;
    const double ur = F[0], ui = F[NS1], ar = c[6], ai = c[7];
    double durdn = 0.0, duidn = 0.0, c2durdn = 0.0, c2duidn = 0.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      const double gr = F[1 + d] * nrm[d], gi = F[NS1 + 1 + d] * nrm[d];
      durdn += gr;
      duidn += gi;
      c2durdn += c[2 * d] * gr - c[2 * d + 1] * gi;
      c2duidn += c[2 * d] * gi + c[2 * d + 1] * gr;
    }
    const double wa = p[0] * alpha_u;
#pragma unroll
    for (int i = 0; i < 2 * NS1; ++i) G[i] = 0.0;
    G[0] = wa * (ar * (ur + ui) - ai * (ui - ur) + (durdn + duidn) - (c2durdn + c2duidn));
    G[NS1] = wa * (ar * (ui - ur) + ai * (ur + ui) + (duidn - durdn) - (c2duidn - c2durdn));
  }
};

// linearelasticity, weak Dirichlet (Nitsche) on all components (src/physics/linearelasticity.cpp:372-390 and its 3-D
// copies): with delta = u - D at the side points the row (a, d) integrates
//   w [ -(sigma n)_d N_a + pen delta_d N_a - sf (b_d . grad N_a) ]
//   sigma  = lambda_s tr(grad u) I + mu (grad u + grad u^T)     (lambda_s = 2 mu under incplanestress, :990-1000)
//   b_dj   = lambda (delta . n) delta_dj + mu (delta_d n_j + delta_j n_d),   pen = penalty (lambda + 2 mu) / h
// affine in u; in the direction F = (u_c, grad u_c)_c, delta = u.
struct LinearElasticitySideForm {
  using Dev = LeBoundaryDev;
  static constexpr bool kNeedsU = false, kHas3D = true;
  static constexpr int NF = 2, NC = 4;  // lambda, mu | lambda_s, pen
  __host__ __device__ static constexpr int NV(int dim) { return dim; }
  __host__ __device__ static constexpr int NS(int dim) { return 1 + dim; }
  __host__ __device__ static bool has_jacobian(int bc) { return bc == MHA_BC_WEAK_DIRICHLET; }
  __device__ static const FuncDesc &func(const Dev &d, int kf) { return d.f[3 + kf]; }
  template <int DIM>
  __device__ static void finish(const Dev &d, double *s_pt, int PT, int nqs, int q, const double *, const double *, int) {
    double *c = s_pt + q * PT + 1 + DIM;
    c[2] = (DIM == 2 && d.plane_stress) ? 2.0 * c[1] : c[0];
    c[3] = d.penalty * (c[0] + 2.0 * c[1]) / side_element_size<DIM>(s_pt, PT, nqs);
  }
  template <int DIM>
  __device__ static void apply(const Dev &dv, const double *p, double alpha_u, const double *F, double *G) {
    constexpr int NS1 = 1 + DIM;
    const double *nrm = p + 1, *c = p + 1 + DIM;
    const double lam = c[0], mu = c[1], lam_s = c[2], pen = c[3], wa = p[0] * alpha_u;
    double tr = 0.0, un = 0.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      tr += F[d * NS1 + 1 + d];
      un += F[d * NS1] * nrm[d];
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      double sn = lam_s * tr * nrm[d];
#pragma unroll
      for (int j = 0; j < DIM; ++j) sn += mu * (F[d * NS1 + 1 + j] + F[j * NS1 + 1 + d]) * nrm[j];
      G[d * NS1] = wa * (pen * F[d * NS1] - sn);
#pragma unroll
      for (int j = 0; j < DIM; ++j) {
        const double b = (d == j ? lam * un : 0.0) + mu * (F[d * NS1] * nrm[j] + F[j * NS1] * nrm[d]);
        G[d * NS1 + 1 + j] = -wa * dv.form_param * b;
      }
    }
  }
};

// shallowwaterHybridized (src/physics/shallowwaterHybridized.cpp:190-263): the rows of H, Hux, Huy test the side flux
// f(S; Shat, Sinf, n) (swh_interface_flux: F(Shat) . n + Stab on interface sides, the boundary term on far-field and slip
// sides) with their values.  f is nonlinear in the side state S of u: the form is its directional derivative at S, one
// evaluation on Dual numbers.  Value slots only.
struct SwhSideForm {
  using Dev = SwhBoundaryDev;
  static constexpr bool kNeedsU = true, kHas3D = false;
  static constexpr int NF = 6, NC = 9;  // Shat (3), Sinf (3) | S (3)
  __host__ __device__ static constexpr int NV(int) { return 3; }
  __host__ __device__ static constexpr int NS(int) { return 1; }
  __host__ __device__ static bool has_jacobian(int bc) { return bc >= MHA_BC_SWH_INTERFACE && bc <= MHA_BC_SWH_SLIP; }
  __device__ static const FuncDesc &func(const Dev &d, int kf) { return kf < 3 ? d.aux[kf] : d.farfield[kf - 3]; }
  // S(q) = sum_a u_(i,a) N_a(q); s_S: the basis table [side point][slot][basis function]
  template <int DIM>
  __device__ static void finish(const Dev &, double *s_pt, int PT, int, int q, const double *s_u, const double *s_S, int card) {
    double *c = s_pt + q * PT + 1 + DIM;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double s = 0.0;
      for (int a = 0; a < card; ++a) s += s_u[i * card + a] * s_S[q * card + a];
      c[6 + i] = s;
    }
  }
  template <int DIM>
  __device__ static void apply(const Dev &d, const double *p, double alpha_u, const double *F, double *G) {
    const double *c = p + 1 + DIM;
    Dual S[3], Sh[3], f[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      S[i] = mk(c[6 + i], F[i]);
      Sh[i] = mk(c[i]);
    }
    swh_interface_flux(d.side_type, d.roe != 0, S, Sh, c + 3, p[1], p[2], d.g, f);
#pragma unroll
    for (int i = 0; i < 3; ++i) G[i] = f[i].d * p[0] * alpha_u;
  }
};

}  // namespace mha
