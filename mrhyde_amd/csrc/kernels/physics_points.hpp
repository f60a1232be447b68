// physics_points.hpp -- the physics modules as POINT functions.
//
// A module's volumeResidual in the reference is a loop nest `res(e, off(dof)) += sum_k F_k(e,pt) * T_k(e,dof,pt)`
// where T_k runs over the test function's value / gradient components / divergence and F_k are expressions in the
// solution fields at the point.  Here each module states only F(U, Udot, x): the engine (point_engine.hip) supplies the
// fields, differentiates F with Dual numbers direction by direction and contracts with the basis tables.
// Slot numbering: variables in the module's myvars order; HGRAD -> [value, d/dx, d/dy(, d/dz)], HVOL -> [value],
// HDIV -> [v_x, v_y(, v_z), div].  The integration weight is applied by the engine.
#pragma once
#include <type_traits>

#include "device_math.hpp"
#include "dual.hpp"
#include "linearelasticity_stress.hpp"

namespace mha {

template <int DIM>
struct PointArgs {
  const Dual *U;    // fields at the point, slot order
  const Dual *Ud;   // time derivatives (value-like slots only)
  const double *x;  // physical coordinates
  double h, dt;     // element size (sum of wts)^(1/dim), time step
  int transient;
  int e, q, nq;
  const PhysParamsDev *pp;
};

// a function of the module at the point as a Dual: field-dependent deck strings carry the derivative with respect to the
// direction the point's fields are seeded with, everything else is a constant of that direction.  nx ny nz h are 0 as
// in eval_func's volume callers (a.h is the stabilisation's element size, not an operand of deck strings)
template <int DIM>
__device__ __forceinline__ Dual func_dual(const FuncDesc &f, const PointArgs<DIM> &a) {
  if (f.kind == MHA_FUNC_EXPRESSION) return eval_expression_dual<DIM>(f, a.x, nullptr, 0.0, a.U, a.Ud);
  return mk(eval_func<DIM, false>(f, a.e, a.q, a.nq, a.x));
}

// thermal (reference: src/physics/thermal.cpp:71-165); functions {source, diffusion, specific heat, density}
// EXPR: 0 constants / closed forms / arrays, 1 deck strings in the coordinates, 2 deck strings that read the solution
// fields ("1+e*e": a nonlinear diffusion; the reference's FunctionManager<AD> differentiates them with Sacado)
template <int DIM, int EXPR>
__device__ __forceinline__ void thermal_point(const PointArgs<DIM> &a, Dual *F) {
  const PhysParamsDev &pp = *a.pp;
  if constexpr (EXPR == 2) {
    const Dual f = func_dual<DIM>(pp.f[0], a), kap = func_dual<DIM>(pp.f[1], a);
    const Dual cp = func_dual<DIM>(pp.f[2], a), rho = func_dual<DIM>(pp.f[3], a);
    F[0] = a.Ud[0] * (rho * cp) - f;
#pragma unroll
    for (int d = 0; d < DIM; ++d) F[1 + d] = a.U[1 + d] * kap;
    return;
  } else {
  constexpr bool EX = EXPR != 0;
  const double f = eval_func<DIM, EX>(pp.f[0], a.e, a.q, a.nq, a.x), kap = eval_func<DIM, EX>(pp.f[1], a.e, a.q, a.nq, a.x);
  const double cp = eval_func<DIM, EX>(pp.f[2], a.e, a.q, a.nq, a.x), rho = eval_func<DIM, EX>(pp.f[3], a.e, a.q, a.nq, a.x);
  F[0] = a.Ud[0] * (rho * cp) - f;
#pragma unroll
  for (int d = 0; d < DIM; ++d) F[1 + d] = a.U[1 + d] * kap;
  // have_advection: (b . grad e) against the value of the test function (thermal.cpp:150-160).  Not in the deck-string
  // instantiation: with the interpreter inlined the kernel is at the scratch it may use (the host refuses that mix)
  if constexpr (!EX)
  if (pp.p[0] != 0.0) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) F[0] = F[0] + a.U[1 + d] * eval_func<DIM, false>(pp.f[4 + d], a.e, a.q, a.nq, a.x);  // (no deck strings: host checks)
  }
  }
}

// porousMixed (reference: src/physics/porousMixed.cpp:158-338); myvars {p (HVOL), u (HDIV)};
// functions {source, Kinv_xx, Kinv_yy, Kinv_zz, total_mobility}; HET: heterogeneous permeability (PorousHetDev) --
// Kinv = 1 / element data column 0 instead of the functions, then divided by exp of the KL log-field
template <int DIM, bool EXPR, bool HET = false>
__device__ __forceinline__ void porous_point(const PointArgs<DIM> &a, Dual *F) {
  const PhysParamsDev &pp = *a.pp;
  const double src = eval_func<DIM, EXPR>(pp.f[0], a.e, a.q, a.nq, a.x), mob = eval_func<DIM, EXPR>(pp.f[4], a.e, a.q, a.nq, a.x);
  const Dual p = a.U[0], divu = a.U[1 + DIM];
  F[0] = mk(src) - divu;  // (source - div u, q)
  double kl[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) kl[d] = 0.0;
  if constexpr (HET)
    if (pp.het.kl) kl_log_field<DIM>(pp.het, a.x, kl);
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    double Kinv;
    if constexpr (HET) {
      Kinv = pp.het.edata ? 1.0 / pp.het.edata[(size_t)a.e * pp.het.ecols] : eval_func<DIM, EXPR>(pp.f[1 + d], a.e, a.q, a.nq, a.x);
      if (pp.het.kl) Kinv = Kinv / exp(kl[d]);
    } else {
      Kinv = eval_func<DIM, EXPR>(pp.f[1 + d], a.e, a.q, a.nq, a.x);
    }
    F[1 + d] = a.U[1 + d] * Kinv / mob;  // ((mobility K)^-1 u, v)
  }
  F[1 + DIM] = -p;  // -(p, div v)
}

// porousWeakGalerkin (reference: src/physics/porousWeakGalerkin.cpp:94-323); myvars of the block {pint (HVOL), u (HDIV),
// t (HDIV)}; slots pint, u_x.., div u, t_x.., div t; functions {source, perm}.  With element data ("use permeability
// data", updatePerm :601-609) perm = data(elem, 0): the value itself, not its inverse as in porousMixed.  The data
// pointer is a kernel argument, so the test is wave-uniform and the same instantiation carries deck strings beside it.
template <int DIM, bool EXPR>
__device__ __forceinline__ void porous_wg_point(const PointArgs<DIM> &a, Dual *F) {
  const PhysParamsDev &pp = *a.pp;
  const double src = eval_func<DIM, EXPR>(pp.f[0], a.e, a.q, a.nq, a.x);
  const double perm = pp.het.edata ? pp.het.edata[(size_t)a.e * pp.het.ecols] : eval_func<DIM, EXPR>(pp.f[1], a.e, a.q, a.nq, a.x);
  constexpr int U0 = 1, T0 = 2 + DIM;
  F[0] = a.U[T0 + DIM] - src;  // (div t - source, q)
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    F[U0 + d] = a.U[U0 + d];                         // (u, v)
    F[T0 + d] = a.U[U0 + d] * perm + a.U[T0 + d];  // (perm u + t, s)
  }
  F[U0 + DIM] = a.U[0];  // (pint, div v)
  F[T0 + DIM] = mk(0.0);
}

// navierstokes (reference: src/physics/navierstokes.cpp:82-849, computeTau :1054-1079); myvars {ux, pr, uy[, uz]};
// functions {source ux, source pr, source uy, source uz, density, viscosity}; p = {useSUPG, usePSPG, fix_uz_offsets}
template <int DIM, bool EXPR>
__device__ __forceinline__ void navierstokes_point(const PointArgs<DIM> &a, Dual *F) {
  constexpr int S = 1 + DIM;                 // slots per HGRAD variable
  constexpr int vnum[3] = {0, 2, 3}, prnum = 1;
  const PhysParamsDev &pp = *a.pp;
  const bool useSUPG = pp.p[0] != 0.0, usePSPG = pp.p[1] != 0.0, fix_uz = pp.p[2] != 0.0;
  const double dens = eval_func<DIM, EXPR>(pp.f[4], a.e, a.q, a.nq, a.x), visc = eval_func<DIM, EXPR>(pp.f[5], a.e, a.q, a.nq, a.x);
  const double src[3] = {eval_func<DIM, EXPR>(pp.f[0], a.e, a.q, a.nq, a.x), eval_func<DIM, EXPR>(pp.f[2], a.e, a.q, a.nq, a.x),
                         DIM == 3 ? eval_func<DIM, EXPR>(pp.f[3], a.e, a.q, a.nq, a.x) : 0.0};
  Dual vel[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) vel[d] = a.U[vnum[d] * S];
  const Dual pr = a.U[prnum * S];
  Dual tau = mk(0.0);
  if (useSUPG || usePSPG) {
    const double C1 = 4.0, C2 = 2.0, C3 = a.transient ? 2.0 : 0.0;
    Dual nvel = mk(0.0);
#pragma unroll
    for (int d = 0; d < DIM; ++d) nvel += vel[d] * vel[d];
    if (nvel.v > 1e-12) nvel = dsqrt(nvel);
    const Dual t2 = nvel * (C2 / a.h);
    const double c1 = C1 * visc / a.h / a.h, c3 = C3 / a.dt;
    tau = 1.0 / dsqrt(t2 * t2 + (c1 * c1 + c3 * c3));
  }
  Dual stab[DIM];
  Dual divu = mk(0.0);
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    const int b = vnum[i] * S;
    Dual conv = mk(0.0);
#pragma unroll
    for (int d = 0; d < DIM; ++d) conv += vel[d] * a.U[b + 1 + d];
    const Dual acc = a.Ud[b] + conv;
    F[b] = (acc - src[i]) * dens;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      F[b + 1 + d] = a.U[b + 1 + d] * visc;
      if (d == i) F[b + 1 + d] -= pr;
    }
    divu += a.U[b + 1 + i];
    if (useSUPG || usePSPG) stab[i] = acc * dens + a.U[prnum * S + 1 + i] - dens * src[i];
    if (useSUPG) {
      const Dual ts = tau * stab[i];
#pragma unroll
      for (int d = 0; d < DIM; ++d) F[b + 1 + d] += ts * vel[d];
    }
  }
  F[prnum * S] = divu;
#pragma unroll
  for (int d = 0; d < DIM; ++d) F[prnum * S + 1 + d] = usePSPG ? stab[d] * tau / dens : mk(0.0);
  if (DIM == 3 && !fix_uz) {
    // the reference scatters the uz momentum block through uy's offsets (navierstokes.cpp:688): uy's rows receive both
    // blocks (same HGRAD basis), uz's rows stay empty
#pragma unroll
    for (int s = 0; s < S; ++s) {
      F[vnum[1] * S + s] += F[vnum[DIM - 1] * S + s];
      F[vnum[DIM - 1] * S + s] = mk(0.0);
    }
  }
}

// navierstokes + thermal on one block (Boussinesq coupling; reference: navierstokes::setWorkset :1026-1046 sets
// have_energy when the block has a variable "e", thermal::setWorkset thermal.cpp:359-379 sets have_nsvel when it has
// "ux"); myvars {ux, pr, uy[, uz], e}; functions {source ux, source pr, source uy, source uz, density, viscosity,
// thermal source, thermal diffusion, specific heat, bx, by, bz} -- "density" is ONE function read by both modules
// (FunctionManager::addFunction keeps the first tree of a name, functionManager.cpp:48-68);
// p = {useSUPG, usePSPG, fix_uz_offsets, T_ambient, beta, include advection}.
// With g_i = beta (e - T_ambient) source_i the momentum rows get the navierstokes terms plus
//   value slot      + density g_i                         (navierstokes.cpp:283-296, 368-381, 529-…, 619-632, 709-722)
//   SUPG            + tau (density g_i) u_d on slot d      (:318-334, 402-418, 654-671, 744-761)
//   PSPG, pr row    + tau density g_d on slot d            (:471-488, 824-845)
// and the energy row is thermal's with (u . grad e, v) added (thermal.cpp:139-149).  Its own function: the two modules'
// point functions above compile exactly as without it.
template <int DIM, bool EXPR>
__device__ __forceinline__ void navierstokes_thermal_point(const PointArgs<DIM> &a, Dual *F) {
  constexpr int S = 1 + DIM;                 // slots per HGRAD variable
  constexpr int vnum[3] = {0, 2, 3}, prnum = 1, eb = (DIM + 1) * S;  // eb: first slot of e
  const PhysParamsDev &pp = *a.pp;
  const bool useSUPG = pp.p[0] != 0.0, usePSPG = pp.p[1] != 0.0, fix_uz = pp.p[2] != 0.0;
  const double T_ambient = pp.p[3], beta = pp.p[4];
  auto fn = [&](int k) { return eval_func<DIM, EXPR>(pp.f[k], a.e, a.q, a.nq, a.x); };
  const double dens = fn(4), visc = fn(5);
  const double src[3] = {fn(0), fn(2), DIM == 3 ? fn(3) : 0.0};
  Dual vel[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) vel[d] = a.U[vnum[d] * S];
  const Dual pr = a.U[prnum * S];
  const Dual bt = (a.U[eb] - T_ambient) * (beta * dens);  // density beta (e - T_ambient)
  Dual tau = mk(0.0);
  if (useSUPG || usePSPG) {  // computeTau (navierstokes.cpp:1054-1079)
    const double C1 = 4.0, C2 = 2.0, C3 = a.transient ? 2.0 : 0.0;
    Dual nvel = mk(0.0);
#pragma unroll
    for (int d = 0; d < DIM; ++d) nvel += vel[d] * vel[d];
    if (nvel.v > 1e-12) nvel = dsqrt(nvel);
    const Dual t2 = nvel * (C2 / a.h);
    const double c1 = C1 * visc / a.h / a.h, c3 = C3 / a.dt;
    tau = 1.0 / dsqrt(t2 * t2 + (c1 * c1 + c3 * c3));
  }
  Dual stab[DIM], buoy[DIM];
  Dual divu = mk(0.0);
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    const int b = vnum[i] * S;
    Dual conv = mk(0.0);
#pragma unroll
    for (int d = 0; d < DIM; ++d) conv += vel[d] * a.U[b + 1 + d];
    const Dual acc = a.Ud[b] + conv;
    buoy[i] = bt * src[i];
    F[b] = (acc - src[i]) * dens + buoy[i];
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      F[b + 1 + d] = a.U[b + 1 + d] * visc;
      if (d == i) F[b + 1 + d] -= pr;
    }
    divu += a.U[b + 1 + i];
    if (useSUPG || usePSPG) stab[i] = acc * dens + a.U[prnum * S + 1 + i] - dens * src[i];
    if (useSUPG) {
      const Dual ts = tau * (stab[i] + buoy[i]);
#pragma unroll
      for (int d = 0; d < DIM; ++d) F[b + 1 + d] += ts * vel[d];
    }
  }
  F[prnum * S] = divu;
  // the buoyancy part of the PSPG term is NOT divided by the density, unlike the part next to it (navierstokes.cpp:480-483
  // and :833-838 against :462-465 and :813-818): the reference's behaviour, reproduced
#pragma unroll
  for (int d = 0; d < DIM; ++d) F[prnum * S + 1 + d] = usePSPG ? stab[d] * tau / dens + tau * buoy[d] : mk(0.0);
  if (DIM == 3 && !fix_uz) {
    // the reference scatters the uz momentum block through uy's offsets (navierstokes.cpp:688 is the `off` of :690-761):
    // the whole block, buoyancy and its SUPG part included, lands on uy's rows; uz's rows stay empty
#pragma unroll
    for (int s = 0; s < S; ++s) {
      F[vnum[1] * S + s] += F[vnum[DIM - 1] * S + s];
      F[vnum[DIM - 1] * S + s] = mk(0.0);
    }
  }
  // energy row (thermal.cpp:125-163): rho cp de/dt - source, kappa grad e, then (u . grad e, v) WITHOUT rho cp
  // (have_nsvel, :139-149) and (b . grad e, v) when "include advection" is set (:150-160)
  const double f = fn(6), kap = fn(7), cp = fn(8);
  F[eb] = a.Ud[eb] * (dens * cp) - f;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    F[eb + 1 + d] = a.U[eb + 1 + d] * kap;
    F[eb] += vel[d] * a.U[eb + 1 + d];
  }
  if (pp.p[5] != 0.0) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) F[eb] += a.U[eb + 1 + d] * fn(9 + d);
  }
}

// cdr, convection-diffusion-reaction (reference: src/physics/cdr.cpp:62-142); myvars {c}; functions {source, diffusion,
// specific heat, density, reaction, xvel, yvel, zvel} with the reference's defaults 0, 1, 1, 1, 1, 1, 1, 1 (:40-47).
//   value slot       c_t + v . grad c + reaction - source      (no rho cp on the time derivative, :104 / :117 / :131)
//   gradient slot d  diffusion / (density specific heat) d_d c
// "SUPG tau" is evaluated by the reference and never used (:82 against :96-140), computeTau (:186-207) has no caller:
// neither is here.  cdr_row is the row of c on any block: cb = first slot of c; COUPLED picks the function table of
// navierstokes_cdr_point below.  EXPR as for thermal_point; with 2 EVERY function goes through func_dual, so a function
// may read c, grad(c)[x|y|z], c_t, the other variables of a coupled block, the coordinates and other named functions
// (reaction: '0.5*c*c', xvel: 'ux').  The functions are evaluated in a loop that is NOT unrolled: the Dual interpreter
// is inlined once, and the kernel keeps to the scratch it may use (require_modest_scratch).
template <bool COUPLED>
__device__ __forceinline__ constexpr int cdr_func_index(int k) {
  // k: 0 source, 1 diffusion, 2 specific heat, 3 density, 4 reaction, 5.. xvel, yvel, zvel
  return !COUPLED ? k : k == 0 ? 1 : k == 3 ? 4 : k < 3 ? 5 + k : 4 + k;
}
template <int DIM, int EXPR, bool COUPLED>
__device__ __forceinline__ void cdr_row(const PointArgs<DIM> &a, int cb, Dual *F) {
  constexpr int NF = 5 + DIM;
  using T = std::conditional_t<EXPR == 2, Dual, double>;
  const PhysParamsDev &pp = *a.pp;
  T fv[NF];
  if constexpr (EXPR == 2) {
#pragma nounroll
    for (int k = 0; k < NF; ++k) fv[k] = func_dual<DIM>(pp.f[cdr_func_index<COUPLED>(k)], a);
  } else if constexpr (EXPR == 1) {
#pragma nounroll
    for (int k = 0; k < NF; ++k) fv[k] = eval_func<DIM, true>(pp.f[cdr_func_index<COUPLED>(k)], a.e, a.q, a.nq, a.x);
  } else {
#pragma unroll
    for (int k = 0; k < NF; ++k) fv[k] = eval_func<DIM, (EXPR != 0)>(pp.f[cdr_func_index<COUPLED>(k)], a.e, a.q, a.nq, a.x);
  }
  Dual f = a.Ud[cb] + fv[4] - fv[0];
  const T kd = fv[1] / (fv[3] * fv[2]);
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    f += a.U[cb + 1 + d] * fv[5 + d];
    F[cb + 1 + d] = a.U[cb + 1 + d] * kd;
  }
  F[cb] = f;
}
template <int DIM, int EXPR>
__device__ __forceinline__ void cdr_point(const PointArgs<DIM> &a, Dual *F) {
  cdr_row<DIM, EXPR, false>(a, 0, F);
}

// navierstokes + cdr on one block (the reference's `modules: navier stokes, cdr`); myvars {ux, pr, uy[, uz], c}.  No
// built-in coupling term: the rows of navierstokes_point and the row of cdr_row side by side; the coupling is whatever
// cdr's functions read (xvel: 'ux' gives the c-row / ux-column entries as the derivative of a deck string).
// functions {source ux, source (cdr's), source uy, source uz, density, viscosity, diffusion, specific heat, reaction,
// xvel, yvel, zvel}: navierstokes' table with cdr's source where "source pr" would be -- navierstokes_point never reads
// that entry, and with it the coupled module would name 13 functions where the table holds 12 -- then cdr's own.
// "density" is ONE function read by both modules (FunctionManager::addFunction keeps the first tree of a name).
// p = navierstokes' {useSUPG, usePSPG, fix_uz_offsets}.  With EXPR = 2 only cdr's functions are Duals; navierstokes'
// own are plain values (the host refuses a field-reading one by name).
template <int DIM, int EXPR>
__device__ __forceinline__ void navierstokes_cdr_point(const PointArgs<DIM> &a, Dual *F) {
  if constexpr (EXPR == 0) {
    navierstokes_point<DIM, false>(a, F);
  } else {
    // navierstokes' five functions (source ux / uy / uz, density, viscosity) in a loop that is not unrolled -- one
    // inlined interpreter instead of five -- then handed to navierstokes_point as constants
    PhysParamsDev nsp;
    double v[5];
#pragma nounroll
    for (int k = 0; k < 5; ++k) v[k] = eval_func<DIM, true>(a.pp->f[k == 0 ? 0 : k + 1], a.e, a.q, a.nq, a.x);
    nsp.f[0].amp = v[0];
#pragma unroll
    for (int k = 1; k < 5; ++k) nsp.f[k + 1].amp = v[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) nsp.p[k] = a.pp->p[k];
    static_assert(MHA_FUNC_CONSTANT == 0, "a default FuncDesc is a constant");
    PointArgs<DIM> an = a;
    an.pp = &nsp;
    navierstokes_point<DIM, false>(an, F);
  }
  cdr_row<DIM, EXPR, true>(a, (DIM + 1) * (1 + DIM), F);
}

// helmholtz, the frequency-domain wave module (reference: src/physics/helmholtz.cpp:175-193, the non-fractional branch);
// myvars {ureal, uimag}, both HGRAD of ONE order (the host refuses two); functions {c2r_x, c2i_x, c2r_y, c2i_y, c2r_z,
// c2i_z, omega2r, omega2i, source_r, source_i}, all 0 by default (:41-70).  The reference tests row ureal with
// (vr, vi) = (ureal's basis i, uimag's basis i) and adds real and imaginary test parts (its own comment: "this residual
// makes no sense to me"); with one order vr = vi = N_i and the two rows are
//   value slot of ureal     -omega2r (ur + ui) + omega2i (ui - ur) - (source_r + source_i)
//   gradient slot d         c2r_d (d_d ur + d_d ui) - c2i_d (d_d ui - d_d ur)
//   value slot of uimag     -omega2r (ui - ur) - omega2i (ur + ui) - (source_i - source_r)
//   gradient slot d         c2r_d (d_d ui - d_d ur) + c2i_d (d_d ur + d_d ui)
// kept as they are: the reference's gold depends on them.  No time-derivative term.  EXPR: 0 constants / closed forms /
// arrays, 1 deck strings in the coordinates, evaluated in a loop that is NOT unrolled (one inlined interpreter).
template <int DIM, bool EXPR>
__device__ __forceinline__ void helmholtz_point(const PointArgs<DIM> &a, Dual *F) {
  constexpr int S = 1 + DIM, NF = 2 * DIM + 4;
  const PhysParamsDev &pp = *a.pp;
  // k: 0 .. 2 DIM - 1 the c2 pairs of the directions, then omega2r, omega2i, source_r, source_i (table entries 6 .. 9)
  double fv[NF];
  if constexpr (EXPR) {
#pragma nounroll
    for (int k = 0; k < NF; ++k) fv[k] = eval_func<DIM, true>(pp.f[k < 2 * DIM ? k : k + 6 - 2 * DIM], a.e, a.q, a.nq, a.x);
  } else {
#pragma unroll
    for (int k = 0; k < NF; ++k) fv[k] = eval_func<DIM, false>(pp.f[k < 2 * DIM ? k : k + 6 - 2 * DIM], a.e, a.q, a.nq, a.x);
  }
  const double w2r = fv[2 * DIM], w2i = fv[2 * DIM + 1], sr = fv[2 * DIM + 2], si = fv[2 * DIM + 3];
  const Dual ur = a.U[0], ui = a.U[S];
  F[0] = (ui - ur) * w2i - (ur + ui) * w2r - (sr + si);
  F[S] = (ur - ui) * w2r - (ur + ui) * w2i - (si - sr);
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const Dual gr = a.U[1 + d], gi = a.U[S + 1 + d];
    const double cr = fv[2 * d], ci = fv[2 * d + 1];
    F[1 + d] = (gr + gi) * cr - (gi - gr) * ci;
    F[S + 1 + d] = (gi - gr) * cr + (gr + gi) * ci;
  }
}

// linearelasticity (reference: src/physics/linearelasticity.cpp:92-240 with computeStress :913-1099, onside = false);
// myvars {dx, dy[, dz]}; functions {lambda, mu, source dx, source dy, source dz}; p = {incplanestress}.
// sigma = lambda tr(grad u) I + mu (grad u + grad u^T); row d gets sum_j sigma_dj d_j v - source_d v.  incplanestress
// (2-D, :990-1000) writes the normal stresses as 4 mu d_x dx + 2 mu d_y dy and its mirror: the Lame form with lambda = 2 mu.
// No time-derivative term: a transient call scales the operator by alpha_u through the seeding.
template <int DIM, bool EXPR>
__device__ __forceinline__ void linearelasticity_point(const PointArgs<DIM> &a, Dual *F) {
  static_assert(DIM >= 2, "");
  constexpr int S = 1 + DIM;  // slots per HGRAD variable
  const PhysParamsDev &pp = *a.pp;
  auto fn = [&](int k) { return eval_func<DIM, EXPR>(pp.f[k], a.e, a.q, a.nq, a.x); };
  const double mu = fn(1);
  const double lam = (DIM == 2 && pp.p[0] != 0.0) ? 2.0 * mu : fn(0);
  Dual tr = mk(0.0);
#pragma unroll
  for (int d = 0; d < DIM; ++d) tr += a.U[d * S + 1 + d];
  const Dual ltr = tr * lam;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    F[d * S] = mk(-fn(2 + d));
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
      F[d * S + 1 + j] = (a.U[d * S + 1 + j] + a.U[j * S + 1 + d]) * mu;
      if (j == d) F[d * S + 1 + j] += ltr;
    }
  }
}

// linearelasticity + thermal on one block (the thermoelastic coupling; reference: linearelasticity::setWorkset
// linearelasticity.cpp:860-906 finds e_num when the block has a variable "e", computeStress :913-1276 then subtracts
// alpha_T (e - T_ambient) c from the normal stresses); myvars {dx, dy[, dz], e}; functions {lambda, mu, source dx,
// source dy, source dz, thermal source, thermal diffusion, specific heat, density, bx, by, bz};
// p = {incplanestress, T_ambient, alpha_T, include advection}.  Displacement rows: those of linearelasticity_point with the
// stress of le_stress (linearelasticity_stress.hpp); energy row: thermal's without have_nsvel (thermal.cpp:125-163).  The
// e-columns of the displacement rows come out of the same forward-AD pass; the energy row reads no displacement.  Its own
// function: the two modules' point functions above compile exactly as without it.
template <int DIM, bool EXPR>
__device__ __forceinline__ void linearelasticity_thermal_point(const PointArgs<DIM> &a, Dual *F) {
  static_assert(DIM >= 2, "");
  constexpr int S = 1 + DIM, eb = DIM * S;  // slots per HGRAD variable; first slot of e
  const PhysParamsDev &pp = *a.pp;
  auto fn = [&](int k) { return eval_func<DIM, EXPR>(pp.f[k], a.e, a.q, a.nq, a.x); };
  const double lam = fn(0), mu = fn(1);
  Dual gu[DIM * DIM], sig[DIM * DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d)
#pragma unroll
    for (int j = 0; j < DIM; ++j) gu[d * DIM + j] = a.U[d * S + 1 + j];
  le_stress<DIM, Dual>(gu, &a.U[eb], lam, mu, pp.p[0] != 0.0, pp.p[2], pp.p[1], sig);
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    F[d * S] = mk(-fn(2 + d));
#pragma unroll
    for (int j = 0; j < DIM; ++j) F[d * S + 1 + j] = sig[d * DIM + j];
  }
  const double f = fn(5), kap = fn(6), cp = fn(7), rho = fn(8);
  F[eb] = a.Ud[eb] * (rho * cp) - f;
#pragma unroll
  for (int d = 0; d < DIM; ++d) F[eb + 1 + d] = a.U[eb + 1 + d] * kap;
  if (pp.p[3] != 0.0) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) F[eb] += a.U[eb + 1 + d] * fn(9 + d);
  }
}

// shallowwaterHybridized (reference: src/physics/shallowwaterHybridized.cpp:113-184 with computeFluxVector(false)
// :409-480); myvars {H, Hux, Huy} (2-D); functions {source H, source Hux, source Huy}; p = {g}
template <int DIM, bool EXPR>
__device__ __forceinline__ void swhdg_point(const PointArgs<DIM> &a, Dual *F) {
  static_assert(DIM >= 2, "");
  constexpr int S = 1 + DIM;
  const PhysParamsDev &pp = *a.pp;
  const double g = pp.p[0];
  const Dual H = a.U[0], Hux = a.U[S], Huy = a.U[2 * S];
  const Dual hh = H * H * (0.5 * g);
  Dual Fl[3][2];
  Fl[0][0] = Hux; Fl[0][1] = Huy;
  Fl[1][0] = Hux * Hux / H + hh; Fl[1][1] = Hux * Huy / H;
  Fl[2][0] = Hux * Huy / H; Fl[2][1] = Huy * Huy / H + hh;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    F[i * S] = a.Ud[i * S] - eval_func<DIM, EXPR>(pp.f[i], a.e, a.q, a.nq, a.x);  // (v, dS/dt) - (v, source)
    F[i * S + 1] = -Fl[i][0];                                               // -(dv/dx, F_x)
    F[i * S + 2] = -Fl[i][1];                                               // -(dv/dy, F_y)
  }
}

// stokes (reference: src/physics/stokes.cpp:178-438); myvars {ux, pr, uy[, uz]}; functions {source ux, source uy,
// source uz, viscosity} -- "source pr" is registered and evaluated by the reference (:59, :78) and read by no term: it is
// not in the table; p = {usePSPG, useLSIC}.
//   momentum row i   value slot -source_i; gradient slot d  viscosity d_d u_i - delta_id pr
//   pr row           value slot div u
//   usePSPG          gradient slot d of the pr row += tau (d_d pr + source_d), tau = h / (2 viscosity) in 2-D (:256; the
//                    line with h^2 is commented out there) and h^2 / (2 viscosity) in 3-D (:402)
//   useLSIC          EVERY gradient slot of the pr row += h^2 / (2 viscosity) div u: the reference tests with
//                    d_x q + d_y q [+ d_z q] (:283, :432)
// kept as they are: the reference's gold depends on them.  No time-derivative term: a transient call scales the
// operator by alpha_u through the seeding.  The uz rows use their own offsets (:353).  a.h is Workset::getElementSize.
// EXPR: deck strings in the coordinates, evaluated in a loop that is NOT unrolled (one inlined interpreter).
template <int DIM, bool EXPR>
__device__ __forceinline__ void stokes_point(const PointArgs<DIM> &a, Dual *F) {
  static_assert(DIM >= 2, "");
  constexpr int S = 1 + DIM, NF = DIM + 1;  // slots per HGRAD variable; functions read
  constexpr int vnum[3] = {0, 2, 3}, prnum = 1;
  const PhysParamsDev &pp = *a.pp;
  double fv[NF];  // source_0 .. source_{DIM-1}, viscosity
  if constexpr (EXPR) {
#pragma nounroll
    for (int k = 0; k < NF; ++k) fv[k] = eval_func<DIM, true>(pp.f[k], a.e, a.q, a.nq, a.x);
  } else {
#pragma unroll
    for (int k = 0; k < NF; ++k) fv[k] = eval_func<DIM, false>(pp.f[k], a.e, a.q, a.nq, a.x);
  }
  const double visc = fv[DIM];
  const Dual pr = a.U[prnum * S];
  Dual divu = mk(0.0);
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    const int b = vnum[i] * S;
    F[b] = mk(-fv[i]);
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      F[b + 1 + d] = a.U[b + 1 + d] * visc;
      if (d == i) F[b + 1 + d] -= pr;
    }
    divu += a.U[b + 1 + i];
  }
  F[prnum * S] = divu;
#pragma unroll
  for (int d = 0; d < DIM; ++d) F[prnum * S + 1 + d] = mk(0.0);
  if (pp.p[0] != 0.0) {
    const double tau = (DIM == 2 ? a.h : a.h * a.h) / (2.0 * visc);
#pragma unroll
    for (int d = 0; d < DIM; ++d) F[prnum * S + 1 + d] += (a.U[prnum * S + 1 + d] + fv[d]) * tau;
  }
  if (pp.p[1] != 0.0) {
    const Dual s = divu * (a.h * a.h / (2.0 * visc));
#pragma unroll
    for (int d = 0; d < DIM; ++d) F[prnum * S + 1 + d] += s;
  }
}

// shallowwater, continuous Galerkin (reference: src/physics/shallowwater.cpp:118-153); myvars {H, Hu, Hv} (2-D);
// functions {bathymetry, bathymetry_x, bathymetry_y, source H, source Hu, source Hv}; p = {gravity}.  The variable H
// holds the surface elevation xi, the depth is D = xi + bathymetry:
//   row H    value slot xi_t - source H;                          gradient slots (-Hu, -Hv)
//   row Hu   value slot Hu_t - g xi bathymetry_x - source Hu;     gradient slots (-(Hu^2/D + g (D D - b b) / 2), -Hu Hv / D)
//   row Hv   the mirror image
// D D - b b is kept as the reference writes it (:137, :145); a dry point (D = 0) divides by zero as there.  "viscosity"
// and "Coriolis" are evaluated by the reference (:79-80) and read by no term: they are not in the table.
// EXPR: deck strings in the coordinates, evaluated in a loop that is NOT unrolled (one inlined interpreter).
template <int DIM, bool EXPR>
__device__ __forceinline__ void shallowwater_point(const PointArgs<DIM> &a, Dual *F) {
  static_assert(DIM == 2, "shallowwater is 2-D");
  constexpr int S = 1 + DIM, NF = 6;
  const PhysParamsDev &pp = *a.pp;
  double fv[NF];
  if constexpr (EXPR) {
#pragma nounroll
    for (int k = 0; k < NF; ++k) fv[k] = eval_func<DIM, true>(pp.f[k], a.e, a.q, a.nq, a.x);
  } else {
#pragma unroll
    for (int k = 0; k < NF; ++k) fv[k] = eval_func<DIM, false>(pp.f[k], a.e, a.q, a.nq, a.x);
  }
  const double g = pp.p[0], bath = fv[0];
  const Dual xi = a.U[0], Hu = a.U[S], Hv = a.U[2 * S];
  const Dual D = xi + bath;
  const Dual uHu = Hu * Hu / D, uHv = Hu * Hv / D, vHv = Hv * Hv / D;
  const Dual pres = (D * D - bath * bath) * (0.5 * g);
  F[0] = a.Ud[0] - fv[3];
  F[1] = -Hu;
  F[2] = -Hv;
  F[S] = a.Ud[S] - xi * (g * fv[1]) - fv[4];
  F[S + 1] = -(uHu + pres);
  F[S + 2] = -uHv;
  F[2 * S] = a.Ud[2 * S] - xi * (g * fv[2]) - fv[5];
  F[2 * S + 1] = -uHv;
  F[2 * S + 2] = -(vHv + pres);
}

}  // namespace mha
