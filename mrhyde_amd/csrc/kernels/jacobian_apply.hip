// jacobian_apply.hip -- matrix-free products y += A x and y += A^T x with the volume Jacobian of a point-function module.
//
// A is the matrix the point engine (point_engine.hip) assembles into the CRS: in that file's notation
//   A_ij = sgn_i sgn_j sum_q T^(i,q)^T C^(q) T^(j,q),   C^ = w G^T (dF/dU) G (alpha_u; alpha_t on the value-like slots),
// with the rows the mesh marks fixed left at zero.  Neither A nor an element matrix nor C^ is formed.  With the
// reference-slot fields of x,  X^(q,m) = sum_j sgn_j x_j T^_m(j,q):
//   forward     one evaluation of the point function per point, seeded with the direction G X^:
//               F^x(q) = w G^T F.d,   y_i += sgn_i sum_q T^(i,q) . F^x(q)            (fixed rows skipped)
//   transposed  one evaluation per (point, unit direction m) -- phase 3 of the engine -- contracted in the thread:
//               z^(q,m) = sum_s [w G^T F.d]_s X^(q,s),   y_j += sgn_j sum_q sum_m T^_m(j,q) z^(q,m)
//               (x read as zero on fixed rows, every row of y written)
// The reference has no counterpart beyond AssemblyManager::applyMassMatrixFree (assemblyManager.cpp:1582-1778): its
// Jacobian exists as a Tpetra CRS matrix only.
//
// One wavefront per element for every shape (no C^, no P panels: 22 KB per 89-dof navierstokes element), wave-level
// synchronisation only; as many wavefronts per workgroup as the LDS holds beside the tables; waves persistent over
// blocked element ranges.  y is written with atomics, like the engine's out.res.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device_math.hpp"
#include "engine_points.hpp"
#include "launch.hpp"

namespace mha {
namespace {

constexpr int kApplyMaxWaves = 8;
constexpr size_t kApplyLdsLimit = 160 * 1024;

// per-element LDS (doubles): u, udot, x, sign | geometry | U^, Udot^, X^, F^x or z^ | row (ints)
__host__ __device__ inline size_t apply_wave_doubles(const VarLayoutDev &vl, int geo) {
  const size_t n = vl.n_tot, NS = vl.ns_tot, NQ = vl.nq;
  return 4 * n + NQ * geo + 4 * NQ * NS + (n + 1) / 2;
}

template <int DIM, int PHYS, int EXPR, int TRANSPOSE>
__global__ __launch_bounds__(64 * kApplyMaxWaves) void jacobian_apply_kernel(BlockDev b, VarLayoutDev vl, PhysParamsDev pp,
                                                                             TimeDev tm, const double *__restrict__ x,
                                                                             double *__restrict__ y) {
  using L = Layout<PHYS, DIM>;
  constexpr int NS = L::NS, GEO = geo_size<DIM>();
  extern __shared__ double smem[];
  const int NQ = vl.nq, n = vl.n_tot, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, NW = blockDim.x >> 6;
  double *tab = smem;
  double *s_Uh = tab + vl.tables_size + wave * (int)apply_wave_doubles(vl, GEO);
  double *s_Udh = s_Uh + NQ * NS, *s_Xh = s_Udh + NQ * NS, *s_out = s_Xh + NQ * NS;
  double *s_geo = s_out + NQ * NS;
  double *s_u = s_geo + NQ * GEO, *s_ud = s_u + n, *s_x = s_ud + n, *s_sgn = s_x + n;
  int *s_row = reinterpret_cast<int *>(s_sgn + n);

  for (int k = tid; k < vl.tables_size; k += blockDim.x) tab[k] = vl.tables[k];
  __syncthreads();  // the only workgroup barrier: from here on a wave meets nobody

  // blocked element ranges per wave: waves running at the same time work far apart in the mesh
  const int nwaves = gridDim.x * NW, gid = blockIdx.x * NW + wave;
  const int chunk = (b.e_count + nwaves - 1) / nwaves;
  const int el_begin = gid * chunk, el_end = min(b.e_count, el_begin + chunk);
  // layout of the variable that holds slot m / dof f (compile-time variable count: see point_engine.hip)
  struct VarAt { int sp, nsl, card, cp, vp, to; };
  auto var_at = [&](int key, bool by_slot) {
    VarAt r = {vl.slotptr[0], vl.nslot[0], vl.card[0], vl.cardpad[0], vl.varptr[0], vl.table_off[0]};
#pragma unroll
    for (int k = 1; k < L::nvars; ++k)
      if (key >= (by_slot ? vl.slotptr[k] : vl.varptr[k]))
        r = {vl.slotptr[k], vl.nslot[k], vl.card[k], vl.cardpad[k], vl.varptr[k], vl.table_off[k]};
    return r;
  };
  for (int el = el_begin; el < el_end; ++el) {
    const int e = b.e_begin + el;
    wave_lds_sync();  // previous element done with the wave's LDS
    // ---- 1. gather u, x + seeding values (x orientation sign), geometry ----
    for (int f = lane; f < n; f += 64) {
      const int pos = b.offsets[f], row = b.lids[(size_t)e * n + pos];
      const double sg = vl.orient ? (double)vl.orient[(size_t)e * n + f] : 1.0;
      double ue, ud, xv = x[row];
      stage_state(tm, row, tm.u[row], ue, ud);
      if (TRANSPOSE && b.fixed && b.fixed[row]) xv = 0.0;  // A has no entries in that row
      s_u[f] = ue * sg;
      s_ud[f] = ud * sg;
      s_x[f] = xv * sg;
      s_sgn[f] = sg;
      s_row[f] = row;
    }
    for (int q = lane; q < NQ; q += 64) MHA_POINT_GEOMETRY(b, e, q, NQ, s_geo + q * GEO);
    wave_lds_sync();
    // ---- 2. reference-slot fields of u, udot and x ----
    for (int idx = lane; idx < NQ * NS; idx += 64) {
      const int q = idx / NS, m = idx - q * NS;
      const VarAt va = var_at(m, true);
      const int sl = m - va.sp, card = va.card;
      const double *T = tab + va.to + (q * va.nsl + sl) * va.cp;
      const double *uu = s_u + va.vp, *ud = s_ud + va.vp, *xx = s_x + va.vp;
      double a = 0.0, ad = 0.0, ax = 0.0;
      if (tm.transient) {
#pragma unroll 4
        for (int dof = 0; dof < card; ++dof) {
          a += uu[dof] * T[dof];
          ad += ud[dof] * T[dof];
          ax += xx[dof] * T[dof];
        }
      } else {  // steady: the time-derivative coefficients are zero
#pragma unroll 4
        for (int dof = 0; dof < card; ++dof) {
          a += uu[dof] * T[dof];
          ax += xx[dof] * T[dof];
        }
      }
      s_Uh[idx] = a;
      s_Udh[idx] = ad;
      s_Xh[idx] = ax;
    }
    wave_lds_sync();
    // ---- 3. point function: forward one thread per point (direction G X^), transposed one per (point, direction) ----
    double vol = 0.0;
    for (int q = 0; q < NQ; ++q) vol += s_geo[q * GEO + 2 * DIM * DIM + 1];
    const double h = (DIM == 2) ? sqrt(vol) : cbrt(vol);  // Workset::getElementSize (workset.cpp:2666-2679)
    for (int idx = lane; idx < (TRANSPOSE ? NQ * NS : NQ); idx += 64) {
      const int q = TRANSPOSE ? idx / NS : idx, m = TRANSPOSE ? idx - q * NS : 0;
      const double *g = s_geo + q * GEO;
      const double *J = g, *Ji = g + DIM * DIM;
      const double det = g[2 * DIM * DIM], w = g[2 * DIM * DIM + 1];
      Dual U[NS], Ud[NS], F[NS];
#pragma unroll
      for (int v = 0; v < L::nvars; ++v) {
        const int type = L::type(v), sp = slotptr_of<L, DIM>(v), ns = slots_of(type, DIM);
        double ref[1 + DIM], phys[1 + DIM], refd[1 + DIM], physd[1 + DIM], dir[1 + DIM], pdir[1 + DIM];
#pragma unroll
        for (int sl = 0; sl < ns; ++sl) {
          ref[sl] = s_Uh[q * NS + sp + sl];
          refd[sl] = s_Udh[q * NS + sp + sl];
          dir[sl] = TRANSPOSE ? ((m == sp + sl) ? 1.0 : 0.0) : s_Xh[q * NS + sp + sl];
        }
        to_phys<DIM>(type, ref, J, Ji, det, phys);
        to_phys<DIM>(type, refd, J, Ji, det, physd);
        to_phys<DIM>(type, dir, J, Ji, det, pdir);
#pragma unroll
        for (int sl = 0; sl < ns; ++sl) {
          U[sp + sl] = mk(phys[sl], tm.alpha_u * pdir[sl]);
          Ud[sp + sl] = value_like(type, sl, DIM) ? mk(physd[sl], tm.alpha_t * pdir[sl]) : mk(0.0);
        }
      }
      PointArgs<DIM> pa;
      pa.U = U; pa.Ud = Ud; pa.x = g + 2 * DIM * DIM + 2; pa.h = h; pa.dt = tm.dt;
      pa.transient = tm.transient; pa.e = e; pa.q = q; pa.nq = NQ; pa.pp = &pp;
      MHA_MODULE_POINT(pa, F);
      double z = 0.0;
#pragma unroll
      for (int v = 0; v < L::nvars; ++v) {
        const int type = L::type(v), sp = slotptr_of<L, DIM>(v), ns = slots_of(type, DIM);
        double phys[1 + DIM], ref[1 + DIM];
#pragma unroll
        for (int sl = 0; sl < ns; ++sl) phys[sl] = F[sp + sl].d;
        to_ref_T<DIM>(type, phys, J, Ji, det, ref);
#pragma unroll
        for (int sl = 0; sl < ns; ++sl) {
          if (TRANSPOSE) z += w * ref[sl] * s_Xh[q * NS + sp + sl];
          else s_out[q * NS + sp + sl] = w * ref[sl];
        }
      }
      if (TRANSPOSE) s_out[idx] = z;
    }
    wave_lds_sync();
    // ---- 4. rows of y ----
    for (int f = lane; f < n; f += 64) {
      const VarAt va = var_at(f, false);
      const double *T = tab + va.to + (f - va.vp);
      const double *o = s_out + va.sp;
      double r = 0.0;
      if (va.nsl == 1) {
#pragma unroll 4
        for (int q = 0; q < NQ; ++q) r += T[q * va.cp] * o[q * NS];
      } else {
#pragma unroll 3
        for (int q = 0; q < NQ; ++q) {
#pragma unroll
          for (int sl = 0; sl < 1 + DIM; ++sl) r += T[(q * (1 + DIM) + sl) * va.cp] * o[q * NS + sl];
        }
      }
      const int row = s_row[f];
      if (!TRANSPOSE && b.fixed && b.fixed[row]) continue;
      unsafeAtomicAdd(y + row, r * s_sgn[f]);
    }
  }
}

template <int DIM, int PHYS>
void launch_typed(const BlockDev &b, const VarLayoutDev &vl, const PhysParamsDev &pp, const TimeDev &tm, const double *x,
                  double *y, int transpose, int overwrite, hipStream_t stream, size_t *lds_bytes, int *waves) {
  using L = Layout<PHYS, DIM>;
  MHA_REQUIRE(vl.nvars == L::nvars && vl.ns_tot == L::NS, MHA_ERR_INVALID,
              "variable layout does not match the physics module (" << vl.nvars << " variables, " << vl.ns_tot
                                                                    << " slots)");
  for (int v = 0; v < L::nvars; ++v)
    MHA_REQUIRE(vl.type[v] == L::type(v), MHA_ERR_INVALID, "basis type of variable " << v << " does not match the module");
  // as many elements (wavefronts) per workgroup as the LDS holds beside the tables
  const size_t per_wave = apply_wave_doubles(vl, geo_size<DIM>()) * sizeof(double);
  const size_t tables = vl.tables_size * sizeof(double);
  MHA_REQUIRE(tables + per_wave <= kApplyLdsLimit, MHA_ERR_INVALID,
              "element needs " << tables + per_wave << " B of LDS (limit 160 KB)");
  const int nw = static_cast<int>(std::min<size_t>(kApplyMaxWaves, (kApplyLdsLimit - tables) / per_wave));
  const size_t lds = tables + nw * per_wave;
  const int num_cu = current_device_num_cus();
  const int per_cu = static_cast<int>(std::max<size_t>(1, std::min<size_t>(size_t(4), kApplyLdsLimit / lds)));
  const int grid = std::max(1, std::min((b.e_count + nw - 1) / nw, num_cu * per_cu));
  if (lds_bytes) *lds_bytes = lds;
  if (waves) *waves = nw;
  auto go = [&](auto kern) {
    require_modest_scratch(kern, "Jacobian product");
    MHA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(kApplyLdsLimit)));
    if (overwrite) MHA_HIP(hipMemsetAsync(y, 0, sizeof(double) * b.nrows, stream));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * nw), lds, stream, b, vl, pp, tm, x, y);
    MHA_HIP(hipGetLastError());
  };
  auto pick = [&](auto expr) {
    constexpr int E = decltype(expr)::value;
    if (transpose) go(jacobian_apply_kernel<DIM, PHYS, E, 1>);
    else go(jacobian_apply_kernel<DIM, PHYS, E, 0>);
  };
  if (uses_fields(pp)) {
    // deck strings that read the solution fields: built for the modules whose point function has an EXPR = 2 form
    if constexpr (PHYS == MHA_PHYSICS_THERMAL || PHYS == MHA_PHYSICS_CDR || PHYS == MHA_PHYSICS_NAVIERSTOKES_CDR) {
      pick(std::integral_constant<int, 2>());
    } else {
      MHA_REQUIRE(false, MHA_ERR_INVALID, "functions of the solution fields are built for the thermal module");
    }
  } else if (PHYS == MHA_PHYSICS_POROUS_MIXED && (pp.het.edata || pp.het.kl)) {
    if constexpr (PHYS == MHA_PHYSICS_POROUS_MIXED) {
      MHA_REQUIRE(!has_expression(pp), MHA_ERR_INVALID,
                  "porousMixed: heterogeneous permeability with deck-string functions is not built; give source / mobility as constants or closed forms");
      pick(std::integral_constant<int, 3>());
    }
  } else if (has_expression(pp)) {
    pick(std::integral_constant<int, 1>());
  } else {
    pick(std::integral_constant<int, 0>());
  }
}

}  // namespace

void launch_jacobian_apply(const BlockDev &b, const VarLayoutDev &vl, const PhysParamsDev &pp, const TimeDev &tm,
                           const double *x, double *y, int transpose, int overwrite, hipStream_t stream,
                           size_t *lds_bytes, int *waves) {
  MHA_REQUIRE(x && y, MHA_ERR_INVALID, "null vector");
  MHA_REQUIRE(pp.physics > 0, MHA_ERR_INVALID, "no physics module");
  if (b.e_count <= 0) {
    if (overwrite) MHA_HIP(hipMemsetAsync(y, 0, sizeof(double) * b.nrows, stream));
    return;
  }
  static_assert(MHA_PHYSICS_HELMHOLTZ < 100, "the switch key holds two decimal digits of module id");
#define MHA_APPLY_CASE(D, P) \
  case D * 100 + P: launch_typed<D, P>(b, vl, pp, tm, x, y, transpose, overwrite, stream, lds_bytes, waves); break;
  switch (b.dim * 100 + pp.physics) {
    MHA_APPLY_CASE(2, MHA_PHYSICS_THERMAL)
    MHA_APPLY_CASE(3, MHA_PHYSICS_THERMAL)
    MHA_APPLY_CASE(2, MHA_PHYSICS_POROUS_MIXED)
    MHA_APPLY_CASE(3, MHA_PHYSICS_POROUS_MIXED)
    MHA_APPLY_CASE(2, MHA_PHYSICS_NAVIERSTOKES)
    MHA_APPLY_CASE(3, MHA_PHYSICS_NAVIERSTOKES)
    MHA_APPLY_CASE(2, MHA_PHYSICS_NAVIERSTOKES_THERMAL)
    MHA_APPLY_CASE(3, MHA_PHYSICS_NAVIERSTOKES_THERMAL)
    MHA_APPLY_CASE(2, MHA_PHYSICS_LINEARELASTICITY)
    MHA_APPLY_CASE(3, MHA_PHYSICS_LINEARELASTICITY)
    MHA_APPLY_CASE(2, MHA_PHYSICS_LINEARELASTICITY_THERMAL)
    MHA_APPLY_CASE(3, MHA_PHYSICS_LINEARELASTICITY_THERMAL)
    MHA_APPLY_CASE(2, MHA_PHYSICS_CDR)
    MHA_APPLY_CASE(3, MHA_PHYSICS_CDR)
    MHA_APPLY_CASE(2, MHA_PHYSICS_NAVIERSTOKES_CDR)
    MHA_APPLY_CASE(3, MHA_PHYSICS_NAVIERSTOKES_CDR)
    MHA_APPLY_CASE(2, MHA_PHYSICS_HELMHOLTZ)
    MHA_APPLY_CASE(3, MHA_PHYSICS_HELMHOLTZ)
    MHA_APPLY_CASE(2, MHA_PHYSICS_SHALLOWWATER_HYBRIDIZED)
    default: MHA_REQUIRE(false, MHA_ERR_INVALID, "no Jacobian-product kernel for physics " << pp.physics << " in " << b.dim << "-D");
  }
#undef MHA_APPLY_CASE
}

}  // namespace mha
