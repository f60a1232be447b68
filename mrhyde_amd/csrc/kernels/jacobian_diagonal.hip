// jacobian_diagonal.hip -- d += diag(A) with the volume Jacobian of a point-function module, matrix-free.
//
// A is the matrix of jacobian_apply.hip (that file's notation): for dof i of variable v
//   A_ii = sum_q sum_{s,m in slots(v)} T^_s(i,q) C^_sm(q) T^_m(i,q),   C^ = w G^T (dF/dU) G,
// the orientation sign squared away, rows the mesh marks fixed left alone.  Phase 3 is the transposed product's: one
// evaluation per (point, unit direction m); the thread's w G^T F.d is column m of C^(q), of which the rows s in the
// variable of m are kept -- NQ sum_v ns_v^2 doubles in place of the product's output array.  Phase 4: one lane per dof
// contracts its variable's block with its own table rows on both sides.  No x, no X^.
//
// Layout as in jacobian_apply.hip: one wavefront per element, wave-level synchronisation only, as many wavefronts per
// workgroup as the LDS holds beside the tables, waves persistent over blocked element ranges, d written with atomics.
// Self-contained: phases 1-2 and the seeding repeat jacobian_apply.hip's statements rather than share them through
// a header, so that file's kernels stay what they were.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device_math.hpp"
#include "engine_points.hpp"
#include "launch.hpp"

namespace mha {
namespace {

constexpr int kDiagMaxWaves = 8;
constexpr size_t kDiagLdsLimit = 160 * 1024;

// sum_v ns_v^2: the doubles of the kept blocks of C^ at one point
template <class L, int DIM>
__host__ __device__ constexpr int coupling_size(int nv = L::nvars) {
  int p = 0;
  for (int k = 0; k < nv; ++k) p += slots_of(L::type(k), DIM) * slots_of(L::type(k), DIM);
  return p;
}

// per-element LDS (doubles): u, udot | geometry | U^, Udot^ | blocks of C^ | row (ints).  The orientation sign is used
// in the gather alone (it squares to 1 in A_ii) and is not kept.
__host__ __device__ inline size_t diag_wave_doubles(const VarLayoutDev &vl, int geo, int cs) {
  const size_t n = vl.n_tot, NS = vl.ns_tot, NQ = vl.nq;
  return 2 * n + NQ * geo + 2 * NQ * NS + NQ * cs + (n + 1) / 2;
}

template <int DIM, int PHYS, int EXPR>
__global__ __launch_bounds__(64 * kDiagMaxWaves) void jacobian_diagonal_kernel(BlockDev b, VarLayoutDev vl, PhysParamsDev pp,
                                                                               TimeDev tm, double *__restrict__ d) {
  using L = Layout<PHYS, DIM>;
  constexpr int NS = L::NS, GEO = geo_size<DIM>(), CS = coupling_size<L, DIM>();
  extern __shared__ double smem[];
  const int NQ = vl.nq, n = vl.n_tot, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, NW = blockDim.x >> 6;
  double *tab = smem;
  double *s_Uh = tab + vl.tables_size + wave * (int)diag_wave_doubles(vl, GEO, CS);
  double *s_Udh = s_Uh + NQ * NS, *s_C = s_Udh + NQ * NS;
  double *s_geo = s_C + NQ * CS;
  double *s_u = s_geo + NQ * GEO, *s_ud = s_u + n;
  int *s_row = reinterpret_cast<int *>(s_ud + n);

  for (int k = tid; k < vl.tables_size; k += blockDim.x) tab[k] = vl.tables[k];
  __syncthreads();  // the only workgroup barrier: from here on a wave meets nobody

  const int nwaves = gridDim.x * NW, gid = blockIdx.x * NW + wave;
  const int chunk = (b.e_count + nwaves - 1) / nwaves;
  const int el_begin = gid * chunk, el_end = min(b.e_count, el_begin + chunk);
  // layout of the variable that holds slot m / dof f; co: offset of its block of C^
  struct VarAt { int sp, nsl, card, cp, vp, to, co; };
  auto var_at = [&](int key, bool by_slot) {
    VarAt r = {vl.slotptr[0], vl.nslot[0], vl.card[0], vl.cardpad[0], vl.varptr[0], vl.table_off[0], 0};
#pragma unroll
    for (int k = 1; k < L::nvars; ++k)
      if (key >= (by_slot ? vl.slotptr[k] : vl.varptr[k]))
        r = {vl.slotptr[k], vl.nslot[k], vl.card[k], vl.cardpad[k], vl.varptr[k], vl.table_off[k], coupling_size<L, DIM>(k)};
    return r;
  };
  for (int el = el_begin; el < el_end; ++el) {
    const int e = b.e_begin + el;
    wave_lds_sync();  // previous element done with the wave's LDS
    // ---- 1. gather u + seeding values, geometry ----
    for (int f = lane; f < n; f += 64) {
      const int pos = b.offsets[f], row = b.lids[(size_t)e * n + pos];
      const double sg = vl.orient ? (double)vl.orient[(size_t)e * n + f] : 1.0;
      double ue, ud;
      stage_state(tm, row, tm.u[row], ue, ud);
      s_u[f] = ue * sg;
      s_ud[f] = ud * sg;
      s_row[f] = row;
    }
    for (int q = lane; q < NQ; q += 64) MHA_POINT_GEOMETRY(b, e, q, NQ, s_geo + q * GEO);
    wave_lds_sync();
    // ---- 2. reference-slot fields of u and udot ----
    for (int idx = lane; idx < NQ * NS; idx += 64) {
      const int q = idx / NS, m = idx - q * NS;
      const VarAt va = var_at(m, true);
      const int sl = m - va.sp, card = va.card;
      const double *T = tab + va.to + (q * va.nsl + sl) * va.cp;
      const double *uu = s_u + va.vp, *ud = s_ud + va.vp;
      double a = 0.0, ad = 0.0;
      if (tm.transient) {
#pragma unroll 4
        for (int dof = 0; dof < card; ++dof) {
          a += uu[dof] * T[dof];
          ad += ud[dof] * T[dof];
        }
      } else {  // steady: the time-derivative coefficients are zero
#pragma unroll 4
        for (int dof = 0; dof < card; ++dof) a += uu[dof] * T[dof];
      }
      s_Uh[idx] = a;
      s_Udh[idx] = ad;
    }
    wave_lds_sync();
    // ---- 3. point function, one thread per (point, unit direction m): column m of C^(q), rows of m's variable ----
    double vol = 0.0;
    for (int q = 0; q < NQ; ++q) vol += s_geo[q * GEO + 2 * DIM * DIM + 1];
    const double h = (DIM == 2) ? sqrt(vol) : cbrt(vol);  // Workset::getElementSize (workset.cpp:2666-2679)
    for (int idx = lane; idx < NQ * NS; idx += 64) {
      const int q = idx / NS, m = idx - q * NS;
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
          dir[sl] = (m == sp + sl) ? 1.0 : 0.0;
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
#pragma unroll
      for (int v = 0; v < L::nvars; ++v) {
        const int type = L::type(v), sp = slotptr_of<L, DIM>(v), ns = slots_of(type, DIM);
        if (m < sp || m >= sp + ns) continue;  // the rows of another variable: off the diagonal
        double phys[1 + DIM], ref[1 + DIM];
#pragma unroll
        for (int sl = 0; sl < ns; ++sl) phys[sl] = F[sp + sl].d;
        to_ref_T<DIM>(type, phys, J, Ji, det, ref);
#pragma unroll
        for (int sl = 0; sl < ns; ++sl) s_C[q * CS + coupling_size<L, DIM>(v) + sl * ns + (m - sp)] = w * ref[sl];
      }
    }
    wave_lds_sync();
    // ---- 4. rows of d: T^(i,q)^T C^_vv(q) T^(i,q) ----
    for (int f = lane; f < n; f += 64) {
      const int row = s_row[f];
      if (b.fixed && b.fixed[row]) continue;
      const VarAt va = var_at(f, false);
      const double *T = tab + va.to + (f - va.vp);
      const double *c = s_C + va.co;
      double r = 0.0;
      if (va.nsl == 1) {
#pragma unroll 4
        for (int q = 0; q < NQ; ++q) r += T[q * va.cp] * c[q * CS] * T[q * va.cp];
      } else {
#pragma unroll 2
        for (int q = 0; q < NQ; ++q) {
          double t[1 + DIM];
#pragma unroll
          for (int sl = 0; sl < 1 + DIM; ++sl) t[sl] = T[(q * (1 + DIM) + sl) * va.cp];
#pragma unroll
          for (int sl = 0; sl < 1 + DIM; ++sl) {
            double cm = 0.0;
#pragma unroll
            for (int ml = 0; ml < 1 + DIM; ++ml) cm += c[q * CS + sl * (1 + DIM) + ml] * t[ml];
            r += t[sl] * cm;
          }
        }
      }
      unsafeAtomicAdd(d + row, r);
    }
  }
}

template <int DIM, int PHYS>
void launch_typed(const BlockDev &b, const VarLayoutDev &vl, const PhysParamsDev &pp, const TimeDev &tm, double *d,
                  int overwrite, hipStream_t stream, size_t *lds_bytes, int *waves) {
  using L = Layout<PHYS, DIM>;
  MHA_REQUIRE(vl.nvars == L::nvars && vl.ns_tot == L::NS, MHA_ERR_INVALID,
              "variable layout does not match the physics module (" << vl.nvars << " variables, " << vl.ns_tot
                                                                    << " slots)");
  for (int v = 0; v < L::nvars; ++v)
    MHA_REQUIRE(vl.type[v] == L::type(v), MHA_ERR_INVALID, "basis type of variable " << v << " does not match the module");
  // as many elements (wavefronts) per workgroup as the LDS holds beside the tables
  const size_t per_wave = diag_wave_doubles(vl, geo_size<DIM>(), coupling_size<L, DIM>()) * sizeof(double);
  const size_t tables = vl.tables_size * sizeof(double);
  MHA_REQUIRE(tables + per_wave <= kDiagLdsLimit, MHA_ERR_INVALID,
              "element needs " << tables + per_wave << " B of LDS (limit 160 KB)");
  const int nw = static_cast<int>(std::min<size_t>(kDiagMaxWaves, (kDiagLdsLimit - tables) / per_wave));
  const size_t lds = tables + nw * per_wave;
  const int num_cu = current_device_num_cus();
  const int per_cu = static_cast<int>(std::max<size_t>(1, std::min<size_t>(size_t(4), kDiagLdsLimit / lds)));
  const int grid = std::max(1, std::min((b.e_count + nw - 1) / nw, num_cu * per_cu));
  if (lds_bytes) *lds_bytes = lds;
  if (waves) *waves = nw;
  auto go = [&](auto kern) {
    require_modest_scratch(kern, "Jacobian diagonal");
    MHA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(kDiagLdsLimit)));
    if (overwrite) MHA_HIP(hipMemsetAsync(d, 0, sizeof(double) * b.nrows, stream));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * nw), lds, stream, b, vl, pp, tm, d);
    MHA_HIP(hipGetLastError());
  };
  if (uses_fields(pp)) {
    // deck strings that read the solution fields: built for the modules whose point function has an EXPR = 2 form
    if constexpr (PHYS == MHA_PHYSICS_THERMAL || PHYS == MHA_PHYSICS_CDR || PHYS == MHA_PHYSICS_NAVIERSTOKES_CDR) {
      go(jacobian_diagonal_kernel<DIM, PHYS, 2>);
    } else {
      MHA_REQUIRE(false, MHA_ERR_INVALID, "functions of the solution fields are built for the thermal module");
    }
  } else if (PHYS == MHA_PHYSICS_POROUS_MIXED && (pp.het.edata || pp.het.kl)) {
    if constexpr (PHYS == MHA_PHYSICS_POROUS_MIXED) {
      MHA_REQUIRE(!has_expression(pp), MHA_ERR_INVALID,
                  "porousMixed: heterogeneous permeability with deck-string functions is not built; give source / mobility as constants or closed forms");
      go(jacobian_diagonal_kernel<DIM, PHYS, 3>);
    }
  } else if (has_expression(pp)) {
    go(jacobian_diagonal_kernel<DIM, PHYS, 1>);
  } else {
    go(jacobian_diagonal_kernel<DIM, PHYS, 0>);
  }
}

}  // namespace

void launch_jacobian_diagonal(const BlockDev &b, const VarLayoutDev &vl, const PhysParamsDev &pp, const TimeDev &tm,
                              double *d, int overwrite, hipStream_t stream, size_t *lds_bytes, int *waves) {
  MHA_REQUIRE(d, MHA_ERR_INVALID, "null vector");
  MHA_REQUIRE(pp.physics > 0, MHA_ERR_INVALID, "no physics module");
  if (b.e_count <= 0) {
    if (overwrite) MHA_HIP(hipMemsetAsync(d, 0, sizeof(double) * b.nrows, stream));
    return;
  }
  static_assert(MHA_PHYSICS_HELMHOLTZ < 100, "the switch key holds two decimal digits of module id");
#define MHA_DIAG_CASE(D, P) \
  case D * 100 + P: launch_typed<D, P>(b, vl, pp, tm, d, overwrite, stream, lds_bytes, waves); break;
  switch (b.dim * 100 + pp.physics) {
    MHA_DIAG_CASE(2, MHA_PHYSICS_THERMAL)
    MHA_DIAG_CASE(3, MHA_PHYSICS_THERMAL)
    MHA_DIAG_CASE(2, MHA_PHYSICS_POROUS_MIXED)
    MHA_DIAG_CASE(3, MHA_PHYSICS_POROUS_MIXED)
    MHA_DIAG_CASE(2, MHA_PHYSICS_NAVIERSTOKES)
    MHA_DIAG_CASE(3, MHA_PHYSICS_NAVIERSTOKES)
    MHA_DIAG_CASE(2, MHA_PHYSICS_NAVIERSTOKES_THERMAL)
    MHA_DIAG_CASE(3, MHA_PHYSICS_NAVIERSTOKES_THERMAL)
    MHA_DIAG_CASE(2, MHA_PHYSICS_LINEARELASTICITY)
    MHA_DIAG_CASE(3, MHA_PHYSICS_LINEARELASTICITY)
    MHA_DIAG_CASE(2, MHA_PHYSICS_LINEARELASTICITY_THERMAL)
    MHA_DIAG_CASE(3, MHA_PHYSICS_LINEARELASTICITY_THERMAL)
    MHA_DIAG_CASE(2, MHA_PHYSICS_CDR)
    MHA_DIAG_CASE(3, MHA_PHYSICS_CDR)
    MHA_DIAG_CASE(2, MHA_PHYSICS_NAVIERSTOKES_CDR)
    MHA_DIAG_CASE(3, MHA_PHYSICS_NAVIERSTOKES_CDR)
    MHA_DIAG_CASE(2, MHA_PHYSICS_HELMHOLTZ)
    MHA_DIAG_CASE(3, MHA_PHYSICS_HELMHOLTZ)
    MHA_DIAG_CASE(2, MHA_PHYSICS_SHALLOWWATER_HYBRIDIZED)
    default: MHA_REQUIRE(false, MHA_ERR_INVALID, "no Jacobian-diagonal kernel for physics " << pp.physics << " in " << b.dim << "-D");
  }
#undef MHA_DIAG_CASE
}

}  // namespace mha
