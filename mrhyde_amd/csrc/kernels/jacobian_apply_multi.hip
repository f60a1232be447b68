// jacobian_apply_multi.hip -- the matrix-free products of jacobian_apply.hip for Kc vectors in one launch:
//   Y_k += A X_k   or   Y_k += A^T X_k,   k = 0 .. Kc-1,   vector k at x + k ldx / y + k ldy (a Krylov basis).
// That file's notation and matrix.  What does not depend on the vector is paid once per element: the gather of u, the
// geometry, U^ and Udot^, and in the transposed product the NQ NS evaluations of the point function.
//   phase 1-2   u once, x for the Kc vectors; U^, Udot^ once and X^_k per vector (work items (point, slot, field))
//   forward     work items (point q, vector k), NQ Kc of them over the 64 lanes: one evaluation seeded with G X^_k(q).
//               The single product keeps NQ lanes busy here (8 at Q1 in 3-D, 9 at Q2 in 2-D, 27 at Q2 in 3-D).
//   transposed  work items (point, unit direction m) as in the single product: one evaluation, then Kc contractions
//               z^_k(q,m) = sum_s C^_sm X^_k(q,s) in the thread
//   phase 4     work items (dof, vector), atomics into Y_k
// Kc is a kernel argument, not a template parameter: the instantiations are the single product's 84.  The launcher
// takes nvec vectors in passes of Kc <= MHA_APPLY_MAX_VECTORS and chooses Kc per shape (choose_vectors); a pass of one
// vector runs jacobian_apply.hip's kernel.
//
// Layout as in jacobian_apply.hip: one wavefront per element, wave-level synchronisation only, waves persistent over
// blocked element ranges.  Self-contained: the statements shared with jacobian_apply.hip are repeated here rather
// than moved to a header, so that file's kernels stay what they were.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device_math.hpp"
#include "engine_points.hpp"
#include "launch.hpp"

namespace mha {
namespace {

constexpr int kMultiMaxWaves = 8;
constexpr size_t kMultiLdsLimit = 160 * 1024;

// per-element LDS (doubles): u, udot, sign, x_k | geometry | U^, Udot^, X^_k, F^x_k or z^_k | row (ints)
__host__ __device__ inline size_t multi_wave_doubles(const VarLayoutDev &vl, int geo, int kc) {
  const size_t n = vl.n_tot, NS = vl.ns_tot, NQ = vl.nq;
  return (3 + kc) * n + NQ * geo + (2 + 2 * kc) * NQ * NS + (n + 1) / 2;
}

template <int DIM, int PHYS, int EXPR, int TRANSPOSE>
__global__ __launch_bounds__(64 * kMultiMaxWaves) void jacobian_apply_multi_kernel(
    BlockDev b, VarLayoutDev vl, PhysParamsDev pp, TimeDev tm, int Kc, const double *__restrict__ x, int64_t ldx,
    double *__restrict__ y, int64_t ldy) {
  using L = Layout<PHYS, DIM>;
  constexpr int NS = L::NS, GEO = geo_size<DIM>();
  extern __shared__ double smem[];
  const int NQ = vl.nq, n = vl.n_tot, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, NW = blockDim.x >> 6;
  const int QS = NQ * NS;
  double *tab = smem;
  double *s_Uh = tab + vl.tables_size + wave * (int)multi_wave_doubles(vl, GEO, Kc);
  double *s_Udh = s_Uh + QS, *s_Xh = s_Udh + QS, *s_out = s_Xh + Kc * QS;  // X^_k at s_Xh + k QS, output k at s_out + k QS
  double *s_geo = s_out + Kc * QS;
  double *s_u = s_geo + NQ * GEO, *s_ud = s_u + n, *s_sgn = s_ud + n, *s_x = s_sgn + n;  // x_k at s_x + k n
  int *s_row = reinterpret_cast<int *>(s_x + Kc * n);

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
    // ---- 1. gather u + seeding values once, x_k (x orientation sign) per vector, geometry ----
    for (int f = lane; f < n; f += 64) {
      const int pos = b.offsets[f], row = b.lids[(size_t)e * n + pos];
      const double sg = vl.orient ? (double)vl.orient[(size_t)e * n + f] : 1.0;
      double ue, ud;
      stage_state(tm, row, tm.u[row], ue, ud);
      const bool zero = TRANSPOSE && b.fixed && b.fixed[row];  // A has no entries in that row
      s_u[f] = ue * sg;
      s_ud[f] = ud * sg;
      s_sgn[f] = sg;
      s_row[f] = row;
      for (int k = 0; k < Kc; ++k) s_x[k * n + f] = zero ? 0.0 : x[k * ldx + row] * sg;
    }
    for (int q = lane; q < NQ; q += 64) MHA_POINT_GEOMETRY(b, e, q, NQ, s_geo + q * GEO);
    wave_lds_sync();
    // ---- 2. reference-slot fields: items (point, slot, field), field 0 = u and udot, field 1 + k = x_k ----
    for (int item = lane; item < QS * (1 + Kc); item += 64) {
      const int t = item / QS, idx = item - t * QS;
      const int q = idx / NS, m = idx - q * NS;
      const VarAt va = var_at(m, true);
      const int sl = m - va.sp, card = va.card;
      const double *T = tab + va.to + (q * va.nsl + sl) * va.cp;
      if (t == 0) {
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
      } else {
        const double *xx = s_x + (t - 1) * n + va.vp;
        double ax = 0.0;
#pragma unroll 4
        for (int dof = 0; dof < card; ++dof) ax += xx[dof] * T[dof];
        s_Xh[(t - 1) * QS + idx] = ax;
      }
    }
    wave_lds_sync();
    // ---- 3. point function: forward items (point, vector), direction G X^_k; transposed items (point, direction) ----
    double vol = 0.0;
    for (int q = 0; q < NQ; ++q) vol += s_geo[q * GEO + 2 * DIM * DIM + 1];
    const double h = (DIM == 2) ? sqrt(vol) : cbrt(vol);  // Workset::getElementSize (workset.cpp:2666-2679)
    for (int idx = lane; idx < (TRANSPOSE ? QS : NQ * Kc); idx += 64) {
      const int kv = TRANSPOSE ? 0 : idx / NQ;  // forward: the item's vector
      const int q = TRANSPOSE ? idx / NS : idx - kv * NQ, m = TRANSPOSE ? idx - q * NS : 0;
      const double *g = s_geo + q * GEO;
      const double *J = g, *Ji = g + DIM * DIM;
      const double det = g[2 * DIM * DIM], w = g[2 * DIM * DIM + 1];
      const double *Xk = s_Xh + kv * QS + q * NS;
      Dual U[NS], Ud[NS], F[NS];
#pragma unroll
      for (int v = 0; v < L::nvars; ++v) {
        const int type = L::type(v), sp = slotptr_of<L, DIM>(v), ns = slots_of(type, DIM);
        double ref[1 + DIM], phys[1 + DIM], refd[1 + DIM], physd[1 + DIM], dir[1 + DIM], pdir[1 + DIM];
#pragma unroll
        for (int sl = 0; sl < ns; ++sl) {
          ref[sl] = s_Uh[q * NS + sp + sl];
          refd[sl] = s_Udh[q * NS + sp + sl];
          dir[sl] = TRANSPOSE ? ((m == sp + sl) ? 1.0 : 0.0) : Xk[sp + sl];
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
      double col[NS];  // w G^T F.d: forward F^x_k(q), transposed column m of C^(q)
#pragma unroll
      for (int v = 0; v < L::nvars; ++v) {
        const int type = L::type(v), sp = slotptr_of<L, DIM>(v), ns = slots_of(type, DIM);
        double phys[1 + DIM], ref[1 + DIM];
#pragma unroll
        for (int sl = 0; sl < ns; ++sl) phys[sl] = F[sp + sl].d;
        to_ref_T<DIM>(type, phys, J, Ji, det, ref);
#pragma unroll
        for (int sl = 0; sl < ns; ++sl) col[sp + sl] = w * ref[sl];
      }
      if (TRANSPOSE) {
        for (int k = 0; k < Kc; ++k) {
          const double *xh = s_Xh + k * QS + q * NS;
          double z = 0.0;
#pragma unroll
          for (int s = 0; s < NS; ++s) z += col[s] * xh[s];
          s_out[k * QS + idx] = z;
        }
      } else {
#pragma unroll
        for (int s = 0; s < NS; ++s) s_out[kv * QS + q * NS + s] = col[s];
      }
    }
    wave_lds_sync();
    // ---- 4. rows of Y_k: items (dof, vector) ----
    for (int item = lane; item < n * Kc; item += 64) {
      const int k = item / n, f = item - k * n;
      const int row = s_row[f];
      if (!TRANSPOSE && b.fixed && b.fixed[row]) continue;
      const VarAt va = var_at(f, false);
      const double *T = tab + va.to + (f - va.vp);
      const double *o = s_out + k * QS + va.sp;
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
      unsafeAtomicAdd(y + k * ldy + row, r * s_sgn[f]);
    }
  }
}

// How many vectors one launch carries for this shape.  Each vector adds n + 2 NQ NS doubles per element, and the LDS
// left beside the tables decides how many elements (wavefronts) a workgroup holds.  Measured (profiles/jacobian_apply.md):
// every shape that keeps seven or eight wavefronts per workgroup gains with each doubling of Kc up to 8 (2 to 5 times
// per vector at Kc = 8), although fewer workgroups fit a CU; the 89-dof 3-D Q2/Q1 element, which holds six wavefronts
// in the single product and four at Kc = 2, loses there (1.19 x per vector forward, 1.04 x transposed) and more beyond:
// the products run at the rate of the wavefronts in flight, and the work the vectors share does not pay for a third
// of them.  Rule: the largest Kc <= min(nvec, MHA_APPLY_MAX_VECTORS) that leaves kMultiMinWaves wavefronts per
// workgroup, or all the single product has where those are fewer; Kc = 1 if none does.  A pass of one vector -- that
// case, and a remainder of one -- runs the single product's kernel: K vectors then cost what K single calls cost.
constexpr int kMultiMinWaves = 7;

inline int waves_for(const VarLayoutDev &vl, int geo, size_t tables, int kc) {
  const size_t per_wave = multi_wave_doubles(vl, geo, kc) * sizeof(double);
  if (tables + per_wave > kMultiLdsLimit) return 0;
  return static_cast<int>(std::min<size_t>(kMultiMaxWaves, (kMultiLdsLimit - tables) / per_wave));
}

inline int choose_vectors(const VarLayoutDev &vl, int geo, size_t tables, int nvec) {
  const int want = std::min(kMultiMinWaves, waves_for(vl, geo, tables, 1));
  int kc = std::min(nvec, MHA_APPLY_MAX_VECTORS);
  while (kc > 1 && waves_for(vl, geo, tables, kc) < want) --kc;
  return kc;
}

template <int DIM, int PHYS>
void launch_typed(const BlockDev &b, const VarLayoutDev &vl, const PhysParamsDev &pp, const TimeDev &tm, int nvec,
                  const double *x, int64_t ldx, double *y, int64_t ldy, int transpose, int overwrite, hipStream_t stream,
                  size_t *lds_bytes, int *waves, int *vectors) {
  using L = Layout<PHYS, DIM>;
  MHA_REQUIRE(vl.nvars == L::nvars && vl.ns_tot == L::NS, MHA_ERR_INVALID,
              "variable layout does not match the physics module (" << vl.nvars << " variables, " << vl.ns_tot
                                                                    << " slots)");
  for (int v = 0; v < L::nvars; ++v)
    MHA_REQUIRE(vl.type[v] == L::type(v), MHA_ERR_INVALID, "basis type of variable " << v << " does not match the module");
  const size_t tables = vl.tables_size * sizeof(double);
  MHA_REQUIRE(waves_for(vl, geo_size<DIM>(), tables, 1) >= 1, MHA_ERR_INVALID,
              "element needs " << tables + multi_wave_doubles(vl, geo_size<DIM>(), 1) * sizeof(double)
                               << " B of LDS (limit 160 KB)");
  const int kc_max = choose_vectors(vl, geo_size<DIM>(), tables, nvec);
  const int num_cu = current_device_num_cus();
  auto go = [&](auto kern) {
    require_modest_scratch(kern, "Jacobian product");
    MHA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(kMultiLdsLimit)));
    // passes of kc_max vectors and a remainder; each pass sized for its own Kc and zeroing its own vectors first
    for (int k0 = 0; k0 < nvec; k0 += kc_max) {
      const int kc = std::min(kc_max, nvec - k0);
      const size_t per_wave = multi_wave_doubles(vl, geo_size<DIM>(), kc) * sizeof(double);
      const int nw = waves_for(vl, geo_size<DIM>(), tables, kc);
      const size_t lds = tables + nw * per_wave;
      const int per_cu = static_cast<int>(std::max<size_t>(1, std::min<size_t>(size_t(4), kMultiLdsLimit / lds)));
      const int grid = std::max(1, std::min((b.e_count + nw - 1) / nw, num_cu * per_cu));
      if (k0 == 0) {  // reported: the first (full) pass
        if (lds_bytes) *lds_bytes = lds;
        if (waves) *waves = nw;
        if (vectors) *vectors = kc;
      }
      if (kc == 1) {  // the single product's launch: same checks, same dispatch, same memset
        launch_jacobian_apply(b, vl, pp, tm, x + k0 * ldx, y + k0 * ldy, transpose, overwrite, stream);
        continue;
      }
      if (overwrite)  // the vectors, not the padding between them
        MHA_HIP(hipMemset2DAsync(y + k0 * ldy, sizeof(double) * ldy, 0, sizeof(double) * b.nrows, kc, stream));
      hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * nw), lds, stream, b, vl, pp, tm, kc, x + k0 * ldx, ldx, y + k0 * ldy,
                         ldy);
      MHA_HIP(hipGetLastError());
    }
  };
  auto pick = [&](auto expr) {
    constexpr int E = decltype(expr)::value;
    if (transpose) go(jacobian_apply_multi_kernel<DIM, PHYS, E, 1>);
    else go(jacobian_apply_multi_kernel<DIM, PHYS, E, 0>);
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

void launch_jacobian_apply_multi(const BlockDev &b, const VarLayoutDev &vl, const PhysParamsDev &pp, const TimeDev &tm,
                                 int nvec, const double *x, int64_t ldx, double *y, int64_t ldy, int transpose,
                                 int overwrite, hipStream_t stream, size_t *lds_bytes, int *waves, int *vectors) {
  MHA_REQUIRE(x && y, MHA_ERR_INVALID, "null vector");
  MHA_REQUIRE(nvec >= 1, MHA_ERR_INVALID, "nvec = " << nvec << ": at least one vector");
  MHA_REQUIRE(ldx >= b.nrows && ldy >= b.nrows, MHA_ERR_INVALID,
              "ldx = " << ldx << ", ldy = " << ldy << ": a vector holds nrows = " << b.nrows << " entries");
  MHA_REQUIRE(pp.physics > 0, MHA_ERR_INVALID, "no physics module");
  if (b.e_count <= 0) {
    if (overwrite) MHA_HIP(hipMemset2DAsync(y, sizeof(double) * ldy, 0, sizeof(double) * b.nrows, nvec, stream));
    return;
  }
  static_assert(MHA_PHYSICS_HELMHOLTZ < 100, "the switch key holds two decimal digits of module id");
#define MHA_APPLY_CASE(D, P)                                                                                              \
  case D * 100 + P:                                                                                                       \
    launch_typed<D, P>(b, vl, pp, tm, nvec, x, ldx, y, ldy, transpose, overwrite, stream, lds_bytes, waves, vectors);     \
    break;
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
