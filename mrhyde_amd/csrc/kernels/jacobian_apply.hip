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
// blocked element ranges.  y is written with atomics, like the engine's out.res.  The statements the element loop has in
// common with the other point-function kernels are engine_points.hpp's macros, the launcher's checks and choices
// engine_dispatch.hpp's; x rides in phase 2's loops over u, so that contraction is this file's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device_math.hpp"
#include "engine_dispatch.hpp"
#include "engine_points.hpp"
#include "launch.hpp"

namespace mha {
namespace {

// per-element LDS (doubles): u, udot, x, sign | geometry | U^, Udot^, X^, F^x or z^ | row (ints)
__host__ __device__ inline size_t apply_wave_doubles(const VarLayoutDev &vl, int geo) {
  const size_t n = vl.n_tot, NS = vl.ns_tot, NQ = vl.nq;
  return 4 * n + NQ * geo + 4 * NQ * NS + (n + 1) / 2;
}

template <int DIM, int PHYS, int EXPR, int TRANSPOSE>
__global__ __launch_bounds__(64 * kProductMaxWaves) void jacobian_apply_kernel(BlockDev b, VarLayoutDev vl, PhysParamsDev pp,
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

  MHA_WAVE_ELEMENT_RANGE(NW, wave);
  MHA_VAR_AT();
  for (int el = el_begin; el < el_end; ++el) {
    const int e = b.e_begin + el;
    wave_lds_sync();  // previous element done with the wave's LDS
    // ---- 1. gather u, x + seeding values (x orientation sign), geometry ----
    for (int f = lane; f < n; f += 64) {
      MHA_DOF_ROW(f);
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
      MHA_REF_SLOT(idx);
      const double *uu = s_u + va.vp, *ud = s_ud + va.vp, *xx = s_x + va.vp;
      double a = 0.0, ad = 0.0, ax = 0.0;  // x rides in the loops of u (MHA_REF_FIELDS has no place for it)
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
    MHA_ELEMENT_SIZE();
    for (int idx = lane; idx < (TRANSPOSE ? NQ * NS : NQ); idx += 64) {
      const int q = TRANSPOSE ? idx / NS : idx, m = TRANSPOSE ? idx - q * NS : 0;
      MHA_POINT_GEO();
      Dual U[NS], Ud[NS], F[NS];
      MHA_SEED_POINT(TRANSPOSE ? ((m == sp + sl) ? 1.0 : 0.0) : s_Xh[q * NS + sp + sl]);
      MHA_POINT_ARGS(pa);
      MHA_MODULE_POINT(pa, F);
      double z = 0.0;
      MHA_BACK_TRANSFORM(F, if (TRANSPOSE) z += w * ref[sl] * s_Xh[q * NS + sp + sl];
                            else s_out[q * NS + sp + sl] = w * ref[sl]);
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
  require_layout<PHYS, DIM>(vl);
  const WaveLaunch g = wave_launch(vl.tables_size * sizeof(double), apply_wave_doubles(vl, geo_size<DIM>()) * sizeof(double),
                                   b.e_count);
  if (lds_bytes) *lds_bytes = g.lds;
  if (waves) *waves = g.nw;
  auto go = [&](auto kern) {
    prepare_kernel(kern, "Jacobian product");
    if (overwrite) MHA_HIP(hipMemsetAsync(y, 0, sizeof(double) * b.nrows, stream));
    hipLaunchKernelGGL(kern, dim3(g.grid), dim3(64 * g.nw), g.lds, stream, b, vl, pp, tm, x, y);
    MHA_HIP(hipGetLastError());
  };
  dispatch_expr<PHYS>(pp, [&](auto expr) {
    constexpr int E = decltype(expr)::value;
    if (transpose) go(jacobian_apply_kernel<DIM, PHYS, E, 1>);
    else go(jacobian_apply_kernel<DIM, PHYS, E, 0>);
  });
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
  dispatch_module(b.dim, pp.physics, "Jacobian-product", [&](auto dim, auto phys) {
    launch_typed<decltype(dim)::value, decltype(phys)::value>(b, vl, pp, tm, x, y, transpose, overwrite, stream, lds_bytes,
                                                              waves);
  });
}

}  // namespace mha
