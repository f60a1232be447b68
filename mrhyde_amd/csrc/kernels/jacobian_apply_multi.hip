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
// Kc is a kernel argument, not a template parameter: the instantiations are the single product's 92.  The launcher
// takes nvec vectors in passes of Kc <= MHA_APPLY_MAX_VECTORS and chooses Kc per shape (choose_vectors); a pass of one
// vector runs jacobian_apply.hip's kernel.
//
// Layout as in jacobian_apply.hip: one wavefront per element, wave-level synchronisation only, waves persistent over
// blocked element ranges.  The statements the element loop has in common with the other point-function kernels are
// engine_points.hpp's macros, the launcher's checks and choices engine_dispatch.hpp's; the handling of
// x_k is this file's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device_math.hpp"
#include "engine_dispatch.hpp"
#include "engine_points.hpp"
#include "launch.hpp"

namespace mha {
namespace {

// per-element LDS (doubles): u, udot, sign, x_k | geometry | U^, Udot^, X^_k, F^x_k or z^_k | row (ints)
__host__ __device__ inline size_t multi_wave_doubles(const VarLayoutDev &vl, int geo, int kc) {
  const size_t n = vl.n_tot, NS = vl.ns_tot, NQ = vl.nq;
  return (3 + kc) * n + NQ * geo + (2 + 2 * kc) * NQ * NS + (n + 1) / 2;
}

template <int DIM, int PHYS, int EXPR, int TRANSPOSE>
__global__ __launch_bounds__(64 * kProductMaxWaves) void jacobian_apply_multi_kernel(
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

  MHA_WAVE_ELEMENT_RANGE(NW, wave);
  MHA_VAR_AT();
  for (int el = el_begin; el < el_end; ++el) {
    const int e = b.e_begin + el;
    wave_lds_sync();  // previous element done with the wave's LDS
    // ---- 1. gather u + seeding values once, x_k (x orientation sign) per vector, geometry ----
    for (int f = lane; f < n; f += 64) {
      MHA_DOF_ROW(f);
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
      MHA_REF_SLOT(idx);
      if (t == 0) {
        MHA_REF_FIELDS(idx);
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
    MHA_ELEMENT_SIZE();
    for (int idx = lane; idx < (TRANSPOSE ? QS : NQ * Kc); idx += 64) {
      const int kv = TRANSPOSE ? 0 : idx / NQ;  // forward: the item's vector
      const int q = TRANSPOSE ? idx / NS : idx - kv * NQ, m = TRANSPOSE ? idx - q * NS : 0;
      MHA_POINT_GEO();
      const double *Xk = s_Xh + kv * QS + q * NS;
      Dual U[NS], Ud[NS], F[NS];
      MHA_SEED_POINT(TRANSPOSE ? ((m == sp + sl) ? 1.0 : 0.0) : Xk[sp + sl]);
      MHA_POINT_ARGS(pa);
      MHA_MODULE_POINT(pa, F);
      double col[NS];  // w G^T F.d: forward F^x_k(q), transposed column m of C^(q)
      MHA_BACK_TRANSFORM(F, col[sp + sl] = w * ref[sl]);
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
  return waves_that_fit(tables, multi_wave_doubles(vl, geo, kc) * sizeof(double));
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
  require_layout<PHYS, DIM>(vl);
  const size_t tables = vl.tables_size * sizeof(double);
  require_wave_fits(tables, multi_wave_doubles(vl, geo_size<DIM>(), 1) * sizeof(double));
  const int kc_max = choose_vectors(vl, geo_size<DIM>(), tables, nvec);
  auto go = [&](auto kern) {
    prepare_kernel(kern, "Jacobian product");
    // passes of kc_max vectors and a remainder; each pass sized for its own Kc and zeroing its own vectors first
    for (int k0 = 0; k0 < nvec; k0 += kc_max) {
      const int kc = std::min(kc_max, nvec - k0);
      const WaveLaunch g = wave_launch(tables, multi_wave_doubles(vl, geo_size<DIM>(), kc) * sizeof(double), b.e_count);
      if (k0 == 0) {  // reported: the first (full) pass
        if (lds_bytes) *lds_bytes = g.lds;
        if (waves) *waves = g.nw;
        if (vectors) *vectors = kc;
      }
      if (kc == 1) {  // the single product's launch: same checks, same dispatch, same memset
        launch_jacobian_apply(b, vl, pp, tm, x + k0 * ldx, y + k0 * ldy, transpose, overwrite, stream);
        continue;
      }
      if (overwrite)  // the vectors, not the padding between them
        MHA_HIP(hipMemset2DAsync(y + k0 * ldy, sizeof(double) * ldy, 0, sizeof(double) * b.nrows, kc, stream));
      hipLaunchKernelGGL(kern, dim3(g.grid), dim3(64 * g.nw), g.lds, stream, b, vl, pp, tm, kc, x + k0 * ldx, ldx,
                         y + k0 * ldy, ldy);
      MHA_HIP(hipGetLastError());
    }
  };
  dispatch_expr<PHYS>(pp, [&](auto expr) {
    constexpr int E = decltype(expr)::value;
    if (transpose) go(jacobian_apply_multi_kernel<DIM, PHYS, E, 1>);
    else go(jacobian_apply_multi_kernel<DIM, PHYS, E, 0>);
  });
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
  dispatch_module(b.dim, pp.physics, "Jacobian-product", [&](auto dim, auto phys) {
    launch_typed<decltype(dim)::value, decltype(phys)::value>(b, vl, pp, tm, nvec, x, ldx, y, ldy, transpose, overwrite,
                                                              stream, lds_bytes, waves, vectors);
  });
}

}  // namespace mha
