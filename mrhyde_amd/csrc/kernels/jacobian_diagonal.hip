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
// The statements the element loop has in common with the other point-function kernels are engine_points.hpp's macros,
// the launcher's checks and choices engine_dispatch.hpp's.  Its own: var_at with the offset `co` of the
// variable's block of C^ (beside the shared one the offset cost other SGPR spill counts), and the back-transform, which
// runs for the variable of m alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device_math.hpp"
#include "engine_dispatch.hpp"
#include "engine_points.hpp"
#include "launch.hpp"

namespace mha {
namespace {

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
__global__ __launch_bounds__(64 * kProductMaxWaves) void jacobian_diagonal_kernel(BlockDev b, VarLayoutDev vl, PhysParamsDev pp,
                                                                               TimeDev tm, double *__restrict__ d) {
  using L = Layout<PHYS, DIM>;
  constexpr int NS = L::NS, GEO = geo_size<DIM>(), CS = coupling_size<L, DIM>();
  extern __shared__ double smem[];
  // wave: the same in every lane, and said so to the compiler -- the element loop is then a scalar loop.  As a per-lane
  // value it made the element loop one with a divergent exit, and under the register pressure of the 3-D deck-string
  // builds the copies and spills of values live across the dof-gather loop were placed in front of the exec restore
  // behind that loop, where no lane is active (check_exec_restore.awk)
  const int NQ = vl.nq, n = vl.n_tot, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63,
            NW = blockDim.x >> 6;
  double *tab = smem;
  double *s_Uh = tab + vl.tables_size + wave * (int)diag_wave_doubles(vl, GEO, CS);
  double *s_Udh = s_Uh + NQ * NS, *s_C = s_Udh + NQ * NS;
  double *s_geo = s_C + NQ * CS;
  double *s_u = s_geo + NQ * GEO, *s_ud = s_u + n;
  int *s_row = reinterpret_cast<int *>(s_ud + n);

  for (int k = tid; k < vl.tables_size; k += blockDim.x) tab[k] = vl.tables[k];
  __syncthreads();  // the only workgroup barrier: from here on a wave meets nobody

  MHA_WAVE_ELEMENT_RANGE(NW, wave);
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
      MHA_DOF_ROW(f);
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
      MHA_REF_SLOT(idx);
      MHA_REF_FIELDS(idx);
    }
    wave_lds_sync();
    // ---- 3. point function, one thread per (point, unit direction m): column m of C^(q), rows of m's variable ----
    MHA_ELEMENT_SIZE();
    for (int idx = lane; idx < NQ * NS; idx += 64) {
      const int q = idx / NS, m = idx - q * NS;
      MHA_POINT_GEO();
      Dual U[NS], Ud[NS], F[NS];
      MHA_SEED_POINT((m == sp + sl) ? 1.0 : 0.0);
      MHA_POINT_ARGS(pa);
      MHA_MODULE_POINT(pa, F);
      // the back-transform is not MHA_BACK_TRANSFORM: it runs for the variable of m alone
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
  require_layout<PHYS, DIM>(vl);
  const WaveLaunch g = wave_launch(vl.tables_size * sizeof(double),
                                   diag_wave_doubles(vl, geo_size<DIM>(), coupling_size<L, DIM>()) * sizeof(double), b.e_count);
  if (lds_bytes) *lds_bytes = g.lds;
  if (waves) *waves = g.nw;
  dispatch_expr<PHYS>(pp, [&](auto expr) {
    auto kern = jacobian_diagonal_kernel<DIM, PHYS, decltype(expr)::value>;
    prepare_kernel(kern, "Jacobian diagonal");
    if (overwrite) MHA_HIP(hipMemsetAsync(d, 0, sizeof(double) * b.nrows, stream));
    hipLaunchKernelGGL(kern, dim3(g.grid), dim3(64 * g.nw), g.lds, stream, b, vl, pp, tm, d);
    MHA_HIP(hipGetLastError());
  });
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
  dispatch_module(b.dim, pp.physics, "Jacobian-diagonal", [&](auto dim, auto phys) {
    launch_typed<decltype(dim)::value, decltype(phys)::value>(b, vl, pp, tm, d, overwrite, stream, lds_bytes, waves);
  });
}

}  // namespace mha
