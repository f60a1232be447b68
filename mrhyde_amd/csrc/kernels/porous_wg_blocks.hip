// porous_wg_blocks.hip -- the element step of porousWeakGalerkin, uncondensed and plain: residual and derivative block
// of the 1 + 4 dim interior unknowns (pint, u, t) and the 2 dim traces pbndry of every element.
//
// reference: porousWeakGalerkin::volumeResidual (src/physics/porousWeakGalerkin.cpp:94-323) and faceResidual (:424-505)
// on all 2 dim faces (`assemble face terms: true`):
//   row pint:     (div t - source, q)
//   rows u:       (u, v) + (pint, div v) - sum_faces <pbndry, v . n>
//   rows t:       (perm u + t, s)
//   rows pbndry:  - sum_faces <t . n, mu>,   mu_k = 1 on face k (HFACE of degree 0)
// res = -res.val(), blocks = d res / d unknown, rows and columns pint, u, t (dof order), pbndry (HFACE face order).  The
// form is linear, so a row's derivative entries are its coefficients and its residual is their product with the state.
// One thread per (element, row), every coefficient integrated where it is needed: written to be read, and to be the
// implementation the fused kernel (porous_wg_fused.hip) is compared with through condense.hip.  Every flux function is
// integrated against every face, as the reference's dense loops do.  A sub-block no formula above writes keeps the +0.0
// it was initialised with.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_math.hpp"
#include "launch.hpp"
#include "porous_hybrid.hpp"
#include "side_geometry.hpp"

namespace mha {
namespace {

// the raw flux function f at reference point xi: value along e_c, and its reference divergence
__device__ __forceinline__ double pwg_phi(int f, const double *xi) { return (f & 1) ? 0.5 * (1.0 + xi[f >> 1]) : 0.5 * (1.0 - xi[f >> 1]); }
__device__ __forceinline__ double pwg_div(int f) { return (f & 1) ? 0.5 : -0.5; }

template <int DIM, bool EXPR>
__global__ __launch_bounds__(256) void porous_wg_blocks_kernel(BlockDev b, SideTablesDev st, PwgElementDev a, TimeDev tm) {
  constexpr int NN = 1 << DIM, NU = 2 * DIM, NI = 1 + 2 * NU, N = NI + NU, U0 = 1, T0 = 1 + NU;
  const int64_t total = (int64_t)b.e_count * N;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int el = (int)(idx / N), r = (int)(idx - (int64_t)el * N), e = b.e_begin + el, nq = b.nq, nqs = st.nqs;
    const double *xn = b.nodes + (size_t)e * NN * DIM;
    const int32_t *L = b.lids + (size_t)e * NI;
    double su[NU], sv[NU], coef[N];  // signs of u and of t
#pragma unroll
    for (int f = 0; f < NU; ++f) {
      su[f] = a.orient ? (double)a.orient[(size_t)e * NI + U0 + f] : 1.0;
      sv[f] = a.orient ? (double)a.orient[(size_t)e * NI + T0 + f] : 1.0;
    }
#pragma unroll
    for (int c = 0; c < N; ++c) coef[c] = 0.0;
    double data = 0.0;  // the part of res.val() that does not depend on the state: -(source, q)
    if (r < NI) {
      // volume rows
      for (int q = 0; q < nq; ++q) {
        double J[DIM * DIM], Ji[DIM * DIM], det, x[DIM], xi[DIM];
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          x[i] = 0.0;
          xi[i] = 0.0;
#pragma unroll
          for (int c = 0; c < DIM; ++c) J[i * DIM + c] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < NN; ++k) {
          const double nv = b.nodeval[k * nq + q];
#pragma unroll
          for (int i = 0; i < DIM; ++i) {
            x[i] += xn[k * DIM + i] * nv;
            xi[i] += pmh_vertex_coord(k, i) * nv;
#pragma unroll
            for (int c = 0; c < DIM; ++c) J[i * DIM + c] += xn[k * DIM + i] * b.nodegrad[(k * nq + q) * DIM + c];
          }
        }
        invert<DIM>(J, Ji, det);
        const double w = b.ref_wts[q] * det;
        if (r == 0) {
          // (div t - source, q), q = 1
#pragma unroll
          for (int g = 0; g < NU; ++g) coef[T0 + g] += sv[g] * pwg_div(g) / det * w;
          data -= eval_func<DIM, EXPR>(a.f[0], e, q, nq, x) * w;
        } else {
          const bool urow = r < T0;
          const int f = urow ? r - U0 : r - T0, cf = f >> 1;
          const double vf = (urow ? su[f] : sv[f]) * pwg_phi(f, xi) / det;  // test function J[:, cf] vf
          if (urow) coef[0] += su[f] * pwg_div(f) / det * w;                // (pint, div v_f)
          const double perm = urow ? 1.0 : a.edata ? a.edata[(size_t)e * a.ecols] : eval_func<DIM, EXPR>(a.f[1], e, q, nq, x);
#pragma unroll
          for (int g = 0; g < NU; ++g) {
            const int cg = g >> 1;
            double jj = 0.0;
#pragma unroll
            for (int d = 0; d < DIM; ++d) jj += J[d * DIM + cg] * J[d * DIM + cf];
            const double pg = pwg_phi(g, xi) / det;
            if (urow) {
              coef[U0 + g] += jj * (su[g] * pg) * vf * w;  // (u_g, v_f)
            } else {
              coef[U0 + g] += perm * jj * (su[g] * pg) * vf * w;  // (perm u_g, s_f)
              coef[T0 + g] += jj * (sv[g] * pg) * vf * w;         // (t_g, s_f)
            }
          }
        }
      }
    }
    if ((r >= U0 && r < T0) || r >= NI) {
      // face terms: -<pbndry_k, v_f . n> on row u_f; -<t_g . n, mu_k> on row pbndry_k
#pragma unroll
      for (int k = 0; k < NU; ++k) {
        if (r >= NI && k != r - NI) continue;
        const int s = pmh_side_of_face(k);
        for (int q = 0; q < nqs; ++q) {
          double J[DIM * DIM], Ji[DIM * DIM], nrm[DIM], w, x[DIM], det;
          side_point<DIM>(xn, st, s, q, Ji, nrm, w, x);
          side_point_J<DIM>(xn, st, s, q, J, x);
          invert<DIM>(J, Ji, det);
          const double *xi = st.ip + (s * nqs + q) * DIM;
#pragma unroll
          for (int g = 0; g < NU; ++g) {
            if (r < NI && g != r - U0) continue;
            double vn = 0.0;
#pragma unroll
            for (int d = 0; d < DIM; ++d) vn += J[d * DIM + (g >> 1)] * nrm[d];
            vn *= pwg_phi(g, xi) / det;
            if (r < NI) coef[NI + k] -= su[g] * vn * w;
            else coef[T0 + g] -= sv[g] * vn * w;
          }
        }
      }
    }
    // the state: pint, u, t (the block's vector), pbndry
    double val = data;
#pragma unroll
    for (int c = 0; c < N; ++c) {
      const double s = c < NI ? stage_value(tm, L[b.offsets[c]]) : a.lambda[(size_t)e * NU + (c - NI)];
      val += coef[c] * s;
    }
    if (a.res) a.res[idx] = -val;
    if (a.blocks) {
      double *out = a.blocks + idx * N;
#pragma unroll
      for (int c = 0; c < N; ++c) out[c] = coef[c];
    }
  }
}

template <int DIM>
void launch_dim(const BlockDev &b, const SideTablesDev &st, const PwgElementDev &a, const TimeDev &tm, hipStream_t stream) {
  bool expr = false;
  for (const FuncDesc &f : a.f) expr = expr || has_expression(f);
  const int64_t total = (int64_t)b.e_count * (1 + 6 * DIM);
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 1 << 20);
  auto go = [&](auto kern) {
    require_modest_scratch(kern, "porousWeakGalerkin blocks kernel");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, b, st, a, tm);
    MHA_HIP(hipGetLastError());
  };
  if (expr) go(porous_wg_blocks_kernel<DIM, true>);
  else go(porous_wg_blocks_kernel<DIM, false>);
}

}  // namespace

void launch_porous_wg_blocks(const BlockDev &b, const SideTablesDev &st, const PwgElementDev &a, const TimeDev &tm,
                             hipStream_t stream) {
  if (b.e_count <= 0) return;
  MHA_REQUIRE((b.dim == 2 || b.dim == 3) && b.n == 1 + 4 * b.dim, MHA_ERR_INVALID,
              "porousWeakGalerkin blocks kernel: pint (HVOL 0), u and t (HDIV 1) on quads or hexes");
  if (b.dim == 2) launch_dim<2>(b, st, a, tm, stream);
  else launch_dim<3>(b, st, a, tm, stream);
}

}  // namespace mha
