// porous_wg_fused.hip -- the whole element step of porousWeakGalerkin in ONE kernel: geometry, local matrices, interior
// solve and Schur complement; nothing but S[2 dim][2 dim], g[2 dim] and du[1 + 4 dim] leaves the chip.
//
// reference: porousWeakGalerkin::volumeResidual + faceResidual (src/physics/porousWeakGalerkin.cpp:94-323, 424-505); the
// reference leaves the elimination of pint, u and t to its global direct solver.  Unfused equivalent, kept as the
// independent implementation the tests compare with: porous_wg_blocks.hip, then condense.hip (a [6 dim + 1]^2 block per
// element through memory, one wavefront per element, pivoted Gauss-Jordan).
//
// One THREAD per element.  With the lowest-order bases the element's block is
//          pint   u     t    lambda
//   pint [  0     0     B^T    0   ]     M_fg = (v_f, v_g)   symmetric positive definite, 2 dim x 2 dim
//   u    [  B     M     0    -C^T  ]     K_fg = (perm v_f, v_g)
//   t    [  0     K     M      0   ]     B_f  = (1, div v_f)
//   lam  [  0     0    -C      0   ]     C_k  = <v_f(k) . n, 1>_F_k   one entry per face
// non-symmetric, but it needs no pivot search: M = L L^T (Cholesky), Mi = M^-1, W = Mi K Mi (symmetric; positive
// definite for perm > 0), Z = W B, sigma = B . Z > 0, and with r = -res.val()
//   dp = (r_p - B . Mi r_t + Z . r_u) / sigma,   du = Mi (r_u - B dp),   dt = Mi (r_t - K du),
//   S_ab = C_a C_b (W_ab - Z_a Z_b / sigma),     g_a = r_l,a + C_a dt_a      (faces and flux dofs paired).
// The orientation signs never enter the matrices: the state is taken to the raw basis on the way in (u_f sg_f), du goes
// back on the way out, S and g do not see them (multiplications by +-1 are exact).
// Registers: the lower triangles of M and K while the points are summed; the residuals are formed before the
// factorisation, so the state dies there; L overwrites M, L^-1 is built beside it and both die into Mi; W is built column
// by column from Mi and K (one column of K Mi at a time).  At most three triangles of 2 dim (2 dim + 1) / 2 values live
// at once (63 doubles in 3-D) beside a handful of vectors.  The Jacobian is evaluated at every volume point and every
// side point (general quads and hexes); the tables are read at wave-uniform addresses.  A non-positive pivot or sigma
// (degenerate element, perm <= 0) is replaced by 1, the element counted and its outputs made finite.
//
// Stores: stream_rows.hpp.  HBM traffic per element: 2^dim dim + 1 + 6 dim doubles in (+ LIDs, signs),
// 4 dim^2 + 6 dim + 1 out.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "device_math.hpp"
#include "launch.hpp"
#include "porous_hybrid.hpp"
#include "side_geometry.hpp"
#include "stream_rows.hpp"

namespace mha {
namespace {

constexpr int kPwgWaves = 4;  // wavefronts (of 64 elements) per workgroup

template <int DIM, bool EXPR>
__global__ __launch_bounds__(64 * kPwgWaves) void porous_wg_fused_kernel(BlockDev b, SideTablesDev st, PwgElementDev a, TimeDev tm) {
  constexpr int NN = 1 << DIM, NU = 2 * DIM, NI = 1 + 2 * NU, NSYM = NU * (NU + 1) / 2, U0 = 1, T0 = 1 + NU;
  constexpr int SBW = (NU * NU) | 1;  // staging row stride of the widest output
  static_assert(((NU * NU) | 1) >= (NI | 1), "the staging buffer holds a row of du");
  __shared__ double s_out[kPwgWaves][64 * SBW];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t e0 = ((int64_t)blockIdx.x * kPwgWaves + wv) * 64;  // first element of the wavefront
  if (e0 >= b.e_count) return;
  const int cnt = (int)(b.e_count - e0 < 64 ? b.e_count - e0 : 64);
  const bool active = lane < cnt;
  const int64_t el = e0 + (active ? lane : 0);  // idle lanes of the last wavefront shadow its first element
  const int e = b.e_begin + (int)el, nq = b.nq, nqs = st.nqs;
  auto sym = [](int f, int g) { return f >= g ? f * (f + 1) / 2 + g : g * (g + 1) / 2 + f; };

  double xn[NN * DIM];
#pragma unroll
  for (int k = 0; k < NN * DIM; ++k) xn[k] = b.nodes[(size_t)e * NN * DIM + k];

  // ---- volume points: M, K (lower triangles), B, the source integral ----
  double M[NSYM], K[NSYM], B[NU], srcint = 0.0;
#pragma unroll
  for (int k = 0; k < NSYM; ++k) {
    M[k] = 0.0;
    K[k] = 0.0;
  }
#pragma unroll
  for (int f = 0; f < NU; ++f) B[f] = 0.0;
  const double pdata = a.edata ? a.edata[(size_t)e * a.ecols] : 0.0;
  for (int q = 0; q < nq; ++q) {
    double J[DIM * DIM], x[DIM], xi[DIM];
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
    double det;
    if constexpr (DIM == 2) det = J[0] * J[3] - J[1] * J[2];
    else det = J[0] * (J[4] * J[8] - J[5] * J[7]) + J[1] * (J[5] * J[6] - J[3] * J[8]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
    const double rdet = 1.0 / det, w = b.ref_wts[q] * det;
    srcint += eval_func<DIM, EXPR>(a.f[0], e, q, nq, x) * w;
    const double perm = a.edata ? pdata : eval_func<DIM, EXPR>(a.f[1], e, q, nq, x);
    // G_cc' = sum_d J_dc J_dc'
    double G[DIM * DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c)
#pragma unroll
      for (int c2 = 0; c2 <= c; ++c2) {
        double v = 0.0;
#pragma unroll
        for (int d = 0; d < DIM; ++d) v += J[d * DIM + c] * J[d * DIM + c2];
        G[c * DIM + c2] = v;
      }
    double t[NU];  // phi_f / det
#pragma unroll
    for (int f = 0; f < NU; ++f) {
      t[f] = ((f & 1) ? 0.5 * (1.0 + xi[f >> 1]) : 0.5 * (1.0 - xi[f >> 1])) * rdet;
      B[f] += ((f & 1) ? 0.5 : -0.5) * rdet * w;
    }
#pragma unroll
    for (int f = 0; f < NU; ++f)
#pragma unroll
      for (int g = 0; g <= f; ++g) {
        const double m = G[(f >> 1) * DIM + (g >> 1)] * t[f] * t[g] * w;
        M[f * (f + 1) / 2 + g] += m;
        K[f * (f + 1) / 2 + g] += perm * m;
      }
  }

  // ---- side points: C_k = <v_f(k) . n, 1> on face k ----
  double C[NU];
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    const int s = pmh_side_of_face(k), f = pmh_dof_of_face(k), c = f >> 1;
    double acc = 0.0;
    for (int q = 0; q < nqs; ++q) {
      // (v . n) w = (J e_c . m) phi / det w_ref with m the normal of side_geometry.hpp before it is scaled to unit length
      // (w = |m| w_ref there): no square root, no inverse of J
      double J[DIM * DIM], x[DIM], m[DIM], det;
      side_point_J<DIM>(xn, st, s, q, J, x);
      if constexpr (DIM == 2) {
        det = J[0] * J[3] - J[1] * J[2];
        m[0] = J[2] * st.tanU[s * 2] + J[3] * st.tanU[s * 2 + 1];
        m[1] = -(J[0] * st.tanU[s * 2] + J[1] * st.tanU[s * 2 + 1]);
      } else {
        det = J[0] * (J[4] * J[8] - J[5] * J[7]) + J[1] * (J[5] * J[6] - J[3] * J[8]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
        double tu[3], tv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          tu[r] = J[r * 3] * st.tanU[s * 3] + J[r * 3 + 1] * st.tanU[s * 3 + 1] + J[r * 3 + 2] * st.tanU[s * 3 + 2];
          tv[r] = J[r * 3] * st.tanV[s * 3] + J[r * 3 + 1] * st.tanV[s * 3 + 1] + J[r * 3 + 2] * st.tanV[s * 3 + 2];
        }
        m[0] = tu[1] * tv[2] - tu[2] * tv[1];
        m[1] = tu[2] * tv[0] - tu[0] * tv[2];
        m[2] = tu[0] * tv[1] - tu[1] * tv[0];
      }
      const double xc = st.ip[(s * nqs + q) * DIM + c];
      double vn = 0.0;
#pragma unroll
      for (int d = 0; d < DIM; ++d) vn += J[d * DIM + c] * m[d];
      acc += vn * ((f & 1) ? 0.5 * (1.0 + xc) : 0.5 * (1.0 - xc)) / det * st.wts[q];
    }
    C[k] = acc;
  }

  // ---- the state in the raw basis and r = -res.val(); the state dies here ----
  const int32_t *L = b.lids + (size_t)e * NI;
  double su[NU], sv[NU];  // signs of u and of t
#pragma unroll
  for (int f = 0; f < NU; ++f) {
    su[f] = a.orient ? (double)a.orient[(size_t)e * NI + U0 + f] : 1.0;
    sv[f] = a.orient ? (double)a.orient[(size_t)e * NI + T0 + f] : 1.0;
  }
  double rp, ru[NU], rt[NU], rl[NU];
  {
    const double p = stage_value(tm, L[b.offsets[0]]);
    double uf[NU], tf[NU];
#pragma unroll
    for (int f = 0; f < NU; ++f) {
      uf[f] = su[f] * stage_value(tm, L[b.offsets[U0 + f]]);
      tf[f] = sv[f] * stage_value(tm, L[b.offsets[T0 + f]]);
    }
    rp = srcint;
#pragma unroll
    for (int f = 0; f < NU; ++f) rp -= B[f] * tf[f];
#pragma unroll
    for (int f = 0; f < NU; ++f) {
      double vu = p * B[f], vt = 0.0;
#pragma unroll
      for (int g = 0; g < NU; ++g) {
        vu += M[sym(f, g)] * uf[g];
        vt += K[sym(f, g)] * uf[g] + M[sym(f, g)] * tf[g];
      }
      ru[f] = -vu;
      rt[f] = -vt;
    }
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      const int f = pmh_dof_of_face(k);
      ru[f] += C[k] * a.lambda[(size_t)e * NU + k];
      rl[k] = C[k] * tf[f];
    }
  }

  // ---- Cholesky M = L L^T in place, L^-1, then Mi = L^-T L^-1 ----
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    double dj = M[sym(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) dj -= M[sym(j, k)] * M[sym(j, k)];
    if (!(dj > 0.0)) { bad = true; dj = 1.0; }
    const double ljj = sqrt(dj), rinv = 1.0 / ljj;
    M[sym(j, j)] = ljj;
#pragma unroll
    for (int i = j + 1; i < NU; ++i) {
      double v = M[sym(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= M[sym(i, k)] * M[sym(j, k)];
      M[sym(i, j)] = v * rinv;
    }
  }
  double Li[NSYM];  // L^-1, lower triangle
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    Li[sym(j, j)] = 1.0 / M[sym(j, j)];
#pragma unroll
    for (int i = j + 1; i < NU; ++i) {
      double v = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) v -= M[sym(i, k)] * Li[sym(k, j)];
      Li[sym(i, j)] = v / M[sym(i, i)];
    }
  }
  double Mi[NSYM];
#pragma unroll
  for (int i = 0; i < NU; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double v = 0.0;
#pragma unroll
      for (int k = i; k < NU; ++k) v += Li[sym(k, i)] * Li[sym(k, j)];
      Mi[sym(i, j)] = v;
    }

  // ---- W = Mi K Mi, column by column: column j of K Mi, then the entries of W at and below the diagonal ----
  double W[NSYM];
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    double col[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < NU; ++k) v += K[sym(i, k)] * Mi[sym(k, j)];
      col[i] = v;
    }
#pragma unroll
    for (int i = j; i < NU; ++i) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < NU; ++k) v += Mi[sym(i, k)] * col[k];
      W[sym(i, j)] = v;
    }
  }

  // ---- the scalar Schur complement of pint, the interior step ----
  double Z[NU], sigma = 0.0;
#pragma unroll
  for (int f = 0; f < NU; ++f) {
    double v = 0.0;
#pragma unroll
    for (int g = 0; g < NU; ++g) v += W[sym(f, g)] * B[g];
    Z[f] = v;
    sigma += B[f] * v;
  }
  if (!(sigma > 0.0)) { bad = true; sigma = 1.0; }
  const double rsig = 1.0 / sigma;
  double xt[NU];  // Mi r_t
  double acc = rp;
#pragma unroll
  for (int f = 0; f < NU; ++f) {
    double v = 0.0;
#pragma unroll
    for (int g = 0; g < NU; ++g) v += Mi[sym(f, g)] * rt[g];
    xt[f] = v;
    acc += Z[f] * ru[f] - B[f] * v;
  }
  const double dp = acc * rsig;
  double du[NU], dt[NU];
#pragma unroll
  for (int f = 0; f < NU; ++f) {
    double v = 0.0;
#pragma unroll
    for (int g = 0; g < NU; ++g) v += Mi[sym(f, g)] * (ru[g] - B[g] * dp);
    du[f] = v;
  }
  {
    double kd[NU];
#pragma unroll
    for (int f = 0; f < NU; ++f) {
      double v = 0.0;
#pragma unroll
      for (int g = 0; g < NU; ++g) v += K[sym(f, g)] * du[g];
      kd[f] = v;
    }
#pragma unroll
    for (int f = 0; f < NU; ++f) {
      double v = xt[f];
#pragma unroll
      for (int g = 0; g < NU; ++g) v -= Mi[sym(f, g)] * kd[g];
      dt[f] = v;
    }
  }
  if (bad && active && a.singular) atomicAdd(a.singular, 1);
  auto finite = [&](double v) { return bad && !(fabs(v) <= DBL_MAX) ? 0.0 : v; };

  // ---- outputs through the wavefront's staging buffer ----
  double *sb = s_out[wv];
  if (a.schur) {
    constexpr int WP = (NU * NU) | 1;
#pragma unroll
    for (int ka = 0; ka < NU; ++ka)
#pragma unroll
      for (int kb = 0; kb < NU; ++kb) {
        const int fa = pmh_dof_of_face(ka), fb = pmh_dof_of_face(kb);
        sb[lane * WP + ka * NU + kb] = finite(C[ka] * C[kb] * (W[sym(fa, fb)] - Z[fa] * Z[fb] * rsig));
      }
    pmh_wave_sync();
    pmh_stream_rows<NU * NU>(a.schur + e0 * NU * NU, sb, lane, cnt);
    pmh_wave_sync();
  }
  if (a.gvec) {
    constexpr int WP = NU | 1;
#pragma unroll
    for (int k = 0; k < NU; ++k) sb[lane * WP + k] = finite(rl[k] + C[k] * dt[pmh_dof_of_face(k)]);
    pmh_wave_sync();
    pmh_stream_rows<NU>(a.gvec + e0 * NU, sb, lane, cnt);
    pmh_wave_sync();
  }
  if (a.du) {
    constexpr int WP = NI | 1;
    sb[lane * WP] = finite(dp);
#pragma unroll
    for (int f = 0; f < NU; ++f) {
      sb[lane * WP + U0 + f] = finite(su[f] * du[f]);
      sb[lane * WP + T0 + f] = finite(sv[f] * dt[f]);
    }
    pmh_wave_sync();
    pmh_stream_rows<NI>(a.du + e0 * NI, sb, lane, cnt);
  }
}

template <int DIM>
void launch_dim(const BlockDev &b, const SideTablesDev &st, const PwgElementDev &a, const TimeDev &tm, hipStream_t stream) {
  bool expr = false;
  for (const FuncDesc &f : a.f) expr = expr || has_expression(f);
  const int per_wg = 64 * kPwgWaves, grid = (b.e_count + per_wg - 1) / per_wg;
  auto go = [&](auto kern) {
    require_modest_scratch(kern, "porousWeakGalerkin fused kernel");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(per_wg), 0, stream, b, st, a, tm);
    MHA_HIP(hipGetLastError());
  };
  if (expr) go(porous_wg_fused_kernel<DIM, true>);
  else go(porous_wg_fused_kernel<DIM, false>);
}

}  // namespace

void launch_porous_wg_fused(const BlockDev &b, const SideTablesDev &st, const PwgElementDev &a, const TimeDev &tm,
                            hipStream_t stream) {
  if (b.e_count <= 0) return;
  MHA_REQUIRE((b.dim == 2 || b.dim == 3) && b.n == 1 + 4 * b.dim, MHA_ERR_INVALID,
              "porousWeakGalerkin fused kernel: pint (HVOL 0), u and t (HDIV 1) on quads or hexes");
  MHA_REQUIRE(b.e_begin == 0, MHA_ERR_INVALID, "porousWeakGalerkin fused kernel: the outputs are those of the whole block");
  for (const double *p : {a.schur, a.gvec, a.du})
    MHA_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0, MHA_ERR_INVALID,
                "porousWeakGalerkin fused kernel: schur, gvec and du must be 16-byte aligned (they are stored in 16-byte pieces)");
  if (b.dim == 2) launch_dim<2>(b, st, a, tm, stream);
  else launch_dim<3>(b, st, a, tm, stream);
}

}  // namespace mha
