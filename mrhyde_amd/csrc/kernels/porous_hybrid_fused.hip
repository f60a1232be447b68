// porous_hybrid_fused.hip -- the whole element step of porousMixedHybridized in ONE kernel: geometry, local matrices,
// interior solve and Schur complement; nothing but S[2 dim][2 dim], g[2 dim] and du[1 + 2 dim] leaves the chip.
//
// reference: porousMixedHybrid::volumeResidual + faceResidual (src/physics/porousMixedHybridized.cpp:72-189, 287-362);
// the reference leaves the elimination of p and u to its global direct solver.  Unfused equivalent, kept as the
// independent implementation the tests compare with: porous_hybrid_blocks.hip, then condense.hip (a [4 dim + 1]^2 block
// per element through memory, one wavefront per element, pivoted Gauss-Jordan).
//
// One THREAD per element.  With the lowest-order bases the element's block is
//        p      u      lambda
//   p [  0    -B^T     0   ]      A_fg = (Kinv v_f, v_g)      symmetric positive definite, 2 dim x 2 dim
//   u [ -B     A      C^T  ]      B_f  = (1, div v_f)
//   l [  0    -C       0   ]      C_k  = <v_f(k) . n, 1>_F_k  one entry per face: v_f . n vanishes on every face but its own
// so the interior solve needs no pivot search: A = L L^T (Cholesky), Y = A^-1 B, sigma = B . Y > 0 the scalar Schur
// complement of p, and with Ai = A^-1
//   S_ab = C_a C_b (Ai_ab - Y_a Y_b / sigma),   dp = -(r_p + Y . r_u) / sigma,   du = Ai r_u + Y dp,   g_a = r_l,a + C_a du_a
// (faces and flux dofs paired).  Everything lives in registers: 2 dim (2 dim + 1) / 2 + 5 (2 dim) + 3 values, no scratch.
// The Jacobian is evaluated at every volume point and every side point (general quads and hexes); the tables are read at
// wave-uniform addresses.  A non-positive pivot (degenerate element, Kinv <= 0) is replaced by 1, the element counted and
// its outputs made finite.
//
// Stores: a wavefront's 64 elements own one contiguous piece of each output; the lanes put their rows into the
// wavefront's LDS buffer (row stride odd: conflict-free 8-byte writes) and the wavefront streams the piece out 16 bytes
// per lane, consecutive lanes at consecutive addresses.  HBM traffic per element: 2^dim dim + 1 + 4 dim doubles in (+
// LIDs, signs), 4 dim^2 + 4 dim + 1 out.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "device_math.hpp"
#include "launch.hpp"
#include "porous_hybrid.hpp"
#include "side_geometry.hpp"
#include "stream_rows.hpp"

namespace mha {
namespace {

constexpr int kPmhWaves = 4;  // wavefronts (of 64 elements) per workgroup
// (pmh_wave_sync, pmh_stream_rows: stream_rows.hpp, shared with porous_wg_fused.hip)

template <int DIM, bool EXPR>
__global__ __launch_bounds__(64 * kPmhWaves) void porous_hybrid_fused_kernel(BlockDev b, SideTablesDev st, PmhElementDev a, TimeDev tm) {
  constexpr int NN = 1 << DIM, NU = 2 * DIM, NI = 1 + NU, NSYM = NU * (NU + 1) / 2;
  constexpr int SBW = (NU * NU) | 1;  // staging row stride of the widest output
  __shared__ double s_out[kPmhWaves][64 * SBW];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t e0 = ((int64_t)blockIdx.x * kPmhWaves + wv) * 64;  // first element of the wavefront
  if (e0 >= b.e_count) return;
  const int cnt = (int)(b.e_count - e0 < 64 ? b.e_count - e0 : 64);
  const bool active = lane < cnt;
  const int64_t el = e0 + (active ? lane : 0);  // idle lanes of the last wavefront shadow its first element
  const int e = b.e_begin + (int)el, nq = b.nq, nqs = st.nqs;
  auto sym = [](int f, int g) { return f >= g ? f * (f + 1) / 2 + g : g * (g + 1) / 2 + f; };

  double xn[NN * DIM];
#pragma unroll
  for (int k = 0; k < NN * DIM; ++k) xn[k] = b.nodes[(size_t)e * NN * DIM + k];

  // ---- volume points: A (lower triangle), B, the source integral ----
  double A[NSYM], B[NU], srcint = 0.0;
#pragma unroll
  for (int k = 0; k < NSYM; ++k) A[k] = 0.0;
#pragma unroll
  for (int f = 0; f < NU; ++f) B[f] = 0.0;
  const double kdata = a.edata ? 1.0 / a.edata[(size_t)e * a.ecols] : 0.0;
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
    // G_cc' = sum_d Kinv_d J_dc J_dc'
    double G[DIM * DIM];
#pragma unroll
    for (int c = 0; c < DIM * DIM; ++c) G[c] = 0.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      const double Kinv = a.edata ? kdata : eval_func<DIM, EXPR>(a.f[1 + d], e, q, nq, x);
#pragma unroll
      for (int c = 0; c < DIM; ++c)
#pragma unroll
        for (int c2 = 0; c2 <= c; ++c2) G[c * DIM + c2] += Kinv * J[d * DIM + c] * J[d * DIM + c2];
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
      for (int g = 0; g <= f; ++g) A[f * (f + 1) / 2 + g] += G[(f >> 1) * DIM + (g >> 1)] * t[f] * t[g] * w;
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

  // ---- orientation signs: v_f = sg_f v_f,raw ----
  if (a.orient) {
    double sg[NU];
#pragma unroll
    for (int f = 0; f < NU; ++f) sg[f] = (double)a.orient[(size_t)e * NI + 1 + f];
#pragma unroll
    for (int f = 0; f < NU; ++f) {
      B[f] *= sg[f];
#pragma unroll
      for (int g = 0; g <= f; ++g) A[f * (f + 1) / 2 + g] *= sg[f] * sg[g];
    }
#pragma unroll
    for (int k = 0; k < NU; ++k) C[k] *= sg[pmh_dof_of_face(k)];
  }

  // ---- the state and r = -res.val() ----
  const int32_t *L = b.lids + (size_t)e * NI;
  const double p = stage_value(tm, L[b.offsets[0]]);
  double uf[NU], ru[NU], rl[NU], lam[NU];
#pragma unroll
  for (int f = 0; f < NU; ++f) uf[f] = stage_value(tm, L[b.offsets[1 + f]]);
#pragma unroll
  for (int k = 0; k < NU; ++k) lam[k] = a.lambda[(size_t)e * NU + k];
  double rp = -srcint;
#pragma unroll
  for (int f = 0; f < NU; ++f) rp += B[f] * uf[f];
#pragma unroll
  for (int f = 0; f < NU; ++f) {
    double v = -p * B[f];
#pragma unroll
    for (int g = 0; g < NU; ++g) v += A[sym(f, g)] * uf[g];
    ru[f] = -v;
  }
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    const int f = pmh_dof_of_face(k);
    ru[f] -= C[k] * lam[k];
    rl[k] = C[k] * uf[f];
  }

  // ---- Cholesky A = L L^T in place, then Ai = L^-T L^-1 ----
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    double dj = A[sym(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) dj -= A[sym(j, k)] * A[sym(j, k)];
    if (!(dj > 0.0)) { bad = true; dj = 1.0; }
    const double ljj = sqrt(dj), rinv = 1.0 / ljj;
    A[sym(j, j)] = ljj;
#pragma unroll
    for (int i = j + 1; i < NU; ++i) {
      double v = A[sym(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= A[sym(i, k)] * A[sym(j, k)];
      A[sym(i, j)] = v * rinv;
    }
  }
  double Li[NSYM];  // L^-1, lower triangle
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    Li[sym(j, j)] = 1.0 / A[sym(j, j)];
#pragma unroll
    for (int i = j + 1; i < NU; ++i) {
      double v = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) v -= A[sym(i, k)] * Li[sym(k, j)];
      Li[sym(i, j)] = v / A[sym(i, i)];
    }
  }
  double Ai[NSYM];
#pragma unroll
  for (int i = 0; i < NU; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double v = 0.0;
#pragma unroll
      for (int k = i; k < NU; ++k) v += Li[sym(k, i)] * Li[sym(k, j)];
      Ai[sym(i, j)] = v;
    }

  // ---- the scalar Schur complement of p, the condensed outputs ----
  double Y[NU], sigma = 0.0;
#pragma unroll
  for (int f = 0; f < NU; ++f) {
    double v = 0.0;
#pragma unroll
    for (int g = 0; g < NU; ++g) v += Ai[sym(f, g)] * B[g];
    Y[f] = v;
    sigma += B[f] * v;
  }
  if (!(sigma > 0.0)) { bad = true; sigma = 1.0; }
  const double rsig = 1.0 / sigma;
  double yr = rp;
#pragma unroll
  for (int f = 0; f < NU; ++f) yr += Y[f] * ru[f];
  const double dp = -yr * rsig;
  double du[NU];
#pragma unroll
  for (int f = 0; f < NU; ++f) {
    double v = Y[f] * dp;
#pragma unroll
    for (int g = 0; g < NU; ++g) v += Ai[sym(f, g)] * ru[g];
    du[f] = v;
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
        sb[lane * WP + ka * NU + kb] = finite(C[ka] * C[kb] * (Ai[sym(fa, fb)] - Y[fa] * Y[fb] * rsig));
      }
    pmh_wave_sync();
    pmh_stream_rows<NU * NU>(a.schur + e0 * NU * NU, sb, lane, cnt);
    pmh_wave_sync();
  }
  if (a.gvec) {
    constexpr int WP = NU | 1;
#pragma unroll
    for (int k = 0; k < NU; ++k) sb[lane * WP + k] = finite(rl[k] + C[k] * du[pmh_dof_of_face(k)]);
    pmh_wave_sync();
    pmh_stream_rows<NU>(a.gvec + e0 * NU, sb, lane, cnt);
    pmh_wave_sync();
  }
  if (a.du) {
    constexpr int WP = NI | 1;
    sb[lane * WP] = finite(dp);
#pragma unroll
    for (int f = 0; f < NU; ++f) sb[lane * WP + 1 + f] = finite(du[f]);
    pmh_wave_sync();
    pmh_stream_rows<NI>(a.du + e0 * NI, sb, lane, cnt);
  }
}

template <int DIM>
void launch_dim(const BlockDev &b, const SideTablesDev &st, const PmhElementDev &a, const TimeDev &tm, hipStream_t stream) {
  bool expr = false;
  for (const FuncDesc &f : a.f) expr = expr || has_expression(f);
  const int per_wg = 64 * kPmhWaves, grid = (b.e_count + per_wg - 1) / per_wg;
  auto go = [&](auto kern) {
    require_modest_scratch(kern, "porousMixedHybridized fused kernel");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(per_wg), 0, stream, b, st, a, tm);
    MHA_HIP(hipGetLastError());
  };
  if (expr) go(porous_hybrid_fused_kernel<DIM, true>);
  else go(porous_hybrid_fused_kernel<DIM, false>);
}

}  // namespace

void launch_porous_hybrid_fused(const BlockDev &b, const SideTablesDev &st, const PmhElementDev &a, const TimeDev &tm,
                                hipStream_t stream) {
  if (b.e_count <= 0) return;
  MHA_REQUIRE((b.dim == 2 || b.dim == 3) && b.n == 1 + 2 * b.dim, MHA_ERR_INVALID,
              "porousMixedHybridized fused kernel: p (HVOL 0) and u (HDIV 1) on quads or hexes");
  MHA_REQUIRE(b.e_begin == 0, MHA_ERR_INVALID, "porousMixedHybridized fused kernel: the outputs are those of the whole block");
  for (const double *p : {a.schur, a.gvec, a.du})
    MHA_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0, MHA_ERR_INVALID,
                "porousMixedHybridized fused kernel: schur, gvec and du must be 16-byte aligned (they are stored in 16-byte pieces)");
  if (b.dim == 2) launch_dim<2>(b, st, a, tm, stream);
  else launch_dim<3>(b, st, a, tm, stream);
}

}  // namespace mha
