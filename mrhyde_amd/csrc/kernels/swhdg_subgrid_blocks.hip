// swhdg_subgrid_blocks.hip -- the UNCONDENSED block [n_int + 24][n_int + 24] and right-hand side of every macro element of
// an HDG subgrid of M x M sub-elements (mha_swhdg_subgrid_blocks): a plain kernel, one thread per row, everything
// recomputed per row and accumulated point by point into global memory.  Slow on purpose: it is the independent
// implementation the fused kernel (swhdg_subgrid_fused.hip) is compared with, in the role the four-kernel pipeline plays
// for swhdg_fused.hip -- another decomposition (scatter per row instead of a gather per entry), another summation order,
// the full eigendecomposition (swh_interface_flux) instead of the lean characteristic products.
//
// reference: SubGridDtN_Solver::assembleJacobianResidual (src/subgrid/subgridDtN_solver.cpp:681-903, :774-808), updateFlux
// (:1542-1616); src/physics/shallowwaterHybridized.cpp:113-184 (volume), :190-263 (boundary), :270-368 (flux);
// src/subgrid/subgridDtN.cpp:746-870 (the macro trace basis at the sub-side points).  Index conventions: swhdg_subgrid.hpp.
#include <hip/hip_runtime.h>

#include "../../../include/mrhyde_amd.h"
#include "device_math.hpp"
#include "launch.hpp"
#include "side_geometry.hpp"
#include "swhdg_side.hpp"
#include "swhdg_subgrid.hpp"

namespace mha {
namespace {

constexpr int kSbThreads = 128;

__global__ __launch_bounds__(kSbThreads) void swhdg_subgrid_blocks_kernel(int M, BlockDev b, SideTablesDev st, SwhElementDev a,
                                                                          TimeDev tm, PhysParamsDev pp) {
  constexpr int DIM = 2, NN = 4;
  const int NP = sg_np(M), NI = sg_ni(M), N = NI + 24, r = threadIdx.x;
  if (r >= N) return;
  const int64_t me = blockIdx.x;
  const int e0 = b.e_begin + (int)me * M * M, nq = b.nq, nqs = st.nqs;
  double *out = a.blocks ? a.blocks + (me * N + r) * N : nullptr;
  if (out) for (int c = 0; c < N; ++c) out[c] = 0.0;
  double rhs = 0.0;
  const bool rint = r < NI;
  int ri, rax = 0, ray = 0, redge = 0, rf = 0;
  if (rint) { ri = r / NP; const int nd = r - ri * NP; rax = nd % (M + 1); ray = nd / (M + 1); }
  else { const int t = r - NI; ri = t >> 3; redge = (t & 7) >> 1; rf = t & 1; }
  // ---- side terms ----
  for (int s = 0; s < 4; ++s) {
    const int edge = (s + 1) & 3;
    if (!rint && redge != edge) continue;
    for (int j = 0; j < M; ++j) {
      int ex, ey;
      sg_side_elem(M, s, j, ex, ey);
      const int la = rint ? sg_local(rax, ray, ex, ey) : 0;
      if (la < 0) continue;
      const double *xn = b.nodes + (size_t)(e0 + ey * M + ex) * NN * DIM;
      double ul[3][4];
      for (int i = 0; i < 3; ++i)
        for (int dof = 0; dof < 4; ++dof) ul[i][dof] = stage_value(tm, sg_row(b, M, e0, i, sg_node(M, ex, ey, dof)));
      for (int q = 0; q < nqs; ++q) {
        double Ji[DIM * DIM], nrm[DIM], w, x[DIM];
        side_point<DIM>(xn, st, s, q, Ji, nrm, w, x);
        const double tl = (edge & 1) ? st.ip[(s * nqs + q) * DIM] : st.ip[(s * nqs + q) * DIM + 1];
        const double tc = -1.0 + (2.0 * j + (tl + 1.0)) / M;
        const double mu[2] = {0.5 * (1.0 - tc), 0.5 * (1.0 + tc)};
        double Nb[4];
        for (int dof = 0; dof < 4; ++dof) Nb[dof] = st.basis[(s * 4 + dof) * nqs + q];
        const double wr = (rint ? Nb[la] : mu[rf]) * w;
        if (wr == 0.0) continue;
        double S[3] = {0, 0, 0}, Sh[3];
        for (int i = 0; i < 3; ++i) {
          for (int dof = 0; dof < 4; ++dof) S[i] += ul[i][dof] * Nb[dof];
          Sh[i] = a.lambda[me * 24 + i * 8 + edge * 2] * mu[0] + a.lambda[me * 24 + i * 8 + edge * 2 + 1] * mu[1];
        }
        const int stype = a.side_types ? a.side_types[me * 4 + s] : 0;
        for (int dir = 0; dir < 7; ++dir) {
          Dual dS[3], dSh[3], f[3];
          for (int i = 0; i < 3; ++i) { dS[i] = mk(S[i], dir == 1 + i ? 1.0 : 0.0); dSh[i] = mk(Sh[i], dir == 4 + i ? 1.0 : 0.0); }
          swh_interface_flux(stype, a.roe != 0, dS, dSh, a.farfield, nrm[0], nrm[1], a.g, f);
          if (dir == 0) rhs -= f[ri].v * wr;
          else if (out) {
            const double dv = f[ri].d * wr;
            if (dir <= 3) {  // through S: the four interior unknowns of variable dir - 1 on this sub-element
              for (int dof = 0; dof < 4; ++dof) out[(dir - 1) * NP + sg_node(M, ex, ey, dof)] += dv * Nb[dof] * tm.alpha_u;
            } else {         // through Shat: the two trace unknowns of variable dir - 4 on this macro edge
              for (int k = 0; k < 2; ++k) out[NI + (dir - 4) * 8 + edge * 2 + k] += dv * mu[k];
            }
          }
        }
      }
    }
  }
  // ---- volume terms of the sub-elements around an interior row's node ----
  if (rint) {
    for (int ey = (ray > 0 ? ray - 1 : 0); ey <= (ray < M ? ray : M - 1); ++ey)
      for (int ex = (rax > 0 ? rax - 1 : 0); ex <= (rax < M ? rax : M - 1); ++ex) {
        const int la = sg_local(rax, ray, ex, ey), se = ey * M + ex;
        const double *xn = b.nodes + (size_t)(e0 + se) * NN * DIM;
        double ul[3][4], udl[3][4];
        for (int i = 0; i < 3; ++i)
          for (int dof = 0; dof < 4; ++dof) stage_state(tm, sg_row(b, M, e0, i, sg_node(M, ex, ey, dof)), ul[i][dof], udl[i][dof]);
        for (int q = 0; q < nq; ++q) {
          double J[DIM * DIM] = {0, 0, 0, 0}, Ji[DIM * DIM], det, x[DIM] = {0, 0}, xi[DIM] = {0, 0};
          const double vx[4] = {-1.0, 1.0, 1.0, -1.0}, vy[4] = {-1.0, -1.0, 1.0, 1.0};
          for (int k = 0; k < NN; ++k) {
            const double nv = b.nodeval[k * nq + q];
            xi[0] += nv * vx[k];
            xi[1] += nv * vy[k];
            for (int d = 0; d < DIM; ++d) {
              x[d] += xn[k * DIM + d] * nv;
              for (int cc = 0; cc < DIM; ++cc) J[d * DIM + cc] += xn[k * DIM + d] * b.nodegrad[(k * nq + q) * DIM + cc];
            }
          }
          invert<DIM>(J, Ji, det);
          const double w = b.ref_wts[q] * det;
          double Nv[4], Gx[4], Gy[4];
          for (int aa = 0; aa < 4; ++aa) {
            const double sx = (aa & 1) ? 1.0 : -1.0, sy = (aa & 2) ? 1.0 : -1.0;
            Nv[aa] = 0.25 * (1.0 + sx * xi[0]) * (1.0 + sy * xi[1]);
            const double gxi = 0.25 * sx * (1.0 + sy * xi[1]), get = 0.25 * sy * (1.0 + sx * xi[0]);
            Gx[aa] = gxi * Ji[0] + get * Ji[2];
            Gy[aa] = gxi * Ji[1] + get * Ji[3];
          }
          double S[3] = {0, 0, 0}, Sd = 0.0;
          for (int i = 0; i < 3; ++i)
            for (int aa = 0; aa < 4; ++aa) S[i] += ul[i][aa] * Nv[aa];
          for (int aa = 0; aa < 4; ++aa) Sd += udl[ri][aa] * Nv[aa];
          const double src = eval_func<DIM, false>(pp.f[ri], e0 + se, q, nq, x);
          for (int dir = 0; dir < 4; ++dir) {
            Dual dS[3], F[3][2];
            for (int i = 0; i < 3; ++i) dS[i] = mk(S[i], dir == 1 + i ? 1.0 : 0.0);
            swh_flux_vector(dS, a.g, F);
            if (dir == 0) {
              rhs -= ((Sd - src) * Nv[la] - F[ri][0].v * Gx[la] - F[ri][1].v * Gy[la]) * w;
            } else if (out) {
              const double dv = -tm.alpha_u * (F[ri][0].d * Gx[la] + F[ri][1].d * Gy[la]) * w;
              for (int bb = 0; bb < 4; ++bb) out[(dir - 1) * NP + sg_node(M, ex, ey, bb)] += dv * Nv[bb];
            }
          }
          if (out)
            for (int bb = 0; bb < 4; ++bb) out[ri * NP + sg_node(M, ex, ey, bb)] += tm.alpha_t * w * Nv[la] * Nv[bb];
        }
      }
  }
  if (a.res) a.res[me * N + r] = rhs;
}

}  // namespace

void launch_swhdg_subgrid_blocks(int m, const BlockDev &b, const SideTablesDev &st, const SwhElementDev &a, const TimeDev &tm,
                                 const PhysParamsDev &pp, hipStream_t stream) {
  if (b.e_count <= 0) return;
  MHA_REQUIRE(m >= 1 && m <= kSgMaxM, MHA_ERR_INVALID, "HDG subgrid blocks: m must be in 1.." << kSgMaxM);
  MHA_REQUIRE(b.dim == 2 && b.n == 12 && b.e_begin == 0 && b.e_count % (m * m) == 0, MHA_ERR_INVALID,
              "HDG subgrid blocks: 2-D, three order-1 HGRAD variables, whole macro elements");
  for (int i = 0; i < 3; ++i)
    MHA_REQUIRE(pp.f[i].kind != MHA_FUNC_EXPRESSION, MHA_ERR_INVALID, "HDG subgrid blocks: deck-string sources are not taken");
  static bool prepared = false;
  if (!prepared) {
    require_modest_scratch(swhdg_subgrid_blocks_kernel, "HDG subgrid blocks kernel");
    prepared = true;
  }
  hipLaunchKernelGGL(swhdg_subgrid_blocks_kernel, dim3(b.e_count / (m * m)), dim3(kSbThreads), 0, stream, m, b, st, a, tm, pp);
  MHA_HIP(hipGetLastError());
}

}  // namespace mha
