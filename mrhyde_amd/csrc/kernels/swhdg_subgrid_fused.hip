// swhdg_subgrid_fused.hip -- the element step of an HDG subgrid of M x M sub-elements per macro element in ONE kernel:
// the multi-element counterpart of swhdg_fused.hip.  One workgroup per macro element assembles the augmented system
// [A_uu A_ul | r_u; A_lu A_ll | r_l] of the n_int = 3 (M+1)^2 continuous interior unknowns and the 24 macro trace unknowns
// in LDS, eliminates A_uu there and writes only S[24][24], g[24] and du[n_int].
//
// reference: SubGridDtN_Solver::assembleJacobianResidual (src/subgrid/subgridDtN_solver.cpp:681-903; the sum of the
// sub-element terms into the sub-mesh rows :774-808), updateFlux (:1542-1616: computeFlux against the macro trace basis
// over the sub-sides of each macro edge), the loop bookkeeping of nonlinearSolver (:909-1041); physics
// src/physics/shallowwaterHybridized.cpp:113-184 (volumeResidual, every sub-element), :190-263 (boundaryResidual, the 4M
// sub-sides on the macro boundary only: the interior is continuous), :270-368 (computeFlux); the trace state at a
// sub-side point is the macro edge's HFACE basis there (src/subgrid/subgridDtN.cpp:746-870, auxside_basis).
// The reference solves the interior system with a sparse direct solver; at n_int <= 75 the dense Gauss-Jordan solve in
// LDS is the form that never leaves the chip.
// The independent implementation the tests compare with: swhdg_subgrid_blocks.hip + condense.hip / numpy.
//
// Phases (256 threads): (1) state and traces to LDS; (2) point data -- one (side point, direction) or (volume point,
// direction) per thread, Dual numbers as in swhdg_fused.hip; (3) every entry of the augmented block is formed by ONE
// thread that gathers the points touching it in a fixed order (row ownership: no LDS atomics, two runs are
// bit-identical); (4) loop bookkeeping on r_u; (5) Gauss-Jordan with partial pivoting across the workgroup, the pivot
// row and the multiplier column staged in LDS; (6) P = A_lu [X_ul | x_r] on the fp64 matrix cores, one 16 x 16 tile per
// wavefront, S = A_ll - P and g = r_l - P[:, 24] straight from the accumulators.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../../include/mrhyde_amd.h"
#include "device_math.hpp"
#include "launch.hpp"
#include "side_geometry.hpp"
#include "swhdg_side.hpp"
#include "swhdg_subgrid.hpp"

namespace mha {
namespace {

constexpr int kSgThreads = 256, kSgMaxNqs = 4, kSgMaxNq = 9;
constexpr int kSgVolRec = 40;   // per volume point: N_a, dN_a/dx, dN_a/dy (12), w, vr (9), vD (18)
constexpr int kSgSideRec = 27;  // per side point: N_a (4), mu (2), flux * w (3), d flux / d S, d flux / d Shat (* w) (18)

template <int M>
struct SgDims {
  static constexpr int NP = sg_np(M), NI = sg_ni(M), N = NI + 24, LD = (N + 1) | 1;  // (odd row stride: column walks spread over the banks)
};

template <int M>
size_t sg_fused_lds(int nq, int nqs) {
  using D = SgDims<M>;
  const size_t dbl = (size_t)D::N * D::LD + 2 * D::NI + 24 + D::NI + D::LD + (size_t)M * M * nq * kSgVolRec + (size_t)4 * M * nqs * kSgSideRec;
  return dbl * sizeof(double) + (D::NI + 4) * sizeof(int);
}

template <int M>
__global__ __launch_bounds__(kSgThreads) void swhdg_subgrid_fused_kernel(BlockDev b, SideTablesDev st, SwhElementDev a, TimeDev tm,
                                                                         PhysParamsDev pp, SwhFusedOut o) {
  constexpr int DIM = 2, NN = 4;
  using D = SgDims<M>;
  constexpr int NP = D::NP, NI = D::NI, N = D::N, LD = D::LD;
  extern __shared__ double sg_lds[];
  const int nq = b.nq, nqs = st.nqs, nvp = M * M * nq, nsp = 4 * M * nqs;
  double *A = sg_lds, *s_u = A + N * LD, *s_ud = s_u + NI, *s_l = s_ud + NI, *s_mult = s_l + 24, *s_prow = s_mult + NI;
  double *s_vp = s_prow + LD, *s_sp = s_vp + nvp * kSgVolRec;
  int *s_rows = reinterpret_cast<int *>(s_sp + nsp * kSgSideRec), *s_go = s_rows + NI;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int64_t me = blockIdx.x;                    // macro element
  const int e0 = b.e_begin + (int)me * M * M;       // its first sub-element
  // ---- (1) state of the interior unknowns and the macro traces ----
  for (int r = tid; r < NI; r += kSgThreads) {
    const int row = sg_row(b, M, e0, r / NP, r % NP);
    double ue, ud;
    stage_state(tm, row, ue, ud);
    s_rows[r] = row;
    s_u[r] = ue;
    s_ud[r] = ud;
  }
  if (tid < 24) s_l[tid] = a.lambda[me * 24 + tid];
  if (tid == 0) s_go[0] = 1;
  __syncthreads();
  // ---- (2a) side points of the 4M boundary sub-sides: (point, direction 0 value, 1..3 d/dS_k, 4..6 d/dShat_k) ----
  for (int idx = tid; idx < nsp * 7; idx += kSgThreads) {
    const int P = idx / 7, dir = idx - P * 7, s = P / (M * nqs), rem = P - s * M * nqs, j = rem / nqs, q = rem - j * nqs;
    const int edge = (s + 1) & 3;  // shards side 0,1,2,3 (bottom, right, top, left) -> HFACE edge 1,2,3,0
    int ex, ey;
    sg_side_elem(M, s, j, ex, ey);
    const double *xn = b.nodes + (size_t)(e0 + ey * M + ex) * NN * DIM;
    double Ji[DIM * DIM], nrm[DIM], w, x[DIM];
    side_point<DIM>(xn, st, s, q, Ji, nrm, w, x);
    const double tl = (edge & 1) ? st.ip[(s * nqs + q) * DIM] : st.ip[(s * nqs + q) * DIM + 1];
    const double tc = -1.0 + (2.0 * j + (tl + 1.0)) / M;  // the macro edge's coordinate of the sub-side point
    const double mu0 = 0.5 * (1.0 - tc), mu1 = 0.5 * (1.0 + tc);
    double S[3] = {0, 0, 0}, Sh[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int dof = 0; dof < 4; ++dof) S[i] += s_u[i * NP + sg_node(M, ex, ey, dof)] * st.basis[(s * 4 + dof) * nqs + q];
      Sh[i] = s_l[i * 8 + edge * 2] * mu0 + s_l[i * 8 + edge * 2 + 1] * mu1;
    }
    const int stype = a.side_types ? a.side_types[me * 4 + s] : 0;
    Dual dS[3], dSh[3], f[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { dS[i] = mk(S[i], dir == 1 + i ? 1.0 : 0.0); dSh[i] = mk(Sh[i], dir == 4 + i ? 1.0 : 0.0); }
    swh_interface_flux_lean(stype, a.roe != 0, dS, dSh, a.farfield, nrm[0], nrm[1], a.g, f);
    double *rec = s_sp + P * kSgSideRec;
    if (dir == 0) {
#pragma unroll
      for (int dof = 0; dof < 4; ++dof) rec[dof] = st.basis[(s * 4 + dof) * nqs + q];
      rec[4] = mu0;
      rec[5] = mu1;
#pragma unroll
      for (int i = 0; i < 3; ++i) rec[6 + i] = f[i].v * w;
    } else {
      const int which = dir > 3, kk = (dir - 1) % 3;
#pragma unroll
      for (int i = 0; i < 3; ++i) rec[9 + which * 9 + i * 3 + kk] = f[i].d * w;
    }
  }
  // ---- (2b) volume points of every sub-element: (point, direction 0..3); shallowwaterHybridized::volumeResidual ----
  for (int idx = tid; idx < nvp * 4; idx += kSgThreads) {
    const int V = idx >> 2, dir = idx & 3, se = V / nq, q = V - se * nq, ex = se % M, ey = se / M;
    const double *xn = b.nodes + (size_t)(e0 + se) * NN * DIM;
    double J[DIM * DIM] = {0, 0, 0, 0}, Ji[DIM * DIM], det, x[DIM] = {0, 0}, xi[DIM] = {0, 0};
    const double vx[4] = {-1.0, 1.0, 1.0, -1.0}, vy[4] = {-1.0, -1.0, 1.0, 1.0};  // reference vertices (shards order)
#pragma unroll
    for (int k = 0; k < NN; ++k) {
      const double nv = b.nodeval[k * nq + q];
      xi[0] += nv * vx[k];
      xi[1] += nv * vy[k];
#pragma unroll
      for (int r = 0; r < DIM; ++r) {
        x[r] += xn[k * DIM + r] * nv;
#pragma unroll
        for (int cc = 0; cc < DIM; ++cc) J[r * DIM + cc] += xn[k * DIM + r] * b.nodegrad[(k * nq + q) * DIM + cc];
      }
    }
    double src[3] = {0.0, 0.0, 0.0};
    if (dir == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) src[i] = eval_func<DIM, false>(pp.f[i], e0 + se, q, nq, x);
    }
    invert<DIM>(J, Ji, det);
    const double w = b.ref_wts[q] * det;
    double Nv[4], Gx[4], Gy[4];  // HGRAD order 1 in dof order (x fastest)
#pragma unroll
    for (int aa = 0; aa < 4; ++aa) {
      const double sx = (aa & 1) ? 1.0 : -1.0, sy = (aa & 2) ? 1.0 : -1.0;
      Nv[aa] = 0.25 * (1.0 + sx * xi[0]) * (1.0 + sy * xi[1]);
      const double gxi = 0.25 * sx * (1.0 + sy * xi[1]), get = 0.25 * sy * (1.0 + sx * xi[0]);
      Gx[aa] = gxi * Ji[0] + get * Ji[2];  // J^-T grad_ref
      Gy[aa] = gxi * Ji[1] + get * Ji[3];
    }
    double S[3] = {0, 0, 0}, Sd[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int aa = 0; aa < 4; ++aa) {
        const int nd = i * NP + sg_node(M, ex, ey, aa);
        S[i] += s_u[nd] * Nv[aa];
        Sd[i] += s_ud[nd] * Nv[aa];
      }
    Dual dS[3], F[3][2];
#pragma unroll
    for (int i = 0; i < 3; ++i) dS[i] = mk(S[i], dir == 1 + i ? 1.0 : 0.0);
    swh_flux_vector(dS, a.g, F);
    double *rec = s_vp + V * kSgVolRec;
    if (dir == 0) {
#pragma unroll
      for (int aa = 0; aa < 4; ++aa) { rec[aa] = Nv[aa]; rec[4 + aa] = Gx[aa]; rec[8 + aa] = Gy[aa]; }
      rec[12] = w;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        rec[13 + i] = (Sd[i] - src[i]) * w;  // (v, dS/dt) - (v, source)
        rec[16 + i] = -F[i][0].v * w;        // -(dv/dx, F_x)
        rec[19 + i] = -F[i][1].v * w;        // -(dv/dy, F_y)
      }
    } else {
      const int kk = dir - 1;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        rec[22 + (i * 2 + 0) * 3 + kk] = F[i][0].d * w;
        rec[22 + (i * 2 + 1) * 3 + kk] = F[i][1].d * w;
      }
    }
  }
  __syncthreads();
  // ---- (3) the augmented block, one owner per entry: rows / columns (equation, test function) ----
  // interior index r < NI: equation r / NP, lattice node r % NP; trace index NI + t: equation t / 8, edge (t & 7) / 2,
  // function t & 1; column N is the right-hand side
  for (int idx = tid; idx < N * (N + 1); idx += kSgThreads) {
    const int r = idx / (N + 1), c = idx - r * (N + 1);
    const bool rint = r < NI, rhs = c == N, cint = c < NI;
    int ri, rax = 0, ray = 0, redge = 0, rf = 0, ck = 0, cax = 0, cay = 0, cedge = 0, cf = 0;
    if (rint) { ri = r / NP; const int nd = r - ri * NP; rax = nd % (M + 1); ray = nd / (M + 1); }
    else { const int t = r - NI; ri = t >> 3; redge = (t & 7) >> 1; rf = t & 1; }
    if (cint) { ck = c / NP; const int nd = c - ck * NP; cax = nd % (M + 1); cay = nd / (M + 1); }
    else if (!rhs) { const int t = c - NI; ck = t >> 3; cedge = (t & 7) >> 1; cf = t & 1; }
    const double cscale = cint ? tm.alpha_u : 1.0;
    const int which = cint ? 0 : 1;
    double v = 0.0;
    // side terms: the sub-sides this row's test function lives on
    for (int s = 0; s < 4; ++s) {
      const int edge = (s + 1) & 3;
      if (!rint && redge != edge) continue;
      for (int j = 0; j < M; ++j) {
        int ex, ey;
        sg_side_elem(M, s, j, ex, ey);
        int la = 0, lb = -1;
        if (rint) { la = sg_local(rax, ray, ex, ey); if (la < 0) continue; }
        if (!rhs) {
          if (cint) { lb = sg_local(cax, cay, ex, ey); if (lb < 0) continue; }
          else if (cedge != edge) continue;
        }
        for (int q = 0; q < nqs; ++q) {
          const double *rec = s_sp + ((s * M + j) * nqs + q) * kSgSideRec;
          const double wr = rint ? rec[la] : rec[4 + rf];
          if (rhs) v -= rec[6 + ri] * wr;
          else v += wr * rec[9 + which * 9 + ri * 3 + ck] * (cint ? rec[lb] : rec[4 + cf]) * cscale;
        }
      }
    }
    // volume terms: interior rows against interior columns and the right-hand side, the sub-elements that hold both nodes
    if (rint && (cint || rhs)) {
      for (int ey = (ray > 0 ? ray - 1 : 0); ey <= (ray < M ? ray : M - 1); ++ey)
        for (int ex = (rax > 0 ? rax - 1 : 0); ex <= (rax < M ? rax : M - 1); ++ex) {
          const int la = sg_local(rax, ray, ex, ey);
          int lb = 0;
          if (cint) { lb = sg_local(cax, cay, ex, ey); if (lb < 0) continue; }
          for (int q = 0; q < nq; ++q) {
            const double *rec = s_vp + ((ey * M + ex) * nq + q) * kSgVolRec;
            const double n_a = rec[la], gx = rec[4 + la], gy = rec[8 + la];
            if (rhs) {
              v -= rec[13 + ri] * n_a + rec[16 + ri] * gx + rec[19 + ri] * gy;
            } else {  // -alpha_u (dN_a/dx_d, dF_i^d/dS_k N_b) + alpha_t (N_a, N_b) on the diagonal variable blocks
              const double nb = rec[lb];
              v += -tm.alpha_u * nb * (rec[22 + (ri * 2 + 0) * 3 + ck] * gx + rec[22 + (ri * 2 + 1) * 3 + ck] * gy);
              if (ri == ck) v += tm.alpha_t * rec[12] * nb * n_a;
            }
          }
        }
    }
    A[r * LD + c] = v;
  }
  __syncthreads();
  // ---- (4) loop bookkeeping of nonlinearSolver (subgrid.hip: combine) on the interior residual, per macro element ----
  if (o.pass >= 0 && o.rn0) {
    if (wv == 0) {
      double nrm = 0.0;
      for (int i = lane; i < NI; i += 64) nrm = fmax(nrm, fabs(A[i * LD + N]));
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) nrm = fmax(nrm, __shfl_xor(nrm, off));
      if (lane == 0) s_go[0] = swh_loop_bookkeeping(o, me, nrm);
    }
  } else if (tid == 0 && o.active) {
    s_go[0] = o.active[me];
  }
  // (the norm reads the right-hand-side column in wavefront 0 alone; the first pivot swap below rewrites an entry of that
  // column from whichever wavefront holds thread N - 1)
  __syncthreads();
  // ---- (5) Gauss-Jordan on the interior rows, partial pivoting; columns <= k are not touched again ----
  bool bad = false;
  for (int k = 0; k < NI; ++k) {
    double best = -1.0;
    int piv = k;
    for (int i = k + lane; i < NI; i += 64) {
      const double av = fabs(A[i * LD + k]);
      if (av > best) { best = av; piv = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {  // every wavefront finds the same pivot: largest entry, lowest row on a tie
      const double ob = __shfl_xor(best, off);
      const int op = __shfl_xor(piv, off);
      if (ob > best || (ob == best && op < piv)) { best = ob; piv = op; }
    }
    if (!(best > 0.0)) { bad = true; break; }
    const double akk = A[piv * LD + k];
    for (int c = k + 1 + tid; c <= N; c += kSgThreads) {  // normalised pivot row; row piv takes what row k held
      s_prow[c] = A[piv * LD + c] / akk;
      if (piv != k) A[piv * LD + c] = A[k * LD + c];
    }
    for (int i = tid; i < NI; i += kSgThreads) s_mult[i] = A[(i == piv ? k : i) * LD + k];
    __syncthreads();
    for (int i = wv; i < NI; i += kSgThreads / 64) {
      const double mi = s_mult[i];
      if (i == k) { for (int c = k + 1 + lane; c <= N; c += 64) A[i * LD + c] = s_prow[c]; }
      else { for (int c = k + 1 + lane; c <= N; c += 64) A[i * LD + c] -= mi * s_prow[c]; }
    }
    __syncthreads();
  }
  if (bad) {  // (uniform: every wavefront saw the same pivot)
    if (tid == 0 && o.singular) atomicAdd(o.singular, 1);
    return;
  }
  // du = x_r; sol += du for the macro elements still in their loop (subgrid.hip: update), fused
  {
    const bool go = s_go[0] != 0;
    for (int i = tid; i < NI; i += kSgThreads) {
      const double dui = A[i * LD + N];
      if (o.du) o.du[me * NI + i] = dui;
      if (o.update_u && go) o.update_u[s_rows[i]] += dui;
    }
  }
  // ---- (6) P = A_lu [X_ul | x_r] on the matrix cores: 2 x 2 tiles of 16 x 16, one per wavefront, K = n_int ----
  if (o.schur || o.gvec) {
    typedef double v4d __attribute__((ext_vector_type(4)));
    const int l15 = lane & 15, g4 = lane >> 4, rt = wv >> 1, ct = wv & 1;
    const int arow = rt * 16 + l15, bcol = ct * 16 + l15;
    v4d d = {0.0, 0.0, 0.0, 0.0};
    for (int ks = 0; ks < (NI + 3) / 4; ++ks) {
      const int kk = 4 * ks + g4;
      const bool kin = kk < NI;
      const double av = (kin && arow < 24) ? A[(NI + arow) * LD + kk] : 0.0;
      const double bv = (kin && bcol <= 24) ? A[kk * LD + NI + bcol] : 0.0;
      d = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, d, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = rt * 16 + g4 + 4 * u;
      if (row < 24 && bcol <= 24) {
        const double sacc = A[(NI + row) * LD + NI + bcol] - d[u];
        if (bcol < 24) { if (o.schur) o.schur[(me * 24 + row) * 24 + bcol] = sacc; }
        else if (o.gvec) o.gvec[me * 24 + row] = sacc;
      }
    }
  }
}

template <int M>
void launch_m(const BlockDev &b, const SideTablesDev &st, const SwhElementDev &a, const TimeDev &tm, const PhysParamsDev &pp,
              const SwhFusedOut &o, hipStream_t stream) {
  auto kern = swhdg_subgrid_fused_kernel<M>;
  const size_t lds = sg_fused_lds<M>(b.nq, st.nqs);
  MHA_REQUIRE(lds <= 160 * 1024, MHA_ERR_INVALID, "fused HDG subgrid kernel: " << lds << " B of LDS needed, 163840 available");
  static bool prepared = false;  // (per instantiation)
  // What the kernel may take beyond the 64 KB every device grants: raised once per size, not per launch.  The attribute
  // belongs to the current device, so the record is kept per device (a device beyond the table sets it on every launch).
  constexpr int kDevs = 64;
  static size_t lds_raised[kDevs] = {};
  if (!prepared) {
    require_modest_scratch(kern, "fused HDG subgrid kernel");
    prepared = true;
  }
  int dev = 0;
  MHA_HIP(hipGetDevice(&dev));
  const size_t allowed = dev < kDevs ? std::max<size_t>(lds_raised[dev], 64 * 1024) : 64 * 1024;
  if (lds > allowed) {
    MHA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (dev < kDevs) lds_raised[dev] = lds;
  }
  hipLaunchKernelGGL(kern, dim3(b.e_count / (M * M)), dim3(kSgThreads), lds, stream, b, st, a, tm, pp, o);
  MHA_HIP(hipGetLastError());
}

}  // namespace

void launch_swhdg_subgrid_fused(int m, const BlockDev &b, const SideTablesDev &st, const SwhElementDev &a, const TimeDev &tm,
                                const PhysParamsDev &pp, const SwhFusedOut &o, hipStream_t stream) {
  if (b.e_count <= 0) return;
  MHA_REQUIRE(m >= 1 && m <= kSgMaxM, MHA_ERR_INVALID, "fused HDG subgrid kernel: m must be in 1.." << kSgMaxM);
  MHA_REQUIRE(b.dim == 2 && b.n == 12 && b.e_begin == 0 && b.e_count % (m * m) == 0 && st.nqs <= kSgMaxNqs && b.nq <= kSgMaxNq,
              MHA_ERR_INVALID, "fused HDG subgrid kernel: 2-D, three order-1 HGRAD variables, whole macro elements, at most "
                                   << kSgMaxNqs << " points per side and " << kSgMaxNq << " volume points");
  for (int i = 0; i < 3; ++i)
    MHA_REQUIRE(pp.f[i].kind != MHA_FUNC_EXPRESSION, MHA_ERR_INVALID,
                "fused HDG subgrid kernel: deck-string sources are not taken");
  switch (m) {
    case 1: launch_m<1>(b, st, a, tm, pp, o, stream); break;
    case 2: launch_m<2>(b, st, a, tm, pp, o, stream); break;
    case 3: launch_m<3>(b, st, a, tm, pp, o, stream); break;
    default: launch_m<4>(b, st, a, tm, pp, o, stream); break;
  }
}

}  // namespace mha
