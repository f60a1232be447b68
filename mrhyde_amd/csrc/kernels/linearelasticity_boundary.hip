// linearelasticity_boundary.hip -- linearelasticity::boundaryResidual on a group of (element, side) entries.
//
// reference: src/physics/linearelasticity.cpp:244-672 with computeStress(onside = true) :931-1099, the side fields of
// evaluateSideSolutionField (src/tools/workset.cpp:1069-1176) and Workset::getSideElementSize (:2682-2696).  The
// boundary-condition type of the group applies to ALL components dx, dy[, dz] of the side:
//   Neumann (traction, :361-371, 419-429, 482-492, 546-556, 609-619):  res(a,d) = -sum_q w g_d N_a       (no Jacobian)
//   weak Dirichlet (Nitsche, :372-390, 430-447, 493-513, 557-577, 620-640), delta = u - D at the side points:
//     res(a,d) = sum_q w [ -(sigma n)_d N_a + pen delta_d N_a - sf (b_d . grad N_a) ]
//     b_dj     = lambda (delta . n) delta_dj + mu (delta_d n_j + delta_j n_d)      (the b vectors of :379-386, 437-443,
//                                                                                    501-509, 565-573, 628-636)
//     pen      = penalty (lambda + 2 mu) / h,  h = (sum_q w)^(1/(dim-1)),  sf = form_param
// Both (sigma n)_d of a trial function N_b e_c and b_d . grad N_a / N_b are the same bilinear form in (n, grad N):
//     T(N; r, s) = lambda n_s d_r N + mu (delta_rs (grad N . n) + n_r d_s N)
//     (sigma(N_b e_c) n)_d = T_s(N_b; c, d)        b_d(N_b e_c) . grad N_a = N_b T(N_a; d, c)
// (T_s: with the stress's lambda, 2 mu under incplanestress, :990-1000), so the Sacado derivative array is
//     d res(a,d) / d u(b,c) = alpha_u sum_q w [ -N_a T_s(N_b; c, d) + pen delta_dc N_a N_b - sf N_b T(N_a; d, c) ].
// Work split: an entry has n = dim * card <= 81 rows and n^2 <= 6 561 matrix entries over at most 16 side points.  Up to
// 32 rows (2-D Q1..Q3, 3-D Q1) one wavefront takes an entry and a workgroup four, as kernels/thermal_boundary.hip;
// above, the whole workgroup takes one entry (26 matrix entries per thread at 81 rows).  The entry's tables -- N, the
// physical gradients and grad N . n at the side points, the side fields -- are at most 20 KB of LDS, so the wave limit,
// not the LDS, bounds the workgroups per CU.  The surface is O(N^{d-1}) against the volume's O(N^d): atomics and the
// CRS column search, as the other boundary kernels.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "launch.hpp"
#include "side_geometry.hpp"

namespace mha {
namespace {

constexpr int kLeThreads = 256, kLeMaxCard = 27, kLeMaxQ = 16;

// doubles of one entry's LDS: N, grad N, grad N . n | u | per point: Ji, then w, lambda_s, lambda, mu, pen, n, delta, sigma n
// | rows (ints)
__host__ __device__ constexpr int le_point_doubles(int dim) { return 5 + 3 * dim; }
__host__ __device__ inline int le_entry_doubles(int dim, int card, int nqs) {
  const int n = dim * card;
  return (card * nqs * (dim + 2) + n + nqs * (dim * dim + le_point_doubles(dim)) + (n + 1) / 2 + 1) & ~1;
}

// TE: the entry is an element of the coupled linearelasticity + thermal block -- its displacement rows are the first
// DIM * le.disp_card of the b.n dofs; traction only (the host refuses everything else on that block)
template <int DIM, int TPE, bool TE>
__device__ __forceinline__ void le_boundary_entry(const BlockDev &b, const SideTablesDev &st, const BoundaryDev &bd,
                                                  const LeBoundaryDev &le, const TimeDev &tm, const ElemOut &out) {
  constexpr int NN = 1 << DIM, PT = le_point_doubles(DIM), NG = kLeThreads / TPE;
  extern __shared__ double smem[];
  const int n = TE ? DIM * le.disp_card : b.n, card = n / DIM, nqs = st.nqs;
  const int grp = threadIdx.x / TPE, t = threadIdx.x % TPE;
  double *s_N = smem + grp * le_entry_doubles(DIM, card, nqs);
  double *s_G = s_N + card * nqs, *s_gn = s_G + card * nqs * DIM;
  double *s_u = s_gn + card * nqs;
  double *s_Ji = s_u + n, *s_pt = s_Ji + nqs * DIM * DIM;
  int *s_row = reinterpret_cast<int *>(s_pt + nqs * PT);
  const int k = blockIdx.x * NG + grp;
  const bool active = k < bd.num;  // inactive groups still take part in the block barriers
  const int e = active ? bd.elem[k] : 0, s = active ? bd.side[k] : 0;
  const bool weak = !TE && bd.bc_type == MHA_BC_WEAK_DIRICHLET;
  const int32_t *L = b.lids + (size_t)e * b.n;

  // A. side geometry, coefficients and data (thread = (side point, function): ONE inlined copy of the deck-string
  // interpreter, which costs registers per copy); gather + seeding value (thread = (component, dof))
  if (active) {
    constexpr int NF = DIM + 2;  // data of the components, lambda, mu
    for (int idx = t; idx < nqs * NF; idx += TPE) {
      const int q = idx / NF, kf = idx - q * NF;
      double Ji[DIM * DIM], nrm[DIM], w, x[DIM];
      side_point<DIM>(b.nodes + (size_t)e * NN * DIM, st, s, q, Ji, nrm, w, x);
      double *p = s_pt + q * PT;
      if (kf == 0) {
        p[0] = w;
#pragma unroll
        for (int d = 0; d < DIM; ++d) p[5 + d] = nrm[d];
#pragma unroll
        for (int i = 0; i < DIM * DIM; ++i) s_Ji[q * DIM * DIM + i] = Ji[i];
      }
      if (kf < DIM || weak) {
        const double v = eval_func<DIM, true>(le.f[kf < DIM ? kf : kf - DIM + 3], k, q, nqs, x, nrm);
        p[kf < DIM ? 5 + DIM + kf : 2 + kf - DIM] = v;  // g_d or D_d (delta_d after phase C) | lambda | mu
      }
    }
    for (int f = t; f < n; f += TPE) {
      const int row = L[b.offsets[f]];
      s_row[f] = row;
      s_u[f] = stage_value(tm, row);
    }
  }
  __syncthreads();
  // B. N, physical gradient = J^{-T} grad_ref and grad N . n at the side points
  if (active) {
    for (int idx = t; idx < card * nqs; idx += TPE) {
      const int a = idx / nqs, q = idx - a * nqs;
      s_N[idx] = st.basis[(size_t)(s * card + a) * nqs + q];
      if (weak) {
        const double *gr = st.grad + ((size_t)(s * card + a) * nqs + q) * DIM;
        double gn = 0.0;
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          double pg = 0.0;
#pragma unroll
          for (int c = 0; c < DIM; ++c) pg += s_Ji[q * DIM * DIM + c * DIM + d] * gr[c];
          s_G[idx * DIM + d] = pg;
          gn += pg * s_pt[q * PT + 5 + d];
        }
        s_gn[idx] = gn;
      }
    }
  }
  __syncthreads();
  if (weak) {
    // C. side fields: delta = u - D, sigma n and the penalty (thread = side point)
    if (active) {
      double vol = 0.0;
      for (int q = 0; q < nqs; ++q) vol += s_pt[q * PT];
      const double h = (DIM == 2) ? vol : sqrt(vol);  // vol^(1/(dim-1)), getSideElementSize
      for (int q = t; q < nqs; q += TPE) {
        double *p = s_pt + q * PT;
        double uv[DIM], gu[DIM][DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          uv[d] = 0.0;
#pragma unroll
          for (int j = 0; j < DIM; ++j) gu[d][j] = 0.0;
        }
        for (int a = 0; a < card; ++a) {
          const double N = s_N[a * nqs + q];
#pragma unroll
          for (int d = 0; d < DIM; ++d) {
            const double ua = s_u[d * card + a];
            uv[d] += ua * N;
#pragma unroll
            for (int j = 0; j < DIM; ++j) gu[d][j] += ua * s_G[(a * nqs + q) * DIM + j];
          }
        }
        const double lam = p[2], mu = p[3], lam_s = (DIM == 2 && le.plane_stress) ? 2.0 * mu : lam;
        p[1] = lam_s;
        double tr = 0.0;
#pragma unroll
        for (int d = 0; d < DIM; ++d) tr += gu[d][d];
        double sn[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          sn[d] = lam_s * tr * p[5 + d];
#pragma unroll
          for (int j = 0; j < DIM; ++j) sn[d] += mu * (gu[d][j] + gu[j][d]) * p[5 + j];
        }
        p[4] = le.penalty * (lam + 2.0 * mu) / h;
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          p[5 + DIM + d] = uv[d] - p[5 + DIM + d];
          p[5 + 2 * DIM + d] = sn[d];
        }
      }
    }
    __syncthreads();
  }
  if (!active) return;
  const double sf = le.form_param;
  // D. residual rows (thread = (component, dof))
  for (int f = t; f < n; f += TPE) {
    const int d = f / card, a = f - d * card;
    double r = 0.0;
    for (int q = 0; q < nqs; ++q) {
      const double *p = s_pt + q * PT;
      const double N = s_N[a * nqs + q];
      if (!weak) {
        r += -p[5 + DIM + d] * N * p[0];
      } else {
        const double *nrm = p + 5, *dl = p + 5 + DIM, *G = s_G + (a * nqs + q) * DIM;
        double dn = 0.0, dg = 0.0;
#pragma unroll
        for (int j = 0; j < DIM; ++j) { dn += dl[j] * nrm[j]; dg += dl[j] * G[j]; }
        const double bg = p[2] * dn * G[d] + p[3] * (dl[d] * s_gn[a * nqs + q] + nrm[d] * dg);  // b_d . grad N_a
        r += (-p[5 + 2 * DIM + d] * N + p[4] * dl[d] * N - sf * bg) * p[0];
      }
    }
    const int row = s_row[f];
    if (out.res && !(b.fixed && b.fixed[row])) unsafeAtomicAdd(out.res + row, -r);
  }
  // E. Jacobian entries (weak Dirichlet only): threads sweep the n x n block
  if (weak && out.compute_jacobian && out.crs_vals) {
    for (int idx = t; idx < n * n; idx += TPE) {
      const int i = idx / n, j = idx - i * n;
      const int d = i / card, a = i - d * card, c = j / card, bb = j - c * card;
      const int ri = s_row[i];
      if (b.fixed && b.fixed[ri]) continue;
      double v = 0.0;
      for (int q = 0; q < nqs; ++q) {
        const double *p = s_pt + q * PT;
        const double *nrm = p + 5, *Ga = s_G + (a * nqs + q) * DIM, *Gb = s_G + (bb * nqs + q) * DIM;
        const double Na = s_N[a * nqs + q], Nb = s_N[bb * nqs + q];
        const double same = (d == c) ? 1.0 : 0.0;
        // T_s(N_b; c, d) and T(N_a; d, c)
        const double Tb = p[1] * nrm[d] * Gb[c] + p[3] * (same * s_gn[bb * nqs + q] + nrm[c] * Gb[d]);
        const double Ta = p[2] * nrm[c] * Ga[d] + p[3] * (same * s_gn[a * nqs + q] + nrm[d] * Ga[c]);
        v += p[0] * (-Na * Tb + p[4] * same * Na * Nb - sf * Nb * Ta);
      }
      const int pos = find_col(b.colind, b.rowptr[ri], b.rowptr[ri + 1], s_row[j]);
      if (pos >= 0) unsafeAtomicAdd(out.crs_vals + pos, tm.alpha_u * v);
    }
  }
}

template <int DIM, int TPE>
__global__ __launch_bounds__(kLeThreads) void linearelasticity_boundary_kernel(BlockDev b, SideTablesDev st, BoundaryDev bd,
                                                                               LeBoundaryDev le, TimeDev tm, ElemOut out) {
  le_boundary_entry<DIM, TPE, false>(b, st, bd, le, tm, out);
}

template <int DIM, int TPE>
__global__ __launch_bounds__(kLeThreads) void linearelasticity_thermal_traction_kernel(BlockDev b, SideTablesDev st,
                                                                                       BoundaryDev bd, LeBoundaryDev le,
                                                                                       TimeDev tm, ElemOut out) {
  le_boundary_entry<DIM, TPE, true>(b, st, bd, le, tm, out);
}

}  // namespace

bool linearelasticity_boundary_supported(int dim, int n, int nqs) {
  return (dim == 2 || dim == 3) && n % dim == 0 && n / dim <= kLeMaxCard && nqs <= kLeMaxQ;
}

void launch_linearelasticity_boundary(const BlockDev &b, const SideTablesDev &st, const BoundaryDev &bd,
                                      const LeBoundaryDev &le, const TimeDev &tm, const ElemOut &out, hipStream_t stream) {
  if (bd.num <= 0) return;
  const bool te = le.disp_card > 0;  // coupled block: traction on the displacement rows
  const int rows = te ? b.dim * le.disp_card : b.n;
  MHA_REQUIRE(!te || (bd.bc_type == MHA_BC_NEUMANN && rows <= b.n), MHA_ERR_INVALID,
              "linearelasticity+thermal: only traction (MHA_BC_NEUMANN) groups are built");
  MHA_REQUIRE(linearelasticity_boundary_supported(b.dim, rows, st.nqs), MHA_ERR_INVALID,
              "linearelasticity boundary kernel: equal-order components with at most " << kLeMaxCard << " dofs each and "
                                                                                      << kLeMaxQ << " side points (got "
                                                                                      << rows << " displacement dofs per element, "
                                                                                      << st.nqs << " side points)");
  const int card = rows / b.dim;
  const bool wave_per_entry = rows <= 32;
  const int per_wg = wave_per_entry ? kLeThreads / 64 : 1;
  const size_t lds = sizeof(double) * per_wg * le_entry_doubles(b.dim, card, st.nqs);
  const int grid = (bd.num + per_wg - 1) / per_wg;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kLeThreads), lds, stream, b, st, bd, le, tm, out);
    MHA_HIP(hipGetLastError());
  };
  if (te) {
    if (b.dim == 2) {
      if (wave_per_entry) go(linearelasticity_thermal_traction_kernel<2, 64>);
      else go(linearelasticity_thermal_traction_kernel<2, kLeThreads>);
    } else {
      if (wave_per_entry) go(linearelasticity_thermal_traction_kernel<3, 64>);
      else go(linearelasticity_thermal_traction_kernel<3, kLeThreads>);
    }
  } else if (b.dim == 2) {
    if (wave_per_entry) go(linearelasticity_boundary_kernel<2, 64>);
    else go(linearelasticity_boundary_kernel<2, kLeThreads>);
  } else {
    if (wave_per_entry) go(linearelasticity_boundary_kernel<3, 64>);
    else go(linearelasticity_boundary_kernel<3, kLeThreads>);
  }
}

}  // namespace mha
