// helmholtz_boundary.hip -- helmholtz::boundaryResidual on a group of (element, side) entries of type MHA_BC_NEUMANN.
//
// reference: src/physics/helmholtz.cpp:254-419 (the non-fractional branch, :357-375), the side fields of
// evaluateSideSolutionField (src/tools/workset.cpp:1069-1176).  The Robin condition alpha u + du/dn - source = 0 with
// the boundary term of the volume form's integration by parts.  At side point q, normal n, weight w, with the test
// pair vr = vi = N_a (ureal and uimag have one order):
//   c2durdn = sum_d (c2r_d d_d ur - c2i_d d_d ui) n_d          c2duidn = sum_d (c2r_d d_d ui + c2i_d d_d ur) n_d
//   Br = ar (ur + ui) - ai (ui - ur) + (durdn + duidn) - (source_r_side + source_i_side) - (c2durdn + c2duidn)
//   Bi = ar (ui - ur) + ai (ur + ui) + (duidn - durdn) - (source_i_side - source_r_side) - (c2duidn - c2durdn)
//   res(ureal, a) += w N_a Br          res(uimag, a) += w N_a Bi
// The form is linear in u.  With gn_b = grad N_b . n, A_b = sum_d c2r_d d_d N_b n_d, B_b = sum_d c2i_d d_d N_b n_d the
// Sacado derivative array is alpha_u sum_q w N_a C(q; b) with
//   d Br / d ur_b = (ar + ai) N_b + gn_b - (A_b + B_b)        d Br / d ui_b = (ar - ai) N_b + gn_b - (A_b - B_b)
//   d Bi / d ur_b = (ai - ar) N_b - gn_b + (A_b - B_b)        d Bi / d ui_b = (ar + ai) N_b + gn_b - (A_b + B_b)
// -- the N_a (grad N_b . n) blocks between all four variable pairs.
// Work split as kernels/linearelasticity_boundary.hip: an entry has n = 2 card <= 54 rows (2-D Q4: 50, 3-D Q2: 54) and
// n^2 <= 2 916 matrix entries over at most 16 side points.  Up to 32 rows (2-D Q1..Q3, 3-D Q1) one wavefront takes an
// entry and a workgroup four; above, the whole workgroup takes one entry (12 matrix entries per thread at 54 rows).  The
// entry's tables -- N, gn, A, B at the side points, the side functions and fields -- are at most 18 KB of LDS, stored
// [side point][basis function]: in the Jacobian sweep neighbouring lanes hold neighbouring columns b, so their 8-byte
// reads of N_b, gn_b, A_b, B_b at one point fall on consecutive doubles (no bank conflict within a half-wave; with
// [basis function][side point] the lanes would stride by the number of side points, 2- or 4-way conflicts at 2 and 4
// points), while N_a of the row is the same address for most lanes (a broadcast).  The wave limit, not the LDS,
// bounds the workgroups per CU.  The surface is O(N^{d-1}) against the volume's O(N^d): atomics
// and the CRS column search, as the other boundary kernels.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "launch.hpp"
#include "side_geometry.hpp"

namespace mha {
namespace {

constexpr int kHbThreads = 256, kHbMaxCard = 27, kHbMaxQ = 16, kHbFuncs = 10;

// doubles of one entry's LDS: N, gn, A, B | u | per point: Ji, then w, n, the ten functions, Br, Bi | rows (ints)
__host__ __device__ constexpr int hb_point_doubles(int dim) { return 1 + dim + kHbFuncs + 2; }
__host__ __device__ inline int hb_entry_doubles(int dim, int card, int nqs) {
  const int n = 2 * card;
  return (4 * card * nqs + n + nqs * (dim * dim + hb_point_doubles(dim)) + (n + 1) / 2 + 1) & ~1;
}

template <int DIM, int TPE>
__global__ __launch_bounds__(kHbThreads) void helmholtz_boundary_kernel(BlockDev b, SideTablesDev st, BoundaryDev bd,
                                                                        HelmholtzBoundaryDev hb, TimeDev tm, ElemOut out) {
  constexpr int NN = 1 << DIM, PT = hb_point_doubles(DIM), NG = kHbThreads / TPE;
  constexpr int PF = 1 + DIM, PB = PF + kHbFuncs;  // first function, first bracket inside a point's record
  extern __shared__ double smem[];
  const int n = b.n, card = n / 2, nqs = st.nqs, cq = card * nqs;
  const int grp = threadIdx.x / TPE, t = threadIdx.x % TPE;
  double *s_N = smem + grp * hb_entry_doubles(DIM, card, nqs);
  double *s_gn = s_N + cq, *s_A = s_gn + cq, *s_B = s_A + cq;
  double *s_u = s_B + cq;
  double *s_Ji = s_u + n, *s_pt = s_Ji + nqs * DIM * DIM;
  int *s_row = reinterpret_cast<int *>(s_pt + nqs * PT);
  const int k = blockIdx.x * NG + grp;
  const bool active = k < bd.num;  // inactive groups still take part in the block barriers
  const int e = active ? bd.elem[k] : 0, s = active ? bd.side[k] : 0;
  const int32_t *L = b.lids + (size_t)e * b.n;

  // A. side geometry and the ten functions (thread = (side point, function): ONE inlined copy of the deck-string
  // interpreter); gather + seeding value (thread = (variable, dof))
  if (active) {
    for (int idx = t; idx < nqs * kHbFuncs; idx += TPE) {
      const int q = idx / kHbFuncs, kf = idx - q * kHbFuncs;
      double Ji[DIM * DIM], nrm[DIM], w, x[DIM];
      side_point<DIM>(b.nodes + (size_t)e * NN * DIM, st, s, q, Ji, nrm, w, x);
      double *p = s_pt + q * PT;
      if (kf == 0) {
        p[0] = w;
#pragma unroll
        for (int d = 0; d < DIM; ++d) p[1 + d] = nrm[d];
#pragma unroll
        for (int i = 0; i < DIM * DIM; ++i) s_Ji[q * DIM * DIM + i] = Ji[i];
      }
      // c2r_z, c2i_z are not read in 2-D (helmholtz.cpp:352-355)
      p[PF + kf] = (DIM == 2 && (kf == 4 || kf == 5)) ? 0.0 : eval_func<DIM, true>(hb.f[kf], k, q, nqs, x, nrm);
    }
    for (int f = t; f < n; f += TPE) {
      const int row = L[b.offsets[f]];
      s_row[f] = row;
      s_u[f] = stage_value(tm, row);
    }
  }
  __syncthreads();
  // B. N, grad N . n and the c2-weighted normal derivatives A, B of every basis function at the side points
  // (physical gradient = J^{-T} grad_ref)
  if (active) {
    for (int idx = t; idx < cq; idx += TPE) {
      const int q = idx / card, a = idx - q * card;  // LDS image [side point][basis function]
      const double *p = s_pt + q * PT;
      const double *gr = st.grad + ((size_t)(s * card + a) * nqs + q) * DIM;
      double gn = 0.0, A = 0.0, B = 0.0;
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        double pg = 0.0;
#pragma unroll
        for (int c = 0; c < DIM; ++c) pg += s_Ji[q * DIM * DIM + c * DIM + d] * gr[c];
        const double pn = pg * p[1 + d];
        gn += pn;
        A += p[PF + 2 * d] * pn;
        B += p[PF + 2 * d + 1] * pn;
      }
      s_N[idx] = st.basis[(size_t)(s * card + a) * nqs + q];
      s_gn[idx] = gn;
      s_A[idx] = A;
      s_B[idx] = B;
    }
  }
  __syncthreads();
  // C. the side fields and the two brackets Br, Bi (thread = side point)
  if (active) {
    for (int q = t; q < nqs; q += TPE) {
      double *p = s_pt + q * PT;
      double ur = 0.0, ui = 0.0, durdn = 0.0, duidn = 0.0, c2durdn = 0.0, c2duidn = 0.0;
      for (int a = 0; a < card; ++a) {
        const double vr = s_u[a], vi = s_u[card + a];
        const double N = s_N[q * card + a], gn = s_gn[q * card + a], A = s_A[q * card + a], B = s_B[q * card + a];
        ur += vr * N;
        ui += vi * N;
        durdn += vr * gn;
        duidn += vi * gn;
        c2durdn += vr * A - vi * B;
        c2duidn += vi * A + vr * B;
      }
      const double ar = p[PF + 6], ai = p[PF + 7], sr = p[PF + 8], si = p[PF + 9];
      p[PB] = ar * (ur + ui) - ai * (ui - ur) + (durdn + duidn) - (sr + si) - (c2durdn + c2duidn);
      p[PB + 1] = ar * (ui - ur) + ai * (ur + ui) + (duidn - durdn) - (si - sr) - (c2duidn - c2durdn);
    }
  }
  __syncthreads();
  if (!active) return;
  // D. residual rows (thread = (variable, dof))
  for (int f = t; f < n; f += TPE) {
    const int v = f / card, a = f - v * card;
    double r = 0.0;
    for (int q = 0; q < nqs; ++q) {
      const double *p = s_pt + q * PT;
      r += p[0] * s_N[q * card + a] * p[PB + v];
    }
    const int row = s_row[f];
    if (out.res && !(b.fixed && b.fixed[row])) unsafeAtomicAdd(out.res + row, -r);
  }
  // E. Jacobian entries: threads sweep the n x n block
  if (out.compute_jacobian && out.crs_vals) {
    for (int idx = t; idx < n * n; idx += TPE) {
      const int i = idx / n, j = idx - i * n;
      const int vr = i / card, a = i - vr * card, vc = j / card, bb = j - vc * card;
      const int ri = s_row[i];
      if (b.fixed && b.fixed[ri]) continue;
      // C = cN N_b + sg (gn_b - A_b) + sB B_b
      const bool same = vr == vc;
      const double sg = (vr == 1 && vc == 0) ? -1.0 : 1.0;
      const double sB = same ? -1.0 : (vr == 0 ? 1.0 : -1.0);
      double v = 0.0;
      for (int q = 0; q < nqs; ++q) {
        const double *p = s_pt + q * PT;
        const double ar = p[PF + 6], ai = p[PF + 7];
        const double cN = same ? ar + ai : (vr == 0 ? ar - ai : ai - ar);
        const int bq = q * card + bb;
        v += p[0] * s_N[q * card + a] * (cN * s_N[bq] + sg * (s_gn[bq] - s_A[bq]) + sB * s_B[bq]);
      }
      const int pos = find_col(b.colind, b.rowptr[ri], b.rowptr[ri + 1], s_row[j]);
      if (pos >= 0) unsafeAtomicAdd(out.crs_vals + pos, tm.alpha_u * v);
    }
  }
}

}  // namespace

bool helmholtz_boundary_supported(int dim, int n, int nqs) {
  return (dim == 2 || dim == 3) && n > 0 && n % 2 == 0 && n / 2 <= kHbMaxCard && nqs > 0 && nqs <= kHbMaxQ;
}

void launch_helmholtz_boundary(const BlockDev &b, const SideTablesDev &st, const BoundaryDev &bd,
                               const HelmholtzBoundaryDev &hb, const TimeDev &tm, const ElemOut &out, hipStream_t stream) {
  if (bd.num <= 0) return;
  MHA_REQUIRE(bd.bc_type == MHA_BC_NEUMANN, MHA_ERR_INVALID, "helmholtz: only MHA_BC_NEUMANN (Robin) groups are built");
  MHA_REQUIRE(helmholtz_boundary_supported(b.dim, b.n, st.nqs), MHA_ERR_INVALID,
              "helmholtz boundary kernel: ureal and uimag of one order with at most "
                  << kHbMaxCard << " dofs each and " << kHbMaxQ << " side points (got " << b.n << " dofs per element, "
                  << st.nqs << " side points)");
  const int card = b.n / 2;
  const bool wave_per_entry = b.n <= 32;
  const int per_wg = wave_per_entry ? kHbThreads / 64 : 1;
  const size_t lds = sizeof(double) * per_wg * hb_entry_doubles(b.dim, card, st.nqs);
  const int grid = (bd.num + per_wg - 1) / per_wg;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kHbThreads), lds, stream, b, st, bd, hb, tm, out);
    MHA_HIP(hipGetLastError());
  };
  if (b.dim == 2) {
    if (wave_per_entry) go(helmholtz_boundary_kernel<2, 64>);
    else go(helmholtz_boundary_kernel<2, kHbThreads>);
  } else {
    if (wave_per_entry) go(helmholtz_boundary_kernel<3, 64>);
    else go(helmholtz_boundary_kernel<3, kHbThreads>);
  }
}

}  // namespace mha
