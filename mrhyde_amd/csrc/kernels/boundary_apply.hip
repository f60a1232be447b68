// boundary_apply.hip -- y += A_b x, y += A_b^T x and d += diag(A_b) for one boundary group, A_b the matrix that the
// group's assembly kernel (thermal_boundary.hip, linearelasticity_boundary.hip, helmholtz_boundary.hip,
// swhdg_boundary.hip) adds into the CRS values: same sign, same alpha_u seeding, zero rows where the mesh marks a row
// fixed.  Neither A_b nor an entry matrix is formed and the CRS graph is not read.  The reference has no counterpart: its
// boundary Jacobian exists as scattered CRS entries only (the boundary loop of assembleJacRes, assemblyManager.cpp:2518-2638).
//
// The entry matrix is sum_q S_a(q)^T C(q) S_b(q) with the module's point form C(q) (boundary_forms.hpp), so the product
// is sum-factorised per (element, side) entry:
//   A. side geometry and the form's functions at the side points (thread = (point, function): one inlined copy of the
//      deck-string interpreter); gather of x (and of u where C depends on it)
//   B. S: value and physical gradient (J^{-T} grad_ref) of every basis function at the side points, into LDS
//   C. the form's derived coefficients; trial fields F(q) = sum_b x_b S_b(q) per (variable, slot)
//   D. forward     G(q)   = apply(F(q))                       (thread = point)
//      transposed  G_c(q) = apply(e_c) . F(q)                 (thread = (point, column): column c of C, dotted with F)
//      diagonal    the columns apply(e_c), rows of c's own variable kept
//   E. y[row_a] += sum_q S_a(q) . G(q)  /  d[row_a] += sum_q S_a(q)^T C_vv(q) S_a(q):  one atomic per row and entry --
//      side entries share rows at edges and corners
// O(n nqs) work per entry in place of the assembly's O(n^2 nqs), n atomics in place of n^2 and no column search.
// Work split as the assembly kernels: up to 32 rows one wavefront takes an entry and a workgroup four; above (helmholtz
// 3-D Q2: 54 rows, linearelasticity 3-D Q2: 81) -- or where four entries' tables would not fit 64 KB of LDS -- the whole
// workgroup takes one.  The LDS tables are [side point][slot][basis function]: in C and E neighbouring threads hold
// neighbouring basis functions, so their 8-byte reads at one point fall on consecutive doubles (the reasoning of
// helmholtz_boundary.hip's header).  Forward: fixed rows of y are not touched; transposed: x is read as zero on fixed
// rows; diagonal: fixed rows get nothing.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "boundary_forms.hpp"
#include "device_math.hpp"
#include "launch.hpp"
#include "side_geometry.hpp"

namespace mha {
namespace {

constexpr int kBaThreads = 256, kBaMaxCard = 27, kBaMaxQ = 16, kBaMaxLds = 64 * 1024;

template <class FORM>
__host__ __device__ constexpr int ba_point_doubles(int dim) { return 1 + dim + FORM::NC; }
// per point: the larger of F and G (products) and the kept columns [P][NS] (diagonal)
template <class FORM>
__host__ __device__ constexpr int ba_work_doubles(int dim) {
  return FORM::NV(dim) * FORM::NS(dim) * (FORM::NS(dim) > 2 ? FORM::NS(dim) : 2);
}
// doubles of one entry's LDS: S | x | u | per point: Ji, the point record, the work area | rows (ints)
template <class FORM>
__host__ __device__ inline int ba_entry_doubles(int dim, int card, int nqs) {
  const int n = FORM::NV(dim) * card;
  return (FORM::NS(dim) * card * nqs + n + (FORM::kNeedsU ? n : 0) +
          nqs * (dim * dim + ba_point_doubles<FORM>(dim) + ba_work_doubles<FORM>(dim)) + (n + 1) / 2 + 1) & ~1;
}

// MODE 1: y += A_b x, 2: y += A_b^T x, 3: y += diag(A_b)
template <class FORM, int DIM, int TPE, int MODE>
__global__ __launch_bounds__(kBaThreads) void boundary_apply_kernel(BlockDev b, SideTablesDev st, BoundaryDev bd,
                                                                    typename FORM::Dev fd, TimeDev tm, const double *x,
                                                                    double *y) {
  constexpr int NN = 1 << DIM, NV = FORM::NV(DIM), NS = FORM::NS(DIM), P = NV * NS, NG = kBaThreads / TPE;
  constexpr int PT = ba_point_doubles<FORM>(DIM), PW = ba_work_doubles<FORM>(DIM), PC = 1 + DIM;  // first coefficient
  extern __shared__ double smem[];
  const int n = b.n, card = n / NV, nqs = st.nqs;
  const int grp = threadIdx.x / TPE, t = threadIdx.x % TPE;
  double *s_S = smem + grp * ba_entry_doubles<FORM>(DIM, card, nqs);
  double *s_x = s_S + NS * card * nqs;
  double *s_u = s_x + n;
  double *s_Ji = s_u + (FORM::kNeedsU ? n : 0), *s_pt = s_Ji + nqs * DIM * DIM;
  double *s_F = s_pt + nqs * PT, *s_G = s_F + nqs * P;  // MODE 3: s_F is the kept columns [point][column][slot]
  int *s_row = reinterpret_cast<int *>(s_F + nqs * PW);
  const int k = blockIdx.x * NG + grp;
  const bool active = k < bd.num;  // inactive groups still take part in the block barriers
  const int e = active ? bd.elem[k] : 0, s = active ? bd.side[k] : 0;
  const int32_t *L = b.lids + (size_t)e * n;

  // A.
  if (active) {
    for (int idx = t; idx < nqs * FORM::NF; idx += TPE) {
      const int q = idx / FORM::NF, kf = idx - q * FORM::NF;
      double Ji[DIM * DIM], nrm[DIM], w, xp[DIM];
      side_point<DIM>(b.nodes + (size_t)e * NN * DIM, st, s, q, Ji, nrm, w, xp);
      double *p = s_pt + q * PT;
      if (kf == 0) {
        p[0] = w;
#pragma unroll
        for (int d = 0; d < DIM; ++d) p[1 + d] = nrm[d];
#pragma unroll
        for (int i = 0; i < DIM * DIM; ++i) s_Ji[q * DIM * DIM + i] = Ji[i];
      }
      p[PC + kf] = eval_func<DIM, true>(FORM::func(fd, kf), k, q, nqs, xp, nrm);
    }
    for (int f = t; f < n; f += TPE) {
      const int row = L[b.offsets[f]];
      s_row[f] = row;
      if (MODE == 1) s_x[f] = x[row];
      if (MODE == 2) s_x[f] = (b.fixed && b.fixed[row]) ? 0.0 : x[row];
      if (FORM::kNeedsU) s_u[f] = stage_value(tm, row);
    }
  }
  __syncthreads();
  // B.
  if (active) {
    for (int idx = t; idx < card * nqs; idx += TPE) {
      const int q = idx / card, a = idx - q * card;
      s_S[(q * NS) * card + a] = st.basis[(size_t)(s * card + a) * nqs + q];
      if (NS > 1) {
        const double *gr = st.grad + ((size_t)(s * card + a) * nqs + q) * DIM;
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          double pg = 0.0;
#pragma unroll
          for (int c = 0; c < DIM; ++c) pg += s_Ji[q * DIM * DIM + c * DIM + d] * gr[c];
          s_S[(q * NS + 1 + d) * card + a] = pg;
        }
      }
    }
  }
  __syncthreads();
  // C.
  if (active) {
    for (int q = t; q < nqs; q += TPE) FORM::template finish<DIM>(fd, s_pt, PT, nqs, q, s_u, s_S, card);
    if (MODE != 3) {
      for (int idx = t; idx < nqs * P; idx += TPE) {
        const int q = idx / P, c = idx - q * P, v = c / NS, sl = c - v * NS;
        const double *S = s_S + (q * NS + sl) * card, *xv = s_x + v * card;
        double sum = 0.0;
        for (int a = 0; a < card; ++a) sum += xv[a] * S[a];
        s_F[idx] = sum;
      }
    }
  }
  __syncthreads();
  // D.
  if (active) {
    if (MODE == 1) {
      for (int q = t; q < nqs; q += TPE) {
        double F[P], G[P];
#pragma unroll
        for (int i = 0; i < P; ++i) F[i] = s_F[q * P + i];
        FORM::template apply<DIM>(fd, s_pt + q * PT, tm.alpha_u, F, G);
#pragma unroll
        for (int i = 0; i < P; ++i) s_G[q * P + i] = G[i];
      }
    } else {
      for (int idx = t; idx < nqs * P; idx += TPE) {
        const int q = idx / P, c = idx - q * P;
        double E[P], col[P];
#pragma unroll
        for (int i = 0; i < P; ++i) E[i] = (i == c) ? 1.0 : 0.0;
        FORM::template apply<DIM>(fd, s_pt + q * PT, tm.alpha_u, E, col);
        if (MODE == 2) {
          double sum = 0.0;
#pragma unroll
          for (int i = 0; i < P; ++i) sum += col[i] * s_F[q * P + i];
          s_G[idx] = sum;
        } else {
          const int v = c / NS;
#pragma unroll
          for (int i = 0; i < P; ++i)
            if (i / NS == v) s_F[idx * NS + i % NS] = col[i];  // C[(v, i % NS)][c]
        }
      }
    }
  }
  __syncthreads();
  if (!active) return;
  // E.
  for (int f = t; f < n; f += TPE) {
    const int v = f / card, a = f - v * card, row = s_row[f];
    if (MODE != 2 && b.fixed && b.fixed[row]) continue;
    double r = 0.0;
    for (int q = 0; q < nqs; ++q) {
      const double *S = s_S + (q * NS) * card + a;
      if (MODE != 3) {
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) r += S[sl * card] * s_G[q * P + v * NS + sl];
      } else {
#pragma unroll
        for (int tc = 0; tc < NS; ++tc) {
          double cs = 0.0;  // sum over the row slots of S_a[slot] C[(v, slot)][(v, tc)]
#pragma unroll
          for (int sl = 0; sl < NS; ++sl) cs += S[sl * card] * s_F[(q * P + v * NS + tc) * NS + sl];
          r += cs * S[tc * card];
        }
      }
    }
    unsafeAtomicAdd(y + row, r);
  }
}

template <class FORM>
void boundary_apply(const char *module, const BlockDev &b, const SideTablesDev &st, const BoundaryDev &bd,
                    const typename FORM::Dev &fd, const TimeDev &tm, const BoundaryApplyRequest &rq, hipStream_t stream) {
  if (bd.num <= 0 || !FORM::has_jacobian(bd.bc_type)) return;  // a group without a Jacobian: no launch
  const int nv = FORM::NV(b.dim);
  MHA_REQUIRE((b.dim == 2 || b.dim == 3) && b.n > 0 && b.n % nv == 0 && b.n / nv <= kBaMaxCard && st.nqs > 0 &&
                  st.nqs <= kBaMaxQ,
              MHA_ERR_INVALID,
              module << " boundary product kernel: " << nv << " equal-order variables with at most " << kBaMaxCard
                     << " dofs each and " << kBaMaxQ << " side points (got " << b.n << " dofs per element, " << st.nqs
                     << " side points)");
  MHA_REQUIRE(rq.mode >= 1 && rq.mode <= 3 && rq.y && (rq.mode == 3 || rq.x), MHA_ERR_INVALID,
              "boundary product: bad request (mode " << rq.mode << ")");
  const int card = b.n / nv;
  const size_t entry = sizeof(double) * ba_entry_doubles<FORM>(b.dim, card, st.nqs);
  MHA_REQUIRE(entry <= (size_t)kBaMaxLds, MHA_ERR_INVALID,
              module << " boundary product kernel: an entry's tables take " << entry << " bytes of LDS, above " << kBaMaxLds);
  const bool wave_per_entry = b.n <= 32 && entry * (kBaThreads / 64) <= (size_t)kBaMaxLds;
  const int per_wg = wave_per_entry ? kBaThreads / 64 : 1;
  const size_t lds = entry * per_wg;
  if (rq.check_only) return;
  if (rq.lds_bytes && *rq.lds_bytes < lds) *rq.lds_bytes = lds;
  const int grid = (bd.num + per_wg - 1) / per_wg;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kBaThreads), lds, stream, b, st, bd, fd, tm, rq.x, rq.y);
    MHA_HIP(hipGetLastError());
  };
  auto by_mode = [&](auto dim_c, auto tpe_c) {
    constexpr int D = decltype(dim_c)::value, T = decltype(tpe_c)::value;
    if (rq.mode == 1) go(boundary_apply_kernel<FORM, D, T, 1>);
    else if (rq.mode == 2) go(boundary_apply_kernel<FORM, D, T, 2>);
    else go(boundary_apply_kernel<FORM, D, T, 3>);
  };
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using W = std::integral_constant<int, 64>;
  using G = std::integral_constant<int, kBaThreads>;
  if (b.dim == 2) {
    if (wave_per_entry) by_mode(I2{}, W{});
    else by_mode(I2{}, G{});
  } else if constexpr (FORM::kHas3D) {
    if (wave_per_entry) by_mode(I3{}, W{});
    else by_mode(I3{}, G{});
  } else {
    throw Error(MHA_ERR_INVALID, std::string(module) + " boundary product kernel: 2-D only");
  }
}

}  // namespace

void launch_boundary_apply(const BlockDev &b, const SideTablesDev &st, const BoundaryDev &bd, const TimeDev &tm,
                           const BoundaryApplyRequest &rq, hipStream_t stream) {
  boundary_apply<ThermalSideForm>("thermal", b, st, bd, bd, tm, rq, stream);
}
void launch_boundary_apply(const BlockDev &b, const SideTablesDev &st, const BoundaryDev &bd, const LeBoundaryDev &le,
                           const TimeDev &tm, const BoundaryApplyRequest &rq, hipStream_t stream) {
  if (le.disp_card > 0) return;  // the coupled block takes traction only: no Jacobian
  boundary_apply<LinearElasticitySideForm>("linearelasticity", b, st, bd, le, tm, rq, stream);
}
void launch_boundary_apply(const BlockDev &b, const SideTablesDev &st, const BoundaryDev &bd,
                           const HelmholtzBoundaryDev &hb, const TimeDev &tm, const BoundaryApplyRequest &rq,
                           hipStream_t stream) {
  boundary_apply<HelmholtzSideForm>("helmholtz", b, st, bd, hb, tm, rq, stream);
}
void launch_boundary_apply(const BlockDev &b, const SideTablesDev &st, const BoundaryDev &bd, const SwhBoundaryDev &sw,
                           const TimeDev &tm, const BoundaryApplyRequest &rq, hipStream_t stream) {
  boundary_apply<SwhSideForm>("shallowwaterHybridized", b, st, bd, sw, tm, rq, stream);
}

}  // namespace mha
