// linearelasticity_stress.hip -- the stress output of the two elasticity blocks.
//
// reference: linearelasticity::getDerivedValues (src/physics/linearelasticity.cpp:1301-1360) with computeStress
// (:913-1099, onside = false): the stress tensor at the volume integration points from the solution as given, then
// "VM stress" and "MAG stress" (:1326-1354).  One launch for all elements of the block, one thread per
// (element, integration point):
//   geometry   J = sum_v x_v grad N_v, J^-1 and x(q), as kernels/var_views.hip forms them (HGRADtransformGRAD);
//   fields     grad u_d = sum_f u(d, f) J^-T grad_ref phi_f, streamed over the dofs -- per thread DIM^2 + 1 accumulators
//              and one physical gradient, never an array of the element's dofs, so the Q2 hexahedron (27 dofs x 3 or 4
//              variables) needs no more registers than the Q1 one;
//   e          sum_f u(e, f) phi_f on the coupled block, with e's own basis;
//   lambda, mu eval_func: constants, ip arrays, closed forms, deck strings in the coordinates at the workset time;
//   stress     le_stress (linearelasticity_stress.hpp), the function the coupled block's point function calls.
// No LDS, no atomics; every output is a plain vector store of the thread's own (element, point) entry.  A thread reads
// card * (DIM + 1) table entries that its 63 neighbours in the wavefront share through the cache (consecutive threads are
// consecutive points of one element) and writes 2 + DIM^2 doubles: the launch is bound by its stores.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_math.hpp"
#include "launch.hpp"
#include "linearelasticity_stress.hpp"

namespace mha {
namespace {

constexpr int kStressThreads = 256;

template <int DIM, bool TE, bool EXPR>
__global__ __launch_bounds__(kStressThreads) void linearelasticity_stress_kernel(BlockDev b, LeStressDev a) {
  constexpr int NN = 1 << DIM;
  const int nq = b.nq;
  const int64_t total = (int64_t)b.nelem * nq;
  const int64_t idx = (int64_t)blockIdx.x * kStressThreads + threadIdx.x;
  if (idx >= total) return;
  const int e = (int)(idx / nq), q = (int)(idx - (int64_t)e * nq);
  const double *xn = b.nodes + (size_t)e * NN * DIM;
  double J[DIM * DIM], Ji[DIM * DIM], det, x[DIM];
#pragma unroll
  for (int r = 0; r < DIM; ++r) {
    x[r] = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) J[r * DIM + c] = 0.0;
  }
  for (int v = 0; v < NN; ++v) {
    const double nv = b.nodeval[v * nq + q];
#pragma unroll
    for (int r = 0; r < DIM; ++r) {
      const double xr = xn[v * DIM + r];
      x[r] += xr * nv;
#pragma unroll
      for (int c = 0; c < DIM; ++c) J[r * DIM + c] += xr * b.nodegrad[((size_t)v * nq + q) * DIM + c];
    }
  }
  invert<DIM>(J, Ji, det);
  const int32_t *L = b.lids + (size_t)e * b.n;
  const int8_t *sg = a.orient ? a.orient + (size_t)e * b.n : nullptr;
  double gu[DIM * DIM];
#pragma unroll
  for (int i = 0; i < DIM * DIM; ++i) gu[i] = 0.0;
  const int card = a.card_u;
  for (int f = 0; f < card; ++f) {
    const double *gr = a.grad_u + ((size_t)f * nq + q) * DIM;
    double g[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      double sum = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; ++c) sum += Ji[c * DIM + d] * gr[c];
      g[d] = sum;
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      const int k = d * card + f;  // the displacements are the block's first DIM variables
      double ud = a.u[L[b.offsets[k]]];
      if (sg) ud *= (double)sg[k];
#pragma unroll
      for (int j = 0; j < DIM; ++j) gu[d * DIM + j] += ud * g[j];
    }
  }
  double T = 0.0;
  if constexpr (TE) {
    for (int f = 0; f < a.card_e; ++f) {
      const int k = a.off_e + f;
      double ue = a.u[L[b.offsets[k]]];
      if (sg) ue *= (double)sg[k];
      T += ue * a.val_e[(size_t)f * nq + q];
    }
  }
  const double lam = eval_func<DIM, EXPR>(a.lam, e, q, nq, x), mu = eval_func<DIM, EXPR>(a.mu, e, q, nq, x);
  double sig[DIM * DIM];
  le_stress<DIM, double>(gu, TE ? &T : nullptr, lam, mu, a.plane_stress != 0, a.alpha_T, a.T_ambient, sig);
  if (a.stress) {
#pragma unroll
    for (int i = 0; i < DIM * DIM; ++i) a.stress[(size_t)idx * (DIM * DIM) + i] = sig[i];
  }
  double vm, mag;
  le_derived<DIM>(sig, vm, mag);
  if (a.vm) a.vm[idx] = vm;
  if (a.mag) a.mag[idx] = mag;
}

}  // namespace

void launch_linearelasticity_stress(const BlockDev &b, const LeStressDev &a, hipStream_t stream) {
  if (b.nelem <= 0) return;
  MHA_REQUIRE(b.dim == 2 || b.dim == 3, MHA_ERR_INVALID, "the stress output is built in 2-D and 3-D");
  MHA_REQUIRE(a.u && a.grad_u && a.card_u > 0 && b.dim * a.card_u + a.card_e <= b.n &&
                  (a.card_e == 0 || (a.val_e && a.off_e >= 0 && a.off_e + a.card_e <= b.n)),
              MHA_ERR_INVALID, "stress output: the variable tables do not match the block");
  MHA_REQUIRE(!uses_fields(a.lam) && !uses_fields(a.mu), MHA_ERR_INVALID,
              "stress output: 'lambda' and 'mu' that read solution fields are not built");
  const int64_t total = (int64_t)b.nelem * b.nq;
  const int64_t grid = (total + kStressThreads - 1) / kStressThreads;
  MHA_REQUIRE(grid <= 0x7fffffff, MHA_ERR_INVALID, "stress output: too many integration points for one launch");
  const bool te = a.card_e > 0, expr = has_expression(a.lam) || has_expression(a.mu);
  auto go = [&](auto kern) {
    require_modest_scratch(kern, "stress output");
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kStressThreads), 0, stream, b, a);
    MHA_HIP(hipGetLastError());
  };
  auto pick = [&](auto dim) {
    constexpr int D = decltype(dim)::value;
    if (te) { if (expr) go(linearelasticity_stress_kernel<D, true, true>); else go(linearelasticity_stress_kernel<D, true, false>); }
    else { if (expr) go(linearelasticity_stress_kernel<D, false, true>); else go(linearelasticity_stress_kernel<D, false, false>); }
  };
  if (b.dim == 2) pick(std::integral_constant<int, 2>());
  else pick(std::integral_constant<int, 3>());
}

}  // namespace mha
