// linearelasticity_stress.hpp -- linearelasticity::computeStress at one point, stated once.
//
// reference: src/physics/linearelasticity.cpp:913-1099 (onside = false).  Read by the point function of the coupled
// block (linearelasticity_thermal_point, T = Dual) and by the stress output (kernels/linearelasticity_stress.hip,
// T = double).
#pragma once
#include "dual.hpp"

namespace mha {

// gu[d * DIM + j] = d_j u_d; e: the temperature at the point, or null on a block without the variable "e".
//   sigma = lambda tr(grad u) I + mu (grad u + grad u^T)                                          (:1014-1023, 1059-1073)
//   incplanestress (2-D): the normal stresses are 4 mu d_x dx + 2 mu d_y dy and its mirror: lambda = 2 mu       (:990-1000)
//   with e: every normal stress gets -alpha_T (e - T_ambient) c, c = 3 lambda + 2 mu (:1024-1034, 1074-1084), and
//   c = 5 mu under incplanestress (:1001-1011; the reference's value, not 3 (2 mu) + 2 mu)
template <int DIM, class T>
__host__ __device__ __forceinline__ void le_stress(const T *gu, const T *e, double lam, double mu, bool plane_stress,
                                                   double alpha_T, double T_ambient, T *sig) {
  const bool ps = DIM == 2 && plane_stress;
  const double l = ps ? 2.0 * mu : lam;
  T tr = gu[0];
#pragma unroll
  for (int d = 1; d < DIM; ++d) tr = tr + gu[d * DIM + d];
  const T ltr = tr * l;
#pragma unroll
  for (int d = 0; d < DIM; ++d)
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
      sig[d * DIM + j] = (gu[d * DIM + j] + gu[j * DIM + d]) * mu;
      if (j == d) sig[d * DIM + j] = sig[d * DIM + j] + ltr;
    }
  if (e) {
    const double c = ps ? 5.0 * mu : 3.0 * lam + 2.0 * mu;
    const T th = (*e - T_ambient) * (alpha_T * c);
#pragma unroll
    for (int d = 0; d < DIM; ++d) sig[d * DIM + d] = sig[d * DIM + d] - th;
  }
}

// getDerivedValues (:1326-1354): "VM stress" and "MAG stress" (the normal components only) of a stress tensor
template <int DIM>
__host__ __device__ __forceinline__ void le_derived(const double *s, double &vm, double &mag) {
  if constexpr (DIM == 2) {
    const double sxx = s[0], syy = s[3], sxy = s[1];
    vm = sqrt(sxx * sxx - sxx * syy + syy * syy + 3.0 * sxy * sxy);
    mag = sqrt(sxx * sxx + syy * syy);
  } else {
    const double sxx = s[0], syy = s[4], szz = s[8], sxy = s[1], syz = s[5], szx = s[6];
    vm = sqrt(0.5 * ((sxx - syy) * (sxx - syy) + (syy - szz) * (syy - szz) + (szz - sxx) * (szz - sxx)) +
              3.0 * (sxy * sxy + syz * syz + szx * szx));
    mag = sqrt(sxx * sxx + syy * syy + szz * szz);
  }
}

}  // namespace mha
