// stream_rows.hpp -- how the one-thread-per-element steps (porous_hybrid_fused.hip, porous_wg_fused.hip) store their
// outputs: a wavefront's 64 elements own one contiguous piece of each output; the lanes put their rows into the
// wavefront's LDS buffer (row stride odd: conflict-free 8-byte writes) and the wavefront streams the piece out 16 bytes
// per lane, consecutive lanes at consecutive addresses.
#pragma once
#include <hip/hip_runtime.h>

namespace mha {
namespace {

// orders a wavefront's LDS writes before its later LDS reads (the buffer is private to the wavefront)
__device__ __forceinline__ void pmh_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// rows of W doubles, one per lane, staged at stride W | 1 in sb -> out[0 .. cnt W) in 16-byte pieces (out 16-byte aligned)
template <int W>
__device__ __forceinline__ void pmh_stream_rows(double *out, const double *sb, int lane, int cnt) {
  constexpr int WP = W | 1;
  const int total = cnt * W;
  for (int i = 2 * lane; i + 1 < total; i += 128) {
    const int r0 = i / W, r1 = (i + 1) / W;
    double2 v;
    v.x = sb[r0 * WP + (i - r0 * W)];
    v.y = sb[r1 * WP + (i + 1 - r1 * W)];
    *reinterpret_cast<double2 *>(out + i) = v;
  }
  if ((total & 1) && lane == 0) {
    const int i = total - 1, r0 = i / W;
    out[i] = sb[r0 * WP + (i - r0 * W)];
  }
}

}  // namespace
}  // namespace mha
