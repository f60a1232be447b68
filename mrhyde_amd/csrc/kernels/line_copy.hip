// line_copy.hip -- the database modes' copy of representative CRS entries, in whole aligned lines (copy_plan.hpp).
//
// One wavefront per work item: a span of kCopySpanLines 128-byte lines of vals, stored 1 KB per instruction (16 bytes
// per lane, nontemporal: the lines are not read again before they leave the L2).  Every line is written once, whole,
// by one instruction -- a run boundary inside a line no longer splits it between two wavefronts, and no lane idles
// except past nnz.  Each lane takes the offset of the last segment that starts at or before each of its two entries:
// the item's segment records are loaded wave-uniform (scalar loads), kCopySegRegs at a time, and compared per lane.
// The sources are the representatives' entries (a few MB, L2-resident) at any entry offset: 8-byte loads, all of a
// span's issued before its first store.  SEP: the sources sit in a buffer of their own (the thermal geometry database's
// kept representatives, copy_plan.hpp) and vals is written only; otherwise they are entries of vals itself.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../common.hpp"
#include "../copy_plan.hpp"

namespace mha {

namespace {

template <int U, int R, bool SEP>
__global__ __launch_bounds__(256) void line_copy_kernel(const int4 *__restrict__ items, int nitems,
                                                        const int2 *__restrict__ seg, int nnz,
                                                        const double *sep_src, double *vals) {
  const double *src = SEP ? sep_src : vals;
  const int lane = threadIdx.x & 63;
  const int wave0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 256 + threadIdx.x) >> 6), nwaves = (gridDim.x * 256) >> 6;
  for (int w = wave0; w < nitems; w += nwaves) {
    const int4 it = items[w];  // wave-uniform
    const int s0 = it.x * kCopyLineEntries, first = it.y, nseg = it.z;
    int off0[U], off1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) off0[u] = off1[u] = 0;
    for (int j = 0; j < nseg; j += R) {  // one pass almost always: a span meets few segments
      // (records past the item's last segment start at or after the span's end -- the host pads the list with R
      // sentinels -- so they never match: no per-record bound)
      const int2 *sp = seg + first + j;
      int2 sr[R];
#pragma unroll
      for (int k = 0; k < R; ++k) sr[k] = sp[k];
#pragma unroll
      for (int k = 0; k < R; ++k) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int e = s0 + u * kCopyWaveEntries + 2 * lane;
          off0[u] = e >= sr[k].x ? sr[k].y : off0[u];
          off1[u] = e + 1 >= sr[k].x ? sr[k].y : off1[u];
        }
      }
    }
    double x0[U], x1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // lanes past nnz load an entry that exists and store nothing
      const int e = s0 + u * kCopyWaveEntries + 2 * lane;
      x0[u] = src[e < nnz ? e + off0[u] : 0];
      x1[u] = src[e + 1 < nnz ? e + 1 + off1[u] : 0];
    }
    typedef double v2d_t __attribute__((ext_vector_type(2)));
    if (s0 + kCopySpanEntries <= nnz) {  // wave-uniform: every span but the last
#pragma unroll
      for (int u = 0; u < U; ++u) {
        v2d_t v = {x0[u], x1[u]};
        __builtin_nontemporal_store(v, reinterpret_cast<v2d_t *>(vals + s0 + u * kCopyWaveEntries + 2 * lane));
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = s0 + u * kCopyWaveEntries + 2 * lane;
        if (e + 1 < nnz) {
          v2d_t v = {x0[u], x1[u]};
          __builtin_nontemporal_store(v, reinterpret_cast<v2d_t *>(vals + e));
        } else if (e < nnz) {
          __builtin_nontemporal_store(x0[u], vals + e);
        }
      }
    }
  }
}

}  // namespace

void launch_line_copy(const int32_t *items, int nitems, const int32_t *seg, int nseg, int64_t nnz, const double *src,
                      double *vals, hipStream_t stream) {
  if (nitems <= 0) return;
  MHA_REQUIRE((reinterpret_cast<uintptr_t>(vals) & 127u) == 0, MHA_ERR_INVALID, "database mode: CRS values must start on a 128-byte line");
  constexpr int U = kCopySpanEntries / kCopyWaveEntries;
  static_assert(U * kCopyWaveEntries == kCopySpanEntries, "a span is whole store instructions of a wavefront");
  // one work item per wavefront: capping the grid (2048 / 8192 workgroups walking the items grid-stride) was slower
  const int grid = (nitems + 3) / 4;
  if (src != vals)
    hipLaunchKernelGGL((line_copy_kernel<U, kCopySegRegs, true>), dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const int4 *>(items), nitems, reinterpret_cast<const int2 *>(seg),
                       static_cast<int>(nnz), src, vals);
  else
    hipLaunchKernelGGL((line_copy_kernel<U, kCopySegRegs, false>), dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const int4 *>(items), nitems, reinterpret_cast<const int2 *>(seg),
                       static_cast<int>(nnz), src, vals);
  MHA_HIP(hipGetLastError());
}

}  // namespace mha
