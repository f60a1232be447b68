// porous_hybrid.hpp -- the index conventions of the porousMixedHybridized element step, stated once for its two kernels
// (porous_hybrid_blocks.hip, porous_hybrid_fused.hip).  No arithmetic of the weak form lives here.
//
// flux dof f = 2 c + s:   the raw lowest-order HDIV function (1 -/+ xi_c) / 2 e_c of direction c, s = 0 low / 1 high
//                         face (Intrepid2 HDIV_QUAD/HEX_In_FEM of degree 1; physical: J phi / det J, times the sign);
// trace face k:           the reference's HFACE order (src/tools/Intrepid2_HFACE_QUAD_In_FEMdef.hpp:84-196,
//                         src/tools/Intrepid2_HFACE_HEX_In_FEMdef.hpp:97-269): left x=-1, bottom y=-1, right x=+1,
//                         top y=+1, front z=-1, back z=+1;
// shards side s:          quad bottom, right, top, left; hex y=-1, x=+1, y=+1, x=-1, z=-1, z=+1 (the side tables' order).
#pragma once

namespace mha {

__host__ __device__ constexpr int pmh_side_of_face(int k) { return k < 4 ? (k + 3) & 3 : k; }
__host__ __device__ constexpr int pmh_dof_of_face(int k) { return k < 4 ? 2 * (k & 1) + (k >> 1) : k; }
// reference coordinate c of shards vertex v (quad 0..3, hex 0..7)
__host__ __device__ constexpr double pmh_vertex_coord(int v, int c) {
  return c == 0 ? (((v & 3) == 1 || (v & 3) == 2) ? 1.0 : -1.0) : c == 1 ? ((v & 2) ? 1.0 : -1.0) : ((v & 4) ? 1.0 : -1.0);
}

}  // namespace mha
