// swhdg_subgrid.hpp -- index arithmetic of an HDG subgrid of M x M sub-elements per macro element (shared by
// swhdg_subgrid_fused.hip and swhdg_subgrid_blocks.hip; the layout mha_swhdg_set_subgrids validates on the host).
//
// Sub-elements of macro element k are elements [k M^2, (k+1) M^2) of the block, row-major with x fastest.  The interior
// unknowns of a macro element are (variable i, sub-mesh node) with the node (ax, ay) of the (M+1)^2 lattice numbered
// ay (M+1) + ax: n_int = 3 (M+1)^2, flattened i (M+1)^2 + node.  The 24 trace unknowns follow in the order of
// mha_swhdg_element_blocks: (variable, HFACE edge left/bottom/right/top, function).
//
// Sub-side j of M on macro side s (shards order: bottom, right, top, left) belongs to sub-element (j, 0), (M-1, j),
// (j, M-1), (0, j) and is that sub-element's own local side s; along the macro edge it covers the edge coordinate
// [-1 + 2j/M, -1 + 2(j+1)/M] (the sub-mesh is the bilinear image of the uniform subdivision, so the macro reference
// coordinate of a sub-side point is affine in the sub-element's: src/subgrid/subgridDtN.cpp:746-870, auxside_basis).
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.hpp"

namespace mha {

constexpr int kSgMaxM = 4;  // sub-elements per direction: n_int = 12, 27, 48, 75

__host__ __device__ constexpr int sg_np(int m) { return (m + 1) * (m + 1); }
__host__ __device__ constexpr int sg_ni(int m) { return 3 * sg_np(m); }

// sub-element (ex, ey) of sub-side j on macro side s
__device__ __forceinline__ void sg_side_elem(int m, int s, int j, int &ex, int &ey) {
  ex = s == 1 ? m - 1 : (s == 3 ? 0 : j);
  ey = s == 0 ? 0 : (s == 2 ? m - 1 : j);
}

// lattice node of local dof aa (x fastest) of sub-element (ex, ey)
__device__ __forceinline__ int sg_node(int m, int ex, int ey, int aa) { return (ey + (aa >> 1)) * (m + 1) + ex + (aa & 1); }

// local dof of lattice node (ax, ay) in sub-element (ex, ey), -1 when the node is not one of its four
__device__ __forceinline__ int sg_local(int ax, int ay, int ex, int ey) {
  const int lx = ax - ex, ly = ay - ey;
  return ((lx | ly) & ~1) ? -1 : lx + 2 * ly;
}

// global row of interior unknown (variable i, node) of the macro element whose first sub-element is e0
__device__ __forceinline__ int sg_row(const BlockDev &b, int m, int e0, int i, int node) {
  const int ax = node % (m + 1), ay = node / (m + 1);
  const int ex = ax < m ? ax : m - 1, ey = ay < m ? ay : m - 1;
  return b.lids[(size_t)(e0 + ey * m + ex) * 12 + b.offsets[i * 4 + (ax - ex) + 2 * (ay - ey)]];
}

}  // namespace mha
