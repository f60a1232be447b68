// mesh.hpp -- structured quad/hex mesh + HGRAD dof map generator, and the CRS graph rule.
// Input generation for tests/bench (the reference's mesh stack is out of scope, SURVEY.md
// section 2 row 11).  2-D order 1 reproduces SimpleMeshManager_Rectangle
// (reference: src/tools/simplemeshmanager.hpp:639-675) with offsets {0,1,3,2}
// (src/interfaces/discretizationInterface.cpp:302).
#pragma once
#include <cstdint>
#include <vector>

namespace mha {

void mesh_sizes(int dim, int order, const int *ncell, int *nverts, int *nelem, int64_t *ndof);
void mesh_structured(int dim, int order, const int *ncell, const double *lo, const double *hi,
                     double *verts, int32_t *cell2vert, int32_t *lids, int32_t *offsets,
                     uint8_t *boundary_dof);

// Blocks with several variables (HGRAD of orders dividing the largest, HVOL order 0, HDIV order 1): sizes, then the mesh
// + subcell-major dof map + lowest-order HDIV orientation signs (mesh.cpp).
void mesh_multi_sizes(int dim, const int *ncell, int nvars, const int *types, const int *orders, int *nverts, int *nelem,
                      int *n_tot, int64_t *ndof);
void mesh_structured_multi(int dim, const int *ncell, const double *lo, const double *hi, int nvars, const int *types,
                           const int *orders, double *verts, int32_t *cell2vert, int32_t *lids, int32_t *offsets,
                           int8_t *orient, uint8_t *side_mask, int32_t *dof_var);

// HDG subgrid mesh of shallowwaterHybridized: ncell_macro[2] macro quads on [lo, hi], each an m x m sub-mesh of three order-1
// HGRAD variables that are continuous inside a macro element and discontinuous across macro elements.  Elements
// [k m^2, (k+1) m^2) are macro element k's sub-elements, row-major with x fastest; nodes[E][4][2] in shards vertex order;
// lids[E][12] / offsets[12] in the subcell-major convention of mesh_structured_multi (vertex-major, variables interleaved);
// trace_lids[Em][24] = (variable, HFACE edge left/bottom/right/top, function) -> row of the macro trace system, an edge's
// two functions numbered along +x / +y for both of its macro elements.  ndof = Em 3 (m+1)^2, ntrace = 6 x macro edges.
void mesh_swhdg_subgrids_sizes(const int *ncell_macro, int m, int *nelem, int64_t *ndof, int64_t *ntrace);
void mesh_swhdg_subgrids(const int *ncell_macro, int m, const double *lo, const double *hi, double *nodes, int32_t *lids,
                         int32_t *offsets, int32_t *trace_lids);

// Mesh of a porousMixedHybridized block (mha_mesh_porous_hybrid): nc[dim] cells on [lo, hi], dim = 2 or 3.  DG unknowns
// p, u of every element (lids[e][k] = e (1 + 2 dim) + k, offsets the identity), the face signs mesh_structured_multi gives
// conforming HDIV, one trace row per face of the mesh (faces numbered direction by direction, as the HDIV dofs of
// mesh_structured_multi) listed per element in HFACE order (left, bottom, right, top[, front, back]), and per trace row
// 0 (interior) or 1 + side (0 left, 1 right, 2 bottom, 3 top, 4 front, 5 back).
void mesh_porous_hybrid_sizes(int dim, const int *nc, int *nelem, int64_t *ndof, int64_t *ntrace);
void mesh_porous_hybrid(int dim, const int *nc, const double *lo, const double *hi, double *nodes, int32_t *lids,
                        int32_t *offsets, int8_t *orient, int32_t *trace_lids, uint8_t *trace_side);

// Mesh of a porousWeakGalerkin block (mha_mesh_porous_weak_galerkin): nodes, trace_lids, trace_side and ntrace are
// mesh_porous_hybrid's; the DG unknowns are pint, u, t (lids[e][k] = e (1 + 4 dim) + k, offsets the identity), and u and
// t carry the same face signs in orient[E][1 + 4 dim].
void mesh_porous_weak_galerkin_sizes(int dim, const int *nc, int *nelem, int64_t *ndof, int64_t *ntrace);
void mesh_porous_weak_galerkin(int dim, const int *nc, const double *lo, const double *hi, double *nodes, int32_t *lids,
                               int32_t *offsets, int8_t *orient, int32_t *trace_lids, uint8_t *trace_side);

// The layout check of mha_swhdg_set_subgrids (throws MHA_ERR_INVALID): elements [k m^2, (k+1) m^2) are macro element k's
// m x m sub-mesh, row-major with x fastest; its rows are shared only inside k with the Q1 connectivity of an m x m grid;
// its vertices are the bilinear image of the uniform subdivision of the macro quad to 1e-12 x its size.  m in 1..4.
void check_swhdg_subgrids(int m, int nelem, int nrows, const double *nodes, const int32_t *lids, const int32_t *offsets);

// Overlapped CRS graph: every dof of an element couples to every dof of that element;
// columns ascending (reference: src/interfaces/linearAlgebraInterface.cpp:218-229).
void build_crs_graph(int nrows, int nelem, int n, const int32_t *lids, std::vector<int32_t> &rowptr,
                     std::vector<int32_t> &colind);

// Checks a caller-supplied graph (throws MHA_ERR_INVALID): well-formed CRS, and every (LID_i, LID_j) of every element present.
void validate_crs_graph(int nrows, int nelem, int n, const int32_t *lids, const int32_t *rowptr, const int32_t *colind);

// row -> incident (element, local position) pairs, CSR layout, element-ascending per row.
struct RowIncidence { std::vector<int32_t> ptr, elem, lpos; };
void build_row_incidence(int nrows, int nelem, int n, const int32_t *lids, std::vector<int32_t> &ptr,
                         std::vector<int32_t> &elem, std::vector<int32_t> &lpos);

}  // namespace mha
