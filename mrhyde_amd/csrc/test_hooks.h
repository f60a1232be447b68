/* test_hooks.h -- exported by libmrhyde_amd.so for the CPU test-suite only; NOT part of the drop-in boundary
 * (include/mrhyde_amd.h).  Host-only, no GPU needed. */
#ifndef MRHYDE_AMD_TEST_HOOKS_H
#define MRHYDE_AMD_TEST_HOOKS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Builds the row blocks (Morton chunks of chunk_elems elements) and the block-pattern plan of the matrix-core
 * row-owner Jacobian (csrc/block_pattern.hpp) for the block (nodes [num_elems][nnodes][dim], lids [num_elems][n],
 * CRS graph, fixed [num_rows] or NULL), then walks workgroups / wavefronts / parts / blocks / MFMA panels exactly as
 * kernels/block_pattern.hip does and evaluates on the host
 *   vals[rowptr[r] + slot] = sum_(e incident to r) sum_m scale(m) * factors[e][m] * khat[m][si(e,r)][sj -> slot]
 * (khat [nsym+1][n*n] in LID-slot space, factors [num_elems][nsym+1], scale = scale_u for m < nsym, scale_t for the
 * mass component; fixed rows give zeros).  counts[4] = {patterns, roles, workgroups, parts}.
 * Returns MHA_ERR_INVALID with a reason when the blocks do not group (too many patterns). */
int mha_test_block_patterns_host_apply(int dim, int num_rows, int num_elems, int nnodes, int n, int nsym,
                                       const double *nodes, const int32_t *lids, const int32_t *rowptr,
                                       const int32_t *colind, const uint8_t *fixed, const double *khat,
                                       const double *factors, double scale_u, double scale_t, int chunk_elems,
                                       int num_cus, int max_patterns, double *vals, int *counts);

/* The database modes' line-aligned copy plan (csrc/copy_plan.hpp), built from runs [num_runs][3] = (source entry,
 * destination entry, length) inside vals[0, nnz) and applied on the host with the copy kernel's lane logic
 * (kernels/line_copy.hip).  stores [stores_len >= nnz rounded up to whole spans]: incremented per stored entry.
 * counts[5] = {work items, segments, most segments of one item, entries per span, segment records held at once}. */
int mha_test_copy_plan_host_apply(int64_t nnz, int64_t num_runs, const int64_t *runs, double *vals, int32_t *stores,
                                  int64_t stores_len, int *counts);

/* The geometry-database mode on the host: the block-pattern plan of the mesh (as mha_test_block_patterns_host_apply,
 * scales 1), vals_full = every row block assembled; vals_db (caller-filled, e.g. NaN) gets the entries no copy run
 * covers from vals_full (the representatives') and then the copy plan of block_pattern_copy_runs.
 * counts[7] = the five of mha_test_copy_plan_host_apply, copy runs, roles. */
int mha_test_block_pattern_copy_plan(int dim, int num_rows, int num_elems, int nnodes, int n, int nsym,
                                     const double *nodes, const int32_t *lids, const int32_t *rowptr,
                                     const int32_t *colind, const uint8_t *fixed, const double *khat,
                                     const double *factors, int chunk_elems, int num_cus, int max_patterns,
                                     double *vals_full, double *vals_db, int32_t *stores, int64_t stores_len,
                                     int *counts);

/* The geometry-database representatives' plan on the host (block_pattern.hpp, BpRepPlan): vals_full = every row block
 * assembled (as mha_test_block_patterns_host_apply); vals_rep (caller-filled) gets what the items store, walked with the
 * kernel's arithmetic; every W entry an item reads is checked against the class range of its unit (an error otherwise).
 * stores [nnz]: incremented per stored entry; expect [nnz]: set to 1 on the entries of the roles' first blocks.
 * units [units_len >= 3 x items]: role, part, column tile of every item; part_tiles [>= 2 x parts]: role, column tiles.
 * counts[4] = {items, roles, parts, copy runs}. */
int mha_test_block_pattern_rep_plan(int dim, int num_rows, int num_elems, int nnodes, int n, int nsym,
                                    const double *nodes, const int32_t *lids, const int32_t *rowptr,
                                    const int32_t *colind, const uint8_t *fixed, const double *khat,
                                    const double *factors, double scale_u, double scale_t, int chunk_elems, int num_cus,
                                    int max_patterns, double *vals_full, double *vals_rep, int32_t *stores, int8_t *expect,
                                    int32_t *units, int64_t units_len, int32_t *part_tiles, int64_t part_tiles_len,
                                    int *counts);

/* The geometry-database step with kept representatives on the host (block_pattern.hpp, BpRepMap): the representatives'
 * items store into a compact buffer of their own (rep_stores [>= its entries]: incremented per stored entry) and the
 * separate-source copy plan (copy_plan.hpp, build_copy_plan_from) writes EVERY entry of vals_db (caller-filled, e.g.
 * NaN) from that buffer; every load of the copy is checked against the buffer (an error otherwise).  vals_full, stores:
 * as mha_test_block_pattern_copy_plan.  segs [segs_len >= 2 x segments]: first destination entry, source index -
 * destination entry; items [items_len >= 4 x work items]: first line, first segment, segments met, 0.
 * counts[9] = the five of mha_test_copy_plan_host_apply, copy runs, roles, entries of the compact buffer, items of the
 * representatives' plan. */
int mha_test_block_pattern_step_plan(int dim, int num_rows, int num_elems, int nnodes, int n, int nsym,
                                     const double *nodes, const int32_t *lids, const int32_t *rowptr,
                                     const int32_t *colind, const uint8_t *fixed, const double *khat,
                                     const double *factors, double scale_u, double scale_t, int chunk_elems, int num_cus,
                                     int max_patterns, double *vals_full, double *vals_db, int32_t *stores,
                                     int64_t stores_len, int32_t *rep_stores, int64_t rep_stores_len, int32_t *segs,
                                     int64_t segs_len, int32_t *items, int64_t items_len, int *counts);

/* The layout check of mha_swhdg_set_subgrids alone (mesh.hpp, check_swhdg_subgrids), on host arrays in mha_set_mesh
 * form: nodes [num_elems][4][2], lids [num_elems][12], offsets [12].  Stateless. */
int mha_test_swhdg_check_subgrids(int m, int num_elems, int num_rows, const double *nodes, const int32_t *lids,
                                  const int32_t *offsets);

/* The host-side plans of the affine row-owner path (csrc/row_owner_plan.hpp).  Stateless.
 * K1 plan of geo [num_elems][20] geometry records: order 0 automatic / 1 natural / 2 morton, row_budget <= 0: the default.
 * wg_elems [groups*256], row_ptr [groups+1], rows [<= num_elems*n], loc [groups*n*256], groups = ceil(num_elems / 256);
 * counts[4] = {distinct rows in all, max_rows, axis_aligned, morton order taken}. */
int mha_test_k1_plan(int num_elems, int n, int dim, const int32_t *lids, const int32_t *offsets, const double *geo, int order,
                     int row_budget, int32_t *wg_elems, int32_t *row_ptr, int32_t *rows, uint16_t *loc, int *counts);
/* shapes [num_elems][16] (the first *count records are filled), index [num_elems] */
int mha_test_distinct_shapes(const double *geo, int num_elems, int dim, double *shapes, int32_t *index, int *count);
/* pairs [2*ceil(n/2)] from the ownership masks emask [len] */
int mha_test_pair_lid_slots(const int32_t *emask, int64_t len, int n, int32_t *pairs);
/* the 1-D tables of the HGRAD basis of `order` at order + 1 Gauss points: dcol, phi, dphi [order+1][order+1] */
int mha_test_collocation_derivative(int order, double *dcol, double *phi, double *dphi);

/* The host-side plans of the porousMixed direct form and its database mode (csrc/porous_plan.hpp) on host arrays in
 * mha_set_mesh / mha_set_graph form.  A mesh the plan refuses gives MHA_ERR_INVALID with the reason.  Stateless.
 * side [num_elems][n], diag [num_rows]. */
int mha_test_porous_direct_plan(int num_rows, int num_elems, int n, const int32_t *lids, const int32_t *offsets,
                                const int32_t *rowptr, const int32_t *colind, uint8_t *side, int32_t *diag);
/* orient [num_elems][n] or NULL, fixed [num_rows] or NULL, slot [num_elems][n][n]: position of column lids[e][j] in row
 * lids[e][i].  jacflag, elist [num_elems], diag [num_rows], runs [runs_len >= 3 x copy runs] = (source entry, destination
 * entry, length); counts[5] = {axis_aligned, listed elements, copy runs, row classes, computed rows}. */
int mha_test_porous_database_plan(int num_rows, int num_elems, int n, int nnodes, int dim, const int32_t *lids,
                                  const int32_t *offsets, const int32_t *rowptr, const int32_t *colind, const double *nodes,
                                  const int8_t *orient, const uint8_t *fixed, const uint8_t *slot, uint8_t *jacflag,
                                  int32_t *elist, int32_t *diag, int64_t *runs, int64_t runs_len, int64_t *counts);

/* What a physics module accepts, asked of the module import_physics builds for physics_id (csrc/physics.hpp); no block,
 * no device.  The block's variables are types / orders / cards [num_vars].  bc_type == 0: the variable rule
 * (PhysicsBase::checkVariables).  Otherwise the boundary-group rule (checkBoundaryGroup; physics_id == 0: the rule of a
 * block without a module) for a group of that type on `sidename`, on a block of n dofs per element, order block_order
 * and nqs points per side; define_neumann_e != 0 puts "Neumann e <sidename>" into the function table the rule sees. */
int mha_test_module_rules(int physics_id, int dim, int num_vars, const int32_t *types, const int32_t *orders,
                          const int32_t *cards, int bc_type, const char *sidename, int n, int block_order, int nqs,
                          int define_neumann_e);

/* What a physics module says to a scalar setting (as_vector == 0: PhysicsBase::setParameter) or to a parameter vector of
 * one entry (as_vector != 0: setParameterVector), asked of a fresh module of import_physics; no block, no device. */
int mha_test_module_parameter(int physics_id, int dim, const char *name, double value, int as_vector);

/* The DG check of the porousMixedHybridized element step alone (porous_hybrid.hpp, check_dg_lids) on a host LID map
 * lids [num_elems][n]: every LID in [0, num_rows) and in exactly one element.  Stateless. */
int mha_test_pmh_check_dg(int num_elems, int n, int num_rows, const int32_t *lids);

#ifdef __cplusplus
}
#endif
#endif
