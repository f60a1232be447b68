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

#ifdef __cplusplus
}
#endif
#endif
