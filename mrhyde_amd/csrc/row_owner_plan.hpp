// row_owner_plan.hpp -- host-side tables and plans of the affine row-owner path (AssemblyManager::prepareRowOwner uploads
// them): pure functions of host arrays, no device state, no environment.
#pragma once
#include <cstdint>
#include <vector>

#include "kernels/device_types.hpp"
#include "ref_tables.hpp"

namespace mha {

// Reference tables of the affine path in LID-slot space: [nsym+1][n*n], khat[k][offsets[ib]*n + offsets[jb]] =
// sum_q w (d_a N_ib d_c N_jb + sym) for the k-th pair a <= c, last = sum_q w N_ib N_jb.
std::vector<double> affine_reference_tables(const RefTables &ref, const int32_t *offsets, int dim, int n, int nq);

// 1-D tables of the thread-per-element K1 (order + 1 points per direction): phi, weights, points by value and the
// collocation derivative D = Phi'^T Phi^-T (Gauss-Jordan on the small, well-conditioned point-value matrix).
AffineTables1D collocation_derivative(const RefTables &ref, int order);

// Lane layout of K2: LID slots that are usually owned together by the same (block, element) -- emask, RowBlocks -- paired
// by a greedy matching on the Jaccard similarity of ownership.  -> [2*ceil(n/2)], -1 = none (odd n: the last pair).
std::vector<int> pair_lid_slots(const std::vector<int32_t> &emask, int n);

// Plan of the workgroup-merged K1 (K1PlanDev): the elements in groups of kK1PlanThreads, per group the distinct rows its
// dofs touch (ascending) and per (element, dof in basis order) the position of its row in that list.
enum class K1Order { automatic, natural, morton };
constexpr int kK1RowBudget = 52 * 1024 / 12;  // distinct rows of a group whose LDS image fits three workgroups deep
struct K1Plan {
  std::vector<int32_t> wg_elems, row_ptr, rows;
  std::vector<uint16_t> loc;
  int max_rows = 0;           // of a group, rounded up to even
  bool axis_aligned = false;  // every element's J is diagonal (the test the kernels make per element)
  bool morton = false;        // the order taken
};
// geo: [nelem][kGeoRec] geometry records.  Order of the elements: as numbered (coalesced record loads; good whenever
// consecutive elements are neighbours), or along a Morton curve through the centroids when the numbering scatters a
// group over the mesh (more than row_budget distinct rows) and the curve does better; `forced` takes one.
K1Plan build_k1_plan(int nelem, int n, int dim, const int32_t *lids, const int32_t *offsets, const double *geo,
                     K1Order forced = K1Order::automatic, int row_budget = kK1RowBudget);

// Geometry database (reference: identifyVolumetricDatabase, assemblyManager.cpp:4314-4467; here exact matching of the 16
// shape doubles, bit for bit, so nothing is substituted): distinct shapes in order of first appearance.
struct ShapeTable {
  std::vector<double> shapes;  // [count][16]
  std::vector<int32_t> index;  // [nelem]
  int count = 0;
};
ShapeTable distinct_shapes(const double *geo, int nelem, int dim);

}  // namespace mha
