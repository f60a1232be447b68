// assembly_manager.hpp -- host orchestration of one element block on one GPU.
//
// Plays the role of AssemblyManager for the volume terms of a block (reference:
// src/managers/assemblyManager.hpp:173-239, src/managers/assemblyManager.cpp:2150-2665):
// owns the block's mesh/map copies on the device, the reference tables, the physics module, the
// function table and the workset; assembleJacRes drives gather -> residual/Jacobian -> scatter.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.hpp"
#include "physics.hpp"
#include "ref_tables.hpp"
#include "mesh.hpp"
#include "row_blocks_device.hpp"
#include "block_pattern.hpp"
#include "workset.hpp"

namespace mha {

class AssemblyManager {
 public:
  explicit AssemblyManager(const mha_block_desc &desc);
  ~AssemblyManager();

  void setStream(hipStream_t s) { stream_ = s; wkset_.stream = s; }
  hipStream_t stream() const { return stream_; }
  // strong-Dirichlet lifting: u[row] = vals[row] (or `scalar` when vals is null) on the fixed rows
  // (SolverManager::setDirichlet, solverManager.cpp:1876-1957)
  void dirichletLift(double *u, const double *vals, double scalar);
  // modules whose volume term only exists as a point function (multi-variable blocks; thermal with advection)
  bool engineOnly() const { return physics_->pointEngineOnly(); }
  void setMesh(int nelem, const double *nodes, const int32_t *lids, const int32_t *offsets, int nrows,
               const uint8_t *fixed);
  void setOrientation(const int8_t *signs);
  void setGraph(const int32_t *rowptr, const int32_t *colind);
  void selectPhysics(int physics_id);
  void setFunction(const std::string &name, int kind, double amp, const double *freq3, const double *ip_dev);
  void setFunctionExpression(const std::string &name, const std::string &text) { functions_.addExpression(name, text); }
  void setTime(double t) { functions_.setTime(t); wkset_.setTime(t); }
  void setTimeIntegration(int transient, int nsteps, int nstages, int stage, double dt, const double *A,
                          const double *b, const double *bdf);

  void assembleJacRes(int flags, int path, const double *u, const double *u_prev,
                      const double *u_stage, double *res, double *crs_vals);
  void computeLocalJacRes(int compute_jacobian, const double *u, const double *u_prev, const double *u_stage,
                          double *local_J, double *local_res);
  void getMass(const double *masswts, double *local_mass);
  // basis database with exact-geometry matching, matrix-free mass apply (assemblyManager.cpp:4314-4467, 1582-1778)
  int databaseBuild();
  void databaseGet(int32_t *index, int32_t *first_users) const;
  void applyMassMatrixFree(int mode, const double *masswts, const double *mass, int maxent, const int32_t *nnz_row,
                           const double *values, const int32_t *columns, const double *x, double *y);
  // y (+)= A x or A^T x with the matrix assembleJacRes stores (volume terms, fixed rows zero), never formed
  // (kernels/jacobian_apply.hip); flags: MHA_ASSEMBLE_OVERWRITE, MHA_APPLY_TRANSPOSE
  void applyJacobian(int flags, const double *u, const double *u_prev, const double *u_stage, const double *x, double *y);
  // d (+)= diag(A) (kernels/jacobian_diagonal.hip; flags: MHA_ASSEMBLE_OVERWRITE) and the products for nvec vectors
  // x + k ldx -> y + k ldy (kernels/jacobian_apply_multi.hip), on the same route
  void jacobianDiagonal(int flags, const double *u, const double *u_prev, const double *u_stage, double *d);
  void applyJacobianMulti(int flags, const double *u, const double *u_prev, const double *u_stage, int nvec,
                          const double *x, int64_t ldx, double *y, int64_t ldy);
  void swhdgElementBlocks(const double *u, const double *u_prev, const double *u_stage, const double *lambda,
                          const uint8_t *side_types, const double *farfield, double *res, double *blocks);
  // SubGridDtN_Solver::nonlinearSolver for HDG elements with element-local interior unknowns (subgridDtN_solver.cpp:909-1041)
  size_t subgridWorkspaceBytes() const;
  // fused element step of the HDG subgrid (side + volume assembly + static condensation in one kernel)
  bool swhdgFusedUsable() const;
  void swhdgCondensedElement(const double *u, const double *u_prev, const double *u_stage, const double *lambda,
                             const uint8_t *side_types, const double *farfield, SwhFusedOut out);
  void subgridSolve(double *u, const double *u_prev, const double *u_stage, const double *lambda, const uint8_t *side_types,
                    const double *farfield, int max_iter, double tol, void *workspace, size_t workspace_bytes, double *schur,
                    double *gvec, int32_t *iters, double *resnorm_scaled, int32_t *num_singular);
  // HDG subgrids of m x m sub-elements per macro element (kernels/swhdg_subgrid.hpp): the layout (validated on the host;
  // m = 0 clears it), the fused element step, the uncondensed blocks of the plain kernel
  void swhdgSetSubgrids(int m);
  int swhdgSubgrids() const { return subgrid_m_; }
  void swhdgCondensedSubgrid(const double *u, const double *u_prev, const double *u_stage, const double *lambda,
                             const uint8_t *side_types, const double *farfield, SwhFusedOut out);
  void swhdgSubgridBlocks(const double *u, const double *u_prev, const double *u_stage, const double *lambda,
                          const uint8_t *side_types, const double *farfield, double *res, double *blocks);
  // the element step of porousMixedHybridized (kernels/porous_hybrid_blocks.hip, kernels/porous_hybrid_fused.hip): the
  // uncondensed block by the plain kernel; geometry, local matrices, interior solve and Schur complement in one launch
  void pmhElementBlocks(const double *u, const double *lambda, double *res, double *blocks);
  void pmhCondensedElement(const double *u, const double *lambda, double *schur, double *gvec, double *du, int32_t *num_singular);
  // the element step of porousWeakGalerkin (kernels/porous_wg_blocks.hip, kernels/porous_wg_fused.hip), as the pair above
  void pwgElementBlocks(const double *u, const double *lambda, double *res, double *blocks);
  void pwgCondensedElement(const double *u, const double *lambda, double *schur, double *gvec, double *du, int32_t *num_singular);
  void scatterLocal(const double *local_J, const double *local_res, double *res, double *crs_vals);
  // boundary groups (reference: src/tools/boundaryGroup.hpp, assemblyManager.cpp:2518-2638)
  int addBoundaryGroup(const std::string &sidename, int bc_type, int num, const int32_t *elem_ids,
                       const int32_t *side_ids);
  // "Flux" condition of one variable on a side set (PhysicsInterface::fluxConditions, physicsInterface.cpp:1702-1762)
  int addFluxGroup(const std::string &sidename, const std::string &varname, int num, const int32_t *elem_ids,
                   const int32_t *side_ids);
  int addDirichletGroup(const std::string &sidename, const std::string &varname, int num, const int32_t *elem_ids,
                        const int32_t *side_ids);
  void setInitial(int lump_mass, double *rhs, double *mass_vals);
  void setInitialNodal(double *initial);
  void setDirichlet(int lump_mass, double *rhs, double *mass_vals);
  void clearBoundaryGroups() { boundary_groups_.clear(); }
  int numBoundaryGroups() const { return static_cast<int>(boundary_groups_.size()); }
  void assembleBoundary(int flags, const double *u, const double *u_prev, const double *u_stage, double *res,
                        double *crs_vals);
  // y += A_b x / A_b^T x and d += diag(A_b) with the matrix A_b that assembleBoundary(MHA_ASSEMBLE_JACOBIAN) adds into
  // crs_vals, never formed (kernels/boundary_apply.hip); flags: MHA_APPLY_TRANSPOSE for the product, none for the diagonal
  void applyBoundaryJacobian(int flags, const double *u, const double *u_prev, const double *u_stage, const double *x,
                             double *y);
  void boundaryJacobianDiagonal(int flags, const double *u, const double *u_prev, const double *u_stage, double *d);
  // <module>::getDerivedNames / getDerivedValues (linearelasticity.cpp:1289-1360) on all elements of the block
  int numDerived() const { return physics_ ? static_cast<int>(physics_->getDerivedNames().size()) : 0; }
  const char *derivedName(int k);
  void getDerivedValues(const double *u, double *vm, double *mag, double *stress);
  void computeFlux(int group, const double *u, const double *u_prev, const double *u_stage, double *flux, double *dflux_du,
                   double *dflux_daux);
  void boundaryUpdate(int group);
  View boundaryView(int group, const std::string &name) const;
  void setPhysicsParameter(const std::string &name, double value);
  void setParameterVector(const std::string &name, int n, const double *values);
  // the block's element data [E][ncols] (reference: groups->data); importMeshData picks each element's row as the data
  // point nearest to its centre (AssemblyManager::importMeshData, assemblyManager.cpp:8235-8400)
  void setElementData(int ncols, const double *data);
  void importMeshData(int64_t npts, const double *points, int ncols, const double *values, int32_t *seed);
  void applyDbcDiag(double *crs_vals);
  void gather(const double *vec, double *elem_vals);

  int numWorksets() const;
  void worksetUpdate(int index);
  View worksetView(const std::string &name) const;
  // Workset::computeSoln for the current workset (workset.cpp:1017-1190): fills the solution-field views
  void worksetComputeSolution(const double *u, const double *u_prev, const double *u_stage);
  // resetResidual + volumeResidual on the current workset: fills the "res" / "res.dx" views (Workset::getResidual)
  void worksetComputeResidual(int compute_jacobian, const double *u, const double *u_prev, const double *u_stage);

  int64_t info(const std::string &key) const;
  void setTiming(bool on) { timing_ = on; }
  double lastKernelMs() const { return last_ms_; }

  const std::vector<int32_t> &rowptr() const { return h_rowptr_; }
  const std::vector<int32_t> &colind() const { return h_colind_; }
  int numRows() const { return nrows_; }
  int device() const { return device_; }

 private:
  void requireReady(bool need_graph) const;
  void prepareRowOwner();
  void tryPrepareRowOwner();
  bool rowOwnerUsable(std::string *why) const;
  void launchRowOwner(bool compute_jacobian, bool overwrite, double *res, double *crs_vals, bool deterministic = false);
  BlockDev blockDev() const;
  void bindState(const double *u, const double *u_prev, const double *u_stage);
  // shared setup of the four HDG element steps (swhdg*): checks, bound state, side tables, kernel arguments
  struct SwhStep { SwhElementDev a; PhysParamsDev pp; };
  SwhStep swhStepArgs(const double *u, const double *u_prev, const double *u_stage, const double *lambda,
                      const uint8_t *side_types, const double *farfield, bool need_layout);
  // shared setup of the two porousMixedHybridized element steps: module, steady state, DG LIDs (once per mesh), side
  // tables, the kernels' arguments without their outputs
  PmhElementDev pmhStepArgs(const double *u, const double *lambda);
  bool pmh_dg_checked_ = false;
  // the same setup for the two porousWeakGalerkin element steps (the DG check is shared: one module per block)
  PwgElementDev pwgStepArgs(const double *u, const double *lambda);
  void timedBegin();
  void timedEnd();

  int dim_ = 0, order_ = 0, qdeg_ = 0, n_ = 0, nq_ = 0, nnodes_ = 0;  // n_ = dofs per element over all variables
  // variables of the block (GroupMetaData::basis_types / basis orders; wkset->usebasis) and the point engine's tables
  std::vector<VarInfo> vars_;
  bool single_hgrad_ = true;  // the thermal kernels of thermal_*.hip need one HGRAD variable
  std::vector<std::string> derived_names_;  // storage behind derivedName()
  VarLayoutDev layout_;
  DeviceBuffer<double> d_slot_tables_;
  DeviceBuffer<int8_t> d_orient_;
  bool has_orient_ = false;
  void buildVarLayout();
  // row-gather path: row -> (element, position) incidences on the device, full-block dense scratch
  DeviceBuffer<int32_t> d_inc_ptr_, d_inc_elem_, d_inc_pos_, d_inc_dof_;
  DeviceBuffer<double> d_gather_J_, d_gather_res_;
  // porousMixed direct form (ElemOut::direct_*): -1 not decided, 0 no (why in porous_direct_why_), 1 yes
  int porous_direct_ = -1, last_porous_direct_ = 0;
  int last_db_mode_ = 0;
  std::string porous_direct_why_;
  DeviceBuffer<double> d_direct_part_;   // [nrows][2][2]
  DeviceBuffer<uint8_t> d_direct_side_;  // [E][n] (dof order): which incidence of its row the element is
  DeviceBuffer<int32_t> d_direct_diag_;  // [nrows] CRS position of the diagonal of a face row, -1 otherwise
  bool porousDirectUsable();
  void assembleRowGather(int compute_jacobian, bool overwrite, bool adjoint, bool lump_mass, bool porous_direct,
                         double *res, double *crs_vals);
  void assemblePorousDirect(ElemOut o, int compute_jacobian, bool overwrite, double *res, double *crs_vals);
  // database mode of the direct form (uniform mesh, constant coefficients: every element matrix is the same): rows of
  // the same CLASS -- same incident local dofs, same column slots -- are equal, so the element threads store the entries
  // of a few representative rows per class only and line_copy_kernel fills the rest
  struct PorousDatabase {
    int state = -1;  // -1 not tried, 0 not usable (why), 1 built
    std::string why;
    DeviceBuffer<uint8_t> jacflag;     // [E]
    DeviceBuffer<int32_t> elist;       // the elements with jacflag set
    DeviceBuffer<double> uniform;      // element matrix of the uniform block + point tables (ElemOut::direct_uniform)
    double uniform_key[5] = {0, 0, 0, 0, 0};  // (Kinv_xx, _yy, _zz, mobility, alpha_u) the tables were made for
    bool uniform_valid = false;
    int num_listed = 0;
    DeviceBuffer<int32_t> diag;        // finishing pass: diagonal positions of the COMPUTED face rows
    DeviceBuffer<int32_t> copy_items, copy_segs;  // the copy plan of the replicated rows (copy_plan.hpp)
    int num_items = 0, num_segs = 0, num_classes = 0;
    bool axis_aligned = false;  // the common element shape is an axis-aligned box
    int64_t computed_rows = 0;
  } porous_db_;
  bool porousDatabaseUsable();
  void launchDatabaseCopy(double *crs_vals);
  bool has_incidence_ = false;
  RowIncidence inc_;  // host copy, shared by the row gather and the two porousMixed plans
  const RowIncidence &rowIncidence();
  int max_row_ = 0;  // longest CRS row (setGraph)
  void prepareRowGather(bool need_jacobian, bool dense = true);
  void launchPointEngine(int compute_jacobian, const ElemOut &out, int e_begin, int e_count);
  int nelem_ = 0, nrows_ = 0, workset_size_ = 0;
  bool has_mesh_ = false, has_graph_ = false;
  int last_path_ = 0;
  int last_row_owner_kind_ = 0;
  hipStream_t stream_ = nullptr;
  int device_ = 0;  // the context's device (mha_block_desc.device): every C-ABI entry runs under a DeviceGuard for it

  RefTables ref_;
  DeviceBuffer<double> d_ref_basis_, d_ref_grad_, d_ref_wts_, d_nodeval_, d_nodegrad_;
  DeviceBuffer<double> d_phi1d_, d_dphi1d_, d_gw1d_, d_gp1d_;
  DeviceBuffer<uint8_t> d_elem_slot_;  // element-major CRS slot map of the general-element kernel (lazy)
  int elem_slot_bytes_ = 1;
  bool has_elem_slot_ = false;
  void prepareElemSlots();
  void useGeneralKernel(bool need_slots);
  DeviceBuffer<double> d_nodes_;
  DeviceBuffer<double> d_elem_data_;  // setElementData
  DeviceBuffer<int32_t> d_lids_, d_offsets_, d_rowptr_, d_colind_;
  DeviceBuffer<uint8_t> d_fixed_;
  std::vector<int32_t> h_lids_, h_rowptr_, h_colind_;
  std::vector<int32_t> h_offsets_, h_p2d_;  // LID position of every dof, and its inverse
  std::vector<double> hostNodes() const;    // downloaded on demand: [E][nnodes][dim]
  std::vector<uint8_t> h_fixed_;
  bool has_fixed_ = false;

  // row-owner path (row_blocks.hpp, kernels/thermal_row_owner.hip), built lazily
  struct RowOwnerData {
    bool ready = false;
    bool failed = false;  // prepareRowOwner threw: AUTO stops trying
    RowBlocks rb;
    RowBlocksOnDevice rb_dev;
    DeviceBuffer<int32_t> affine_list, general_list;
    DeviceBuffer<double> geo;  // [E][kGeoRec] cached element geometry
    DeviceBuffer<double> erec;  // block-major element records of K2
    DeviceBuffer<uint16_t> pair_off16;
    DeviceBuffer<int> slot_pair;  // LID slots paired by co-ownership (K2 lane layout)
    DeviceBuffer<uint8_t> slot, flags;
    DeviceBuffer<double> khat, phi, dphi, gw, gp;
    AffineTables1D tab1d;  // thread-per-element K1
    bool k1_thread = false;
    // workgroup-merged K1 (K1PlanDev): distinct rows of every 256 consecutive elements + 16-bit positions
    DeviceBuffer<int32_t> k1_row_ptr, k1_rows, k1_elems, k1_shape_idx;
    DeviceBuffer<double> k1_shape;
    bool k1_wg = false;
    DeviceBuffer<uint16_t> k1_loc;
    K1PlanDev k1_plan;
    double max_abs_coord[3] = {0, 0, 0};  // of the block's vertices (bounds the arguments of a closed-form source)
    int slot_bytes = 1;
    int num_affine_elems = 0, num_affine_blocks = 0, num_general_blocks = 0;
    int num_shapes = 0;  // distinct geometry records (shape part, bit for bit) of the block's affine elements
    bool all_rows_covered = false;
  } ro_;
  // general-element row-owner kernel (kernels/thermal_general_row_owner.hip): its own row blocks (2x2x2 / 4x4 chunks,
  // caps sized to that kernel's LDS) and block-major slot table
  struct GeneralRowOwnerData {
    bool tried = false, usable = false;
    std::string why;
    RowBlocks rb;
    RowBlocksOnDevice rb_dev;  // without the accumulator tables, which this kernel does not read
    DeviceBuffer<int32_t> blk_rows;  // [touched element of every block][n]: global row of dof j
    DeviceBuffer<int32_t> blk_hdr;   // [block][12] counts and offsets of the block's tables
    DeviceBuffer<uint8_t> slot;
    bool all_rows_covered = false;
    size_t lds_bytes = 0;
  } gro_;
  void prepareGeneralRowOwner();
  void launchGeneralRowOwner(bool compute_jacobian, bool overwrite, double *res, double *crs_vals, bool ordered = false);
  // row blocks keyed by assembly pattern: the matrix-core form of K2 (block_pattern.hpp); !usable -> the row-block kernel
  // inputs of the geometry-database representatives: the bits of su = alpha_u * kappa and st = alpha_t * rho * c_p,
  // the generation of the tables, the stream rep_vals was written on
  struct RepKey {
    uint64_t su = 0, st = 0, generation = 0;
    hipStream_t stream = nullptr;
    bool operator==(const RepKey &o) const { return su == o.su && st == o.st && generation == o.generation && stream == o.stream; }
  };
  struct BlockPatternData {
    bool tried = false, usable = false;
    std::string why;
    int num_patterns = 0, num_roles = 0, num_blocks = 0;
    int64_t mfma_per_assembly = 0;
    BlockPatternDev dev;
    DeviceBuffer<int32_t> role, seg, wg_seg_ptr, part_ptr, part_hdr, part_lane, rowbase, erec_elem;
    DeviceBuffer<double> w, erec2;
    // geometry-database mode (one shape in the block): the kernel on one representative block per role + replication
    bool db_mode = false;
    DeviceBuffer<int32_t> rep_items, rep_lanes;  // the representatives, one wavefront per item (BpRepPlan)
    DeviceBuffer<double> rep_vals;  // the representatives' CRS entries, compact (BpRepMap), kept across assemblies
    DeviceBuffer<int32_t> copy_items, copy_segs;  // the copy plan, every CRS entry from rep_vals: copy_plan.hpp
    int rep_num_items = 0, copy_num_items = 0, copy_num_segs = 0;
    RepKey rep_key;  // what rep_vals was computed from
    bool rep_key_valid = false;
    bool keep_reps = true;  // MHA_BP_REP_CACHE != 0
  } bpat_;
  uint64_t bpat_generation_ = 0;  // bumped whenever prepareBlockPattern rebuilds erec2, w or the plans
  int64_t rep_launches_ = 0;
  void prepareBlockPattern();

  std::vector<int32_t> db_index_, db_first_users_;  // basis database: representative of every element, their element ids
  DeviceBuffer<int32_t> d_db_index_, d_pos_var_;
  std::vector<int8_t> h_orient_;
  bool subgrid_checked_ = false;
  int subgrid_m_ = 0;  // sub-elements per direction of an HDG subgrid layout, 0 = none (swhdgSetSubgrids)
  // per-variable views (multi-variable blocks): reference tables at the volume / side points, physical basis arrays
  struct VarTables { DeviceBuffer<double> val, grad, div; bool ready = false; };
  struct VarViews { DeviceBuffer<double> basis, grad, div; };
  std::vector<VarTables> var_vol_tables_, var_side_tables_;
  std::vector<VarViews> ws_var_views_;
  std::map<std::string, DeviceBuffer<double>> ws_fields_;  // solution fields of the current workset, by reference name
  int ws_fields_first_ = -1;
  DeviceBuffer<double> ws_res_, ws_res_dx_;
  int ws_res_first_ = -1, ws_res_num_ = 0;
  bool ws_res_has_dx_ = false;
  int varIndex(const std::string &name) const;
  std::string varName(int v) const;
  int varComps(int v) const { return vars_[v].type == MHA_BASIS_HDIV ? dim_ : 1; }
  VarPointsDev varPoints(int v, bool side);
  int addVarGroup(int bc_type, const std::string &sidename, const std::string &varname, int num, const int32_t *elem_ids,
                  const int32_t *side_ids);
  int keepGroup(int bc_type, const std::string &sidename, int var, int num, const int32_t *elem_ids, const int32_t *side_ids);
  void initialFunctions(int v, FuncDesc f[3]) const;
  // basis arrays of variable v on the current workset (aliases the single-variable views of the workset)
  void worksetVarArrays(int v, const double **basis, const double **grad, const double **div) const;

  // host mirror of BoundaryGroup: entries + the side views evaluated on request
  struct BoundaryGroupData {
    std::string sidename;
    int bc_type = 0, num = 0;
    int var = -1;  // MHA_BC_FLUX / MHA_BC_DIRICHLET: the variable the condition is for
    DeviceBuffer<int32_t> elem, side;
    DeviceBuffer<double> wts, xyz[3], nrm[3], basis, basis_grad;
    std::vector<VarViews> var_views;  // multi-variable blocks: "basis side <var>", "basis_grad side <var>"
    bool has_views = false;
  };
  std::vector<std::unique_ptr<BoundaryGroupData>> boundary_groups_;
  SideTables side_ref_;
  DeviceBuffer<double> d_side_ip_, d_side_wts_, d_side_tanU_, d_side_tanV_, d_side_basis_, d_side_grad_, d_side_nodeval_,
      d_side_nodegrad_;
  bool has_side_tables_ = false;
  void prepareSideTables();
  SideTablesDev sideTablesDev() const;
  BoundaryDev boundaryDev(const BoundaryGroupData &g) const;
  // the selected module's rule for a group of the modules (PhysicsBase::checkBoundaryGroup), the default one without a module
  void checkModuleGroup(int bc_type, const std::string &sidename) const;
  void checkModuleGroups() const;
  void bindBoundaryGroup(const BoundaryGroupData &g);
  void boundaryProduct(int mode, const double *u, const double *u_prev, const double *u_stage, const double *x, double *y);

  // scratch of the two-step (updateJac/scatterJac) path, one workset wide
  DeviceBuffer<double> d_local_J_, d_local_res_;

  std::unique_ptr<PhysicsBase> physics_;
  FunctionManager functions_;
  Workset wkset_;
  TimeDev time_;

  bool timing_ = false;
  double last_ms_ = 0.0;
  hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
  // second stream for kernels that run beside the context's stream (K1 next to K2, the porousMixed database mode)
  hipStream_t side_stream_ = nullptr;
  hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
  void ensureSideStream();
};

}  // namespace mha
