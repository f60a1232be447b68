"""ctypes binding of include/mrhyde_amd.h (one Python method per C entry point)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "lib", "libmrhyde_amd.so")

PATH_AUTO, PATH_ELEMENT_ATOMIC, PATH_ROW_OWNER, PATH_LOCAL_THEN_SCATTER = 0, 1, 2, 3
FUNC_CONSTANT, FUNC_IP_ARRAY, FUNC_SINPROD = 0, 1, 2
TOPO_QUAD4, TOPO_HEX8 = 4, 8
PHYSICS_THERMAL = 1
MAX_VARS = 8

# every symbol include/mrhyde_amd.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "mha_last_error", "mha_version", "mha_device_count", "mha_block_create", "mha_block_destroy", "mha_set_stream",
    "mha_set_mesh", "mha_set_graph", "mha_get_graph_sizes", "mha_get_graph", "mha_physics_select",
    "mha_set_function", "mha_set_time_integration", "mha_assemble_jacres", "mha_compute_local_jacres",
    "mha_scatter_local", "mha_apply_dbc_diag", "mha_gather", "mha_num_worksets", "mha_workset_update",
    "mha_workset_view", "mha_mesh_sizes", "mha_mesh_structured", "mha_mesh_multi_sizes", "mha_mesh_structured_multi", "mha_swhdg_condensed_element", "mha_compute_flux", "mha_newton_create", "mha_newton_destroy", "mha_newton_reset", "mha_newton_residual", "mha_newton_norm", "mha_newton_decide", "mha_newton_jacobian", "mha_newton_update", "mha_newton_step", "mha_newton_state", "mha_dirichlet_lift", "mha_export_plan_create", "mha_export_plan_destroy", "mha_export_pack", "mha_export_unpack_add", "mha_export_buffers", "mha_export_bytes_on_wire", "mha_comm_unique_id", "mha_comm_create", "mha_comm_destroy", "mha_export_add", "mha_get_info", "mha_set_timing",
    "mha_get_last_kernel_ms", "mha_row_partition_build", "mha_row_partition_sizes", "mha_row_partition_get",
    "mha_row_partition_destroy", "mha_scatter_plan_create", "mha_scatter_plan_nnz",
    "mha_scatter_plan_graph", "mha_scatter_plan_apply", "mha_scatter_plan_destroy", "mha_add_boundary_group", "mha_clear_boundary_groups", "mha_num_boundary_groups",
    "mha_assemble_boundary", "mha_boundary_update", "mha_boundary_view", "mha_set_physics_parameter",
    "mha_set_orientation", "mha_swhdg_side_terms", "mha_swhdg_eigendecomp", "mha_get_mass", "mha_swhdg_element_blocks", "mha_batched_condense", "mha_set_function_expression", "mha_set_time", "mha_check_expression",
    "mha_add_flux_group", "mha_add_dirichlet_group", "mha_set_initial", "mha_set_initial_nodal", "mha_set_dirichlet",
    "mha_workset_compute_solution", "mha_workset_compute_residual",
    "mha_sparse3d_create", "mha_sparse3d_views", "mha_sparse3d_size", "mha_sparse3d_destroy", "mha_database_build",
    "mha_database_get", "mha_apply_mass_matrix_free", "mha_swhdg_subgrid_workspace_bytes", "mha_swhdg_subgrid_solve",
    "mha_set_element_data", "mha_import_mesh_data", "mha_set_parameter_vector", "mha_closest_points", "mha_kl_expansion",
    "mha_kl_indices", "mha_swhdg_set_subgrids", "mha_swhdg_condensed_subgrid", "mha_swhdg_subgrid_blocks",
    "mha_mesh_swhdg_subgrids_sizes", "mha_mesh_swhdg_subgrids",
    "mha_num_derived", "mha_derived_name", "mha_get_derived_values", "mha_apply_jacobian",
    "mha_jacobian_diagonal", "mha_apply_jacobian_multi", "mha_apply_boundary_jacobian",
    "mha_boundary_jacobian_diagonal",
    "mha_pmh_element_blocks", "mha_pmh_condensed_element", "mha_mesh_porous_hybrid_sizes", "mha_mesh_porous_hybrid",
    "mha_pwg_element_blocks", "mha_pwg_condensed_element", "mha_mesh_porous_weak_galerkin_sizes",
    "mha_mesh_porous_weak_galerkin",
]
KL_MAX_TERMS = 8  # MHA_KL_MAX_TERMS: KL roots per direction the kernels evaluate
MASS_ON_THE_FLY, MASS_LOCAL, MASS_DATABASE, MASS_DATABASE_SPARSE = 0, 1, 2, 3
ASSEMBLE_OVERWRITE, APPLY_TRANSPOSE = 2, 32  # the flags of mha_apply_jacobian
APPLY_MAX_VECTORS = 8  # MHA_APPLY_MAX_VECTORS: vectors one launch of mha_apply_jacobian_multi carries
ERR_INVALID = 1  # MHA_ERR_INVALID
SWH_INTERFACE, SWH_FARFIELD, SWH_SLIP = 0, 1, 2
BASIS_HGRAD, BASIS_HVOL, BASIS_HDIV = 0, 1, 2
PHYSICS_IDS = {"thermal": 1, "porousMixed": 2, "navierstokes": 3, "shallowwaterHybridized": 4,
               "navierstokes+thermal": 5,  # 5: `modules: navierstokes, thermal` on one block (ux, pr, uy[, uz], e)
               "linearelasticity": 6,  # dx, dy[, dz] (HGRAD)
               "linearelasticity+thermal": 7}  # `modules: thermal, linearelasticity` on one block (dx, dy[, dz], e)
# cdr: c (HGRAD), convection-diffusion-reaction, its functions may read the solution fields;
# navierstokes+cdr: `modules: navier stokes, cdr` on one block (ux, pr, uy[, uz], c)
PHYSICS_IDS.update({"cdr": 8, "navierstokes+cdr": 9})
PHYSICS_LINEARELASTICITY = 6
PHYSICS_LINEARELASTICITY_THERMAL = 7
PHYSICS_CDR = 8
PHYSICS_NAVIERSTOKES_CDR = 9
# helmholtz: ureal, uimag (HGRAD, one order), the frequency-domain wave module.  Its id is the first with two decimal
# digits.  PHYSICS_IDS stays the table of the one-digit ids (tests/test_cdr.py pins its largest value); Block looks a
# name up in ALL_PHYSICS_IDS, which holds every module.
PHYSICS_HELMHOLTZ = 10
ALL_PHYSICS_IDS = dict(PHYSICS_IDS, helmholtz=PHYSICS_HELMHOLTZ)
# porousMixedHybridized: p (HVOL), u (HDIV-DG) on the block, the trace lambda (HFACE) as data per element.  Id 11 stays
# unassigned (tests/test_module_rules.py pins it as an id that names no module, and ALL_PHYSICS_IDS as the table of the
# ten modules before this one); Block looks a name up in MODULE_IDS, which holds every module.
PHYSICS_POROUS_MIXED_HYBRIDIZED = 12
# porousWeakGalerkin: pint (HVOL), u, t (HDIV-DG) on the block, the trace pbndry (HFACE) as data per element
PHYSICS_POROUS_WEAK_GALERKIN = 13
# stokes: ux, pr, uy[, uz] (HGRAD), optional PSPG / LSIC; shallowwater: H, Hu, Hv (HGRAD, 2-D), continuous Galerkin
PHYSICS_STOKES = 14
PHYSICS_SHALLOWWATER = 15
MODULE_IDS = dict(ALL_PHYSICS_IDS, porousMixedHybridized=PHYSICS_POROUS_MIXED_HYBRIDIZED,
                  porousWeakGalerkin=PHYSICS_POROUS_WEAK_GALERKIN, stokes=PHYSICS_STOKES,
                  shallowwater=PHYSICS_SHALLOWWATER)
PATH_POINT_ENGINE = 4
PATH_ROW_GATHER = 5
BC_NEUMANN, BC_WEAK_DIRICHLET, BC_FLUX = 1, 2, 3
BC_INTERFACE = 5  # thermal: weak-Dirichlet terms with the trace "aux e <side>" as data
BC_SWH_INTERFACE, BC_SWH_FARFIELD, BC_SWH_SLIP = 10, 11, 12


class MhaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mrhyde_amd error %d: %s" % (code, msg))
        self.code = code


class BlockDesc(C.Structure):
    _fields_ = [("dimension", C.c_int), ("topology", C.c_int), ("num_vars", C.c_int),
                ("basis_type", C.c_int * MAX_VARS), ("basis_order", C.c_int * MAX_VARS),
                ("quadrature_degree", C.c_int), ("workset_size", C.c_int), ("device", C.c_int)]


_lib = None


def lib_path():
    return _LIB


def load_library():
    """Load the HIP shared library; fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise ImportError("%s is missing: run `make -C mrhyde_amd/csrc` (or __graft_entry__.build()); "
                              "there is no fallback path" % _LIB)
        # PyTorch bundles its own libamdhip64 (same soname as /opt/rocm's): load torch first so the process
        # holds exactly one HIP runtime, the one that owns torch's device memory and streams.
        import torch  # noqa: F401
        _lib = C.CDLL(_LIB)
        _lib.mha_last_error.restype = C.c_char_p
        _lib.mha_version.restype = C.c_char_p
        _lib.mha_block_destroy.restype = None
        _lib.mha_set_function.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        _lib.mha_set_time_integration.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mha_assemble_jacres.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        _lib.mha_compute_local_jacres.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        _lib.mha_scatter_local.argtypes = [C.c_void_p] * 5
        _lib.mha_apply_dbc_diag.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mha_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mha_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mha_set_mesh.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.mha_set_graph.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mha_get_graph.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mha_get_graph_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mha_physics_select.argtypes = [C.c_void_p, C.c_int]
        _lib.mha_num_worksets.argtypes = [C.c_void_p]
        _lib.mha_workset_update.argtypes = [C.c_void_p, C.c_int]
        _lib.mha_workset_view.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mha_get_info.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
        _lib.mha_set_timing.argtypes = [C.c_void_p, C.c_int]
        _lib.mha_get_last_kernel_ms.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mha_block_destroy.argtypes = [C.c_void_p]
        _lib.mha_add_boundary_group.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p]
        _lib.mha_add_flux_group.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mha_add_dirichlet_group.argtypes = _lib.mha_add_flux_group.argtypes
        _lib.mha_set_initial.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.mha_set_initial_nodal.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mha_set_dirichlet.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.mha_workset_compute_solution.argtypes = [C.c_void_p] * 4
        _lib.mha_workset_compute_residual.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
        _lib.mha_clear_boundary_groups.argtypes = [C.c_void_p]
        _lib.mha_sparse3d_create.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        _lib.mha_sparse3d_views.argtypes = [C.c_void_p] * 5
        _lib.mha_sparse3d_size.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mha_sparse3d_destroy.argtypes = [C.c_void_p]
        _lib.mha_sparse3d_destroy.restype = None
        _lib.mha_database_build.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mha_swhdg_subgrid_workspace_bytes.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mha_swhdg_subgrid_solve.argtypes = ([C.c_void_p] * 7 + [C.c_int, C.c_double, C.c_void_p, C.c_int64] + [C.c_void_p] * 5)
        _lib.mha_database_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mha_apply_mass_matrix_free.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        _lib.mha_apply_jacobian.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        _lib.mha_jacobian_diagonal.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        _lib.mha_apply_boundary_jacobian.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        _lib.mha_boundary_jacobian_diagonal.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        _lib.mha_apply_jacobian_multi.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [
            C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        _lib.mha_num_boundary_groups.argtypes = [C.c_void_p]
        _lib.mha_assemble_boundary.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        _lib.mha_boundary_update.argtypes = [C.c_void_p, C.c_int]
        _lib.mha_boundary_view.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mha_set_physics_parameter.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        _lib.mha_set_orientation.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mha_get_mass.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.mha_swhdg_element_blocks.argtypes = [C.c_void_p] * 9
        _lib.mha_set_function_expression.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        _lib.mha_set_time.argtypes = [C.c_void_p, C.c_double]
        _lib.mha_batched_condense.argtypes = [C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 7
        _lib.mha_swhdg_side_terms.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int64] + [C.c_void_p] * 10
        _lib.mha_swhdg_eigendecomp.argtypes = [C.c_double, C.c_int64] + [C.c_void_p] * 6
        _lib.mha_set_element_data.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.mha_import_mesh_data.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.mha_set_parameter_vector.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
        _lib.mha_closest_points.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _lib.mha_kl_expansion.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        _lib.mha_kl_indices.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        _lib.mha_swhdg_set_subgrids.argtypes = [C.c_void_p, C.c_int]
        _lib.mha_swhdg_condensed_subgrid.argtypes = [C.c_void_p] * 11
        _lib.mha_swhdg_subgrid_blocks.argtypes = [C.c_void_p] * 9
        _lib.mha_mesh_swhdg_subgrids_sizes.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
        _lib.mha_mesh_swhdg_subgrids.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
        _lib.mha_pmh_element_blocks.argtypes = [C.c_void_p] * 5
        _lib.mha_pmh_condensed_element.argtypes = [C.c_void_p] * 7
        _lib.mha_mesh_porous_hybrid_sizes.argtypes = [C.c_int] + [C.c_void_p] * 4
        _lib.mha_mesh_porous_hybrid.argtypes = [C.c_int] + [C.c_void_p] * 9
        _lib.mha_pwg_element_blocks.argtypes = [C.c_void_p] * 5
        _lib.mha_pwg_condensed_element.argtypes = [C.c_void_p] * 7
        _lib.mha_mesh_porous_weak_galerkin_sizes.argtypes = [C.c_int] + [C.c_void_p] * 4
        _lib.mha_mesh_porous_weak_galerkin.argtypes = [C.c_int] + [C.c_void_p] * 9
    return _lib


def _check(rc):
    if rc != 0:
        raise MhaError(rc, load_library().mha_last_error().decode())


def version():
    return load_library().mha_version().decode()


def device_count():
    return load_library().mha_device_count()


def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device arguments must be contiguous CUDA tensors"
    return C.c_void_p(t.data_ptr())


def swhdg_side_terms(side_type, roe, g, S, Shat, normals, Sinf=None, want=("fluxvec", "term", "iflux", "d_dS", "d_dShat")):
    """shallowwaterHybridized side terms at the points of CUDA tensors S, Shat [npts,3], normals [npts,2] (mha_swhdg_side_terms).
    -> dict of CUDA tensors."""
    import torch
    npts = S.shape[0]
    shapes = dict(fluxvec=(npts, 3, 2), term=(npts, 3), iflux=(npts, 3), d_dS=(npts, 3, 3), d_dShat=(npts, 3, 3))
    out = {k: torch.zeros(shapes[k], dtype=torch.float64, device=S.device) for k in want}
    _check(load_library().mha_swhdg_side_terms(side_type, int(roe), float(g), npts, _ptr(S), _ptr(Shat), _ptr(normals),
                                               _ptr(Sinf), _ptr(out.get("fluxvec")), _ptr(out.get("term")),
                                               _ptr(out.get("iflux")), _ptr(out.get("d_dS")), _ptr(out.get("d_dShat")),
                                               None))
    return out


def batched_condense(n_int, n_trace, blocks, res, want_du=True):
    """Static condensation of element blocks [E][n][n] / [E][n] (CUDA tensors) -> (schur, gvec, du, num_singular)."""
    import torch
    E = blocks.shape[0]
    schur = torch.zeros((E, n_trace, n_trace), dtype=torch.float64, device=blocks.device)
    gvec = torch.zeros((E, n_trace), dtype=torch.float64, device=blocks.device)
    du = torch.zeros((E, n_int), dtype=torch.float64, device=blocks.device) if want_du else None
    ns = C.c_int()
    _check(load_library().mha_batched_condense(n_int, n_trace, E, _ptr(blocks), _ptr(res), _ptr(schur), _ptr(gvec), _ptr(du),
                                               C.byref(ns), None))
    return schur, gvec, du, ns.value


NEWTON_SOLVE, NEWTON_BACKTRACKED, NEWTON_DONE = 1, 2, 3


class Newton:
    """The nonlinear-solve protocol of SolverManager::nonlinearSolver behind the C ABI (mha_newton_*): the caller supplies
    the linear solve between step() and update()."""

    def __init__(self, blk, max_iter=10, nl_tol=1e-6, nl_abs_tol=1e-6, use_relative=True, use_absolute=False,
                 allow_backtracking=False, autotune=True):
        lib = load_library()
        self._blk, self._h = blk, C.c_void_p()
        lib.mha_newton_create.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _check(lib.mha_newton_create(blk._h, int(max_iter), float(nl_tol), float(nl_abs_tol), int(use_relative), int(use_absolute),
                                     int(allow_backtracking), int(autotune), C.byref(self._h)))

    def step(self, u, res, vals, u_prev=None, u_stage=None):
        lib = load_library()
        a = C.c_int()
        lib.mha_newton_step.argtypes = [C.c_void_p] * 7
        _check(lib.mha_newton_step(self._h, _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(res), _ptr(vals), C.byref(a)))
        return a.value

    def residual(self, u, res, u_prev=None, u_stage=None):
        lib = load_library()
        lib.mha_newton_residual.argtypes = [C.c_void_p] * 5
        _check(lib.mha_newton_residual(self._h, _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(res)))

    def norm(self, res):
        lib = load_library()
        v = C.c_double()
        lib.mha_newton_norm.argtypes = [C.c_void_p] * 3
        _check(lib.mha_newton_norm(self._h, _ptr(res), C.byref(v)))
        return v.value

    def decide(self, resnorm, u):
        lib = load_library()
        a = C.c_int()
        lib.mha_newton_decide.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        _check(lib.mha_newton_decide(self._h, float(resnorm), _ptr(u), C.byref(a)))
        return a.value

    def jacobian(self, u, res, vals, u_prev=None, u_stage=None):
        lib = load_library()
        lib.mha_newton_jacobian.argtypes = [C.c_void_p] * 6
        _check(lib.mha_newton_jacobian(self._h, _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(res), _ptr(vals)))

    def update(self, u, du):
        lib = load_library()
        lib.mha_newton_update.argtypes = [C.c_void_p] * 3
        _check(lib.mha_newton_update(self._h, _ptr(u), _ptr(du)))

    def state(self):
        lib = load_library()
        it, st = C.c_int(), C.c_int()
        rn, rs, rf, al = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        lib.mha_newton_state.argtypes = [C.c_void_p] * 7
        _check(lib.mha_newton_state(self._h, C.byref(it), C.byref(rn), C.byref(rs), C.byref(rf), C.byref(al), C.byref(st)))
        return dict(iteration=it.value, resnorm=rn.value, resnorm_scaled=rs.value, resnorm_first=rf.value, alpha=al.value,
                    status=st.value)

    def close(self):
        if getattr(self, "_h", None):
            lib = load_library()
            lib.mha_newton_destroy.argtypes = [C.c_void_p]
            lib.mha_newton_destroy.restype = None
            lib.mha_newton_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScatterPlan:
    """Scatter of dense element blocks through an arbitrary LID map (mha_scatter_plan_*): the flux -> trace scatter of
    the HDG caller.  lids [E][n] int32 (host); graph given or built (every dof of an element couples)."""

    def __init__(self, lids, nrows, rowptr=None, colind=None, fixed=None):
        lib = load_library()
        lids = _np(lids, np.int32)
        self.n, self.nrows = lids.shape[1], int(nrows)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rp = None if rowptr is None else _np(rowptr, np.int32)
        ci = None if colind is None else _np(colind, np.int32)
        fx = None if fixed is None else _np(fixed, np.uint8)
        self._h = C.c_void_p()
        lib.mha_scatter_plan_create.argtypes = [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 5
        _check(lib.mha_scatter_plan_create(self.n, lids.shape[0], self.nrows, vp(lids), vp(rp), vp(ci), vp(fx),
                                           C.byref(self._h)))
        nnz = C.c_int64()
        lib.mha_scatter_plan_nnz.argtypes = [C.c_void_p, C.c_void_p]
        _check(lib.mha_scatter_plan_nnz(self._h, C.byref(nnz)))
        self.nnz = nnz.value

    def graph(self):
        lib = load_library()
        rowptr, colind = np.zeros(self.nrows + 1, np.int32), np.zeros(self.nnz, np.int32)
        lib.mha_scatter_plan_graph.argtypes = [C.c_void_p] * 3
        _check(lib.mha_scatter_plan_graph(self._h, rowptr.ctypes.data_as(C.c_void_p), colind.ctypes.data_as(C.c_void_p)))
        return rowptr, colind

    def apply(self, blocks=None, vec=None, res=None, vals=None, overwrite=False, stream=None):
        lib = load_library()
        lib.mha_scatter_plan_apply.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
        _check(lib.mha_scatter_plan_apply(self._h, _ptr(blocks), _ptr(vec), _ptr(res), _ptr(vals), int(overwrite),
                                          None if stream is None else C.c_void_p(stream)))

    def close(self):
        if getattr(self, "_h", None):
            lib = load_library()
            lib.mha_scatter_plan_destroy.argtypes = [C.c_void_p]
            lib.mha_scatter_plan_destroy.restype = None
            lib.mha_scatter_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sparse3D:
    """Sparse3DView (src/tools/sparse3DView.hpp) of a CUDA tensor dense[E][n][n]; device-resident."""

    def __init__(self, dense, tol):
        E, n, n2 = dense.shape
        assert n == n2 and dense.is_contiguous()
        self._h = C.c_void_p()
        self.num_elems, self.n = E, n
        _check(load_library().mha_sparse3d_create(E, n, _ptr(dense), float(tol), None, C.byref(self._h)))
        me, v, c, z = C.c_int(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(load_library().mha_sparse3d_views(self._h, C.byref(me), C.byref(v), C.byref(c), C.byref(z)))
        self.maxent, self._values, self._columns, self._nnz = me.value, v.value, c.value, z.value

    def size(self):
        t = C.c_int64()
        _check(load_library().mha_sparse3d_size(self._h, C.byref(t)))
        return t.value

    def numpy(self):
        """(values[E][n][maxent], columns[E][n][maxent], nnz_row[E][n]) copied to the host."""
        import torch
        torch.cuda.synchronize()
        E, n, me = self.num_elems, self.n, max(self.maxent, 1)
        vals, cols, nnz = np.zeros((E, n, me)), np.zeros((E, n, me), np.int32), np.zeros((E, n), np.int32)
        for arr, ptr in ((vals, self._values), (cols, self._columns), (nnz, self._nnz)):
            assert _hip_memcpy_dtoh(arr.ctypes.data, ptr, arr.size * arr.itemsize) == 0
        return vals[:, :, :self.maxent], cols[:, :, :self.maxent], nnz

    def close(self):
        if self._h:
            load_library().mha_sparse3d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check_expression(text):
    """Raises MhaError if the deck string is not in the supported grammar (host only)."""
    lib = load_library()
    lib.mha_check_expression.argtypes = [C.c_char_p]
    _check(lib.mha_check_expression(text.encode()))


def swhdg_eigendecomp(g, Shat, normals):
    import torch
    npts = Shat.shape[0]
    L = torch.zeros((npts, 3, 3), dtype=torch.float64, device=Shat.device)
    lam = torch.zeros((npts, 3), dtype=torch.float64, device=Shat.device)
    R = torch.zeros_like(L)
    _check(load_library().mha_swhdg_eigendecomp(float(g), npts, _ptr(Shat), _ptr(normals), _ptr(L), _ptr(lam), _ptr(R), None))
    return L, lam, R


def closest_points(query, points):
    """Index of the nearest of points [np, dim] for every row of query [nq, dim] (squared Euclidean distance, ties to the
    lowest index; mha_closest_points, host only).  -> int32 [nq]."""
    q, p = np.atleast_2d(_np(query, np.float64)), np.atleast_2d(_np(points, np.float64))
    assert q.shape[1] == p.shape[1], "query and points differ in dimension"
    idx = np.zeros(q.shape[0], dtype=np.int32)
    _check(load_library().mha_closest_points(q.shape[1], q.shape[0], q.ctypes.data_as(C.c_void_p), p.shape[0],
                                             p.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p)))
    return idx


def kl_expansion(N, L, sigma, eta):
    """The first N roots omega and eigenvalues lambda of a 1-D KL expansion (mha_kl_expansion, host only)."""
    om, lam = np.zeros(N), np.zeros(N)
    _check(load_library().mha_kl_expansion(int(N), float(L), float(sigma), float(eta), om.ctypes.data_as(C.c_void_p),
                                           lam.ctypes.data_as(C.c_void_p)))
    return om, lam


def kl_indices(dim, N):
    """Multi-indices [prod N, dim] of a dim-D KL expansion in the reference's total order (mha_kl_indices, host only)."""
    n = np.ones(3, dtype=np.int32)
    n[:len(N)] = N
    idx = np.zeros((int(np.prod(n[:dim])), dim), dtype=np.int32)
    _check(load_library().mha_kl_indices(int(dim), n.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p)))
    return idx


def mesh_structured(dim, order, ncell, lo=None, hi=None):
    """Structured quad/hex mesh + HGRAD dof map (mha_mesh_structured).  Host numpy arrays."""
    lib = load_library()
    ncell = _np(ncell, np.int32)
    lo = _np(np.zeros(3) if lo is None else lo, np.float64)
    hi = _np(np.ones(3) if hi is None else hi, np.float64)
    nv, ne, nd = C.c_int(), C.c_int(), C.c_int64()
    _check(lib.mha_mesh_sizes(dim, order, ncell.ctypes.data_as(C.c_void_p), C.byref(nv), C.byref(ne), C.byref(nd)))
    n, nn = (order + 1) ** dim, 2 ** dim
    m = dict(verts=np.zeros((nv.value, dim)), cell2vert=np.zeros((ne.value, nn), np.int32),
             lids=np.zeros((ne.value, n), np.int32), offsets=np.zeros(n, np.int32),
             boundary=np.zeros(nd.value, np.uint8), ndof=nd.value, nelem=ne.value, dim=dim, order=order)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(lib.mha_mesh_structured(dim, order, vp(ncell), vp(lo), vp(hi), vp(m["verts"]), vp(m["cell2vert"]),
                                   vp(m["lids"]), vp(m["offsets"]), vp(m["boundary"])))
    m["nodes"] = np.ascontiguousarray(m["verts"][m["cell2vert"]])
    return m


def mesh_multi(dim, ncell, types, orders, lo=None, hi=None):
    """Structured mesh + subcell-major dof map of a block of several variables (mha_mesh_structured_multi).
    -> dict(verts, cell2vert, nodes, lids, offsets, orient, side_mask, dof_var, ndof, nelem, n_tot)."""
    lib = load_library()
    ncell = np.ascontiguousarray(ncell, dtype=np.int32)
    lo = np.zeros(3) if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ones(3) if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
    types, orders = np.ascontiguousarray(types, dtype=np.int32), np.ascontiguousarray(orders, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    nv, ne, nt, nd = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    lib.mha_mesh_multi_sizes.argtypes = [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    _check(lib.mha_mesh_multi_sizes(dim, vp(ncell), len(types), vp(types), vp(orders), C.byref(nv), C.byref(ne), C.byref(nt), C.byref(nd)))
    nn = 2 ** dim
    m = dict(verts=np.zeros((nv.value, dim)), cell2vert=np.zeros((ne.value, nn), np.int32),
             lids=np.zeros((ne.value, nt.value), np.int32), offsets=np.zeros(nt.value, np.int32),
             orient=np.ones((ne.value, nt.value), np.int8), side_mask=np.zeros(nd.value, np.uint8),
             dof_var=np.zeros(nd.value, np.int32), ndof=nd.value, nelem=ne.value, n_tot=nt.value, dim=dim)
    lib.mha_mesh_structured_multi.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 9
    _check(lib.mha_mesh_structured_multi(dim, vp(ncell), vp(lo), vp(hi), len(types), vp(types), vp(orders), vp(m["verts"]),
                                         vp(m["cell2vert"]), vp(m["lids"]), vp(m["offsets"]), vp(m["orient"]),
                                         vp(m["side_mask"]), vp(m["dof_var"])))
    m["nodes"] = np.ascontiguousarray(m["verts"][m["cell2vert"]])
    return m


def mesh_swhdg_subgrids(ncell_macro, m, lo=None, hi=None):
    """HDG subgrid mesh of shallowwaterHybridized (mha_mesh_swhdg_subgrids): ncell_macro macro quads, each an m x m sub-mesh
    whose elements are consecutive (row-major, x fastest).  -> dict(nodes [E][4][2], lids [E][12], offsets [12], trace_lids
    [Em][24], nelem, nmacro, ndof, ntrace, n_int, m)."""
    lib = load_library()
    nc = _np(ncell_macro, np.int32)
    lo = _np(np.zeros(2) if lo is None else lo, np.float64)
    hi = _np(np.ones(2) if hi is None else hi, np.float64)
    ne, nd, nt = C.c_int(), C.c_int64(), C.c_int64()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(lib.mha_mesh_swhdg_subgrids_sizes(vp(nc), int(m), C.byref(ne), C.byref(nd), C.byref(nt)))
    nm = int(nc[0]) * int(nc[1])
    out = dict(nodes=np.zeros((ne.value, 4, 2)), lids=np.zeros((ne.value, 12), np.int32), offsets=np.zeros(12, np.int32),
               trace_lids=np.zeros((nm, 24), np.int32), nelem=ne.value, nmacro=nm, ndof=nd.value, ntrace=nt.value,
               n_int=3 * (m + 1) ** 2, m=int(m), dim=2)
    _check(lib.mha_mesh_swhdg_subgrids(vp(nc), int(m), vp(lo), vp(hi), vp(out["nodes"]), vp(out["lids"]), vp(out["offsets"]),
                                       vp(out["trace_lids"])))
    return out


PMH_SIDES = ("left", "right", "bottom", "top", "front", "back")  # trace_side - 1 of mesh_porous_hybrid


def mesh_porous_hybrid(ncell, lo=None, hi=None):
    """Mesh of a porousMixedHybridized block (mha_mesh_porous_hybrid): len(ncell) = 2 (quads) or 3 (hexes).
    -> dict(nodes [E][2^dim][dim], lids [E][1+2dim] (DG), offsets, orient [E][1+2dim], trace_lids [E][2dim] (HFACE face
    order: left, bottom, right, top[, front, back]), trace_side [ntrace] (0 interior, 1 + index into PMH_SIDES on the
    boundary), ndof, ntrace, nelem, dim)."""
    lib = load_library()
    nc = _np(ncell, np.int32)
    dim = len(nc)
    lo = _np(np.zeros(dim) if lo is None else lo, np.float64)
    hi = _np(np.ones(dim) if hi is None else hi, np.float64)
    if dim not in (2, 3) or len(lo) != dim or len(hi) != dim:
        raise ValueError("mesh_porous_hybrid: ncell, lo, hi of length 2 or 3")
    ne, nd, nt = C.c_int(), C.c_int64(), C.c_int64()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(lib.mha_mesh_porous_hybrid_sizes(dim, vp(nc), C.byref(ne), C.byref(nd), C.byref(nt)))
    ni, nu = 1 + 2 * dim, 2 * dim
    out = dict(nodes=np.zeros((ne.value, 2 ** dim, dim)), lids=np.zeros((ne.value, ni), np.int32), offsets=np.zeros(ni, np.int32),
               orient=np.ones((ne.value, ni), np.int8), trace_lids=np.zeros((ne.value, nu), np.int32),
               trace_side=np.zeros(nt.value, np.uint8), ndof=nd.value, ntrace=nt.value, nelem=ne.value, dim=dim)
    _check(lib.mha_mesh_porous_hybrid(dim, vp(nc), vp(lo), vp(hi), vp(out["nodes"]), vp(out["lids"]), vp(out["offsets"]),
                                      vp(out["orient"]), vp(out["trace_lids"]), vp(out["trace_side"])))
    return out


def mesh_porous_weak_galerkin(ncell, lo=None, hi=None):
    """Mesh of a porousWeakGalerkin block (mha_mesh_porous_weak_galerkin): len(ncell) = 2 (quads) or 3 (hexes).
    -> dict as mesh_porous_hybrid gives it, with the same nodes, trace_lids, trace_side and ntrace; lids [E][1+4dim] (DG:
    pint, u, t), offsets, orient [E][1+4dim] (u and t carry the same face signs), ndof = nelem (1 + 4 dim)."""
    lib = load_library()
    nc = _np(ncell, np.int32)
    dim = len(nc)
    lo = _np(np.zeros(dim) if lo is None else lo, np.float64)
    hi = _np(np.ones(dim) if hi is None else hi, np.float64)
    if dim not in (2, 3) or len(lo) != dim or len(hi) != dim:
        raise ValueError("mesh_porous_weak_galerkin: ncell, lo, hi of length 2 or 3")
    ne, nd, nt = C.c_int(), C.c_int64(), C.c_int64()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(lib.mha_mesh_porous_weak_galerkin_sizes(dim, vp(nc), C.byref(ne), C.byref(nd), C.byref(nt)))
    ni, nu = 1 + 4 * dim, 2 * dim
    out = dict(nodes=np.zeros((ne.value, 2 ** dim, dim)), lids=np.zeros((ne.value, ni), np.int32), offsets=np.zeros(ni, np.int32),
               orient=np.ones((ne.value, ni), np.int8), trace_lids=np.zeros((ne.value, nu), np.int32),
               trace_side=np.zeros(nt.value, np.uint8), ndof=nd.value, ntrace=nt.value, nelem=ne.value, dim=dim)
    _check(lib.mha_mesh_porous_weak_galerkin(dim, vp(nc), vp(lo), vp(hi), vp(out["nodes"]), vp(out["lids"]), vp(out["offsets"]),
                                             vp(out["orient"]), vp(out["trace_lids"]), vp(out["trace_side"])))
    return out


def check_dg_lids(lids, nrows):
    """Host-only test hook (csrc/test_hooks.h): the DG check of the porousMixedHybridized element step; raises MhaError."""
    lids = _np(lids, np.int32)
    f = load_library().mha_test_pmh_check_dg
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    _check(f(lids.shape[0], lids.shape[1], int(nrows), lids.ctypes.data_as(C.c_void_p)))


def module_parameter(physics, dim, name, value=1.0, as_vector=False):
    """Host-only test hook (csrc/test_hooks.h): what a fresh module of `physics` says to a setting; raises MhaError."""
    f = load_library().mha_test_module_parameter
    f.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_double, C.c_int]
    _check(f(MODULE_IDS[physics], int(dim), name.encode(), float(value), int(as_vector)))


def check_swhdg_subgrids(m, nodes, lids, offsets, nrows):
    """Host-only test hook (csrc/test_hooks.h, not part of the boundary): the layout check of Block.set_swhdg_subgrids
    on host arrays; raises MhaError."""
    nodes, lids, offsets = _np(nodes, np.float64), _np(lids, np.int32), _np(offsets, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    f = load_library().mha_test_swhdg_check_subgrids
    f.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
    _check(f(int(m), lids.shape[0], int(nrows), vp(nodes), vp(lids), vp(offsets)))


def block_patterns_host_apply(dim, nodes, lids, nrows, rowptr, colind, khat, factors, fixed=None, scale_u=1.0,
                              scale_t=1.0, chunk_elems=16, num_cus=8, max_patterns=256):
    """Host-only test hook (csrc/test_hooks.h, not part of the boundary): the block-pattern plan of the matrix-core
    row-owner Jacobian, walked as the kernel walks it.  -> (vals [nnz], (patterns, roles, workgroups, parts))."""
    lib = load_library()
    nodes, lids, rowptr, colind = _np(nodes, np.float64), _np(lids, np.int32), _np(rowptr, np.int32), _np(colind, np.int32)
    khat, factors = _np(khat, np.float64), _np(factors, np.float64)
    fx = None if fixed is None else _np(fixed, np.uint8)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    nsym = khat.shape[0] - 1
    vals = np.full(len(colind), np.nan)
    counts = (C.c_int * 4)()
    f = lib.mha_test_block_patterns_host_apply
    f.argtypes = [C.c_int] * 6 + [C.c_void_p] * 7 + [C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    _check(f(int(dim), int(nrows), lids.shape[0], nodes.shape[1], lids.shape[1], nsym, vp(nodes), vp(lids), vp(rowptr),
             vp(colind), vp(fx), vp(khat), vp(factors), float(scale_u), float(scale_t), int(chunk_elems), int(num_cus),
             int(max_patterns), vp(vals), counts))
    return vals, tuple(counts)



def copy_plan_host_apply(nnz, runs, vals):
    """Host-only test hook: the database modes' line-aligned copy plan of `runs` [n][3] = (source, destination, length)
    inside vals[0, nnz), applied on the host as the copy kernel's lanes apply it.  `vals` (float64, at least nnz long)
    is updated in place.  -> (stores [nnz rounded up to whole spans]: entries stored per position,
    dict(items, segments, max_item_segments, span_entries, segment_registers))."""
    lib = load_library()
    runs = _np(np.asarray(runs, np.int64).reshape(-1, 3), np.int64)
    assert vals.dtype == np.float64 and vals.flags.c_contiguous and len(vals) >= nnz
    stores = np.zeros(int(nnz) + 4096, np.int32)
    counts = (C.c_int * 5)()
    f = lib.mha_test_copy_plan_host_apply
    f.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    _check(f(int(nnz), runs.shape[0], runs.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p),
             stores.ctypes.data_as(C.c_void_p), len(stores), counts))
    return stores, dict(zip(("items", "segments", "max_item_segments", "span_entries", "segment_registers"), counts))


def block_pattern_copy_plan(dim, nodes, lids, nrows, rowptr, colind, khat, factors, fixed=None, chunk_elems=16,
                            num_cus=8, max_patterns=256):
    """Host-only test hook: the geometry-database mode of the block-pattern plan on the host.  -> (vals_full: every
    row block assembled, vals_db: NaN but for the representatives' entries, then the copy plan applied, stores, dict)."""
    lib = load_library()
    nodes, lids, rowptr, colind = _np(nodes, np.float64), _np(lids, np.int32), _np(rowptr, np.int32), _np(colind, np.int32)
    khat, factors = _np(khat, np.float64), _np(factors, np.float64)
    fx = None if fixed is None else _np(fixed, np.uint8)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    nsym = khat.shape[0] - 1
    full, db = np.full(len(colind), np.nan), np.full(len(colind), np.nan)
    stores = np.zeros(len(colind) + 4096, np.int32)
    counts = (C.c_int * 7)()
    f = lib.mha_test_block_pattern_copy_plan
    f.argtypes = [C.c_int] * 6 + [C.c_void_p] * 7 + [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]
    _check(f(int(dim), int(nrows), lids.shape[0], nodes.shape[1], lids.shape[1], nsym, vp(nodes), vp(lids), vp(rowptr),
             vp(colind), vp(fx), vp(khat), vp(factors), int(chunk_elems), int(num_cus), int(max_patterns), vp(full),
             vp(db), vp(stores), len(stores), counts))
    return full, db, stores, dict(zip(("items", "segments", "max_item_segments", "span_entries", "segment_registers",
                                       "runs", "roles"), counts))

def block_pattern_rep_plan(dim, nodes, lids, nrows, rowptr, colind, khat, factors, fixed=None, scale_u=1.0, scale_t=1.0,
                           chunk_elems=16, num_cus=8, max_patterns=256):
    """Host-only test hook: the geometry-database representatives' plan (one wavefront per unit column tile of every
    role's first block), walked on the host as its kernel walks it; every W entry an item reads is checked against its
    unit's class range (an error otherwise).  -> (vals_full: every row block assembled, vals_rep: NaN but for the
    entries the items store, stores [nnz], expect [nnz]: 1 on the roles' first blocks, units [items][3]: role, part,
    column tile, part_tiles [parts][2]: role, column tiles, dict)."""
    lib = load_library()
    nodes, lids, rowptr, colind = _np(nodes, np.float64), _np(lids, np.int32), _np(rowptr, np.int32), _np(colind, np.int32)
    khat, factors = _np(khat, np.float64), _np(factors, np.float64)
    fx = None if fixed is None else _np(fixed, np.uint8)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    nsym = khat.shape[0] - 1
    nnz = len(colind)
    full, rep = np.full(nnz, np.nan), np.full(nnz, np.nan)
    stores, expect = np.zeros(nnz, np.int32), np.zeros(nnz, np.int8)
    units, part_tiles = np.full((nnz // 16 + 4096, 3), -1, np.int32), np.full((nnz // 16 + 4096, 2), -1, np.int32)
    counts = (C.c_int * 4)()
    f = lib.mha_test_block_pattern_rep_plan
    f.argtypes = ([C.c_int] * 6 + [C.c_void_p] * 7 + [C.c_double, C.c_double] + [C.c_int] * 3 + [C.c_void_p] * 5 +
                  [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p])
    _check(f(int(dim), int(nrows), lids.shape[0], nodes.shape[1], lids.shape[1], nsym, vp(nodes), vp(lids), vp(rowptr),
             vp(colind), vp(fx), vp(khat), vp(factors), float(scale_u), float(scale_t), int(chunk_elems), int(num_cus),
             int(max_patterns), vp(full), vp(rep), vp(stores), vp(expect), vp(units), units.size, vp(part_tiles),
             part_tiles.size, counts))
    info = dict(zip(("items", "roles", "parts", "runs"), counts))
    return full, rep, stores, expect, units[:info["items"]], part_tiles[:info["parts"]], info


def block_pattern_step_plan(dim, nodes, lids, nrows, rowptr, colind, khat, factors, fixed=None, scale_u=1.0, scale_t=1.0,
                            chunk_elems=16, num_cus=8, max_patterns=256):
    """Host-only test hook: the geometry-database step with kept representatives.  The representatives' items store into
    their own compact buffer; the separate-source copy plan then writes every CRS entry from it (each load checked
    against the buffer).  -> (vals_full: every row block assembled, vals_db: NaN, then the plan applied, stores,
    rep_stores [entries of the compact buffer], segs [segments][2]: first destination entry, source index - destination,
    items [work items][4], dict)."""
    lib = load_library()
    nodes, lids, rowptr, colind = _np(nodes, np.float64), _np(lids, np.int32), _np(rowptr, np.int32), _np(colind, np.int32)
    khat, factors = _np(khat, np.float64), _np(factors, np.float64)
    fx = None if fixed is None else _np(fixed, np.uint8)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    nsym = khat.shape[0] - 1
    nnz = len(colind)
    full, db = np.full(nnz, np.nan), np.full(nnz, np.nan)
    stores, rep_stores = np.zeros(nnz + 4096, np.int32), np.zeros(nnz, np.int32)
    segs, items = np.zeros((nnz + 16, 2), np.int32), np.zeros((nnz // 16 + 16, 4), np.int32)
    counts = (C.c_int * 9)()
    f = lib.mha_test_block_pattern_step_plan
    f.argtypes = ([C.c_int] * 6 + [C.c_void_p] * 7 + [C.c_double, C.c_double] + [C.c_int] * 3 + [C.c_void_p] * 3 +
                  [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p])
    _check(f(int(dim), int(nrows), lids.shape[0], nodes.shape[1], lids.shape[1], nsym, vp(nodes), vp(lids), vp(rowptr),
             vp(colind), vp(fx), vp(khat), vp(factors), float(scale_u), float(scale_t), int(chunk_elems), int(num_cus),
             int(max_patterns), vp(full), vp(db), vp(stores), len(stores), vp(rep_stores), len(rep_stores), vp(segs),
             segs.size, vp(items), items.size, counts))
    info = dict(zip(("items", "segments", "max_item_segments", "span_entries", "segment_registers", "runs", "roles",
                     "rep_entries", "rep_items"), counts))
    return (full, db, stores, rep_stores[:info["rep_entries"]], segs[:info["segments"]], items[:info["items"]], info)


def k1_plan(dim, lids, offsets, geo, order="auto", row_budget=0):
    """Host-only test hook: the plan of the workgroup-merged residual kernel (csrc/row_owner_plan.hpp) for the geometry
    records geo [E][20].  order: "auto", "natural" or "morton"; row_budget 0: the kernel's.  -> dict(wg_elems [G*256],
    row_ptr [G+1], rows, loc [G][n][256], max_rows, axis_aligned, morton)."""
    lids, offsets, geo = _np(lids, np.int32), _np(offsets, np.int32), _np(geo, np.float64)
    ne, n = lids.shape
    assert geo.shape == (ne, 20)
    G = (ne + 255) // 256
    out = dict(wg_elems=np.zeros(G * 256, np.int32), row_ptr=np.zeros(G + 1, np.int32), rows=np.zeros(ne * n, np.int32),
               loc=np.zeros((G, n, 256), np.uint16))
    counts = (C.c_int * 4)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    f = load_library().mha_test_k1_plan
    f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_void_p] * 5
    _check(f(ne, n, int(dim), vp(lids), vp(offsets), vp(geo), ("auto", "natural", "morton").index(order), int(row_budget),
             vp(out["wg_elems"]), vp(out["row_ptr"]), vp(out["rows"]), vp(out["loc"]), counts))
    out["rows"] = out["rows"][:counts[0]]
    out.update(max_rows=counts[1], axis_aligned=bool(counts[2]), morton=bool(counts[3]))
    return out


def distinct_shapes(dim, geo):
    """Host-only test hook: the bit-exact geometry-shape database of geo [E][20].  -> (shapes [count][16], index [E])."""
    geo = _np(geo, np.float64)
    shapes, index, count = np.zeros((geo.shape[0], 16)), np.zeros(geo.shape[0], np.int32), C.c_int()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    f = load_library().mha_test_distinct_shapes
    f.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3
    _check(f(vp(geo), geo.shape[0], int(dim), vp(shapes), vp(index), C.byref(count)))
    return shapes[:count.value], index


def pair_lid_slots(emask, n):
    """Host-only test hook: LID slots paired by co-ownership from the ownership masks.  -> int32 [2*ceil(n/2)]."""
    emask = _np(emask, np.int32)
    pairs = np.zeros(2 * ((n + 1) // 2), np.int32)
    f = load_library().mha_test_pair_lid_slots
    f.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    _check(f(emask.ctypes.data_as(C.c_void_p), len(emask), int(n), pairs.ctypes.data_as(C.c_void_p)))
    return pairs


def collocation_derivative(order):
    """Host-only test hook: the 1-D collocation derivative of the residual kernel and the 1-D tables it was made from.
    -> (dcol [q][q'], phi [i][q], dphi [i][q]), each [order+1][order+1]."""
    m = order + 1
    dcol, phi, dphi = np.zeros((m, m)), np.zeros((m, m)), np.zeros((m, m))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    f = load_library().mha_test_collocation_derivative
    f.argtypes = [C.c_int] + [C.c_void_p] * 3
    _check(f(int(order), vp(dcol), vp(phi), vp(dphi)))
    return dcol, phi, dphi


def porous_direct_plan(lids, offsets, nrows, rowptr, colind):
    """Host-only test hook: the plan of the porousMixed direct form (csrc/porous_plan.hpp); raises MhaError with the reason
    when the mesh does not allow it.  -> (side [E][n], diag [nrows])."""
    lids, offsets, rowptr, colind = _np(lids, np.int32), _np(offsets, np.int32), _np(rowptr, np.int32), _np(colind, np.int32)
    side, diag = np.zeros(lids.shape, np.uint8), np.zeros(nrows, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    f = load_library().mha_test_porous_direct_plan
    f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 6
    _check(f(int(nrows), lids.shape[0], lids.shape[1], vp(lids), vp(offsets), vp(rowptr), vp(colind), vp(side), vp(diag)))
    return side, diag


def porous_database_plan(nodes, lids, offsets, nrows, rowptr, colind, slot, orient=None, fixed=None):
    """Host-only test hook: the plan of the porousMixed database mode; raises MhaError with the reason when the block does
    not allow it.  slot [E][n][n]: position of column lids[e][j] in row lids[e][i].  -> dict(axis_aligned, jacflag [E],
    elist, diag [nrows], runs [k][3] = (source, destination, length), num_classes, computed_rows)."""
    nodes, lids, offsets = _np(nodes, np.float64), _np(lids, np.int32), _np(offsets, np.int32)
    rowptr, colind, slot = _np(rowptr, np.int32), _np(colind, np.int32), _np(slot, np.uint8)
    ori = None if orient is None else _np(orient, np.int8)
    fx = None if fixed is None else _np(fixed, np.uint8)
    ne, n = lids.shape
    jacflag, elist, diag = np.zeros(ne, np.uint8), np.zeros(ne, np.int32), np.zeros(nrows, np.int32)
    runs, counts = np.zeros((len(colind) + 1, 3), np.int64), np.zeros(5, np.int64)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    f = load_library().mha_test_porous_database_plan
    f.argtypes = [C.c_int] * 5 + [C.c_void_p] * 12 + [C.c_int64, C.c_void_p]
    _check(f(int(nrows), ne, n, nodes.shape[1], nodes.shape[2], vp(lids), vp(offsets), vp(rowptr), vp(colind), vp(nodes),
             vp(ori), vp(fx), vp(slot), vp(jacflag), vp(elist), vp(diag), vp(runs), runs.size, vp(counts)))
    return dict(axis_aligned=bool(counts[0]), jacflag=jacflag, elist=elist[:counts[1]], diag=diag, runs=runs[:counts[2]],
                num_classes=int(counts[3]), computed_rows=int(counts[4]))


def row_partition(dim, nodes, lids, nrows, rowptr, caps=None):
    """Host-only: the row-owner partition (mha_row_partition_*).  -> dict(row_ptr, rows, elem_ptr, elems, max_*)."""
    lib = load_library()
    nodes, lids, rowptr = _np(nodes, np.float64), _np(lids, np.int32), _np(rowptr, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    cp = None if caps is None else _np(caps, np.int32)
    lib.mha_row_partition_build.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5
    _check(lib.mha_row_partition_build(dim, lids.shape[0], lids.shape[1], int(nrows), vp(nodes), vp(lids), vp(rowptr),
                                       None if cp is None else vp(cp), C.byref(h)))
    try:
        nb, nr, ne = C.c_int(), C.c_int64(), C.c_int64()
        mr, me, ma = C.c_int(), C.c_int(), C.c_int()
        lib.mha_row_partition_sizes.argtypes = [C.c_void_p] * 7
        _check(lib.mha_row_partition_sizes(h, C.byref(nb), C.byref(nr), C.byref(ne), C.byref(mr), C.byref(me),
                                           C.byref(ma)))
        out = dict(row_ptr=np.zeros(nb.value + 1, np.int32), rows=np.zeros(nr.value, np.int32),
                   elem_ptr=np.zeros(nb.value + 1, np.int32), elems=np.zeros(ne.value, np.int32),
                   max_rows=mr.value, max_elems=me.value, max_entries=ma.value, num_blocks=nb.value)
        lib.mha_row_partition_get.argtypes = [C.c_void_p] * 5
        _check(lib.mha_row_partition_get(h, vp(out["row_ptr"]), vp(out["rows"]), vp(out["elem_ptr"]), vp(out["elems"])))
    finally:
        lib.mha_row_partition_destroy.argtypes = [C.c_void_p]
        lib.mha_row_partition_destroy.restype = None
        lib.mha_row_partition_destroy(h)
    return out


class Block:
    """One element block on one GPU (mha_context)."""

    def __init__(self, dim, order=1, quadrature=0, workset_size=100, device=0, physics="thermal", variables=None):
        """variables: list of (basis type, order) in the module's myvars order; default one HGRAD variable of `order`."""
        lib = load_library()
        d = BlockDesc()
        variables = [(BASIS_HGRAD, order)] if variables is None else list(variables)
        d.dimension, d.topology, d.num_vars = dim, (TOPO_QUAD4 if dim == 2 else TOPO_HEX8), len(variables)
        for v, (t, o) in enumerate(variables):
            d.basis_type[v], d.basis_order[v] = int(t), int(o)
        d.quadrature_degree, d.workset_size, d.device = quadrature, workset_size, device
        self._h = C.c_void_p()
        _check(lib.mha_block_create(C.byref(d), C.byref(self._h)))
        self.dim, self.order = dim, order
        self._keep = []
        if physics is not None:
            if physics not in MODULE_IDS:
                raise ValueError(physics)
            _check(lib.mha_physics_select(self._h, MODULE_IDS[physics]))

    def close(self):
        if getattr(self, "_h", None):
            load_library().mha_block_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- setup ------------------------------------------------------------
    def set_stream(self, cuda_stream_handle):
        _check(load_library().mha_set_stream(self._h, C.c_void_p(cuda_stream_handle)))

    def set_mesh(self, nodes, lids, offsets, nrows, fixed=None):
        nodes, lids, offsets = _np(nodes, np.float64), _np(lids, np.int32), _np(offsets, np.int32)
        fixed = None if fixed is None else _np(fixed, np.uint8)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _check(load_library().mha_set_mesh(self._h, lids.shape[0], vp(nodes), vp(lids), vp(offsets), int(nrows),
                                           vp(fixed)))
        self.nelem, self.n, self.nrows = lids.shape[0], lids.shape[1], int(nrows)

    def set_orientation(self, signs):
        signs = None if signs is None else _np(signs, np.int8)
        _check(load_library().mha_set_orientation(self._h, None if signs is None else signs.ctypes.data_as(C.c_void_p)))

    def set_graph(self, rowptr=None, colind=None):
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        if rowptr is not None:
            rowptr, colind = _np(rowptr, np.int32), _np(colind, np.int32)
        _check(load_library().mha_set_graph(self._h, vp(rowptr), vp(colind)))

    def get_graph(self):
        nr, nnz = C.c_int(), C.c_int64()
        _check(load_library().mha_get_graph_sizes(self._h, C.byref(nr), C.byref(nnz)))
        rowptr, colind = np.zeros(nr.value + 1, np.int32), np.zeros(nnz.value, np.int32)
        _check(load_library().mha_get_graph(self._h, rowptr.ctypes.data_as(C.c_void_p),
                                            colind.ctypes.data_as(C.c_void_p)))
        return rowptr, colind

    def set_function(self, name, value):
        """value: float | deck string ("8*pi*pi*sin(2*pi*x)") | ("sinprod", amp, freq[dim]) | CUDA tensor [E, numip]."""
        lib = load_library()
        if isinstance(value, str):
            _check(lib.mha_set_function_expression(self._h, name.encode(), value.encode()))
        elif isinstance(value, (int, float)):
            _check(lib.mha_set_function(self._h, name.encode(), FUNC_CONSTANT, float(value), None, None))
        elif isinstance(value, tuple) and value[0] == "sinprod":
            fr = np.zeros(3)
            fr[:len(value[2])] = value[2]
            _check(lib.mha_set_function(self._h, name.encode(), FUNC_SINPROD, float(value[1]),
                                        fr.ctypes.data_as(C.c_void_p), None))
        else:
            self._keep.append(value)
            _check(lib.mha_set_function(self._h, name.encode(), FUNC_IP_ARRAY, 0.0, None, _ptr(value)))

    def set_time(self, t):
        _check(load_library().mha_set_time(self._h, float(t)))

    def set_time_integration(self, transient, nsteps=0, nstages=0, stage=0, dt=1.0, butcher_A=None, butcher_b=None,
                             bdf=None):
        vp = lambda a: None if a is None else _np(a, np.float64).ctypes.data_as(C.c_void_p)
        A, b, w = (None if x is None else _np(x, np.float64) for x in (butcher_A, butcher_b, bdf))
        _check(load_library().mha_set_time_integration(self._h, int(transient), nsteps, nstages, stage, float(dt),
                                                       vp(A), vp(b), vp(w)))

    # -- assembly -----------------------------------------------------------
    def assemble_jacres(self, u, res, crs_vals=None, compute_jacobian=True, path=PATH_AUTO, u_prev=None,
                        u_stage=None, overwrite=False, adjoint=False, lump_mass=False, deterministic=False):
        """adjoint / lump_mass: the scatter options isAdjoint_ / lump_mass_ of the reference (MHA_ASSEMBLE_ADJOINT, _LUMP_MASS);
        deterministic: MHA_ASSEMBLE_DETERMINISTIC (bit-reproducible results on the affine row-owner path)."""
        flags = ((1 if compute_jacobian else 0) | (2 if overwrite else 0) | (4 if adjoint else 0) | (8 if lump_mass else 0) |
                 (16 if deterministic else 0))
        _check(load_library().mha_assemble_jacres(self._h, flags, path, _ptr(u), _ptr(u_prev),
                                                  _ptr(u_stage), _ptr(res), _ptr(crs_vals)))

    def compute_local_jacres(self, u, local_J, local_res, compute_jacobian=True, u_prev=None, u_stage=None):
        _check(load_library().mha_compute_local_jacres(self._h, int(compute_jacobian), _ptr(u), _ptr(u_prev),
                                                       _ptr(u_stage), _ptr(local_J), _ptr(local_res)))

    def get_mass(self, local_mass, masswts=None):
        w = None if masswts is None else _np(masswts, np.float64)
        _check(load_library().mha_get_mass(self._h, None if w is None else w.ctypes.data_as(C.c_void_p), _ptr(local_mass)))

    def swhdg_element_blocks(self, u, lam, res, blocks, side_types=None, farfield=None, u_prev=None, u_stage=None):
        ff = None if farfield is None else _np(farfield, np.float64)
        _check(load_library().mha_swhdg_element_blocks(self._h, _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(lam),
                                                       _ptr(side_types), None if ff is None else ff.ctypes.data_as(C.c_void_p),
                                                       _ptr(res), _ptr(blocks)))

    def database_build(self):
        """identifyVolumetricDatabase with exact matching -> (basis_index[E], first_users[U])."""
        nu = C.c_int()
        _check(load_library().mha_database_build(self._h, C.byref(nu)))
        ne = self.info("num_elems")
        idx, fu = np.zeros(ne, np.int32), np.zeros(nu.value, np.int32)
        _check(load_library().mha_database_get(self._h, idx.ctypes.data_as(C.c_void_p), fu.ctypes.data_as(C.c_void_p)))
        return idx, fu

    def apply_mass_matrix_free(self, x, y, mode=MASS_ON_THE_FLY, masswts=None, mass=None, sparse=None):
        """y += M x (AssemblyManager::applyMassMatrixFree); mass: CUDA tensor of dense element / database masses, sparse: Sparse3D."""
        w = None if masswts is None else _np(masswts, np.float64)
        _check(load_library().mha_apply_mass_matrix_free(self._h, mode, None if w is None else w.ctypes.data_as(C.c_void_p),
                                                         _ptr(mass), None if sparse is None else sparse._h, _ptr(x), _ptr(y)))

    def apply_jacobian(self, u, x, y, transpose=False, overwrite=False, u_prev=None, u_stage=None):
        """y += A x (transpose: A^T x; overwrite: y = ...) with the matrix assemble_jacres stores -- volume terms, current
        time-integration seeding, fixed rows zero -- never formed (mha_apply_jacobian)."""
        flags = (ASSEMBLE_OVERWRITE if overwrite else 0) | (APPLY_TRANSPOSE if transpose else 0)
        _check(load_library().mha_apply_jacobian(self._h, flags, _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(x), _ptr(y)))

    def jacobian_diagonal(self, u, d, overwrite=False, u_prev=None, u_stage=None):
        """d += diag(A) (overwrite: d = ...) with the matrix of apply_jacobian, never formed (mha_jacobian_diagonal).  d is
        zero where A is: on fixed rows and on rows the module leaves empty."""
        _check(load_library().mha_jacobian_diagonal(self._h, ASSEMBLE_OVERWRITE if overwrite else 0, _ptr(u), _ptr(u_prev),
                                                    _ptr(u_stage), _ptr(d)))

    def apply_boundary_jacobian(self, u, x, y, transpose=False, u_prev=None, u_stage=None):
        """y += A_b x (transpose: A_b^T x) with the matrix assemble_boundary adds into crs_vals -- all groups of the block,
        current seeding, fixed rows zero -- never formed (mha_apply_boundary_jacobian).  Always accumulates: run
        apply_jacobian(..., overwrite=True) first and this on the same y."""
        _check(load_library().mha_apply_boundary_jacobian(self._h, APPLY_TRANSPOSE if transpose else 0, _ptr(u), _ptr(u_prev),
                                                          _ptr(u_stage), _ptr(x), _ptr(y)))

    def boundary_jacobian_diagonal(self, u, d, u_prev=None, u_stage=None):
        """d += diag(A_b) with the matrix of apply_boundary_jacobian, never formed (mha_boundary_jacobian_diagonal)."""
        _check(load_library().mha_boundary_jacobian_diagonal(self._h, 0, _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(d)))

    def apply_jacobian_multi(self, u, X, Y, transpose=False, overwrite=False, u_prev=None, u_stage=None):
        """Y[k] += A X[k] (transpose: A^T X[k]; overwrite: Y[k] = ...) for every row k of X (mha_apply_jacobian_multi).
        X, Y: 2-D float64 device tensors [K, >= nrows] with stride(1) == 1 and the same shape -- a Krylov basis; the
        leading dimension is stride(0), and columns past nrows are never written."""
        import torch
        for name, t in (("X", X), ("Y", Y)):
            if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2 or t.dtype != torch.float64
                    or (t.shape[1] > 1 and t.stride(1) != 1)):
                raise MhaError(ERR_INVALID, "apply_jacobian_multi: %s must be a 2-D float64 device tensor, contiguous in "
                               "its last dimension" % name)
        if X.shape != Y.shape:
            raise MhaError(ERR_INVALID, "apply_jacobian_multi: X %s and Y %s differ in shape" % (tuple(X.shape), tuple(Y.shape)))
        ld = lambda t: t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
        flags = (ASSEMBLE_OVERWRITE if overwrite else 0) | (APPLY_TRANSPOSE if transpose else 0)
        _check(load_library().mha_apply_jacobian_multi(self._h, flags, _ptr(u), _ptr(u_prev), _ptr(u_stage), X.shape[0],
                                                       C.c_void_p(X.data_ptr()), ld(X), C.c_void_p(Y.data_ptr()), ld(Y)))

    def swhdg_condensed_element(self, u, lam, schur=None, gvec=None, du=None, num_singular=None, side_types=None,
                                farfield=None, u_prev=None, u_stage=None):
        """Side + volume assembly + static condensation of every HDG element in one kernel (mha_swhdg_condensed_element):
        fills the given CUDA tensors schur [E][24][24], gvec [E][24], du [E][12]; nothing else leaves the chip."""
        ff = None if farfield is None else _np(farfield, np.float64)
        lib = load_library()
        lib.mha_swhdg_condensed_element.argtypes = [C.c_void_p] * 11
        _check(lib.mha_swhdg_condensed_element(self._h, _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(lam), _ptr(side_types),
                                               None if ff is None else ff.ctypes.data_as(C.c_void_p), _ptr(schur), _ptr(gvec),
                                               _ptr(du), _ptr(num_singular)))

    def pmh_element_blocks(self, u, lam, res=None, blocks=None):
        """The uncondensed element block of porousMixedHybridized by the plain kernel (mha_pmh_element_blocks): fills the CUDA
        tensors res [E][n] = -res.val(), blocks [E][n][n] (n = 1 + 4 dim: p, u, then the traces in HFACE order)."""
        _check(load_library().mha_pmh_element_blocks(self._h, _ptr(u), _ptr(lam), _ptr(res), _ptr(blocks)))

    def pmh_condensed_element(self, u, lam, schur=None, gvec=None, du=None, num_singular=None):
        """The element step of porousMixedHybridized in one kernel (mha_pmh_condensed_element): fills the given CUDA tensors
        schur [E][2dim][2dim], gvec [E][2dim], du [E][1+2dim]; num_singular: int32 device counter, incremented.  No sync."""
        _check(load_library().mha_pmh_condensed_element(self._h, _ptr(u), _ptr(lam), _ptr(schur), _ptr(gvec), _ptr(du),
                                                        _ptr(num_singular)))

    def pwg_element_blocks(self, u, lam, res=None, blocks=None):
        """The uncondensed element block of porousWeakGalerkin by the plain kernel (mha_pwg_element_blocks): fills the CUDA
        tensors res [E][n] = -res.val(), blocks [E][n][n] (n = 1 + 6 dim: pint, u, t, then the traces in HFACE order)."""
        _check(load_library().mha_pwg_element_blocks(self._h, _ptr(u), _ptr(lam), _ptr(res), _ptr(blocks)))

    def pwg_condensed_element(self, u, lam, schur=None, gvec=None, du=None, num_singular=None):
        """The element step of porousWeakGalerkin in one kernel (mha_pwg_condensed_element): fills the given CUDA tensors
        schur [E][2dim][2dim], gvec [E][2dim], du [E][1+4dim]; num_singular: int32 device counter, incremented.  No sync."""
        _check(load_library().mha_pwg_condensed_element(self._h, _ptr(u), _ptr(lam), _ptr(schur), _ptr(gvec), _ptr(du),
                                                        _ptr(num_singular)))

    def set_swhdg_subgrids(self, m):
        """Declare elements [k m^2, (k+1) m^2) as macro element k's m x m sub-mesh (mha_swhdg_set_subgrids; validated on the
        host; m = 0 clears the layout)."""
        _check(load_library().mha_swhdg_set_subgrids(self._h, int(m)))
        self._subgrid_m = int(m)

    def swhdg_condensed_subgrid(self, u, lam, schur=None, gvec=None, du=None, num_singular=None, side_types=None,
                                farfield=None, u_prev=None, u_stage=None):
        """The element step of an HDG subgrid in one kernel (mha_swhdg_condensed_subgrid): fills the given CUDA tensors
        schur [Em][24][24], gvec [Em][24], du [Em][n_int] per macro element; lam [Em][24], side_types [Em][4]."""
        ff = None if farfield is None else _np(farfield, np.float64)
        _check(load_library().mha_swhdg_condensed_subgrid(self._h, _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(lam),
                                                          _ptr(side_types), None if ff is None else ff.ctypes.data_as(C.c_void_p),
                                                          _ptr(schur), _ptr(gvec), _ptr(du), _ptr(num_singular)))

    def swhdg_subgrid_blocks(self, u, lam, res, blocks, side_types=None, farfield=None, u_prev=None, u_stage=None):
        """The uncondensed res [Em][n_int+24] and blocks [Em][n_int+24][n_int+24] of an HDG subgrid by the plain kernel
        (mha_swhdg_subgrid_blocks), the independent implementation the fused step is compared with."""
        ff = None if farfield is None else _np(farfield, np.float64)
        _check(load_library().mha_swhdg_subgrid_blocks(self._h, _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(lam),
                                                       _ptr(side_types), None if ff is None else ff.ctypes.data_as(C.c_void_p),
                                                       _ptr(res), _ptr(blocks)))

    def swhdg_subgrid_solve(self, u, lam, max_iter, tol, side_types=None, farfield=None, u_prev=None, u_stage=None,
                            want_condensed=True):
        """SubGridDtN_Solver::nonlinearSolver on the device (u updated in place) -> dict(iters, resnorm, schur, gvec, num_singular).
        No host synchronisation happens inside the call; the tensors are ready once the stream is.  On a block with a
        subgrid layout (set_swhdg_subgrids) lam is [Em][24] and every output is per macro element."""
        import torch
        nb = C.c_int64()
        _check(load_library().mha_swhdg_subgrid_workspace_bytes(self._h, C.byref(nb)))
        E = lam.shape[0]
        # one workspace per Block, reallocated only when the size changes (a new mesh): a time loop that calls this once
        # per macro step must not grow the heap (0.8 GB per call at 256^2 elements)
        ws = getattr(self, "_subgrid_ws", None)
        if ws is None or ws.numel() != nb.value or ws.device != u.device:
            ws = torch.empty(nb.value, dtype=torch.uint8, device=u.device)
            self._subgrid_ws = ws
        out = dict(iters=torch.zeros(E, dtype=torch.int32, device=u.device), resnorm=torch.zeros(E, dtype=torch.float64, device=u.device),
                   num_singular=torch.zeros(1, dtype=torch.int32, device=u.device))
        if want_condensed:
            out["schur"] = torch.zeros((E, 24, 24), dtype=torch.float64, device=u.device)
            out["gvec"] = torch.zeros((E, 24), dtype=torch.float64, device=u.device)
        ff = None if farfield is None else _np(farfield, np.float64)
        _check(load_library().mha_swhdg_subgrid_solve(self._h, _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(lam), _ptr(side_types),
                                                      None if ff is None else ff.ctypes.data_as(C.c_void_p), int(max_iter),
                                                      float(tol), _ptr(ws), nb.value, _ptr(out.get("schur")), _ptr(out.get("gvec")),
                                                      _ptr(out["iters"]), _ptr(out["resnorm"]), _ptr(out["num_singular"])))
        return out

    def scatter_local(self, local_J, local_res, res, crs_vals):
        _check(load_library().mha_scatter_local(self._h, _ptr(local_J), _ptr(local_res), _ptr(res), _ptr(crs_vals)))

    def dirichlet_lift(self, u, fixed_soln=None, scalar=0.0):
        """u[row] = fixed_soln[row] (or scalar) on the fixed rows (SolverManager::setDirichlet)."""
        lib = load_library()
        lib.mha_dirichlet_lift.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double]
        _check(lib.mha_dirichlet_lift(self._h, _ptr(u), _ptr(fixed_soln), float(scalar)))

    def apply_dbc_diag(self, crs_vals):
        _check(load_library().mha_apply_dbc_diag(self._h, _ptr(crs_vals)))

    def gather(self, vec, out):
        _check(load_library().mha_gather(self._h, _ptr(vec), _ptr(out)))

    # -- boundary groups -------------------------------------------------------
    def add_boundary_group(self, sidename, bc_type, elem_ids, side_ids):
        e, s_ = _np(elem_ids, np.int32), _np(side_ids, np.int32)
        gid = C.c_int()
        _check(load_library().mha_add_boundary_group(self._h, sidename.encode(), bc_type, len(e),
                                                     e.ctypes.data_as(C.c_void_p), s_.ctypes.data_as(C.c_void_p),
                                                     C.byref(gid)))
        return gid.value

    def compute_flux(self, group_id, u, flux, dflux_du=None, dflux_daux=None, u_prev=None, u_stage=None):
        """<module>::computeFlux on one boundary group (mha_compute_flux): flux [num][nqs] (+ derivative arrays)."""
        lib = load_library()
        lib.mha_compute_flux.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
        _check(lib.mha_compute_flux(self._h, int(group_id), _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(flux), _ptr(dflux_du),
                                    _ptr(dflux_daux)))

    def derived_names(self):
        """<module>::getDerivedNames: ["VM stress", "MAG stress"] on the two elasticity blocks, [] on every other."""
        lib = load_library()
        lib.mha_derived_name.restype = C.c_char_p
        lib.mha_derived_name.argtypes = [C.c_void_p, C.c_int]
        return [lib.mha_derived_name(self._h, k).decode() for k in range(lib.mha_num_derived(self._h))]

    def derived_values(self, u, stress=None):
        """<module>::getDerivedValues at the integration points of every element from the solution u as given (CUDA
        tensor [nrows]).  -> {name: CUDA tensor [E, numip]}; stress: optional CUDA tensor [E, numip, dim, dim] that
        receives the full stress tensor."""
        import torch
        lib = load_library()
        lib.mha_get_derived_values.argtypes = [C.c_void_p] * 5
        shape = (self.info("num_elems"), self.info("num_ip"))
        vm = torch.empty(shape, dtype=torch.float64, device=u.device)  # (the kernel writes every entry)
        mag = torch.empty(shape, dtype=torch.float64, device=u.device)
        _check(lib.mha_get_derived_values(self._h, _ptr(u), _ptr(vm), _ptr(mag), _ptr(stress)))
        return {"VM stress": vm, "MAG stress": mag}

    def add_flux_group(self, sidename, varname, elem_ids, side_ids):
        """The "Flux" condition of PhysicsInterface::fluxConditions for one variable; data = function "Flux <var> <side>"."""
        e, s_ = _np(elem_ids, np.int32), _np(side_ids, np.int32)
        gid = C.c_int()
        _check(load_library().mha_add_flux_group(self._h, sidename.encode(), varname.encode(), len(e),
                                                 e.ctypes.data_as(C.c_void_p), s_.ctypes.data_as(C.c_void_p),
                                                 C.byref(gid)))
        return gid.value

    def add_dirichlet_group(self, sidename, varname, elem_ids, side_ids):
        """Strong Dirichlet entries of one variable (setDirichlet); data = function "Dirichlet <var> <side>"."""
        e, s_ = _np(elem_ids, np.int32), _np(side_ids, np.int32)
        gid = C.c_int()
        _check(load_library().mha_add_dirichlet_group(self._h, sidename.encode(), varname.encode(), len(e),
                                                      e.ctypes.data_as(C.c_void_p), s_.ctypes.data_as(C.c_void_p),
                                                      C.byref(gid)))
        return gid.value

    def set_initial(self, rhs, mass_vals, lump_mass=False):
        """AssemblyManager::setInitial: rhs += (initial, basis), mass_vals += mass matrix (CRS), zero rows -> identity."""
        _check(load_library().mha_set_initial(self._h, int(lump_mass), _ptr(rhs), _ptr(mass_vals)))

    def set_initial_nodal(self, initial):
        """AssemblyManager::setInitial(initial): values of "initial <var>" at the vertices (HGRAD order 1)."""
        _check(load_library().mha_set_initial_nodal(self._h, _ptr(initial)))

    def set_dirichlet(self, rhs, mass_vals, lump_mass=False):
        """AssemblyManager::setDirichlet: boundary mass + data on the fixed rows, identity on the others."""
        _check(load_library().mha_set_dirichlet(self._h, int(lump_mass), _ptr(rhs), _ptr(mass_vals)))

    def clear_boundary_groups(self):
        _check(load_library().mha_clear_boundary_groups(self._h))

    def num_boundary_groups(self):
        return load_library().mha_num_boundary_groups(self._h)

    def assemble_boundary(self, u, res, crs_vals=None, compute_jacobian=True, u_prev=None, u_stage=None, flags=None):
        flags = (1 if compute_jacobian else 0) if flags is None else flags
        _check(load_library().mha_assemble_boundary(self._h, flags, _ptr(u), _ptr(u_prev), _ptr(u_stage), _ptr(res),
                                                    _ptr(crs_vals)))

    def boundary_update(self, gid):
        _check(load_library().mha_boundary_update(self._h, gid))

    def boundary_view(self, gid, name):
        p, ext, rank = C.c_void_p(), (C.c_int64 * 4)(), C.c_int()
        _check(load_library().mha_boundary_view(self._h, gid, name.encode(), C.byref(p), ext, C.byref(rank)))
        return p.value, tuple(ext[k] for k in range(rank.value))

    def boundary_view_numpy(self, gid, name):
        import torch
        ptr, shape = self.boundary_view(gid, name)
        out = np.zeros(shape, np.float64)
        torch.cuda.synchronize()
        rc = _hip_memcpy_dtoh(out.ctypes.data, ptr, out.size * out.itemsize)
        assert rc == 0, rc
        return out

    def set_physics_parameter(self, name, value):
        _check(load_library().mha_set_physics_parameter(self._h, name.encode(), float(value)))

    # -- porousMixed heterogeneous permeability -----------------------------------
    def set_element_data(self, data):
        """Element data [E, ncols] (host array, set_mesh element order; column 0 is the permeability)."""
        d = _np(data, np.float64)
        d = d.reshape(d.shape[0], -1)
        _check(load_library().mha_set_element_data(self._h, d.shape[1], d.ctypes.data_as(C.c_void_p)))

    def import_mesh_data(self, points, values):
        """Each element takes the values row of the data point nearest to its centre.  points [np, dim], values
        [np, ncols] (host arrays).  -> the chosen point of every element (int32 [E])."""
        p, v = _np(points, np.float64), _np(values, np.float64)
        v = v.reshape(p.shape[0], -1)
        seed = np.zeros(self.info("num_elems"), dtype=np.int32)
        _check(load_library().mha_import_mesh_data(self._h, p.shape[0], p.ctypes.data_as(C.c_void_p), v.shape[1],
                                                   v.ctypes.data_as(C.c_void_p), seed.ctypes.data_as(C.c_void_p)))
        return seed

    def set_parameter_vector(self, name, values):
        """"KLUQcoeffs" / "KLStochcoeffs" (host array); takes effect at the next assembly."""
        v = _np(values, np.float64).ravel()
        _check(load_library().mha_set_parameter_vector(self._h, name.encode(), len(v), v.ctypes.data_as(C.c_void_p)))

    # -- workset views ---------------------------------------------------------
    def num_worksets(self):
        return load_library().mha_num_worksets(self._h)

    def workset_update(self, index):
        _check(load_library().mha_workset_update(self._h, index))

    def workset_compute_solution(self, u, u_prev=None, u_stage=None):
        """Workset::computeSoln on the current workset; the fields become views ("e", "grad(e)[x]", "u[x]", "div(u)", ...)."""
        _check(load_library().mha_workset_compute_solution(self._h, _ptr(u), _ptr(u_prev), _ptr(u_stage)))

    def workset_compute_residual(self, u, compute_jacobian=True, u_prev=None, u_stage=None):
        """resetResidual + volumeResidual on the current workset; views "res" and "res.dx"."""
        _check(load_library().mha_workset_compute_residual(self._h, int(compute_jacobian), _ptr(u), _ptr(u_prev),
                                                           _ptr(u_stage)))

    def workset_view(self, name):
        """-> (device pointer, shape tuple)."""
        p, ext, rank = C.c_void_p(), (C.c_int64 * 4)(), C.c_int()
        _check(load_library().mha_workset_view(self._h, name.encode(), C.byref(p), ext, C.byref(rank)))
        return p.value, tuple(ext[k] for k in range(rank.value))

    def workset_view_numpy(self, name):
        """Copy a workset view to the host (tests)."""
        import torch
        ptr, shape = self.workset_view(name)
        is_int = name in ("LIDs", "offsets")
        count = int(np.prod(shape))
        out = np.zeros(shape, np.int32 if is_int else np.float64)
        torch.cuda.synchronize()
        rc = _hip_memcpy_dtoh(out.ctypes.data, ptr, count * out.itemsize)
        assert rc == 0, rc
        return out

    # -- introspection --------------------------------------------------------------
    def info(self, key):
        v = C.c_int64()
        _check(load_library().mha_get_info(self._h, key.encode(), C.byref(v)))
        return v.value

    def set_timing(self, on=True):
        _check(load_library().mha_set_timing(self._h, int(on)))

    def last_kernel_ms(self):
        v = C.c_double()
        _check(load_library().mha_get_last_kernel_ms(self._h, C.byref(v)))
        return v.value


_hip = None


def _hip_memcpy_dtoh(dst_host, src_dev, nbytes):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hip.hipMemcpy(C.c_void_p(dst_host), C.c_void_p(src_dev), nbytes, 2)
