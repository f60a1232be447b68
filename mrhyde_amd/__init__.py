"""mrhyde_amd -- MI355X-native element-local assembly path of MrHyDE.

The product is the C-ABI shared library built from mrhyde_amd/csrc (see
include/mrhyde_amd.h).  This package is a thin ctypes binding used by the
tests, bench.py and __graft_entry__.py: it only moves pointers across the
boundary.  Device memory, streams and torch.distributed come from PyTorch
(plumbing); every computation runs in the HIP kernels.  There is no CPU
fallback: creating a Block without a GPU raises.
"""
from .api import (Sparse3D, MASS_ON_THE_FLY, MASS_LOCAL, MASS_DATABASE, MASS_DATABASE_SPARSE, batched_condense, BASIS_HDIV, BASIS_HGRAD, BASIS_HVOL, BC_NEUMANN, BC_WEAK_DIRICHLET, BC_FLUX, BC_INTERFACE, Newton, NEWTON_SOLVE, NEWTON_BACKTRACKED, NEWTON_DONE, PATH_POINT_ENGINE, PATH_ROW_GATHER, Block, MhaError, ScatterPlan, PATH_AUTO, PATH_ELEMENT_ATOMIC, PATH_LOCAL_THEN_SCATTER, PATH_ROW_OWNER,
                  device_count, lib_path, load_library, mesh_structured, mesh_multi, mesh_swhdg_subgrids, check_swhdg_subgrids, mesh_porous_hybrid, mesh_porous_weak_galerkin, PHYSICS_POROUS_WEAK_GALERKIN, check_dg_lids, module_parameter, MODULE_IDS, PMH_SIDES, PHYSICS_POROUS_MIXED_HYBRIDIZED, row_partition, block_patterns_host_apply, copy_plan_host_apply, block_pattern_copy_plan, block_pattern_rep_plan, block_pattern_step_plan, k1_plan, distinct_shapes, pair_lid_slots, collocation_derivative, porous_direct_plan, porous_database_plan, swhdg_eigendecomp,
                  swhdg_side_terms, version, closest_points, kl_expansion, kl_indices, KL_MAX_TERMS, PHYSICS_IDS, ALL_PHYSICS_IDS, PHYSICS_HELMHOLTZ, PHYSICS_STOKES, PHYSICS_SHALLOWWATER)

__all__ = ["Sparse3D", "MASS_ON_THE_FLY", "MASS_LOCAL", "MASS_DATABASE", "MASS_DATABASE_SPARSE", "batched_condense", "BASIS_HDIV", "BASIS_HGRAD", "BASIS_HVOL", "PATH_POINT_ENGINE", "PATH_ROW_GATHER", "BC_NEUMANN", "BC_WEAK_DIRICHLET", "BC_FLUX", "BC_INTERFACE", "Newton", "NEWTON_SOLVE", "NEWTON_BACKTRACKED", "NEWTON_DONE", "Block", "MhaError", "ScatterPlan", "PATH_AUTO", "PATH_ELEMENT_ATOMIC", "PATH_LOCAL_THEN_SCATTER", "PATH_ROW_OWNER",
           "device_count", "lib_path", "load_library", "mesh_structured", "mesh_multi", "mesh_swhdg_subgrids", "check_swhdg_subgrids", "mesh_porous_hybrid", "mesh_porous_weak_galerkin", "PHYSICS_POROUS_WEAK_GALERKIN", "check_dg_lids", "module_parameter", "MODULE_IDS", "PMH_SIDES", "PHYSICS_POROUS_MIXED_HYBRIDIZED", "row_partition", "block_patterns_host_apply", "copy_plan_host_apply", "block_pattern_copy_plan", "block_pattern_rep_plan", "block_pattern_step_plan", "k1_plan", "distinct_shapes", "pair_lid_slots", "collocation_derivative", "porous_direct_plan", "porous_database_plan", "swhdg_eigendecomp", "swhdg_side_terms", "version", "closest_points", "kl_expansion", "kl_indices", "KL_MAX_TERMS", "PHYSICS_IDS", "ALL_PHYSICS_IDS", "PHYSICS_HELMHOLTZ", "PHYSICS_STOKES", "PHYSICS_SHALLOWWATER"]
