/*
 * mrhyde_amd.h -- C ABI of the MI355X-native element-local assembly path.
 *
 * Drop-in boundary for MrHyDE's AssemblyManager / Workset / PhysicsBase hot
 * path.  Plain pointers and sizes only; every entry
 * point returns an int status (0 = MHA_OK) and sets mha_last_error(); nothing
 * throws across the boundary and nothing calls back into the caller.
 *
 * The reference has no FFI: its boundary is the C++ interface contract
 *   AssemblyManager::assembleJacRes / assembleRes   src/managers/assemblyManager.hpp:173-239
 *   Workset<EvalT> field views                       src/tools/workset.hpp:193-316
 *   PhysicsBase<EvalT>::volumeResidual() etc.        src/physics/physicsBase.hpp:59-85
 * Each entry point below cites the reference routine it replaces (file:line
 * under the reference tree).  INTEGRATION.md shows the adapter a MrHyDE
 * maintainer would add on the reference side.
 *
 * Conventions:
 *  - "host" pointers are read during the call and may be freed afterwards;
 *    "dev" pointers are HIP device pointers owned by the caller (the assembler
 *    never owns res / J, as in the reference).
 *  - LIDs are int32 (LO=int, src/preferences.hpp:40-47) and are consumed
 *    bit-exact; scalars are double (ScalarT).
 *  - the global residual receives -res.val(), the Jacobian +d res(row)/d u(col)
 *    (assemblyManager.cpp:4094,4128); rows with isFixedDOF are skipped (:4075,:4120).
 *  - one HIP stream per context; calls on one context are not thread-safe
 *    (the reference processes worksets sequentially, assemblyManager.cpp:2355).
 */
#ifndef MRHYDE_AMD_H
#define MRHYDE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHA_OK 0
#define MHA_ERR_INVALID 1      /* bad argument / unsupported configuration      */
#define MHA_ERR_STATE 2        /* call order violated (e.g. assemble before mesh) */
#define MHA_ERR_DEVICE 3       /* HIP runtime error (no GPU, launch failure, ...)  */
#define MHA_ERR_UNKNOWN_FIELD 4

typedef struct mha_context mha_context; /* one element block on one GPU        */

const char *mha_last_error(void);
const char *mha_version(void);
/* number of visible HIP devices, or 0 (never fails) */
int mha_device_count(void);

/* ---- block descriptor ---------------------------------------------------
 * replaces: GroupMetaData + Workset construction for one block
 *   src/tools/groupMetaData.hpp:23-129, src/managers/assemblyManager.cpp:272-712
 *   DiscretizationInterface::getBasis/getQuadrature  discretizationInterface.cpp:346-478 */
#define MHA_TOPO_QUAD4 4
#define MHA_TOPO_HEX8 8
#define MHA_BASIS_HGRAD 0   /* Basis_HGRAD_{QUAD,HEX}_Cn_FEM, equispaced   (discretizationInterface.cpp:354-371) */
#define MHA_BASIS_HVOL 1    /* Basis_HVOL_C0_FEM: order 0                   (:372-374)                             */
#define MHA_BASIS_HDIV 2    /* Basis_HDIV_{QUAD,HEX}_In_FEM: order 1        (:375-393)                             */
#define MHA_MAX_VARS 8

typedef struct mha_block_desc {
  int dimension;                 /* 2 or 3                                      */
  int topology;                  /* MHA_TOPO_QUAD4 / MHA_TOPO_HEX8              */
  int num_vars;                  /* thermal: 1 ("e"); porousMixed: 2 ("p","u");
                                    navierstokes: dim+1 ("ux","pr","uy"[,"uz"]);
                                    navierstokes + thermal: dim+2
                                    ("ux","pr","uy"[,"uz"],"e");
                                    linearelasticity: dim ("dx","dy"[,"dz"]);
                                    linearelasticity + thermal: dim+1
                                    ("dx","dy"[,"dz"],"e")                       */
  int basis_type[MHA_MAX_VARS];  /* MHA_BASIS_*, in the module's myvars order    */
  int basis_order[MHA_MAX_VARS]; /* Discretization: order                       */
  int quadrature_degree;         /* Discretization: quadrature (0 => 2*max order,
                                    discretizationInterface.cpp:166)             */
  int workset_size;              /* Solver: workset size (100; <=0 => all,
                                    assemblyManager.cpp:326-332)                 */
  int device;                    /* HIP device ordinal                          */
} mha_block_desc;

int mha_block_create(const mha_block_desc *desc, mha_context **out);
void mha_block_destroy(mha_context *ctx);
/* hipStream_t passed as void*; NULL = the null stream */
int mha_set_stream(mha_context *ctx, void *hip_stream);

/* ---- mesh, maps, graph ---------------------------------------------------
 * replaces: createGroups' LID/node copies (assemblyManager.cpp:656-688),
 * wkset offsets (solverManager.cpp:856-982), createFixedDOFs (assemblyManager.cpp:185-265).
 * nodes[E][nnodes][dim] f64 in the cell topology's (shards) vertex order;
 * lids[E][n] int32; offsets[var][dof] flattened in variable order, values are
 * positions in the element's LID list; is_fixed[nrows] u8 (may be NULL).        */
int mha_set_mesh(mha_context *ctx, int num_elems, const double *nodes_host, const int32_t *lids_host,
                 const int32_t *offsets_host, int num_rows, const uint8_t *is_fixed_host);
/* replaces: OrientTools::modifyBasisByOrientation for lowest-order HDIV face dofs
 * (discretizationInterface.cpp:1021-1027,1055-1061): signs[E][n] int8 (+1/-1) per element and flattened
 * (variable, dof); the caller computes them from Intrepid2::Orientation (:2467).  NULL resets to +1.
 * Call after mha_set_mesh.                                                           */
int mha_set_orientation(mha_context *ctx, const int8_t *signs_host);
/* overlapped CRS graph of the caller (Tpetra local graph: rowptr[nrows+1], colind sorted
 * ascending per row).  Pass NULL/NULL to build it by the reference rule
 * (linearAlgebraInterface.cpp:218-229).                                          */
int mha_set_graph(mha_context *ctx, const int32_t *rowptr_host, const int32_t *colind_host);
int mha_get_graph_sizes(mha_context *ctx, int *num_rows, int64_t *nnz);
int mha_get_graph(mha_context *ctx, int32_t *rowptr_host, int32_t *colind_host);

/* ---- physics module -------------------------------------------------------
 * replaces: PhysicsImporter::import + thermal::defineFunctions
 *   src/physics/physicsImporter.cpp:48-204, src/physics/thermal.cpp:24-66
 * Coefficients are what FunctionManager::evaluate(name,"ip") would return
 * (functionManager.cpp:543-760): a constant, or a per-(elem,ip) array.            */
#define MHA_PHYSICS_THERMAL 1        /* src/physics/thermal.cpp: e (HGRAD)                                   */
#define MHA_PHYSICS_POROUS_MIXED 2   /* src/physics/porousMixed.cpp: p (HVOL 0), u (HDIV 1)                   */
#define MHA_PHYSICS_NAVIERSTOKES 3   /* src/physics/navierstokes.cpp: ux, pr, uy[, uz] (HGRAD)                */
#define MHA_PHYSICS_SHALLOWWATER_HYBRIDIZED 4 /* src/physics/shallowwaterHybridized.cpp: H, Hux, Huy (HGRAD, 2-D):
                                                volumeResidual only; the side terms are mha_swhdg_side_terms */
/* The reference's `modules: navierstokes, thermal` on ONE block (Boussinesq coupling, natural convection).  Variables,
 * all HGRAD, in the order of the reference's variable list when navierstokes is imported before thermal:
 * ux, pr, uy[, uz], e (num_vars = dim + 2).  navierstokes finds "e" (navierstokes::setWorkset, navierstokes.cpp:1026-1046:
 * have_energy) and adds the buoyancy terms density * beta * (e - T_ambient) * source_i to the momentum rows and to their
 * SUPG / PSPG parts (:283-…, 368-…, 471-… in 2-D, :529-…, 619-632, 654-671, 709-722, 744-761, 824-845 in 3-D); thermal
 * finds "ux" (thermal::setWorkset, thermal.cpp:359-379: have_nsvel) and adds (u . grad e, v) (:117-121, 139-149).
 * Functions: the six of navierstokes (navierstokes.cpp:68-74) and "thermal source", "thermal diffusion", "specific heat",
 * "bx", "by", "bz" (thermal.cpp:52-63); "density" is ONE function read by both modules (FunctionManager::addFunction
 * keeps the first tree of a name, functionManager.cpp:48-68).  Parameters: useSUPG, usePSPG, fix_uz_offsets, T_ambient
 * (0), beta (1) (navierstokes.cpp:45-53), "include advection" (0; thermal.cpp:39).  Volume terms only: thermal boundary
 * groups (Neumann, weak Dirichlet, interface) and computeFlux on this block are refused with MHA_ERR_INVALID; strong
 * Dirichlet rows and the generic "Flux" condition work per variable as on every block.  Deck strings in the
 * coordinates are accepted; deck strings that read the solution fields are refused.                              */
#define MHA_PHYSICS_NAVIERSTOKES_THERMAL 5
/* linearelasticity (src/physics/linearelasticity.cpp): displacements dx, dy[, dz], all HGRAD, in that order (:28-39;
 * num_vars = dim, 2-D and 3-D).  Volume terms (:92-240 with computeStress :913-1099): row d gets
 * sum_j sigma_dj d_j v - "source d<x|y|z>" v with sigma = lambda tr(grad u) I + mu (grad u + grad u^T); the parameter
 * "incplanestress" (2-D) replaces the normal stresses by 4 mu d_x dx + 2 mu d_y dy and its mirror (:990-1000).  No
 * time-derivative term.  Functions "lambda" (1), "mu" (0.5), "source dx|dy|dz" (0) (:72-76): constants, arrays,
 * closed forms or deck strings in the coordinates.  Boundary groups (:244-672) act on ALL components of the side:
 * MHA_BC_NEUMANN adds -g_d v with g_d = "Neumann d<x|y|z> <sidename>" (default 0; :361-371); MHA_BC_WEAK_DIRICHLET adds
 * -(sigma n)_d v + penalty (u_d - D_d) v - form_param (b_d . grad v) with D_d = "Dirichlet d<x|y|z> <sidename>",
 * penalty = "penalty" (10) * (lambda + 2 mu) / h, h = (sum of the side weights)^(1/(dim-1)), "form_param" (1) and
 * b_dj = lambda ((u - D) . n) delta_dj + mu ((u - D)_d n_j + (u - D)_j n_d) (:379-386, 437-443, 501-509, 565-573,
 * 628-636); lambda and mu are evaluated at the side points (constants, closed forms or deck strings).  Not built, and
 * refused with MHA_ERR_INVALID: "use crystal elasticity", "Biot", "use Lame parameters" = 0, an "e" variable on the
 * block (the thermoelastic term is MHA_PHYSICS_LINEARELASTICITY_THERMAL), MHA_BC_INTERFACE, mha_compute_flux, 1-D.
 * The stress output is mha_get_derived_values.                                                                    */
#define MHA_PHYSICS_LINEARELASTICITY 6
/* linearelasticity + thermal on one block: the reference's `modules: thermal, linearelasticity` (thermoelastic coupling).
 * Variables dx, dy[, dz], e, all HGRAD, in that order (num_vars = dim + 1; the reference finds them by name); the
 * displacements share one order, e may have its own.  linearelasticity::setWorkset (linearelasticity.cpp:860-906) finds
 * e_num, computeStress (:913-1276) then adds -alpha_T (e - T_ambient) c to every normal stress, c = 3 lambda + 2 mu
 * (:1024-1034, 1074-1084) and c = 5 mu under "incplanestress" in 2-D (:1001-1011).  The e row is thermal's
 * (thermal.cpp:125-163): rho cp de/dt - source, kappa grad e, (b . grad e) with "include advection".  Functions: "lambda"
 * (1), "mu" (0.5), "source dx|dy|dz" (0), "thermal source" (0), "thermal diffusion" (1), "specific heat" (1), "density"
 * (1), "bx", "by", "bz" (0).  Parameters: "incplanestress", "T_ambient" (0), "alpha_T" (1e-6) (:54-58), "include
 * advection"; "form_param" and "penalty" are accepted and unused.  Volume terms on every assembly path, strong Dirichlet
 * rows, the generic "Flux" condition and MHA_BC_NEUMANN (traction on the displacements; e order <= displacement order).
 * Refused with MHA_ERR_INVALID: MHA_BC_WEAK_DIRICHLET and MHA_BC_INTERFACE groups (their side stress needs the
 * thermoelastic term at the side points), thermal's own boundary groups on e, mha_compute_flux,
 * MHA_ASSEMBLE_DETERMINISTIC, deck strings that read solution fields, and the options the plain block refuses.       */
#define MHA_PHYSICS_LINEARELASTICITY_THERMAL 7
/* cdr, convection-diffusion-reaction (src/physics/cdr.cpp): one HGRAD variable c (:22-23), 2-D and 3-D.  Volume terms
 * (:62-142): (c_t + v . grad c + reaction - source) v + diffusion / (density * specific heat) grad c . grad v; no
 * density * specific heat on the time derivative.  Functions and the reference's defaults (:40-48): "source" (0),
 * "diffusion" (1), "specific heat" (1), "density" (1), "reaction" (1), "xvel", "yvel", "zvel" (1 each); "SUPG tau" (0) is
 * accepted and unused, as in the reference (evaluated :82, read by no term; computeTau :186-207 has no caller).  Every
 * function may be a constant, an array, a closed form, a deck string in the coordinates or a deck string that reads the
 * solution fields c, grad(c)[x|y|z], c_t and other named functions (reaction: "0.5*c*c"): the Jacobian then holds the
 * derivative of the string.  boundaryResidual and computeFlux are empty in the reference (:147-164): boundary groups on
 * the block add nothing, mha_compute_flux returns zeros.  Runs on the point engine (MHA_PATH_AUTO / _ROW_GATHER /
 * _POINT_ENGINE / _LOCAL_THEN_SCATTER); MHA_PATH_ROW_OWNER and MHA_ASSEMBLE_DETERMINISTIC are refused.  1-D is refused. */
/* (ids 8 and 9, stated relative to the last id of the list above) */
#define MHA_PHYSICS_CDR (MHA_PHYSICS_LINEARELASTICITY_THERMAL + 1)
/* The reference's `modules: navier stokes, cdr` on ONE block: ux, pr, uy[, uz], c, all HGRAD, each with its own order
 * (num_vars = dim + 2).  The rows of navierstokes (navierstokes.cpp:82-849) and the row of cdr (cdr.cpp:62-142) with no
 * built-in coupling term: the coupling is what cdr's functions read, e.g. xvel = "ux", yvel = "uy".  Functions: "source
 * ux|pr|uy|uz", "viscosity" (navierstokes.cpp:68-74), "source", "diffusion", "specific heat", "reaction", "xvel", "yvel",
 * "zvel", "SUPG tau" (cdr.cpp:40-48), and "density", ONE function read by both modules (functionManager.cpp:48-68).
 * "source pr" is read by no term.  Parameters: useSUPG, usePSPG, fix_uz_offsets.  cdr's functions may read the solution
 * fields of the block; navierstokes' own ("source u*", "density", "viscosity") may not (MHA_ERR_INVALID, by name).
 * Refused with MHA_ERR_INVALID: boundary groups of the modules, mha_compute_flux, MHA_PATH_ROW_OWNER,
 * MHA_ASSEMBLE_DETERMINISTIC, and the 3-D Q2/Q1/Q2/Q2/Q2 element (its LDS need).  Strong Dirichlet rows and the generic
 * "Flux" condition work per variable as on every block.                                                             */
#define MHA_PHYSICS_NAVIERSTOKES_CDR (MHA_PHYSICS_LINEARELASTICITY_THERMAL + 2)
/* helmholtz, the frequency-domain wave module (src/physics/helmholtz.cpp): the complex field as two HGRAD variables
 * ureal, uimag (:24-27) of the SAME order (the reference indexes uimag's basis with ureal's loop index, :155-159;
 * different orders are refused), 2-D and 3-D.  Volume terms (:175-193, the non-fractional branch) with vr = vi = N_i:
 *   row ureal: -omega2r (ur + ui) + omega2i (ui - ur) - (source_r + source_i)   against the test value,
 *              c2r_d (d_d ur + d_d ui) - c2i_d (d_d ui - d_d ur)                against its d-th derivative;
 *   row uimag: -omega2r (ui - ur) - omega2i (ur + ui) - (source_i - source_r),
 *              c2r_d (d_d ui - d_d ur) + c2i_d (d_d ur + d_d ui)
 * -- the reference's own sums of real and imaginary test parts, kept as they are.  No time-derivative term.  Functions,
 * all 0 by default (:41-70): "c2r_x", "c2i_x", "c2r_y", "c2i_y", "c2r_z", "c2i_z", "omega2r", "omega2i", "source_r",
 * "source_i" (constants, arrays, closed forms, deck strings in the coordinates with named helpers); on sides also
 * "robin_alpha_r", "robin_alpha_i", "source_r_side", "source_i_side".  "omegar", "omegai", "alphaHr", "alphaHi",
 * "alphaTr", "alphaTi", "freqExp" are accepted and read by no built term.  A MHA_BC_NEUMANN boundary group is the
 * Robin condition of boundaryResidual (:254-419, non-fractional): alpha u + du/dn - source - c2 du/dn on both rows, its
 * Jacobian holding the N_a (grad N_b . n) blocks between all four variable pairs.  computeFlux is empty in the
 * reference (:430-433): mha_compute_flux returns zeros.  Runs on the point engine (MHA_PATH_AUTO / _ROW_GATHER /
 * _POINT_ENGINE / _LOCAL_THEN_SCATTER) and in the matrix-free products.  Refused with MHA_ERR_INVALID: the parameter
 * "fractional" != 0 (its volume form names 13 functions), 1-D, MHA_PATH_ROW_OWNER, MHA_ASSEMBLE_DETERMINISTIC, deck
 * strings that read the solution fields, weak-Dirichlet and interface groups, and any of the ten volume functions given
 * as a volume MHA_FUNC_IP_ARRAY while a Neumann group exists.                                                        */
#define MHA_PHYSICS_HELMHOLTZ (MHA_PHYSICS_LINEARELASTICITY_THERMAL + 3)
/* porousMixedHybridized, hybridized mixed Darcy flow (src/physics/porousMixedHybridized.cpp; the reference's label is
 * "porousMixedHybrid", the deck's module name "porous mixed hybridized"): p (HVOL 0), u (HDIV-DG 1) and the trace lambda
 * (HFACE 0) of :20-41.  The BLOCK holds p and u, in that order, on 2-D quads and 3-D hexes; lambda, one constant per
 * face, is no block variable: as with shallowwaterHybridized it arrives as data per element, lambda[E][2 dim], and its
 * rows live in the caller's trace system.  The block's LIDs are DG: every LID belongs to exactly one element (checked on
 * the host by the element step, once per mesh; a conforming HDIV map is refused).  Functions (:54-66): "source" (0),
 * "Kinv_xx", "Kinv_yy", "Kinv_zz" (1): constants, arrays, closed forms or deck strings in the coordinates.  Parameter
 * "use permeability data" (:42): Kinv_xx = Kinv_yy = Kinv_zz = 1 / data(elem, 0) of the block's element data, as on
 * porousMixed.  volumeResidual (:72-189) is porousMixed's with total_mobility == 1 and runs on porousMixed's point
 * function with that function pinned to the constant 1: mha_assemble_jacres, mha_compute_local_jacres,
 * mha_apply_jacobian, mha_jacobian_diagonal, mha_get_mass and the workset views (p, u[x], div(u)) work on the block.
 * faceResidual (:287-362, `assemble face terms: true`) on all 2 dim faces of every element is the element step
 * mha_pmh_element_blocks / mha_pmh_condensed_element below.  Dirichlet data enters as the decks give it, `Dirichlet
 * conditions: lambda`: the caller fixes the trace rows (mha_scatter_plan_create, fixed_host) and puts the values into
 * lambda; the step is a Newton residual at the given state, so non-zero data lifts itself.  Refused with
 * MHA_ERR_INVALID: the KL options of porousMixed (the reference module has none), deck strings that read the solution
 * fields, boundary groups of the module (the weak "Dirichlet p" and "interface" branches of boundaryResidual :196-280),
 * mha_compute_flux (:369-408), 1-D, MHA_ASSEMBLE_DETERMINISTIC, a transient state in the element step.  Not built: HDIV
 * or HFACE above lowest order, triangles and tetrahedra, the multiscale interface / "aux p" coupling.                  */
/* (id 12: + 4 stays unassigned, the module-rule tests pin 11 as an id that names no module) */
#define MHA_PHYSICS_POROUS_MIXED_HYBRIDIZED (MHA_PHYSICS_LINEARELASTICITY_THERMAL + 5)
/* porousWeakGalerkin, weak Galerkin Darcy flow (src/physics/porousWeakGalerkin.cpp; the deck's module name is "porous
 * weak Galerkin"): pint (HVOL 0), pbndry (HFACE 0), the weak gradient u (HDIV-DG 1) and the flux t (HDIV-DG 1) of :14-64.
 * The BLOCK holds pint, u and t, in that order, on 2-D quads and 3-D hexes, with DG LIDs (checked on the host by the
 * element step, once per mesh); pbndry, one constant per face, is no block variable: it arrives as data per element,
 * lambda[E][2 dim], and its rows live in the caller's trace system.  Functions (:69-88): "source" (0) and "perm" (1):
 * constants, arrays, closed forms or deck strings in the coordinates.  Parameter "use permeability data" (:58, updatePerm
 * :601-609): perm = data(elem, 0) of the block's element data -- the value itself, not its inverse as in porousMixed; it
 * may stand beside a deck-string source.  volumeResidual (:94-323) runs on the point function porous_wg_point:
 * mha_assemble_jacres, mha_compute_local_jacres, mha_apply_jacobian, mha_apply_jacobian_multi, mha_jacobian_diagonal,
 * mha_get_mass and the workset views (pint, u[x], div(u), t[y], div(t)) work on the block.  faceResidual (:424-505) on all
 * 2 dim faces of every element is the element step mha_pwg_element_blocks / mha_pwg_condensed_element below.  Dirichlet
 * data enters as the decks give it, `Dirichlet conditions: pbndry`: fixed trace rows and the values in lambda.  Refused
 * with MHA_ERR_INVALID: "useAC" other than 0 (HDIV_AC is not built), any order above lowest, KL options and parameter
 * vectors, deck strings that read the solution fields, boundary groups of the module (the weak "Dirichlet pbndry" and
 * "interface" branches of boundaryResidual :329-417), mha_compute_flux (:511-554), 1-D, MHA_ASSEMBLE_DETERMINISTIC,
 * MHA_PATH_ROW_OWNER, a transient state in the element step.  Not built: triangles and tetrahedra, the multiscale
 * interface / "aux pbndry" coupling.  (id 13; 11 stays unassigned, see above) */
#define MHA_PHYSICS_POROUS_WEAK_GALERKIN (MHA_PHYSICS_LINEARELASTICITY_THERMAL + 6)
/* stokes (src/physics/stokes.cpp): ux, pr, uy[, uz], all HGRAD, in that order (:25-41), each with its own order (Q1/Q1
 * with PSPG, Q2/Q1 without), 2-D and 3-D.  Volume terms (:178-438): momentum row i gets -"source u<i>" against the test
 * value and viscosity d_d u_i - delta_id pr against its d-th derivative; the pr row gets div u against the test value.
 * Parameter "usePSPG" (0; :45) adds tau (d_d pr + source_d) against the d-th derivative of the pr test function, with
 * tau = h / (2 viscosity) in 2-D (:256; the h^2 line is commented out there) and h^2 / (2 viscosity) in 3-D (:402);
 * "useLSIC" (0; :44) adds h^2 / (2 viscosity) div u against the SUM of the derivatives of the pr test function (:283,
 * :432).  h is Workset::getElementSize.  No time-derivative term.  Functions (:58-62): "source ux", "source pr", "source
 * uy", "source uz" (0), "viscosity" (1): constants, arrays, closed forms or deck strings in the coordinates; "source pr"
 * is registered and evaluated and read by no term.  boundaryResidual and computeFlux are empty in the reference
 * (:444-456): boundary groups on the block add nothing, mha_compute_flux returns zeros.  The variable layout is
 * navierstokes': every element shape of that module runs, the 3-D Q2/Q1 element included.  Runs on the point engine
 * (MHA_PATH_AUTO / _ROW_GATHER / _POINT_ENGINE / _LOCAL_THEN_SCATTER) and in the matrix-free products.  Refused with
 * MHA_ERR_INVALID: MHA_PATH_ROW_OWNER, MHA_ASSEMBLE_DETERMINISTIC, deck strings that read the solution fields, 1-D.
 * (id 14) */
#define MHA_PHYSICS_STOKES (MHA_PHYSICS_LINEARELASTICITY_THERMAL + 7)
/* shallowwater, the continuous-Galerkin shallow water module (src/physics/shallowwater.cpp): H, Hu, Hv, all HGRAD, in
 * that order (:24-29), 2-D only.  The variable H holds the surface elevation xi; the depth is D = xi + bathymetry.
 * Volume terms (:118-153):
 *   row H:  xi_t - "source H"                                  against the test value, (-Hu, -Hv) against its gradient;
 *   row Hu: Hu_t - gravity xi bathymetry_x - "source Hu"       against the test value,
 *           (-(Hu^2 / D + gravity (D^2 - bathymetry^2) / 2), -Hu Hv / D)          against its gradient;
 *   row Hv: the mirror image with bathymetry_y and "source Hv".
 * A dry point (D = 0) divides by zero as in the reference.  Functions (:47-62): "bathymetry" (1), "bathymetry_x" (0),
 * "bathymetry_y" (0), "source H", "source Hu", "source Hv" (0): constants, arrays, closed forms or deck strings in the
 * coordinates.  "viscosity" (0) and "Coriolis" (0) are evaluated by the reference (:79-80) and read by no term;
 * "bottom friction" (1), "flux left|right|top|bottom", "Neumann source Hu|Hv" (0) and "bathymetry side" are registered and
 * never evaluated: all are accepted and unread here.  Parameters: "gravity" (9.8; :32 -- not shallowwaterHybridized's
 * g = 9.81) and "form_param" (accepted, unused; :34).  boundaryResidual and computeFlux are empty in the reference
 * (:161-174): boundary groups add nothing, mha_compute_flux returns zeros.  Runs on the point engine and in the
 * matrix-free products.  Refused with MHA_ERR_INVALID: 3-D and 1-D, MHA_PATH_ROW_OWNER, MHA_ASSEMBLE_DETERMINISTIC, deck
 * strings that read the solution fields.  (id 15) */
#define MHA_PHYSICS_SHALLOWWATER (MHA_PHYSICS_LINEARELASTICITY_THERMAL + 8)
int mha_physics_select(mha_context *ctx, int physics_id);
#define MHA_FUNC_CONSTANT 0
#define MHA_FUNC_IP_ARRAY 1     /* dev pointer to [E][numip] f64                    */
#define MHA_FUNC_SINPROD 2      /* amp * prod_d sin(freq[d]*x_d), evaluated at ip   */
#define MHA_FUNC_EXPRESSION 3   /* a deck string, see mha_set_function_expression    */
/* thermal: "thermal source","thermal diffusion","specific heat","density" (thermal.cpp:52-63);
 * porousMixed: "source","Kinv_xx","Kinv_yy","Kinv_zz","total_mobility" (porousMixed.cpp:141-151);
 * navierstokes: "source ux","source pr","source uy","source uz","density","viscosity"
 * (navierstokes.cpp:68-74); shallowwaterHybridized: "source H","source Hux","source Huy"
 * (shallowwaterHybridized.cpp:84-88); or a boundary
 * data function "Neumann e <sidename>" / "Dirichlet e <sidename>" (see boundary groups)    */
int mha_set_function(mha_context *ctx, const char *name, int kind, double amp, const double *freq3,
                     const double *ip_array_dev);

/* A function given as the string of the reference's input deck ("Functions:" / boundary-condition entries), e.g.
 * "8*(pi*pi)*sin(2*pi*x)*sin(2*pi*y)": compiled on the host, interpreted at the integration points on the device.
 * replaces: FunctionManager::addFunction + decomposeFunctions + evaluate for position/time expressions
 *   src/managers/functionManager.cpp:60-93, 95-540, 543-860, src/tools/interpreter.cpp.
 * Grammar: numbers; x y z t nx ny nz h pi (functionManager.cpp:21); + - * / ^, unary minus, < > <= >=, parentheses;
 * sin cos tan exp log abs sqrt sinh cosh (:22).  nx ny nz are the unit normal in side functions (Neumann / Dirichlet /
 * flux data) and 0 in volume functions; h is 0 wherever no caller supplies it -- today everywhere, as in the reference,
 * which gives the h leaf no data (:386-404).  Solution fields, other named functions and the view reductions
 * max/min/mean/emax/emin/emean are rejected (MHA_ERR_INVALID).  `t` is the time given to mha_set_time.              */
int mha_set_function_expression(mha_context *ctx, const char *name, const char *expression);
/* syntax / vocabulary check of a deck string without a context (host only, no GPU needed): MHA_OK or MHA_ERR_INVALID */
int mha_check_expression(const char *expression);
/* replaces: Workset::setTime (src/tools/workset.hpp:127): the value of `t` in expressions                         */
int mha_set_time(mha_context *ctx, double time);

/* ---- time integration state -----------------------------------------------
 * replaces: Workset::setDeltat/setStage + butcher/BDF tables consumed by
 * computeSolnTransientSeeded  src/tools/workset.cpp:559-623.  Steady = never call.  */
int mha_set_time_integration(mha_context *ctx, int transient, int num_steps, int num_stages, int stage,
                             double deltat, const double *butcher_A_host, const double *butcher_b_host,
                             const double *bdf_wts_host);

/* ---- assembly --------------------------------------------------------------
 * replaces: AssemblyManager::assembleJacRes<EvalT>  assemblyManager.cpp:2150-2665
 *   (volume loop: performGather :3598, updateWorkset :6512, volumeResidual,
 *    scatter :4031) and assembleRes :2946-3151 (compute_jacobian = 0).
 * u_dev[nrows]; u_prev_dev[nrows][num_steps], u_stage_dev[nrows][num_stages] (transient only).
 * flags: MHA_ASSEMBLE_JACOBIAN (seedwhat = 1: residual and Jacobian; without it the ScalarT
 *   residual-only pass), MHA_ASSEMBLE_OVERWRITE (see below).
 * res_dev[nrows] and crs_vals_dev[nnz] are ACCUMULATED into: the caller zeroes them first, as
 * SolverManager does (solverManager.cpp:1528-1533).  With MHA_ASSEMBLE_OVERWRITE the call stores
 * instead, i.e. it fuses that zeroing (res_over->putScalar(0), J_over->setAllToScalar(0)) into the
 * assembly; use it when this call is the first contribution of the Newton step.
 * crs_vals_dev may be NULL iff the Jacobian is not requested.
 * path: MHA_PATH_AUTO picks the fastest valid kernel; the others force one.          */
#define MHA_ASSEMBLE_JACOBIAN 1
#define MHA_ASSEMBLE_OVERWRITE 2
/* scatter options of AssemblyManager::scatter (assemblyManager.cpp:4124-4133), reproduced as the reference has them:
 * ADJOINT (isAdjoint_): every column of a row receives res(elem,row).fastAccessDx(row); LUMP_MASS (lump_mass_): every
 * column's value is added to the row's diagonal entry (cols[col] = rowIndex).  Both go through the element matrices +
 * row gather (MHA_PATH_AUTO picks it; the fused fast paths do not carry the options).                             */
#define MHA_ASSEMBLE_ADJOINT 4
#define MHA_ASSEMBLE_LUMP_MASS 8
/* DETERMINISTIC: results do not depend on scheduling -- two calls with the same inputs give bit-identical res / crs_vals.
 * (The reference sums element contributions in element order on one thread, or with atomics in any order on a device
 * build, assemblyManager.cpp:4058-4061; the default fast paths here add a row's contributions in an order that depends
 * on wavefront timing, which moves the last bits.)  Available on the affine row-owner path (MHA_PATH_AUTO /
 * MHA_PATH_ROW_OWNER on affine elements with constant coefficients): the Jacobian rows are register sums in a fixed order
 * (kernels/block_pattern.hip) and the residual entries are summed pair by pair in pair order by the row's owner
 * (kernels/thermal_general_row_owner.hip, residual-only, ordered) instead of the thread-per-element kernel's atomics;
 * MHA_ERR_INVALID where that combination does not exist.  Slower: the residual costs ~1 ms more at config 2.          */
#define MHA_ASSEMBLE_DETERMINISTIC 16
#define MHA_PATH_AUTO 0
#define MHA_PATH_ELEMENT_ATOMIC 1 /* per-element kernel, atomic scatter (reference's
                                     fused "assembly insert Jac" with useAtomics)     */
#define MHA_PATH_ROW_OWNER 2      /* fused row-owner kernel, no global atomics           */
#define MHA_PATH_LOCAL_THEN_SCATTER 3 /* updateJac/updateRes then scatterJac/scatterRes   */
#define MHA_PATH_POINT_ENGINE 4   /* multi-variable kernel: point-level forward AD + B^T C B
                                     contraction, atomic scatter; the path of porousMixed and
                                     navierstokes, available to thermal as a cross-check    */
#define MHA_PATH_ROW_GATHER 5     /* element kernel -> dense element matrices (device scratch,
                                     E*n*n doubles) -> every CRS row summed by one wavefront from
                                     its incident elements: no global atomics; AUTO for
                                     porousMixed / navierstokes                                */
int mha_assemble_jacres(mha_context *ctx, int flags, int path, const double *u_dev,
                        const double *u_prev_dev, const double *u_stage_dev, double *res_dev,
                        double *crs_vals_dev);
/* replaces: updateJac / updateRes  assemblyManager.cpp:7412-7455, 7115-7152
 * local_J_dev[E][n][n] += res(e,r).dx(c), local_res_dev[E][n] -= res(e,r).val()      */
int mha_compute_local_jacres(mha_context *ctx, int compute_jacobian, const double *u_dev,
                             const double *u_prev_dev, const double *u_stage_dev, double *local_J_dev,
                             double *local_res_dev);
/* replaces: getMass / getWeightedMass  assemblyManager.cpp:7776-7840, 7847-7925: dense element mass matrices
 * local_mass_dev[E][n][n] += sum_q basis_v(i,q) . basis_v(j,q) wts(q) * masswts[v] at (offsets(v,i), offsets(v,j)),
 * every variable of the block (HGRAD / HVOL values, HDIV vector values); masswts_host[num_vars] or NULL (= 1).
 * mha_scatter_local turns them into CRS values.                                                          */
int mha_get_mass(mha_context *ctx, const double *masswts_host, double *local_mass_dev);
/* ---- mass storage and the matrix-free mass apply ----------------------------------------------------------------
 * Sparse3DView (src/tools/sparse3DView.hpp:21-161): compressed storage of dense element matrices dense_dev[E][n][n]:
 * the entries with |a| / max|a| > tol, row by row in column order.  Device-resident; mha_sparse3d_views returns
 * values_dev[E][n][maxent] (f64), columns_dev[E][n][maxent] (int32, local column = position in the element's LID list)
 * and nnz_row_dev[E][n] (int32) -- getValues / getColumns / getNNZPerRow; mha_sparse3d_size = size().  Stateless.   */
typedef struct mha_sparse3d mha_sparse3d;
int mha_sparse3d_create(int64_t num_elems, int n, const double *dense_dev, double tol, void *hip_stream, mha_sparse3d **out);
int mha_sparse3d_views(mha_sparse3d *s, int *maxent, double **values_dev, int32_t **columns_dev, int32_t **nnz_row_dev);
int mha_sparse3d_size(mha_sparse3d *s, int64_t *total_nnz);
void mha_sparse3d_destroy(mha_sparse3d *s);
/* The basis database (AssemblyManager::identifyVolumetricDatabase, assemblyManager.cpp:4314-4467): elements that share
 * their geometry share one set of stored data (basis, mass).  The reference scans earlier representatives and accepts
 * relative differences below "database TOL" (1e-10) in measure and Jacobians; here the match is EXACT -- bit-identical
 * vertex offsets from the element's first vertex and identical orientation signs (found by hashing: O(E), not O(E U)),
 * which is the subset of the reference's matches that substitutes nothing: results are unchanged to rounding.
 * Representatives are numbered in order of first appearance, as in the reference.  index_host[E] (basis_index),
 * first_users_host[num_unique] (element id of every representative); either may be NULL.                          */
int mha_database_build(mha_context *ctx, int *num_unique);
int mha_database_get(mha_context *ctx, int32_t *index_host, int32_t *first_users_host);
/* AssemblyManager::applyMassMatrixFree (assemblyManager.cpp:1582-1778): y_dev += M x_dev with M block diagonal by
 * variable, never assembled.  masswts_host[num_vars] or NULL (= 1; physics->mass_wts).  mode:
 *   MHA_MASS_ON_THE_FLY   basis and weights recomputed per element (the !storeMass branch :1607-1672); mass_dev, sparse NULL
 *   MHA_MASS_LOCAL        mass_dev[E][n][n], e.g. from mha_get_mass (:1760-1772)
 *   MHA_MASS_DATABASE     mass_dev[num_unique][n][n] of the database representatives + basis_index (:1730-1755)
 *   MHA_MASS_DATABASE_SPARSE  the same in Sparse3DView storage (:1690-1726; "sparse mass format")
 * masswts applies to MHA_MASS_ON_THE_FLY only (stored masses carry their weights, as in the reference).            */
#define MHA_MASS_ON_THE_FLY 0
#define MHA_MASS_LOCAL 1
#define MHA_MASS_DATABASE 2
#define MHA_MASS_DATABASE_SPARSE 3
int mha_apply_mass_matrix_free(mha_context *ctx, int mode, const double *masswts_host, const double *mass_dev,
                               mha_sparse3d *sparse, const double *x_dev, double *y_dev);
/* ---- matrix-free Jacobian products ------------------------------------------------------------------------------
 * y_dev (+)= A x_dev or, with MHA_APPLY_TRANSPOSE, y_dev (+)= A^T x_dev, where A is the matrix that
 * mha_assemble_jacres(ctx, MHA_ASSEMBLE_JACOBIAN | MHA_ASSEMBLE_OVERWRITE, MHA_PATH_AUTO, u, u_prev, u_stage, ...) stores in
 * crs_vals: the volume terms with the block's current time-integration seeding, zero rows where the mesh marks a row
 * fixed, no mha_apply_dbc_diag -- sign +dR/du (the sign of crs_vals, not the -R of res).  Replaces the product with the
 * matrix of AssemblyManager::assembleJacRes (a Krylov solver's J x, an adjoint solve's J^T x): neither A nor an element
 * matrix is formed; the module's point function is evaluated once per integration point (forward) or once per point and
 * slot (transposed) (kernels/jacobian_apply.hip).  The reference has no counterpart beyond applyMassMatrixFree: its
 * Jacobian exists as a CRS matrix only.  Every module of the point engine (thermal, porousMixed, navierstokes,
 * navierstokes+thermal, linearelasticity, linearelasticity+thermal, cdr, navierstokes+cdr, the volume terms of
 * shallowwaterHybridized); thermal runs through its point function here, as under MHA_PATH_POINT_ENGINE.
 * x_dev[nrows], y_dev[nrows] (a residual-like overlapped vector: shared rows take the Export(ADD) of res).  The forward
 * product skips fixed rows of y; the transposed product reads x as zero on fixed rows and writes every row.
 * flags: MHA_ASSEMBLE_OVERWRITE (y is zeroed on the block's stream first; otherwise accumulated into) and
 * MHA_APPLY_TRANSPOSE; any other bit, a missing mesh / module / graph and a null x or y give MHA_ERR_INVALID, and so do
 * the refusals of the modules' own validation (e.g. a deck string that reads solution fields on a module without that
 * form).  A refused call writes nothing to y.  No allocation and no host synchronisation (beyond mha_set_timing's).
 * diag(A): mha_jacobian_diagonal; several vectors per call: mha_apply_jacobian_multi (below).
 * Boundary-group terms: mha_apply_boundary_jacobian on the same y, after this call (below).
 * Not built: block diagonals, the HDG element / trace blocks, the wiring into the Newton driver.                     */
#define MHA_APPLY_TRANSPOSE 32
int mha_apply_jacobian(mha_context *ctx, int flags, const double *u_dev, const double *u_prev_dev,
                       const double *u_stage_dev, const double *x_dev, double *y_dev);
/* d_dev[nrows] (+)= diag(A) with the matrix A of mha_apply_jacobian -- volume terms, the current seeding, the sign of
 * crs_vals, zero on the rows the mesh marks fixed (d is exactly 0 there under MHA_ASSEMBLE_OVERWRITE), no
 * mha_apply_dbc_diag -- without the matrix: what a Jacobi or Chebyshev smoother of a matrix-free Krylov solve is built
 * from.  One point-function evaluation per integration point and slot, as in the transposed product; per dof the block
 * of its own variable is contracted with the dof's basis values on both sides (kernels/jacobian_diagonal.hip).  d is
 * a residual-like overlapped vector: shared rows take the Export(ADD) of res.  A is zero, and so is d, on fixed rows and
 * on rows the module leaves empty (pressure without PSPG, the uz rows under the uz-offset quirk): a Jacobi user gives
 * those a value of their own.  flags: MHA_ASSEMBLE_OVERWRITE only (d is zeroed on the block's stream first; otherwise
 * accumulated into); any other bit, a missing mesh / module / graph, a null d and the refusals of the modules' own
 * validation give MHA_ERR_INVALID with d untouched.  No allocation and no host synchronisation.  The reference has no
 * counterpart.  Boundary-group terms: mha_boundary_jacobian_diagonal on the same d.  Not built: block diagonals.       */
int mha_jacobian_diagonal(mha_context *ctx, int flags, const double *u_dev, const double *u_prev_dev,
                          const double *u_stage_dev, double *d_dev);
/* Y_k (+)= A X_k or, with MHA_APPLY_TRANSPOSE, A^T X_k for k = 0 .. nvec-1 with the matrix A and the flags of
 * mha_apply_jacobian.  Vector k is x_dev + k ldx (y_dev + k ldy), nrows entries each -- the layout of a Krylov basis;
 * ldx, ldy >= nrows.  What does not depend on the vector -- the gather of u, the geometry, the fields of u and, in the
 * transposed product, the point-function evaluations -- is paid once per launch, and the forward product fills the
 * lanes the single call leaves idle with the other vectors (kernels/jacobian_apply_multi.hip).  One launch carries up
 * to MHA_APPLY_MAX_VECTORS vectors (fewer where the LDS of the element shape says so: mha_info
 * "jacobian_apply_vectors"); any nvec >= 1 is taken, in passes.  Fixed rows as in the single call: the forward product
 * skips them in every Y_k, the transposed product reads X_k as zero there.  MHA_ASSEMBLE_OVERWRITE zeroes Y_k[0, nrows)
 * only: the padding between vectors is never written.  nvec < 1, ldx or ldy < nrows, a null pointer and everything
 * mha_apply_jacobian refuses give MHA_ERR_INVALID with Y untouched.  No allocation and no host synchronisation.      */
#define MHA_APPLY_MAX_VECTORS 8     /* vectors one launch carries; more are taken in passes */
int mha_apply_jacobian_multi(mha_context *ctx, int flags, const double *u_dev, const double *u_prev_dev,
                             const double *u_stage_dev, int nvec, const double *x_dev, int64_t ldx,
                             double *y_dev, int64_t ldy);
/* ---- matrix-free boundary-group products ---------------------------------------------------------------------------
 * y_dev += A_b x_dev or, with MHA_APPLY_TRANSPOSE, y_dev += A_b^T x_dev, and d_dev += diag(A_b), where A_b is exactly the
 * matrix that mha_assemble_boundary(ctx, MHA_ASSEMBLE_JACOBIAN, ...) adds into crs_vals: summed over the block's groups,
 * the same sign and alpha_u seeding, zero rows where the mesh marks a row fixed.  Neither A_b nor an entry matrix is
 * formed and the CRS graph is not read (it must be set, as for mha_assemble_boundary): per (element, side) entry the
 * module's point form between (variable, slot) pairs is applied to the trial fields at the side points
 * (kernels/boundary_forms.hpp, kernels/boundary_apply.hip) -- O(n nqs) work and n atomics per entry where the assembly
 * takes O(n^2 nqs), n^2 atomics and a column search.  The calls always accumulate, as mha_assemble_boundary does: run
 * mha_apply_jacobian(MHA_ASSEMBLE_OVERWRITE) first and this call on the same y for the operator of the whole problem.
 * The forward product does not touch fixed rows of y, the transposed product reads x as zero on fixed rows, the diagonal
 * adds nothing on fixed rows.  Groups with a Jacobian: thermal MHA_BC_WEAK_DIRICHLET / _INTERFACE, linearelasticity
 * MHA_BC_WEAK_DIRICHLET, helmholtz MHA_BC_NEUMANN (Robin), shallowwaterHybridized MHA_BC_SWH_*.  Every other group
 * (Neumann data, porousMixed, the thermoelastic traction, flux and strong-Dirichlet groups, cdr) is passed over without a
 * launch; a block without groups returns MHA_OK with the output untouched.  flags: MHA_APPLY_TRANSPOSE for the product, 0
 * for the diagonal; any other bit (MHA_ASSEMBLE_OVERWRITE and MHA_ASSEMBLE_DETERMINISTIC among them) and a null x, y or d
 * give MHA_ERR_INVALID.  Everything mha_assemble_boundary refuses is refused here -- a missing mesh / module / graph, a
 * group the module has no term for (with the group's name), the module's own validation, the kernel's limits -- before
 * anything is written.  No allocation and no host synchronisation (beyond mha_set_timing's).  mha_get_info
 * "boundary_apply_lds_bytes": LDS per workgroup of the largest launch of the last call.
 * Not built: several vectors per call, the wiring into the Newton driver, the HDG element / trace blocks, a
 * deterministic variant.                                                                                              */
int mha_apply_boundary_jacobian(mha_context *ctx, int flags, const double *u_dev, const double *u_prev_dev,
                                const double *u_stage_dev, const double *x_dev, double *y_dev);
int mha_boundary_jacobian_diagonal(mha_context *ctx, int flags, const double *u_dev, const double *u_prev_dev,
                                   const double *u_stage_dev, double *d_dev);
/* replaces: scatterJac / scatterRes  assemblyManager.cpp:3882-3935, 3943-3978          */
int mha_scatter_local(mha_context *ctx, const double *local_J_dev, const double *local_res_dev,
                      double *res_dev, double *crs_vals_dev);
/* replaces: dofConstraints -> updateJacDBC  assemblyManager.cpp:3158-3187, 1166-1179   */
int mha_apply_dbc_diag(mha_context *ctx, double *crs_vals_dev);
/* replaces: performGather  assemblyManager.cpp:3598-3643: out[E][n] (dof order = basis order) */
int mha_gather(mha_context *ctx, const double *vec_dev, double *elem_vals_dev);

/* ---- the nonlinear-solve protocol around the assembler --------------------------------------------------------------
 * replaces: the loop of SolverManager::nonlinearSolver (src/managers/solverManager.cpp:1465-1709) around assembleRes /
 * assembleJacRes, and the strong-Dirichlet lifting of SolverManager::setDirichlet (:1876-1957).  The linear solver, the
 * Export / Import between ranks and the all-reduce of the norm stay with the caller (out of scope: SURVEY.md section 2);
 * the driver is a state machine stepped with plain calls, no callbacks:
 *   mha_newton_residual : zero res_dev; assembleRes (AUTOTUNE: the residual-only ScalarT path first, :1538-1552) incl. the
 *                         boundary groups -> res_dev = -res.val()                    [caller: Export(ADD) of res_dev]
 *   mha_newton_norm     : |res_dev|_inf of this rank's rows (:1571)                  [caller: all-reduce max]
 *   mha_newton_decide   : iteration 0 fixes resnorm_first; resnorm_scaled = resnorm / resnorm_first (:1575-1581);
 *                         backtracking when allowed and the scaled norm exceeds 1.1: alpha halved, u -= alpha du (the last
 *                         update), no solve (:1591-1616); relative tolerance (scaled < nl_tol, or resnorm < 1e-100) or
 *                         absolute tolerance ends the loop (:1617-1632); *action = MHA_NEWTON_SOLVE / _BACKTRACKED / _DONE
 *   mha_newton_jacobian : only when a solve is needed (:1638-1641): zero res_dev, assembleJacRes (+ boundary groups) with
 *                         the CRS values overwritten, unit diagonal on the fixed rows  [caller: Export(ADD) of the matrix,
 *                         solve J du = res, Import du]
 *   mha_newton_update   : u += alpha du with alpha = 1 (:1656-1672); closes the iteration (NLiter++, :1681-1685)
 *   mha_newton_step     : residual + norm + decide (+ jacobian) in one call for a single-rank caller.
 * autotune = 0: assembleJacRes at once, as the reference does for adjoint / multiscale runs (:1540-1547).
 * mha_newton_state: iteration count, norms, alpha, status (1: the iteration limit was reached without convergence).
 * mha_dirichlet_lift: u[row] = fixed_soln_dev[row] (or scalar_value when fixed_soln_dev is NULL) on the rows the mesh
 * marks fixed -- the lifted solution carries the strong boundary condition (:1905-1935).                              */
#define MHA_NEWTON_SOLVE 1
#define MHA_NEWTON_BACKTRACKED 2
#define MHA_NEWTON_DONE 3
typedef struct mha_newton mha_newton;
int mha_newton_create(mha_context *ctx, int max_iter, double nl_tol, double nl_abs_tol, int use_relative, int use_absolute,
                      int allow_backtracking, int autotune, mha_newton **out);
void mha_newton_destroy(mha_newton *nw);
int mha_newton_reset(mha_newton *nw);
int mha_newton_residual(mha_newton *nw, const double *u_dev, const double *u_prev_dev, const double *u_stage_dev,
                        double *res_dev);
int mha_newton_norm(mha_newton *nw, const double *res_dev, double *resnorm);
int mha_newton_decide(mha_newton *nw, double resnorm, double *u_dev, int *action);
int mha_newton_jacobian(mha_newton *nw, const double *u_dev, const double *u_prev_dev, const double *u_stage_dev,
                        double *res_dev, double *crs_vals_dev);
int mha_newton_update(mha_newton *nw, double *u_dev, const double *du_dev);
int mha_newton_step(mha_newton *nw, double *u_dev, const double *u_prev_dev, const double *u_stage_dev, double *res_dev,
                    double *crs_vals_dev, int *action);
int mha_newton_state(const mha_newton *nw, int *iteration, double *resnorm, double *resnorm_scaled, double *resnorm_first,
                     double *alpha, int *status);
int mha_dirichlet_lift(mha_context *ctx, double *u_dev, const double *fixed_soln_dev, double scalar_value);

/* ---- workset views -----------------------------------------------------------
 * replaces: updateWorkset aliasing the group's stored views (assemblyManager.cpp:6512-6596)
 * and Group::computeBasis -> getPhysicalVolumetricBasis / getPhysicalIntegrationData
 *   src/tools/group.cpp:134-243, discretizationInterface.cpp:732-776, 898-1127.
 * mha_workset_update evaluates the views for workset `index` (elements
 * [index*ws, min((index+1)*ws, E))) on the device; mha_workset_view returns a
 * device pointer + extents (LayoutRight) valid until the next update.
 * names: "basis" (numElem,n,numip,1)  "basis_grad" (numElem,n,numip,dim)
 *        "wts" (numElem,numip)  "x","y","z" (numElem,numip)  "LIDs" (numElem,n) int32
 *        "offsets" (numvars, maxdof) int32
 * per variable (any block; <var> is the module's variable name, "var<k>" without a module):
 *   "basis <var>" (numElem,card,numip,ncomp)   getBasis(var)      workset.hpp:241   ncomp = dim for HDIV (Piola
 *                                              value J phi / detJ, orientation sign applied), 1 for HGRAD / HVOL
 *   "basis_grad <var>" (numElem,card,numip,dim) getBasisGrad(var) workset.hpp:249   HGRAD
 *   "basis_div <var>" (numElem,card,numip)      getBasisDiv(var)  workset.hpp:270   HDIV
 *   (discretizationInterface.cpp:898-1127; "basis"/"basis_grad" without a name: single-variable HGRAD blocks)
 * mha_workset_compute_solution: Workset::computeSoln on the current workset (workset.cpp:1017-1190) from
 *   u / u_prev / u_stage with the transient seeding of :589-623; afterwards the solution fields are views
 *   (numElem,numip) under the reference's names -- getSolutionField (workset.hpp:229): "<var>", "<var>_t",
 *   "grad(<var>)[x|y|z]" (HGRAD), "<var>[x|y|z]", "<var>_t[x|y|z]", "div(<var>)" (HDIV).  The views hold the
 *   fields' values; their derivative arrays never leave the chip (d field / d u_j = alpha_u * basis).
 * mha_workset_compute_residual: resetResidual + volumeResidual on the current workset (what assembleJacRes does
 *   between updateWorkset and scatter, assemblyManager.cpp:2426-2440); afterwards "res" (numElem,n) = res(e,i).val()
 *   and, with compute_jacobian, "res.dx" (numElem,n,n) = res(e,i).fastAccessDx(j) -- getResidual (workset.hpp:193),
 *   i, j = positions in the element's LID list.
 * unknown names: MHA_ERR_UNKNOWN_FIELD (the reference prints and continues,
 * workset.cpp:1576-1577).                                                             */
int mha_num_worksets(mha_context *ctx);
int mha_workset_update(mha_context *ctx, int index);
int mha_workset_view(mha_context *ctx, const char *name, void **dev_ptr, int64_t extents[4], int *rank);
int mha_workset_compute_solution(mha_context *ctx, const double *u_dev, const double *u_prev_dev,
                                 const double *u_stage_dev);
int mha_workset_compute_residual(mha_context *ctx, int compute_jacobian, const double *u_dev,
                                 const double *u_prev_dev, const double *u_stage_dev);

/* ---- boundary groups -----------------------------------------------------------
 * replaces: BoundaryGroup (src/tools/boundaryGroup.hpp:23-186, boundaryGroup.cpp:25-178), the
 * boundary-group loop of assembleJacRes (assemblyManager.cpp:2518-2638: updateWorksetBoundary :5646-5710,
 * performBoundaryGather :3650-3700, boundaryResidual, scatter), side integration data
 * (discretizationInterface.cpp:1608-1790, 1810-1955) and thermal::boundaryResidual
 * (src/physics/thermal.cpp:172-281).
 * A group = the (element, local side) entries of one side set that carry one boundary-condition
 * type for the variable; local side ids are the cell topology's (shards): quad edges
 * {0,1},{1,2},{2,3},{3,0}; hex faces {0,1,5,4},{1,2,6,5},{2,3,7,6},{0,4,7,3},{0,3,2,1},{4,5,6,7}.
 * The boundary data is the function "Neumann e <sidename>" / "Dirichlet e <sidename>"
 * (thermal.cpp:217,238) registered with mha_set_function; an MHA_FUNC_IP_ARRAY for it is a
 * dev array [num_sides][side numip].  Strong Dirichlet needs no group (is_fixed rows).
 * mha_assemble_boundary ACCUMULATES all groups into res / crs_vals (call after the volume
 * assembly of the same Newton step; MHA_ASSEMBLE_OVERWRITE is rejected).
 * mha_boundary_update / mha_boundary_view expose the side data the reference keeps in the
 * workset: "wts side" (num,numip) "x","y","z" (num,numip) "n[x]","n[y]","n[z]" (num,numip)
 * "basis side" (num,n,numip,1) "basis_grad side" (num,n,numip,dim); per variable on any block
 * (getBasisSide(var) / getBasisGradSide(var), workset.hpp:281-293; getPhysicalBoundaryBasis,
 * discretizationInterface.cpp:1840-1950): "basis side <var>" (num,card,numip,ncomp), "basis_grad side <var>".
 * mha_add_flux_group: the generic "Flux" condition of PhysicsInterface::fluxConditions
 * (src/interfaces/physicsInterface.cpp:1702-1762) for one variable of any block on one side set:
 * res(elem, off(dof)) += -flux * wts side * basis side(elem,dof,pt,0) with flux = the function
 * "Flux <var> <sidename>" at the side points (constant, closed form, expression in x,y,z,t,nx,ny,nz, or a dev
 * array [num_sides][side numip]); no Jacobian contribution.  mha_assemble_boundary runs it with the other groups. */
#define MHA_BC_NEUMANN 1
#define MHA_BC_WEAK_DIRICHLET 2
#define MHA_BC_FLUX 3
#define MHA_BC_INTERFACE 5 /* thermal: the weak-Dirichlet branch with the trace, the function "aux e <sidename>", as data (thermal.cpp:227-243) */
#define MHA_BC_DIRICHLET 4 /* strong condition (mha_add_dirichlet_group): nothing in mha_assemble_boundary, see mha_set_dirichlet */
/* linearelasticity: a group's type holds for ALL components of the side (linearelasticity.cpp:244-672); MHA_BC_NEUMANN reads
 * "Neumann dx|dy|dz <sidename>" (:361-371), MHA_BC_WEAK_DIRICHLET "Dirichlet dx|dy|dz <sidename>" (:372-390, 430-447, 493-513,
 * 557-577, 620-640); MHA_BC_INTERFACE and mha_compute_flux are refused on that block (see MHA_PHYSICS_LINEARELASTICITY).
 * linearelasticity + thermal: MHA_BC_NEUMANN only (traction on dx, dy[, dz]; see MHA_PHYSICS_LINEARELASTICITY_THERMAL). */
/* shallowwaterHybridized side types (bcs(H_num, side): "interface", "Far-field", "Slip",
 * shallowwaterHybridized.cpp:286-300, 612-620): the group's entries are element sides (all four sides of every
 * element for the HDG interior problem); the trace state comes from the functions "aux H <sidename>",
 * "aux Hux <sidename>", "aux Huy <sidename>" (constants or dev arrays [num_sides][side numip]), the far-field state
 * from "Far-field H <sidename>", ... (:648-653).  mha_assemble_boundary adds boundaryResidual (:190-263) and its
 * derivative with respect to the interior unknowns; settings "Roe-like stabilization" (default 1; 0 = max EV), "g". */
#define MHA_BC_SWH_INTERFACE 10
#define MHA_BC_SWH_FARFIELD 11
#define MHA_BC_SWH_SLIP 12
int mha_add_boundary_group(mha_context *ctx, const char *sidename, int bc_type, int num_sides,
                           const int32_t *elem_ids_host, const int32_t *local_side_ids_host, int *group_id);
int mha_add_flux_group(mha_context *ctx, const char *sidename, const char *varname, int num_sides,
                       const int32_t *elem_ids_host, const int32_t *local_side_ids_host, int *group_id);
int mha_clear_boundary_groups(mha_context *ctx);

/* ---- L2-projection systems of initial and strong-Dirichlet data -------------------------------------------------
 * The caller solves mass * x = rhs (the reference hands both to its linear solver, solverManager.cpp:1876-1957);
 * building them is the assembly manager's part.  mass_vals_dev / rhs_dev are ACCUMULATED into (zero them first).
 *
 * mha_set_initial replaces AssemblyManager::setInitial(set, rhs, mass, useadjoint, lumpmass, scale)
 *   (src/managers/assemblyManager.cpp:1185-1305) with getInitial(project = true) (:7632-7682), getMass (:7776-7840) and
 *   PhysicsInterface::getInitial (src/interfaces/physicsInterface.cpp:898-958):
 *     rhs[LIDs(e, off_v(i))] += sum_q init_v(e,q) . basis_v(e,i,q) wts(e,q)            (no sign change, fixed rows too)
 *     mass(LIDs(e, off_v(i)), LIDs(e, off_v(j))) += sum_q basis_v(e,i,q) . basis_v(e,j,q) wts(e,q); with lump_mass
 *     every entry goes to the diagonal; afterwards rows with sum |a| < 1e-14 get a one on the diagonal (:1284-1302).
 *   Data = the functions "initial <var>" (HGRAD / HVOL) or "initial <var>[x]", "[y]", "[z]" (HDIV) registered with
 *   mha_set_function / mha_set_function_expression (MHA_FUNC_IP_ARRAY: [E][numip]).
 * mha_set_initial_nodal replaces AssemblyManager::setInitial(set, initial, useadjoint) (:1830-1850) with
 *   getInitial(project = false) (:7683-7727): initial[LIDs(e, off_v(k))] = "initial <var>" at vertex k of element e
 *   (replaceLocalValue).  As in the reference this is for HGRAD variables of order 1 only: MHA_ERR_INVALID otherwise.
 *   (MHA_FUNC_IP_ARRAY here: [E][vertices per element].)
 * mha_add_dirichlet_group + mha_set_dirichlet replace AssemblyManager::setDirichlet (:1855-1943) with
 *   getDirichletBoundary (:6288-6350), getMassBoundary (:6360-6425) and PhysicsInterface::getDirichlet
 *   (physicsInterface.cpp:1065-1083): for every entry of the groups whose variable carries "Dirichlet" on the side set,
 *   and only in rows with is_fixed,
 *     rhs[row] += sum_pt D(k,pt) basis side(k,i,pt,0) wts side(k,pt)        HGRAD / HVOL
 *              += sum_pt D(k,pt) sum_c basis side(k,i,pt,c) n_c(k,pt) wts   HDIV
 *     mass(row, LIDs(e, off_v(j))) += sum_pt basis side_i basis side_j wts  (HDIV: sum_c b_i,c n_c b_j,c n_c wts, :6400-6408)
 *   with D = the function "Dirichlet <var> <sidename>" at the side points; every row that is NOT fixed and is touched
 *   by an element gets a one on its diagonal (replaceValues, :1920-1938).  With lump_mass the reference adds the row total
 *   to the column of the LAST entry of the element's LID list, not to the diagonal (the `cols[0]` its summing loop leaves
 *   behind, :1888-1897); reproduced as it is.                                                                        */
int mha_add_dirichlet_group(mha_context *ctx, const char *sidename, const char *varname, int num_sides,
                            const int32_t *elem_ids_host, const int32_t *local_side_ids_host, int *group_id);
int mha_set_initial(mha_context *ctx, int lump_mass, double *rhs_dev, double *mass_vals_dev);
int mha_set_initial_nodal(mha_context *ctx, double *initial_dev);
int mha_set_dirichlet(mha_context *ctx, int lump_mass, double *rhs_dev, double *mass_vals_dev);

int mha_num_boundary_groups(mha_context *ctx);
int mha_assemble_boundary(mha_context *ctx, int flags, const double *u_dev, const double *u_prev_dev,
                          const double *u_stage_dev, double *res_dev, double *crs_vals_dev);
/* computeFlux of the block's module on one boundary group: the workset's flux view (elem, auxvar, pt).
 * replaces: AssemblyManager::computeFlux -> PhysicsInterface::computeFlux -> <module>::computeFlux
 *   (src/managers/assemblyManager.hpp:573-727; called by SubGridDtN_Solver::updateFlux, subgridDtN_solver.cpp:1579)
 *   thermal (src/physics/thermal.cpp:288-347):       flux = (10 / h) kappa (lambda - T) + kappa grad T . n, lambda = the
 *                                                    function "aux e <sidename>" at the side points, h = side element size
 *   porousMixed (src/physics/porousMixed.cpp:440-500): flux = u . n (HDIV side basis, Piola, orientation sign)
 *   navierstokes (src/physics/navierstokes.cpp:1016-1018): empty in the reference: zeros
 *   shallowwaterHybridized: mha_swhdg_side_terms / mha_swhdg_element_blocks (trace rows).
 * flux_dev[num][nqs]; optional derivative arrays (what the AD type of the reference's view carries):
 * dflux_du_dev[num][nqs][n] with respect to the element's unknowns in flattened (variable, dof) order (time-integration
 * factor alpha_u included), dflux_daux_dev[num][nqs] with respect to the aux value at the point.                     */
int mha_compute_flux(mha_context *ctx, int group_id, const double *u_dev, const double *u_prev_dev, const double *u_stage_dev,
                     double *flux_dev, double *dflux_du_dev, double *dflux_daux_dev);
/* Derived quantities of the block's module at the volume integration points.
 * replaces: linearelasticity::getDerivedNames / getDerivedValues (src/physics/linearelasticity.cpp:1289-1360).
 * mha_num_derived: 2 on MHA_PHYSICS_LINEARELASTICITY and MHA_PHYSICS_LINEARELASTICITY_THERMAL, 0 on every other module
 * (-1: bad context).  mha_derived_name: "VM stress", "MAG stress" (:1292-1293); NULL out of range.                     */
int mha_num_derived(mha_context *ctx);
const char *mha_derived_name(mha_context *ctx, int k);
/* getDerivedValues (:1301-1360) for all elements of the block in one launch: computeStress (:913-1099, with the
 * thermoelastic term on the coupled block) from the solution u_dev as given (no stage seeding), "lambda" and "mu"
 * evaluated at the integration points at the current time (mha_set_time); then
 *   2-D (:1326-1338): VM = sqrt(sxx^2 - sxx syy + syy^2 + 3 sxy^2), MAG = sqrt(sxx^2 + syy^2)
 *   3-D (:1339-1354): VM = sqrt(((sxx-syy)^2 + (syy-szz)^2 + (szz-sxx)^2) / 2 + 3 (sxy^2 + syz^2 + szx^2)),
 *                     MAG = sqrt(sxx^2 + syy^2 + szz^2)   (the normal components only, as the reference has it).
 * vm_dev[E][nq], mag_dev[E][nq], stress_dev[E][nq][dim][dim]; each may be NULL and is then skipped.  Every module
 * without derived quantities refuses the call with MHA_ERR_INVALID.                                                 */
int mha_get_derived_values(mha_context *ctx, const double *u_dev, double *vm_dev, double *mag_dev, double *stress_dev);
int mha_boundary_update(mha_context *ctx, int group_id);
int mha_boundary_view(mha_context *ctx, int group_id, const char *name, void **dev_ptr, int64_t extents[4],
                      int *rank);
/* scalar settings of the physics module; thermal: "form_param" (thermal.cpp:35, default 1:
 * symmetric Nitsche; -1 the non-symmetric variant), "include advection" (thermal.cpp:39, default 0; 1 adds
 * (b . grad e, v) with the functions "bx","by","bz", thermal.cpp:59-61, 150-160: the block then assembles on the
 * point engine, MHA_PATH_ROW_OWNER is refused); navierstokes: "useSUPG", "usePSPG"
 * (navierstokes.cpp:45-46) and "fix_uz_offsets": the reference scatters the 3-D uz momentum
 * block through uy's offsets (navierstokes.cpp:688); 0 (default) reproduces that, 1 uses uz's;
 * shallowwaterHybridized: "g" (shallowwaterHybridized.cpp:72, default 9.81); navierstokes + cdr: navierstokes' three;
 * cdr: none; helmholtz: "fractional" (helmholtz.cpp:22), accepted at 0 only.                       */
/* porousMixed (porousMixed.cpp:46-120) also takes: "use permeability data" (Kinv_xx = Kinv_yy = Kinv_zz = 1 / data(elem, 0)
 * from the block's element data, in place of the Kinv_* functions, updatePerm :550-563; total_mobility still divides);
 * "use KL expansion" (Kinv_dd divided by exp(KL_dd), a Karhunen-Loeve field evaluated at every integration point,
 * updateKLPerm :567-714) with the "KL parameters" sublist flattened to "KL N x", "KL L x", "KL sigma x", "KL eta x" and
 * the same for y and z (2-D: x and y); N is at most MHA_KL_MAX_TERMS per direction.  "fix_KL_3d" (default 0) reproduces
 * the 3-D KLUQcoeffs branch of the reference (lambda_z from the y expansion, the term twice into KL_xx, once into
 * KL_yy, never into KL_zz, :614-637); 1 uses lambda_z and adds every term once to each component.  Either option makes
 * the porousMixed database mode decline (mha_get_info "porous_direct" then reads 1).  Heterogeneous permeability with
 * deck-string functions is refused. */
int mha_set_physics_parameter(mha_context *ctx, const char *name, double value);

/* ---- porousMixed heterogeneous permeability -----------------------------------------------
 * Element data of the block, [num_elems][ncols] host array in mha_set_mesh element order, copied and owned by the
 * context (the analogue of groups[block][grp]->data; column 0 is the permeability).  ncols >= 1; data(e, 0) must be
 * finite and nonzero.  A new mesh drops it.  "use permeability data" without element data fails at assembly time with
 * MHA_ERR_STATE.  Waits for the context's stream before replacing an earlier array. */
#define MHA_KL_MAX_TERMS 8
int mha_set_element_data(mha_context *ctx, int ncols, const double *data_host);
/* AssemblyManager::importMeshData (assemblyManager.cpp:8235-8400), non-grid branch: each element takes the value row of
 * the data point nearest to its centre (the reference-cell centre in the physical frame: the vertex average of a Q1
 * cell), squared Euclidean distance, ties to the lowest point index (tools/data.cpp:391-420); then as
 * mha_set_element_data.  points_host [npts][dim], values_host [npts][ncols]; seed_out (nullable) [num_elems] receives
 * the chosen point of every element (data_seed). */
int mha_import_mesh_data(mha_context *ctx, int64_t npts, const double *points_host, int ncols, const double *values_host,
                         int32_t *seed_out);
/* A vector-valued parameter of the physics module (wkset->getParameter); porousMixed: "KLUQcoeffs" (terms
 * 0 .. min(n, nterms)) and "KLStochcoeffs" (terms prog .. min(nterms, prog + n), prog = the length of KLUQcoeffs if that
 * is set, 0 otherwise).  Any other name is refused.  The values are copied; they take effect at the next assembly, which
 * waits for the work already queued on the context's stream before it replaces the device tables.  Between UQ samples
 * this is the only call needed. */
int mha_set_parameter_vector(mha_context *ctx, const char *name, int n, const double *values_host);
/* Host-only, no GPU needed.  mha_closest_points: for each of nq query points [nq][dim] the index of the nearest of np
 * points [np][dim] (exact; as mha_import_mesh_data).  mha_kl_expansion: the first N roots omega and eigenvalues lambda
 * of one 1-D expansion (tools/klexpansion.hpp:38-90; N <= MHA_KL_MAX_TERMS; fewer than N roots found is an error).
 * mha_kl_indices: the multi-indices [prod N][dim] of a 2-D or 3-D expansion in the reference's total order
 * (porousMixed.cpp:73-118). */
int mha_closest_points(int dim, int64_t nq, const double *query, int64_t np, const double *points, int32_t *idx_out);
int mha_kl_expansion(int N, double L, double sigma, double eta, double *omega_out, double *lambda_out);
int mha_kl_indices(int dim, const int N[3], int32_t *idx_out);

/* ---- shallowwaterHybridized side terms ---------------------------------------------------
 * replaces: computeFluxVector(on_side) :409-480, eigendecompFluxJacobian :765-823,
 * computeStabilizationTerm :487-588, computeBoundaryTerm :595-758 and computeFlux :270-368 of
 * src/physics/shallowwaterHybridized.cpp, evaluated at npts side integration points (2-D; state
 * order H, Hux, Huy).  S = interior state ("H","Hux","Huy" side fields), Shat = trace state
 * ("aux H", ...), normals[npts][2], Sinf[npts][3] = "Far-field <var> <side>" (Far-field only).
 * Outputs (any may be NULL): fluxvec[npts][3][2] = fluxes_side; term[npts][3] = stab_bound_side
 * (stabilisation term for MHA_SWH_INTERFACE, boundary term otherwise); iflux[npts][3] = what
 * computeFlux stores in wkset->flux; d_iflux_dS / d_iflux_dShat [npts][3][3] = its derivatives
 * (the SFad part of the reference's result), by forward AD on the device.  All pointers device.
 * Stateless: no context; hip_stream may be NULL.                                              */
#define MHA_SWH_INTERFACE 0
#define MHA_SWH_FARFIELD 1
#define MHA_SWH_SLIP 2
int mha_swhdg_side_terms(int side_type, int roe_stabilization, double g, int64_t npts, const double *S_dev,
                         const double *Shat_dev, const double *normals_dev, const double *Sinf_dev,
                         double *fluxvec_dev, double *term_dev, double *iflux_dev, double *d_iflux_dS_dev,
                         double *d_iflux_dShat_dev, void *hip_stream);
/* The HDG element, side part: residual and derivative blocks of the 12 interior unknowns (H, Hux, Huy, HGRAD
 * order 1, flattened (variable, dof)) and the 24 trace unknowns of every element of a shallowwaterHybridized block.
 * replaces: boundaryResidual :190-263 on the four sides (interior rows), computeFlux :270-368 integrated against the
 * trace basis as SubGridDtN_Solver::updateFlux does (src/subgrid/subgridDtN_solver.cpp:1583-1601, trace rows), with
 * Basis_HFACE_QUAD_In_FEM of degree 1 (src/tools/Intrepid2_HFACE_QUAD_In_FEMdef.hpp:84-196: per edge the two linear
 * Lagrange functions of the edge's reference coordinate; edges left x=-1, bottom y=-1, right x=+1, top y=+1).
 * lambda_dev[E][24]: variable, edge, function.  side_types_dev[E][4] u8 in shards side order (bottom, right, top,
 * left): MHA_SWH_*; NULL = all interface.  farfield_host[3] (Far-field sides).  Outputs, element-major, rows/columns
 * = 12 interior then 24 traces: res_dev[E][36] = -res.val(), blocks_dev[E][36][36] = res(r).dx(c) (stored); either may
 * be NULL.  The volume part of the interior block comes from mha_compute_local_jacres.                           */
int mha_swhdg_element_blocks(mha_context *ctx, const double *u_dev, const double *u_prev_dev, const double *u_stage_dev,
                             const double *lambda_dev, const uint8_t *side_types_dev, const double *farfield_host,
                             double *res_dev, double *blocks_dev);
/* The subgrid sub-iteration loop: SubGridDtN_Solver::nonlinearSolver (src/subgrid/subgridDtN_solver.cpp:909-1041) with
 * its assembleJacobianResidual (:681-903) and element-local direct solve, for a shallowwaterHybridized block whose interior
 * unknowns are element-local (one HDG element per subgrid: every LID belongs to one element -- checked).  Per element,
 * with the trace lambda held fixed: pass 0 records resnorm_initial = |res_u|_inf and sets the scaled norm to 1 (0 if the
 * residual vanishes); while scaled > tol (sub_NLtol) and passes < max_iter (sub_maxNLiter): du = A_uu^-1 r_u,
 * u += du, reassemble, scaled = |res_u|_inf / resnorm_initial.  u_dev is updated in place.  Outputs: iters_dev[E] =
 * assemblies the element's loop performed (the reference's `iter`), resnorm_scaled_dev[E], and -- from one closing
 * assembly at the final state -- schur_dev[E][24][24], gvec_dev[E][24] as mha_batched_condense defines them (either may
 * be NULL: no closing pass), *num_singular_dev = singular interior blocks met, CUMULATIVE over all max_iter + 1
 * condensation passes (an element that stays singular is counted once per pass, also after it has left its loop):
 * zero means no pass met one; it is not a count of elements.  Everything is enqueued on the context's
 * stream: NO host synchronisation and NO allocation inside (workspace_dev of mha_swhdg_subgrid_workspace_bytes bytes is
 * the caller's; side tables are built on the first call).  Elements that have converged are still swept by the remaining
 * passes and ignored: the uniform schedule is what keeps the host out of the loop.                                   */
int mha_swhdg_subgrid_workspace_bytes(mha_context *ctx, int64_t *bytes);
int mha_swhdg_subgrid_solve(mha_context *ctx, double *u_dev, const double *u_prev_dev, const double *u_stage_dev,
                            const double *lambda_dev, const uint8_t *side_types_dev, const double *farfield_host,
                            int max_iter, double tol, void *workspace_dev, int64_t workspace_bytes, double *schur_dev,
                            double *gvec_dev, int32_t *iters_dev, double *resnorm_scaled_dev, int32_t *num_singular_dev);
/* The element step of the HDG subgrid in ONE kernel: side terms (mha_swhdg_element_blocks) + volume terms
 * (shallowwaterHybridized::volumeResidual, src/physics/shallowwaterHybridized.cpp:113-184) + static condensation
 * (mha_batched_condense), one wavefront per element -- the [36 x 36] block of SubGridDtN_Solver::assembleJacobianResidual
 * (src/subgrid/subgridDtN_solver.cpp:681-903) and updateFlux (:1542-1616) never leaves the chip.  Outputs as
 * mha_batched_condense defines them: schur_dev[E][24][24], gvec_dev[E][24], du_dev[E][12] (flattened (variable, dof));
 * any may be NULL, not all.  *num_singular_dev += singular interior blocks (device counter, may be NULL).  Enqueued on
 * the context's stream: no synchronisation, no allocation (side tables are built on the first call).  Sources given as
 * deck strings are refused (MHA_ERR_INVALID): the unfused entry points take those.  mha_swhdg_subgrid_solve runs this
 * kernel once per pass with the loop bookkeeping and sol += du inside (MHA_SUBGRID_UNFUSED=1 keeps the four-kernel
 * pipeline, the independent implementation the tests compare with).                                                 */
int mha_swhdg_condensed_element(mha_context *ctx, const double *u_dev, const double *u_prev_dev, const double *u_stage_dev,
                                const double *lambda_dev, const uint8_t *side_types_dev, const double *farfield_host,
                                double *schur_dev, double *gvec_dev, double *du_dev, int32_t *num_singular_dev);
/* ---- HDG subgrids of m x m sub-elements per macro element -------------------------------------------------------
 * The DtN subgrid model refines the macro element (SubGridDtN_Solver::assembleJacobianResidual,
 * src/subgrid/subgridDtN_solver.cpp:681-903); one HDG element per subgrid (the entry points above) is its degenerate case.
 * Scope: 2-D quads, H / Hux / Huy HGRAD order 1 and continuous inside a macro element, the macro trace HFACE degree 1 (24
 * unknowns, as above), m in 1..4: n_int = 3 (m+1)^2 = 12, 27, 48, 75 interior unknowns per macro element.
 * mha_swhdg_set_subgrids declares that elements [k m^2, (k+1) m^2) of the block are macro element k's structured sub-mesh,
 * row-major with x fastest, and validates on the host that the LIDs of macro element k are shared only inside k with the Q1
 * connectivity of an m x m grid, and that the sub-mesh vertices are the bilinear image of the uniform m x m subdivision of
 * the macro quad to 1e-12 x its size.  m = 0 clears the layout; m > 4 is refused (MHA_ERR_INVALID: the dense interior
 * solve holds at most 75 unknowns on the chip); mha_set_mesh clears it.  With no layout set every other entry point behaves
 * exactly as before.
 * Semantics: volumeResidual (src/physics/shallowwaterHybridized.cpp:113-184) on every sub-element, summed into the interior
 * rows through the sub-mesh LIDs (subgridDtN_solver.cpp:774-808); boundaryResidual (:190-263) on the 4m sub-sides on the
 * macro boundary only; the trace state at a sub-side point is the macro edge's HFACE basis there
 * (src/subgrid/subgridDtN.cpp:746-870, auxside_basis): sub-side j of m on a macro edge covers the edge coordinate
 * [-1 + 2j/m, -1 + 2(j+1)/m], edges oriented as mha_swhdg_element_blocks documents; trace rows: computeFlux (:270-368)
 * against that macro trace basis over the sub-sides of each macro edge (updateFlux, subgridDtN_solver.cpp:1542-1616).
 * Interior unknowns of a macro element are flattened (variable, sub-mesh node), node = ay (m+1) + ax; for m = 1 that is
 * the (variable, dof) order of mha_swhdg_condensed_element.  lambda_dev[Em][24], side_types_dev[Em][4] (per MACRO side).
 * mha_swhdg_condensed_subgrid: assembly + static condensation in one kernel, one workgroup per macro element, the
 * [n_int + 24] x [n_int + 24 + 1] system in LDS, a dense Gauss-Jordan solve with partial pivoting there (the reference
 * uses a sparse direct solver; at these sizes the dense solve is the one that never leaves the chip), the A_lu A_uu^-1 A_ul
 * product on the fp64 matrix cores.  Outputs as mha_batched_condense defines them: schur_dev[Em][24][24], gvec_dev[Em][24],
 * du_dev[Em][n_int]; any may be NULL, not all; *num_singular_dev += singular interior blocks.  Contributions are summed
 * in a fixed order: two runs are bit-identical.  Deck-string sources are refused.  No synchronisation, no allocation.
 * mha_swhdg_subgrid_solve on a block with a layout runs this kernel per pass: the same protocol with norms and du over the
 * n_int unknowns of a macro element, iters / resnorm / schur / gvec per macro element, workspace bytes following the layout.
 * mha_swhdg_subgrid_blocks: the UNCONDENSED res_dev[Em][n_int+24] = -res.val() and blocks_dev[Em][n_int+24][n_int+24] (either
 * may be NULL), by a plain unfused kernel: the independent implementation the fused kernel is compared with.
 * The condensed blocks feed mha_scatter_plan_* with the macro trace LIDs, unchanged.                                   */
int mha_swhdg_set_subgrids(mha_context *ctx, int m);
int mha_swhdg_condensed_subgrid(mha_context *ctx, const double *u_dev, const double *u_prev_dev, const double *u_stage_dev,
                                const double *lambda_dev, const uint8_t *side_types_dev, const double *farfield_host,
                                double *schur_dev, double *gvec_dev, double *du_dev, int32_t *num_singular_dev);
int mha_swhdg_subgrid_blocks(mha_context *ctx, const double *u_dev, const double *u_prev_dev, const double *u_stage_dev,
                             const double *lambda_dev, const uint8_t *side_types_dev, const double *farfield_host,
                             double *res_dev, double *blocks_dev);
/* Mesh helper (input generation): ncell_macro[2] macro quads on [lo, hi], each an m x m sub-mesh.  sizes: nelem = Em m^2,
 * ndof = Em n_int, ntrace = rows of the macro trace system.  nodes[nelem][4][2], lids[nelem][12], offsets[12] for
 * mha_set_mesh; trace_lids[Em][24] for mha_scatter_plan_create.                                                          */
int mha_mesh_swhdg_subgrids_sizes(const int *ncell_macro, int m, int *nelem, int64_t *ndof, int64_t *ntrace);
int mha_mesh_swhdg_subgrids(const int *ncell_macro, int m, const double *lo, const double *hi, double *nodes,
                            int32_t *lids, int32_t *offsets, int32_t *trace_lids);
/* ---- porousMixedHybridized: the element step --------------------------------------------------------------------
 * replaces: porousMixedHybrid::volumeResidual + faceResidual (src/physics/porousMixedHybridized.cpp:72-189, 287-362) on
 * every element and all of its 2 dim faces, in the layout and conventions of the shallowwaterHybridized entry points
 * above.  Unknowns of an element: the interior ones first -- p, then the 2 dim flux dofs in (variable, dof) order, dof
 * 2 c + s = the face of direction c on the low (s = 0) or high (s = 1) side -- then the 2 dim traces in the reference's
 * HFACE order: left x=-1, bottom y=-1, right x=+1, top y=+1 for quads (src/tools/Intrepid2_HFACE_QUAD_In_FEMdef.hpp),
 * then front z=-1, back z=+1 for hexes (src/tools/Intrepid2_HFACE_HEX_In_FEMdef.hpp:97-269).  n_int = 1 + 2 dim,
 * n = n_int + 2 dim.  With the block's quadrature in the volume and the side points of the side tables:
 *   R_u = int (Kinv u) . v - p div v + sum_faces int_F lambda v . n,   R_p = int (-div u + source) q,
 *   R_lambda = - sum_faces int_F (u . n) mu.
 * u_dev[nrows] is the block's state (steady; a transient context is refused), lambda_dev[E][2 dim] the traces.
 * mha_pmh_element_blocks: res_dev[E][n] = -res.val(), blocks_dev[E][n][n] = d res / d unknown (either may be NULL), by a
 * plain kernel, one thread per (element, row): the implementation the fused kernel is compared with, through
 * mha_batched_condense.  The p-lambda, lambda-lambda and p-p entries are exactly 0.0.
 * mha_pmh_condensed_element: geometry, local matrices, interior solve and Schur complement in one launch, one thread per
 * element; schur_dev[E][2 dim][2 dim], gvec_dev[E][2 dim], du_dev[E][n_int] as mha_batched_condense defines them (any may
 * be NULL, not all) are all that is written, in whole 16-byte pieces that are contiguous across a wavefront.  It uses
 * the structure instead of a pivoted dense solve: A = (Kinv phi_i, phi_j) is symmetric positive definite (Cholesky),
 * the p unknown has the scalar Schur complement B A^-1 B^T > 0, the trace coupling is one entry per face.  A
 * non-positive pivot (degenerate element, Kinv <= 0) is counted into *num_singular_dev (device counter, may be NULL;
 * an integer atomic that runs for such elements only); that element's outputs are unspecified but finite.  Enqueued on
 * the context's stream: no host synchronisation, no allocation (side tables and the DG check are made on the first call
 * after mha_set_mesh).  No floating-point atomics: two runs are bit-identical.
 * The linear solve on one block is two calls: step at (u, lambda); mha_scatter_plan_apply(schur, gvec) with the boundary
 * trace rows fixed; the caller solves the trace system and updates lambda; step again and u += du.  The second call's
 * gvec is zero to round-off on free rows.                                                                            */
int mha_pmh_element_blocks(mha_context *ctx, const double *u_dev, const double *lambda_dev, double *res_dev,
                           double *blocks_dev);
int mha_pmh_condensed_element(mha_context *ctx, const double *u_dev, const double *lambda_dev, double *schur_dev,
                              double *gvec_dev, double *du_dev, int32_t *num_singular_dev);
/* Mesh helper (input generation, host only): ncell[dim] cells on [lo, hi], dim = 2 or 3, for a porousMixedHybridized
 * block.  sizes: nelem, ndof = nelem (1 + 2 dim) DG unknowns, ntrace = faces of the mesh.  nodes[E][2^dim][dim] (shards
 * vertex order), lids[E][1 + 2 dim] (every LID once), offsets[1 + 2 dim] and orient[E][1 + 2 dim] (the face signs
 * mha_mesh_structured_multi gives conforming HDIV) for mha_set_mesh / mha_set_orientation; trace_lids[E][2 dim] in the
 * HFACE face order above for mha_scatter_plan_create; trace_side[ntrace] u8: 0 for an interior face, 1 + side on the
 * boundary with side 0 left (x low), 1 right, 2 bottom (y low), 3 top, 4 front (z low), 5 back.                       */
int mha_mesh_porous_hybrid_sizes(int dim, const int *ncell, int *nelem, int64_t *ndof, int64_t *ntrace);
int mha_mesh_porous_hybrid(int dim, const int *ncell, const double *lo, const double *hi, double *nodes, int32_t *lids,
                           int32_t *offsets, int8_t *orient, int32_t *trace_lids, uint8_t *trace_side);
/* ---- porousWeakGalerkin: the element step ---------------------------------------------------------------------------
 * replaces: porousWeakGalerkin::volumeResidual + faceResidual (src/physics/porousWeakGalerkin.cpp:94-323, 424-505) on
 * every element and all of its 2 dim faces, in the layout and conventions of the porousMixedHybridized entry points
 * above.  Unknowns of an element: pint, the 2 dim dofs of u, the 2 dim dofs of t (dof 2 c + s as above), then the 2 dim
 * traces pbndry in HFACE order; n_int = 1 + 4 dim, n = 1 + 6 dim (13 or 19).
 *   R_pint = int (div t - source) q,              R_u = int u . v + pint div v - sum_faces int_F pbndry (v . n),
 *   R_t = int (perm u + t) . s,                   R_pbndry = - sum_faces int_F (t . n) mu.
 * u_dev[nrows] is the block's state (steady; a transient context is refused), lambda_dev[E][2 dim] the traces.
 * mha_pwg_element_blocks: res_dev[E][n] = -res.val(), blocks_dev[E][n][n] = d res / d unknown (either may be NULL), by a
 * plain kernel, one thread per (element, row), every volume and side point of general quads and hexes: the
 * implementation the fused kernel is compared with, through mha_batched_condense.  The structurally empty sub-blocks
 * (pint-pint, pint-u, pint-lambda, u-t, t-pint, t-lambda, lambda-pint, lambda-u, lambda-lambda) are exactly +0.0.
 * mha_pwg_condensed_element: the same step with the interior solve and the Schur complement inside, one launch, one
 * thread per element; schur_dev[E][2 dim][2 dim], gvec_dev[E][2 dim], du_dev[E][n_int] as mha_batched_condense defines
 * them (any may be NULL, not all; each 16-byte aligned) are all that is written, in whole 16-byte pieces that are
 * contiguous across a wavefront.  No pivot search: with M = (v_f, v_g) = L L^T, K = (perm v_f, v_g), B = (1, div v_f),
 * C_k = <v_f(k) . n, 1>:  W = M^-1 K M^-1,  Z = W B,  sigma = B^T W B > 0,
 *   dp = (r_p - B^T M^-1 r_t + Z^T r_u) / sigma,  du = M^-1 (r_u - B dp),  dt = M^-1 (r_t - K du),
 *   S_ab = C_a C_b (W_ab - Z_a Z_b / sigma),      g_a = r_lambda,a + C_a dt_a.
 * A non-positive Cholesky pivot or sigma <= 0 (degenerate element, perm <= 0) is counted into *num_singular_dev (device
 * counter, may be NULL); that element's outputs are unspecified but finite.  Enqueued on the context's stream: no host
 * synchronisation, no allocation after the first call on a mesh.  No floating-point atomics: two runs are bit-identical.
 * The linear solve on one block is the two calls of porousMixedHybridized.                                            */
int mha_pwg_element_blocks(mha_context *ctx, const double *u_dev, const double *lambda_dev, double *res_dev,
                           double *blocks_dev);
int mha_pwg_condensed_element(mha_context *ctx, const double *u_dev, const double *lambda_dev, double *schur_dev,
                              double *gvec_dev, double *du_dev, int32_t *num_singular_dev);
/* Mesh helper (input generation, host only) for a porousWeakGalerkin block: nodes, trace_lids, trace_side and ntrace as
 * mha_mesh_porous_hybrid gives them; lids[E][1 + 4 dim] (every LID once), offsets[1 + 4 dim] and orient[E][1 + 4 dim]
 * (u and t carry the same face signs); ndof = nelem (1 + 4 dim).                                                       */
int mha_mesh_porous_weak_galerkin_sizes(int dim, const int *ncell, int *nelem, int64_t *ndof, int64_t *ntrace);
int mha_mesh_porous_weak_galerkin(int dim, const int *ncell, const double *lo, const double *hi, double *nodes,
                                  int32_t *lids, int32_t *offsets, int8_t *orient, int32_t *trace_lids, uint8_t *trace_side);
/* Batched static condensation of element blocks: eliminates the n_int interior unknowns of every element.
 * replaces: the element-local direct solve of the subgrid solver and its forward sensitivities d u / d lambda
 * (SubGridDtN_Solver, src/subgrid/subgridDtN_solver.cpp:681-903, 1542-1616) in Schur-complement form.
 * blocks_dev[E][n][n], res_dev[E][n] with n = n_int + n_trace, interior unknowns first (the layout of
 * mha_swhdg_element_blocks; add the volume block of mha_compute_local_jacres to the interior part first);
 * outputs: schur_dev[E][n_trace][n_trace] = A_ll - A_lu A_uu^-1 A_ul, gvec_dev[E][n_trace] = r_l - A_lu A_uu^-1 r_u,
 * du_dev[E][n_int] = A_uu^-1 r_u (any may be NULL).  Gauss-Jordan with partial pivoting, one wavefront per
 * element; n_int <= 32, n_int + n_trace + 1 <= 64.  Singular interior blocks: counted into *num_singular_host
 * if given, MHA_ERR_INVALID otherwise.  Stateless; synchronises the stream.                                  */
int mha_batched_condense(int n_int, int n_trace, int64_t num_elems, const double *blocks_dev, const double *res_dev,
                         double *schur_dev, double *gvec_dev, double *du_dev, int *num_singular_host, void *hip_stream);
/* Scatter of dense element blocks through an arbitrary LID map: the flux -> trace scatter of the HDG caller (condensed
 * blocks [E][24][24] and flux vectors [E][24] of mha_batched_condense into the macro trace system).
 * replaces: SubGridDtN_Solver::updateFlux's scatter and the macro assembly's sumIntoValues for those blocks
 * (src/subgrid/subgridDtN_solver.cpp:1542-1616, src/managers/assemblyManager.cpp:4031-4145).
 * create: lids_host[E][n] = global row of unknown t of element e; the CRS graph of the target (colind ascending inside a
 * row), or NULL/NULL to have the every-dof-of-an-element-couples graph built (read it back with _graph); fixed_host
 * [num_rows] or NULL.  apply: vals[rowptr[r] + slot] (+)= sum blocks[e][t][s], res[r] (+)= sum vec[e][t], one wavefront
 * per CRS row, no global atomics, results independent of scheduling; overwrite = 1 stores (fixed rows: zeros),
 * 0 accumulates (fixed rows untouched).  blocks+vals or vec+res may be NULL.                                    */
typedef struct mha_scatter_plan mha_scatter_plan;
int mha_scatter_plan_create(int n, int64_t num_elems, int64_t num_rows, const int32_t *lids_host,
                            const int32_t *rowptr_host, const int32_t *colind_host, const uint8_t *fixed_host,
                            mha_scatter_plan **out);
int mha_scatter_plan_nnz(const mha_scatter_plan *p, int64_t *nnz);
int mha_scatter_plan_graph(const mha_scatter_plan *p, int32_t *rowptr_host, int32_t *colind_host);
int mha_scatter_plan_apply(const mha_scatter_plan *p, const double *blocks_dev, const double *vec_dev, double *res_dev,
                           double *vals_dev, int overwrite, void *hip_stream);
void mha_scatter_plan_destroy(mha_scatter_plan *p);
/* L[npts][3][3], lam[npts][3], R[npts][3][3] (row-major) of the normal flux Jacobian at Shat */
int mha_swhdg_eigendecomp(double g, int64_t npts, const double *Shat_dev, const double *normals_dev,
                          double *L_dev, double *lam_dev, double *R_dev, void *hip_stream);

/* ---- structured mesh helper (input generation, not part of the hot path) ------
 * 2-D order 1 = SimpleMeshManager_Rectangle (src/tools/simplemeshmanager.hpp:639-675)
 * with offsets {0,1,3,2} (discretizationInterface.cpp:302).                            */
int mha_mesh_sizes(int dim, int order, const int *ncell, int *nverts, int *nelem, int64_t *ndof);
int mha_mesh_structured(int dim, int order, const int *ncell, const double *lo, const double *hi,
                        double *verts, int32_t *cell2vert, int32_t *lids, int32_t *offsets,
                        uint8_t *boundary_dof);

/* The same for a block of several variables (types MHA_BASIS_*; HGRAD orders dividing the largest, HVOL order 0, HDIV
 * order 1): vertices, cell -> vertex map, the subcell-major dof map (nodes of the finest HGRAD lattice, then cells, then
 * faces by direction), offsets [n_tot] (position of every variable's dofs in an element's LID list, variables
 * concatenated), orientation signs [E][n_tot] (lowest-order HDIV: -+1, others 1; what Intrepid2's
 * modifyBasisByOrientation applies, discretizationInterface.cpp:957-1055), side_mask [ndof] (bit 2d / 2d+1: the dof
 * lies on the low / high boundary in direction d) and dof_var [ndof].  orient / side_mask / dof_var may be NULL.   */
int mha_mesh_multi_sizes(int dim, const int *ncell, int nvars, const int *types, const int *orders, int *nverts,
                         int *nelem, int *n_tot, int64_t *ndof);
int mha_mesh_structured_multi(int dim, const int *ncell, const double *lo, const double *hi, int nvars, const int *types,
                              const int *orders, double *verts, int32_t *cell2vert, int32_t *lids, int32_t *offsets,
                              int8_t *orient, uint8_t *side_mask, int32_t *dof_var);

/* ---- row partition (host only; no GPU needed) -------------------------------------
 * The fused kernel is row-owner: each CRS row is produced by exactly one workgroup that
 * visits all elements incident to its rows -- the scatter of the reference
 * (assemblyManager.cpp:4063-4144) without atomics.  These entry points expose the partition
 * for inspection: blocks of rows (ascending) and the elements each block touches.
 * caps[4] = {elements per Morton chunk, max CRS entries, max rows, max elements} or NULL.   */
typedef struct mha_row_partition mha_row_partition;
int mha_row_partition_build(int dim, int num_elems, int dofs_per_elem, int num_rows, const double *nodes_host,
                            const int32_t *lids_host, const int32_t *rowptr_host, const int *caps,
                            mha_row_partition **out);
int mha_row_partition_sizes(const mha_row_partition *p, int *num_blocks, int64_t *num_rows, int64_t *num_elems,
                            int *max_rows, int *max_elems, int *max_entries);
int mha_row_partition_get(const mha_row_partition *p, int32_t *row_ptr, int32_t *rows, int32_t *elem_ptr,
                          int32_t *elems);
void mha_row_partition_destroy(mha_row_partition *p);

/* ---- Export(ADD) of shared-DOF rows between element-block shards (one process per GPU) -----------------------------
 * Replaces LinearAlgebraInterface::exportMatrixFromOverlapped / exportVectorFromOverlapped
 * (src/interfaces/linearAlgebraInterface.hpp:296-337: Tpetra::Export, combine mode ADD): every rank assembles its
 * overlapped CRS values / residual; the ranks that do not own a shared row send its partial values to the owner, which
 * adds them.  The shared rows are explicit lists agreed at setup (any partition: HGRAD planes between slabs, HDIV face
 * dofs, HDG trace rows, unequal slabs), CSR-style per neighbour (all *_ptr have num_neighbors + 1 entries, host arrays):
 *   send_val_index: entries of my value array that go to the neighbour;  send_row_index: entries of my residual;
 *   recv_val_target: for every value arriving from it, the entry of MY value array it is added to, or -1 (an off-rank
 *                    column of one of my rows: stays in the receive buffer);  recv_row_target: likewise for the residual.
 * No indices travel: both sides list a shared row's entries in the same (global id) order.
 * mha_export_pack / mha_export_unpack_add are the device halves (the caller moves the buffers, e.g. with
 * torch.distributed P2P, whose "nccl" backend is RCCL); mha_export_add does pack + ncclSend / ncclRecv with every
 * neighbour in one group + unpack on this library's own RCCL communicator (mha_comm_*; librccl.so is loaded on first
 * use).  Neighbours are unpacked in the order given: the sum is reproducible.
 * nnz / nrows are the sizes of the value array and the residual the lists index: every index is range-checked at plan
 * creation and the receive targets of one neighbour must be distinct (MHA_ERR_INVALID otherwise).  vals_dev == NULL in
 * pack / unpack_add / export_add means a residual-only exchange (assembleRes, solverManager.cpp:1552-1556): the value
 * segments are skipped, on the wire too; res_dev == NULL likewise.                                                     */
typedef struct mha_export_plan mha_export_plan;
typedef struct mha_comm mha_comm;
int mha_export_plan_create(int num_neighbors, const int32_t *neighbor_ranks, const int64_t *send_val_ptr,
                           const int32_t *send_val_index, const int64_t *send_row_ptr, const int32_t *send_row_index,
                           const int64_t *recv_val_ptr, const int32_t *recv_val_target, const int64_t *recv_row_ptr,
                           const int32_t *recv_row_target, int64_t nnz, int64_t nrows, mha_export_plan **out);
void mha_export_plan_destroy(mha_export_plan *p);
int mha_export_pack(const mha_export_plan *p, const double *vals_dev, const double *res_dev, void *hip_stream);
int mha_export_unpack_add(const mha_export_plan *p, double *vals_dev, double *res_dev, void *hip_stream);
/* buffers of neighbour k (device pointers; layout [values | residual entries]) and the bytes one exchange sends */
int mha_export_buffers(const mha_export_plan *p, int k, double **send_dev, int64_t *send_count, double **recv_dev,
                       int64_t *recv_count);
int mha_export_bytes_on_wire(const mha_export_plan *p, int64_t *bytes);
int mha_comm_unique_id(char id_out[128]);                       /* rank 0; broadcast the 128 bytes to the others */
int mha_comm_create(int num_ranks, int rank, const char id[128], mha_comm **out); /* collective; current HIP device */
void mha_comm_destroy(mha_comm *c);
int mha_export_add(const mha_export_plan *p, mha_comm *c, double *vals_dev, double *res_dev, void *hip_stream);

/* ---- introspection for bench / tests ---------------------------------------------
 * keys: "num_elems","num_rows","nnz","dofs_per_elem","num_ip","workset_size","last_path",
 *       "row_blocks","num_affine_elems","row_block_max_rows","row_block_max_elems",
 *       "row_block_max_acc","row_owner_lds_bytes","block_patterns","block_pattern_roles",
 *       "block_pattern_blocks","block_pattern_mfma"
 * (the block_pattern keys are 0 when the matrix-core form of the row-owner Jacobian is not in use: MHA_K2=blocks,
 * or a mesh whose row blocks share too few assembly patterns)
 * round 3: "row_owner_kind" (1 affine kernels, 2 general-element kernel, of the last assembly), "general_row_blocks",
 *   "affine_shapes"          distinct geometry records (shape part, bit for bit) of the block's affine elements -- the
 *                            geometry database behind the affine path (reference: identifyVolumetricDatabase,
 *                            assemblyManager.cpp:4314-4467, with exact matching)
 *   "jacobian_database_mode" 1: the last affine row-owner Jacobian was computed for one row block per assembly pattern
 *                            and replicated (one shape, overwriting assembly); bit-identical to the full kernel
 *   "porous_direct"          last porousMixed assembly behind MHA_PATH_ROW_GATHER: 0 dense element arrays + row gather,
 *                            1 element threads stored into the CRS, 2 database mode (representative rows + replication) */
int mha_get_info(mha_context *ctx, const char *key, int64_t *value);
/* average device time (ms) of the last assembly's kernels, measured with HIP events on the
 * context's stream; valid after mha_set_timing(ctx,1).                                  */
int mha_set_timing(mha_context *ctx, int enable);
int mha_get_last_kernel_ms(mha_context *ctx, double *ms);

#ifdef __cplusplus
}
#endif
#endif
