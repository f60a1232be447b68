"""What each physics module accepts, asked of the module itself (PhysicsBase::checkVariables / checkBoundaryGroup)
through the host-only hook mha_test_module_rules (csrc/test_hooks.h): no block, no mesh, no GPU.  The tables below are
written out from the modules' documented rules, not read from the library."""
import ctypes as C

import numpy as np
import pytest

import mrhyde_amd

HGRAD, HVOL, HDIV = 0, 1, 2
INVALID = 1  # MHA_ERR_INVALID
NEUMANN, WEAK_DIRICHLET, INTERFACE, SWH_SLIP = 1, 2, 5, 12
BCS = (NEUMANN, WEAK_DIRICHLET, INTERFACE, SWH_SLIP)
H = HGRAD

# module -> id, variable list in 2-D and 3-D (None: the module does not exist there), text of its refusal per dimension
MODULES = {
    "thermal": (1, [H], [H], ("one HGRAD variable (e)",) * 2),
    "porousMixed": (2, [HVOL, HDIV], [HVOL, HDIV], ("p (HVOL) and u (HDIV), in that order",) * 2),
    "navierstokes": (3, [H] * 3, [H] * 4, ("ux, pr, uy[, uz], in that order",) * 2),
    "shallowwaterHybridized": (4, [H] * 3, None, ("H, Hux, Huy in 2-D",) * 2),
    "navierstokes+thermal": (5, [H] * 4, [H] * 5, ("4 HGRAD variables ux, pr, uy, e,", "5 HGRAD variables ux, pr, uy, uz, e,")),
    "linearelasticity": (6, [H] * 2, [H] * 3, ("2 HGRAD variables dx, dy,", "3 HGRAD variables dx, dy, dz,")),
    "linearelasticity+thermal": (7, [H] * 3, [H] * 4, ("3 HGRAD variables dx, dy, e,", "4 HGRAD variables dx, dy, dz, e,")),
    "cdr": (8, [H], [H], ("one HGRAD variable (c)",) * 2),
    "navierstokes+cdr": (9, [H] * 4, [H] * 5, ("4 HGRAD variables ux, pr, uy, c,", "5 HGRAD variables ux, pr, uy, uz, c,")),
    "helmholtz": (10, [H] * 2, [H] * 2, ("two HGRAD variables ureal, uimag",) * 2),
}
COUPLED_NS = ("navierstokes+thermal", "navierstokes+cdr")


def test_the_table_names_every_module():
    assert {k: v[0] for k, v in MODULES.items()} == mrhyde_amd.ALL_PHYSICS_IDS


def card(basis, order, dim):
    return (order + 1) ** dim if basis == HGRAD else 1 if basis == HVOL else 2 * dim


def ask(physics_id, dim, types, orders=None, cards=None, bc=0, side="left", n=None, block_order=1, nqs=None, neumann_e=False):
    """bc == 0: the variable rule; otherwise the boundary-group rule.  Returns (code, message)."""
    lib = mrhyde_amd.load_library()
    f = lib.mha_test_module_rules
    f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int, C.c_char_p] + [C.c_int] * 4
    orders = [1] * len(types) if orders is None else orders
    cards = [card(t, o, dim) for t, o in zip(types, orders)] if cards is None else cards
    t, o, c = (np.asarray(a, dtype=np.int32) for a in (types, orders, cards))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    code = f(physics_id, dim, len(types), vp(t), vp(o), vp(c), bc, side.encode(), int(sum(cards)) if n is None else n,
             block_order, 2 ** (dim - 1) if nqs is None else nqs, int(neumann_e))
    return code, lib.mha_last_error().decode()


def refused(text, *args, **kw):
    code, msg = ask(*args, **kw)
    assert code == INVALID and text in msg, (args, kw, code, msg)
    return msg


def accepted(*args, **kw):
    assert ask(*args, **kw) == (0, ""), (args, kw, ask(*args, **kw))


@pytest.mark.parametrize("name", sorted(MODULES))
@pytest.mark.parametrize("dim", [2, 3])
def test_variable_rule(name, dim):
    pid, v2, v3, texts = MODULES[name]
    right, text = (v2, v3)[dim - 2], texts[dim - 2]
    if right is None:  # 2-D only: its 2-D list is refused in 3-D
        refused(text, pid, dim, v2)
        return
    accepted(pid, dim, right)
    refused(text, pid, dim, right[:-1])
    refused(text, pid, dim, right + [HGRAD])
    wrong = [HDIV, HVOL] if name == "porousMixed" else right[:-1] + [HVOL]
    refused(text, pid, dim, wrong)
    if name == "linearelasticity":
        assert "thermoelastic" in refused(text, pid, dim, right + [HGRAD])


@pytest.mark.parametrize("dim", [2, 3])
def test_orders_that_must_agree(dim):
    pid, right = MODULES["helmholtz"][0], [H, H]
    assert "ureal and uimag" in refused("same order", pid, dim, right, orders=[1, 2])
    accepted(pid, dim, right, orders=[2, 2])
    pid, right = MODULES["linearelasticity+thermal"][0], [H] * (dim + 1)
    refused("same order", pid, dim, right, orders=[1] * (dim - 1) + [2, 1])
    accepted(pid, dim, right, orders=[2] * dim + [1])  # e may have its own


def test_an_id_that_is_not_a_module():
    for pid in (0, 11, -1, 99):
        refused("unknown physics module id %d" % pid, pid, 2, [H])


# module -> the group types it takes; the first five have no rule of their own and take every valid type
TAKES = {name: BCS for name in ("thermal", "porousMixed", "navierstokes", "shallowwaterHybridized", "cdr")}
TAKES.update({"navierstokes+thermal": (), "navierstokes+cdr": (), "linearelasticity+thermal": (NEUMANN,),
              "helmholtz": (NEUMANN,), "linearelasticity": (NEUMANN, WEAK_DIRICHLET)})
REFUSAL = {"navierstokes+thermal": "navierstokes+thermal: thermal boundary groups (Neumann, weak Dirichlet, interface on e) are "
                                   "not built for the coupled block",
           "navierstokes+cdr": "navierstokes+cdr: boundary groups of the modules (Neumann, weak Dirichlet, interface) are not "
                               "built for the coupled block",
           "linearelasticity+thermal": "linearelasticity+thermal: boundary groups are MHA_BC_NEUMANN",
           "helmholtz": "helmholtz: boundary groups are MHA_BC_NEUMANN",
           "linearelasticity": "linearelasticity: boundary groups are MHA_BC_NEUMANN (traction) or MHA_BC_WEAK_DIRICHLET"}


@pytest.mark.parametrize("name", sorted(MODULES))
@pytest.mark.parametrize("dim", [2, 3])
def test_boundary_group_rule_by_type(name, dim):
    pid, v2, v3, _ = MODULES[name]
    right = (v2, v3)[dim - 2]
    if right is None:
        return
    for bc in BCS:
        if bc in TAKES[name]:
            accepted(pid, dim, right, bc=bc)
        else:
            msg = refused(REFUSAL[name], pid, dim, right, bc=bc)
            if name == "linearelasticity+thermal":
                assert "MHA_BC_WEAK_DIRICHLET" in msg and "MHA_BC_INTERFACE" in msg
            if name == "linearelasticity":
                assert "(MHA_BC_INTERFACE) is not built" in msg


@pytest.mark.parametrize("dim", [2, 3])
def test_a_block_without_a_module_takes_every_valid_type(dim):
    for bc in BCS:
        accepted(0, dim, [H], bc=bc)


@pytest.mark.parametrize("dim", [2, 3])
def test_thermoelastic_neumann_side_with_data_for_e(dim):
    pid, right = MODULES["linearelasticity+thermal"][0], [H] * (dim + 1)
    accepted(pid, dim, right, bc=NEUMANN, side="top")
    msg = refused("on e", pid, dim, right, bc=NEUMANN, side="top", neumann_e=True)
    assert "'Neumann e top'" in msg and "not built for the coupled block" in msg
    # the displacements at the block's order (a traction group on e's higher order is not built)
    accepted(pid, dim, right, orders=[2] * dim + [1], bc=NEUMANN, block_order=2)
    refused("order of e not above the displacements'", pid, dim, right, orders=[1] * dim + [2], bc=NEUMANN, block_order=2)


@pytest.mark.parametrize("dim", [2, 3])
def test_size_limits_of_the_boundary_kernels(dim):
    # thermal_boundary_supported: n <= 32 dofs per element, nqs <= 16 side points -- every module without a rule of its own
    for pid in (0, MODULES["thermal"][0], MODULES["cdr"][0]):
        accepted(pid, dim, [H], cards=[32], bc=NEUMANN, nqs=16)
        refused("boundary terms are not available for 33 dofs per element with 16 side", pid, dim, [H], cards=[33], bc=NEUMANN, nqs=16)
        refused("boundary terms are not available for 32 dofs per element with 17 side", pid, dim, [H], cards=[32], bc=NEUMANN, nqs=17)
    accepted(MODULES["porousMixed"][0], dim, [HVOL, HDIV], cards=[8, 24], bc=WEAK_DIRICHLET, nqs=16)
    refused("boundary terms are not available for 33 dofs", MODULES["porousMixed"][0], dim, [HVOL, HDIV], cards=[8, 25],
            bc=WEAK_DIRICHLET, nqs=16)
    # linearelasticity_boundary_supported: n a multiple of dim, n / dim <= 27, nqs <= 16
    pid = MODULES["linearelasticity"][0]
    text = "linearelasticity boundary terms are not available for"
    accepted(pid, dim, [H] * dim, cards=[27] * dim, bc=WEAK_DIRICHLET, nqs=16)
    refused(text, pid, dim, [H] * dim, cards=[28] * dim, bc=WEAK_DIRICHLET, nqs=16)
    refused(text, pid, dim, [H] * dim, cards=[27] * dim, bc=NEUMANN, nqs=17)
    refused(text, pid, dim, [H] * dim, cards=[27] * (dim - 1) + [26], bc=NEUMANN, nqs=16)  # n no multiple of dim
    # the coupled block: dim x the displacement card, whatever e has
    pid = MODULES["linearelasticity+thermal"][0]
    accepted(pid, dim, [H] * (dim + 1), cards=[27] * dim + [8], bc=NEUMANN, nqs=16)
    refused(text + " 28 dofs per component", pid, dim, [H] * (dim + 1), cards=[28] * dim + [8], bc=NEUMANN, nqs=16)
    refused(text, pid, dim, [H] * (dim + 1), cards=[27] * dim + [8], bc=NEUMANN, nqs=17)
    # helmholtz_boundary_supported: n even, n / 2 <= 27, 0 < nqs <= 16
    pid = MODULES["helmholtz"][0]
    text = "helmholtz boundary terms are not available for"
    accepted(pid, dim, [H, H], cards=[27, 27], bc=NEUMANN, nqs=16)
    refused(text + " 56 dofs per element", pid, dim, [H, H], cards=[28, 28], bc=NEUMANN, nqs=16)
    refused(text, pid, dim, [H, H], cards=[27, 27], bc=NEUMANN, nqs=17)
    refused(text, pid, dim, [H, H], cards=[27, 27], bc=NEUMANN, nqs=0)


def test_the_hook_is_not_part_of_the_boundary():
    lib = mrhyde_amd.load_library()
    assert hasattr(lib, "mha_test_module_rules") and "mha_test_module_rules" not in mrhyde_amd.api.EXPORTS
