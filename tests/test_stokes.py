"""CPU tests of the stokes module (MHA_PHYSICS_STOKES): the yardstick tests/stokes_ref.py against the reference's two
golds and against a finite difference of itself, the module's variable rule and ids, and the host-only dispatch check of
the two new modules.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mrhyde_amd
import shallowwater_ref as W
import stokes_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "reference")
HGRAD, HVOL = 0, 1
PID = 14


def test_gold_2d_verification_pspg(oracle):
    """One direct solve; each value to half a unit of the gold's last printed digit.  With tau = h^2 / (2 nu) the values
    would be 0.0101669, 0.102239, 0.00098238: the gold tells the 2-D tau from the 3-D one."""
    gold = W.read_gold(os.path.join(GOLD, "stokes_2D_verification_pspg.gold"))
    assert sorted(gold) == ["pr", "ux", "uy"] and [gold[k][0][0] for k in ("ux", "pr", "uy")] == ["0.0188527", "0.193776", "0.00063617"]
    got = R.gold_pspg(oracle, R.host_assembler(oracle, 2, dict(usePSPG=1)))
    for k, ((s, t),) in gold.items():
        print(k, got[k], s)
        assert t == 0.0 and abs(got[k] - float(s)) <= W.half_unit(s), (k, got[k], s)


def test_gold_channel(oracle):
    """The gold's values are round-off (1e-16 to 1e-18): the exact solution lies in the Q2/Q1 space.  A wrong term shows at
    1e-4 and above."""
    gold = W.read_gold(os.path.join(GOLD, "stokes_channel.gold"))
    assert sorted(gold) == ["pr", "ux", "uy"] and all(float(v[0][0]) < 1e-15 for v in gold.values())
    got = R.gold_channel(oracle, R.host_assembler(oracle, 2))
    for k in gold:
        print(k, got[k])
        assert got[k] < 1e-12, (k, got[k])


@pytest.mark.parametrize("transient", [False, True])
def test_ad_jacobian_against_a_central_difference(oracle, transient):
    """PSPG + LSIC on a warped 3x3 mesh: the AD Jacobian against a central difference of the yardstick's own residual,
    step 1e-6, 1e-7 relative to the matrix's largest entry."""
    rng = np.random.default_rng(141)
    m = R.stokes_mesh(oracle, 2, (3, 3), (1, 1))
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"]) if transient else None
    kw = dict(funcs={"source ux": 0.3, "source uy": "sin(x)*y", "viscosity": "0.7+0.1*x"}, params=dict(usePSPG=1, useLSIC=1),
              transient=tr)
    ref = R.assemble(oracle, m, 2, u, **kw)
    import scipy.sparse as sp
    J = sp.csr_matrix((ref["crs_vals"], ref["colind"], ref["rowptr"]), shape=(m["ndof"],) * 2).toarray()
    fd = np.zeros_like(J)
    eps = 1e-6
    for j in range(m["ndof"]):
        up, um = u.copy(), u.copy()
        up[j] += eps
        um[j] -= eps
        # the scatter stores -res.val() in the vector and +res.dx in the matrix
        fd[:, j] = -(R.residual_only(oracle, m, 2, up, **kw) - R.residual_only(oracle, m, 2, um, **kw)) / (2 * eps)
    err = np.abs(J - fd).max() / np.abs(J).max()
    print("AD against central difference:", err)
    assert err < 1e-7


def ask(pid, dim, types, orders=None):
    lib = mrhyde_amd.load_library()
    f = lib.mha_test_module_rules
    f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int, C.c_char_p] + [C.c_int] * 4
    orders = [1] * len(types) if orders is None else orders
    t, o = np.asarray(types, np.int32), np.asarray(orders, np.int32)
    c = np.asarray([1 if b == HVOL else (k + 1) ** dim for b, k in zip(types, orders)], np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    code = f(pid, dim, len(types), vp(t), vp(o), vp(c), 0, b"left", int(c.sum()), 1, 2 ** (dim - 1), 0)
    return code, lib.mha_last_error().decode()


@pytest.mark.parametrize("dim", [2, 3])
def test_variable_rule(dim):
    right = [HGRAD] * (dim + 1)
    text = "stokes needs ux, pr, uy, uz, in that order" if dim == 3 else "stokes needs ux, pr, uy, in that order"
    assert ask(PID, dim, right) == (0, "")
    assert ask(PID, dim, right, [2, 1] + [2] * (dim - 1)) == (0, "")  # Q2/Q1: the orders are free per variable
    for wrong in (right[:-1], right + [HGRAD], right[:-1] + [HVOL]):
        code, msg = ask(PID, dim, wrong)
        assert code == 1 and text in msg, (wrong, code, msg)


def test_module_ids_and_names():
    src = open(os.path.join(HERE, "..", "include", "mrhyde_amd.h")).read()
    for name, key, pid in (("STOKES", "stokes", 14), ("SHALLOWWATER", "shallowwater", 15)):
        m = re.search(r"#define\s+MHA_PHYSICS_%s\s+\(MHA_PHYSICS_LINEARELASTICITY_THERMAL \+ (\d+)\)" % name, src)
        assert m and 7 + int(m.group(1)) == pid == mrhyde_amd.MODULE_IDS[key] == getattr(mrhyde_amd, "PHYSICS_" + name)
        assert pid not in mrhyde_amd.ALL_PHYSICS_IDS.values() and key not in mrhyde_amd.ALL_PHYSICS_IDS
    assert mrhyde_amd.ALL_PHYSICS_IDS == {"thermal": 1, "porousMixed": 2, "navierstokes": 3, "shallowwaterHybridized": 4,
                                          "navierstokes+thermal": 5, "linearelasticity": 6, "linearelasticity+thermal": 7,
                                          "cdr": 8, "navierstokes+cdr": 9, "helmholtz": 10}
    assert all(mrhyde_amd.MODULE_IDS[k] == v for k, v in mrhyde_amd.ALL_PHYSICS_IDS.items())
    assert sorted(mrhyde_amd.MODULE_IDS.values()) == list(range(1, 11)) + [12, 13, 14, 15]  # 11 names no module


def test_parameters():
    for name in ("usePSPG", "useLSIC"):
        mrhyde_amd.module_parameter("stokes", 2, name, 1)
    for name in ("useSUPG", "fix_uz_offsets", "gravity"):
        with pytest.raises(mrhyde_amd.MhaError, match="has no parameter '%s'" % name) as ei:
            mrhyde_amd.module_parameter("stokes", 3, name, 1)
        assert ei.value.code == 1


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_dispatch_table_of_the_two_modules(tmp_path):
    exe = tmp_path / "stokes_shallowwater_dispatch_check"
    build = subprocess.run([HIPCC, "-std=c++17", "-O0", "-Wall", "-Wextra", "-Wno-unused-parameter", "-x", "hip",
                            "--cuda-host-only", os.path.join(HERE, "stokes_shallowwater_dispatch_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
