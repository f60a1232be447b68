"""CPU side of the matrix-free boundary-group products (mha_apply_boundary_jacobian, mha_boundary_jacobian_diagonal;
Block.apply_boundary_jacobian, Block.boundary_jacobian_diagonal): the prototypes against the header, the exports and the
Python signatures.  The products themselves are checked on the device (tests/test_boundary_apply_gpu.py) with the helpers
of tests/test_jacobian_apply.py and tests/test_jacobian_diag_multi.py."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prototypes_are_in_the_header():
    text = open(os.path.join(ROOT, "include", "mrhyde_amd.h")).read()
    assert re.search(r"int\s+mha_apply_boundary_jacobian\(mha_context \*ctx, int flags, const double \*u_dev, const double \*u_prev_dev,\s*"
                     r"const double \*u_stage_dev, const double \*x_dev, double \*y_dev\);", text)
    assert re.search(r"int\s+mha_boundary_jacobian_diagonal\(mha_context \*ctx, int flags, const double \*u_dev, const double \*u_prev_dev,\s*"
                     r"const double \*u_stage_dev, double \*d_dev\);", text)
    # the volume products no longer send the user to the assembled boundary matrix
    assert not re.search(r"Not built:[^/]*boundary-group terms", text)


def test_names_are_exported():
    import mrhyde_amd
    lib = mrhyde_amd.load_library()
    for name in ("mha_apply_boundary_jacobian", "mha_boundary_jacobian_diagonal"):
        assert name in mrhyde_amd.api.EXPORTS
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)


def test_block_method_signatures():
    import mrhyde_amd
    sig = inspect.signature(mrhyde_amd.Block.apply_boundary_jacobian)
    assert list(sig.parameters) == ["self", "u", "x", "y", "transpose", "u_prev", "u_stage"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["transpose"] is False and d["u_prev"] is None and d["u_stage"] is None
    sig = inspect.signature(mrhyde_amd.Block.boundary_jacobian_diagonal)
    assert list(sig.parameters) == ["self", "u", "d", "u_prev", "u_stage"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["u_prev"] is None and d["u_stage"] is None


def test_apply_jacobian_signature_is_unchanged():
    import mrhyde_amd
    sig = inspect.signature(mrhyde_amd.Block.apply_jacobian)
    assert list(sig.parameters) == ["self", "u", "x", "y", "transpose", "overwrite", "u_prev", "u_stage"]
    sig = inspect.signature(mrhyde_amd.Block.jacobian_diagonal)
    assert list(sig.parameters) == ["self", "u", "d", "overwrite", "u_prev", "u_stage"]
