"""Step times of the stokes and shallowwater blocks (profiles/stokes_shallowwater.md), one process per configuration:
the assembly (Jacobian + residual, overwrite, transient stage, point-engine path with its atomic scatter, and the row
gather that MHA_PATH_AUTO takes), the matrix-free products J x and J^T x, and the Jacobian diagonal.
  * stokes beside a navierstokes block on the same cells (the same variable layout and engine, a shorter point function);
  * shallowwater beside the volume terms of shallowwaterHybridized on the same cells (three HGRAD variables each).
HIP-event time of repeated calls after a warm-up of every shape, over windows of more than 150 ms; three windows each.
Usage: python profiles/stokes_shallowwater_cost.py CONFIG [ncell]
  CONFIG: stokes3d (64^3 Q2/Q1) | stokes2d (512^2 Q2/Q1) | shallowwater_q1 (1024^2 Q1) | shallowwater_q2 (512^2 Q2)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrhyde_amd  # noqa: E402
from helmholtz_cost import windows  # noqa: E402
from ns_thermal_cost import block  # noqa: E402

CONFIGS = {"stokes3d": (3, 64, (2, 1), 4), "stokes2d": (2, 512, (2, 1), 4), "shallowwater_q1": (2, 1024, (1,), 2),
           "shallowwater_q2": (2, 512, (2,), 4)}
KEYS = ("assembly", "assembly_row_gather", "apply", "apply_transpose", "diagonal")


def positive_depth(m, st):
    """the first variable (xi of shallowwater, the depth H of shallowwaterHybridized) in [0.5, 1.5] in every state array"""
    rows = torch.tensor(np.flatnonzero(m["dof_var"] == 0), device="cuda")
    for k in ("u", "u_prev", "u_stage"):
        st[k][rows] = st[k][rows].abs() + 0.5


def main():
    which = sys.argv[1]
    dim, nc, orders, qdeg = CONFIGS[which]
    nc = int(sys.argv[2]) if len(sys.argv) > 2 else nc
    src = ("sinprod", 1.0, [1.0, 2.0, 0.5][:dim])
    if which.startswith("stokes"):
        ov, op = orders
        layout = [ov, op] + [ov] * (dim - 1)
        f = {"source ux": 0.3, "source uy": src, "viscosity": 0.05}
        cases = {"stokes": ("stokes", layout, dict(funcs=f, params={"usePSPG": 1, "useLSIC": 1})),
                 "navierstokes": ("navierstokes", layout, dict(funcs=dict(f, density=1.3), params={"useSUPG": 1, "usePSPG": 1}))}
    else:
        layout = [orders[0]] * 3
        cases = {"shallowwater": ("shallowwater", layout, dict(funcs={"bathymetry": 0.8, "bathymetry_x": 0.1, "source Hu": src})),
                 "shallowwaterHybridized": ("shallowwaterHybridized", layout, dict(funcs={"source Hux": src}))}
    new, old = list(cases)
    result = dict(config=which, ncell=nc, num_cu=torch.cuda.get_device_properties(0).multi_processor_count)
    for name, (physics, lay, settings) in cases.items():
        blk, m, st = block(dim, nc, physics, lay, qdeg, settings)
        if not which.startswith("stokes"):
            positive_depth(m, st)
        kw = dict(u_prev=st["u_prev"], u_stage=st["u_stage"])
        x, y = torch.ones_like(st["u"]), torch.zeros_like(st["u"])
        r = dict(elements=m["nelem"], dofs_per_element=int(m["lids"].shape[1]), rows=int(m["ndof"]), nnz=int(st["vals"].numel()))
        r["assembly"] = windows(lambda: blk.assemble_jacres(st["u"], st["res"], st["vals"], path=mrhyde_amd.PATH_POINT_ENGINE,
                                                            overwrite=True, **kw))
        r["assembly_row_gather"] = windows(lambda: blk.assemble_jacres(st["u"], st["res"], st["vals"],
                                                                       path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw))
        r["apply"] = windows(lambda: blk.apply_jacobian(st["u"], x, y, overwrite=True, **kw))
        r["apply_transpose"] = windows(lambda: blk.apply_jacobian(st["u"], x, y, transpose=True, overwrite=True, **kw))
        r["diagonal"] = windows(lambda: blk.jacobian_diagonal(st["u"], y, overwrite=True, **kw))
        assert bool(torch.isfinite(st["res"]).all()) and bool(torch.isfinite(y).all())
        result[name] = r
        print(json.dumps({name: r}), flush=True)
        del blk, st
        torch.cuda.empty_cache()
    for k in KEYS:
        result["%s_%s_over_%s" % (k, new, old)] = min(result[new][k]["ms"]) / min(result[old][k]["ms"])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
