"""Step times of the helmholtz block beside a plain thermal block on the same cells (profiles/helmholtz.md): the assembly
(Jacobian + residual, overwrite, point-engine path with its atomic scatter), the matrix-free products J x and J^T x, and
the Jacobian diagonal.  helmholtz has two variables where thermal has one: twice the rows, four times the matrix entries.
In 3-D also the Robin group of one face (`right`) beside the volume step.
HIP-event time of repeated calls after a warm-up of every shape, over windows of more than 150 ms; three windows each.
Usage: python profiles/helmholtz_cost.py [2d|3d] [ncell]       (2d: 512^2 Q2;  3d: 64^3 Q1)"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrhyde_amd  # noqa: E402
from ns_thermal_cost import block  # noqa: E402


def windows(go):
    for _ in range(3):  # warm-up: code objects, the one-time plans of the path
        go()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    go()
    t1.record()
    torch.cuda.synchronize()
    reps = max(5, int(math.ceil(150.0 / max(t0.elapsed_time(t1), 1e-3))))
    out = []
    for _ in range(3):
        t0.record()
        for _ in range(reps):
            go()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / reps)
    return dict(reps=reps, ms=out, window_ms=min(out) * reps)


def right_face(dim, nc):
    """(element ids, local side ids) of the x+ side of the structured mesh (elements numbered x-fastest; shards side 1)"""
    idx = np.arange(nc ** (dim - 1), dtype=np.int64)
    e = (nc - 1) + nc * idx
    return e.astype(np.int32), np.full(len(e), 1, dtype=np.int32)


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "3d"
    dim, order, qdeg = (2, 2, 4) if which == "2d" else (3, 1, 2)
    nc = int(sys.argv[2]) if len(sys.argv) > 2 else (512 if dim == 2 else 64)
    src = ("sinprod", 3.0, [2.0, 1.0, 1.5][:dim])
    hf = {"c2r_x": 1.3, "c2i_x": 0.35, "c2r_y": 0.9, "c2i_y": -0.45, "omega2r": 2.1, "omega2i": -0.6, "source_r": src,
          "source_i": -1.7, "robin_alpha_r": 0.55, "robin_alpha_i": -0.65, "source_r_side": 1.9, "source_i_side": 0.75}
    if dim == 3:
        hf.update({"c2r_z": 1.1, "c2i_z": 0.25})
    thf = {"thermal source": src, "thermal diffusion": 1.7, "specific heat": 1.4, "density": 1.3}
    cases = {"helmholtz": ("helmholtz", [order, order], dict(funcs=hf)), "thermal": ("thermal", [order], dict(funcs=thf))}
    result = dict(case=which, ncell=nc, num_cu=torch.cuda.get_device_properties(0).multi_processor_count)
    for name, (physics, orders, settings) in cases.items():
        blk, m, st = block(dim, nc, physics, orders, qdeg, settings)
        kw = dict(u_prev=st["u_prev"], u_stage=st["u_stage"])
        x, y = torch.ones_like(st["u"]), torch.zeros_like(st["u"])
        r = dict(elements=m["nelem"], dofs_per_element=int(m["lids"].shape[1]), rows=int(m["ndof"]), nnz=int(st["vals"].numel()))
        r["assembly"] = windows(lambda: blk.assemble_jacres(st["u"], st["res"], st["vals"], path=mrhyde_amd.PATH_POINT_ENGINE,
                                                            overwrite=True, **kw))
        r["apply"] = windows(lambda: blk.apply_jacobian(st["u"], x, y, overwrite=True, **kw))
        r["apply_transpose"] = windows(lambda: blk.apply_jacobian(st["u"], x, y, transpose=True, overwrite=True, **kw))
        r["diagonal"] = windows(lambda: blk.jacobian_diagonal(st["u"], y, overwrite=True, **kw))
        if name == "helmholtz" and dim == 3:
            be, bs = right_face(dim, nc)
            blk.add_boundary_group("right", mrhyde_amd.BC_NEUMANN, be, bs)
            r["robin_group_one_face"] = dict(entries=len(be), **windows(lambda: blk.assemble_boundary(st["u"], st["res"], st["vals"], **kw)))
        result[name] = r
        print(json.dumps({name: r}), flush=True)
        del blk, st
        torch.cuda.empty_cache()
    for k in ("assembly", "apply", "apply_transpose", "diagonal"):
        result[k + "_helmholtz_over_thermal"] = min(result["helmholtz"][k]["ms"]) / min(result["thermal"][k]["ms"])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
