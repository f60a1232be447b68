"""Step time of the linearelasticity block beside a navierstokes block on the same cells (profiles/linearelasticity.md).
HIP-event time of repeated assemblies (Jacobian + residual, overwrite, transient stage), after a warm-up of every shape,
over windows of more than 150 ms; three windows per block and path.
Usage: python profiles/linearelasticity_cost.py [order] [ncell]     (3-D; order 1 or 2)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrhyde_amd  # noqa: E402
from ns_thermal_cost import PATHS, block, timed  # noqa: E402


def main():
    order = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    nc = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    dim, qdeg = 3, 2 * order
    lef = {"lambda": ("sinprod", 1.7, [0.9, 1.1, 0.7]), "mu": 0.8, "source dx": 0.3, "source dy": ("sinprod", 1.0, [1.0, 2.0, 0.5])}
    nsf = {"source ux": 0.3, "source uy": ("sinprod", 1.0, [1.0, 2.0, 0.5]), "viscosity": 0.05, "density": 1.3}
    cases = {
        "linearelasticity": ([order] * dim, dict(funcs=lef)),
        "navierstokes": ([order, 1] + [order] * (dim - 1), dict(funcs=nsf)),
    }
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    result = dict(order=order, ncell=nc, num_cu=num_cu)
    for name, (orders, settings) in cases.items():
        blk, m, st = block(dim, nc, name, orders, qdeg, settings)
        r = dict(elements=m["nelem"], dofs_per_element=int(m["lids"].shape[1]), rows=int(m["ndof"]), nnz=int(st["vals"].numel()))
        for pname, path in PATHS.items():
            r[pname] = timed(blk, st, path)
        result[name] = r
        print(json.dumps({name: r}), flush=True)
        del blk, st
        torch.cuda.empty_cache()
    for pname in PATHS:
        result[pname + "_ratio_le_over_ns"] = min(result["linearelasticity"][pname]["ms"]) / min(result["navierstokes"][pname]["ms"])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
