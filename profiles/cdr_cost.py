"""Step time of the cdr block and of the coupled navierstokes + cdr block (profiles/cdr.md).
  * cdr with constants and with reaction: '0.5*c*c' beside the thermal + "include advection" block of the same shape: the
    same operator when the reaction is constant, through a point function the two modules do not share;
  * the coupled block (xvel: 'ux', ...) beside the sum of a navierstokes and a cdr block on the same cells.
HIP-event time of repeated assemblies (Jacobian + residual, overwrite, transient stage) on the point-engine path (atomic
scatter), after a warm-up of every shape, over windows of more than 150 ms; three windows per block.
Usage: python profiles/cdr_cost.py [2d|3d] [ncell]       (2d: 512^2 Q2 / Q2,Q1,Q2,Q2;  3d: 64^3 Q1)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrhyde_amd  # noqa: E402
from ns_thermal_cost import block, timed  # noqa: E402


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "3d"
    dim, (ov, op, oc), qdeg = (2, (2, 1, 2), 4) if which == "2d" else (3, (1, 1, 1), 2)
    nc = int(sys.argv[2]) if len(sys.argv) > 2 else (512 if dim == 2 else 64)
    vel = [ov, op] + [ov] * (dim - 1)
    b = [0.7, -1.1, 0.4][:dim]
    src = ("sinprod", 3.0, [2.0, 1.0, 1.5][:dim])
    cdrf = dict(zip(["xvel", "yvel", "zvel"], b), source=src, diffusion=1.7, reaction=0.6)
    thf = dict(zip(["bx", "by", "bz"], b), **{"thermal source": src, "thermal diffusion": 1.7})
    nsf = {"source ux": 0.3, "source uy": ("sinprod", 1.0, [1.0, 2.0, 0.5][:dim]), "viscosity": 0.05, "density": 1.3}
    stab = {"useSUPG": 1, "usePSPG": 1}
    coupling = dict(zip(["xvel", "yvel", "zvel"], ["ux", "uy", "uz"][:dim]))
    cases = {
        "cdr constants": ("cdr", [oc], dict(funcs=cdrf)),
        "cdr reaction 0.5*c*c": ("cdr", [oc], dict(funcs=dict(cdrf, reaction="0.5*c*c"))),
        "thermal + advection": ("thermal", [oc], dict(funcs=thf, params={"include advection": 1})),
        "navierstokes+cdr": ("navierstokes+cdr", vel + [oc],
                             dict(funcs=dict(nsf, source=src, diffusion=1.7, reaction="0.5*c*c", **coupling), params=stab)),
        "navierstokes": ("navierstokes", vel, dict(funcs=nsf, params=stab)),
    }
    result = dict(case=which, ncell=nc, num_cu=torch.cuda.get_device_properties(0).multi_processor_count)
    for name, (physics, orders, settings) in cases.items():
        blk, m, st = block(dim, nc, physics, orders, qdeg, settings)
        r = dict(elements=m["nelem"], dofs_per_element=int(m["lids"].shape[1]), rows=int(m["ndof"]), nnz=int(st["vals"].numel()))
        r["point_engine"] = timed(blk, st, mrhyde_amd.PATH_POINT_ENGINE)
        result[name] = r
        print(json.dumps({name: r}), flush=True)
        del blk, st
        torch.cuda.empty_cache()
    t = lambda k: min(result[k]["point_engine"]["ms"])
    result["cdr_constants_over_thermal_advection"] = t("cdr constants") / t("thermal + advection")
    result["cdr_fields_over_thermal_advection"] = t("cdr reaction 0.5*c*c") / t("thermal + advection")
    result["coupled_over_sum"] = t("navierstokes+cdr") / (t("navierstokes") + t("cdr reaction 0.5*c*c"))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
