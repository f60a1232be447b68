"""Cost of the thermoelastic coupling and of the stress output (profiles/thermoelastic.md): the coupled
linearelasticity + thermal block against a linearelasticity block and a thermal block on the same cells, and
derived_values against plain fills of its output arrays.  HIP-event time of repeated calls (Jacobian + residual, overwrite,
transient stage), after a warm-up of every shape, over windows of more than 150 ms; three windows per block and path.
Usage: MHA_ROW_GATHER_KERNEL=engine python profiles/thermoelastic_cost.py [order] [ncell]     (3-D; order 1 or 2)
(the variable routes the thermal block's row gather through the point engine, the kernel the coupled block runs)"""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrhyde_amd  # noqa: E402
from ns_thermal_cost import PATHS, block, timed  # noqa: E402


def windows(go):
    """three windows of more than 150 ms of go() after three warm-up calls -> ms per call"""
    for _ in range(3):
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


def main():
    order = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    nc = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    dim, qdeg = 3, 2 * order
    lef = {"lambda": ("sinprod", 1.7, [0.9, 1.1, 0.7]), "mu": 0.8, "source dx": 0.3, "source dy": ("sinprod", 1.0, [1.0, 2.0, 0.5])}
    thf = {"thermal source": ("sinprod", 3.0, [2.0, 1.0, 1.5]), "thermal diffusion": 1.7, "specific heat": 1.4, "density": 1.3}
    cases = {
        "linearelasticity+thermal": ([order] * (dim + 1), dict(funcs=dict(lef, **thf), params=dict(alpha_T=0.35, T_ambient=0.3))),
        "linearelasticity": ([order] * dim, dict(funcs=lef)),
        "thermal": ([order], dict(funcs=thf)),
    }
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    result = dict(order=order, ncell=nc, num_cu=num_cu, row_gather_kernel=os.environ.get("MHA_ROW_GATHER_KERNEL", ""))
    for name, (orders, settings) in cases.items():
        blk, m, st = block(dim, nc, name, orders, qdeg, settings)
        r = dict(elements=m["nelem"], dofs_per_element=int(m["lids"].shape[1]), rows=int(m["ndof"]), nnz=int(st["vals"].numel()))
        for pname, path in PATHS.items():
            r[pname] = timed(blk, st, path)
        if name != "thermal":
            E, nq = m["nelem"], blk.info("num_ip")
            stress = torch.zeros((E, nq, dim, dim), dtype=torch.float64, device="cuda")
            r["derived_values"] = windows(lambda: blk.derived_values(st["u"], stress=stress))
            r["derived_values_no_tensor"] = windows(lambda: blk.derived_values(st["u"]))
            vm, mag = torch.zeros((E, nq), dtype=torch.float64, device="cuda"), torch.zeros((E, nq), dtype=torch.float64, device="cuda")
            r["fill_outputs"] = windows(lambda: (stress.fill_(1.0), vm.fill_(1.0), mag.fill_(1.0)))
            r["output_bytes"] = 8 * E * nq * (dim * dim + 2)
            del stress, vm, mag
        result[name] = r
        print(json.dumps({name: r}), flush=True)
        del blk, st
        torch.cuda.empty_cache()
    for pname in PATHS:
        t = lambda k: min(result[k][pname]["ms"])
        result[pname + "_ratio_coupled_over_sum"] = t("linearelasticity+thermal") / (t("linearelasticity") + t("thermal"))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
