"""Cost of the Boussinesq coupling: the coupled navierstokes + thermal block against the sum of a navierstokes block and a
thermal block on the same cells (profiles/ns_thermal.md).  HIP-event time of repeated assemblies (Jacobian + residual,
overwrite), after a warm-up of every shape, over a window of more than 100 ms; three windows per block.
Usage: python profiles/ns_thermal_cost.py [2d|3d] [ncell]"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mrhyde_amd  # noqa: E402

H = mrhyde_amd.BASIS_HGRAD
PATHS = {"point_engine": mrhyde_amd.PATH_POINT_ENGINE, "row_gather": mrhyde_amd.PATH_ROW_GATHER}


def block(dim, nc, physics, orders, qdeg, settings):
    m = mrhyde_amd.mesh_multi(dim, (nc,) * dim, [H] * len(orders), orders)
    blk = mrhyde_amd.Block(dim, quadrature=qdeg, physics=physics, variables=[(H, o) for o in orders])
    blk.set_mesh(m["nodes"], m["lids"], m["offsets"], m["ndof"])
    blk.set_orientation(m["orient"])
    blk.set_graph()
    for k, v in settings.get("funcs", {}).items():
        blk.set_function(k, v)
    for k, v in settings.get("params", {}).items():
        blk.set_physics_parameter(k, v)
    rowptr, colind = blk.get_graph()
    rng = np.random.default_rng(7)
    A, b, bdf = np.array([[0.5, 0.0], [0.3, 0.7]]), np.array([0.4, 0.6]), np.array([1.5, -2.0, 0.5])
    blk.set_time_integration(True, 2, 2, 1, 0.05, A, b, bdf)
    nd = m["ndof"]
    st = dict(u=torch.tensor(rng.uniform(-1, 1, nd), device="cuda"),
              u_prev=torch.tensor(rng.uniform(-1, 1, (nd, 2)), device="cuda"),
              u_stage=torch.tensor(rng.uniform(-1, 1, (nd, 2)), device="cuda"),
              res=torch.zeros(nd, dtype=torch.float64, device="cuda"),
              vals=torch.zeros(len(colind), dtype=torch.float64, device="cuda"))
    return blk, m, st


def timed(blk, st, path):
    def go():
        blk.assemble_jacres(st["u"], st["res"], st["vals"], path=path, overwrite=True, u_prev=st["u_prev"], u_stage=st["u_stage"])
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


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "2d"
    dim, (ov, op, oe), qdeg = (2, (2, 1, 2), 4) if which == "2d" else (3, (1, 1, 1), 2)
    nc = int(sys.argv[2]) if len(sys.argv) > 2 else (512 if dim == 2 else 64)
    vel = [ov, op] + [ov] * (dim - 1)
    nsf = {"source ux": 0.3, "source uy": ("sinprod", 1.0, [1.0, 2.0, 0.5][:dim]), "viscosity": 0.05, "density": 1.3}
    thf = {"thermal source": ("sinprod", 3.0, [2.0, 1.0, 1.5][:dim]), "thermal diffusion": 1.7, "specific heat": 1.4}
    stab = {"useSUPG": 1, "usePSPG": 1}
    cases = {
        "navierstokes+thermal": (vel + [oe], dict(funcs=dict(nsf, **thf), params=dict(stab, beta=0.7, T_ambient=0.3))),
        "navierstokes": (vel, dict(funcs=nsf, params=stab)),
        "thermal": ([oe], dict(funcs=dict(thf, density=1.3))),
    }
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    result = dict(case=which, ncell=nc, num_cu=num_cu)
    for name, (orders, settings) in cases.items():
        blk, m, st = block(dim, nc, name, orders, qdeg, settings)
        r = dict(elements=m["nelem"], dofs_per_element=int(m["lids"].shape[1]), rows=int(m["ndof"]), nnz=int(st["vals"].numel()),
                 elements_per_cu=m["nelem"] / num_cu)
        for pname, path in PATHS.items():
            if name == "thermal" and pname == "row_gather":
                continue  # (thermal's row gather takes its own element kernel, not the engine)
            r[pname] = timed(blk, st, path)
        result[name] = r
        del blk, st
        torch.cuda.empty_cache()
    pe = lambda k: min(result[k]["point_engine"]["ms"])
    result["point_engine_ratio_coupled_over_sum"] = pe("navierstokes+thermal") / (pe("navierstokes") + pe("thermal"))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
