"""porousMixed heterogeneous permeability, direct form (MHA_POROUS_DATABASE=0), 128^3 hexes, uniform and warped:
  A constant Kinv   B three IP-array Kinv (1 / data at every point)   C element data
  D KL field, 4x4x4 stochastic terms   E C and D together
Jacobian + residual assemblies (overwrite), timed with HIP events; `--rounds` rounds alternate A..E, each round the median
of `--iters` assemblies; the table prints the median over rounds.  C is checked against B at the timed size.
Results: profiles/porous_heterogeneous.md."""
import argparse
import os
import sys

os.environ["MHA_POROUS_DATABASE"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mrhyde_amd  # noqa: E402


def warp(m):
    v = m["verts"].copy()
    w = v.copy()
    w[:, 0] += 0.06 * np.sin(1.3 * v[:, 1] + 0.4) + 0.04 * v[:, 2] ** 2
    w[:, 1] += 0.05 * np.cos(1.1 * v[:, 0]) * (1 + 0.5 * v[:, 1])
    w[:, 2] += 0.05 * v[:, 0] * v[:, 1] + 0.03 * np.sin(2.0 * v[:, 2])
    m["nodes"] = np.ascontiguousarray(w[m["cell2vert"]])
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--mesh", default="uniform,warped")
    args = ap.parse_args()
    nc = args.ncell
    for mesh in args.mesh.split(","):
        m = mrhyde_amd.mesh_multi(3, (nc,) * 3, [mrhyde_amd.BASIS_HVOL, mrhyde_amd.BASIS_HDIV], [0, 1])
        if mesh == "warped":
            m = warp(m)
        E = m["nelem"]
        rng = np.random.default_rng(3)
        data = rng.uniform(0.5, 2.0, E)
        u = torch.tensor(rng.uniform(-1, 1, m["ndof"]), device="cuda")
        blocks = {}
        for v in "ABCDE":
            blk = mrhyde_amd.Block(3, quadrature=2, physics="porousMixed", workset_size=E,
                                   variables=[(mrhyde_amd.BASIS_HVOL, 0), (mrhyde_amd.BASIS_HDIV, 1)])
            blk.set_mesh(m["nodes"], m["lids"], m["offsets"], m["ndof"], None)
            blk.set_orientation(m["orient"])
            blk.set_graph()
            blk.set_function("source", ("sinprod", 2.0, [1.1, 0.7, 1.9]))
            blk.set_function("total_mobility", 1.9)
            for k, c in zip(("Kinv_xx", "Kinv_yy", "Kinv_zz"), (1.3, 0.7, 2.1)):
                blk.set_function(k, c)
            if v == "B":
                kinv = torch.tensor(np.repeat(1.0 / data[:, None], 8, axis=1), device="cuda")
                for k in ("Kinv_xx", "Kinv_yy", "Kinv_zz"):
                    blk.set_function(k, kinv)
            if v in "CE":
                blk.set_element_data(data)
                blk.set_physics_parameter("use permeability data", 1)
            if v in "DE":
                blk.set_physics_parameter("use KL expansion", 1)
                blk.set_physics_parameter("fix_KL_3d", 1)
                for d in "xyz":
                    for key, val in (("N", 4), ("L", 1.0), ("sigma", 1.0), ("eta", 0.2)):
                        blk.set_physics_parameter("KL %s %s" % (key, d), val)
                blk.set_parameter_vector("KLStochcoeffs", rng.normal(0, 0.3, 64))
            rowptr, colind = blk.get_graph()
            res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
            vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
            blk.assemble_jacres(u, res, vals, overwrite=True)
            torch.cuda.synchronize()
            assert blk.info("porous_direct") == 1
            blocks[v] = (blk, res, vals)
        eC = max(float((blocks["C"][i] - blocks["B"][i]).abs().max() / blocks["B"][i].abs().max()) for i in (1, 2))
        times = {v: [] for v in blocks}
        for _ in range(args.rounds):
            for v, (blk, res, vals) in blocks.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
                blk.assemble_jacres(u, res, vals, overwrite=True)
                ev[0].record()
                for i in range(args.iters):
                    blk.assemble_jacres(u, res, vals, overwrite=True)
                    ev[i + 1].record()
                torch.cuda.synchronize()
                times[v].append(float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(args.iters)])))
        a = np.median(times["A"])
        print("%s %d^3: C vs B max rel diff %.2e" % (mesh, nc, eC))
        for v in "ABCDE":
            t = np.median(times[v])
            print("  %s  %.3f ms  (%+.1f %% vs A; rounds %s)" % (v, t, 100 * (t / a - 1), " ".join("%.3f" % x for x in times[v])))
        sys.stdout.flush()
        del blocks
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
