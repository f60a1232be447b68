"""Time per step of the fused HDG subgrid element step (mha_swhdg_condensed_subgrid) at 256^2 macro elements x m = 2 and
128^2 x m = 4, beside the one-element step (mha_swhdg_condensed_element) at 512^2: 262 144 sub-elements each.  Device
events around `steps` calls after `warmup` calls; transient, mixed side types.  Usage: python profiles/swhdg_subgrids.py
[steps] [only]   (only = m of a single case, 0 = the one-element step: for a profiler run)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrhyde_amd  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
only = int(sys.argv[2]) if len(sys.argv) > 2 else -1
warmup = 5


def run(nmacro, m, layout):
    sm = mrhyde_amd.mesh_swhdg_subgrids((nmacro, nmacro), m)
    rng = np.random.default_rng(5)
    nd, Em = sm["ndof"], sm["nmacro"]
    isH = (np.arange(nd) % 3) == 0
    u = rng.uniform(-1, 1, nd)
    u[isH] = rng.uniform(1.0, 2.0, isH.sum())
    lam = rng.uniform(-1, 1, (Em, 3, 4, 2))
    lam[:, 0] = rng.uniform(1.0, 2.0, (Em, 4, 2))
    st = rng.integers(0, 3, (Em, 4)).astype(np.uint8)
    up, us = rng.uniform(-1, 1, (nd, 2)), rng.uniform(-1, 1, (nd, 2))
    up[isH], us[isH] = rng.uniform(1.0, 2.0, (isH.sum(), 2)), rng.uniform(1.0, 2.0, (isH.sum(), 2))
    blk = mrhyde_amd.Block(2, quadrature=2, physics="shallowwaterHybridized", variables=[(mrhyde_amd.BASIS_HGRAD, 1)] * 3)
    blk.set_mesh(sm["nodes"], sm["lids"], sm["offsets"], nd)
    blk.set_graph()
    blk.set_time_integration(True, 2, 2, 1, 0.05 / (nmacro * m), np.array([[0.5, 0.0], [0.3, 0.7]]), np.array([0.4, 0.6]),
                             np.array([1.5, -2.0, 0.5]))
    if layout:
        blk.set_swhdg_subgrids(m)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")
    ud, ld, sd, pd, gd = t(u), t(lam.reshape(Em, 24)), t(st), t(up), t(us)
    S = torch.zeros((Em, 24, 24), dtype=torch.float64, device="cuda")
    g = torch.zeros((Em, 24), dtype=torch.float64, device="cuda")
    du = torch.zeros((Em, sm["n_int"]), dtype=torch.float64, device="cuda")
    ns = torch.zeros(1, dtype=torch.int32, device="cuda")
    step = blk.swhdg_condensed_subgrid if layout else blk.swhdg_condensed_element
    call = lambda: step(ud, ld, schur=S, gvec=g, du=du, num_singular=ns, side_types=sd, farfield=[1.4, -0.3, 0.5], u_prev=pd, u_stage=gd)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(3):                                     # three windows: the spread is reported
        e0.record()
        for _ in range(steps):
            call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / steps)
    assert int(ns[0]) == 0 and bool(torch.isfinite(S).all())
    nsub = Em * m * m
    print("%-28s %7d macro x m=%d: %8.3f ms/step (windows %s), %6.2f ns per sub-element" % (
        "condensed_subgrid" if layout else "condensed_element (1 elem)", Em, m, min(times),
        " ".join("%.3f" % x for x in times), 1e6 * min(times) / nsub), flush=True)
    blk.close()


for nm, m, layout in ((512, 1, False), (256, 2, True), (128, 4, True), (512, 1, True), (171, 3, True)):
    if only >= 0 and (m if layout else 0) != only:
        continue
    run(nm, m, layout)
