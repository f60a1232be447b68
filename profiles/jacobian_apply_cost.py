"""Time of the matrix-free Jacobian products (Block.apply_jacobian) beside the assembly they replace
(profiles/jacobian_apply.md).  Per case: the forward and the transposed product, assemble_jacres with and without the
Jacobian (MHA_PATH_AUTO), and the floor of the SpMV a product replaces -- one pass over the block's crs_vals (8 B) and
colind (4 B) at the copy rate measured on this device.  HIP-event time of repeated calls after a warm-up, over windows of
more than 150 ms; three windows each (the blocks and the window loop of profiles/ns_thermal_cost.py).
Usage: python profiles/jacobian_apply_cost.py [ns3d|ns2d|thermoelastic|cdr ...] [--ncell N]"""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrhyde_amd  # noqa: E402
from ns_thermal_cost import block  # noqa: E402

NSF = lambda dim: {"source ux": 0.3, "source uy": ("sinprod", 1.0, [1.0, 2.0, 0.5][:dim]), "viscosity": 0.05, "density": 1.3}
STAB = {"useSUPG": 1, "usePSPG": 1}
CASES = {
    "ns3d": (3, 64, "navierstokes", [2, 1, 2, 2], 4, lambda: dict(funcs=NSF(3), params=STAB)),
    "ns2d": (2, 512, "navierstokes", [2, 1, 2], 4, lambda: dict(funcs=NSF(2), params=STAB)),
    "thermoelastic": (3, 64, "linearelasticity+thermal", [1, 1, 1, 1], 2,
                      lambda: dict(funcs={"lambda": 1.7, "mu": 0.8, "thermal source": ("sinprod", 3.0, [2.0, 1.0, 1.5]),
                                          "thermal diffusion": 1.7}, params={"alpha_T": 0.35, "T_ambient": 0.3})),
    "cdr": (3, 64, "cdr", [1], 2, lambda: dict(funcs={"xvel": 0.7, "yvel": -1.1, "zvel": 0.4, "diffusion": 1.7,
                                                      "source": ("sinprod", 3.0, [2.0, 1.0, 1.5]), "reaction": "0.5*c*c"})),
}


def windows(go):
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
    return dict(reps=reps, ms=out)


def copy_rate_gbs():
    """bytes read + written per second of a device-to-device copy of 1 GiB"""
    a = torch.empty(1 << 27, dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    r = windows(lambda: b.copy_(a))
    return 2 * a.numel() * 8 / (min(r["ms"]) * 1e-3) / 1e9


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ncell = int(sys.argv[sys.argv.index("--ncell") + 1]) if "--ncell" in sys.argv else None
    rate = copy_rate_gbs()
    print(json.dumps(dict(copy_rate_GBs=rate, num_cu=torch.cuda.get_device_properties(0).multi_processor_count)), flush=True)
    for name in args or list(CASES):
        dim, nc, physics, orders, qdeg, settings = CASES[name]
        blk, m, st = block(dim, ncell or nc, physics, orders, qdeg, settings())
        kw = dict(u_prev=st["u_prev"], u_stage=st["u_stage"])
        x = torch.rand_like(st["u"]) + 0.5
        y = torch.zeros_like(st["u"])
        nnz = int(st["vals"].numel())
        r = dict(case=name, elements=m["nelem"], dofs_per_element=int(m["lids"].shape[1]), rows=int(m["ndof"]), nnz=nnz)
        r["forward"] = windows(lambda: blk.apply_jacobian(st["u"], x, y, overwrite=True, **kw))
        r["lds_bytes"], r["waves"] = blk.info("jacobian_apply_lds_bytes"), blk.info("jacobian_apply_waves")
        r["transposed"] = windows(lambda: blk.apply_jacobian(st["u"], x, y, transpose=True, overwrite=True, **kw))
        r["assembly"] = windows(lambda: blk.assemble_jacres(st["u"], st["res"], st["vals"], overwrite=True, **kw))
        r["residual_only"] = windows(lambda: blk.assemble_jacres(st["u"], st["res"], None, compute_jacobian=False,
                                                                 overwrite=True, **kw))
        r["spmv_floor_ms"] = nnz * 12 / (rate * 1e9) * 1e3
        t = lambda k: min(r[k]["ms"])
        for k in ("forward", "transposed"):
            extra = t(k) - r["spmv_floor_ms"]  # what a product costs more than the SpMV it replaces
            r["break_even_products_" + k] = t("assembly") / extra if extra > 0 else float("inf")
        print(json.dumps(r), flush=True)
        del blk, st
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
