"""Time of the matrix-free Jacobian diagonal (Block.jacobian_diagonal) and of the multi-vector products
(Block.apply_jacobian_multi) beside the single products and the assembly (profiles/jacobian_apply.md).  The cases, blocks
and window loop of profiles/jacobian_apply_cost.py: HIP-event time of repeated calls after a warm-up, over windows of more
than 150 ms, three windows each.  Per case: the single forward and transposed product, the diagonal, one assembly, and at
K = 2, 4, 8 in both directions K single calls on K vectors beside the multi call on the same vectors (ms per K vectors;
the table divides by K), with the Kc, wavefronts and LDS the launcher chose.  --singles-only leaves out the new calls:
that part runs on a build without them, which is how the parent build's K single calls are measured in the same job.
Usage: python profiles/jacobian_diag_multi_cost.py [ns3d|ns2d|thermoelastic|cdr ...] [--ncell N] [--singles-only]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrhyde_amd  # noqa: E402,F401
from jacobian_apply_cost import CASES, windows  # noqa: E402
from ns_thermal_cost import block  # noqa: E402

KS = (2, 4, 8)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ncell = None
    if "--ncell" in sys.argv:
        ncell = int(sys.argv[sys.argv.index("--ncell") + 1])
        args.remove(sys.argv[sys.argv.index("--ncell") + 1])
    singles_only = "--singles-only" in sys.argv
    for name in args or list(CASES):
        dim, nc, physics, orders, qdeg, settings = CASES[name]
        blk, m, st = block(dim, ncell or nc, physics, orders, qdeg, settings())
        kw = dict(u_prev=st["u_prev"], u_stage=st["u_stage"])
        n = int(m["ndof"])
        x = torch.rand_like(st["u"]) + 0.5
        y = torch.zeros_like(st["u"])
        r = dict(case=name, lib=mrhyde_amd.lib_path(), elements=m["nelem"], dofs_per_element=int(m["lids"].shape[1]), rows=n)
        for key, tr in (("forward", False), ("transposed", True)):
            r[key] = windows(lambda: blk.apply_jacobian(st["u"], x, y, transpose=tr, overwrite=True, **kw))
        for K in KS:
            X = torch.rand((K, n), dtype=torch.float64, device="cuda") + 0.5
            Y = torch.zeros_like(X)
            for key, tr in (("forward", False), ("transposed", True)):
                def singles():  # K single calls on K vectors: what the multi call replaces
                    for k in range(K):
                        blk.apply_jacobian(st["u"], X[k], Y[k], transpose=tr, overwrite=True, **kw)
                r["singles_%s_K%d" % (key, K)] = windows(singles)
                if not singles_only:
                    w = windows(lambda: blk.apply_jacobian_multi(st["u"], X, Y, transpose=tr, overwrite=True, **kw))
                    w.update(Kc=blk.info("jacobian_apply_vectors"), waves=blk.info("jacobian_apply_waves"),
                             lds_bytes=blk.info("jacobian_apply_lds_bytes"))
                    r["multi_%s_K%d" % (key, K)] = w
        if not singles_only:  # last: the products above see the same history on both builds
            r["diagonal"] = windows(lambda: blk.jacobian_diagonal(st["u"], y, overwrite=True, **kw))
            r["diag_lds_bytes"], r["diag_waves"] = blk.info("jacobian_diag_lds_bytes"), blk.info("jacobian_diag_waves")
            r["assembly"] = windows(lambda: blk.assemble_jacres(st["u"], st["res"], st["vals"], overwrite=True, **kw))
        print(json.dumps(r), flush=True)
        del blk, st
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
