"""Cost of the porousWeakGalerkin element step (profiles/porous_weak_galerkin.md); follows profiles/porous_hybrid.py.

  resources        compile the two kernels for gfx950 with -Rpass-analysis=kernel-resource-usage (needs no GPU) and print
                   one JSON line: VGPRs, AGPRs, SGPRs, scratch, spills, occupancy, static LDS per instantiation
  time <2d|3d>     one size on the GPU, one JSON line: 2-D 1024^2 quads or 3-D 128^3 hexes, constant perm and source.
                   HIP-event time of repeated calls after a warm-up of each, three windows of more than 150 ms each:
                     fused    mha_pwg_condensed_element (schur, gvec, du)
                     generic  mha_pwg_element_blocks followed by mha_batched_condense on the same block
                     copy     a device-to-device copy that moves the fused step's algorithmic bytes -- nodes, u, lambda in;
                              schur, gvec, du out -- as half of them read and half written, in the same process
                     pmh      mha_pmh_condensed_element of a porousMixedHybridized block on the same mesh
                   `share` is copy time over fused time: the fused step's share of the copy rate.
  once <2d|3d>     the same block, the fused step three times and nothing else: the program of a counter run
  all <dir>        resources, then both sizes as child processes under their own `timeout`, stopping at the first that
                   fails; writes <dir>/porous_weak_galerkin.json"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrhyde_amd", "csrc")
SIZES = {"2d": (1024, 1024), "3d": (128, 128, 128)}

from porous_hybrid import windows  # noqa: E402  (the same measuring loop)


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("porous_wg_fused", "porous_wg_blocks"):
            cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-ffp-contract=fast",
                   "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernels", name + ".hip"), "-o",
                   os.path.join(tmp, "k.o")]
            text = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, universal_newlines=True).stderr
            for part in re.split(r"(?=remark: [^\n]*Function Name:)", text):
                m = re.search(r"Function Name: \S*(porous_wg_\w+?_kernel)ILi(\d)ELb(\d)E", part)
                if not m:
                    continue
                get = lambda key: int(re.search(key + r": (\d+)", part).group(1))
                rows.append(dict(kernel=m.group(1), dim=int(m.group(2)), deck_strings=int(m.group(3)), vgprs=get("VGPRs"),
                                 agprs=get("AGPRs"), sgprs=get("SGPRs"), scratch=get(r"ScratchSize \[bytes/lane\]"),
                                 vgpr_spill=get("VGPRs Spill"), occupancy=get(r"Occupancy \[waves/SIMD\]"),
                                 static_lds=get(r"LDS Size \[bytes/block\]")))
    return rows


def time_size(which, once=False):
    import torch
    import mrhyde_amd
    assert torch.cuda.is_available(), "the measurement needs a GPU; there is no fallback"
    ncell = SIZES[which]
    dim = len(ncell)
    HVOL, HDIV = mrhyde_amd.BASIS_HVOL, mrhyde_amd.BASIS_HDIV
    mesh = mrhyde_amd.mesh_porous_weak_galerkin(ncell)
    E, NI, NU = mesh["nelem"], 1 + 4 * dim, 2 * dim
    blk = mrhyde_amd.Block(dim, quadrature=2, physics="porousWeakGalerkin", variables=[(HVOL, 0), (HDIV, 1), (HDIV, 1)])
    blk.set_mesh(mesh["nodes"], mesh["lids"], mesh["offsets"], mesh["ndof"])
    blk.set_orientation(mesh["orient"])
    blk.set_function("perm", 1.5)
    blk.set_function("source", 0.7)
    rng = np.random.default_rng(0)
    f64 = dict(dtype=torch.float64, device="cuda")
    u = torch.tensor(rng.uniform(-1, 1, mesh["ndof"]), **f64)
    lam = torch.tensor(rng.uniform(-1, 1, mesh["ntrace"])[mesh["trace_lids"]], **f64)
    schur, gvec, du = torch.zeros((E, NU, NU), **f64), torch.zeros((E, NU), **f64), torch.zeros((E, NI), **f64)
    ns = torch.zeros(1, dtype=torch.int32, device="cuda")
    if once:
        for _ in range(3):
            blk.pwg_condensed_element(u, lam, schur=schur, gvec=gvec, du=du, num_singular=ns)
        torch.cuda.synchronize()
        blk.close()
        return dict(size=which, elements=E, singular=int(ns[0]))
    n = NI + NU
    res, blocks = torch.zeros((E, n), **f64), torch.zeros((E, n, n), **f64)
    lib = mrhyde_amd.load_library()
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())
    s2, g2, d2 = torch.zeros_like(schur), torch.zeros_like(gvec), torch.zeros_like(du)
    nsh = C.c_int()

    def fused():
        blk.pwg_condensed_element(u, lam, schur=schur, gvec=gvec, du=du, num_singular=ns)

    def generic():
        blk.pwg_element_blocks(u, lam, res, blocks)
        rc = lib.mha_batched_condense(NI, NU, E, p(blocks), p(res), p(s2), p(g2), p(d2), C.byref(nsh), None)
        assert rc == 0

    bytes_in = 8 * (E * 2 ** dim * dim + E * NI + E * NU)
    bytes_out = 8 * (E * NU * NU + E * NU + E * NI)
    half = (bytes_in + bytes_out) // 16
    src, dst = torch.zeros(half, **f64), torch.zeros(half, **f64)

    def copy():
        dst.copy_(src)

    # porousMixedHybridized on the same mesh, beside it
    hm = mrhyde_amd.mesh_porous_hybrid(ncell)
    hyb = mrhyde_amd.Block(dim, quadrature=2, physics="porousMixedHybridized", variables=[(HVOL, 0), (HDIV, 1)])
    hyb.set_mesh(hm["nodes"], hm["lids"], hm["offsets"], hm["ndof"])
    hyb.set_orientation(hm["orient"])
    for d in "xyz":
        hyb.set_function("Kinv_" + d * 2, 1 / 1.5)
    hyb.set_function("source", 0.7)
    hu = torch.tensor(rng.uniform(-1, 1, hm["ndof"]), **f64)
    hs, hg, hd = torch.zeros((E, NU, NU), **f64), torch.zeros((E, NU), **f64), torch.zeros((E, 1 + NU), **f64)

    def pmh():
        hyb.pmh_condensed_element(hu, lam, schur=hs, gvec=hg, du=hd, num_singular=ns)

    out = dict(size=which, ncell=list(ncell), elements=E, bytes_in=bytes_in, bytes_out=bytes_out)
    for name, call in (("fused", fused), ("generic", generic), ("copy", copy), ("pmh", pmh), ("fused_again", fused)):
        out[name + "_ms"] = windows(torch, call)
    torch.cuda.synchronize()
    assert int(ns[0]) == 0 and nsh.value == 0
    scale = float(schur.abs().max())
    out["fused_vs_generic_max_rel"] = float((schur - s2).abs().max()) / scale
    out["schur_vs_pmh_max_rel"] = float((schur - hs).abs().max()) / scale
    best = min(out["fused_ms"] + out["fused_again_ms"])
    out["share"] = min(out["copy_ms"]) / best
    out["fused_GBps"] = (bytes_in + bytes_out) / (best * 1e-3) / 1e9
    out["copy_GBps"] = (bytes_in + bytes_out) / (min(out["copy_ms"]) * 1e-3) / 1e9
    out["generic_over_fused"] = min(out["generic_ms"]) / best
    out["fused_over_pmh"] = best / min(out["pmh_ms"])
    blk.close()
    hyb.close()
    return out


def main(argv):
    if argv[:1] == ["resources"]:
        print(json.dumps(resources()))
    elif argv[:1] == ["time"] and len(argv) == 2 and argv[1] in SIZES:
        print(json.dumps(time_size(argv[1])))
    elif argv[:1] == ["once"] and len(argv) == 2 and argv[1] in SIZES:
        print(json.dumps(time_size(argv[1], once=True)))
    elif argv[:1] == ["all"] and len(argv) == 2:
        os.makedirs(argv[1], exist_ok=True)
        result = dict(resources=resources(), times=[])
        for which in SIZES:
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "time", which],
                               stdout=subprocess.PIPE, universal_newlines=True)
            if r.returncode != 0:
                print("time %s ended with status %d: stopping" % (which, r.returncode))
                break
            result["times"].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(result["times"][-1]), flush=True)
        with open(os.path.join(argv[1], "porous_weak_galerkin.json"), "w") as f:
            json.dump(result, f, indent=1)
        return 0 if len(result["times"]) == len(SIZES) else 1
    else:
        print(__doc__)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
