"""Cost of the matrix-free boundary-group products beside the assembly of the same groups' matrix
(profiles/boundary_apply.md): per kernel instantiation the compiler's resource figures, and per workload the time of
y += A_b x, y += A_b^T x, d += diag(A_b) and assemble_boundary with the Jacobian on the same groups.

  resources             compile kernels/boundary_apply.hip for gfx950 with -Rpass-analysis=kernel-resource-usage (needs no
                        GPU) and print one JSON line: VGPRs, AGPRs, SGPRs, scratch, occupancy, static LDS per instantiation
  time <workload>       one workload on the GPU, one JSON line.  HIP-event time of repeated calls after a warm-up of every
                        call, over windows of more than 150 ms; three windows each
  all <dir> [<json>]    `resources` (or the file a `resources` run wrote), then every workload as a child process under its
                        own `timeout`, stopping at the first one that fails; writes <dir>/boundary_apply.json and
                        <dir>/boundary_apply.md
  report <json>         the markdown of a result file

Workloads: helmholtz 3-D 64^3 Q1 with one Robin face; thermal 3-D 64^3 Q2 with six weak-Dirichlet faces;
linearelasticity 3-D 32^3 Q2 with one Nitsche face."""
import json
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "mrhyde_amd", "csrc")
SIDES = {"bottom": (1, 0, 0), "right": (0, 1, 1), "top": (1, 1, 2), "left": (0, 0, 3), "back": (2, 0, 4), "front": (2, 1, 5)}
WORKLOADS = {"helmholtz": 300, "thermal": 360, "linearelasticity": 360}  # seconds a child may take (mesh and graph included)


def face(nc, name):
    """(element ids, local side ids) of a side of the nc^3 structured mesh (elements numbered x-fastest; shards side ids)"""
    axis, high, side = SIDES[name]
    idx = np.indices((nc, nc, nc))  # [axis][ix][iy][iz]
    eid = idx[0] + nc * (idx[1] + nc * idx[2])
    e = np.sort(eid[idx[axis] == (nc - 1 if high else 0)]).astype(np.int32)
    return e, np.full(len(e), side, dtype=np.int32)


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-ffp-contract=fast",
               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernels", "boundary_apply.hip"), "-o",
               os.path.join(tmp, "k.o")]
        text = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, universal_newlines=True).stderr
    rows = []
    for blockt in re.split(r"(?=remark: [^\n]*Function Name:)", text):
        m = re.search(r"Function Name: (\S+)", blockt)
        if not m:
            continue
        k = re.search(r"boundary_apply_kernelINS_\d+(\w+?)SideFormELi(\d)ELi(\d+)ELi(\d)E", m.group(1))
        if not k:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", blockt).group(1))
        rows.append(dict(form=k.group(1), dim=int(k.group(2)), threads_per_entry=int(k.group(3)), mode=int(k.group(4)),
                         vgprs=get("VGPRs"), agprs=get("AGPRs"), sgprs=get("SGPRs"), scratch=get(r"ScratchSize \[bytes/lane\]"),
                         occupancy=get(r"Occupancy \[waves/SIMD\]"), static_lds=get(r"LDS Size \[bytes/block\]")))
    return rows


def windows(go):
    import torch
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


def time_workload(name):
    import torch
    import mrhyde_amd
    H = mrhyde_amd.BASIS_HGRAD
    if name == "helmholtz":
        nc, qdeg, orders, faces, bc = 64, 2, [1, 1], ["right"], mrhyde_amd.BC_NEUMANN
        funcs = {"c2r_x": 1.3, "c2i_x": 0.35, "c2r_y": 0.9, "c2i_y": -0.45, "c2r_z": 1.1, "c2i_z": 0.25, "robin_alpha_r": 0.55,
                 "robin_alpha_i": -0.65, "source_r_side": 1.9, "source_i_side": 0.75}
    elif name == "thermal":
        nc, qdeg, orders, faces, bc = 64, 4, [2], list(SIDES), mrhyde_amd.BC_WEAK_DIRICHLET
        funcs = {"thermal diffusion": 1.7}
        funcs.update({"Dirichlet e " + f: 0.3 for f in faces})
    else:
        nc, qdeg, orders, faces, bc = 32, 4, [2, 2, 2], ["right"], mrhyde_amd.BC_WEAK_DIRICHLET
        funcs = {"lambda": 1.7, "mu": 0.8}
        funcs.update({"Dirichlet %s right" % v: 0.1 for v in ("dx", "dy", "dz")})
    m = mrhyde_amd.mesh_multi(3, (nc,) * 3, [H] * len(orders), orders)
    blk = mrhyde_amd.Block(3, quadrature=qdeg, physics=name, variables=[(H, o) for o in orders])
    blk.set_mesh(m["nodes"], m["lids"], m["offsets"], m["ndof"])
    blk.set_orientation(m["orient"])
    blk.set_graph()
    for k, v in funcs.items():
        blk.set_function(k, v)
    entries = 0
    for f in faces:
        be, bs = face(nc, f)
        blk.add_boundary_group(f, bc, be, bs)
        entries += len(be)
    nnz = len(blk.get_graph()[1])
    rng = np.random.default_rng(7)
    u = torch.tensor(rng.uniform(-1, 1, m["ndof"]), device="cuda")
    x, y = torch.ones_like(u), torch.zeros_like(u)
    res, vals = torch.zeros_like(u), torch.zeros(nnz, dtype=torch.float64, device="cuda")
    r = dict(workload=name, ncell=nc, orders=orders, faces=faces, entries=entries, dofs_per_element=int(m["lids"].shape[1]),
             rows=int(m["ndof"]), nnz=nnz, num_cu=torch.cuda.get_device_properties(0).multi_processor_count)
    # the calls alternate inside one process: every figure of a workload is from the same visit
    r["assemble_boundary_jacobian"] = windows(lambda: blk.assemble_boundary(u, res, vals))
    r["forward"] = windows(lambda: blk.apply_boundary_jacobian(u, x, y))
    r["transposed"] = windows(lambda: blk.apply_boundary_jacobian(u, x, y, transpose=True))
    r["diagonal"] = windows(lambda: blk.boundary_jacobian_diagonal(u, y))
    r["lds_bytes"] = blk.info("boundary_apply_lds_bytes")
    r["assemble_boundary_jacobian_again"] = windows(lambda: blk.assemble_boundary(u, res, vals))
    return r


def report(result):
    out = ["# Matrix-free boundary-group products: resources and times", "",
           "Written by `profiles/boundary_apply.py all`; one MI355X, %s compute units." % result.get("num_cu", "?"), "",
           "## Kernel resources (`-Rpass-analysis=kernel-resource-usage`, gfx950)", "",
           "`boundary_apply_kernel<form, DIM, threads per entry, mode>`; mode 1 forward, 2 transposed, 3 diagonal.  LDS is",
           "dynamic (per launch: `Block.info(\"boundary_apply_lds_bytes\")`, below per workload), so the static figure is 0.", "",
           "| form | DIM | threads/entry | mode | VGPRs | AGPRs | SGPRs | scratch B/lane | waves/SIMD | static LDS |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for k in result["resources"]:
        out.append("| %(form)s | %(dim)d | %(threads_per_entry)d | %(mode)d | %(vgprs)d | %(agprs)d | %(sgprs)d | %(scratch)d | "
                   "%(occupancy)d | %(static_lds)d |" % k)
    out += ["", "## Times", "",
            "HIP-event time per call in ms, three windows of more than 150 ms each after a warm-up; the assembly is",
            "`assemble_boundary` with the Jacobian (residual + CRS values, accumulating) on the same groups, timed before and",
            "after the products in the same process.", "",
            "| workload | entries | dofs/element | LDS/workgroup | assembly | forward | transposed | diagonal | assembly again |",
            "|---|---|---|---|---|---|---|---|---|"]
    f = lambda w: ", ".join("%.4f" % t for t in w["ms"])
    for w in result["times"]:
        out.append("| %s 3-D %d^3 Q%d, %d face(s) | %d | %d | %d B | %s | %s | %s | %s | %s |" % (
            w["workload"], w["ncell"], w["orders"][0], len(w["faces"]), w["entries"], w["dofs_per_element"], w["lds_bytes"],
            f(w["assemble_boundary_jacobian"]), f(w["forward"]), f(w["transposed"]), f(w["diagonal"]),
            f(w["assemble_boundary_jacobian_again"])))
    if result["times"]:
        out += ["", "Assembly over product (best windows): " + "; ".join(
            "%s %.1f forward, %.1f transposed, %.1f diagonal" % (
                w["workload"], *(min(w["assemble_boundary_jacobian"]["ms"]) / min(w[k]["ms"]) for k in ("forward", "transposed", "diagonal")))
            for w in result["times"]) + ".",
            "A product is one launch per group with a Jacobian and O(n nqs) work and n atomics per entry; the assembly sweeps",
            "the n x n entry matrix with a CRS column search and an atomic per entry.  Where single-launch workloads of very",
            "different size take the same time, that time is a floor per launch rather than the kernel's work; the floor has",
            "not been taken apart here (no kernel trace).  Scratch is 0 in every instantiation; the deck-string interpreter,",
            "inlined at one call site, sets the register count."]
    if result.get("failed"):
        out += ["", "Not measured (the child process failed or ran out of its time): " + ", ".join(result["failed"])]
    return "\n".join(out) + "\n"


def main():
    cmd = sys.argv[1] if len(sys.argv) > 1 else "all"
    if cmd == "resources":
        print(json.dumps(resources()))
    elif cmd == "time":
        print(json.dumps(time_workload(sys.argv[2])))
    elif cmd == "report":
        sys.stdout.write(report(json.load(open(sys.argv[2]))))
    else:
        outdir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
        os.makedirs(outdir, exist_ok=True)
        # the resource figures need the compiler only: a file written by `resources` beforehand is taken as it is
        res = json.load(open(sys.argv[3])) if len(sys.argv) > 3 else resources()
        result = dict(resources=res, times=[], failed=[])
        for name, limit in WORKLOADS.items():
            print("timing", name, "(limit %d s)" % limit, flush=True)
            p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "time", name],
                               stdout=subprocess.PIPE, universal_newlines=True)
            if p.returncode != 0:  # nothing more is started on the GPU after a failure
                result["failed"] = [w for w in WORKLOADS if w not in [t["workload"] for t in result["times"]]]
                break
            result["times"].append(json.loads(p.stdout.strip().splitlines()[-1]))
            result["num_cu"] = result["times"][-1]["num_cu"]
            json.dump(result, open(os.path.join(outdir, "boundary_apply.json"), "w"), indent=1)
        json.dump(result, open(os.path.join(outdir, "boundary_apply.json"), "w"), indent=1)
        open(os.path.join(outdir, "boundary_apply.md"), "w").write(report(result))
        sys.exit(1 if result["failed"] else 0)


if __name__ == "__main__":
    main()
