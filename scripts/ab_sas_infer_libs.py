#!/usr/bin/env python3
"""A/B of the SASRec inference paths (csrc/sasrec.hip's plan and driver over sasrec_fused.hip,
sasrec_rowtile.hip, sasrec_tail.hip, attn.hip) between two builds of the library, under the rule and
driver of scripts/ab_chain_libs.py: fresh child per build (GR_AMD_LIB), interleaved repetitions,
outputs bitwise the parent's, median device time within the parent's trimmed spread.

    python scripts/ab_sas_infer_libs.py PARENT/lib/libgr_amd.so lib/libgr_amd.so [repetitions = 10]

A build whose library sits in a whole tree (TREE/<package>/lib/libgr_amd.so beside TREE/gr_amd.py) is
run through that tree's Python package, so a parent whose C ABI lacks an entry point the branch
declares still loads.

Per case one call each of last_hidden, forward, predict and sasrec_rank; the time is of the four
together, the hash covers all four outputs.  Cases: bench.py's C3 shape (d 64, n 50, 2 blocks, 2048
sequences) under sas_fused 1 / 3 / 0; C5 (d 128, n 200, 2 blocks, 512 users) under sas_rowtile x
attn_k16 x emb_proj; the pruned final block (128, 2, 100, 77, 2); the scalar attention kernel
(128, 8, 64, 33, 2); the layer-wise H-form tail (64, 2, 128, 100, 2).

    rocprofv3 --kernel-trace -d OUT -- python scripts/ab_sas_infer_libs.py --once
    python scripts/ab_sas_infer_libs.py --launches OUT/.../*_kernel_trace.csv

--once runs every case once (a float64 torch fill, a kernel nothing else here launches, in front of
each marks the case in the trace); --launches prints, case by case, the ordered names and grid sizes
of the library's kernels in such a trace.
"""
import csv
import hashlib
import json
import os
import sys

DEFAULTS = {"sas_fused": 2, "sas_rowtile": 1, "attn_k16": 1, "emb_proj": 1}
ITEMS = 5000
# (name, (d, heads, mlp, n, blocks), B, options)
CASES = [(f"C3 sas_fused {f}", (64, 1, 64, 50, 2), 2048, {"sas_fused": f}) for f in (1, 3, 0)] + \
        [(f"C5 rowtile {rt} k16 {k} emb_proj {e}", (128, 1, 64, 200, 2), 512,
          {"sas_rowtile": rt, "attn_k16": k, "emb_proj": e}) for rt in (1, 0) for k in (1, 0) for e in (1, 0)] + \
        [("pruned", (128, 2, 100, 77, 2), 512, {}), ("scalar attention", (128, 8, 64, 33, 2), 512, {}),
         ("H-form tail", (64, 2, 128, 100, 2), 512, {})]


def tree_of_build():
    """The tree whose Python package declares the library under test."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.environ.get("GR_AMD_LIB")
    if lib:
        tree = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(lib))))
        if os.path.exists(os.path.join(tree, "gr_amd.py")):
            return tree
    return here


def cases(dev):
    """(name, fn) per case; fn runs the four calls under the case's options and returns their outputs."""
    import torch
    from gr_amd import _lib, ops, synth
    for name, (d, heads, mlp, n, blocks), B, opts in CASES:
        m = synth.sasrec_model(ITEMS, synth.sasrec_params(d, n, blocks, heads, mlp, dev), dev, seed=d + n)
        seqs = synth.sequences(B, n, ITEMS, 7 + n, dev)
        tg = torch.randint(1, ITEMS + 1, (B,), generator=torch.Generator(device=dev).manual_seed(n), device=dev)

        def fn(m=m, seqs=seqs, tg=tg):
            return (m.last_hidden(seqs), m.forward(seqs), m.predict(seqs), ops.sasrec_rank(m._binding(seqs), seqs, tg))

        for k, v in {**DEFAULTS, **opts}.items():
            _lib.set_option(k, v)
        yield name, fn
    for k, v in DEFAULTS.items():
        _lib.set_option(k, v)


def child(out):
    sys.path.insert(0, tree_of_build())
    import torch
    from gr_amd import ops
    dev = torch.device("cuda:0")
    res = {}
    for i, (name, fn) in enumerate(cases(dev)):
        if out is None:   # --once: one call of each, behind the case's marker
            torch.empty(8, dtype=torch.float64, device=dev).fill_(0.0)
            fn()
            continue
        for _ in range(5):
            r = fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        hsh = hashlib.sha256()
        for t in r:
            hsh.update(t.contiguous().cpu().numpy().tobytes())
        res[name] = [e0.elapsed_time(e1) / 20 * 1e3, hsh.hexdigest()]
    torch.cuda.synchronize()
    ops.check_errors(dev)
    if out is not None:
        with open(out, "w") as f:
            json.dump(res, f)


def launches(path):
    """One line per dispatch of a library kernel (gr::) in a rocprofv3 kernel trace, in dispatch order,
    under its case: name (template arguments kept, parameter list dropped), grid and workgroup size."""
    rows = [r for r in csv.DictReader(open(path)) if r.get("Kind", "KERNEL_DISPATCH") == "KERNEL_DISPATCH"]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]) if r.get("Dispatch_Id") else int(r["Start_Timestamp"]))
    case = 0
    for r in rows:
        name = r["Kernel_Name"].replace("(anonymous namespace)", "{anonymous}")
        if "FillFunctor<double>" in name:
            print(f"# {CASES[case][0]}: {CASES[case][1]}, B {CASES[case][2]}; last_hidden, forward, predict, sasrec_rank")
            case += 1
        elif "gr::" in name and case:
            cut = name.find("(")
            print(name[:cut] if cut > 0 else name, "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"),
                  "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ"))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--once"]:
        child(None)
    elif sys.argv[1:2] == ["--launches"]:
        launches(sys.argv[2])
    else:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import ab_chain_libs
        ab_chain_libs.main(child, os.path.abspath(__file__))
