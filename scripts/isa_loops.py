"""Instruction mix of the MFMA loops in a hipcc -S listing: for every basic block that branches back to
its own label and holds v_mfma instructions, the counts of MFMA, other VALU, SALU, VMEM, DS and waits.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -I csrc -I include -S csrc/rq_fused.hip -o rq.s
    python scripts/isa_loops.py rq.s [--kernel rq_encoder] [--dump LABEL | --ranges]
"""
import argparse
import collections
import re

ap = argparse.ArgumentParser()
ap.add_argument("listing")
ap.add_argument("--kernel", default="")
ap.add_argument("--dump", default="", help="print the block with this label")
ap.add_argument("--ranges", action="store_true", help="multi-block loops with one barrier instead")
a = ap.parse_args()


def kind(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_accvgpr"):
        return "acc_mov"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_barrier"):
        return "barrier"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "ds"
    return "other"


kernel, label, body = "", "", []
blocks = []
for line in open(a.listing):
    m = re.match(r"^(\S+):", line)
    if m:
        if label:
            blocks.append((kernel, label, body))
        name = m.group(1)
        if not name.startswith("."):
            kernel = name
        label, body = name, []
        continue
    t = line.strip()
    if not t or t.startswith((".", ";")):
        continue
    body.append(t)
if label:
    blocks.append((kernel, label, body))

def mix(ops):
    c = collections.Counter(kind(o) for o in ops)
    valu = collections.Counter(o for o in ops if kind(o) == "valu")
    return (" ".join(f"{k}={c[k]}" for k in ("mfma", "valu", "acc_mov", "salu", "vmem", "ds", "wait", "barrier")) +
            "   valu: " + ", ".join(f"{k} x{v}" for k, v in sorted(valu.items())))


if a.ranges:
    # loops of several blocks (a branch around the MFMAs inside): label .. backward branch, one barrier
    sel = [b for b in blocks if a.kernel in b[0]]
    index = {b[1]: i for i, b in enumerate(sel)}
    for i, (kernel, label, body) in enumerate(sel):
        for t in body:
            m = re.match(r"s_cbranch\S*\s+(\S+)", t)
            if m and m.group(1) in index and index[m.group(1)] < i:
                ops = [u.split()[0] for b in sel[index[m.group(1)]:i + 1] for u in b[2]]
                if any(o.startswith("v_mfma") for o in ops) and sum(o == "s_barrier" for o in ops) == 1:
                    print(f"{m.group(1):10s} .. {label:10s} {mix(ops)}")
    raise SystemExit

for kernel, label, body in blocks:
    if a.kernel not in kernel:
        continue
    if a.dump:
        if label == a.dump:
            print(f"{label}:")
            for t in body:
                print("\t" + t)
        continue
    ops = [t.split()[0] for t in body]
    if not any(o.startswith("v_mfma") for o in ops):
        continue
    loop = any(o.startswith("s_cbranch") and label in t for o, t in zip(ops, body))
    print(f"{label:12s} {'loop ' if loop else 'block'} {mix(ops)}")
