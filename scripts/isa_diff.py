"""Per-kernel comparison of two hipcc -S device listings of the same translation unit: the instruction
sequence (mnemonics and operands; comments dropped, local labels renumbered in order of appearance)
and the .amdhsa_ resource lines (VGPRs, AGPRs, SGPRs, LDS, scratch, ...).  Prints, per kernel symbol,
"identical" or the number of differing lines; exit status 1 when any kernel differs or is missing.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -I csrc -I include -S csrc/score.hip -o new/score.s
    python scripts/isa_diff.py old/score.s new/score.s [--show KERNEL_SUBSTRING]
"""
import argparse
import difflib
import re
import sys


def kernels(path):
    """{symbol: normalised lines} for every .amdhsa_kernel of the listing."""
    text, meta = {}, {}
    sym, body, in_meta = None, [], None
    for raw in open(path):
        line = raw.split(";", 1)[0].rstrip()
        t = line.strip()
        if not t:
            continue
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            sym, body = m.group(1), []
            text[sym] = body
            continue
        if t.startswith(".amdhsa_kernel"):
            in_meta = t.split()[1]
            meta[in_meta] = []
            continue
        if t.startswith(".end_amdhsa_kernel"):
            in_meta = None
            continue
        if in_meta is not None:
            meta[in_meta].append(" ".join(t.split()))
            continue
        if sym is None or (t.startswith(".") and not t.startswith(".L")):   # directives
            continue
        body.append(" ".join(t.split()))
    out = {}
    for k, res in meta.items():
        labels = {}

        def renum(mm):
            return labels.setdefault(mm.group(0), "L%d" % len(labels))

        out[k] = [re.sub(r"\.L\w+", renum, s) for s in text.get(k, [])] + res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--show", default="", help="print the diff of kernels whose symbol contains this")
    ap.add_argument("--map", default="", help="OLD=NEW: substring of old symbols renamed in new (a moved type)")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    if a.map:
        o, n = a.map.split("=")
        old = {k.replace(o, n): v for k, v in old.items()}
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print("%s: only in %s" % (k, "old" if k in old else "new"))
            bad += 1
            continue
        d = [x for x in difflib.unified_diff(old[k], new[k], lineterm="", n=0)
             if x[:1] in "+-" and not x.startswith(("+++", "---"))]
        print("%s: %s" % (k, "identical (%d lines)" % len(new[k]) if not d else "%d differing lines" % len(d)))
        if d:
            bad += 1
            if a.show and a.show in k:
                print("\n".join("    " + x for x in d))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
