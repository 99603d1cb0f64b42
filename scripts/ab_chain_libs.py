#!/usr/bin/env python3
"""A/B of every kernel built on csrc/score_chain.h between two builds of the library (the parent
commit's and the branch's): outputs compared bitwise, device time compared against the parent's own
spread.  Each build runs in a fresh child process (GR_AMD_LIB), repetitions interleaved
parent / branch / parent / ...; a child writes {case: [microseconds, sha256 of its outputs]}.

    python scripts/ab_chain_libs.py lib/libgr_amd_parent.so lib/libgr_amd.so [repetitions = 10]

Cases (one per kernel instantiation the launchers can reach):
  score_direct  d x {128, 512 users: one / two user tiles per wave} x {padded rows: streaming stores,
                contiguous rows: cached stores};  score_rot d 16..64 / score_ring d 128: 2048 users,
                contiguous rows above the cached-store limit
  pairs, count  d x {thresholds given, thresholds = pairs inside the count kernel (sasrec_rank; the
                time includes the model's forward, the same machine code in both builds)}
  topk          d x k {4, 10, 16} x tile maxima {32-row, 16-row}
The score_direct and count (thresholds given) cases run machine code identical to the parent's and
serve as controls of the criterion itself.

A case passes when its outputs are bitwise the parent's in every repetition and
median(branch) <= median(parent) + trimmed spread(parent), the trimmed spread being the parent's
range with its highest and lowest repetition left out.  Medians and a trimmed range do not move with
one slow repetition, and the margin does not widen as repetitions are added (a max - min would).
"""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

DS = (16, 32, 64, 128)


def child(out):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gr_amd import _lib, ops, synth
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    res = {}

    def run(name, fn):
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
        for t in (r if isinstance(r, tuple) else (r,)):
            hsh.update(t.contiguous().cpu().numpy().tobytes())
        res[name] = [e0.elapsed_time(e1) / 20 * 1e3, hsh.hexdigest()]

    rows = 20001
    for d in DS:
        table = torch.randn(rows, d, generator=g, device=dev)
        for B in (128, 512, 2048):
            h = torch.randn(B, d, generator=g, device=dev)
            for ld in ((20032, rows) if B < 2048 else (rows,)):
                buf = torch.empty(B, ld, device=dev)
                kind = "direct" if B < 2048 else ("ring" if d == 128 else "rot")
                run(f"score_{kind} d{d} B{B} ld{ld}", lambda: ops.score(h, table, out=buf[:, :rows]))
        big = torch.randn(100001, d, generator=g, device=dev)
        h = torch.randn(4096, d, generator=g, device=dev)
        ids = torch.randint(0, 100001, (4096,), generator=g, device=dev)
        run(f"pairs d{d}", lambda: ops.score_pairs(h, big, ids))
        thr = torch.randn(512, generator=g, device=dev)
        run(f"count d{d}", lambda: ops.score_count_gt(h[:512], big, thr))
        m = synth.sasrec_model(20000, synth.sasrec_params(d, 20, 2, 1, 64, dev), dev, seed=d)
        seqs = synth.sequences(256, 20, 20000, 7, dev)
        tg = torch.randint(0, 20001, (256,), generator=g, device=dev)
        run(f"count_pairs d{d}", lambda: ops.sasrec_rank(m._binding(seqs), seqs, tg))
        for k in (4, 10, 16):
            for half in (0, 1):
                _lib.set_option("topk_half", half)
                run(f"topk d{d} k{k} half{half}", lambda: ops.score_topk(h[:256], big[:50001], k, thresholds=thr[:256]))
        _lib.set_option("topk_half", 2)
    ops.check_errors(dev)
    with open(out, "w") as f:
        json.dump(res, f)


def main(child=child, script=__file__):
    """``child`` / ``script``: another case set under the same rule (scripts/ab_train_libs.py)."""
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    libs = [os.path.abspath(p) for p in sys.argv[1:3]]
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    if reps < 5:
        sys.exit("at least five repetitions: the trimmed spread leaves out the highest and the lowest")
    tmp = tempfile.mkdtemp(prefix="ab_chain_")
    runs = ([], [])
    for rep in range(reps):
        for i, lib in enumerate(libs):
            out = os.path.join(tmp, f"{i}_{rep}.json")
            # a failed or hung child ends the whole run: nothing more is started on the GPU
            subprocess.run(["timeout", "-k", "10", "240", sys.executable, script, "--child", out],
                           env=dict(os.environ, GR_AMD_LIB=lib), check=True)
            runs[i].append(json.load(open(out)))
    bad = 0
    print(f"parent {os.path.basename(libs[0])}\nbranch {os.path.basename(libs[1])}\n{reps} interleaved repetitions, microseconds per call")
    for case in runs[0][0]:
        p = [r[case][0] for r in runs[0]]
        b = [r[case][0] for r in runs[1]]
        same = len({r[case][1] for r in runs[0] + runs[1]}) == 1
        ps = sorted(p)
        spread = ps[-2] - ps[1]
        mp, mb = statistics.median(p), statistics.median(b)
        ok = same and mb <= mp + spread
        bad += not ok
        print(f"{case:28s} bitwise equal: {same}  parent {' '.join(f'{x:8.1f}' for x in p)}  "
              f"branch {' '.join(f'{x:8.1f}' for x in b)}  medians {mp:7.2f} {mb:7.2f}  margin {spread:5.2f}  "
              f"{'ok' if ok else 'OUTSIDE'}", flush=True)
    print("ALL WITHIN THE PARENT'S SPREAD, ALL BITWISE EQUAL" if not bad else f"{bad} CASES OUTSIDE")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
