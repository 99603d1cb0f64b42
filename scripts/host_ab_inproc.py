#!/usr/bin/env python3
"""Host time of gr_sasrec_forward_f32 (last position) and gr_sasrec_rank_f32 of two builds of the library
loaded into ONE process, at scripts/host_cost.py's shape (d 16, n 20, 2 blocks, 128 users): every argument
prebuilt, blocks of 2000 unsynchronised calls alternating between the builds, median microseconds per block.
Separate processes (host_cost.py run once per build) differ by more than a few tenths of a microsecond even
between two copies of one build; within a process the two libraries see the same interpreter, allocator and
HIP runtime state.

    python scripts/host_ab_inproc.py PARENT/lib/libgr_amd.so lib/libgr_amd.so
"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gr_amd import _lib as L, ops, synth
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
libs = {"parent": ctypes.CDLL(os.path.abspath(sys.argv[1])), "branch": ctypes.CDLL(os.path.abspath(sys.argv[2]))}
items, n, d = 706, 20, 16
sm = synth.sasrec_model(items, synth.sasrec_params(d, n, 2, 1, 64, dev), dev, seed=16)
seqs = synth.sequences(128, n, items, 9000, dev)
tg = torch.randint(1, items + 1, (128,), device=dev)
b = ops.sasrec_binding(sm)
out = torch.empty(128, d, device=dev)
ranks = torch.empty(128, dtype=torch.int64, device=dev)
nb, cnb = b.rank_workspace_bytes(128, n)
ws = torch.empty(nb, dtype=torch.uint8, device=dev)
cws = torch.zeros(max(cnb, 1), dtype=torch.uint8, device=dev)
st = L.stream_of(dev)
fns = {}
for w, lib in libs.items():
    f = lib.gr_sasrec_forward_f32
    f.restype, f.argtypes = L.SIGNATURES["gr_sasrec_forward_f32"]
    r = lib.gr_sasrec_rank_f32
    r.restype, r.argtypes = L.SIGNATURES["gr_sasrec_rank_f32"]
    fa = (b.p_ref, seqs.data_ptr(), 128, n, out.data_ptr(), 1, ws.data_ptr(), nb, None, st)
    ra = (b.p_ref, seqs.data_ptr(), 128, n, tg.data_ptr(), 1, ranks.data_ptr(), ws.data_ptr(), nb, cws.data_ptr(), cnb, None, st)
    fns[w] = (lambda f=f, fa=fa: f(*fa), lambda r=r, ra=ra: r(*ra))
    assert fns[w][0]() == 0 and fns[w][1]() == 0
torch.cuda.synchronize()


def block(fn, reps=2000):
    ts = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        if i % 64 == 63:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return float(np.median(ts)) * 1e6


for k, what in enumerate(("forward_last", "rank")):
    res = {"parent": [], "branch": []}
    for rep in range(10):
        for w in (("parent", "branch") if rep % 2 == 0 else ("branch", "parent")):
            res[w].append(block(fns[w][k]))
    for w in res:
        print(what, w, " ".join(f"{x:.2f}" for x in res[w]), "median %.3f" % np.median(res[w]), flush=True)
