"""Device time of RQVAE.get_indices (graph-captured, 20 calls per replay) with the library named by
$GR_AMD_LIB (default: the built one) -- one process per library, so ablation builds of the encoder
(scripts/build_variant.sh ... -DGR_EDIAG=1/2/3, wrong results, timing only) and builds of other
trees can be timed on the same inputs.

    GR_AMD_LIB=lib/libgr_amd_e1.so python scripts/ab_rq_getidx.py [--n 100000,409600] [--reps 3]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gr_amd import _lib as L, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="100000,409600")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
dev = torch.device("cuda:0")


def graph_us(fn, calls=20, reps=10):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    for _ in range(30):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * calls) * 1e3


rq = synth.rqvae_model(3, 256, dev)
name = os.path.basename(L.LIB_PATH)
for n in [int(v) for v in a.n.split(",")]:
    x = synth.items(n, 1000, dev)
    rq.get_indices(x)
    torch.cuda.synchronize()
    us = [graph_us(lambda: rq.get_indices(x)) for _ in range(a.reps)]
    print(f"{name:22s} n={n:7d}: " + " ".join(f"{u:8.2f}" for u in us) + f" us/call (min {min(us):8.2f})", flush=True)
