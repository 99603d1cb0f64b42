"""Device-time A/B of gr_rq_quantize_f32 alone across builds of libgr_amd.so (the filtered
quantizer's ablation builds, scripts/build_variant.sh rq.hip -DGR_FDIAG=...), graph-captured and
replayed as scripts/ab_lib.py does, the libraries interleaved within every reading.

    python scripts/ab_rq_filter.py lib/libgr_amd_parent.so lib/libgr_amd.so [--n 100000] [--L 3 --K 256]
        [--readings 3] [--counts lib/libgr_amd_f_d3.so]

--counts: a -DGR_FDIAG=3 build; prints the number of codes re-scored per item and level.
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gr_amd import _lib as L, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="*")
ap.add_argument("--n", type=int, default=100_000)
ap.add_argument("--L", type=int, default=3)
ap.add_argument("--K", type=int, default=256)
ap.add_argument("--readings", type=int, default=3)
ap.add_argument("--counts", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
vp = ctypes.c_void_p


def cur():
    return vp(torch.cuda.current_stream().cuda_stream)


def graph_of(fn, calls=20):
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
    return g


def time_us(g, calls=20, reps=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * calls) * 1e3


m = synth.rqvae_model(a.L, a.K, dev)
b = m.encode_binding()
z = m.encoder(synth.items(a.n, 1000, dev)).contiguous()
ca, ks = L.ptr_array(b.cbs), L.i32_array(b.Ks)
e, nl = b.dims[-1], len(b.cbs)


def quant_fn(lib, idx):
    return lambda: lib.gr_rq_quantize_f32(vp(z.data_ptr()), ctypes.c_int64(a.n), e, nl, ks, ca, None,
                                          vp(idx.data_ptr()), None, None, cur())


graphs, ref = [], None
for path in a.libs:
    lib = ctypes.CDLL(os.path.abspath(path))
    idx = torch.empty((a.n, nl), dtype=torch.int64, device=dev)
    fn = quant_fn(lib, idx)
    assert fn() == 0
    torch.cuda.synchronize()
    differ = 0 if ref is None else int((idx != ref).any(1).sum())
    ref = idx.clone() if ref is None else ref
    graphs.append((os.path.basename(path), graph_of(fn), differ, idx))
times = {name: [] for name, *_ in graphs}
for _ in range(a.readings):
    for name, g, _, _ in graphs:
        times[name].append(time_us(g))
for name, _, differ, _ in graphs:
    print(f"{name:28s} n={a.n} L={a.L} K={a.K}: quantize " + " ".join(f"{t:8.2f}" for t in times[name]) +
          f" us  rows differing from the first library: {differ}", flush=True)

if a.counts:
    lib = ctypes.CDLL(os.path.abspath(a.counts))
    cnt = torch.zeros((a.n, nl), dtype=torch.int32, device=dev)
    idx = torch.empty((a.n, nl), dtype=torch.int64, device=dev)
    lib.gr_rq_filter_diag_counts(vp(cnt.data_ptr()))
    assert quant_fn(lib, idx)() == 0
    torch.cuda.synchronize()
    lib.gr_rq_filter_diag_counts(None)
    tiles = torch.nn.functional.pad(cnt, (0, 0, 0, -a.n % 32)).reshape(-1, 32, nl)
    for l in range(nl):
        c = cnt[:, l].float()
        hist = torch.bincount(cnt[:, l].clamp(max=8), minlength=9).tolist()
        print(f"re-scored codes, level {l}: mean {float(c.mean()):.4f} max {int(c.max())}  items with 0..8+: {hist}  "
              f"largest per 32-item tile: mean {float(tiles[:, :, l].max(1).values.float().mean()):.3f}", flush=True)
