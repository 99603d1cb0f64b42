"""Run scripts/micro/mfma_rate.hip (built into scripts/micro/libmfma_rate.so by
``hipcc -O3 -shared -fPIC --offload-arch=gfx950``): sustained fp32 MFMA TFLOP/s on the whole chip
and the effective shader clock, per (waves per workgroup, chains per wave): register operands, the A
operand from LDS read just in time and one 4-MFMA step ahead, and the two LDS forms again with a
workgroup barrier every 32 MFMAs per chain (profiles/r08/mfma_rate_prefetch.txt)."""
import ctypes
import os

import torch

lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmfma_rate.so"))
lib.run_mfma_rate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                              ctypes.c_int, ctypes.c_void_p]
lib.run_mfma_rate_lds.argtypes = lib.run_mfma_rate.argtypes
lib.run_mfma_rate_lds_ahead.argtypes = lib.run_mfma_rate.argtypes
lib.run_mfma_rate_lds_sync.argtypes = lib.run_mfma_rate.argtypes + [ctypes.c_int]
cus = torch.cuda.get_device_properties(0).multi_processor_count
out = torch.zeros(1024, device="cuda")
clk = torch.zeros(2 * cus, dtype=torch.int64, device="cuda")
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
iters = 20000
# "LDS ahead": every ds_read_b128 issued one 4-MFMA step before its use (double-buffered fragments)
# "+ barrier": a workgroup barrier every 32 MFMAs per chain, as the kernels' chunk loops have -- it
# keeps the waves of a SIMD in step (the cycles column is wave 0's: below 64 x its share where the
# older wave outran the other, which then finishes alone) and puts every wave's exposed read behind it
for fn, tag in ((lib.run_mfma_rate, "registers"), (lib.run_mfma_rate_lds, "A from LDS"),
                (lib.run_mfma_rate_lds_ahead, "LDS ahead"),
                (lambda *a: lib.run_mfma_rate_lds_sync(*a, 0), "A from LDS + barrier"),
                (lambda *a: lib.run_mfma_rate_lds_sync(*a, 1), "LDS ahead + barrier")):
  for waves, chains in [(w, c) for w in (4, 8, 16) for c in (1, 2, 4)]:
    for _ in range(3):
        fn(out.data_ptr(), clk.data_ptr(), cus, waves, chains, iters, st)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(out.data_ptr(), clk.data_ptr(), cus, waves, chains, iters, st)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    flop = cus * waves * chains * iters * 32 * 32 * 2 * 2
    c = clk.view(-1, 2).double()
    ghz = (c[:, 0] / c[:, 1] * 0.1).mean().item()   # s_memrealtime ticks at 100 MHz
    cyc = (c[:, 0].mean().item()) / (iters * chains * waves / 4)
    print(f"{tag:20s} waves/WG {waves:2d} chains/wave {chains}: {flop / ms / 1e9:7.1f} TFLOP/s  "
          f"({flop / ms / 1e9 / 157.3:5.3f} of 157.3)  shader clock {ghz:5.3f} GHz  "
          f"{cyc:6.1f} cycles per MFMA per SIMD", flush=True)
