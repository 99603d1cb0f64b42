"""Time of the semantic-ID emission tail (collision groups + dedup digit; RQ-VAE/infer.py:29-41 and
:139-162) on the host functions and on the device path, on the same box.

    python scripts/time_code_emission.py [--out FILE] [--skip-host]

  N = 100,000 (K 64, L 3)   infer.collision_groups and infer.dedup_codes on the CPU (one call each,
                            host clock) against ops.code_groups on the GPU, outputs compared;
  N = 10,000,000 (K 256, L 3)  the device path alone.

Device times are event times over the enqueued work (hash build, lookup, torch.sort of the keys,
segment pass), median of ``--reps`` calls after ``--warmup``; "with host read" adds the one read of
the stats and group sizes that a collision round needs, on the host clock around a synchronise."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gr_amd import infer, ops  # noqa: E402


def device_times(codes_t, warmup, reps, listing=True):
    for _ in range(warmup):
        ops.code_groups(codes_t, listing=listing)
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        g = ops.code_groups(codes_t, listing=listing)
        b.record()
        g.host()
        wall.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    return g, statistics.median(ev), min(ev), max(ev), statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_code_emission: needs a ROCm GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
        f"warm-up {args.warmup}, median of {args.reps}")
    for n, K, L, host in ((100_000, 64, 3, not args.skip_host), (10_000_000, 256, 3, False)):
        codes = np.random.default_rng(n + K).integers(0, K, size=(n, L)).astype(np.int64)
        t = torch.from_numpy(codes).to(dev)
        say(f"N {n:,} K {K} L {L}")
        g, med, lo, hi, wall = device_times(t, args.warmup, args.reps)
        (distinct, max_count, m, groups), sizes = g.host()
        say(f"  codes: {distinct:,} distinct, {groups:,} groups over {m:,} rows, largest {max_count}")
        say(f"  device ops.code_groups (groups + digit): {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); "
            f"with host read of stats and sizes {wall:.3f} ms")
        _, med_h, lo, hi, wall = device_times(t, args.warmup, args.reps, listing=False)
        say(f"  device hash build + lookup only (collision rate): {med_h:.3f} ms (min {lo:.3f}, max {hi:.3f}); "
            f"with host read {wall:.3f} ms")
        if host:
            t0 = time.perf_counter()
            hg = infer.collision_groups(codes)
            t_groups = time.perf_counter() - t0
            say(f"  host infer.collision_groups: {t_groups:.3f} s per call")
            t0 = time.perf_counter()
            hd = infer.dedup_codes(codes)
            t_dedup = time.perf_counter() - t0
            say(f"  host infer.dedup_codes: {t_dedup:.3f} s")
            same = (np.array_equal(g.rows.cpu().numpy(), np.concatenate(hg))
                    and np.array_equal(sizes, [len(x) for x in hg])
                    and np.array_equal(g.digit.cpu().numpy(), hd[:, -1]))
            say(f"  device outputs equal the host functions': {same}")
            say(f"  host / device: {(t_groups + t_dedup) * 1e3 / med:,.0f}x (device time without the read)")
            if not same:
                raise SystemExit("time_code_emission: device and host outputs differ")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
