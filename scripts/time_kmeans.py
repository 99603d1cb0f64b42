"""Time of the codebook k-means init (RQ-VAE/models/layers.py:69-82 behind vq.py:39-47 init_emb) on
the host path (scikit-learn, the default backend) and on the device path (ops.kmeans), same box.

    python scripts/time_kmeans.py [--out FILE] [--skip-host] [--only ROWS]

  (64, 32) K 8, 50 iterations      the reference's shape: one level's init_emb;
  (8192, 32) K 256, (100000, 32) K 256, 50 iterations;
  shapes near each limit of the one-workgroup form (rows x features, clusters, the work bound);
  first forward                    RQVAE(kmeans_init=True).forward on a batch of 64: three levels.

Device times are event times over the enqueued work, median of ``--reps`` calls after ``--warmup``,
in both launch forms where the one-workgroup form takes the shape (option ``kmeans_small``; each line
names the form that ran, from ``gr_kmeans_form``).  Host
times are the host clock around ``VectorQuantizer.init_emb`` with the "host" backend (device-to-host
copy, scikit-learn, copy back) followed by a synchronise, median of ``--host-reps`` calls."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gr_amd import RQVAE, ops  # noqa: E402
from gr_amd import _lib as L  # noqa: E402
from gr_amd.rqvae import VectorQuantizer  # noqa: E402


def event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def model(dev, backend):
    torch.manual_seed(0)
    m = RQVAE(in_dim=768, num_emb_list=[8, 8, 8], e_dim=32, layers=[256, 128], dropout_prob=0.1,
              kmeans_init=True, kmeans_iters=50, sk_epsilons=[0.01] * 3, sk_iters=50).to(dev).train()
    return m.set_kmeans(backend, seed=0 if backend == "device" else None)


def first_forward(m, x):
    for q in m.rq.vq_layers:
        q.initted = False
    with torch.no_grad():
        m(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=0, help="time the shape with this many rows only (for a profiler run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_kmeans: needs a ROCm GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
        f"{torch.get_num_threads()} host threads, warm-up {args.warmup}, median of {args.reps} "
        f"(host: {args.host_reps})")
    g = torch.Generator().manual_seed(0)
    lib = L.lib()
    # the issue's shapes (host path timed too), then shapes near each limit of the one-workgroup form
    shapes = ((64, 32, 8, True), (8192, 32, 256, True), (100000, 32, 256, True),
              (256, 32, 8, True), (256, 5, 7, False), (256, 8, 32, False), (256, 64, 16, False),
              (256, 32, 32, False), (256, 16, 64, False), (128, 32, 64, False), (200, 1, 5, False),
              (600, 32, 8, False), (1000, 5, 7, False))
    iters = 50
    for n, e, K, host in shapes:
        if args.only and n != args.only:
            continue
        x = torch.randn(n, e, generator=g).to(dev)
        say(f"({n}, {e}) K {K}, max_iter {iters}, tol 1e-4")
        res = {}
        for opt in (1, 0):
            L.set_option("kmeans_small", opt)
            form = "one workgroup" if lib.gr_kmeans_form(n, e, K) == 1 else "tiled"   # the form that runs
            if form in res:
                continue
            r = ops.kmeans(x, K, max_iter=iters, seed=0)
            med, lo, hi = event_ms(lambda: ops.kmeans(x, K, max_iter=iters, seed=0), args.warmup, args.reps)
            res[form] = (med, r)
            say(f"  device, {form} form (kmeans_small={opt}): {med:.3f} ms per call (min {lo:.3f}, "
                f"max {hi:.3f}); n_iter {int(r.n_iter)}, inertia {float(r.inertia):.6g}")
        L.set_option("kmeans_small", 1)
        if len(res) == 2:
            same = torch.equal(res["one workgroup"][1].centers, res["tiled"][1].centers)
            say(f"  both forms give the same bits: {same}; tiled / one workgroup "
                f"{res['tiled'][0] / res['one workgroup'][0]:.2f}x")
        else:
            say("  the one-workgroup form does not take this shape")
        if host and not args.skip_host:
            q = VectorQuantizer(K, e, kmeans_init=True, kmeans_iters=iters).to(dev)
            reps = args.host_reps if n <= 8192 else 1
            q.init_emb(x)
            med_h, lo, hi = wall_ms(lambda: q.init_emb(x), reps)
            best = min(v[0] for v in res.values())
            say(f"  host init_emb (scikit-learn, copies included): {med_h:.3f} ms per call (min {lo:.3f}, max {hi:.3f}, "
                f"{reps} calls); host / device {med_h / best:.1f}x")
    if args.only:
        return
    x = torch.randn(64, 768, generator=g).to(dev)
    say("first forward of RQVAE([8, 8, 8], e 32, kmeans_iters 50) on a batch of 64 (three level inits)")
    for opt in (1, 0):
        L.set_option("kmeans_small", opt)
        form = "one workgroup" if lib.gr_kmeans_form(64, 32, 8) == 1 else "tiled"
        m = model(dev, "device")
        med, lo, hi = wall_ms(lambda: first_forward(m, x), args.reps)
        say(f"  device backend, {form} form: {med:.3f} ms host clock per forward (min {lo:.3f}, max {hi:.3f})")
    L.set_option("kmeans_small", 1)
    if not args.skip_host:
        m = model(dev, "host")
        first_forward(m, x)
        med, lo, hi = wall_ms(lambda: first_forward(m, x), args.host_reps)
        say(f"  host backend: {med:.3f} ms host clock per forward (min {lo:.3f}, max {hi:.3f})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
