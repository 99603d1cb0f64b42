"""A/B of the whole SASRec training step at the large shape (d 128, n 200, 2 blocks, 1 head, mlp 64,
B 128, 100k items, 10 negatives, dropout 0.2, Adam as bench.bench_sas_train_step):

    module  ops.SasTrainGraph.replay with SASRec.fused_train = False: the transformer as torch modules
            under autograd (run eagerly, ops._CapturedStep explains why) -- the only path this
            shape had before the tiled kernels
    tiled   ops.SasTrainGraph.replay with the defaults: the tiled training kernels
            (csrc/sasrec_train_tiled.hip), the whole step one captured graph

Both arms live in one process and alternate, ROUNDS rounds of STEPS steps each, every round between
device synchronisations after a warm-up; the spread is (max - min) / median over an arm's rounds.  The
transformer forward + backward alone (model(inputs).backward(upstream), no loss, no optimizer) is
timed the same way on both arms.  Prints one JSON line and writes it to --out.

    python scripts/time_sas_train_tiled.py --out profiles/sas_train_tiled_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from gr_amd import ops, synth  # noqa: E402


def rounds_ms(fn, rounds, steps):
    """Per-step milliseconds of each round: host clock around `steps` calls ending in a synchronise."""
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return out


def summary(ms):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "spread": (max(ms) - min(ms)) / med,
            "rounds_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sas_train_tiled: needs a ROCm GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    B, n, d, items, J, mlp, blocks = a.batch, 200, 128, 100_000, 10, 64, 2
    prm = synth.sasrec_params(d, n, blocks, 1, mlp, dev)
    g = torch.Generator(device=dev).manual_seed(4000)
    lens = torch.randint(3, n + 1, (B,), generator=g, device=dev)
    targets = torch.randint(1, items + 1, (B, n), generator=g, device=dev)
    targets[torch.arange(n, device=dev)[None, :] < (n - lens)[:, None]] = 0
    inputs = torch.roll(targets, 1, dims=1)
    inputs[:, 0] = 0
    upstream = torch.randn(B, n, d, generator=g, device=dev)

    def make(fused):
        m = synth.sasrec_model(items, prm, dev, seed=11).train()   # dropout 0.2 (main.py)
        m.fused_train = fused
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.98), capturable=True, fused=fused or None)
        return m, opt

    arms, models = {}, {}
    for name, fused in (("module", False), ("tiled", True)):
        m, opt = make(fused)
        assert ops.sasrec_train_supported(m, n) and not ops.sasrec_train_fits_sequence(m, n)
        step = ops.SasTrainGraph(m, opt, inputs, targets, items, J, 1e-24, seed=5000)
        assert (step.graph is not None) == fused
        arms[name], models[name] = step.replay, m

    def fwd_bwd(m):
        def run():
            for q in m.parameters():
                q.grad = None
            m(inputs).backward(upstream)
        return run

    tf = {name: fwd_bwd(m) for name, m in models.items()}
    for fn in (*arms.values(), *tf.values()):
        for _ in range(a.warmup):
            fn()
    step_ms = {k: [] for k in arms}
    tf_ms = {k: [] for k in tf}
    for _ in range(a.rounds):   # alternate the arms round by round
        for k in arms:
            step_ms[k] += rounds_ms(arms[k], 1, a.steps)
        for k in tf:
            tf_ms[k] += rounds_ms(tf[k], 1, a.steps)
    torch.cuda.synchronize()
    ops.check_errors(dev)
    res = {"workload": f"SASRec whole training step, B {B}, n {n}, d {d}, {blocks} blocks, 1 head, mlp {mlp}, "
                       f"{items} items, {J} negatives, dropout 0.2, Adam",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps_per_round": a.steps,
           "step": {k: summary(v) for k, v in step_ms.items()},
           "transformer_fwd_bwd": {k: summary(v) for k, v in tf_ms.items()}}
    for part in ("step", "transformer_fwd_bwd"):
        r = res[part]
        r["ratio_module_over_tiled"] = r["module"]["median_ms"] / r["tiled"]["median_ms"]
        r["combined_spread"] = r["module"]["spread"] + r["tiled"]["spread"]
        r["tiled_faster_beyond_spread"] = bool(r["ratio_module_over_tiled"] - 1.0 > r["combined_spread"])
    fl = bench.sas_step_flop_per_user(d, n, mlp, blocks, J) * B
    res["step"]["tiled"]["frac_of_fp32_peak"] = (fl / (res["step"]["tiled"]["median_ms"] * 1e-3) / 1e12
                                                 / bench.FP32_PEAK_TFLOPS)
    res["flop_per_step"] = fl
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
