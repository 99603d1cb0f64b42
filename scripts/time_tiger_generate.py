"""Time of one TIGER.generate call at the reference's inference shape (RQVAE-T5/main.py: 256 users,
20 beams, 80 history tokens, 2 + 2 layers, d_model 64) on the gfx950 kernels, next to the reference
formulation (transformers' T5ForConditionalGeneration.generate under torch-ROCm on the same GPU)
when ``transformers`` is importable, else next to that formulation on the host CPU, labelled so.

    python scripts/time_tiger_generate.py [--out profiles/r15/tiger_generate.txt]

Device time per call from events around ``--reps`` back-to-back calls, host time per call from
perf_counter without synchronisation, launches per call from the design (checked against a
torch.profiler kernel count when it is available).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gr_amd  # noqa: E402

CFG = dict(vocab_size=64, num_layers=2, num_decoder_layers=2, d_model=64, d_ff=256, num_heads=4, d_kv=16,
           dropout_rate=0.1, feed_forward_proj="relu", pad_token_id=0, eos_token_id=31)


def inputs(B, items, dev):
    rng = np.random.default_rng(0)
    S = 4 * items
    ids = np.zeros((B, S), np.int64)
    for b in range(B):
        n = int(rng.integers(1, items + 1))
        ids[b, S - 4 * n:] = (rng.integers(0, 8, size=(n, 4)) + np.arange(4) * 8 + 1).reshape(-1)
    ids = torch.from_numpy(ids).to(dev)
    return ids, (ids != 0).to(torch.int64)


def timed(fn, reps, warmup, sync, on_gpu=True):
    for _ in range(warmup):
        fn()
    sync()
    host = []
    if on_gpu:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    t_all = time.perf_counter()
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        host.append(time.perf_counter() - t0)
    if on_gpu:
        e1.record()
    sync()
    wall = (time.perf_counter() - t_all) / reps * 1e3
    dev_ms = e0.elapsed_time(e1) / reps if on_gpu else None
    return dict(device_ms_per_call=dev_ms, host_ms_per_call=float(np.median(host)) * 1e3, wall_ms_per_call=wall)


def count_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type.name == "CUDA" and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception:       # the profiler is optional
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--beams", type=int, default=20)
    ap.add_argument("--items", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = gr_amd.TIGER(CFG).to(dev).eval()
    ids, mask = inputs(a.batch, a.items, dev)
    run = lambda: model.generate(ids, mask, num_beams=a.beams)
    res = {"shape": dict(B=a.batch, beams=a.beams, tokens=4 * a.items, max_length=5),
           "device": torch.cuda.get_device_name(0)}
    res["gr_amd"] = dict(timed(run, a.reps, 5, torch.cuda.synchronize), launches=2, profiled_kernels=count_kernels(run))
    try:
        import transformers
    except ImportError:
        transformers = None
    if transformers is not None:
        t5 = transformers.T5ForConditionalGeneration(transformers.T5Config(
            decoder_start_token_id=CFG["pad_token_id"], **CFG)).eval()
        t5.load_state_dict({k[len("model."):]: v for k, v in model.state_dict().items()})
        for where in ("cuda", "cpu"):
            try:
                m = t5.to(where)
                i2, m2 = ids.to(where), mask.to(where)
                ref = lambda: m.generate(input_ids=i2, attention_mask=m2, max_length=5, num_beams=a.beams,
                                         num_return_sequences=a.beams)
                with torch.no_grad():
                    sync = torch.cuda.synchronize if where == "cuda" else (lambda: None)
                    r = timed(ref, a.ref_reps, 1, sync, on_gpu=where == "cuda")
                    if where == "cuda":
                        r["profiled_kernels"] = count_kernels(ref)
                        same = torch.equal(ref().cpu(), run().cpu())
                        r["same_sequences_as_gr_amd"] = bool(same)
                res[f"transformers_{where}"] = r
            except Exception as e:      # report, do not hide
                res[f"transformers_{where}"] = {"error": repr(e)[:300]}
        res["transformers_version"] = transformers.__version__
    else:
        res["transformers_cuda"] = {"error": "transformers is not importable here"}
    g = res["gr_amd"]["device_ms_per_call"]
    base = res.get("transformers_cuda", {})
    if "wall_ms_per_call" in base:
        res["ratio_reference_over_gr_amd"] = base["wall_ms_per_call"] / g
        res["ratio_baseline"] = "transformers generate under torch-ROCm on the same GPU, wall time per call"
    elif "wall_ms_per_call" in res.get("transformers_cpu", {}):
        res["ratio_reference_over_gr_amd"] = res["transformers_cpu"]["wall_ms_per_call"] / g
        res["ratio_baseline"] = "transformers generate on the host CPU (not a GPU baseline), wall time per call"
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
