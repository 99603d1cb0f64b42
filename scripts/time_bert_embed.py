"""Device time of one ``BertEncoder.embed`` call at bert-base (12 layers, H 768, 12 heads, I 3072) on the gfx950 kernels,
batches of 32 sequences at S 128 and at S 512 with seeded weights, next to ``transformers.BertModel`` in float32 plus
the reference's pooling lines (when it imports) and to the float32 restatement tests/bert_embed_ref.py, both run by
torch on the same GPU in the same process with the same weights.

    python scripts/time_bert_embed.py [--out profiles/r21/bert_embed.txt]
    rocprofv3 --kernel-trace --stats ... -- python scripts/time_bert_embed.py --only-kernels   (per-kernel shares)
    python scripts/time_bert_embed.py --ragged [--out profiles/r23/bert_embed_ragged.txt]
    python scripts/time_bert_embed.py --padded-only       (the padded call alone: for a build of another commit)
    python scripts/time_bert_embed.py --bf16 [--ragged] [--out profiles/r24/bert_embed_bf16.txt]
    rocprofv3 --kernel-trace --stats ... -- python scripts/time_bert_embed.py --only-kernels --bf16

``--bf16``: the bf16 precision (``embed(..., precision="bf16")``: bf16 GEMM operands, fp32 accumulation) next to the fp32
call on the same inputs in the same process; with ``--ragged`` the ragged entry of both precisions as well.

``--ragged``: the ragged entry (``embed(..., ragged=True)``: only the rows up to each sequence's last live position)
next to the padded call on the same inputs in the same process, for two length distributions -- one sequence of S
and the rest uniform on S/2..S, or on 8..S -- with the exact row bound (a host-side mask) and with the bound B * S
(a device-side mask: oversized grids that exit on the device's row count).

Each call is timed by its own pair of events after a warm-up; the figure is the median over ``--reps`` calls with
the minimum, the quartiles and the maximum beside it.  The fp32 floor is the multiply-adds the shapes need (every
position computed, the padded ones too: the call does not pack) over the 157 TFLOP/s fp32 matrix rate.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gr_amd  # noqa: E402
import bert_embed_ref as ref  # noqa: E402

CONFIG = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
              hidden_act="gelu", max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=0)
FP32_MATRIX_FLOPS = 157e12


def inputs(B, S, dev, low=None):
    """Right-padded sequences, the first of full length, the others uniform on low..S (S/2..S by default)."""
    rng = np.random.default_rng(0)
    ids = np.zeros((B, S), np.int64)
    mask = np.zeros((B, S), np.int64)
    low = S // 2 if low is None else low
    for b in range(B):
        n = S if b == 0 else int(rng.integers(low, S + 1))
        ids[b, :n] = rng.integers(1, CONFIG["vocab_size"], n)
        mask[b, :n] = 1
    return torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    q = np.percentile(ms, [0, 25, 50, 75, 100])
    return dict(median_ms=float(q[2]), min_ms=float(q[0]), q25_ms=float(q[1]), q75_ms=float(q[3]), max_ms=float(q[4]),
                calls=reps)


def macs(B, S):
    H, I, L = CONFIG["hidden_size"], CONFIG["intermediate_size"], CONFIG["num_hidden_layers"]
    projections = S * (4 * H * H + 2 * H * I)
    attention = 2 * S * S * H
    return B * L * (projections + attention), B * L * projections, B * L * attention


def seeded_model(dev):
    torch.manual_seed(0)
    model = gr_amd.bert_embed.BertEncoder(CONFIG)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "LayerNorm.weight" in name:
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            elif name.endswith(".bias"):
                p.copy_(0.1 * torch.randn_like(p))
            elif name.startswith("embeddings."):
                p.copy_(torch.randn_like(p))
            else:
                p.copy_(torch.randn_like(p) * p.shape[1] ** -0.5)
    return model.to(dev).eval()


def ragged_report(model, a, dev):
    """The padded call, the ragged call with the exact bound and the ragged call with the bound B * S, per shape and
    length distribution, interleaved in one process on the same weights."""
    res = {"config": {k: CONFIG[k] for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size")},
           "device": torch.cuda.get_device_name(0), "timing": f"one pair of events per call, median of {a.reps} calls "
           "after 5 warm-up calls, quartiles beside it", "points": []}
    for S in a.positions:
        for name, low in (("one of S, the others uniform on S/2..S", None), ("one of S, the others uniform on 8..S", 8)):
            ids, mask = inputs(a.batch, S, dev, low)
            lens = mask.sum(1).cpu().numpy().astype(np.int64)              # right padding: the length is the live count
            exact = gr_amd.bert_embed.row_bound(mask.cpu())
            assert exact == int(lens.sum())
            row = {"B": a.batch, "S": S, "lengths": name, "kept_rows": exact,
                   "kept_row_share": exact / (a.batch * S), "attention_share": float((lens ** 2).sum()) / (a.batch * S * S)}
            padded = lambda: model.embed(ids, mask)
            ragged = lambda: model.embed(ids, mask, ragged=True, rows_bound=exact)
            loose = lambda: model.embed(ids, mask, ragged=True)
            row["same_bits"] = bool(torch.equal(padded(), ragged()) and torch.equal(padded(), loose()))
            row["padded"] = timed(padded, a.reps, 5)
            row["ragged_exact_bound"] = timed(ragged, a.reps, 5)
            row["ragged_bound_B_S"] = timed(loose, a.reps, 5)
            row["padded_again"] = timed(padded, a.reps, 5)                  # the drift of the run itself
            row["ragged_over_padded"] = row["ragged_exact_bound"]["median_ms"] / row["padded"]["median_ms"]
            row["ragged_bound_B_S_over_padded"] = row["ragged_bound_B_S"]["median_ms"] / row["padded"]["median_ms"]
            res["points"].append(row)
    return res


def bf16_report(model, a, dev):
    """The bf16 precision next to the fp32 call on the same inputs in the same process, interleaved: the padded calls,
    and with ``--ragged`` the ragged calls with the exact row bound as well."""
    res = {"config": {k: CONFIG[k] for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size")},
           "device": torch.cuda.get_device_name(0), "timing": f"one pair of events per call, median of {a.reps} calls "
           "after 5 warm-up calls, quartiles beside it", "shapes": []}
    for S in a.positions:
        ids, mask = inputs(a.batch, S, dev)
        total, proj, attn = macs(a.batch, S)
        exact = gr_amd.bert_embed.row_bound(mask.cpu())
        row = {"B": a.batch, "S": S, "lengths": "one of S, the others uniform on S/2..S", "multiply_adds_per_call": total,
               "projection_multiply_adds": proj, "attention_multiply_adds": attn, "kept_rows": exact}
        fp32 = lambda: model.embed(ids, mask)
        bf16 = lambda: model.embed(ids, mask, precision="bf16")
        a32, a16 = fp32(), bf16()
        row["bf16_max_difference_from_fp32_over_max"] = float((a16 - a32).abs().max()) / float(a32.abs().max())
        row["fp32_padded"] = timed(fp32, a.reps, 5)
        row["bf16_padded"] = timed(bf16, a.reps, 5)
        row["fp32_padded_again"] = timed(fp32, a.reps, 5)                  # the drift of the run itself
        row["bf16_over_fp32_padded"] = row["bf16_padded"]["median_ms"] / row["fp32_padded"]["median_ms"]
        row["fp32_over_bf16_padded"] = row["fp32_padded"]["median_ms"] / row["bf16_padded"]["median_ms"]
        row["bf16_padded_tflops"] = 2 * total / (row["bf16_padded"]["median_ms"] * 1e-3) / 1e12
        row["fp32_padded_tflops"] = 2 * total / (row["fp32_padded"]["median_ms"] * 1e-3) / 1e12
        if a.ragged:
            r32 = lambda: model.embed(ids, mask, ragged=True, rows_bound=exact)
            r16 = lambda: model.embed(ids, mask, ragged=True, rows_bound=exact, precision="bf16")
            row["ragged_same_bits"] = bool(torch.equal(r32(), a32) and torch.equal(r16(), a16))
            row["fp32_ragged"] = timed(r32, a.reps, 5)
            row["bf16_ragged"] = timed(r16, a.reps, 5)
            row["bf16_over_fp32_ragged"] = row["bf16_ragged"]["median_ms"] / row["fp32_ragged"]["median_ms"]
            row["bf16_ragged_over_bf16_padded"] = row["bf16_ragged"]["median_ms"] / row["bf16_padded"]["median_ms"]
        res["shapes"].append(row)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--positions", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only-kernels", action="store_true", help="a few calls of the kernels alone (for a kernel trace)")
    ap.add_argument("--ragged", action="store_true", help="the ragged entry next to the padded call")
    ap.add_argument("--padded-only", action="store_true", help="the padded call alone")
    ap.add_argument("--bf16", action="store_true", help="the bf16 precision next to the fp32 call (with --ragged: both entries)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model = seeded_model(dev)
    if a.only_kernels:
        for S in a.positions:
            ids, mask = inputs(a.batch, S, dev)
            exact = gr_amd.bert_embed.row_bound(mask.cpu()) if a.ragged else None
            precision = "bf16" if a.bf16 else "fp32"
            for _ in range(5):
                if a.ragged:
                    model.embed(ids, mask, ragged=True, rows_bound=exact, precision=precision)
                else:
                    model.embed(ids, mask, precision=precision)
        torch.cuda.synchronize()
        return
    if a.bf16 or a.ragged or a.padded_only:
        if a.bf16:
            res = bf16_report(model, a, dev)
        elif a.ragged:
            res = ragged_report(model, a, dev)
        else:
            res = {"device": torch.cuda.get_device_name(0), "shapes": []}
            for S in a.positions:
                ids, mask = inputs(a.batch, S, dev)
                res["shapes"].append({"B": a.batch, "S": S, "padded": timed(lambda: model.embed(ids, mask), a.reps, 5)})
        line = json.dumps(res, indent=1)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    res = {"config": {k: CONFIG[k] for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size")},
           "device": torch.cuda.get_device_name(0), "launches_per_call": 2 + 7 * CONFIG["num_hidden_layers"],
           "weight_bytes": sum(v.numel() for k, v in sd.items() if k.startswith("encoder.")) * 4, "shapes": []}
    hf = None
    try:
        import transformers
        hf = transformers.BertModel(transformers.BertConfig(**CONFIG, attn_implementation="eager")).to(dev).eval()
        hf.load_state_dict(sd, strict=False)
        res["transformers_version"] = transformers.__version__
    except Exception as e:      # report, do not hide
        res["transformers_BertModel"] = {"error": repr(e)[:300]}
    for S in a.positions:
        ids, mask = inputs(a.batch, S, dev)
        total, proj, attn = macs(a.batch, S)
        row = {"B": a.batch, "S": S, "lengths": "one of S, the others uniform on S/2..S", "multiply_adds_per_call": total,
               "projection_multiply_adds": proj, "attention_multiply_adds": attn,
               "fp32_floor_ms_by_the_shapes": 2 * total / FP32_MATRIX_FLOPS * 1e3}
        run = lambda: model.embed(ids, mask)
        row["gr_amd"] = timed(run, a.reps, 5)
        mine = run()
        scale = float(mine.abs().max())
        with torch.no_grad():
            if hf is not None:
                def hf_run():
                    hidden = hf(input_ids=ids, attention_mask=mask).last_hidden_state
                    masked = hidden * mask.unsqueeze(-1)
                    return masked[:, 1:, :].sum(dim=1) / mask[:, 1:].sum(dim=-1, keepdim=True).clamp(min=1e-9)
                got = hf_run()
                row["transformers_BertModel_float32"] = timed(hf_run, a.reps, 5)
                row["transformers_BertModel_float32"]["max_difference_from_gr_amd_over_max"] = float((got - mine).abs().max()) / scale
                row["BertModel_over_gr_amd"] = row["transformers_BertModel_float32"]["median_ms"] / row["gr_amd"]["median_ms"]

            def restated():
                return ref.pool(ref.forward(CONFIG, sd, ids, mask, None, torch.float32), mask, "mean_no_cls")
            got = restated()
            row["restatement_float32_torch"] = timed(restated, max(5, a.reps // 5), 2)
            row["restatement_float32_torch"]["max_difference_from_gr_amd_over_max"] = float((got - mine).abs().max()) / scale
        row["restatement_over_gr_amd"] = row["restatement_float32_torch"]["median_ms"] / row["gr_amd"]["median_ms"]
        row["share_of_fp32_floor"] = row["fp32_floor_ms_by_the_shapes"] / row["gr_amd"]["median_ms"]
        row["tflops"] = 2 * total / (row["gr_amd"]["median_ms"] * 1e-3) / 1e12
        res["shapes"].append(row)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
