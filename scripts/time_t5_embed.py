"""Device time of one ``generate`` call of the T5 embedding retriever at the reference's inference shape
(T5/main.py: 256 users, [user vector, up to 20 items] = 21 positions, d_model 512, d_ff 256, 4 heads of 16, six
blocks, 768 -> 768) on the gfx950 kernels, next to the float32 restatement tests/t5_embed_ref.py run by torch on
the same GPU in the same process, and next to transformers' T5EncoderModel with two nn.Linear when it imports.

    python scripts/time_t5_embed.py [--out profiles/r20/t5_embed.txt]
    rocprofv3 --kernel-trace --stats ... -- python scripts/time_t5_embed.py --only-kernels   (per-kernel shares)
    python scripts/time_t5_embed.py --rows [--out profiles/r25/t5_embed_rows.txt]       (the id-sequence entry)
    rocprofv3 --kernel-trace --stats ... -- python scripts/time_t5_embed.py --rows --only-kernels

Each call is timed by its own pair of events after a warm-up; the figure is the median over ``--reps`` calls
with the minimum, the quartiles and the maximum beside it.  The fp32 floor is the multiply-adds the shapes
need over the 157 TFLOP/s fp32 matrix rate.
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
import t5_embed_ref as ref  # noqa: E402

PARAMS = dict(d_model=512, d_ff=256, num_heads=4, d_kv=16, dropout_rate=0.1, num_layers=2, input_emb_dim=768,
              target_emb_dim=768, temperature=0.07)
FP32_MATRIX_FLOPS = 157e12


def inputs(B, S, dim, dev):
    """Right-padded sequences, lengths uniform on 2..S."""
    rng = np.random.default_rng(0)
    seq = np.zeros((B, S, dim), np.float32)
    mask = np.zeros((B, S), np.int64)
    for b in range(B):
        n = int(rng.integers(2, S + 1))
        seq[b, :n] = 0.5 * rng.standard_normal((n, dim)).astype(np.float32)
        mask[b, :n] = 1
    return torch.from_numpy(seq).to(dev), torch.from_numpy(mask).to(dev)


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


def macs_per_user(S, p, layers):
    d, inner = p["d_model"], p["num_heads"] * p["d_kv"]
    block = S * (d * 3 * inner + inner * d + 2 * d * p["d_ff"])
    return S * p["input_emb_dim"] * d + layers * block + p["target_emb_dim"] * d


def weight_bytes(p, layers):
    d, inner = p["d_model"], p["num_heads"] * p["d_kv"]
    return 4 * (p["input_emb_dim"] * d + layers * (4 * inner * d + 2 * d * p["d_ff"]) + p["target_emb_dim"] * d)


def wall(fn, reps, warmup):
    """Wall-clock of ``fn`` from an idle device to an idle device (host work included), per call."""
    import time
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    q = np.percentile(np.array(ms), [0, 25, 50, 75, 100])
    return dict(median_ms=float(q[2]), min_ms=float(q[0]), q25_ms=float(q[1]), q75_ms=float(q[3]), max_ms=float(q[4]),
                calls=reps)


def rows_report(a, model, dev):
    """``--rows``: the id-sequence entry (``Tables``, ``embed_rows``) next to the dense call, in one process.

    1  the dense call, ``seq_embs`` already on the device (twice: the spread between the two runs is the yardstick)
    2  the dense path as the reference runs it: per sample the host gather from the numpy tables
       (T5/data_vision.py:131-154), ``collate``, ``.to(device)``, the call -- wall-clock around a synchronise
    3  the rows call, every user at ``--positions`` rows: the dense call's work minus input_proj plus the gather
    4  the rows call, lengths uniform on 2..``--positions`` (and the dense call on the same sequences, padded)
    5  the one-off projection of a 10,000-row table
    """
    from gr_amd import t5_embed
    B, S, dim = a.batch, a.positions, PARAMS["input_emb_dim"]
    rng = np.random.default_rng(0)
    items = (0.5 * rng.standard_normal((10000 - B, dim))).astype(np.float32)
    users = (0.5 * rng.standard_normal((B, dim))).astype(np.float32)
    full = [dict(history=rng.integers(0, len(items), S - 1).tolist(), user_id=u + 1, target_id=0) for u in range(B)]
    ragged = [dict(s, history=s["history"][:int(rng.integers(2, S + 1)) - 1]) for s in full]
    tables = t5_embed.Tables(model, items, users)

    def vectors(samples):      # the reference's __getitem__
        return [dict(seq_embs=np.concatenate([np.expand_dims(users[s["user_id"] - 1], 0),
                                              np.array([items[i] for i in s["history"]])], axis=0),
                     seq_len=len(s["history"]) + 1, target_emb=items[s["target_id"]], target_id=s["target_id"],
                     user_id=s["user_id"]) for s in samples]

    def dense_inputs(samples):
        b = t5_embed.collate(vectors(samples))
        return b["seq_embs"].to(dev), b["attention_mask"].to(dev)

    def ids(samples):
        b = t5_embed.collate_ids(samples, tables.n_items)
        return b["tokens"].to(dev), b["offsets"].to(dev)

    seq, mask = dense_inputs(full)
    rseq, rmask = dense_inputs(ragged)
    tok, off = ids(full)
    rtok, roff = ids(ragged)
    dense = lambda: model.generate(seq, mask)
    rows = lambda: model.embed_rows(tables, tok, off)
    rows_ragged = lambda: model.embed_rows(tables, rtok, roff)
    if a.only_kernels:
        for _ in range(10):
            rows_ragged()
        torch.cuda.synchronize()
        return None
    same = lambda x, y: bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
    res = {"shape": dict(B=B, S=S, table_rows=int(tables.table.shape[0]), live_rows_uniform=int(rtok.shape[0]),
                         **{k: PARAMS[k] for k in ("d_model", "d_ff", "num_heads", "d_kv", "input_emb_dim", "target_emb_dim")},
                         blocks=len(model.model.encoder.block)),
           "device": torch.cuda.get_device_name(0),
           "upload_bytes_dense": int(seq.numel() * 4 + mask.numel() * 8), "upload_bytes_ids": int((tok.numel() + off.numel()) * 8),
           "bits_equal_full": same(rows(), dense()), "bits_equal_uniform": same(rows_ragged(), model.generate(rseq, rmask))}
    res["1_dense_on_device_run1"] = timed(dense, a.reps, 5)
    res["3_rows_all_full"] = timed(rows, a.reps, 5)
    res["1_dense_on_device_run2"] = timed(dense, a.reps, 5)
    res["2_dense_as_the_reference_feeds_it_wall"] = wall(lambda: model.generate(*dense_inputs(full)), a.reps, 3)
    res["2b_rows_from_host_ids_wall"] = wall(lambda: model.embed_rows(tables, *ids(full)), a.reps, 3)
    res["4_rows_uniform_lengths"] = timed(rows_ragged, a.reps, 5)
    res["4b_dense_uniform_lengths"] = timed(lambda: model.generate(rseq, rmask), a.reps, 5)
    binding, table = model.binding(), tables.table
    res["5_project_10000_rows"] = timed(lambda: gr_amd.ops.t5_embed_project(binding, table), a.reps, 5)
    d1, d2 = res["1_dense_on_device_run1"]["median_ms"], res["1_dense_on_device_run2"]["median_ms"]
    r3 = res["3_rows_all_full"]["median_ms"]
    res["dense_run_to_run_spread_ms"] = abs(d1 - d2)
    res["rows_full_minus_dense_ms"] = r3 - min(d1, d2)
    res["rows_full_within_the_spread_of_dense"] = bool(r3 <= max(d1, d2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--positions", type=int, default=21)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only-kernels", action="store_true", help="a few calls of the kernels alone (for a kernel trace)")
    ap.add_argument("--rows", action="store_true", help="the id-sequence entry next to the dense call (see rows_report)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = gr_amd.t5_embed.TIGER(PARAMS)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    model = model.to(dev).eval()
    if a.rows:
        res = rows_report(a, model, dev)
        if res is not None:
            line = json.dumps(res, indent=1)
            print(line)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    f.write(line + "\n")
        return
    seq, mask = inputs(a.batch, a.positions, PARAMS["input_emb_dim"], dev)
    run = lambda: model.generate(seq, mask)
    if a.only_kernels:
        for _ in range(10):
            run()
        torch.cuda.synchronize()
        return
    layers = len(model.model.encoder.block)
    macs = macs_per_user(a.positions, PARAMS, layers) * a.batch
    res = {"shape": dict(B=a.batch, S=a.positions, lengths="uniform on 2..S", **{k: PARAMS[k] for k in
                         ("d_model", "d_ff", "num_heads", "d_kv", "input_emb_dim", "target_emb_dim")}, blocks=layers),
           "device": torch.cuda.get_device_name(0),
           "multiply_adds_per_call": macs, "fp32_floor_ms_by_the_shapes": 2 * macs / FP32_MATRIX_FLOPS * 1e3,
           "weight_bytes": weight_bytes(PARAMS, layers), "launches_per_call": 1 + 4 * layers + 3}
    res["gr_amd"] = timed(run, a.reps, 5)
    cfg = dict(model.config)
    sd = {k: v.detach() for k, v in model.state_dict().items() if v.shape[0] != 32128}
    with torch.no_grad():
        restated = lambda: ref.forward(cfg, sd, seq, mask, torch.float32)[0]
        want = restated()
        res["restatement_float32_torch"] = timed(restated, a.reps, 5)
        res["restatement_float32_torch"]["max_abs_difference_from_gr_amd"] = float((want - run()).abs().max())
        try:
            import transformers
            enc = transformers.T5EncoderModel(transformers.T5Config(
                d_model=PARAMS["d_model"], d_ff=PARAMS["d_ff"], num_heads=PARAMS["num_heads"], d_kv=PARAMS["d_kv"],
                dropout_rate=PARAMS["dropout_rate"])).to(dev).eval()
            enc.load_state_dict({k[len("model."):]: v for k, v in model.state_dict().items() if k.startswith("model.")})
            inp, outp = model.input_proj, model.output_proj

            def hf():
                hid = enc(inputs_embeds=inp(seq), attention_mask=mask).last_hidden_state
                m = mask.unsqueeze(-1).float()
                pooled = (hid * m).sum(dim=1) / m.sum(dim=1).clamp(min=1e-9)
                return torch.nn.functional.normalize(outp(pooled), p=2, dim=1, eps=1e-8)
            got = hf()
            res["transformers_T5EncoderModel"] = timed(hf, a.reps, 5)
            res["transformers_T5EncoderModel"]["max_abs_difference_from_gr_amd"] = float((got - run()).abs().max())
            res["transformers_version"] = transformers.__version__
        except Exception as e:      # report, do not hide
            res["transformers_T5EncoderModel"] = {"error": repr(e)[:300]}
    g = res["gr_amd"]["median_ms"]
    res["restatement_over_gr_amd"] = res["restatement_float32_torch"]["median_ms"] / g
    res["faster_than_the_restatement"] = bool(g < res["restatement_float32_torch"]["median_ms"])
    res["share_of_fp32_floor"] = res["fp32_floor_ms_by_the_shapes"] / g
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
