"""Time of one TIGER teacher-forced forward (the call of the reference's ``eval_loss``) at the reference's
evaluation shape (256 users, 80 history tokens, labels [256, 4], d_model 64, 2 + 2 layers) on the gfx950
kernels, plain and prefixed (five 768-wide BERT vectors per level), next to two baselines on the same GPU, in
the same process, with the same weights: the float32 restatement tests/tiger_forward_ref.py under torch, and
``transformers``' T5ForConditionalGeneration.forward when it is importable (plain call only: the prefix model
is the reference's own class).  ``generate(num_beams=20)`` is timed in the same run: the forward does the same
encoder work and at most Ld decoder rows per user where generate does up to 20 per step.

    python scripts/time_tiger_forward.py [--out profiles/r22/tiger_forward.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_tiger_forward.py --calls-only 50

Every figure is the median of ``--reps`` calls, each between its own pair of events, after warm-up.
``--calls-only N`` runs N plain and N prefix calls and nothing else: the run a kernel trace is taken from.
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
from time_tiger_generate import CFG, inputs  # noqa: E402


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)
    return dict(median_ms=float(np.median(t)), min_ms=t[0], max_ms=t[-1], reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--items", type=int, default=20)
    ap.add_argument("--label-len", type=int, default=4)
    ap.add_argument("--bert-dim", type=int, default=768)
    ap.add_argument("--n-vec", type=int, default=5)
    ap.add_argument("--beams", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = gr_amd.tiger_prefix.TIGER(dict(CFG, bert_dim=a.bert_dim)).to(dev).eval()
    ids, mask = inputs(a.batch, a.items, dev)
    g = torch.Generator().manual_seed(1)
    labels = torch.randint(1, CFG["vocab_size"], (a.batch, a.label_len), generator=g)
    labels[torch.rand(a.batch, generator=g) < 0.1, -1] = -100
    labels = labels.to(dev)
    prof = [torch.randn(a.batch, a.n_vec, a.bert_dim, device=dev) for _ in range(3)]
    with torch.no_grad():
        plain = lambda: model(ids, mask, labels)
        prefixed = lambda: model(ids, mask, labels, *prof)
        generate = lambda: model.generate(ids, mask, num_beams=a.beams)
        if a.calls_only:
            for _ in range(a.calls_only):
                plain()
                prefixed()
            torch.cuda.synchronize()
            return
        res = {"shape": dict(B=a.batch, tokens=4 * a.items, labels=[a.batch, a.label_len], d_model=CFG["d_model"],
                             layers="2 + 2", bert_dim=a.bert_dim, n_vec=a.n_vec),
               "device": torch.cuda.get_device_name(0), "method": f"median of {a.reps} event-timed calls after "
               f"{a.warmup} warm-up calls; device time between the events around one call"}
        res["gr_amd_forward"] = dict(median_ms(plain, a.reps, a.warmup), launches=3)
        res["gr_amd_forward_prefix"] = dict(median_ms(prefixed, a.reps, a.warmup), launches=4)
        res["gr_amd_generate_20_beams"] = dict(median_ms(generate, a.reps, a.warmup), launches=2)
        res["forward_not_slower_than_generate"] = bool(res["gr_amd_forward"]["median_ms"]
                                                       <= res["gr_amd_generate_20_beams"]["median_ms"])
        # baseline 1: the float32 restatement under torch on the same GPU (factory calls land on the device)
        import tiger_forward_ref as fref
        sd = {k[len("model."):]: v.detach() for k, v in model.state_dict().items() if k.startswith("model.")}
        ad = {k: v.detach() for k, v in model.state_dict().items() if k.startswith("adapter_lvl")}
        cfg = dict(CFG, layer_norm_epsilon=1e-6)
        with torch.device(dev):
            loss_r, logits_r, _ = fref.forward(cfg, sd, ids, mask, labels)
            loss_g, logits_g = plain()
            res["restatement_torch"] = dict(
                median_ms(lambda: fref.forward(cfg, sd, ids, mask, labels), a.reps, a.warmup),
                max_abs_logit_difference_from_gr_amd=float((logits_r - logits_g).abs().max()),
                loss_difference_from_gr_amd=float((loss_r - loss_g).abs()))
            loss_r, logits_r, _ = fref.forward_prefix(cfg, {**sd, **ad}, ids, mask, prof, labels)
            loss_g, logits_g = prefixed()
            res["restatement_torch_prefix"] = dict(
                median_ms(lambda: fref.forward_prefix(cfg, {**sd, **ad}, ids, mask, prof, labels), a.reps, a.warmup),
                max_abs_logit_difference_from_gr_amd=float((logits_r - logits_g).abs().max()),
                loss_difference_from_gr_amd=float((loss_r - loss_g).abs()))
        # baseline 2: transformers' own forward, when it imports
        try:
            import transformers
            t5 = transformers.T5ForConditionalGeneration(transformers.T5Config(
                decoder_start_token_id=CFG["pad_token_id"], **CFG)).eval()
            t5.load_state_dict(sd)
            t5 = t5.to(dev)
            ref = lambda: t5(input_ids=ids, attention_mask=mask, labels=labels)
            out = ref()
            loss_g, logits_g = plain()
            res["transformers_forward"] = dict(
                median_ms(ref, a.reps, a.warmup), version=transformers.__version__,
                max_abs_logit_difference_from_gr_amd=float((out.logits - logits_g).abs().max()),
                loss_difference_from_gr_amd=float((out.loss - loss_g).abs()))
        except Exception as e:      # report, do not hide
            res["transformers_forward"] = {"error": repr(e)[:300]}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
