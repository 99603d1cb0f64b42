"""Time of one prefix TIGER.generate call at the reference's inference shape (256 users, 20 beams, 80
history tokens, 2 + 2 layers, d_model 64, five 768-wide BERT vectors per level) on the gfx950 kernels,
next to the plain ``gr_amd.TIGER.generate`` on the same T5 weights in the same process (the difference
is what the three adapters and the three extra encoder positions cost) and, when ``transformers`` is
importable, next to the reference formulation on the same GPU: the adapters as torch modules plus
``T5ForConditionalGeneration.generate(inputs_embeds=...)`` under torch-ROCm.

    python scripts/time_tiger_prefix_generate.py [--out profiles/r18/tiger_prefix_generate.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_tiger_prefix_generate.py --calls-only 50

Device time per call from events around ``--reps`` back-to-back calls, host time per call from
perf_counter without synchronisation, launches per call from the design (checked against a
torch.profiler kernel count when it is available).  ``--calls-only N`` runs N prefix calls and nothing
else: the run a kernel trace is taken from (per-kernel times are not measured by this script).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gr_amd  # noqa: E402
from time_tiger_generate import CFG, count_kernels, inputs, timed  # noqa: E402

# multiply-adds of one user's three adapters and of its encoder, from the shapes (not measured)
def adapter_macs(S, d, bert_dim, n_vec):
    per = n_vec * bert_dim * d + 2 * n_vec * d * d + 2 * S * d * d + 2 * S * n_vec * d + 8 * S * d * d
    return 3 * per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--beams", type=int, default=20)
    ap.add_argument("--items", type=int, default=20)
    ap.add_argument("--bert-dim", type=int, default=768)
    ap.add_argument("--n-vec", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = dict(CFG, bert_dim=a.bert_dim)
    model = gr_amd.tiger_prefix.TIGER(cfg).to(dev).eval()
    ids, mask = inputs(a.batch, a.items, dev)
    prof = [torch.randn(a.batch, a.n_vec, a.bert_dim, device=dev) for _ in range(3)]
    run = lambda: model.generate(ids, mask, num_beams=a.beams, prof_lvl1=prof[0], prof_lvl2=prof[1], prof_lvl3=prof[2])
    if a.calls_only:
        for _ in range(a.calls_only):
            run()
        torch.cuda.synchronize()
        return
    plain_model = gr_amd.TIGER(CFG)
    plain_model.load_state_dict({k: v for k, v in model.state_dict().items() if k.startswith("model.")})
    plain_model = plain_model.to(dev).eval()
    plain = lambda: plain_model.generate(ids, mask, num_beams=a.beams)
    S = 4 * a.items
    res = {"shape": dict(B=a.batch, beams=a.beams, tokens=S, max_length=5, bert_dim=a.bert_dim, n_vec=a.n_vec),
           "device": torch.cuda.get_device_name(0),
           "adapter_multiply_adds_per_user": adapter_macs(S, CFG["d_model"], a.bert_dim, a.n_vec)}
    # the two alternate, so that a drift of the clock or of the shared host shows in both
    rounds = []
    for _ in range(3):
        rounds.append((timed(run, a.reps, 5, torch.cuda.synchronize), timed(plain, a.reps, 5, torch.cuda.synchronize)))
    best = lambda i: min((r[i] for r in rounds), key=lambda t: t["device_ms_per_call"])
    res["gr_amd_prefix"] = dict(best(0), launches=3, profiled_kernels=count_kernels(run),
                                device_ms_per_call_rounds=[r[0]["device_ms_per_call"] for r in rounds])
    res["gr_amd_plain"] = dict(best(1), launches=2, profiled_kernels=count_kernels(plain),
                               device_ms_per_call_rounds=[r[1]["device_ms_per_call"] for r in rounds])
    res["prefix_minus_plain_device_ms"] = (res["gr_amd_prefix"]["device_ms_per_call"]
                                           - res["gr_amd_plain"]["device_ms_per_call"])
    try:
        import transformers
    except ImportError:
        transformers = None
    if transformers is not None:
        try:
            t5 = transformers.T5ForConditionalGeneration(transformers.T5Config(
                decoder_start_token_id=CFG["pad_token_id"], **CFG)).eval()
            t5.load_state_dict({k[len("model."):]: v for k, v in model.state_dict().items() if k.startswith("model.")})
            t5 = t5.to(dev)
            adapters = [model.adapter_lvl1, model.adapter_lvl2, model.adapter_lvl3]

            def adapter(m, h, vecs):       # ProfessionalAdapter.forward on torch's own modules
                kv = m.bert_proj(vecs)
                attn, _ = m.cross_attn(h, kv, kv)
                x = m.norm1(h + attn)
                x = m.norm2(x + m.ffn(x))
                return x.mean(dim=1, keepdim=True)

            def ref():
                h = t5.shared(ids)
                emb = torch.cat([adapter(m, h, p) for m, p in zip(adapters, prof)] + [h], dim=1)
                ext = torch.cat([torch.ones(a.batch, 3, device=dev, dtype=mask.dtype), mask], dim=1)
                return t5.generate(inputs_embeds=emb, attention_mask=ext, max_length=5, num_beams=a.beams,
                                   num_return_sequences=a.beams)

            with torch.no_grad():
                r = timed(ref, a.ref_reps, 1, torch.cuda.synchronize)
                r["profiled_kernels"] = count_kernels(ref)
                got, want = run().cpu(), ref().cpu()
                r["same_sequences_as_gr_amd"] = bool(got.shape == want.shape and torch.equal(got, want))
                if got.shape == want.shape:
                    rows = (got.view(a.batch, -1) == want.view(a.batch, -1)).all(1)
                    r["users_with_the_same_hypotheses"] = int(rows.sum())
            res["transformers_cuda"] = r
            res["ratio_reference_over_gr_amd"] = r["wall_ms_per_call"] / res["gr_amd_prefix"]["device_ms_per_call"]
            res["ratio_baseline"] = ("torch-module adapters + transformers generate(inputs_embeds) under torch-ROCm on "
                                     "the same GPU, wall time per call")
        except Exception as e:      # report, do not hide
            res["transformers_cuda"] = {"error": repr(e)[:300]}
        res["transformers_version"] = transformers.__version__
    else:
        res["transformers_cuda"] = {"error": "transformers is not importable here"}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
