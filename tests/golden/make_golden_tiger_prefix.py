"""Fixtures for the TIGER prefix tests: the reference's own prefix ``TIGER`` (RQVAE-T5-prefix/model.py and
utils.py, imported at run time from a checkout of the reference; needs ``transformers``) on seeded
models, histories and professional-hierarchy vectors, next to the plain-torch restatement
tests/tiger_prefix_ref.py in float32 and float64.

    python tests/golden/make_golden_tiger_prefix.py <reference checkout>   ->  tests/golden/tiger_prefix_*.npz

It follows make_golden_tiger.py (the same ``histories``, bf16-representable weights, float64 margins
and ``meta``) and stores only data: the config, the state dict (T5 entries without their ``model.``
prefix and tied entries once, adapters under their full names), ids, mask, the three prof tensors
(bf16-representable as well), the reference's prefix tokens (rows 0..2 of ``_build_prefix_inputs``), its
encoder output on ``inputs_embeds`` for the first users, its sequences and scores, the float64
restatement's results, gaps, certification and the reference's metrics.

Before a file is written the generator asserts: restatement == reference in float32 (sequences on
every user, scores within 1e-6, prefix tokens and encoder output within 1e-5), at least 90 % of the
users certified, that the prefix changes the returned set for at least a quarter of the users, and
that a restatement which averages the adapter's rows over the unmasked positions only (the reference
averages over all of them, padding included) moves user 0's prefix tokens by more than 100 x
``prefix_err32``, so a test at 4 x ``prefix_err32`` tells the two apart.  A d_model-64 T5 and a
768-wide bert_proj do not fit one file under 1 MiB, so the 768-long chain has a fixture of its own on a
small T5.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_tiger as base  # noqa: E402  (puts tests/ on the path)
import tiger_prefix_ref as pref  # noqa: E402
import tiger_ref  # noqa: E402

TOPK = base.TOPK
ENC_USERS = base.ENC_USERS

FIXTURES = {
    #  name                   config changes (S = the history's tokens)                                 B  beams seed
    "tiger_prefix_main":     (dict(bert_dim=96, n_vec=5, S=80),                                          16, 20, 21),
    "tiger_prefix_bert768":  (dict(d_model=32, num_heads=4, d_kv=16, num_layers=1, num_decoder_layers=1,
                                   d_ff=64, bert_dim=768, n_vec=5, S=12),                                8, 5, 22),
    "tiger_prefix_h2_s125":  (dict(num_heads=2, d_kv=32, num_layers=1, num_decoder_layers=3, d_ff=128,
                                   bert_dim=32, n_vec=7, S=125),                                         8, 20, 23),
}


def load_reference(ref_dir):
    mods = []
    for name in ("model", "utils"):
        try:
            spec = importlib.util.spec_from_file_location(f"tiger_prefix_reference_{name}",
                                                          os.path.join(ref_dir, "RQVAE-T5-prefix", name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        except ImportError:
            if name == "model":
                raise
            mod = None          # utils.py imports matplotlib and tqdm
        mods.append(mod)
    return mods


def histories(cfg, S, B, rng):
    """make_golden_tiger.histories at S // 4 items, left-padded to S tokens."""
    ids, mask = base.histories(dict(cfg, max_len=S // 4), B, rng)
    pad = np.zeros((B, S - ids.shape[1]), np.int64)
    return np.concatenate([pad, ids], 1), np.concatenate([pad, mask], 1)


def bf16(t):
    return t.to(torch.bfloat16).float()


def make(name, model_mod, utils_mod):
    delta, B, beams, seed = FIXTURES[name]
    delta = dict(delta)
    S, n_vec = delta.pop("S"), delta.pop("n_vec")
    cfg = dict(base.MAIN, **delta)
    cfg.pop("max_len")
    torch.manual_seed(seed)
    model = model_mod.TIGER(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(bf16(p))
    t5cfg = model.model.config
    cfg_full = dict(cfg, layer_norm_epsilon=float(t5cfg.layer_norm_epsilon),
                    relative_attention_num_buckets=int(t5cfg.relative_attention_num_buckets),
                    relative_attention_max_distance=int(t5cfg.relative_attention_max_distance),
                    scale_decoder_outputs=bool(getattr(t5cfg, "scale_decoder_outputs", True)))
    assert cfg_full["relative_attention_num_buckets"] == 32 and cfg_full["relative_attention_max_distance"] == 128
    assert model.adapter_lvl1.norm1.eps == pref.LN_EPS
    full_sd = model.state_dict()
    keys = [[k, list(v.shape)] for k, v in full_sd.items()]
    sd32 = {(k[len("model."):] if k.startswith("model.") else k): v.detach().clone() for k, v in full_sd.items()}
    for k in base.TIED:
        assert torch.equal(sd32[k], sd32["shared.weight"])
    sd64 = {k: v.double() for k, v in sd32.items()}

    use_cache = cfg["num_decoder_layers"] <= cfg["num_layers"]     # see make_golden_tiger.ref_generate
    if not use_cache:
        model.model.generation_config.use_cache = False
    rng = np.random.default_rng(seed)
    ids, mask = histories(cfg, S, B, rng)
    tid, tmask = torch.from_numpy(ids), torch.from_numpy(mask)
    prof = [bf16(torch.from_numpy(rng.standard_normal((B, n_vec, cfg["bert_dim"]), dtype=np.float32)))
            for _ in range(3)]
    prof64 = [p.double() for p in prof]
    T = 5
    with torch.no_grad():
        out = model.generate(tid, tmask, num_beams=beams, prof_lvl1=prof[0], prof_lvl2=prof[1], prof_lvl3=prof[2],
                             return_dict_in_generate=True, output_scores=True)
        seq_ref, sc_ref = out.sequences, out.sequences_scores
        assert seq_ref.shape[1] == T, f"{name}: the reference cropped its result to {seq_ref.shape[1]} columns"
        seq_ref, sc_ref = seq_ref.view(B, beams, T), sc_ref.view(B, beams)
        embeds, ext_mask = model._build_prefix_inputs(tid, tmask, *prof)
        prefix_ref = embeds[:, :3].clone()
        enc_ref = model.model.encoder(inputs_embeds=embeds, attention_mask=ext_mask).last_hidden_state
        live = ext_mask.bool()
        # float32 restatement == reference
        tr32 = {}
        s32, c32, width = pref.beam_search(cfg_full, sd32, tid, tmask, prof, beams, T, trace=tr32, use_cache=use_cache)
        assert width == T
        bad = [b for b in range(B) if not torch.equal(s32[b], seq_ref[b])]
        assert not bad, f"{name}: float32 restatement != reference on users {bad}"
        d = (c32 - sc_ref).abs().max().item()
        assert d <= 1e-6, f"{name}: float32 restatement scores differ from the reference by {d}"
        d = (tr32["prefix"] - prefix_ref).abs().max().item()
        assert d <= 1e-5, f"{name}: prefix restatement differs from the reference by {d}"
        d = (tr32["enc"] - enc_ref)[live].abs().max().item()
        assert d <= 1e-5, f"{name}: encoder restatement differs from the reference by {d}"
        # float64 restatement, margins, tolerances
        tr64 = {}
        s64, c64, _ = pref.beam_search(cfg_full, sd64, tid, tmask, prof64, beams, T, trace=tr64, use_cache=use_cache)
        same = torch.tensor([torch.equal(s64[b], seq_ref[b]) for b in range(B)])
        score_err = (sc_ref.double() - c64)[same].abs().max().item()
        m = 4.0 * score_err
        certified = tr64["gaps"] > m
        share = certified.float().mean().item()
        prefix_err32 = ((prefix_ref.double() - tr64["prefix"]).abs().max() / tr64["prefix"].abs().max()).item()
        enc_err32 = ((enc_ref.double() - tr64["enc"])[live].abs().max() / tr64["enc"][live].abs().max()).item()
        logit_err32 = 0.0
        stopped = tr64["stopped_after"]
        assert torch.equal(stopped, tr32["stopped_after"])
        for t, (l32, l64) in enumerate(zip(tr32["logits"], tr64["logits"])):
            on = same & ((stopped < 0) | (stopped > t))
            e = (l32.double() - l64)[on].abs().amax(-1) / l64[on].abs().amax(-1)
            logit_err32 = max(logit_err32, e.max().item())
        early = int(((stopped > 0) & (stopped < T - 1)).sum())
        print(f"{name}: B {B} beams {beams}  ref==fp64 on {int(same.sum())}/{B} users, score err {score_err:.3e}, "
              f"m {m:.3e}, certified {int(certified.sum())}/{B}, min gap {tr64['gaps'].min().item():.3e}, "
              f"prefix err32 {prefix_err32:.3e}, enc err32 {enc_err32:.3e}, logit err32 {logit_err32:.3e}, "
              f"{early} users stop early")
        assert share >= 0.9, f"{name}: only {share:.2f} of the users certified"
        for b in range(B):
            if certified[b]:
                assert torch.equal(s64[b], seq_ref[b]), f"{name}: certified user {b} differs between fp32 and fp64"
        # the prefix matters, and the mean over all rows differs from a mean over the unmasked rows
        plain, _, _ = tiger_ref.beam_search(cfg_full, {k: v for k, v in sd32.items() if not k.startswith("adapter")},
                                            tid, tmask, beams, T, use_cache=use_cache)
        changed = sum(set(map(tuple, plain[b].tolist())) != set(map(tuple, s32[b].tolist())) for b in range(B))
        print(f"{name}: the prefix changes the returned set for {changed}/{B} users")
        assert changed * 4 >= B
        masked = pref.prefix_tokens(cfg_full, sd64, tid, prof64, row_mask=tmask)
        moved = ((masked - tr64["prefix"])[0].abs().max() / tr64["prefix"].abs().max()).item()
        print(f"{name}: a mean over the unmasked rows moves user 0's prefix by {moved:.3e} "
              f"({moved / prefix_err32:.0f} x prefix_err32; user 0 has {int(tmask[0].sum())} of {S} rows unmasked)")
        assert moved > 100 * prefix_err32
        # labels: every fourth user's label is one of its own returned hypotheses, the rest are random
        labels = torch.from_numpy(rng.integers(1, cfg["vocab_size"], size=(B, 4)))
        for b in range(0, B, 4) if beams >= 20 else range(0, B, 2):
            labels[b] = seq_ref[b, (3 * b) % beams, 1:5]
        half = B // 2
        batches = [dict(history=tid[sl], attention_mask=tmask[sl], target=labels[sl], prof_lvl1=prof[0][sl],
                        prof_lvl2=prof[1][sl], prof_lvl3=prof[2][sl]) for sl in (slice(0, half), slice(half, B))]
        rec, nd, got = {}, {}, None
        if beams >= 20:
            assert utils_mod is not None, f"{name}: the reference's evaluate_model could not be imported"
            got = utils_mod.evaluate_model(model, batches, TOPK, beams, "cpu")
            rec, nd = {f"Recall@{k}": [] for k in TOPK}, {f"NDCG@{k}": [] for k in TOPK}
            for bt, sl in zip(batches, (slice(0, half), slice(half, B))):
                r, n = tiger_ref.metrics(tiger_ref.pos_index(seq_ref[sl][:, :, 1:5], bt["target"]), TOPK)
                for k in r:
                    rec[k].append(r[k])
                for k in n:
                    nd[k].append(n[k])
            rec = {k: sum(v) / len(v) for k, v in rec.items()}
            nd = {k: sum(v) / len(v) for k, v in nd.items()}
            assert got[0] == rec and got[1] == nd, f"{name}: restated metrics differ from the reference's"
            print(f"{name}: metrics {rec} {nd}")

    import transformers
    meta = dict(name=name, config=cfg_full, num_beams=beams, max_length=T, n_vec=n_vec, keys=keys, tied=base.TIED,
                topk_list=TOPK, m=m, score_err32=score_err, prefix_err32=prefix_err32, enc_err32=enc_err32,
                logit_err32=logit_err32, recall=rec, ndcg=nd, enc_users=min(ENC_USERS, B), torch=torch.__version__,
                use_cache=use_cache, reference_metrics_ran=got is not None, early_stopped=early,
                prefix_changed_users=changed, masked_mean_moves_user0=moved, transformers=transformers.__version__)
    out = {"meta": np.array(json.dumps(meta)), "input_ids": ids, "attention_mask": mask,
           "prof_lvl1": prof[0].numpy(), "prof_lvl2": prof[1].numpy(), "prof_lvl3": prof[2].numpy(),
           "labels": labels.numpy(), "sequences": seq_ref.numpy(), "sequences_scores": sc_ref.numpy(),
           "prefix": prefix_ref.numpy(), "encoder_output": enc_ref[:ENC_USERS].numpy(), "sequences64": s64.numpy(),
           "scores64": c64.numpy(), "gaps": tr64["gaps"].numpy(), "certified": certified.numpy(),
           "stopped_after": stopped.numpy()}
    for k, v in sd32.items():
        if k not in base.TIED:
            out["sd/" + k] = v.numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{name}: wrote {size} bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    model_mod, utils_mod = load_reference(sys.argv[1])
    for nm in (sys.argv[2:] or FIXTURES):
        make(nm, model_mod, utils_mod)
