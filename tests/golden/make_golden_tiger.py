"""Fixtures for the TIGER tests: the reference's own ``TIGER`` (RQVAE-T5/model.py, imported at run time
from a checkout of the reference; needs ``transformers``) on seeded models and histories, next to
the plain-torch restatement tests/tiger_ref.py in float32 and float64.

    python tests/golden/make_golden_tiger.py <reference checkout>   ->  tests/golden/tiger_*.npz

Each file holds the config, the state dict (tied entries stored once, see ``meta["tied"]``), the
inputs, the reference's float32 sequences / scores (and its encoder output for the first users),
the float64 restatement's sequences and scores, the per-user selection gaps and the certification
margin, the float32 distances from float64 that set the GPU tolerances, and the reference's metrics.
The per-step float64 logits are a function of the stored state dict and inputs; the tests recompute
them with the restatement instead of storing them (a file must stay under 1 MiB).

The weights are the library's seeded initialisation rounded to bf16-representable float32 values, so
that the compressed state dict of the main config (234k parameters) fits the size limit.  Before a
file is written the generator asserts: restatement == reference in float32 (sequences on every
user, scores within 1e-6), at least 90 % of the users certified, for the EOS fixture that moving
the EOS id to an unused token changes the returned set for at least a quarter of the users, and for
the early-stop fixture that at least a quarter of the users satisfy the stop heuristic before the last
step (and at least one does not, or the library would crop its result).
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tiger_ref  # noqa: E402

MAIN = dict(vocab_size=64, num_layers=2, num_decoder_layers=2, d_model=64, d_ff=256, num_heads=4, d_kv=16,
            dropout_rate=0.1, feed_forward_proj="relu", pad_token_id=0, eos_token_id=31, codebook_size=8,
            max_len=20)
TOPK = [2, 5, 10, 20]
ENC_USERS = 8            # users whose reference encoder output is stored

FIXTURES = {
    #  name            config changes                                               B   beams seed eos-scale
    "tiger_main":     (dict(),                                                       32, 20, 11, None),
    "tiger_eos":      (dict(eos_token_id=11),                                        32, 20, 12, 3.0),
    "tiger_h2_ff128": (dict(num_heads=2, d_kv=32, d_ff=128, num_layers=1, num_decoder_layers=3), 16, 20, 13, None),
    "tiger_v40_len3": (dict(vocab_size=40, max_len=3),                               16, 20, 14, None),
    "tiger_d32_b5":   (dict(d_model=32, num_heads=4, d_kv=8),                        16, 5, 15, None),
    # early stop exercised: 5 beams and an EOS that is likely in every context (EOS_PULL below)
    "tiger_stop":     (dict(eos_token_id=40),                                        32, 5, 18, "pull"),
}
# The "pull" model: a seeded T5 predicts its own input token (tied embeddings), so scaling the EOS row
# makes EOS likely in some contexts only.  Here row 0 of the last decoder block's wo is made positive
# (|wo[0]| * 3), which adds a positive amount to residual feature 0 after the ReLU in every context; the
# EOS row's feature 0 is set to 10, and the decoder's final norm weight is halved (the logits and their
# float32 noise halve, so the scores stay comparable within 1e-6).  Most users then fill all their
# finished slots at step 2 or 3 and stop; the generator asserts the share.
EOS_PULL = dict(wo_scale=3.0, eos_feature=10.0, final_norm=0.5)
TIED = ["encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight"]


def load_reference(ref_dir):
    spec = importlib.util.spec_from_file_location("tiger_reference_model", os.path.join(ref_dir, "RQVAE-T5", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.TIGER


def histories(cfg, B, rng):
    """Left-padded token histories: 1..max_len items of 4 codes, token = c + level * codebook + 1.  User 0
    has a single item, user 1 all max_len."""
    cb, max_len = cfg["codebook_size"], cfg["max_len"]
    S = 4 * max_len
    ids = np.zeros((B, S), np.int64)
    mask = np.zeros((B, S), np.int64)
    for b in range(B):
        n = 1 if b == 0 else max_len if b == 1 else int(rng.integers(1, max_len + 1))
        codes = rng.integers(0, cb, size=(n, 4))
        toks = (codes + np.arange(4)[None, :] * cb + 1).reshape(-1)
        ids[b, S - toks.size:] = toks
        mask[b, S - toks.size:] = 1
    return ids, mask


def ref_generate(model, ids, mask, beams):
    # The library sizes its key/value cache by the encoder's layer count and fails (IndexError) on a
    # deeper decoder; there the reference runs without the cache, which changes no result.
    if model.model.config.num_decoder_layers > model.model.config.num_layers:
        model.model.generation_config.use_cache = False
    out = model.generate(torch.from_numpy(ids), torch.from_numpy(mask), num_beams=beams,
                         return_dict_in_generate=True, output_scores=True)
    return out.sequences, out.sequences_scores


def ref_metrics(ref_dir, model, batches, beams):
    """The reference's evaluate_model when its imports (matplotlib, tqdm) are there, else None."""
    try:
        spec = importlib.util.spec_from_file_location("tiger_reference_utils", os.path.join(ref_dir, "RQVAE-T5", "utils.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    except ImportError:
        return None
    return mod.evaluate_model(model, batches, TOPK, beams, "cpu")


def make(name, ref_dir, TIGER):
    delta, B, beams, seed, eos_scale = FIXTURES[name]
    cfg = dict(MAIN, **delta)
    torch.manual_seed(seed)
    model = TIGER(cfg).eval()
    with torch.no_grad():
        if eos_scale == "pull":
            wo = model.model.decoder.block[-1].layer[-1].DenseReluDense.wo.weight
            wo[0] = wo[0].abs() * EOS_PULL["wo_scale"]
            model.model.shared.weight[cfg["eos_token_id"], 0] = EOS_PULL["eos_feature"]
            model.model.decoder.final_layer_norm.weight.mul_(EOS_PULL["final_norm"])
        for p in model.parameters():
            p.copy_(p.to(torch.bfloat16).float())
        if eos_scale not in (None, "pull"):
            model.model.shared.weight[cfg["eos_token_id"]] *= eos_scale
    t5cfg = model.model.config
    cfg_full = dict(cfg, layer_norm_epsilon=float(t5cfg.layer_norm_epsilon),
                    relative_attention_num_buckets=int(t5cfg.relative_attention_num_buckets),
                    relative_attention_max_distance=int(t5cfg.relative_attention_max_distance),
                    scale_decoder_outputs=bool(getattr(t5cfg, "scale_decoder_outputs", True)))
    assert cfg_full["relative_attention_num_buckets"] == 32 and cfg_full["relative_attention_max_distance"] == 128
    full_sd = model.state_dict()
    keys = [[k, list(v.shape)] for k, v in full_sd.items()]
    sd32 = {k[len("model."):]: v.detach().clone() for k, v in full_sd.items()}
    for k in TIED:
        assert torch.equal(sd32[k], sd32["shared.weight"])
    sd64 = {k: v.double() for k, v in sd32.items()}

    use_cache = cfg["num_decoder_layers"] <= cfg["num_layers"]     # see ref_generate
    rng = np.random.default_rng(seed)
    ids, mask = histories(cfg, B, rng)
    tid, tmask = torch.from_numpy(ids), torch.from_numpy(mask)
    T = 5
    with torch.no_grad():
        seq_ref, sc_ref = ref_generate(model, ids, mask, beams)
        enc_ref = model.model.encoder(input_ids=tid, attention_mask=tmask).last_hidden_state
        assert seq_ref.shape[1] == T, f"{name}: the reference cropped its result to {seq_ref.shape[1]} columns"
        seq_ref, sc_ref = seq_ref.view(B, beams, T), sc_ref.view(B, beams)
        # float32 restatement == reference
        tr32 = {}
        s32, c32, width = tiger_ref.beam_search(cfg_full, sd32, tid, tmask, beams, T, trace=tr32, use_cache=use_cache)
        assert width == T
        bad = [b for b in range(B) if not torch.equal(s32[b], seq_ref[b])]
        assert not bad, f"{name}: float32 restatement != reference on users {bad}"
        d = (c32 - sc_ref).abs().max().item()
        assert d <= 1e-6, f"{name}: float32 restatement scores differ from the reference by {d}"
        live = tmask.bool()
        d = (tr32["enc"] - enc_ref)[live].abs().max().item()
        assert d <= 1e-5, f"{name}: encoder restatement differs from the reference by {d}"
        # float64 restatement, margins, tolerances
        tr64 = {}
        s64, c64, _ = tiger_ref.beam_search(cfg_full, sd64, tid, tmask, beams, T, trace=tr64, use_cache=use_cache)
        same = torch.tensor([torch.equal(s64[b], seq_ref[b]) for b in range(B)])
        score_err = (sc_ref.double() - c64)[same].abs().max().item()
        m = 4.0 * score_err
        certified = tr64["gaps"] > m
        share = certified.float().mean().item()
        enc_err32 = ((enc_ref.double() - tr64["enc"])[live].abs().max() / tr64["enc"][live].abs().max()).item()
        logit_err32 = 0.0
        stopped = tr64["stopped_after"]
        assert torch.equal(stopped, tr32["stopped_after"])
        for t, (l32, l64) in enumerate(zip(tr32["logits"], tr64["logits"])):
            on = same & ((stopped < 0) | (stopped > t))        # a stopped user's later steps are not compared
            e = (l32.double() - l64)[on].abs().amax(-1) / l64[on].abs().amax(-1)
            logit_err32 = max(logit_err32, e.max().item())
        early = int(((stopped > 0) & (stopped < T - 1)).sum())
        print(f"{name}: {early}/{B} users stop before the last step (after steps {sorted(set(stopped.tolist()))})")
        if eos_scale == "pull":
            assert early * 4 >= B, f"{name}: only {early} of {B} users stop early"
            assert int((stopped == T - 1).sum()) >= 1, f"{name}: every user stops early, the library would crop"
        print(f"{name}: B {B} beams {beams}  ref==fp64 on {int(same.sum())}/{B} users, score err {score_err:.3e}, "
              f"m {m:.3e}, certified {int(certified.sum())}/{B}, min gap {tr64['gaps'].min().item():.3e}, "
              f"enc err32 {enc_err32:.3e}, logit err32 {logit_err32:.3e}")
        assert share >= 0.9, f"{name}: only {share:.2f} of the users certified"
        for b in range(B):
            if certified[b]:
                assert torch.equal(s64[b], seq_ref[b]), f"{name}: certified user {b} differs between fp32 and fp64"
        eos = cfg["eos_token_id"]
        after = 0
        for row in seq_ref.view(-1, T).tolist():
            if eos in row[1:]:
                p = row.index(eos, 1)
                after += any(t != cfg["pad_token_id"] for t in row[p + 1:])
        print(f"{name}: {after} of {B * beams} hypotheses hold non-pad tokens after an EOS")
        if eos_scale not in (None, "pull"):
            unused = cfg["vocab_size"] - 1
            alt, _, _ = tiger_ref.beam_search(dict(cfg_full, eos_token_id=unused), sd32, tid, tmask, beams, T)
            changed = sum(set(map(tuple, alt[b].tolist())) != set(map(tuple, s32[b].tolist())) for b in range(B))
            print(f"{name}: moving EOS to token {unused} changes the returned set for {changed}/{B} users")
            assert changed * 4 >= B and after > 0
        # labels: every fourth user's label is one of its own returned hypotheses, the rest are random
        labels = torch.from_numpy(rng.integers(1, cfg["vocab_size"], size=(B, 4)))
        for b in range(0, B, 4) if beams >= 20 else range(0, B, 2):
            labels[b] = seq_ref[b, (3 * b) % beams, 1:5] if T >= 5 else labels[b]
        half = B // 2
        batches = [dict(history=tid[:half], attention_mask=tmask[:half], target=labels[:half]),
                   dict(history=tid[half:], attention_mask=tmask[half:], target=labels[half:])]
        got = ref_metrics(ref_dir, model, batches, beams if beams >= 20 else 20) if beams >= 20 else None
        # the restated metric tail on the reference's own sequences
        rec, nd = {f"Recall@{k}": [] for k in TOPK}, {f"NDCG@{k}": [] for k in TOPK}
        if beams >= 20:
            for bt, sl in zip(batches, (slice(0, half), slice(half, B))):
                r, n = tiger_ref.metrics(tiger_ref.pos_index(seq_ref[sl][:, :, 1:5], bt["target"]), TOPK)
                for k in r:
                    rec[k].append(r[k])
                for k in n:
                    nd[k].append(n[k])
            rec = {k: sum(v) / len(v) for k, v in rec.items()}
            nd = {k: sum(v) / len(v) for k, v in nd.items()}
            assert got is not None, f"{name}: the reference's evaluate_model could not be imported"
            if got is not None:
                assert got[0] == rec and got[1] == nd, f"{name}: restated metrics differ from the reference's"
            print(f"{name}: metrics {rec} {nd} (reference's evaluate_model ran: {got is not None})")
        else:
            rec, nd = {}, {}

    meta = dict(name=name, config=cfg_full, num_beams=beams, max_length=T, keys=keys, tied=TIED, topk_list=TOPK,
                m=m, score_err32=score_err, enc_err32=enc_err32, logit_err32=logit_err32,
                recall=rec, ndcg=nd, enc_users=min(ENC_USERS, B), torch=torch.__version__,
                use_cache=use_cache, reference_metrics_ran=got is not None, early_stopped=early)
    try:
        import transformers
        meta["transformers"] = transformers.__version__
    except ImportError:
        pass
    out = {"meta": np.array(json.dumps(meta)), "input_ids": ids, "attention_mask": mask,
           "labels": labels.numpy(), "sequences": seq_ref.numpy(), "sequences_scores": sc_ref.numpy(),
           "encoder_output": enc_ref[:ENC_USERS].numpy(), "sequences64": s64.numpy(), "scores64": c64.numpy(),
           "gaps": tr64["gaps"].numpy(), "certified": certified.numpy(), "stopped_after": stopped.numpy()}
    for k, v in sd32.items():
        if k not in TIED:
            out["sd/" + k] = v.numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{name}: wrote {size} bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    ref = sys.argv[1]
    cls = load_reference(ref)
    for nm in (sys.argv[2:] or FIXTURES):
        make(nm, ref, cls)
