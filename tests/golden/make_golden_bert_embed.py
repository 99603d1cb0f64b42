"""Fixtures of the BERT encoder pass: ``transformers``' ``BertModel`` (built from a config, nothing downloaded; eager
attention, eval mode, float32, CPU) on seeded bf16-representable weights.

    python tests/golden/make_golden_bert_embed.py        ->  tests/golden/bert_embed_{main,types,h64}.npz

Each file holds the config, the state dict (``sd/<BertModel key>``), ``input_ids``, ``attention_mask``,
``token_type_ids``, HF's ``last_hidden_state`` and the two poolings of the reference computed on it (``hf_hidden``,
``hf_mean_no_cls``, ``hf_cls``), the float64 restatement's (``hidden64``, ``mean_no_cls64``, ``cls64``), and in meta
``hidden_err32`` / ``pooled_err32`` / ``cls_err32``: the float32 restatement's worst distance from its float64 run,
relative to the tensor's largest magnitude over live rows; ``hf_*_err``: HF's own distance from the float64 run; and
``keys``: HF's state-dict keys and shapes.

Before writing, the generator asserts that the float32 restatement equals HF within 1e-5 and that a mean which
includes the [CLS] row lies more than 100 x pooled_err32 from the reference pooling, so the tests can tell them apart.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bert_embed_ref as ref  # noqa: E402

COMMON = dict(vocab_size=48, type_vocab_size=2, hidden_act="gelu", layer_norm_eps=1e-12, pad_token_id=0,
              hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
FIXTURES = {
    # right padding, no token types
    "bert_embed_main": (dict(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                             max_position_embeddings=24), [12, 1, 7, 2], 12, False, False, 11),
    # nonzero token_type_ids and a mask with holes
    "bert_embed_types": (dict(hidden_size=128, num_attention_heads=2, intermediate_size=160, num_hidden_layers=1,
                              max_position_embeddings=40), [19, 11, 5], 19, True, True, 12),
    # one head of 64, 35 positions (one 32-key tile and a tail)
    "bert_embed_h64": (dict(hidden_size=64, num_attention_heads=1, intermediate_size=96, num_hidden_layers=3,
                            max_position_embeddings=35), [35, 20, 33], 35, True, False, 13),
}


def bf16(t):
    return t.to(torch.bfloat16).float()


def make(name):
    import transformers
    delta, lengths, S, types, holes, seed = FIXTURES[name]
    cfg = dict(COMMON, **delta)
    model = transformers.BertModel(transformers.BertConfig(**cfg, attn_implementation="eager")).eval()
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        if not v.dtype.is_floating_point:
            continue
        r = torch.randn(v.shape, generator=g)
        if "LayerNorm.weight" in k:
            sd[k] = bf16(1.0 + 0.1 * r)
        elif k.endswith(".bias"):
            sd[k] = bf16(0.1 * r)
        elif "embeddings." in k:
            sd[k] = bf16(r)
        else:
            sd[k] = bf16(r * v.shape[1] ** -0.5)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(not model.state_dict()[k].dtype.is_floating_point for k in missing), (missing, unexpected)
    keys = [[k, list(v.shape)] for k, v in model.state_dict().items() if v.dtype.is_floating_point]
    assert keys == ref.state_keys(cfg), "BertModel's parameter tree is not the restatement's"

    B = len(lengths)
    ids = torch.randint(1, cfg["vocab_size"], (B, S), generator=g)
    mask = torch.zeros(B, S, dtype=torch.int64)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    if holes:
        mask[0, 3] = 0
        mask[0, 9:12] = 0
        mask[1, 0] = 0
    ids[mask == 0] = 0
    tt = torch.zeros(B, S, dtype=torch.int64)
    if types:
        for b, n in enumerate(lengths):
            tt[b, (n + 1) // 2:n] = 1
    with torch.no_grad():
        hf = model(input_ids=ids, attention_mask=mask, token_type_ids=tt).last_hidden_state
    hf_run = dict(hidden=hf, mean_no_cls=ref.pool(hf, mask, "mean_no_cls"), cls=ref.pool(hf, mask, "cls"))
    r64 = ref.run(cfg, sd, ids, mask, tt, torch.float64)
    r32 = ref.run(cfg, sd, ids, mask, tt, torch.float32)
    err = ref.measure(r32, r64, mask)
    hf_err = {"hf_" + k[:-2]: v for k, v in ref.measure(hf_run, r64, mask).items()}       # hf_hidden_err, ...
    agree = ref.live_err(r32["hidden"], hf, mask)
    assert agree <= 1e-5, f"{name}: the float32 restatement is {agree:.3e} from HF"
    with_cls = ref.pool(r64["hidden"], mask, "mean_with_cls")
    apart = ref.live_err(with_cls, r64["mean_no_cls"])
    assert apart > 100 * err["pooled_err32"], (name, apart, err["pooled_err32"])
    meta = dict(name=name, config=cfg, keys=keys, seed=seed, transformers=transformers.__version__,
                restatement_vs_hf=agree, mean_with_cls_distance=apart, **err, **hf_err)
    arrays = {"sd/" + k: v.numpy() for k, v in sd.items()}
    arrays.update(input_ids=ids.numpy(), attention_mask=mask.numpy(), token_type_ids=tt.numpy(), hf_hidden=hf.numpy(),
                  hf_mean_no_cls=hf_run["mean_no_cls"].numpy(), hf_cls=hf_run["cls"].numpy(),
                  hidden64=r64["hidden"].numpy(), mean_no_cls64=r64["mean_no_cls"].numpy(), cls64=r64["cls"].numpy())
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (name, size)
    print(f"{name}: {size} bytes, restatement vs HF {agree:.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in {**err, **hf_err}.items()))


if __name__ == "__main__":
    for fixture in FIXTURES:
        make(fixture)
