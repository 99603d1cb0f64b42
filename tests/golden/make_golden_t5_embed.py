"""Fixtures for the T5 embedding retriever tests: the reference's own ``TIGER`` (T5/model.py, imported at run
time from a checkout of the reference; needs ``transformers``, constructs from a config, no download) on
seeded models and sequences, next to the plain-torch restatement tests/t5_embed_ref.py in float32 and float64.

    python tests/golden/make_golden_t5_embed.py <reference checkout>   ->  tests/golden/t5e_*.npz

Each file holds the config, the reference's state-dict key list with shapes, the weights the forward uses
(the tied [32128, d_model] token table is stored as its shape alone: the forward never reads it), the
inputs and masks, the reference's float32 ``pred`` and ``last_hidden_state``, the float64 restatement's, and
in ``meta`` the float32 reference's worst distance from float64 relative to the tensor's largest magnitude
over live rows (``pred_err32``, ``hidden_err32``): the GPU tests allow four times that.

The weights are the library's seeded initialisation rounded to bf16-representable float32 values (the
compressed file stays under 1 MiB; asserted).  The reference's constructor never passes ``num_layers``, so
every fixture has T5Config's six blocks and the fixtures are narrow instead.  Before a file is written the
generator asserts: restatement == reference in float32 within 1e-6 of the scale on ``pred`` and on the
live rows of ``hidden``; and that a restatement with the 1/sqrt(d_kv) scale added, and one whose bias
uses query - key, each move ``pred`` by more than 100 x ``pred_err32`` -- so a test at 4 x tells them apart.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import t5_embed_ref as ref  # noqa: E402

TABLE = "model.shared.weight", "model.encoder.embed_tokens.weight"

FIXTURES = {
    #  name          params                                                                       B   S  seed peaked
    "t5e_main":   (dict(d_model=64, num_heads=2, d_kv=16, d_ff=96, input_emb_dim=48, target_emb_dim=40), 16, 21, 31, False),
    "t5e_h3":     (dict(d_model=96, num_heads=3, d_kv=8, d_ff=160, input_emb_dim=32, target_emb_dim=64), 8, 32, 32, False),
    "t5e_peaked": (dict(d_model=64, num_heads=2, d_kv=16, d_ff=96, input_emb_dim=48, target_emb_dim=40), 16, 21, 33, True),
}
QK_SCALE = 4.0       # t5e_peaked: q and k rows x 4, so the scores spread the softmax
HOLES = {2: [1, 4, 5], 5: [0, 7]}     # t5e_peaked: user -> positions switched off inside its length


def load_reference(ref_dir):
    spec = importlib.util.spec_from_file_location("t5_embed_reference_model", os.path.join(ref_dir, "T5", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.TIGER


def sequences(B, S, dim, rng, peaked):
    """Right-padded [user vector, items...] sequences: user 0 is full, user 1 has one position."""
    seq = np.zeros((B, S, dim), np.float32)
    mask = np.zeros((B, S), np.int64)
    for b in range(B):
        n = S if b == 0 else 1 if b == 1 else int(rng.integers(1, S + 1))
        if peaked and b in HOLES:
            n = max(n, 10)
        seq[b, :n] = 0.5 * rng.standard_normal((n, dim)).astype(np.float32)
        mask[b, :n] = 1
        if peaked and b in HOLES:
            mask[b, HOLES[b]] = 0        # the vectors stay: a masked position may hold anything
    return seq, mask


def make(name, TIGER):
    params, B, S, seed, peaked = FIXTURES[name]
    params = dict(params, dropout_rate=0.1, num_layers=2, temperature=0.07)    # num_layers: ignored, as deployed
    torch.manual_seed(seed)
    model = TIGER(params).eval()
    t5cfg = model.model.config
    with torch.no_grad():
        if peaked:
            rel = model.model.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
            rel.mul_(1.0 / rel.abs().max())                   # O(1) biases
            for blk in model.model.encoder.block:
                blk.layer[0].SelfAttention.q.weight.mul_(QK_SCALE)
                blk.layer[0].SelfAttention.k.weight.mul_(QK_SCALE)
        for p in model.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    cfg = dict(d_model=int(t5cfg.d_model), d_kv=int(t5cfg.d_kv), num_heads=int(t5cfg.num_heads), d_ff=int(t5cfg.d_ff),
               num_layers=int(t5cfg.num_layers), input_emb_dim=params["input_emb_dim"],
               target_emb_dim=params["target_emb_dim"], layer_norm_epsilon=float(t5cfg.layer_norm_epsilon),
               feed_forward_proj=str(t5cfg.feed_forward_proj), temperature=params["temperature"],
               relative_attention_num_buckets=int(t5cfg.relative_attention_num_buckets),
               relative_attention_max_distance=int(t5cfg.relative_attention_max_distance))
    assert cfg["num_layers"] == 6 and cfg["relative_attention_num_buckets"] == 32
    assert cfg["relative_attention_max_distance"] == 128 and cfg["feed_forward_proj"] == "relu"
    full_sd = model.state_dict()
    keys = [[k, list(v.shape)] for k, v in full_sd.items()]
    assert torch.equal(full_sd[TABLE[0]], full_sd[TABLE[1]])
    sd = {k: v.detach().clone() for k, v in full_sd.items() if k not in TABLE}

    rng = np.random.default_rng(seed)
    seq, mask = sequences(B, S, params["input_emb_dim"], rng, peaked)
    target = rng.standard_normal((B, params["target_emb_dim"])).astype(np.float32)
    tseq, tmask = torch.from_numpy(seq), torch.from_numpy(mask)
    live = tmask.bool()
    with torch.no_grad():
        loss_ref, pred_ref = model(tseq, tmask, torch.from_numpy(target))
        hid_ref = model.model(inputs_embeds=model.input_proj(tseq), attention_mask=tmask).last_hidden_state
        p32, h32, _ = ref.forward(cfg, sd, tseq, tmask, torch.float32)
        p64, h64, _ = ref.forward(cfg, sd, tseq, tmask, torch.float64)
        d = ref.live_err(p32, pred_ref)
        assert d <= 1e-6, f"{name}: float32 restatement's pred differs from the reference by {d}"
        d = ref.live_err(h32, hid_ref, tmask)
        assert d <= 1e-6, f"{name}: float32 restatement's hidden differs from the reference by {d}"
        l32 = ref.info_nce(p32, torch.from_numpy(target), params["temperature"]).item()
        assert abs(l32 - loss_ref.item()) <= 1e-5 * abs(loss_ref.item()), (l32, loss_ref.item())
        pred_err32 = ref.live_err(pred_ref, p64)
        hidden_err32 = ref.live_err(hid_ref, h64, tmask)
        moved = {}
        for variant in ("scaled", "flipped"):
            pv, _, _ = ref.forward(cfg, sd, tseq, tmask, torch.float64, variant=variant)
            moved[variant] = ref.live_err(pv, p64)
            assert moved[variant] > 100 * pred_err32, \
                f"{name}: the {variant} model moves pred by {moved[variant]:.3e}, pred_err32 is {pred_err32:.3e}"
        # padding is inert in the reference: random finite values in the masked positions change nothing
        noisy = tseq.clone()
        noisy[~live] = 5.0 * torch.from_numpy(rng.standard_normal((int((~live).sum()), seq.shape[-1])).astype(np.float32))
        zeroed = tseq.clone()
        zeroed[~live] = 0.0
        inert = (model(noisy, tmask)[1] - model(zeroed, tmask)[1]).abs().max().item()
    print(f"{name}: B {B} S {S}  pred_err32 {pred_err32:.3e} hidden_err32 {hidden_err32:.3e}  scaled moves pred "
          f"{moved['scaled']:.3e}, flipped {moved['flipped']:.3e}; padding noise moves the reference by {inert}")
    assert inert == 0.0

    meta = dict(name=name, config=cfg, params=params, keys=keys, table=list(TABLE), pred_err32=pred_err32,
                hidden_err32=hidden_err32, moved=moved, loss=loss_ref.item(), torch=torch.__version__)
    try:
        import transformers
        meta["transformers"] = transformers.__version__
    except ImportError:
        pass
    out = {"meta": np.array(json.dumps(meta)), "seq_embs": seq, "attention_mask": mask, "target_emb": target,
           "pred": pred_ref.numpy(), "hidden": hid_ref.numpy(), "pred64": p64.numpy(), "hidden64": h64.numpy()}
    for k, v in sd.items():
        out["sd/" + k] = v.numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{name}: wrote {size} bytes, {len(keys)} keys")
    assert size < (1 << 20)


if __name__ == "__main__":
    cls = load_reference(sys.argv[1])
    for nm in (sys.argv[2:] or FIXTURES):
        make(nm, cls)
