"""Plain-torch restatement of the BERT encoder pass (``transformers``' ``BertModel`` in eval mode, eager attention,
absolute positions) and of the reference's two poolings, generic in dtype: the float64 run is the oracle of the
BERT tests, the float32 run measures what float32 can give on the same inputs.  Imports neither ``transformers``
nor the reference.

    embeddings   LayerNorm((word[ids] + token_type[type_ids]) + position[0..S-1]); type_ids None means zeros
    per layer    q/k/v with bias; per head softmax(q k^T / sqrt(head_dim)) over the live keys (a masked key has
                 probability exactly 0: what HF's additive finfo.min gives whenever a live key exists);
                 LayerNorm(x + dense(context)); LayerNorm(x + output.dense(gelu(intermediate.dense(x)))), exact-erf gelu
    LayerNorm    biased variance of the centred row, eps inside the square root
    no live key  the sequence's hidden rows are zeros
    mean_no_cls  (hidden * mask)[:, 1:].sum(1) / mask[:, 1:].sum(-1).clamp(min=1e-9), mask taken as (mask != 0)
    cls          hidden[:, 0]
"""
import math

import torch

LAYER_KEYS = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
              "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm")


def state_keys(cfg):
    """[[name, shape], ...] of ``BertModel``'s state dict for ``cfg``, in its order."""
    H, I, V = int(cfg["hidden_size"]), int(cfg["intermediate_size"]), int(cfg["vocab_size"])
    keys = [["embeddings.word_embeddings.weight", [V, H]],
            ["embeddings.position_embeddings.weight", [int(cfg["max_position_embeddings"]), H]],
            ["embeddings.token_type_embeddings.weight", [int(cfg["type_vocab_size"]), H]],
            ["embeddings.LayerNorm.weight", [H]], ["embeddings.LayerNorm.bias", [H]]]
    for l in range(int(cfg["num_hidden_layers"])):
        for k in LAYER_KEYS:
            n_out, n_in = (I, H) if k == "intermediate.dense" else (H, I) if k == "output.dense" else (H, H)
            keys.append([f"encoder.layer.{l}.{k}.weight", [H] if k.endswith("LayerNorm") else [n_out, n_in]])
            keys.append([f"encoder.layer.{l}.{k}.bias", [n_out if not k.endswith("LayerNorm") else H]])
    keys += [["pooler.dense.weight", [H, H]], ["pooler.dense.bias", [H]]]
    return keys


def layer_norm(x, w, b, eps):
    d = x - x.mean(-1, keepdim=True)
    var = (d * d).mean(-1, keepdim=True)
    return d / torch.sqrt(var + eps) * w + b


def gelu(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def forward(cfg, sd, ids, mask=None, type_ids=None, dtype=torch.float64):
    """-> last hidden state [B, S, H] in ``dtype``."""
    H, nh = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    hd, eps = H // nh, float(cfg.get("layer_norm_eps", 1e-12))
    B, S = ids.shape

    def w(k):
        return sd[k].to(dtype)
    tt = torch.zeros_like(ids) if type_ids is None else type_ids
    live = torch.ones(B, S, dtype=torch.bool) if mask is None else mask != 0
    x = (w("embeddings.word_embeddings.weight")[ids] + w("embeddings.token_type_embeddings.weight")[tt]) \
        + w("embeddings.position_embeddings.weight")[:S]
    x = layer_norm(x, w("embeddings.LayerNorm.weight"), w("embeddings.LayerNorm.bias"), eps)
    for l in range(int(cfg["num_hidden_layers"])):
        p = f"encoder.layer.{l}."

        def lin(t, k):
            return t @ w(p + k + ".weight").T + w(p + k + ".bias")

        def heads(t):
            return t.view(B, S, nh, hd).transpose(1, 2)
        q, k, v = (heads(lin(x, "attention.self." + n)) for n in ("query", "key", "value"))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
        s = s.masked_fill(~live[:, None, None, :], float("-inf"))
        pr = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)          # a sequence with no live key: zeros
        ctx = (pr @ v).transpose(1, 2).reshape(B, S, H)
        x = layer_norm(x + lin(ctx, "attention.output.dense"), w(p + "attention.output.LayerNorm.weight"),
                       w(p + "attention.output.LayerNorm.bias"), eps)
        f = gelu(lin(x, "intermediate.dense"))
        x = layer_norm(x + lin(f, "output.dense"), w(p + "output.LayerNorm.weight"), w(p + "output.LayerNorm.bias"), eps)
    return x * live.any(dim=1)[:, None, None].to(dtype)


def pool(hidden, mask, pooling):
    """``"mean_no_cls"`` / ``"cls"`` / ``"mean_with_cls"`` (the pooling the reference does NOT use: the tests show
    that they can tell it apart)."""
    B, S, _ = hidden.shape
    m = torch.ones(B, S, dtype=hidden.dtype) if mask is None else (mask != 0).to(hidden.dtype)
    if pooling == "cls":
        return hidden[:, 0]
    first = 1 if pooling == "mean_no_cls" else 0
    return (hidden * m[:, :, None])[:, first:].sum(1) / m[:, first:].sum(-1, keepdim=True).clamp(min=1e-9)


def run(cfg, sd, ids, mask, type_ids, dtype):
    """-> dict(hidden, mean_no_cls, cls) in ``dtype``."""
    with torch.no_grad():
        h = forward(cfg, sd, ids, mask, type_ids, dtype)
        return dict(hidden=h, mean_no_cls=pool(h, mask, "mean_no_cls"), cls=pool(h, mask, "cls"))


def live_err(got, want64, mask=None):
    """Worst |got - want| over the live rows, relative to want's largest magnitude over them.  ``mask`` [B, S] for
    a [B, S, H] tensor; None: every row."""
    d = (got.double() - want64.double()).abs()
    mag = want64.double().abs()
    if mask is not None:
        on = mask != 0
        d, mag = d[on], mag[on]
    return (d.max() / mag.max()).item()


def measure(r32, r64, mask):
    """The float32 run's distances from the float64 run: hidden_err32, pooled_err32 (mean_no_cls), cls_err32."""
    return dict(hidden_err32=live_err(r32["hidden"], r64["hidden"], mask),
                pooled_err32=live_err(r32["mean_no_cls"], r64["mean_no_cls"]),
                cls_err32=live_err(r32["cls"], r64["cls"]))
