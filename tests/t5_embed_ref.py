"""Plain-torch restatement of the T5 embedding retriever's forward (the math of include/gr_amd.h's
gr_t5_embed_f32 section), dtype-generic: float32 stands for the reference, float64 is the yardstick the
GPU tests compare against.

    x = seq . in_w^T + in_b
    per block:  x += o(softmax(q k^T + bias + mask) v) on rms(x);  x += wo(relu(wi(rms(x))))
    hidden = rms_final(x);  pooled = sum_j m_j hidden_j / max(sum_j m_j, 1e-9)
    pred = pooled . out_w^T + out_b;  pred_norm = pred / max(|pred|, 1e-8)

with rms(x) = w * (x * rsqrt(mean(x^2) + eps)), no 1/sqrt(d_kv) scale, bias[h, i, j] = rel[bucket(j - i), h]
from block 0's table (32 bidirectional buckets, max distance 128) and a masked key removed by adding the
dtype's most negative number.  The attention step is written with torch's fused
``scaled_dot_product_attention`` (scale 1, additive bias + mask): in float32 that is bit for bit what the
reference computes under transformers 5.15, where the unfused softmax(...) @ v differs from it by rounding
(3.7e-6 of the scale on the peaked fixture, whose float32 noise against float64 is 6e-6).  ``variant`` builds the two wrong models the fixture generator separates
from the right one: "scaled" (scores / sqrt(d_kv)) and "flipped" (bias from query - key).
"""
import math

import torch

NUM_BUCKETS, MAX_DISTANCE = 32, 128


def bucket(rel):
    """Bucket of key position - query position (int64 tensor), bidirectional.  Half of the buckets for each
    sign; within a half the first 8 distances have a bucket each and the rest are spaced logarithmically
    up to the maximum distance.  The logarithm is taken in float32 and truncated, which is what defines
    the bucket of a distance that sits on a boundary (16, 32, 64)."""
    half = NUM_BUCKETS // 2
    exact = half // 2
    n = rel.abs()
    far = exact + (torch.log(n.float() / exact) / math.log(MAX_DISTANCE / exact) * (half - exact)).to(torch.long)
    far = torch.clamp(far, max=half - 1)
    return (rel > 0).to(torch.long) * half + torch.where(n < exact, n, far)


def rms(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def forward(cfg, sd, seq_embs, attention_mask=None, dtype=torch.float64, variant=None):
    """-> (pred_norm [B, out], hidden [B, S, d_model], pred [B, out]) in ``dtype``.  ``sd``: the reference's names
    (``input_proj.weight``, ``model.encoder.block.0.layer.0.SelfAttention.q.weight``, ...)."""
    p = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point() and v.dim() and v.shape[0] != 32128}
    H, dkv, eps = int(cfg["num_heads"]), int(cfg["d_kv"]), float(cfg.get("layer_norm_epsilon", 1e-6))
    x = seq_embs.to(dtype) @ p["input_proj.weight"].T + p["input_proj.bias"]
    B, S, _ = x.shape
    m = torch.ones(B, S, dtype=dtype, device=x.device) if attention_mask is None else attention_mask.to(dtype)
    pos = torch.arange(S, device=x.device)
    rel = pos[None, :] - pos[:, None]                       # [query i, key j] = j - i
    if variant == "flipped":
        rel = -rel
    table = p["model.encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
    bias = table[bucket(rel)].permute(2, 0, 1)              # [H, S, S]
    keymask = (1.0 - m)[:, None, None, :] * torch.finfo(dtype).min
    for l in range(int(cfg["num_layers"])):
        pre = f"model.encoder.block.{l}.layer."
        h = rms(x, p[pre + "0.layer_norm.weight"], eps)
        q, k, v = (( h @ p[pre + f"0.SelfAttention.{n}.weight"].T).view(B, S, H, dkv).transpose(1, 2) for n in "qkv")
        # softmax(scale * q k^T + (bias + mask)) v, in the fused form torch evaluates it in
        a = torch.nn.functional.scaled_dot_product_attention(
            q, k, v, attn_mask=bias + keymask, scale=1.0 / math.sqrt(dkv) if variant == "scaled" else 1.0)
        x = x + a.transpose(1, 2).reshape(B, S, H * dkv) @ p[pre + "0.SelfAttention.o.weight"].T
        h = rms(x, p[pre + "1.layer_norm.weight"], eps)
        x = x + torch.relu(h @ p[pre + "1.DenseReluDense.wi.weight"].T) @ p[pre + "1.DenseReluDense.wo.weight"].T
    hidden = rms(x, p["model.encoder.final_layer_norm.weight"], eps)
    pooled = (hidden * m[..., None]).sum(1) / m.sum(1, keepdim=True).clamp(min=1e-9)
    pred = pooled @ p["output_proj.weight"].T + p["output_proj.bias"]
    return pred / pred.norm(dim=1, keepdim=True).clamp(min=1e-8), hidden, pred


def unit(x, eps=1e-12):
    return x / x.norm(dim=1, keepdim=True).clamp(min=eps)


def info_nce(pred, target, temperature, eps=1e-8):
    """Symmetric in-batch InfoNCE on unit vectors."""
    logits = unit(pred, eps) @ unit(target.to(pred.dtype), eps).T / temperature
    n = torch.arange(logits.shape[0])
    ls = torch.log_softmax(logits, dim=1)[n, n].mean() + torch.log_softmax(logits.T, dim=1)[n, n].mean()
    return -ls / 2.0


def scores(pred_norm, item_embs):
    """Cosine scores of the (re-normalised) predictions against the normalised catalog."""
    return unit(pred_norm) @ unit(item_embs.to(pred_norm.dtype)).T


def metrics(topk_idx, target_id, topk_list):
    """Recall@k, NDCG@k of one batch (float32 means, as the reference takes them)."""
    out = {}
    hit = topk_idx == target_id[:, None]
    for k in topk_list:
        out[f"Recall@{k}"] = hit[:, :k].any(1).float().mean().item()
        out[f"NDCG@{k}"] = (hit[:, :k].float() / torch.log2(torch.arange(1, k + 1) + 1)).sum(1).mean().item()
    return out


def live_err(a, b64, mask=None):
    """Worst |a - b64| relative to b64's largest magnitude, over live rows when a mask is given."""
    a, b64 = a.double(), b64.double()
    if mask is not None:
        a, b64 = a[mask.bool()], b64[mask.bool()]
    return ((a - b64).abs().max() / b64.abs().max()).item()
