"""Plain-torch restatement of the TIGER prefix variant (RQVAE-T5-prefix/model.py), in the dtype of the
state dict it is given: ``ProfessionalAdapter.forward`` in eval mode, ``_build_prefix_inputs`` and the
beam search on ``inputs_embeds``.  The T5 stack and the search are tests/tiger_ref.py's: its ``Model`` is
subclassed so that ``encode`` starts from the prefixed embeddings, and swapped in around the call.

State-dict names: the T5 entries as tiger_ref takes them (``shared.weight``, ...), the adapters as
``adapter_lvl1.bert_proj.weight``, ...
"""
import contextlib
import math

import torch

import tiger_ref

LN_EPS = 1e-5


def _layer_norm(x, w, b, eps=LN_EPS):
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).pow(2).mean(-1, keepdim=True)          # biased
    return (x - mu) / torch.sqrt(var + eps) * w + b


def adapter(sd, name, e, prof, num_heads, row_mask=None):
    """One prefix token [B, d]: e [B, S, d] token embeddings (padding included), prof [B, n, bert_dim].
    ``row_mask`` [B, S] (not the reference): the mean over the unmasked rows only."""
    w = lambda k: sd[f"{name}.{k}"]
    B, S, d = e.shape
    hd = d // num_heads
    kv = prof @ w("bert_proj.weight").T + w("bert_proj.bias")
    wq, wk, wv = w("cross_attn.in_proj_weight").split(d, 0)
    bq, bk, bv = w("cross_attn.in_proj_bias").split(d, 0)
    heads = lambda t: t.view(B, -1, num_heads, hd).transpose(1, 2)
    q = heads(e @ wq.T + bq) * math.sqrt(1.0 / hd)
    k, v = heads(kv @ wk.T + bk), heads(kv @ wv.T + bv)
    p = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
    ctx = (p @ v).transpose(1, 2).reshape(B, S, d)
    attn = ctx @ w("cross_attn.out_proj.weight").T + w("cross_attn.out_proj.bias")
    x = _layer_norm(e + attn, w("norm1.weight"), w("norm1.bias"))
    h = x @ w("ffn.0.weight").T + w("ffn.0.bias")
    h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    x = _layer_norm(x + h @ w("ffn.2.weight").T + w("ffn.2.bias"), w("norm2.weight"), w("norm2.bias"))
    if row_mask is not None:
        m = row_mask.to(x.dtype)[:, :, None]
        return (x * m).sum(1) / m.sum(1)
    return x.mean(1)


def prefix_tokens(cfg, sd, input_ids, prof, row_mask=None):
    """[B, 3, d]: rows 0..2 of ``_build_prefix_inputs``; prof = (prof_lvl1, prof_lvl2, prof_lvl3)."""
    dtype = sd["shared.weight"].dtype
    e = sd["shared.weight"][input_ids]
    return torch.stack([adapter(sd, f"adapter_lvl{i + 1}", e, prof[i].to(dtype), int(cfg["num_heads"]), row_mask)
                        for i in range(3)], 1)


def extend(input_ids, attention_mask):
    """Ids and mask of the S + 3 encoder positions (the three prefix ids are placeholders)."""
    B = input_ids.shape[0]
    ids = torch.cat([torch.zeros(B, 3, dtype=input_ids.dtype), input_ids], 1)
    mask = torch.cat([torch.ones(B, 3, dtype=attention_mask.dtype), attention_mask], 1)
    return ids, mask


@contextlib.contextmanager
def prefixed(prefix):
    """Inside, tiger_ref's ``Model.encode`` takes rows 0..2 of its input from ``prefix`` [B, 3, d]."""
    base = tiger_ref.Model

    class PrefixModel(base):
        def encode(self, input_ids, attention_mask):
            sd, H = self.sd, self.H
            B, S = input_ids.shape
            x = torch.cat([prefix.to(self.dtype), sd["shared.weight"][input_ids[:, 3:]]], 1)
            pos = torch.arange(S)
            bucket = tiger_ref.relative_bucket(pos[None, :] - pos[:, None], True)
            bias = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"][bucket]
            bias = bias.permute(2, 0, 1)[None]
            mask = torch.zeros(B, 1, 1, S, dtype=self.dtype)
            mask = mask.masked_fill(attention_mask[:, None, None, :] == 0, torch.finfo(self.dtype).min)
            bias = bias + mask
            for i in range(int(self.cfg["num_layers"])):
                p = f"encoder.block.{i}.layer."
                h = tiger_ref._norm(x, sd[p + "0.layer_norm.weight"], self.eps)
                q = tiger_ref._heads(h @ sd[p + "0.SelfAttention.q.weight"].T, H)
                k = tiger_ref._heads(h @ sd[p + "0.SelfAttention.k.weight"].T, H)
                v = tiger_ref._heads(h @ sd[p + "0.SelfAttention.v.weight"].T, H)
                x = x + tiger_ref._attend(q, k, v, bias) @ sd[p + "0.SelfAttention.o.weight"].T
                h = tiger_ref._norm(x, sd[p + "1.layer_norm.weight"], self.eps)
                x = x + torch.relu(h @ sd[p + "1.DenseReluDense.wi.weight"].T) @ sd[p + "1.DenseReluDense.wo.weight"].T
            return tiger_ref._norm(x, sd["encoder.final_layer_norm.weight"], self.eps)

    tiger_ref.Model = PrefixModel
    try:
        yield
    finally:
        tiger_ref.Model = base


def beam_search(cfg, sd, input_ids, attention_mask, prof, num_beams=20, max_length=5, trace=None, use_cache=True,
                row_mask=None):
    """tiger_ref.beam_search on the prefixed input -> (sequences, scores, width); ``trace`` also receives
    ``prefix`` [B, 3, d] (``enc`` then is [B, S + 3, d])."""
    prefix = prefix_tokens(cfg, sd, input_ids, prof, row_mask)
    ids, mask = extend(input_ids, attention_mask)
    with prefixed(prefix):
        out = tiger_ref.beam_search(cfg, sd, ids, mask, num_beams, max_length, trace=trace, use_cache=use_cache)
    if trace is not None:
        trace["prefix"] = prefix
    return out


def rescore(cfg, sd, input_ids, attention_mask, prof, sequences):
    """tiger_ref.rescore of hypotheses on the prefixed input."""
    prefix = prefix_tokens(cfg, sd, input_ids, prof)
    ids, mask = extend(input_ids, attention_mask)
    with prefixed(prefix):
        return tiger_ref.rescore(cfg, sd, ids, mask, sequences)
