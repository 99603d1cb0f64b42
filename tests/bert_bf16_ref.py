"""CPU restatement of the BERT encoder's bf16 precision (``gr_bert_embed_bf16``, the contract in include/gr_amd.h):
``bert_embed_ref.forward`` in float32 with ``t.to(torch.bfloat16).float()`` (round-to-nearest-even) applied at exactly
the contract's rounding points --

    GEMM operands   the A operand and the weight of the four projections per layer (the bias stays float32)
    q, k, v         the q/k/v projections' outputs
    probabilities   the softmax's output where it becomes the P . v operand.  NORMALISED here: the kernel's online
                    softmax rounds the un-normalised exp(s - running max) and divides by the float32 sum of the
                    rounded values; both are one bf16 rounding of each weight, the kernel's rows sum to 1 within float32,
                    these within bf16
    context, GELU   the attention context and the GELU output (they are only ever GEMM A operands)

-- and everything else (scores and their scale, softmax, bias, GELU, residual, LayerNorm, pooling) in float32.  With
``rounding=False`` it is ``bert_embed_ref.forward`` in float32, operation for operation.  ``measured_bf16(name)`` is
its distance from the float64 run: what bf16 operands cost on that case, and the tolerance the GPU tests scale.

``mistake`` injects one wrong step, to show which ones that tolerance can tell: ``"no_attention_output_bias"``,
``"no_output_bias"``, ``"relu"`` (for GELU) and ``"no_mask"`` are detectable; ``"no_key_bias"`` (softmax-invariant: it
adds the same q . b_k to every score of a row) and ``"tanh_gelu"`` (within about 1.2 x the exact one's error) are NOT.

``wide`` is one extra case beside the five of tests/bert_cases.py: H 1024, 16 heads of 64, I 4096, 1 layer, B 1, S 48,
all live -- the envelope's longest bf16 k chain (4096), which no float32 case reaches.
"""
import functools
import math

import torch

import bert_cases as bc
import bert_embed_ref as ref

WIDE = (dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=1,
             max_position_embeddings=48), 1, 48, [48], False, 306)
NAMES = list(bc.NAMES) + ["wide"]
MISTAKES = ("no_attention_output_bias", "no_output_bias", "relu", "no_mask", "no_key_bias", "tanh_gelu")


class _Wide:
    def __init__(self):
        delta, B, S, recipe, types, seed = WIDE
        self.name = "wide"
        self.cfg = dict(bc.BASE, **delta)
        self.B, self.S = B, S
        self.sd = bc.state(self.cfg, seed)
        self.ids, self.mask, self.type_ids = bc.inputs(self.cfg, B, S, recipe, types, seed)


@functools.lru_cache(maxsize=None)
def case(name):
    return _Wide() if name == "wide" else bc.case(name)


def bf16(t):
    return t.to(torch.bfloat16).float()


def forward(cfg, sd, ids, mask=None, type_ids=None, rounding=True, mistake=None):
    """-> last hidden state [B, S, H], float32."""
    assert mistake is None or mistake in MISTAKES
    dtype = torch.float32
    r = bf16 if rounding else (lambda t: t)
    H, nh = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    hd, eps = H // nh, float(cfg.get("layer_norm_eps", 1e-12))
    B, S = ids.shape

    def w(k):
        return sd[k].to(dtype)
    tt = torch.zeros_like(ids) if type_ids is None else type_ids
    live = torch.ones(B, S, dtype=torch.bool) if mask is None else mask != 0
    keys = torch.ones(B, S, dtype=torch.bool) if mistake == "no_mask" else live
    x = (w("embeddings.word_embeddings.weight")[ids] + w("embeddings.token_type_embeddings.weight")[tt]) \
        + w("embeddings.position_embeddings.weight")[:S]
    x = ref.layer_norm(x, w("embeddings.LayerNorm.weight"), w("embeddings.LayerNorm.bias"), eps)
    for l in range(int(cfg["num_hidden_layers"])):
        p = f"encoder.layer.{l}."

        def lin(t, k, bias=True):
            y = r(t) @ r(w(p + k + ".weight")).T
            return y + w(p + k + ".bias") if bias else y

        def heads(t):
            return t.view(B, S, nh, hd).transpose(1, 2)
        q = heads(r(lin(x, "attention.self.query")))
        k = heads(r(lin(x, "attention.self.key", bias=mistake != "no_key_bias")))
        v = heads(r(lin(x, "attention.self.value")))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
        s = s.masked_fill(~keys[:, None, None, :], float("-inf"))
        pr = r(torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0))
        ctx = r((pr @ v).transpose(1, 2).reshape(B, S, H))
        x = ref.layer_norm(x + lin(ctx, "attention.output.dense", bias=mistake != "no_attention_output_bias"),
                           w(p + "attention.output.LayerNorm.weight"), w(p + "attention.output.LayerNorm.bias"), eps)
        t = lin(x, "intermediate.dense")
        if mistake == "relu":
            f = torch.relu(t)
        elif mistake == "tanh_gelu":
            f = 0.5 * t * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (t + 0.044715 * t ** 3)))
        else:
            f = ref.gelu(t)
        x = ref.layer_norm(x + lin(r(f), "output.dense", bias=mistake != "no_output_bias"),
                           w(p + "output.LayerNorm.weight"), w(p + "output.LayerNorm.bias"), eps)
    return x * live.any(dim=1)[:, None, None].to(dtype)


def run(c, rounding=True, mistake=None):
    """-> dict(hidden, mean_no_cls, cls), float32, of the restatement on case object ``c``."""
    with torch.no_grad():
        h = forward(c.cfg, c.sd, c.ids, c.mask, c.type_ids, rounding, mistake)
        return dict(hidden=h, mean_no_cls=ref.pool(h, c.mask, "mean_no_cls"), cls=ref.pool(h, c.mask, "cls"))


@functools.lru_cache(maxsize=None)
def restated(name, dtype):
    """``bert_cases.restated`` with ``wide``: the float64 oracle and the float32 run, once per process."""
    if name != "wide":
        return bc.restated(name, dtype)
    c = case(name)
    return ref.run(c.cfg, c.sd, c.ids, c.mask, c.type_ids, dtype)


@functools.lru_cache(maxsize=None)
def measured(name):
    """``bert_cases.measured`` with ``wide``: the float32 restatement's distance from float64."""
    return ref.measure(restated(name, torch.float32), restated(name, torch.float64), case(name).mask)


def distance(got, name):
    """dict(hidden, mean_no_cls, cls): ``live_err`` of ``got`` against the float64 run of case ``name``."""
    want, mask = restated(name, torch.float64), case(name).mask
    return {k: ref.live_err(got[k], want[k], mask if k == "hidden" else None) for k in ("hidden", "mean_no_cls", "cls")}


@functools.lru_cache(maxsize=None)
def measured_bf16(name):
    """The bf16 restatement's distance from the float64 run: dict(hidden, mean_no_cls, cls)."""
    return distance(run(case(name)), name)
