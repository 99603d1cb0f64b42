"""Loading of tests/golden/t5e_*.npz, seeded parameter sets for shapes no fixture holds, and the restatement
runs the T5 embedding tests share (computed once per case and dtype, then left unchanged)."""
import functools

import numpy as np
import torch

import golden_lib as gl
import t5_embed_ref as ref

NAMES = ["t5e_main", "t5e_h3", "t5e_peaked"]
LAYER = ("layer.0.SelfAttention.q", "layer.0.SelfAttention.k", "layer.0.SelfAttention.v", "layer.0.SelfAttention.o",
         "layer.0.layer_norm", "layer.1.DenseReluDense.wi", "layer.1.DenseReluDense.wo", "layer.1.layer_norm")
REL = "model.encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


class Fixture:
    def __init__(self, name):
        sd, out, meta = gl.load(name)
        self.name, self.meta, self.out = name, meta, out
        self.cfg, self.params = meta["config"], meta["params"]
        self.sd = {k: torch.from_numpy(v) for k, v in sd.items()}
        self.seq = torch.from_numpy(out["seq_embs"])
        self.mask = torch.from_numpy(out["attention_mask"])
        self.target = torch.from_numpy(out["target_emb"])
        self.pred64 = torch.from_numpy(out["pred64"])
        self.hidden64 = torch.from_numpy(out["hidden64"])

    def state_dict(self):
        """The reference's state dict: every key of meta["keys"]; the unused token table is zeros."""
        return {k: self.sd[k].clone() if k in self.sd else torch.zeros(shape) for k, shape in self.meta["keys"]}


@functools.lru_cache(maxsize=None)
def fixture(name):
    return Fixture(name)


def bf16(t):
    return t.to(torch.bfloat16).float()


def random_state(cfg, seed, rel_scale=1.0):
    """Seeded bf16-representable parameters under the reference's names (the token table left out), in T5's
    initialisation scales: unit-RMS rows give O(1) scores, so the softmax and the buckets matter."""
    g = torch.Generator().manual_seed(seed)
    d, H, dkv, dff, nl = (int(cfg[k]) for k in ("d_model", "num_heads", "d_kv", "d_ff", "num_layers"))
    din, dout, inner = int(cfg["input_emb_dim"]), int(cfg["target_emb_dim"]), H * dkv

    def n(shape, std):
        return bf16(torch.randn(shape, generator=g) * std)
    sd = {"input_proj.weight": n((d, din), din ** -0.5), "input_proj.bias": n((d,), 0.1),
          "output_proj.weight": n((dout, d), d ** -0.5), "output_proj.bias": n((dout,), 0.1),
          REL: n((32, H), rel_scale), "model.encoder.final_layer_norm.weight": bf16(1.0 + n((d,), 0.1))}
    for l in range(nl):
        pre = f"model.encoder.block.{l}."
        sd[pre + LAYER[0] + ".weight"] = n((inner, d), (d * dkv) ** -0.5)
        sd[pre + LAYER[1] + ".weight"] = n((inner, d), d ** -0.5)
        sd[pre + LAYER[2] + ".weight"] = n((inner, d), d ** -0.5)
        sd[pre + LAYER[3] + ".weight"] = n((d, inner), inner ** -0.5)
        sd[pre + LAYER[4] + ".weight"] = bf16(1.0 + n((d,), 0.1))
        sd[pre + LAYER[5] + ".weight"] = n((dff, d), d ** -0.5)
        sd[pre + LAYER[6] + ".weight"] = n((d, dff), dff ** -0.5)
        sd[pre + LAYER[7] + ".weight"] = bf16(1.0 + n((d,), 0.1))
    return sd


def sequences(B, S, dim, seed, lengths=None):
    """Right-padded random sequences (zeros in the padding) and their int64 mask."""
    rng = np.random.default_rng(seed)
    if lengths is None:
        lengths = [S if b == 0 else 1 if b == 1 else int(rng.integers(1, S + 1)) for b in range(B)]
    seq = np.zeros((B, S, dim), np.float32)
    mask = np.zeros((B, S), np.int64)
    for b, n in enumerate(lengths):
        seq[b, :n] = 0.5 * rng.standard_normal((n, dim)).astype(np.float32)
        mask[b, :n] = 1
    return torch.from_numpy(seq), torch.from_numpy(mask)


def restate(cfg, sd, seq, mask):
    """-> dict: the float64 restatement's pred / hidden, and the float32 restatement's distance from it (live
    rows, relative to the largest magnitude): the measure of what float32 can give on these inputs."""
    with torch.no_grad():
        p64, h64, _ = ref.forward(cfg, sd, seq, mask, torch.float64)
        p32, h32, _ = ref.forward(cfg, sd, seq, mask, torch.float32)
    return dict(pred64=p64, hidden64=h64, pred32=p32, pred_err32=ref.live_err(p32, p64),
                hidden_err32=ref.live_err(h32, h64, mask))
