"""Seeded BERT encoder cases at the smallest shapes at which each mechanism of csrc/bert_embed.hip can go wrong
(tests/test_bert_embed_gpu.py).  No fixture file: the weights are drawn here under ``BertModel``'s key names --
tables std 1 (a LayerNorm follows), linear weights std fan_in**-0.5 so that the scores are O(1) and the softmax
matters, biases 0.1 N(0, 1), LayerNorm weights 1 + 0.1 N(0, 1) and biases 0.1 N(0, 1) so that a dropped multiply
or add shows.  Every value is drawn in float64 from a seeded generator and rounded to float32 once, so the
float32 and the float64 runs hold the same numbers.  The oracle is the float64 run of tests/bert_embed_ref.py; its
float32 run, measured here, gives the tolerances.  Neither ``transformers`` nor the reference is imported.

    case        shape                                                       what it reaches
    tiny        H 64, 1 head of 64, I 96, 2 layers, B 6, S 33,              one row past a 32-row tile; a [CLS]-only
                lengths 33 1 2 17 32 5                                      sequence (mean 0); N and K below one tile
    heads32     H 96, 3 heads of 32, I 160, 1 layer, B 5, S 65, holes,      the narrow head; N not a multiple of 64;
                nonzero token types                                         three 32-deep k steps with a tail tile
    base_width  H 768, 12 heads, I 3072, 1 layer, B 3, S 130,               bert-base's GEMM shapes, the longest k chain
                lengths 130 64 7
    long        H 128, 2 heads of 64, I 512, 2 layers, B 2, S 512,          online softmax over every key tile, the last
                lengths 512 257                                             position row, a partly and a wholly masked tile
    deep        H 128, 2 heads, I 256, 12 layers, B 4, S 40                 rounding carried through twelve post-LN layers
"""
import functools

import torch

import bert_embed_ref as ref

BASE = dict(vocab_size=61, type_vocab_size=2, hidden_act="gelu", layer_norm_eps=1e-12,
            position_embedding_type="absolute", pad_token_id=0)

#  name         config                                                                          B    S   mask                        types  seed
CASES = {
    "tiny":       (dict(hidden_size=64, num_attention_heads=1, intermediate_size=96, num_hidden_layers=2,
                        max_position_embeddings=40),                                              6,  33, [33, 1, 2, 17, 32, 5],       False, 301),
    "heads32":    (dict(hidden_size=96, num_attention_heads=3, intermediate_size=160, num_hidden_layers=1,
                        max_position_embeddings=65),                                              5,  65, "holes",                     True,  302),
    "base_width": (dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=1,
                        max_position_embeddings=130),                                             3, 130, [130, 64, 7],                False, 303),
    "long":       (dict(hidden_size=128, num_attention_heads=2, intermediate_size=512, num_hidden_layers=2,
                        max_position_embeddings=512),                                             2, 512, [512, 257],                  False, 304),
    "deep":       (dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=12,
                        max_position_embeddings=64),                                              4,  40, [40, 9, 23, 31],             True,  305),
}
NAMES = list(CASES)


def state(cfg, seed):
    """A float32 ``BertModel`` state dict (pooler included) for ``cfg``."""
    g = torch.Generator().manual_seed(seed)

    def n(shape, std=1.0, mean=0.0):
        return (mean + std * torch.randn(*shape, generator=g, dtype=torch.float64)).float()
    sd = {}
    for name, shape in ref.state_keys(cfg):
        if "LayerNorm.weight" in name:
            sd[name] = n(shape, 0.1, 1.0)
        elif name.endswith(".bias"):
            sd[name] = n(shape, 0.1)
        elif "embeddings." in name:
            sd[name] = n(shape)
        else:
            sd[name] = n(shape, shape[1] ** -0.5)
    return sd


def inputs(cfg, B, S, recipe, types, seed):
    """(ids, mask, type_ids or None).  ``recipe``: a list of lengths (right padding) or "holes": each position
    kept with probability 0.7; sequence 0 all live; sequence 1 without its position 0; the last column live in
    sequence 2.  Masked positions hold the pad id.  ``types``: segment 1 from a drawn position on."""
    g = torch.Generator().manual_seed(seed + 1000)
    ids = torch.randint(1, int(cfg["vocab_size"]), (B, S), generator=g)
    mask = torch.zeros(B, S, dtype=torch.int64)
    if recipe == "holes":
        mask = (torch.rand(B, S, generator=g) < 0.7).to(torch.int64)
        mask[:, 0] = 1
        mask[0] = 1
        mask[1, 0] = 0
        mask[2, S - 1] = 1
    else:
        for b, length in enumerate(recipe):
            mask[b, :length] = 1
    ids[mask == 0] = int(cfg["pad_token_id"])
    type_ids = None
    if types:
        start = torch.randint(1, S, (B, 1), generator=g)
        type_ids = (torch.arange(S)[None, :] >= start).to(torch.int64)
    return ids, mask, type_ids


class Case:
    def __init__(self, name):
        delta, B, S, recipe, types, seed = CASES[name]
        self.name = name
        self.cfg = dict(BASE, **delta)
        self.B, self.S = B, S
        self.sd = state(self.cfg, seed)
        self.ids, self.mask, self.type_ids = inputs(self.cfg, B, S, recipe, types, seed)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def restated(name, dtype):
    """dict(hidden, mean_no_cls, cls) of the restatement on the case; computed once per process, left unchanged."""
    c = case(name)
    return ref.run(c.cfg, c.sd, c.ids, c.mask, c.type_ids, dtype)


@functools.lru_cache(maxsize=None)
def measured(name):
    """hidden_err32, pooled_err32, cls_err32: the float32 restatement against the float64 one."""
    return ref.measure(restated(name, torch.float32), restated(name, torch.float64), case(name).mask)
