"""Seeded TIGER cases at the edges of the envelope that ``ops.TIGER_ENVELOPE`` promises and no recorded
fixture reaches (tests/test_tiger_envelope_ref.py on the CPU, tests/test_tiger_envelope_gpu.py and
tests/test_tiger_prefix_envelope_gpu.py on the GPU).  No fixture file: the weights are drawn here, under
the reference's T5 key names and with the library's initialisation scales (``shared`` std 1, ``q`` std
(d_model * d_kv)**-0.5, ``k`` / ``v`` / ``wi`` / the relative bias std d_model**-0.5, ``o`` std
inner**-0.5, ``wo`` std d_ff**-0.5), the norm weights as 1 + 0.1 N(0, 1) so that a dropped multiply
shows, ``lm_head`` and both ``embed_tokens`` tied to ``shared``.  The oracle is the restatement
tests/tiger_ref.py (tests/tiger_prefix_ref.py for the adapters) in float64; its float32 run gives the
tolerances.  Neither ``transformers`` nor the reference is imported.

Every value is drawn in float64 from a seeded generator and rounded to float32 once, so the float32 and
the float64 state dicts hold the same numbers.
"""
import functools

import torch

import tiger_prefix_ref as pref
import tiger_ref

TIED = ["encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight"]
BASE = dict(num_layers=1, num_decoder_layers=1, d_model=64, num_heads=4, d_kv=16, d_ff=64, pad_token_id=0,
            dropout_rate=0.1, feed_forward_proj="relu", layer_norm_epsilon=1e-6)
# The fixture generator's recipe for an EOS that is likely in every context (tests/golden/make_golden_tiger.py):
# row 0 of the last decoder block's wo becomes |wo[0]| * wo_scale, feature 0 of the EOS row eos_feature, and
# the decoder's final norm weight is multiplied by final_norm.  The eos_feature of each case was fixed by a
# CPU scan of the restatement alone (test_tiger_envelope_ref.py asserts the conditions):
#   stop_T8     9.0 (scan 6.0 .. 16.0 over seeds 106 .. 111; seed 107): in float64 the users stop after steps
#               {2: 6, 3: 5, 5: 2, 7: 3}, all 16 certified
#   holes_pad3  12.0 (scan 4.0 .. 12.0): nobody stops early, 14 of the 56 returned hypotheses end before the
#               last column, so their unfilled columns show the fill id; all 8 certified
EOS_PULL = dict(wo_scale=3.0, final_norm=0.5)
PULLED = {"stop_T8": 9.0, "holes_pad3": 12.0}

#  name          config changes                                                         B   S   beams T  mask     seed
CASES = {
    "env_max":    (dict(vocab_size=128, num_layers=4, num_decoder_layers=4, num_heads=8, d_kv=8, d_ff=256,
                        eos_token_id=127),                                               6, 128, 32, 8, "ones",  101),
    "v65_b32":    (dict(vocab_size=65, d_model=32, num_heads=1, d_kv=32, d_ff=32, eos_token_id=64),
                                                                                         6,   5, 32, 3, "left",  102),
    "v2_b1_T2":   (dict(vocab_size=2, num_heads=2, d_kv=16, d_ff=96, eos_token_id=1),    6,   1,  1, 2, "ones",  103),
    "b1_T8":      (dict(vocab_size=100, d_model=32, num_heads=4, d_kv=16, num_layers=2, num_decoder_layers=4,
                        d_ff=224, eos_token_id=9),                                       6,  67,  1, 8, "left",  104),
    "holes_pad3": (dict(vocab_size=96, num_layers=3, num_decoder_layers=2, num_heads=4, d_kv=8, d_ff=160,
                        eos_token_id=50, pad_token_id=3),                                8, 127,  7, 6, "holes", 105),
    "stop_T8":    (dict(vocab_size=80, num_layers=2, num_decoder_layers=2, num_heads=2, d_kv=32, d_ff=128,
                        eos_token_id=40),                                               16,  33, 12, 8, "left",  107),
    # env_max's weights and inputs with attention_mask=None: the restatement's result is env_max's
    "nomask":     ("env_max", None, None, None, None, "none", None),
}
NAMES = list(CASES)

#  name            T5 config changes                            bert  n_vec  B   S  beams T  mask     seed
PREFIX_CASES = {
    "pfx_one":     (dict(num_heads=1, d_kv=32),                    4,   1,   6,   1,  4, 3, "ones",  201),
    "pfx_wide":    (dict(d_model=32, num_heads=8, d_kv=8),      1024,  16,   6,  17,  4, 3, "left",  202),
    "pfx_tile":    (dict(num_heads=8, d_kv=8),                    96,  16,   6,  16,  4, 3, "left",  203),
    "pfx_holes":   (dict(num_heads=4, d_kv=16),                   32,   3,   8, 125,  6, 4, "holes", 204),
}
PREFIX_NAMES = list(PREFIX_CASES)
PREFIX_SEARCH = "pfx_holes"          # the one prefix case whose beam results are compared
PREFIX_VOCAB, PREFIX_EOS = 48, 7


def _draw(g):
    def n(*shape, std=1.0, mean=0.0):
        return (mean + std * torch.randn(*shape, generator=g, dtype=torch.float64)).float()
    return n


def t5_state(cfg, seed):
    """A float32 T5 state dict under the reference's key names, tied entries included."""
    n = _draw(torch.Generator().manual_seed(seed))
    D, dkv, H, dff, V = (int(cfg[k]) for k in ("d_model", "d_kv", "num_heads", "d_ff", "vocab_size"))
    inner = H * dkv
    sd = {"shared.weight": n(V, D)}

    def attention(p):
        sd[p + "q.weight"] = n(inner, D, std=(D * dkv) ** -0.5)
        sd[p + "k.weight"] = n(inner, D, std=D ** -0.5)
        sd[p + "v.weight"] = n(inner, D, std=D ** -0.5)
        sd[p + "o.weight"] = n(D, inner, std=inner ** -0.5)

    for side, layers in (("encoder", int(cfg["num_layers"])), ("decoder", int(cfg["num_decoder_layers"]))):
        for i in range(layers):
            p = f"{side}.block.{i}.layer."
            sd[p + "0.layer_norm.weight"] = n(D, std=0.1, mean=1.0)
            attention(p + "0.SelfAttention.")
            if i == 0:
                sd[p + "0.SelfAttention.relative_attention_bias.weight"] = n(tiger_ref.NUM_BUCKETS, H, std=D ** -0.5)
            ff = 1
            if side == "decoder":
                sd[p + "1.layer_norm.weight"] = n(D, std=0.1, mean=1.0)
                attention(p + "1.EncDecAttention.")
                ff = 2
            sd[p + f"{ff}.layer_norm.weight"] = n(D, std=0.1, mean=1.0)
            sd[p + f"{ff}.DenseReluDense.wi.weight"] = n(dff, D, std=D ** -0.5)
            sd[p + f"{ff}.DenseReluDense.wo.weight"] = n(D, dff, std=dff ** -0.5)
        sd[f"{side}.final_layer_norm.weight"] = n(D, std=0.1, mean=1.0)
    for k in TIED:
        sd[k] = sd["shared.weight"]
    return sd


def pull_eos(cfg, sd, eos_feature):
    """EOS_PULL on a state dict, in place."""
    last = int(cfg["num_decoder_layers"]) - 1
    wo = sd[f"decoder.block.{last}.layer.2.DenseReluDense.wo.weight"]
    wo[0] = wo[0].abs() * EOS_PULL["wo_scale"]
    sd["shared.weight"][int(cfg["eos_token_id"]), 0] = eos_feature
    sd["decoder.final_layer_norm.weight"] *= EOS_PULL["final_norm"]
    return sd


def adapter_state(cfg, bert_dim, seed):
    """The three ProfessionalAdapters under the reference's names (``ops.TIGER_ADAPTER_KEYS``): linear weights
    with std fan_in**-0.5, biases std 0.1, LayerNorm weights 1 + 0.1 N(0, 1) and biases 0.1 N(0, 1)."""
    n = _draw(torch.Generator().manual_seed(seed))
    d = int(cfg["d_model"])
    sd = {}
    for lvl in (1, 2, 3):
        p = f"adapter_lvl{lvl}."
        sd[p + "bert_proj.weight"] = n(d, bert_dim, std=bert_dim ** -0.5)
        sd[p + "bert_proj.bias"] = n(d, std=0.1)
        sd[p + "cross_attn.in_proj_weight"] = n(3 * d, d, std=d ** -0.5)
        sd[p + "cross_attn.in_proj_bias"] = n(3 * d, std=0.1)
        sd[p + "cross_attn.out_proj.weight"] = n(d, d, std=d ** -0.5)
        sd[p + "cross_attn.out_proj.bias"] = n(d, std=0.1)
        sd[p + "ffn.0.weight"] = n(4 * d, d, std=d ** -0.5)
        sd[p + "ffn.0.bias"] = n(4 * d, std=0.1)
        sd[p + "ffn.2.weight"] = n(d, 4 * d, std=(4 * d) ** -0.5)
        sd[p + "ffn.2.bias"] = n(d, std=0.1)
        for k in ("norm1", "norm2"):
            sd[p + k + ".weight"] = n(d, std=0.1, mean=1.0)
            sd[p + k + ".bias"] = n(d, std=0.1)
    return sd


def inputs(cfg, B, S, recipe, seed):
    """(ids [B, S] int64, mask [B, S] int64 or None).  Live ids are uniform over the vocabulary, masked
    positions hold the pad id.  Recipes: "ones"; "none" (no mask at all); "left" (contiguous left padding:
    user 0 keeps one token, user 1 all S); "holes" (each key kept with probability 0.6 and the last column
    always; user 0 all live; user 1 exactly one live key, in the middle)."""
    g = torch.Generator().manual_seed(seed + 1000)
    ids = torch.randint(0, int(cfg["vocab_size"]), (B, S), generator=g)
    if recipe == "none":
        return ids, None
    mask = torch.ones(B, S, dtype=torch.int64)
    if recipe == "left":
        for b in range(B):
            keep = 1 if b == 0 else S if b == 1 else int(torch.randint(1, S + 1, (1,), generator=g))
            mask[b, :S - keep] = 0
    elif recipe == "holes":
        mask = (torch.rand(B, S, generator=g) < 0.6).to(torch.int64)
        mask[:, -1] = 1
        mask[0] = 1
        mask[1] = 0
        mask[1, S // 2] = 1
    else:
        assert recipe == "ones", recipe
    ids[mask == 0] = int(cfg["pad_token_id"])
    return ids, mask


class Case:
    def __init__(self, name):
        delta, B, S, beams, T, recipe, seed = CASES[name]
        self.name, self.mask_recipe = name, recipe
        if isinstance(delta, str):                      # another case's weights and inputs, without the mask
            base = case(delta)
            self.ref = delta
            self.cfg, self.sd, self.B, self.S, self.beams, self.T = base.cfg, base.sd, base.B, base.S, base.beams, base.T
            self.ids, self.mask = base.ids, None
            assert bool(base.mask.all())
            return
        self.ref = name
        self.cfg = dict(BASE, **delta)
        self.B, self.S, self.beams, self.T = B, S, beams, T
        self.sd = t5_state(self.cfg, seed)
        if name in PULLED:
            pull_eos(self.cfg, self.sd, PULLED[name])
        self.ids, self.mask = inputs(self.cfg, B, S, recipe, seed)

    def sd_as(self, dtype):
        return {k: v.to(dtype) for k, v in self.sd.items()}

    @property
    def live(self):
        return torch.ones_like(self.ids, dtype=torch.bool) if self.mask is None else self.mask.bool()


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def restated(name, dtype):
    """(sequences, scores, trace) of the restatement on the case's inputs; computed once per process."""
    c = case(name)
    if c.ref != name:
        return restated(c.ref, dtype)
    trace = {}
    with torch.no_grad():
        s, sc, _ = tiger_ref.beam_search(c.cfg, c.sd_as(dtype), c.ids, c.mask, c.beams, c.T, trace=trace)
    return s, sc, trace


def _measure(r32, r64, live, extra=()):
    """The float32 restatement's distances from the float64 one, the margin m = 4 x the score distance and
    the users it certifies (every selection gap of the float64 run above m)."""
    (s32, c32, t32), (s64, c64, t64) = r32, r64
    B = s64.shape[0]
    same = torch.tensor([torch.equal(s32[b], s64[b]) for b in range(B)])
    score_err32 = (c32.double() - c64)[same].abs().max().item()
    m = 4.0 * score_err32
    e64 = t64["enc"]
    out = dict(same=same, score_err32=score_err32, m=m, certified=t64["gaps"] > m,
               enc_err32=((t32["enc"].double() - e64)[live].abs().max() / e64[live].abs().max()).item())
    stopped = t64["stopped_after"]
    worst = 0.0
    for t, (l32, l64) in enumerate(zip(t32["logits"], t64["logits"])):
        on = same & ((stopped < 0) | (stopped > t))         # a stopped user's later steps are not compared
        if on.any():
            e = (l32.double() - l64)[on].abs().amax(-1) / l64[on].abs().amax(-1)
            worst = max(worst, e.max().item())
    out["logit_err32"] = worst
    for k in extra:
        out[k + "_err32"] = ((t32[k].double() - t64[k]).abs().max() / t64[k].abs().max()).item()
    return out


@functools.lru_cache(maxsize=None)
def measured(name):
    """dict(same, score_err32, m, certified, enc_err32, logit_err32) of a case: reference against reference."""
    return _measure(restated(name, torch.float32), restated(name, torch.float64), case(name).live)


class PrefixCase:
    def __init__(self, name):
        delta, bert_dim, n_vec, B, S, beams, T, recipe, seed = PREFIX_CASES[name]
        self.name, self.mask_recipe = name, recipe
        self.cfg = dict(BASE, vocab_size=PREFIX_VOCAB, eos_token_id=PREFIX_EOS, **delta)
        self.bert_dim, self.n_vec, self.B, self.S, self.beams, self.T = bert_dim, n_vec, B, S, beams, T
        self.t5 = t5_state(self.cfg, seed)
        self.adapters = adapter_state(self.cfg, bert_dim, seed + 1)
        self.sd = {**self.t5, **self.adapters}
        self.ids, self.mask = inputs(self.cfg, B, S, recipe, seed)
        g = torch.Generator().manual_seed(seed + 2)
        self.prof = [torch.randn(B, n_vec, bert_dim, generator=g, dtype=torch.float64).float() for _ in range(3)]

    def sd_as(self, dtype):
        return {k: v.to(dtype) for k, v in self.sd.items()}

    @property
    def live(self):
        """The prefix rows and the unmasked history rows of the S + 3 encoder positions."""
        return pref.extend(self.ids, self.mask)[1].bool()


@functools.lru_cache(maxsize=None)
def prefix_case(name):
    return PrefixCase(name)


@functools.lru_cache(maxsize=None)
def prefix_restated(name, dtype):
    """(sequences, scores, trace) of the prefix restatement; the trace holds ``prefix`` and ``enc``."""
    c = prefix_case(name)
    trace = {}
    with torch.no_grad():
        s, sc, _ = pref.beam_search(c.cfg, c.sd_as(dtype), c.ids, c.mask, [p.to(dtype) for p in c.prof], c.beams, c.T,
                                    trace=trace)
    return s, sc, trace


@functools.lru_cache(maxsize=None)
def prefix_measured(name):
    """``measured`` of a prefix case, with prefix_err32 next to it."""
    return _measure(prefix_restated(name, torch.float32), prefix_restated(name, torch.float64), prefix_case(name).live,
                    extra=("prefix",))
