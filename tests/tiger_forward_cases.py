"""The data of the TIGER teacher-forced forward tests (tests/test_tiger_forward_*.py).

Recorded fixtures: tests/golden/tiger_fwd_<source>.npz (tests/golden/make_golden_tiger_forward.py) next to the
weights and inputs of ``<source>.npz``.

Seeded edge cases, the smallest shapes at which the teacher kernel can go wrong; weights and inputs are drawn by
tests/tiger_cases.py (``t5_state``, ``adapter_state``, ``inputs``), the oracle is tests/tiger_forward_ref.py in
float64 and its float32 run gives the tolerances, measured at run time as ``tiger_cases._measure`` does:

    fwd_one    Ld 1, S 1, V 2, B 1: one decoder row, one key, a softmax over two logits, a user group of one
    fwd_max    Ld 8, S 128, V 128, 4 + 4 layers, 8 heads of 8, d_ff 256, B 6: the full LDS layout, a full
               group of four users and a tail of two
    fwd_d32    d_model 32, one head of 32, d_ff 32, V 65, Ld 3, B 5
    fwd_holes  a holed mask with a user of one live key, pad_token_id 3 (the shifted input's first column is 3)
    fwd_nomask fwd_max's weights and inputs with attention_mask=None (its mask is all ones)
    fwd_pfx    the prefix variant at S 125 (128 encoder positions), n_vec 16, Ld 8

Labels are uniform over the vocabulary with the generator's -100 pattern where the shape has room for it: user 0
loses its last label, user 1 keeps only its first, user 2 is ignored entirely, user 3 has -100 at position 1
followed by real labels.  Every case keeps at least one counted position.
"""
import functools
import json
import os

import numpy as np
import torch

import tiger_cases as tc
import tiger_fixtures as tf
import tiger_forward_ref as fref
import tiger_prefix_fixtures as tpf
from tiger_cases import adapter_state, inputs, t5_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLAIN_FIXTURES = ["tiger_main", "tiger_d32_b5", "tiger_v40_len3", "tiger_eos", "tiger_h2_ff128"]
PREFIX_FIXTURES = ["tiger_prefix_main", "tiger_prefix_bert768", "tiger_prefix_h2_s125"]


class Recorded:
    """tiger_fwd_<source>.npz and its source fixture (``.fx``: weights, ids, mask[, prof])."""

    def __init__(self, source):
        z = np.load(os.path.join(GOLDEN, f"tiger_fwd_{source}.npz"), allow_pickle=False)
        self.meta = json.loads(str(z["meta"]))
        self.prefixed = bool(self.meta["prefixed"])
        self.fx = (tpf if self.prefixed else tf).fixture(source)
        self.labels = torch.from_numpy(z["labels"])
        self.loss, self.logits = torch.from_numpy(z["loss"]), torch.from_numpy(z["logits"])
        self.loss64, self.logits64, self.nll64 = (torch.from_numpy(z[k]) for k in ("loss64", "logits64", "nll64"))
        self.logit_tol, self.nll_tol = 4 * self.meta["logit_err32"], 4 * self.meta["nll_err32"]


@functools.lru_cache(maxsize=None)
def recorded(source):
    return Recorded(source)


#  name          config changes                                                         B   S   Ld mask     seed
CASES = {
    "fwd_one":    (dict(vocab_size=2, num_heads=2, d_kv=16, d_ff=96, eos_token_id=1),    1,   1, 1, "ones",  301),
    "fwd_max":    (dict(vocab_size=128, num_layers=4, num_decoder_layers=4, num_heads=8, d_kv=8, d_ff=256,
                        eos_token_id=127),                                               6, 128, 8, "ones",  302),
    "fwd_d32":    (dict(vocab_size=65, d_model=32, num_heads=1, d_kv=32, d_ff=32, eos_token_id=64),
                                                                                         5,   5, 3, "left",  303),
    "fwd_holes":  (dict(vocab_size=96, num_layers=3, num_decoder_layers=2, num_heads=4, d_kv=8, d_ff=160,
                        eos_token_id=50, pad_token_id=3),                                8, 127, 5, "holes", 304),
    "fwd_nomask": ("fwd_max", None, None, None, "none", None),
}
NAMES = list(CASES)
#  name          T5 config changes            bert n_vec B   S  Ld mask     seed
PREFIX_CASES = {
    "fwd_pfx":    (dict(num_heads=4, d_kv=16),  32,  16,  6, 125, 8, "holes", 401),
}
PREFIX_NAMES = list(PREFIX_CASES)


def draw_labels(cfg, B, Ld, seed):
    g = torch.Generator().manual_seed(seed + 2000)
    labels = torch.randint(0, int(cfg["vocab_size"]), (B, Ld), generator=g)
    if Ld > 1:
        labels[0, -1] = -100
    if B > 1 and Ld > 1:
        labels[1, 1:] = -100
    if B > 2:
        labels[2, :] = -100
    if B > 3 and Ld > 2:
        labels[3, 1] = -100
    return labels


class Case:
    def __init__(self, name):
        delta, B, S, Ld, recipe, seed = CASES[name]
        self.name, self.prefixed = name, False
        if isinstance(delta, str):                      # another case's weights and inputs, without the mask
            base = case(delta)
            assert bool(base.mask.all())
            self.ref, self.cfg, self.sd, self.B, self.S, self.Ld = delta, base.cfg, base.sd, base.B, base.S, base.Ld
            self.ids, self.mask, self.labels = base.ids, None, base.labels
            return
        self.ref = name
        self.cfg = dict(tc.BASE, **delta)
        self.B, self.S, self.Ld = B, S, Ld
        self.sd = t5_state(self.cfg, seed)
        self.ids, self.mask = inputs(self.cfg, B, S, recipe, seed)
        self.labels = draw_labels(self.cfg, B, Ld, seed)

    def sd_as(self, dtype):
        return {k: v.to(dtype) for k, v in self.sd.items()}

    def restate(self, dtype):
        return fref.forward(self.cfg, self.sd_as(dtype), self.ids, self.mask, self.labels)


class PrefixCase:
    def __init__(self, name):
        delta, bert_dim, n_vec, B, S, Ld, recipe, seed = PREFIX_CASES[name]
        self.name, self.ref, self.prefixed = name, name, True
        self.cfg = dict(tc.BASE, vocab_size=tc.PREFIX_VOCAB, eos_token_id=tc.PREFIX_EOS, **delta)
        self.bert_dim, self.n_vec, self.B, self.S, self.Ld = bert_dim, n_vec, B, S, Ld
        self.t5 = t5_state(self.cfg, seed)
        self.adapters = adapter_state(self.cfg, bert_dim, seed + 1)
        self.sd = {**self.t5, **self.adapters}
        self.ids, self.mask = inputs(self.cfg, B, S, recipe, seed)
        g = torch.Generator().manual_seed(seed + 2)
        self.prof = [torch.randn(B, n_vec, bert_dim, generator=g, dtype=torch.float64).float() for _ in range(3)]
        self.labels = draw_labels(self.cfg, B, Ld, seed)

    def sd_as(self, dtype):
        return {k: v.to(dtype) for k, v in self.sd.items()}

    def restate(self, dtype):
        return fref.forward_prefix(self.cfg, self.sd_as(dtype), self.ids, self.mask, [p.to(dtype) for p in self.prof],
                                   self.labels)


@functools.lru_cache(maxsize=None)
def case(name):
    return PrefixCase(name) if name in PREFIX_CASES else Case(name)


@functools.lru_cache(maxsize=None)
def restated(name, dtype):
    """(loss, logits, nll) of the restatement on the case's inputs; computed once per process."""
    c = case(name)
    if c.ref != name:
        return restated(c.ref, dtype)
    return c.restate(dtype)


@functools.lru_cache(maxsize=None)
def measured(name):
    """The float32 restatement's distances from the float64 one: dict(logit_err32 row-scaled, nll_err32 absolute
    over the counted positions) -- reference against reference; the tests allow 4 x each."""
    (_, g32, n32), (_, g64, n64) = restated(name, torch.float32), restated(name, torch.float64)
    counted = case(name).labels != -100
    return dict(logit_err32=((g32.double() - g64).abs().amax(-1) / g64.abs().amax(-1)).max().item(),
                nll_err32=(n32.double() - n64)[counted].abs().max().item())


def check(got_loss, got_logits, got_nll, loss64, logits64, nll64, labels, logit_tol, nll_tol, what):
    """The comparison every float64 test makes (tensors on the CPU); prints each figure before it asserts."""
    counted = labels != -100
    le = ((got_logits.double() - logits64).abs().amax(-1) / logits64.abs().amax(-1)).max().item()
    ne = (got_nll.double() - nll64)[counted].abs().max().item() if counted.any() else 0.0
    de = abs(got_loss.double().item() - loss64.item())
    loss_tol = nll_tol + 2.0 ** -23 * abs(loss64.item())
    print(f"{what}: logit err {le:.3e} (tolerance {logit_tol:.3e}), nll err {ne:.3e} (tolerance {nll_tol:.3e}), "
          f"loss {got_loss.item():.7f} vs {loss64.item():.9f}: err {de:.3e} (tolerance {loss_tol:.3e})")
    assert got_logits.shape == logits64.shape and got_nll.shape == nll64.shape and got_loss.dim() == 0
    assert got_loss.dtype == got_logits.dtype == got_nll.dtype == torch.float32
    assert le <= logit_tol
    assert not got_nll[~counted].any(), "an ignored position carries a NLL"
    assert ne <= nll_tol
    assert de <= loss_tol
