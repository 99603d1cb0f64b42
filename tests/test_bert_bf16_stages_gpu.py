"""The BERT encoder's bf16 kernels (gr_bert_embed_bf16 / gr_bert_embed_ragged_bf16, csrc/bert_embed.hip) stage by stage
against float64 on their OWN operands, read from the call's workspace (tests/bert_bf16_stages.py has the method, the
criteria and the cases; tests/test_bert_bf16_stages_ref.py shows on the CPU that each check fails on a subtly wrong
kernel: tanh-GELU, truncation for RNE, an fp32 row sum, normalise-then-round, a dropped k step, a wrong x16).

Per case two bindings over the same tensors, ``A`` with layer 0 alone and ``B`` with both layers, each run once with
hidden_out.  On ``B`` (layer 1): qkv from A's x16; ctx from B's qkv; x from A's hidden_out and B's ctx; ff from RNE(B's
x); t from B's x and ff; hidden_out from B's t, and x16 == RNE(hidden_out) bit for bit; both poolings from hidden_out.
On ``A`` (layer 0) the same without qkv, the residual being the float64 embedding LayerNorm from the tables, which pins
the embedding stage.  No part may hold NaN (the workspace is 0xFF-filled before the call).  One ragged run of ``heads32``
with the exact row bound must leave the padded run's bits in all six parts.

Measured on an MI355X, the ranges over the five cases and both layers (delta = 4 x the float32 restatement's distance
from float64 on the same operands; the device's own noise is max(|got - y64| - 1/2 ulp, 0) for the bf16 parts and
max |got - y64| for the fp32 ones; 1/2 ulp_bf16 of 1.0 is 3.9e-3):
    stage         device noise          delta                 elements / rows outside
    qkv           0 .. 3.2e-7           1.6e-6 .. 6.0e-6      0
    ctx           0 .. 1.8e-6 (inside)  6.0e-7 .. 2.8e-6      0 .. 0.29 % of rows (long; the float32 restatement's own
                                                              flipped share 0 .. 0.93 %), none past the loose bound
    x             5.4e-7 .. 1.7e-6      2.3e-6 .. 4.7e-6
    ff            0 .. 3.6e-7           1.6e-6 .. 6.9e-6      0
    t             4.3e-7 .. 3.0e-6      1.7e-6 .. 8.5e-6
    hidden        4.0e-7 .. 7.4e-7      1.9e-6 .. 3.5e-6      x16 == RNE(hidden_out) everywhere
    mean_no_cls   8.4e-8 .. 2.0e-7      6.5e-7 .. 2.2e-6
    cls           0                     0
The kernels need at most 1.8 x the restatement's own distance (t of base_width's layer 0: 3.0e-6 against 1.66e-6; x of
wide's layer 1 1.6 x), so the 4 x rule holds with room on every stage.
"""
import functools

import pytest
import torch

import bert_bf16_stages as bs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _runs(name):
    """(A, B) on the CPU: computed once per case, left unchanged."""
    import gr_amd
    c = bs.case(name)
    sd = {k: v.to(DEV) for k, v in c.sd.items()}
    A = bs.device_run(gr_amd.ops.BertBf16Binding(c.cfg1, sd), c)
    B = bs.device_run(gr_amd.ops.BertBf16Binding(c.cfg, sd), c)
    return A, B


@pytest.mark.parametrize("name", bs.NAMES)
def test_layer_1_stages_on_the_call_s_own_operands(name, dev):
    c = bs.case(name)
    A, B = _runs(name)
    assert bs.report(name, 1, bs.judge_all(c, bs.stages(c, 1, B, A), B)) == []


@pytest.mark.parametrize("name", bs.NAMES)
def test_layer_0_stages_and_the_embeddings(name, dev):
    c = bs.case(name)
    A, _ = _runs(name)
    assert bs.report(name, 0, bs.judge_all(c, bs.stages(c, 0, A, None), A)) == []


def test_dead_sequence_parts(dev):
    """tiny's sequence 4 has no live key: its context rows and hidden_out are zeros, its x16 is not (the pooling kernel
    zeroes hidden_out alone), and both pooled rows are zeros."""
    c = bs.case("tiny")
    _, B = _runs("tiny")
    rows = slice(4 * c.S, 5 * c.S)
    assert c.lens[4] == 0
    assert bool((B["ctx"][rows].float() == 0).all()) and bool((B["hidden"][4] == 0).all())
    assert bool((B["x16"][rows].float() != 0).any())
    assert bool((B["mean_no_cls"][4] == 0).all()) and bool((B["cls"][4] == 0).all())


def test_ragged_parts_are_the_padded_run_s_bits(dev):
    import gr_amd
    c = bs.case("heads32")
    _, B = _runs("heads32")
    exact = sum(c.lens)
    assert 0 < exact < c.B * c.S
    binding = gr_amd.ops.BertBf16Binding(c.cfg, {k: v.to(DEV) for k, v in c.sd.items()})
    pooled, hidden, off, v = bs.call_ragged(binding, c.ids, c.mask, c.type_ids, "mean_no_cls", exact)
    off = off.tolist()
    assert off == [sum(c.lens[:i]) for i in range(c.B + 1)]
    for k in bs.PARTS:
        got = v[k].cpu()
        assert not bool(torch.isnan(got.float()).any()), k
        for b, n in enumerate(c.lens):
            assert torch.equal(bs.bits(got[off[b]:off[b] + n]), bs.bits(B[k][b * c.S:b * c.S + n])), (k, b)
    hidden = hidden.cpu()
    for b, n in enumerate(c.lens):
        assert torch.equal(bs.bits(hidden[off[b]:off[b] + n]), bs.bits(B["hidden"][b, :n])), b
    assert torch.equal(bs.bits(pooled.cpu()), bs.bits(B["mean_no_cls"]))
