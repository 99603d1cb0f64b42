"""The CPU restatement of the BERT encoder's bf16 precision (tests/bert_bf16_ref.py): what it is when its rounding is
off, what the rounding costs, and which wrong steps the GPU tests' tolerance -- 4 x the restatement's own distance
from the float64 run -- can tell apart.

Documented limits, asserted nowhere: a dropped key bias is not detectable by any tolerance (it adds q . b_k to every
score of a row, and the softmax is invariant under a per-row shift; in exact arithmetic the output does not change),
and tanh-GELU for the exact erf-GELU is not detectable by this one (measured: its distance from float64 stays within
about 1.2 x the exact restatement's).  The second IS detected by the per-stage checks on the call's own operands
(tests/bert_bf16_stages.py, test_bert_bf16_stages_gpu.py; shown on the CPU in test_bert_bf16_stages_ref.py: 7-9 % of the
GELU stage's elements fall outside the rounding bound), as are truncation for RNE, a row sum from unrounded weights and
normalise-then-round, which this end-to-end tolerance cannot see either.
"""
import pytest
import torch

import bert_bf16_ref as bref
import bert_cases as bc


@pytest.mark.parametrize("name", bc.NAMES)
def test_without_rounding_it_is_the_float32_restatement(name):
    got = bref.run(bc.case(name), rounding=False)
    want = bc.restated(name, torch.float32)
    for k in ("hidden", "mean_no_cls", "cls"):
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("name", bc.NAMES)
def test_rounding_costs_more_than_100_times_float32(name):
    b, f = bref.measured_bf16(name), bc.measured(name)
    for k, e in (("hidden", "hidden_err32"), ("mean_no_cls", "pooled_err32"), ("cls", "cls_err32")):
        print(f"{name}: {k} bf16 restatement {b[k]:.3e}, float32 restatement {f[e]:.3e}")
        assert b[k] > 100 * f[e], (k, b[k], f[e])


@pytest.mark.parametrize("mistake", ["no_attention_output_bias", "no_output_bias", "relu", "no_mask"])
@pytest.mark.parametrize("name", bc.NAMES)
def test_mistakes_the_tolerance_can_tell(name, mistake):
    d = bref.distance(bref.run(bc.case(name), mistake=mistake), name)["hidden"]
    bound = 4 * bref.measured_bf16(name)["hidden"]
    print(f"{name} {mistake}: hidden {d:.3e} against the bound {bound:.3e}")
    assert d > bound, (d, bound)


def test_the_wide_case_reaches_the_longest_chain():
    c = bref.case("wide")
    assert c.cfg["intermediate_size"] == 4096 and c.cfg["hidden_size"] == 1024 and c.ids.shape == (1, 48)
    assert int(c.mask.sum()) == 48
    assert max(cc.cfg["intermediate_size"] for cc in map(bc.case, bc.NAMES)) < 4096
    b = bref.measured_bf16("wide")
    assert all(0 < v < 0.1 for v in b.values()), b
