"""The per-stage checks of tests/bert_bf16_stages.py, proven on the CPU: an emulated device (the stage functions in
float32, GEMM chains in 64-deep steps, scores perturbed by relative 2^-23 noise so that its weight flips are not the
restatement's, the row sum added in the other order) fills the six workspace parts for both bindings of every case.

    The honest emulation passes every check that test_bert_bf16_stages_gpu.py makes on the kernels.
    Each of these, injected alone into layer 1, fails the check of its own stage on every case: tanh-GELU for erf-GELU;
    truncation for RNE in the q/k/v epilogue, the context store and the GELU epilogue; truncated softmax weights; a row
    sum taken from the unrounded weights; weights normalised before they are rounded; the last 16-deep k step dropped
    from each of the four GEMMs; an x16 that is not the RNE of the fp32 row.

So the GPU test would fail on a kernel that is subtly wrong in any of these ways.  The margins are printed.
"""
import functools

import pytest
import torch

import bert_bf16_stages as bs


@functools.lru_cache(maxsize=None)
def _honest(name):
    """(A, B, A's stages, B's stages): computed once per case, left unchanged."""
    c = bs.case(name)
    A, B = bs.emulate(c, 1), bs.emulate(c, 2)
    return A, B, bs.stages(c, 0, A, None), bs.stages(c, 1, B, A)


def test_cases_are_the_issue_s_shapes():
    c = bs.case("tiny")
    assert c.lens == [33, 1, 2, 17, 0, 5] and c.alive.tolist() == [True, True, True, True, False, True]
    assert [(bs.case(n).H, bs.case(n).I, bs.case(n).B, bs.case(n).S, bs.case(n).hd) for n in bs.NAMES] == [
        (64, 96, 6, 33, 64), (96, 160, 5, 65, 32), (768, 3072, 3, 130, 64), (128, 512, 2, 512, 64), (1024, 4096, 1, 48, 64)]
    assert all(bs.case(n).cfg["num_hidden_layers"] == 2 for n in bs.NAMES)
    assert bs.case("long").lens == [512, 257] and bs.case("base_width").lens == [130, 64, 7]


def test_layout_matches_the_header_formula():
    cfg = bs.case("heads32").cfg
    off, sizes, total = bs.layout(cfg, 7)                # 7 rows of H 96, I 160: x16 and ctx are 1344 bytes, a multiple of 16
    assert off == dict(x=0, t=2688, x16=5376, qkv=6720, ctx=10752, ff=12096) and total == 12096 + 2240
    off, sizes, total = bs.layout(dict(hidden_size=32, intermediate_size=32), 3)   # 3 x 32 x 2 = 192; 3 x 32 x 4 = 384
    assert total == 2 * 384 + 192 + 576 + 192 + 192
    ws = torch.arange(total, dtype=torch.int64).to(torch.uint8)
    v = bs.views(ws, dict(hidden_size=32, intermediate_size=32), 3)
    assert v["x"].shape == (3, 32) and v["x"].dtype == torch.float32 and v["qkv"].shape == (3, 96)
    assert v["ff"].dtype == torch.bfloat16 and v["ff"].data_ptr() == ws.data_ptr() + 2 * 384 + 192 + 576 + 192


def test_half_ulp():
    a = torch.tensor([1.0, 1.99, 2.0, 0.75, 0.0, 3.0e-39], dtype=torch.float64)
    assert bs.half_ulp_bf16(a).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -134, 2.0 ** -134]


@pytest.mark.parametrize("name", bs.NAMES)
def test_honest_emulation_passes_every_check(name):
    c = bs.case(name)
    A, B, stA, stB = _honest(name)
    assert bs.report(name, 0, bs.judge_all(c, stA, A)) == []
    assert bs.report(name, 1, bs.judge_all(c, stB, B)) == []
    assert "qkv" in stB and "qkv" not in stA


def test_an_unwritten_part_fails():
    """A part the call did not write keeps the 0xFF fill, which reads as NaN in fp32 and in bf16."""
    c = bs.case("tiny")
    A, B, _, stB = _honest("tiny")
    filled = torch.full((4,), 0xFF, dtype=torch.uint8)
    assert bool(torch.isnan(filled.view(torch.float32)).all()) and bool(torch.isnan(filled.view(torch.bfloat16).float()).all())
    for k in bs.PARTS:
        stale = B[k].clone()
        stale[c.S + 1, 3] = float("nan")                       # one element of a live sequence's row
        failed = {v.stage for v in bs.judge_all(c, stB, dict(B, **{k: stale})) if not v.ok}
        assert "written" in failed and k in failed, (k, failed)


@pytest.mark.parametrize("mistake", bs.MISTAKES)
@pytest.mark.parametrize("name", bs.NAMES)
def test_each_mistake_fails_its_own_stage(name, mistake):
    c = bs.case(name)
    A, B, _, stB = _honest(name)
    part, value = bs.mistaken(c, 1, B, A, mistake)
    stage = bs.CAUGHT_BY[mistake]
    assert part == ("x16" if stage == "x16" else stage)
    v = bs.x16_is_rne(c, dict(B, x16=value)) if stage == "x16" else bs.judge(stB[stage], value)
    print(f"{name} {mistake}: {v!r}")
    assert not v.ok, (name, mistake, v.text)
