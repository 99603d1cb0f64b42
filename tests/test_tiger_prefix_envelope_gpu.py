"""The adapter kernel of the TIGER prefix variant (csrc/tiger.hip: tiger_adapter_kernel) at the edges of what
``ops.tiger_prefix_check`` accepts, against the float64 restatement tests/tiger_prefix_ref.py on the seeded
cases of tests/tiger_cases.py:

    pfx_one     n_vec 1, bert_dim 4, S 1, d_model 64, one head of width 64: a softmax over one key, a single
                float4 in bert_proj, one history row
    pfx_wide    n_vec 16, bert_dim 1024, S 17, d_model 32, 8 heads of width 4: the full score array, the
                longest fma chains, a row tile of 16 and a tail of 1
    pfx_tile    n_vec 16, bert_dim 96, S 16, d_model 64, 8 heads: exactly one full row tile, 128 (row, head) items
    pfx_holes   n_vec 3, S 125 with holes in the mask, d_model 64, 4 heads: the mean divides by S over all
                rows, masked or not, and the extended mask reaches the encoder

Tolerances are 4 x the float32 restatement's own worst distance from float64 on the same case, measured at
run time by ``tiger_cases.prefix_measured``; a CPU run gave

    case        prefix_err32   enc_err32   logit_err32   score_err32 (m = 4 x)   certified
    pfx_one     2.96e-07       3.10e-07    2.35e-07      7.27e-07                6/6
    pfx_wide    1.91e-07       3.26e-07    3.87e-07      4.80e-07                6/6
    pfx_tile    3.44e-07       2.54e-07    2.41e-07      4.65e-07                6/6
    pfx_holes   2.89e-07       2.64e-07    3.78e-07      5.25e-07                8/8

(prefix tokens and hidden states relative to the tensor's largest magnitude).  The search kernel is the plain
entry's, so only pfx_holes compares beam results.
"""
import pytest
import torch

import tiger_cases as tc
import tiger_prefix_ref as pref

pytestmark = pytest.mark.gpu

_RUNS = {}


def _run(name, dev):
    """One ops call per case with the prefix tokens and the encoder output, shared by the tests."""
    if name not in _RUNS:
        import gr_amd
        c = tc.prefix_case(name)
        t5 = {k: v.to(dev) for k, v in c.t5.items() if k not in tc.TIED}
        for k in tc.TIED:
            t5[k] = t5["shared.weight"]
        bind = gr_amd.ops.TigerPrefixBinding(c.cfg, t5, {k: v.to(dev) for k, v in c.adapters.items()})
        out = gr_amd.ops.tiger_generate_prefix(bind, c.ids.to(dev), c.mask.to(dev), *[p.to(dev) for p in c.prof],
                                               c.beams, c.T, with_prefix=True, with_encoder=True)
        _RUNS[name] = tuple(t.cpu() for t in out)
    return _RUNS[name]


@pytest.mark.parametrize("name", tc.PREFIX_NAMES)
def test_prefix_tokens_and_encoder_against_float64(name, dev):
    c, m = tc.prefix_case(name), tc.prefix_measured(name)
    _, _, prefix, enc = _run(name, dev)
    tr = tc.prefix_restated(name, torch.float64)[2]
    p64 = tr["prefix"]
    assert prefix.shape == p64.shape == (c.B, 3, c.cfg["d_model"])
    err = ((prefix.double() - p64).abs().max() / p64.abs().max()).item()
    tol = 4 * m["prefix_err32"]
    print(f"{name}: prefix err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    live = c.live                                               # the prefix rows and the unmasked rows
    assert live[:, :3].all()
    e64 = tr["enc"]
    assert enc.shape == e64.shape == (c.B, c.S + 3, c.cfg["d_model"])
    err = ((enc.double() - e64)[live].abs().max() / e64[live].abs().max()).item()
    tol = 4 * m["enc_err32"]
    print(f"{name}: encoder err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol


def test_the_mean_runs_over_masked_rows_too(dev):
    """pfx_holes: the kernel's prefix tokens are the mean over all 125 rows; the mean over the unmasked rows
    lies more than 100 tolerances from the float64 restatement, so it cannot pass for it."""
    c, m = tc.prefix_case("pfx_holes"), tc.prefix_measured("pfx_holes")
    prefix = _run("pfx_holes", dev)[2]
    p64 = tc.prefix_restated("pfx_holes", torch.float64)[2]["prefix"]
    with torch.no_grad():
        masked = pref.prefix_tokens(c.cfg, c.sd_as(torch.float64), c.ids, [p.double() for p in c.prof], row_mask=c.mask)
    tol = 4 * m["prefix_err32"]
    scale = p64.abs().max()
    apart = ((masked - p64).abs().max() / scale).item()
    print(f"pfx_holes: the masked mean lies {apart:.3e} from the mean over all rows (tolerance {tol:.3e})")
    assert apart > 100 * tol
    assert ((prefix.double() - p64).abs().max() / scale).item() <= tol
    assert ((prefix.double() - masked).abs().max() / scale).item() > 99 * tol


def test_beam_results_on_the_holed_history(dev):
    name = tc.PREFIX_SEARCH
    c, m = tc.prefix_case(name), tc.prefix_measured(name)
    seqs, scores = _run(name, dev)[:2]
    s64, c64, _ = tc.prefix_restated(name, torch.float64)
    cert = m["certified"]
    assert cert.float().mean() >= 0.9
    bad = [b for b in range(c.B) if cert[b] and not torch.equal(seqs[b], s64[b])]
    d = (scores.double() - c64)[cert].abs().max().item()
    print(f"{name}: {int(cert.sum())}/{c.B} certified, users differing {bad}, score err {d:.3e} (m {m['m']:.3e})")
    assert not bad
    assert d <= m["m"]
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    with torch.no_grad():
        r = pref.rescore(c.cfg, c.sd_as(torch.float64), c.ids, c.mask, [p.double() for p in c.prof], seqs)
    d = (r - scores.double()).abs().max().item()
    print(f"{name}: re-scored hypotheses differ by {d:.3e} (m {m['m']:.3e})")
    assert d <= m["m"]
    assert bool((seqs[:, :, 0] == c.cfg["pad_token_id"]).all())
