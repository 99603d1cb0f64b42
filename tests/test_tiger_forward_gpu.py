"""TIGER's teacher-forced forward on the GPU (csrc/tiger.hip: tiger_teacher_kernel, tiger_loss_kernel) against the
float64 restatement tests/tiger_forward_ref.py.

Tolerances are 4 x the float32 reference's own distance from float64 on the same data (the suite's rule): logits
``4 * logit_err32`` per row scaled by the row's largest |logit|, per-position NLL ``4 * nll_err32`` absolute, and
``|loss - loss64| <= 4 * nll_err32 + 2**-23 * |loss64|`` (a mean of values each within the NLL tolerance is within
it; the double-accumulated sum adds one rounding).  For the recorded fixtures the reference is ``transformers``'
own run and the generator stored its distances; for the seeded cases of tests/tiger_forward_cases.py the float32
restatement is measured at run time:

    fixture          logit_err32   nll_err32        case        logit_err32   nll_err32
    tiger_main       5.24e-07      1.85e-06         fwd_one     2.40e-08      5.13e-08
    tiger_d32_b5     5.37e-07      8.04e-07         fwd_max     5.61e-07      8.84e-07
    tiger_v40_len3   3.92e-07      7.45e-07         fwd_d32     1.95e-07      4.14e-07
    tiger_eos        6.33e-07      2.82e-06         fwd_holes   3.05e-07      1.39e-06
    tiger_h2_ff128   5.69e-07      8.33e-07         fwd_nomask  fwd_max's
"""
import math

import pytest
import torch

import tiger_cases as tc
import tiger_fixtures as tf
import tiger_forward_cases as fc
import tiger_forward_ref as fref

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _binding(cfg, sd, tied, dev):
    import gr_amd
    tensors = {k: v.to(dev) for k, v in sd.items() if k not in tied}
    for k in tied:
        tensors[k] = tensors["shared.weight"]
    return gr_amd.ops.TigerBinding(cfg, tensors)


def _module(fx, dev):
    import gr_amd
    m = gr_amd.TIGER(fx.cfg)
    m.load_state_dict(fx.state_dict())
    return m.to(dev)


_RUNS = {}


def _run(name, dev):
    """One ops call per fixture or case with the logits and the per-position NLL, shared by the tests."""
    if name not in _RUNS:
        import gr_amd
        if name in fc.CASES:
            c = fc.case(name)
            bind, ids, mask, labels = _binding(c.cfg, c.sd, tc.TIED, dev), c.ids, c.mask, c.labels
        else:
            r = fc.recorded(name)
            bind, ids, mask, labels = _binding(r.fx.cfg, r.fx.sd, r.fx.meta["tied"], dev), r.fx.ids, r.fx.mask, r.labels
        out = gr_amd.ops.tiger_forward(bind, ids.to(dev), None if mask is None else mask.to(dev), labels.to(dev),
                                       with_logits=True, with_nll=True)
        _RUNS[name] = tuple(t.cpu() for t in out)
    return _RUNS[name]


@pytest.mark.parametrize("source", fc.PLAIN_FIXTURES)
def test_recorded_fixture_against_float64(source, dev):
    r = fc.recorded(source)
    loss, logits, nll = _run(source, dev)
    fc.check(loss, logits, nll, r.loss64, r.logits64, r.nll64, r.labels, r.logit_tol, r.nll_tol, source)


@pytest.mark.parametrize("name", fc.NAMES)
def test_seeded_case_against_float64(name, dev):
    c, m = fc.case(name), fc.measured(name)
    loss, logits, nll = _run(name, dev)
    loss64, logits64, nll64 = fc.restated(name, torch.float64)
    fc.check(loss, logits, nll, loss64, logits64, nll64, c.labels, 4 * m["logit_err32"], 4 * m["nll_err32"], name)


def test_no_mask_is_the_all_ones_mask(dev):
    """attention_mask=None takes the kernels' null-pointer branches: bit for bit the all-ones run."""
    for a, b in zip(_run("fwd_nomask", dev), _run("fwd_max", dev)):
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def test_ignored_positions_contribute_nothing(dev):
    """The loss is the NLLs' sum over the counted positions divided by their number, rounded once (in double the
    sum of so few float32 values is exact, whatever its order); ignoring one more last-column label, which is no
    position's input, changes no logit and removes exactly its NLL."""
    import gr_amd
    r = fc.recorded("tiger_main")
    loss, logits, nll = _run("tiger_main", dev)
    counted = r.labels != -100
    assert not nll[~counted].any() and (nll[counted] > 0).all()
    want = torch.tensor(nll.double().sum().item() / int(counted.sum()), dtype=torch.float64).float()
    assert torch.equal(_bits(loss.view(1)), _bits(want.view(1)))
    labels = r.labels.clone()
    assert labels[5, -1] != -100
    labels[5, -1] = -100
    bind = _binding(r.fx.cfg, r.fx.sd, r.fx.meta["tied"], dev)
    loss2, logits2, nll2 = (t.cpu() for t in gr_amd.ops.tiger_forward(bind, r.fx.ids.to(dev), r.fx.mask.to(dev),
                                                                      labels.to(dev), with_nll=True))
    assert torch.equal(_bits(logits2), _bits(logits)) and nll2[5, -1] == 0
    keep = torch.ones_like(counted)
    keep[5, -1] = False
    assert torch.equal(_bits(nll2[keep]), _bits(nll[keep]))
    want2 = torch.tensor((nll.double().sum() - nll[5, -1].double()).item() / (int(counted.sum()) - 1),
                         dtype=torch.float64).float()
    assert torch.equal(_bits(loss2.view(1)), _bits(want2.view(1)))
    # the optional outputs change nothing
    only = gr_amd.ops.tiger_forward(bind, r.fx.ids.to(dev), r.fx.mask.to(dev), labels.to(dev), with_logits=False)
    assert len(only) == 1 and torch.equal(_bits(only[0].cpu().view(1)), _bits(loss2.view(1)))


def test_nan_cases_and_the_empty_batch(dev):
    """No counted position in the whole batch: NaN, as torch.  A label outside [0, vocab) that is not -100: every
    read uses a clamped index, that position's NLL and the loss are NaN, everything else is what it was."""
    import gr_amd
    r = fc.recorded("tiger_d32_b5")
    V = int(r.fx.cfg["vocab_size"])
    bind = _binding(r.fx.cfg, r.fx.sd, r.fx.meta["tied"], dev)
    ids, mask = r.fx.ids.to(dev), r.fx.mask.to(dev)
    loss, logits, nll = _run("tiger_d32_b5", dev)
    out = gr_amd.ops.tiger_forward(bind, ids, mask, torch.full_like(r.labels, -100).to(dev), with_nll=True)
    assert math.isnan(out[0].item()) and not out[2].any() and bool(torch.isfinite(out[1]).all())
    for bad in (V, -1, 1 << 40, -(1 << 40)):
        labels = r.labels.clone()
        assert labels[4, 1] != -100
        labels[4, 1] = bad
        clamped = labels.clone()
        clamped[4, 1] = min(max(bad, 0), V - 1)
        got = [t.cpu() for t in gr_amd.ops.tiger_forward(bind, ids, mask, labels.to(dev), with_nll=True)]
        ref = [t.cpu() for t in gr_amd.ops.tiger_forward(bind, ids, mask, clamped.to(dev), with_nll=True)]
        assert math.isnan(got[0].item()) and math.isnan(got[2][4, 1].item()) and int(torch.isnan(got[2]).sum()) == 1
        assert torch.equal(_bits(got[1]), _bits(ref[1])) and bool(torch.isfinite(got[1]).all())
        keep = torch.ones_like(labels, dtype=torch.bool)
        keep[4, 1] = False
        assert torch.equal(_bits(got[2][keep]), _bits(ref[2][keep]))
    empty = gr_amd.ops.tiger_forward(bind, ids[:0], mask[:0], r.labels[:0].to(dev), with_nll=True)
    assert math.isnan(empty[0].item()) and empty[1].shape == (0, 4, V) and empty[2].shape == (0, 4)


def test_repeatable_and_independent_of_the_batch(dev):
    """fwd_max: a second call gives the same bits; user 5 alone, at position 2 of a batch of 3 and at position 9 of a
    batch of 17 (other group-mates, another place in its group, the tail group) gives its rows' bits."""
    import gr_amd
    c = fc.case("fwd_max")
    bind = _binding(c.cfg, c.sd, tc.TIED, dev)
    full = _run("fwd_max", dev)
    ids, mask, labels = c.ids.to(dev), c.mask.to(dev), c.labels.to(dev)
    again = gr_amd.ops.tiger_forward(bind, ids, mask, labels, with_nll=True)
    for a, b in zip(again, full):
        assert torch.equal(_bits(a.cpu()), _bits(b))
    for B, at in [(1, 0), (3, 2), (17, 9)]:
        order = torch.arange(B) % c.B
        order[at] = 5
        o = order.to(dev)
        _, logits, nll = (t.cpu() for t in gr_amd.ops.tiger_forward(bind, ids[o], mask[o], labels[o], with_nll=True))
        assert torch.equal(_bits(logits[at]), _bits(full[1][5])) and torch.equal(_bits(nll[at]), _bits(full[2][5]))
        assert torch.equal(_bits(logits), _bits(full[1][order])) and torch.equal(_bits(nll), _bits(full[2][order]))


@pytest.mark.parametrize("name", ["tiger_main", "tiger_stop"])
def test_teacher_forcing_the_top_hypothesis_gives_its_score(name, dev):
    """The labels are what generate returned first for each user, the columns after the first EOS ignored: the
    user's mean NLL is minus the returned (length-normalised) score, within the fixture's margin m.  No top
    hypothesis of tiger_main ends early; every one of tiger_stop does."""
    import gr_amd
    fx = tf.fixture(name)
    bind = _binding(fx.cfg, fx.sd, fx.meta["tied"], dev)
    ids, mask = fx.ids.to(dev), fx.mask.to(dev)
    seqs, scores = gr_amd.ops.tiger_generate(bind, ids, mask, fx.beams, fx.T)
    top = seqs[:, 0, 1:].cpu()
    is_eos = top == fx.cfg["eos_token_id"]
    after = (is_eos.long().cumsum(1) - is_eos.long()) > 0            # strictly after the first EOS
    labels = top.masked_fill(after, -100)
    assert bool(after.any(1).all()) == (name == "tiger_stop") and bool(after.any()) == (name == "tiger_stop")
    _, nll = gr_amd.ops.tiger_forward(bind, ids, mask, labels.to(dev), with_logits=False, with_nll=True)
    mean = nll.cpu().double().sum(1) / (labels != -100).sum(1)
    d = (mean + scores[:, 0].cpu().double()).abs().max().item()
    print(f"{name}: mean NLL of the top hypothesis vs its score: {d:.3e} (m {fx.m:.3e})")
    assert d <= fx.m


def test_module_forward_is_the_ops_call_and_sees_weight_updates(dev):
    r = fc.recorded("tiger_main")
    fx = r.fx
    m = _module(fx, dev).eval()
    ids, mask, labels = fx.ids.to(dev), fx.mask.to(dev), r.labels.to(dev)
    full = _run("tiger_main", dev)
    with torch.no_grad():
        loss, logits = m(ids, mask, labels)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device == ids.device
        assert torch.equal(_bits(loss.cpu().view(1)), _bits(full[0].view(1))) and torch.equal(_bits(logits.cpu()), _bits(full[1]))
        # no host round trip once the binding caches are filled
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss2, logits2 = m(input_ids=ids, attention_mask=mask, labels=labels)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(_bits(loss2.cpu().view(1)), _bits(full[0].view(1))) and torch.equal(logits2.cpu(), full[1])
        # an in-place update is seen by the next call: the float64 restatement on the new weights, at 4 x the
        # float32 restatement's distance from it
        bind = m.binding()
        m.model.shared.weight[1:9] *= 1.5
        assert m.binding() is bind
        loss3, logits3 = m(ids[:8], mask[:8], labels[:8])
    new = fx.sd["shared.weight"].clone()
    new[1:9] *= 1.5
    sd = dict(fx.sd, **{k: new for k in ["shared.weight"] + fx.meta["tied"]})
    sd64 = {k: v.double() for k, v in sd.items()}
    l32, g32, n32 = fref.forward(fx.cfg, sd, fx.ids[:8], fx.mask[:8], r.labels[:8])
    l64, g64, n64 = fref.forward(fx.cfg, sd64, fx.ids[:8], fx.mask[:8], r.labels[:8])
    counted = r.labels[:8] != -100
    logit_tol = 4 * ((g32.double() - g64).abs().amax(-1) / g64.abs().amax(-1)).max().item()
    nll_tol = 4 * (n32.double() - n64)[counted].abs().max().item()
    le = ((logits3.cpu().double() - g64).abs().amax(-1) / g64.abs().amax(-1)).max().item()
    de = abs(loss3.item() - l64.item())
    print(f"after the update: logit err {le:.3e} (tolerance {logit_tol:.3e}), loss err {de:.3e} "
          f"(tolerance {nll_tol + 2.0 ** -23 * abs(l64.item()):.3e})")
    assert not torch.equal(logits3.cpu(), full[1][:8])
    assert le <= logit_tol and de <= nll_tol + 2.0 ** -23 * abs(l64.item())


def test_eval_loss_over_two_half_batches(dev):
    import gr_amd
    r = fc.recorded("tiger_h2_ff128")
    fx = r.fx
    m = _module(fx, dev)
    half = fx.ids.shape[0] // 2
    parts = (slice(0, half), slice(half, None))
    batches = [dict(history=fx.ids[sl], attention_mask=fx.mask[sl], target=r.labels[sl]) for sl in parts]
    assert m.training and torch.is_grad_enabled()
    got = gr_amd.tiger.eval_loss(m, batches, dev)
    assert m.training and torch.is_grad_enabled() and isinstance(got, float)
    sd64 = fx.sd_as(torch.float64)
    want = [fref.forward(fx.cfg, sd64, fx.ids[sl], fx.mask[sl], r.labels[sl])[0].item() for sl in parts]
    mean = sum(want) / 2
    tol = r.nll_tol + 2.0 ** -23 * abs(mean)
    print(f"eval_loss {got:.7f} vs float64 {mean:.9f} (halves {want}): err {abs(got - mean):.3e} (tolerance {tol:.3e})")
    assert abs(want[0] - want[1]) > 100 * tol          # the mean over batches is not the mean over tokens' batch
    assert abs(got - mean) <= tol
