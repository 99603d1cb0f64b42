"""The prefix variant's teacher-forced forward on the GPU (gr_tiger_forward_prefix_f32: the adapter launch,
tiger_encoder_kernel<true> on S + 3 positions, tiger_teacher_kernel, tiger_loss_kernel) against the float64
restatement tests/tiger_forward_ref.py ``forward_prefix``; the rule and the code shape of
test_tiger_forward_gpu.py.  The reference's own distances from float64 (recorded fixtures) and the float32
restatement's (the seeded case), of which the tests allow 4 x:

    fixture                logit_err32   nll_err32        case      logit_err32   nll_err32
    tiger_prefix_main      4.11e-07      9.82e-07         fwd_pfx   4.44e-07      1.50e-06
    tiger_prefix_bert768   3.65e-07      8.02e-07
    tiger_prefix_h2_s125   6.63e-07      7.49e-07
"""
import pytest
import torch

import tiger_cases as tc
import tiger_forward_cases as fc
import tiger_forward_ref as fref

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _binding(cfg, sd, tied, dev):
    import gr_amd
    t5 = {k: v.to(dev) for k, v in sd.items() if k not in tied and not k.startswith("adapter_lvl")}
    for k in tied:
        t5[k] = t5["shared.weight"]
    return gr_amd.ops.TigerPrefixBinding(cfg, t5, {k: v.to(dev) for k, v in sd.items() if k.startswith("adapter_lvl")})


def _module(fx, dev):
    import gr_amd
    m = gr_amd.tiger_prefix.TIGER(fx.cfg)
    m.load_state_dict(fx.state_dict())
    return m.to(dev)


_RUNS = {}


def _run(name, dev):
    """One ops call per fixture or case with the logits and the per-position NLL, shared by the tests."""
    if name not in _RUNS:
        import gr_amd
        if name in fc.PREFIX_CASES:
            c = fc.case(name)
            bind, ids, mask, prof, labels = _binding(c.cfg, c.sd, tc.TIED, dev), c.ids, c.mask, c.prof, c.labels
        else:
            r = fc.recorded(name)
            fx = r.fx
            bind, ids, mask, prof, labels = _binding(fx.cfg, fx.sd, fx.meta["tied"], dev), fx.ids, fx.mask, fx.prof, r.labels
        out = gr_amd.ops.tiger_forward_prefix(bind, ids.to(dev), mask.to(dev), *[p.to(dev) for p in prof], labels.to(dev),
                                              with_logits=True, with_nll=True)
        _RUNS[name] = tuple(t.cpu() for t in out)
    return _RUNS[name]


@pytest.mark.parametrize("source", fc.PREFIX_FIXTURES)
def test_recorded_fixture_against_float64(source, dev):
    r = fc.recorded(source)
    loss, logits, nll = _run(source, dev)
    fc.check(loss, logits, nll, r.loss64, r.logits64, r.nll64, r.labels, r.logit_tol, r.nll_tol, source)


@pytest.mark.parametrize("name", fc.PREFIX_NAMES)
def test_seeded_case_against_float64(name, dev):
    c, m = fc.case(name), fc.measured(name)
    loss, logits, nll = _run(name, dev)
    loss64, logits64, nll64 = fc.restated(name, torch.float64)
    fc.check(loss, logits, nll, loss64, logits64, nll64, c.labels, 4 * m["logit_err32"], 4 * m["nll_err32"], name)


def test_seeded_case_is_repeatable_and_returns_the_encoder_output(dev):
    import gr_amd
    c = fc.case("fwd_pfx")
    bind = _binding(c.cfg, c.sd, tc.TIED, dev)
    out = gr_amd.ops.tiger_forward_prefix(bind, c.ids.to(dev), c.mask.to(dev), *[p.to(dev) for p in c.prof],
                                          c.labels.to(dev), with_nll=True, with_encoder=True)
    for a, b in zip(out[:3], _run("fwd_pfx", dev)):
        assert torch.equal(_bits(a.cpu()), _bits(b))
    assert out[3].shape == (c.B, c.S + 3, c.cfg["d_model"]) and bool(torch.isfinite(out[3]).all())


def test_module_forward_with_and_without_the_prefix(dev):
    """With all three prof_lvl*: the ops call, bit for bit, with no host round trip on a second call.  Without
    them (or with one missing): the plain module's loss and logits, bit for bit -- and not the prefixed ones."""
    import gr_amd
    r = fc.recorded("tiger_prefix_main")
    fx = r.fx
    m = _module(fx, dev).eval()
    ids, mask, labels = fx.ids.to(dev), fx.mask.to(dev), r.labels.to(dev)
    prof = [p.to(dev) for p in fx.prof]
    full = _run("tiger_prefix_main", dev)
    plain = gr_amd.TIGER(fx.cfg)
    plain.load_state_dict({k: v for k, v in fx.state_dict().items() if k.startswith("model.")})
    plain = plain.to(dev).eval()
    with torch.no_grad():
        loss, logits = m(ids, mask, labels, *prof)
        assert torch.equal(_bits(loss.cpu().view(1)), _bits(full[0].view(1))) and torch.equal(_bits(logits.cpu()), _bits(full[1]))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss2, logits2 = m(input_ids=ids, attention_mask=mask, labels=labels, prof_lvl1=prof[0], prof_lvl2=prof[1],
                               prof_lvl3=prof[2])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(_bits(loss2.cpu().view(1)), _bits(full[0].view(1))) and torch.equal(logits2.cpu(), full[1])
        want_loss, want_logits = plain(ids, mask, labels)
        for kw in ({}, dict(prof_lvl1=prof[0], prof_lvl3=prof[2])):
            got_loss, got_logits = m(ids, mask, labels, **kw)
            assert torch.equal(_bits(got_loss.view(1)), _bits(want_loss.view(1)))
            assert torch.equal(_bits(got_logits), _bits(want_logits))
        assert not torch.equal(want_logits.cpu(), full[1]) and want_loss.item() != full[0].item()
        # an in-place update of an adapter weight is seen by the next call
        bind = m.prefix_binding()
        m.adapter_lvl2.bert_proj.weight.mul_(1.5)
        assert m.prefix_binding() is bind
        loss3, logits3 = m(ids, mask, labels, *prof)
    sd = dict(fx.sd)
    sd["adapter_lvl2.bert_proj.weight"] = sd["adapter_lvl2.bert_proj.weight"] * 1.5
    l32, g32, n32 = fref.forward_prefix(fx.cfg, sd, fx.ids, fx.mask, fx.prof, r.labels)
    l64, g64, n64 = fref.forward_prefix(fx.cfg, {k: v.double() for k, v in sd.items()}, fx.ids, fx.mask,
                                        [p.double() for p in fx.prof], r.labels)
    counted = r.labels != -100
    logit_tol = 4 * ((g32.double() - g64).abs().amax(-1) / g64.abs().amax(-1)).max().item()
    nll_tol = 4 * (n32.double() - n64)[counted].abs().max().item()
    le = ((logits3.cpu().double() - g64).abs().amax(-1) / g64.abs().amax(-1)).max().item()
    de = abs(loss3.item() - l64.item())
    print(f"after the update: logit err {le:.3e} (tolerance {logit_tol:.3e}), loss err {de:.3e} "
          f"(tolerance {nll_tol + 2.0 ** -23 * abs(l64.item()):.3e})")
    assert not torch.equal(logits3.cpu(), full[1])
    assert le <= logit_tol and de <= nll_tol + 2.0 ** -23 * abs(l64.item())


def test_eval_loss_over_two_half_batches(dev):
    import gr_amd
    r = fc.recorded("tiger_prefix_h2_s125")
    fx = r.fx
    m = _module(fx, dev)
    half = fx.ids.shape[0] // 2
    parts = (slice(0, half), slice(half, None))
    batches = [dict(history=fx.ids[sl], attention_mask=fx.mask[sl], target=r.labels[sl], prof_lvl1=fx.prof[0][sl],
                    prof_lvl2=fx.prof[1][sl], prof_lvl3=fx.prof[2][sl]) for sl in parts]
    assert m.training and torch.is_grad_enabled()
    got = gr_amd.tiger_prefix.eval_loss(m, batches, dev)
    assert m.training and torch.is_grad_enabled() and isinstance(got, float)
    sd64 = fx.sd_as(torch.float64)
    want = [fref.forward_prefix(fx.cfg, sd64, fx.ids[sl], fx.mask[sl], [p[sl].double() for p in fx.prof],
                                r.labels[sl])[0].item() for sl in parts]
    mean = sum(want) / 2
    tol = r.nll_tol + 2.0 ** -23 * abs(mean)
    print(f"eval_loss {got:.7f} vs float64 {mean:.9f} (halves {want}): err {abs(got - mean):.3e} (tolerance {tol:.3e})")
    assert abs(got - mean) <= tol
