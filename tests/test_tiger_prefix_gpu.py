"""The TIGER prefix variant on the GPU (csrc/tiger.hip: tiger_adapter_kernel, then the encoder and search
kernels on S + 3 positions) against the float64 restatement tests/tiger_prefix_ref.py.

Tolerances are 4 x the float32 reference's own worst distance from float64 on the same fixture, per
class (the rule of test_tiger_gpu.py); the generator measured them and stored them in each fixture's
meta:

    fixture                prefix_err32   enc_err32   logit_err32   score_err32 (m = 4 x)   certified
    tiger_prefix_main      3.61e-07       3.63e-07    5.71e-07      7.24e-07                16/16
    tiger_prefix_bert768   1.75e-07       3.81e-07    3.38e-07      2.52e-07                8/8
    tiger_prefix_h2_s125   2.80e-07       4.92e-07    7.36e-07      4.90e-07                8/8

(prefix tokens and hidden states relative to the tensor's largest magnitude, logits relative to the row
scale, scores absolute; no user of these fixtures stops early).  A user is certified when every
selection gap of the float64 run clears m; certified users must match the restatement exactly, in
order.  A mean over the unmasked rows only would move user 0's prefix tokens by about 1.0 of that scale.
"""
import numpy as np
import pytest
import torch

import tiger_prefix_fixtures as tpf
import tiger_prefix_ref as pref

pytestmark = pytest.mark.gpu


def _binding(fx, dev):
    import gr_amd
    t5 = {k: v.to(dev) for k, v in fx.t5().items() if k not in fx.meta["tied"]}
    for k in fx.meta["tied"]:
        t5[k] = t5["shared.weight"]
    return gr_amd.ops.TigerPrefixBinding(fx.cfg, t5, {k: v.to(dev) for k, v in fx.adapters().items()})


def _module(fx, dev):
    import gr_amd
    m = gr_amd.tiger_prefix.TIGER(fx.cfg)
    m.load_state_dict(fx.state_dict())
    return m.to(dev).eval()


_RUNS = {}


def _run(name, dev):
    """One ops call per fixture with the prefix tokens, the encoder output and the step logits, shared by
    the tests."""
    if name not in _RUNS:
        import gr_amd
        fx = tpf.fixture(name)
        out = gr_amd.ops.tiger_generate_prefix(_binding(fx, dev), fx.ids.to(dev), fx.mask.to(dev),
                                               *[p.to(dev) for p in fx.prof], fx.beams, fx.T, with_prefix=True,
                                               with_encoder=True, with_logits=True)
        _RUNS[name] = tuple(t.cpu() for t in out)
    return _RUNS[name]


@pytest.mark.parametrize("name", tpf.NAMES)
def test_prefix_encoder_and_step_logits_against_float64(name, dev):
    fx = tpf.fixture(name)
    seqs, scores, prefix, enc, logits = _run(name, dev)
    _, _, _, tr = tpf.restated(name, torch.float64)
    p64 = tr["prefix"]
    assert prefix.shape == p64.shape == (fx.ids.shape[0], 3, fx.cfg["d_model"])
    err = ((prefix.double() - p64).abs().max() / p64.abs().max()).item()
    tol = 4 * fx.meta["prefix_err32"]
    print(f"{name}: prefix err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    live = pref.extend(fx.ids, fx.mask)[1].bool()               # the prefix rows and the unmasked rows
    assert live[:, :3].all()
    e64 = tr["enc"]
    assert enc.shape == e64.shape
    err = ((enc.double() - e64)[live].abs().max() / e64[live].abs().max()).item()
    tol = 4 * fx.meta["enc_err32"]
    print(f"{name}: encoder err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    cert = torch.from_numpy(fx.out["certified"])
    tol = 4 * fx.meta["logit_err32"]
    worst = 0.0
    stopped = tr["stopped_after"]
    for t, (l64, nlive) in enumerate(zip(tr["logits"], tr["live"])):
        on = cert & ((stopped < 0) | (stopped > t))
        got = logits[:, t, :nlive].double()
        e = ((got - l64).abs().amax(-1) / l64.abs().amax(-1))[on]
        worst = max(worst, e.max().item())
    print(f"{name}: step-logit err {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol


@pytest.mark.parametrize("name", tpf.NAMES)
def test_beam_results(name, dev):
    fx = tpf.fixture(name)
    seqs, scores = _run(name, dev)[:2]
    s64, c64 = torch.from_numpy(fx.out["sequences64"]), torch.from_numpy(fx.out["scores64"])
    cert = torch.from_numpy(fx.out["certified"])
    assert cert.float().mean() >= 0.9
    bad = [b for b in range(len(cert)) if cert[b] and not torch.equal(seqs[b], s64[b])]
    d = (scores.double() - c64)[cert].abs().max().item()
    print(f"{name}: {int(cert.sum())}/{len(cert)} certified, users differing {bad}, score err {d:.3e} (m {fx.m:.3e})")
    assert not bad
    assert d <= fx.m
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    with torch.no_grad():
        r = pref.rescore(fx.cfg, fx.sd_as(torch.float64), fx.ids, fx.mask, [p.double() for p in fx.prof], seqs)
    d = (r - scores.double()).abs().max().item()
    print(f"{name}: re-scored hypotheses differ by {d:.3e}")
    assert d <= fx.m
    assert bool((seqs[:, :, 0] == fx.cfg["pad_token_id"]).all())


@pytest.mark.parametrize("name", ["tiger_prefix_main", "tiger_prefix_bert768"])
def test_without_all_three_prof_it_is_the_plain_model(name, dev):
    import gr_amd
    fx = tpf.fixture(name)
    m = _module(fx, dev)
    plain = gr_amd.TIGER(fx.cfg)
    plain.load_state_dict({k: v for k, v in fx.state_dict().items() if k.startswith("model.")})
    plain = plain.to(dev).eval()
    ids, mask = fx.ids.to(dev), fx.mask.to(dev)
    p = [t.to(dev) for t in fx.prof]
    want_s, want_c = plain.generate_scored(ids, mask, fx.beams)
    assert not torch.equal(want_s.cpu(), _run(name, dev)[0])
    for kw in (dict(), dict(prof_lvl1=p[0], prof_lvl2=p[1]), dict(prof_lvl1=p[0], prof_lvl3=p[2]),
               dict(prof_lvl2=p[1], prof_lvl3=p[2])):
        s, c = m.generate_scored(ids, mask, fx.beams, **kw)
        assert torch.equal(s, want_s) and torch.equal(c.view(torch.int32), want_c.view(torch.int32))
        assert torch.equal(m.generate(ids, mask, num_beams=fx.beams, **kw), want_s.view(-1, fx.T))


def test_batch_independence_and_repeatability(dev):
    import gr_amd
    fx = tpf.fixture("tiger_prefix_main")
    bind = _binding(fx, dev)
    full = _run("tiger_prefix_main", dev)
    ids, mask, prof = fx.ids.to(dev), fx.mask.to(dev), [p.to(dev) for p in fx.prof]
    bits = lambda t: t.view(torch.int32)
    again = gr_amd.ops.tiger_generate_prefix(bind, ids, mask, *prof, fx.beams, fx.T, with_prefix=True,
                                             with_encoder=True, with_logits=True)
    for a, b in zip(again, full):
        assert torch.equal(a.cpu() if a.dtype == torch.int64 else bits(a.cpu()), b if b.dtype == torch.int64 else bits(b))
    for B, at in [(1, 0), (3, 2), (17, 9)]:
        order = torch.arange(B) % ids.shape[0]
        order[at] = 5                                   # user 5 at position `at` of a batch of B
        o = order.to(dev)
        s, c, p = gr_amd.ops.tiger_generate_prefix(bind, ids[o], mask[o], *[t[o] for t in prof], fx.beams, fx.T,
                                                   with_prefix=True)
        s, c, p = s.cpu(), c.cpu(), p.cpu()
        assert torch.equal(s[at], full[0][5]) and torch.equal(bits(c[at]), bits(full[1][5]))
        assert torch.equal(s, full[0][order]) and torch.equal(bits(c), bits(full[1][order]))
        assert torch.equal(bits(p), bits(full[2][order]))


def test_each_level_uses_its_own_weights(dev):
    """prof_lvl1 and prof_lvl2 swapped: prefix rows 0 and 1 move to what the restatement gives for the swap."""
    import gr_amd
    fx = tpf.fixture("tiger_prefix_main")
    ids, mask, prof = fx.ids.to(dev), fx.mask.to(dev), [p.to(dev) for p in fx.prof]
    prefix = gr_amd.ops.tiger_generate_prefix(_binding(fx, dev), ids, mask, prof[1], prof[0], prof[2], fx.beams, fx.T,
                                              with_prefix=True)[2].cpu()
    p64 = [p.double() for p in fx.prof]
    with torch.no_grad():
        want = pref.prefix_tokens(fx.cfg, fx.sd_as(torch.float64), fx.ids, [p64[1], p64[0], p64[2]])
    scale = want.abs().max()
    tol = 4 * fx.meta["prefix_err32"]
    assert ((prefix.double() - want).abs().max() / scale) <= tol
    straight = _run("tiger_prefix_main", dev)[2]
    assert ((straight[:, :2].double() - want[:, :2]).abs().max() / scale) > 100 * tol
    assert torch.equal(straight[:, 2].view(torch.int32), prefix[:, 2].view(torch.int32))


def test_module_matches_ops_and_sees_weight_updates(dev):
    fx = tpf.fixture("tiger_prefix_main")
    m = _module(fx, dev)
    ids, mask = fx.ids.to(dev), fx.mask.to(dev)
    kw = {f"prof_lvl{i + 1}": p.to(dev) for i, p in enumerate(fx.prof)}
    full_s, full_c = _run("tiger_prefix_main", dev)[:2]
    flat = m.generate(ids, mask, num_beams=fx.beams, **kw)
    assert flat.shape == (ids.shape[0] * fx.beams, fx.T) and flat.dtype == torch.int64
    assert torch.equal(flat.cpu(), full_s.view(-1, fx.T))
    s, c = m.generate_scored(ids, mask, fx.beams, **kw)
    assert torch.equal(s.cpu(), full_s) and torch.equal(c.cpu(), full_c)
    # no host round trip once the binding caches are filled
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        s2, c2 = m.generate_scored(ids, mask, fx.beams, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(s2.cpu(), full_s) and torch.equal(c2.cpu(), full_c)
    # an in-place update of an adapter bias is seen by the next call: the float64 restatement on the new weights
    bind = m.prefix_binding()
    delta = torch.linspace(-2.0, 2.0, fx.cfg["d_model"])
    with torch.no_grad():
        m.adapter_lvl2.ffn[2].bias += delta.to(dev)
    assert m.prefix_binding() is bind
    import gr_amd
    s3, c3, p3 = gr_amd.ops.tiger_generate_prefix(bind, ids, mask, *kw.values(), fx.beams, fx.T, with_prefix=True)
    sd = dict(fx.sd_as(torch.float64))
    sd["adapter_lvl2.ffn.2.bias"] = sd["adapter_lvl2.ffn.2.bias"] + delta.double()
    tr = {}
    with torch.no_grad():
        r, rc, _ = pref.beam_search(fx.cfg, sd, fx.ids, fx.mask, [p.double() for p in fx.prof], fx.beams, fx.T, trace=tr)
    err = ((p3.cpu().double() - tr["prefix"]).abs().max() / tr["prefix"].abs().max()).item()
    assert err <= 4 * fx.meta["prefix_err32"]
    old = _run("tiger_prefix_main", dev)[2]
    assert torch.equal(p3.cpu()[:, 0], old[:, 0]) and not torch.equal(p3.cpu()[:, 1], old[:, 1])
    ok = tr["gaps"] > fx.m
    assert ok.sum() >= 12
    assert torch.equal(s3.cpu()[ok], r[ok]) and (c3.cpu().double() - rc)[ok].abs().max() <= fx.m
    s4, _ = m.generate_scored(ids, mask, fx.beams, **kw)
    assert torch.equal(s4, s3)


@pytest.mark.parametrize("name", ["tiger_prefix_main", "tiger_prefix_h2_s125"])
def test_evaluate_model_reproduces_the_reference_metrics(name, dev):
    import gr_amd
    fx = tpf.fixture(name)
    m = _module(fx, dev)
    half = fx.ids.shape[0] // 2
    batches = [dict(history=fx.ids[sl], attention_mask=fx.mask[sl], target=fx.labels[sl], prof_lvl1=fx.prof[0][sl],
                    prof_lvl2=fx.prof[1][sl], prof_lvl3=fx.prof[2][sl]) for sl in (slice(0, half), slice(half, None))]
    rec, nd = gr_amd.tiger_prefix.evaluate_model(m, batches, fx.meta["topk_list"], 5)
    assert fx.meta["reference_metrics_ran"] and rec == fx.meta["recall"] and nd == fx.meta["ndcg"]
    assert rec["Recall@20"] > 0
