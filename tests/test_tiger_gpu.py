"""TIGER on the GPU (csrc/tiger.hip) against the float64 restatement tests/tiger_ref.py.

Tolerances are 4 x the float32 reference's own worst distance from float64 on the same fixture, per
class (the rule of test_sasrec_infer_fp64_gpu.py); the generator measured them and stored them in
each fixture's meta:

    fixture          enc_err32   logit_err32   score_err32 (m = 4 x)   certified   stop early
    tiger_main       3.43e-07    5.31e-07      9.31e-07                32/32       0
    tiger_eos        3.72e-07    8.33e-07      8.52e-07                32/32       0
    tiger_h2_ff128   2.79e-07    6.65e-07      5.82e-07                16/16       0
    tiger_v40_len3   3.33e-07    5.13e-07      4.43e-07                16/16       0
    tiger_d32_b5     2.64e-07    5.05e-07      3.83e-07                16/16       0
    tiger_stop       3.57e-07    8.89e-07      1.67e-06                32/32       31/32

(hidden states relative to the tensor's largest magnitude, logits relative to the row scale, scores
absolute).  A user is certified when every selection gap of the float64 run clears m; certified
users must match the restatement exactly, in order.  A user whose early-stop heuristic is satisfied
after step s runs no further step in the kernel: its step logits are compared up to step s only.
"""
import numpy as np
import pytest
import torch

import tiger_fixtures as tf
import tiger_ref

pytestmark = pytest.mark.gpu


def _binding(fx, dev):
    import gr_amd
    tensors = {k: v.to(dev) for k, v in fx.sd.items() if k not in fx.meta["tied"]}
    for k in fx.meta["tied"]:
        tensors[k] = tensors["shared.weight"]
    return gr_amd.ops.TigerBinding(fx.cfg, tensors)


_RUNS = {}


def _run(name, dev):
    """One ops call per fixture with the encoder output and the step logits, shared by the tests."""
    if name not in _RUNS:
        import gr_amd
        fx = tf.fixture(name)
        out = gr_amd.ops.tiger_generate(_binding(fx, dev), fx.ids.to(dev), fx.mask.to(dev), fx.beams, fx.T,
                                        with_encoder=True, with_logits=True)
        _RUNS[name] = tuple(t.cpu() for t in out)
    return _RUNS[name]


@pytest.mark.parametrize("name", tf.NAMES)
def test_encoder_and_step_logits_against_float64(name, dev):
    fx = tf.fixture(name)
    seqs, scores, enc, logits = _run(name, dev)
    _, _, _, tr = tf.restated(name, torch.float64)
    live = fx.mask.bool()
    e64 = tr["enc"]
    err = ((enc.double() - e64)[live].abs().max() / e64[live].abs().max()).item()
    tol = 4 * fx.meta["enc_err32"]
    print(f"{name}: encoder err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    cert = torch.from_numpy(fx.out["certified"])
    tol = 4 * fx.meta["logit_err32"]
    worst = 0.0
    stopped = tr["stopped_after"]
    for t, (l64, nlive) in enumerate(zip(tr["logits"], tr["live"])):
        on = cert & ((stopped < 0) | (stopped > t))          # the users whose search runs step t
        got = logits[:, t, :nlive].double()
        e = ((got - l64).abs().amax(-1) / l64.abs().amax(-1))[on]
        worst = max(worst, e.max().item())
        off = ~((stopped < 0) | (stopped > t))
        assert not logits[off, t].any(), "a stopped user ran another step"
        assert logits[on, t, :nlive].abs().amax((-1, -2)).gt(0).all()
    print(f"{name}: step-logit err {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol


@pytest.mark.parametrize("name", tf.NAMES)
def test_beam_results(name, dev):
    fx = tf.fixture(name)
    seqs, scores, _, _ = _run(name, dev)
    s64, c64 = torch.from_numpy(fx.out["sequences64"]), torch.from_numpy(fx.out["scores64"])
    cert = torch.from_numpy(fx.out["certified"])
    assert cert.float().mean() >= 0.9
    bad = [b for b in range(len(cert)) if cert[b] and not torch.equal(seqs[b], s64[b])]
    d = (scores.double() - c64)[cert].abs().max().item()
    print(f"{name}: {int(cert.sum())}/{len(cert)} certified, users differing {bad}, score err {d:.3e} (m {fx.m:.3e})")
    assert not bad
    assert d <= fx.m
    # every user: descending scores, and each hypothesis re-scored by teacher forcing in float64
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    with torch.no_grad():
        r = tiger_ref.rescore(fx.cfg, fx.sd_as(torch.float64), fx.ids, fx.mask, seqs)
    d = (r - scores.double()).abs().max().item()
    print(f"{name}: re-scored hypotheses differ by {d:.3e}")
    assert d <= fx.m
    assert bool((seqs[:, :, 0] == fx.cfg["pad_token_id"]).all())


def test_eos_fill_is_reproduced(dev):
    fx = tf.fixture("tiger_eos")
    seqs = _run("tiger_eos", dev)[0]
    eos = fx.cfg["eos_token_id"]
    early = [r for r in seqs.view(-1, fx.T).tolist() if eos in r[1:fx.T - 1]]
    ref = [r for r in fx.out["sequences"].reshape(-1, fx.T).tolist() if eos in r[1:fx.T - 1]]
    assert early and early == ref
    assert np.array_equal(seqs.numpy(), fx.out["sequences"])


def test_early_stop_and_the_library_crop(dev):
    """tiger_stop: 31 of 32 users stop at step 2 or 3.  Their hypotheses are the reference's, and a batch
    in which every user stops early compares, in the metric tail, as the library's cropped and
    zero-padded result does."""
    import gr_amd
    fx = tf.fixture("tiger_stop")
    seqs = _run("tiger_stop", dev)[0]
    st = torch.from_numpy(fx.out["stopped_after"])
    assert ((st > 0) & (st < fx.T - 1)).sum() * 4 >= len(st)
    assert np.array_equal(seqs.numpy(), fx.out["sequences"])
    sub = torch.nonzero(st == 2)[:6, 0]
    with torch.no_grad():
        ref = tiger_ref.generate(fx.cfg, fx.sd, fx.ids[sub], fx.mask[sub], fx.beams, fx.T)     # cropped
    width = ref.shape[1]
    assert width == 3
    padded = torch.cat([ref, torch.zeros(ref.shape[0], fx.T - width, dtype=torch.int64)], 1).view(len(sub), fx.beams, fx.T)
    got = gr_amd.tiger.crop_like_library(seqs[sub].to(dev), fx.cfg["eos_token_id"])
    assert torch.equal(got.cpu(), padded)
    labels = padded[:, 3, 1:].clone()                     # beam 3 of each user, as evaluate_model sees it
    want = tiger_ref.pos_index(padded[:, :, 1:], labels)
    assert want.any(1).all()
    assert torch.equal(gr_amd.ops.beam_hits(got, labels.to(dev), skip=1).cpu(), want)
    assert not torch.equal(gr_amd.ops.beam_hits(seqs[sub].to(dev), labels.to(dev), skip=1).cpu(), want)


def test_batch_independence(dev):
    import gr_amd
    fx = tf.fixture("tiger_main")
    bind = _binding(fx, dev)
    full_s, full_c = _run("tiger_main", dev)[:2]
    ids, mask = fx.ids.to(dev), fx.mask.to(dev)
    for B, at in [(1, 0), (3, 2), (33, 17)]:
        order = torch.arange(B) % ids.shape[0]
        order[at] = 5                                   # user 5 at position `at` of a batch of B
        s, c = gr_amd.ops.tiger_generate(bind, ids[order.to(dev)], mask[order.to(dev)], fx.beams, fx.T)
        s, c = s.cpu(), c.cpu()
        assert torch.equal(s[at], full_s[5]) and torch.equal(c[at].view(torch.int32), full_c[5].view(torch.int32))
        assert torch.equal(s, full_s[order]) and torch.equal(c.view(torch.int32), full_c[order].view(torch.int32))


def test_module_matches_ops_and_sees_weight_updates(dev):
    import gr_amd
    fx = tf.fixture("tiger_main")
    m = gr_amd.TIGER(fx.cfg)
    m.load_state_dict(fx.state_dict())
    m = m.to(dev).eval()
    ids, mask = fx.ids.to(dev), fx.mask.to(dev)
    full_s, full_c = _run("tiger_main", dev)[:2]
    flat = m.generate(ids, mask, num_beams=fx.beams)
    assert flat.shape == (ids.shape[0] * fx.beams, fx.T) and flat.dtype == torch.int64
    assert torch.equal(flat.cpu(), full_s.view(-1, fx.T))
    s, c = m.generate_scored(ids, mask, fx.beams)
    assert torch.equal(s.cpu(), full_s) and torch.equal(c.cpu(), full_c)
    # no host round trip once the binding caches are filled
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        s2, c2 = m.generate_scored(ids, mask, fx.beams)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(s2.cpu(), full_s) and torch.equal(c2.cpu(), full_c)
    # an in-place update is seen by the next call: the float64 restatement on the new weights
    bind = m.binding()
    with torch.no_grad():
        m.model.shared.weight[1:9] *= 1.5
    assert m.binding() is bind
    s3, c3 = m.generate_scored(ids[:8], mask[:8], fx.beams)
    sd = {k: v.clone() for k, v in fx.sd_as(torch.float64).items()}
    new = sd["shared.weight"].clone()
    new[1:9] *= 1.5
    for k in ["shared.weight"] + fx.meta["tied"]:
        sd[k] = new
    tr = {}
    with torch.no_grad():
        r, rc, _ = tiger_ref.beam_search(fx.cfg, sd, fx.ids[:8], fx.mask[:8], fx.beams, fx.T, trace=tr)
    ok = tr["gaps"] > fx.m
    assert ok.sum() >= 6 and not torch.equal(s3.cpu(), full_s[:8])
    assert torch.equal(s3.cpu()[ok], r[ok]) and (c3.cpu().double() - rc)[ok].abs().max() <= fx.m


def _hits_case():
    k, T = 20, 5
    g = torch.Generator().manual_seed(3)
    preds = torch.randint(1, 60, (6, k, T), generator=g)
    preds[:, :, 0] = 0
    labels = torch.randint(60, 64, (6, 4), generator=g)      # no hit unless planted
    labels[0] = preds[0, 0, 1:]                              # hit at beam 0
    labels[1] = preds[1, k - 1, 1:]                          # hit at the last beam
    preds[3, 4] = preds[3, 9]                                # duplicate beams: the first one counts
    preds[3, 15] = preds[3, 9]
    labels[3] = preds[3, 9, 1:]
    labels[4] = preds[4, 7, 1:]
    labels[5, 0] = -100                                      # a padded label never matches
    return preds, labels


def test_beam_hits_on_constructed_cases(dev):
    import gr_amd
    preds, labels = _hits_case()
    want = tiger_ref.pos_index(preds[:, :, 1:], labels)
    got = gr_amd.ops.beam_hits(preds.to(dev), labels.to(dev), skip=1).cpu()
    assert got.dtype == torch.bool and torch.equal(got, want)
    assert want[0, 0] and want[1, 19] and not want[2].any() and want[3, 4] and want[3].sum() == 1 and want[4, 7]
    # predictions shorter than the labels are zero-padded, longer ones are cut (evaluate_model)
    wide = torch.cat([labels, torch.zeros(6, 2, dtype=torch.int64)], 1)
    wide[2, 5] = 9
    padded = torch.cat([preds[:, :, 1:], torch.zeros(6, 20, 2, dtype=torch.int64)], -1)
    assert torch.equal(gr_amd.ops.beam_hits(preds.to(dev), wide.to(dev), skip=1).cpu(), tiger_ref.pos_index(padded, wide))
    narrow = labels[:, :2].contiguous()
    assert torch.equal(gr_amd.ops.beam_hits(preds.to(dev), narrow.to(dev), skip=1).cpu(),
                       tiger_ref.pos_index(preds[:, :, 1:3], narrow))


@pytest.mark.parametrize("name", ["tiger_main", "tiger_h2_ff128"])
def test_evaluate_model_reproduces_the_reference_metrics(name, dev):
    import gr_amd
    fx = tf.fixture(name)
    m = gr_amd.TIGER(fx.cfg)
    m.load_state_dict(fx.state_dict())
    m = m.to(dev).eval()
    half = fx.ids.shape[0] // 2
    batches = [dict(history=fx.ids[sl], attention_mask=fx.mask[sl], target=fx.labels[sl])
               for sl in (slice(0, half), slice(half, None))]
    rec, nd = gr_amd.tiger.evaluate_model(m, batches, fx.meta["topk_list"], 5)
    assert rec == fx.meta["recall"] and nd == fx.meta["ndcg"]
