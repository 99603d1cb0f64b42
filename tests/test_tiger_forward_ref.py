"""The oracle of the TIGER teacher-forced forward tests (CPU): tests/tiger_forward_ref.py against the values the
reference's own ``TIGER.forward`` gave in eval mode (tests/golden/tiger_fwd_*.npz), and its rules on hand-made
rows -- the shift to the right, -100, the two NaN cases."""
import math

import pytest
import torch

import tiger_fixtures as tf
import tiger_forward_cases as fc
import tiger_forward_ref as fref


def _restate(r, dtype):
    fx = r.fx
    if r.prefixed:
        return fref.forward_prefix(fx.cfg, fx.sd_as(dtype), fx.ids, fx.mask, [p.to(dtype) for p in fx.prof], r.labels)
    return fref.forward(fx.cfg, fx.sd_as(dtype), fx.ids, fx.mask, r.labels)


@pytest.mark.parametrize("source", fc.PLAIN_FIXTURES + fc.PREFIX_FIXTURES)
def test_restatement_is_the_reference(source):
    """float32: the generator's own bounds (logits 1e-5 row-scaled, loss 1e-6 relative); float64: the stored run."""
    r = fc.recorded(source)
    lab = r.labels
    assert lab[0, -1] == -100 and (lab[1, 1:] == -100).all() and (lab[2] == -100).all() and lab[3, 1] == -100
    assert lab[3, 2] != -100 and lab[1, 0] != -100 and int((lab != -100).sum()) == r.meta["counted"]
    loss, logits, nll = _restate(r, torch.float32)
    d = ((logits - r.logits).abs().amax(-1) / r.logits.abs().amax(-1)).max().item()
    assert logits.dtype == torch.float32 and d <= 1e-5
    assert abs(loss.item() - r.loss.item()) <= 1e-6 * abs(r.loss.item())
    loss64, logits64, nll64 = _restate(r, torch.float64)
    assert torch.equal(logits64, r.logits64) or (logits64 - r.logits64).abs().max() <= 1e-12
    assert abs(loss64.item() - r.loss64.item()) <= 1e-12 and (nll64 - r.nll64).abs().max() <= 1e-12
    # the stored tolerances are the reference's own distances from float64
    le = ((r.logits.double() - r.logits64).abs().amax(-1) / r.logits64.abs().amax(-1)).max().item()
    assert le == pytest.approx(r.meta["logit_err32"], rel=1e-9) and 0 < r.meta["nll_err32"] < 1e-5
    assert not nll64[lab == -100].any() and (nll64[lab != -100] > 0).all()
    assert loss64.item() == pytest.approx(nll64.sum().item() / r.meta["counted"], rel=1e-12)


def test_shift_right_and_ignore_rules_on_a_hand_made_row():
    fx = tf.fixture("tiger_d32_b5")
    pad = int(fx.cfg["pad_token_id"])
    labels = torch.tensor([[7, -100, 9, 4], [5, 6, -100, -100]])
    assert fref.shift_right(labels, pad).tolist() == [[pad, 7, pad, 9], [pad, 5, 6, pad]]
    assert fref.shift_right(labels, 3).tolist() == [[3, 7, 3, 9], [3, 5, 6, 3]]
    sd = fx.sd_as(torch.float64)
    ids, mask = fx.ids[:2], fx.mask[:2]
    loss, logits, nll = fref.forward(fx.cfg, sd, ids, mask, labels)
    # the same logits from the decoder input written out by hand, and torch's own cross-entropy on them
    m = fref.tiger_ref.Model(fx.cfg, sd)
    with torch.no_grad():
        want = m.decode(torch.tensor([[pad, 7, pad, 9], [pad, 5, 6, pad]]), m.cross_kv(m.encode(ids, mask)), mask)
    assert torch.equal(logits, want)
    ce = torch.nn.functional.cross_entropy(want.view(-1, want.shape[-1]), labels.view(-1), ignore_index=-100)
    assert loss.item() == pytest.approx(ce.item(), rel=1e-14)
    assert nll[0, 1] == 0 and nll[1, 2] == 0 and nll[1, 3] == 0 and (nll != 0).sum() == 5
    # an ignored label changes no other position's logits' inputs except through the shifted pad token
    labels2 = labels.clone()
    labels2[0, 3] = -100                                 # the last label is never a decoder input
    loss2, logits2, nll2 = fref.forward(fx.cfg, sd, ids, mask, labels2)
    assert torch.equal(logits2, logits) and nll2[0, 3] == 0
    assert loss2.item() == pytest.approx((nll.sum() - nll[0, 3]).item() / 4, rel=1e-14)
    # attention_mask=None is the all-ones mask
    a = fref.forward(fx.cfg, sd, ids, None, labels)
    b = fref.forward(fx.cfg, sd, ids, torch.ones_like(ids), labels)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


def test_no_counted_token_gives_nan():
    fx = tf.fixture("tiger_d32_b5")
    labels = torch.full((3, 4), -100)
    loss, logits, nll = fref.forward(fx.cfg, fx.sd, fx.ids[:3], fx.mask[:3], labels)
    assert math.isnan(loss.item()) and not nll.any() and bool(torch.isfinite(logits).all())
    ce = torch.nn.functional.cross_entropy(logits.view(-1, logits.shape[-1]), labels.view(-1), ignore_index=-100)
    assert math.isnan(ce.item())


@pytest.mark.parametrize("bad", [-1, -99, 64, 1 << 40])
def test_out_of_range_label_gives_nan(bad):
    fx = tf.fixture("tiger_d32_b5")
    V = int(fx.cfg["vocab_size"])
    assert V == 64
    labels = fx.labels[:3].clone()
    labels[1, 1] = bad
    loss, logits, nll = fref.forward(fx.cfg, fx.sd, fx.ids[:3], fx.mask[:3], labels)
    assert math.isnan(loss.item()) and math.isnan(nll[1, 1].item()) and int(torch.isnan(nll).sum()) == 1
    assert bool(torch.isfinite(logits).all())
    # the embedding read of the shifted row uses the clamped id
    clamped = labels.clone()
    clamped[1, 1] = min(max(bad, 0), V - 1)
    assert torch.equal(fref.forward(fx.cfg, fx.sd, fx.ids[:3], fx.mask[:3], clamped)[1], logits)


@pytest.mark.parametrize("name", fc.NAMES + fc.PREFIX_NAMES)
def test_every_seeded_case_counts_a_token(name):
    c = fc.case(name)
    counted = c.labels != -100
    assert counted.any() and c.labels.shape == (c.B, c.Ld)
    assert bool(((c.labels == -100) | ((c.labels >= 0) & (c.labels < c.cfg["vocab_size"]))).all())
    if c.B > 3:
        assert not counted[2].any() and c.labels[3, 1] == -100 and c.labels[3, 2] != -100


def test_seeded_cases_reach_what_they_name():
    one, mx, d32, holes, pfx = (fc.case(n) for n in ("fwd_one", "fwd_max", "fwd_d32", "fwd_holes", "fwd_pfx"))
    assert (one.B, one.S, one.Ld, one.cfg["vocab_size"]) == (1, 1, 1, 2)
    assert (mx.B, mx.S, mx.Ld, mx.cfg["vocab_size"], mx.cfg["d_ff"]) == (6, 128, 8, 128, 256) and bool(mx.mask.all())
    assert mx.cfg["num_layers"] == mx.cfg["num_decoder_layers"] == 4 and mx.cfg["num_heads"] * mx.cfg["d_kv"] == 64
    assert (d32.cfg["d_model"], d32.cfg["num_heads"], d32.cfg["d_kv"], d32.cfg["vocab_size"], d32.Ld) == (32, 1, 32, 65, 3)
    assert holes.cfg["pad_token_id"] == 3 and int(holes.mask[1].sum()) == 1 and not bool(holes.mask.all())
    assert fref.shift_right(holes.labels, 3)[:, 0].eq(3).all()
    assert fc.case("fwd_nomask").mask is None and fc.case("fwd_nomask").ids is mx.ids
    assert (pfx.S, pfx.n_vec, pfx.Ld) == (125, 16, 8) and int(pfx.mask[1].sum()) == 1
    for n in fc.NAMES + fc.PREFIX_NAMES:
        m = fc.measured(n)
        print(f"{n}: logit_err32 {m['logit_err32']:.3e}, nll_err32 {m['nll_err32']:.3e}")
        assert 0 < m["logit_err32"] < 1e-5 and 0 <= m["nll_err32"] < 1e-5
