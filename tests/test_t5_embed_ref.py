"""The plain-torch restatement of the T5 embedding retriever (tests/t5_embed_ref.py) against the recorded runs
of the reference (tests/golden/t5e_*.npz), on the CPU."""
import pytest
import torch

import t5_embed_fixtures as tf
import t5_embed_ref as ref


@pytest.mark.parametrize("name", tf.NAMES)
def test_float32_restatement_is_the_reference(name):
    fx = tf.fixture(name)
    with torch.no_grad():
        pred, hidden, _ = ref.forward(fx.cfg, fx.sd, fx.seq, fx.mask, torch.float32)
    assert ref.live_err(pred, torch.from_numpy(fx.out["pred"])) <= 1e-6
    assert ref.live_err(hidden, torch.from_numpy(fx.out["hidden"]), fx.mask) <= 1e-6


@pytest.mark.parametrize("name", tf.NAMES)
def test_float64_restatement_is_the_recorded_yardstick(name):
    fx = tf.fixture(name)
    with torch.no_grad():
        pred, hidden, _ = ref.forward(fx.cfg, fx.sd, fx.seq, fx.mask, torch.float64)
    assert ref.live_err(pred, fx.pred64) <= 1e-12
    assert ref.live_err(hidden, fx.hidden64, fx.mask) <= 1e-12
    # the reference sits within its recorded distance of it
    assert ref.live_err(torch.from_numpy(fx.out["pred"]), pred) <= fx.meta["pred_err32"] * (1 + 1e-6)
    assert torch.allclose(pred.norm(dim=1), torch.ones(len(pred), dtype=torch.float64), atol=1e-12)


@pytest.mark.parametrize("name", tf.NAMES)
def test_wrong_models_are_far_from_the_margin(name):
    """The 1/sqrt(d_kv) scale and a bias read at query - key each move pred by more than 100 x the float32
    reference's error, so the GPU tests' 4 x margin separates them."""
    fx = tf.fixture(name)
    for variant in ("scaled", "flipped"):
        with torch.no_grad():
            pv, _, _ = ref.forward(fx.cfg, fx.sd, fx.seq, fx.mask, torch.float64, variant=variant)
        assert ref.live_err(pv, fx.pred64) > 100 * fx.meta["pred_err32"], variant


def test_buckets():
    r = torch.arange(-127, 128)
    b = ref.bucket(r)
    assert b[127].item() == 0 and b[127 + 1].item() == 17 and b[127 - 1].item() == 1
    assert b[127 + 7].item() == 16 + 7 and b[127 - 7].item() == 7
    assert b.min().item() == 0 and b.max().item() == 31 and b[0].item() == 15 and b[-1].item() == 31
    assert (b[127:].diff() >= 0).all() and (b[:128].flip(0).diff() >= 0).all()
    from gr_amd import ops
    assert torch.equal(b, ops.t5_relative_bucket(r, True))


def test_padding_is_inert_and_an_empty_user_is_the_bias():
    fx = tf.fixture("t5e_peaked")
    noisy = fx.seq.clone()
    noisy[~fx.mask.bool()] = 5.0 * torch.randn(int((~fx.mask.bool()).sum()), fx.seq.shape[-1],
                                               generator=torch.Generator().manual_seed(1))
    zero = fx.seq.clone()
    zero[~fx.mask.bool()] = 0.0
    mask = fx.mask.clone()
    mask[3] = 0
    with torch.no_grad():
        a, _, _ = ref.forward(fx.cfg, fx.sd, noisy, mask, torch.float64)
        b, _, _ = ref.forward(fx.cfg, fx.sd, zero, mask, torch.float64)
    keep = torch.arange(len(mask)) != 3
    assert torch.equal(a[keep], b[keep])
    bias = fx.sd["output_proj.bias"].double()
    assert torch.allclose(a[3], bias / bias.norm(), atol=1e-12) and torch.allclose(b[3], a[3], atol=1e-12)


def test_loss_restatement_matches_the_reference():
    fx = tf.fixture("t5e_main")
    loss = ref.info_nce(torch.from_numpy(fx.out["pred"]), fx.target, fx.cfg["temperature"]).item()
    assert abs(loss - fx.meta["loss"]) <= 1e-5 * abs(fx.meta["loss"])
