"""The plain-torch restatement tests/tiger_prefix_ref.py against the reference's stored results
(tests/golden/tiger_prefix_*.npz, made by make_golden_tiger_prefix.py), at the generator's bars: float32
sequences equal on every user, scores within 1e-6, prefix tokens and encoder output within 1e-5; the
float64 run's certified users equal the stored float64 sequences."""
import numpy as np
import pytest
import torch

import tiger_prefix_fixtures as tpf
import tiger_prefix_ref as pref


@pytest.mark.parametrize("name", tpf.NAMES)
def test_float32_restatement_equals_the_reference(name):
    fx = tpf.fixture(name)
    s, c, width, tr = tpf.restated(name, torch.float32)
    assert width == fx.T
    assert np.array_equal(s.numpy(), fx.out["sequences"])
    assert (c - torch.from_numpy(fx.out["sequences_scores"])).abs().max() <= 1e-6
    assert (tr["prefix"] - torch.from_numpy(fx.out["prefix"])).abs().max() <= 1e-5
    n = fx.meta["enc_users"]
    live = pref.extend(fx.ids, fx.mask)[1][:n].bool()
    assert (tr["enc"][:n] - torch.from_numpy(fx.out["encoder_output"]))[live].abs().max() <= 1e-5
    assert tr["enc"].shape[1] == fx.ids.shape[1] + 3


@pytest.mark.parametrize("name", tpf.NAMES)
def test_float64_restatement_and_certification(name):
    fx = tpf.fixture(name)
    s, c, _, tr = tpf.restated(name, torch.float64)
    cert = torch.from_numpy(fx.out["certified"])
    assert cert.float().mean() >= 0.9
    assert torch.equal(tr["gaps"] > fx.m, cert)
    assert np.array_equal(s.numpy()[cert.numpy()], fx.out["sequences64"][cert.numpy()])
    assert np.array_equal(s.numpy()[cert.numpy()], fx.out["sequences"][cert.numpy()])
    assert (c - torch.from_numpy(fx.out["scores64"]))[cert].abs().max() <= 1e-12
    p64 = tr["prefix"]
    err = ((torch.from_numpy(fx.out["prefix"]).double() - p64).abs().max() / p64.abs().max()).item()
    assert err == pytest.approx(fx.meta["prefix_err32"], rel=1e-6)


def test_mean_over_unmasked_rows_is_another_function():
    """User 0 has one item: the reference's mean takes the padding rows too."""
    fx = tpf.fixture("tiger_prefix_main")
    sd = fx.sd_as(torch.float64)
    prof = [p.double() for p in fx.prof]
    full = pref.prefix_tokens(fx.cfg, sd, fx.ids[:1], [p[:1] for p in prof])
    masked = pref.prefix_tokens(fx.cfg, sd, fx.ids[:1], [p[:1] for p in prof], row_mask=fx.mask[:1])
    assert int(fx.mask[0].sum()) == 4
    assert ((masked - full).abs().max() / full.abs().max()) > 100 * fx.meta["prefix_err32"]
