"""The seeded envelope cases of tests/tiger_cases.py, reference against reference on the CPU: what
tests/test_tiger_envelope_gpu.py and tests/test_tiger_prefix_envelope_gpu.py take for granted about them.

Per case the float32 restatement is measured against the float64 one: m = 4 x the score distance over the
users whose sequences agree, a user is certified when every selection gap of its float64 run clears m, and
at least 90 % of the users must be (the cap of the recorded fixtures; a seed that misses it is changed, the
cap is not).  Then the conditions that make each case reach the branch it is there for.
"""
import pytest
import torch

import tiger_cases as tc
import tiger_prefix_ref as pref


def _has_hole(row):
    """A 0 between two 1s."""
    on = row.nonzero()[:, 0]
    return bool((row[int(on[0]):int(on[-1]) + 1] == 0).any())


@pytest.mark.parametrize("name", tc.NAMES)
def test_cases_are_certified(name):
    c = tc.case(name)
    m = tc.measured(name)
    s32, s64 = tc.restated(name, torch.float32)[0], tc.restated(name, torch.float64)[0]
    cert = m["certified"]
    print(f"{name}: enc_err32 {m['enc_err32']:.3e}, logit_err32 {m['logit_err32']:.3e}, score_err32 "
          f"{m['score_err32']:.3e} (m {m['m']:.3e}), certified {int(cert.sum())}/{c.B}")
    assert m["same"].any() and 0 < m["score_err32"] < 1e-5
    assert cert.float().mean() >= 0.9
    assert torch.equal(s32[cert], s64[cert])
    assert s64.shape == (c.B, c.beams, c.T) and 6 <= c.B <= 16


@pytest.mark.parametrize("name", tc.NAMES)
def test_cases_lie_inside_the_envelope(name):
    """The Python-side gate accepts every case (the C gate is the same list, tests/test_tiger_abi.py)."""
    import gr_amd
    c = tc.case(name)
    gr_amd.ops.tiger_check_config(c.cfg, c.beams, c.S, c.T)


def test_env_max_sits_at_every_limit():
    c = tc.case("env_max")
    assert (c.cfg["vocab_size"], c.beams, c.T, c.S) == (128, 32, 8, 128)
    assert (c.cfg["num_layers"], c.cfg["num_decoder_layers"], c.cfg["num_heads"], c.cfg["d_ff"]) == (4, 4, 8, 256)
    tr = tc.restated("env_max", torch.float64)[2]
    assert tr["steps"] == 7 and tr["live"] == [1] + [32] * 6         # 32 * 128 candidates from step 1 on
    n = tc.case("nomask")
    assert n.mask is None and bool(c.mask.all()) and n.ids is c.ids and n.sd is c.sd


@pytest.mark.parametrize("name", ["v65_b32", "env_max"])
def test_the_upper_half_wave_is_selected(name):
    """A token id >= 64 among the certified users' float64 hypotheses: the `lane + 64` half of the search
    kernel's log-softmax decides returned tokens."""
    s64 = tc.restated(name, torch.float64)[0]
    cert = tc.measured(name)["certified"]
    assert int((s64[cert][:, :, 1:] >= 64).sum()) >= 1


def test_stop_T8_stops_at_several_steps():
    c = tc.case("stop_T8")
    s64, _, tr = tc.restated("stop_T8", torch.float64)
    st = tr["stopped_after"]
    assert torch.equal(st, tc.restated("stop_T8", torch.float32)[2]["stopped_after"])
    early = (st > 0) & (st < c.T - 1)
    hist = {int(v): int((st == v).sum()) for v in st.unique()}
    print(f"stop_T8: stopped after {hist} (eos_feature {tc.PULLED['stop_T8']})")
    assert early.sum() * 4 >= c.B
    assert len(st[early].unique()) >= 2
    assert (st == c.T - 1).any()                        # or the library would crop its result
    eos = c.cfg["eos_token_id"]
    assert any(eos in r[1:c.T - 1] for r in s64.view(-1, c.T).tolist())


def test_holes_pad3_masks_and_fill():
    c = tc.case("holes_pad3")
    assert c.cfg["pad_token_id"] == 3
    assert int(c.mask[1].sum()) == 1 and 0 < int(c.mask[1].argmax()) < c.S - 1
    assert bool(c.mask[0].all())
    holes = [_has_hole(row) for row in c.mask]
    assert any(holes)                                   # a 0 between two 1s
    s64 = tc.restated("holes_pad3", torch.float64)[0]
    assert bool((s64[:, :, 0] == 3).all())
    eos = c.cfg["eos_token_id"]
    unfilled = 0
    for r in s64.view(-1, c.T).tolist():
        if eos in r[1:c.T - 1]:
            p = r.index(eos, 1)
            assert all(t == 3 for t in r[p + 1:])
            unfilled += len(r[p + 1:])
    assert unfilled > 0


def test_one_beam_cases_take_single_rows():
    """v2_b1_T2: one step whose continuations all reach max_length; b1_T8: seven steps of one beam, and a
    user whose only beam selects EOS stops with no running beam left."""
    tr = tc.restated("v2_b1_T2", torch.float64)[2]
    assert tr["steps"] == 1 and tr["live"] == [1]
    c = tc.case("v2_b1_T2")
    assert c.cfg["vocab_size"] == 2 * c.beams and c.S == 1
    tr = tc.restated("b1_T8", torch.float64)[2]
    assert tr["steps"] == 7 and tr["live"] == [1] * 7
    c = tc.case("b1_T8")
    assert c.S % 4 and c.cfg["num_decoder_layers"] > c.cfg["num_layers"]


@pytest.mark.parametrize("name", tc.PREFIX_NAMES)
def test_prefix_cases_are_certified(name):
    import gr_amd
    c = tc.prefix_case(name)
    gr_amd.ops.tiger_prefix_check(c.cfg, c.bert_dim, c.n_vec, c.S)
    gr_amd.ops.tiger_check_config(c.cfg, c.beams, c.S + 3, c.T)
    assert set(k.split(".", 1)[1] for k in c.adapters) == set(gr_amd.ops.TIGER_ADAPTER_KEYS)
    m = tc.prefix_measured(name)
    s32, s64 = tc.prefix_restated(name, torch.float32)[0], tc.prefix_restated(name, torch.float64)[0]
    cert = m["certified"]
    print(f"{name}: prefix_err32 {m['prefix_err32']:.3e}, enc_err32 {m['enc_err32']:.3e}, logit_err32 "
          f"{m['logit_err32']:.3e}, score_err32 {m['score_err32']:.3e} (m {m['m']:.3e}), certified "
          f"{int(cert.sum())}/{c.B}")
    assert m["prefix_err32"] > 0 and m["enc_err32"] > 0
    assert cert.float().mean() >= 0.9
    assert torch.equal(s32[cert], s64[cert])


def test_prefix_holes_tell_the_two_means_and_the_two_masks_apart():
    """pfx_holes: the adapters' mean runs over all S rows, masked or not.  The float64 mean over the unmasked
    rows only lies more than 100 tolerances away, and so does the encoder output under an all-ones mask, so
    the GPU test can tell either mistake from rounding."""
    name = "pfx_holes"
    c = tc.prefix_case(name)
    m = tc.prefix_measured(name)
    tr = tc.prefix_restated(name, torch.float64)[2]
    assert int(c.mask[1].sum()) == 1 and c.S == 125
    assert any(_has_hole(row) for row in c.mask)
    prof = [p.double() for p in c.prof]
    sd = c.sd_as(torch.float64)
    with torch.no_grad():
        masked = pref.prefix_tokens(c.cfg, sd, c.ids, prof, row_mask=c.mask)
        other = {}
        pref.beam_search(c.cfg, sd, c.ids, torch.ones_like(c.mask), prof, c.beams, c.T, trace=other)
    p64 = tr["prefix"]
    d = ((masked - p64).abs().max() / p64.abs().max()).item()
    assert d > 100 * 4 * m["prefix_err32"]
    live = c.live
    e64 = tr["enc"]
    d = ((other["enc"] - e64)[live].abs().max() / e64[live].abs().max()).item()
    assert d > 100 * 4 * m["enc_err32"]
