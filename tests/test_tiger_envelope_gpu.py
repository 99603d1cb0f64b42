"""TIGER on the GPU (csrc/tiger.hip) at the edges of its envelope, against the float64 restatement
tests/tiger_ref.py on the seeded cases of tests/tiger_cases.py (the rule and the code shape of
test_tiger_gpu.py; what the cases reach is asserted on the CPU by test_tiger_envelope_ref.py).

Tolerances are 4 x the float32 restatement's own worst distance from float64 on the same case, per class,
measured at run time by ``tiger_cases.measured``; a CPU run gave

    case         enc_err32   logit_err32   score_err32 (m = 4 x)   certified   stopped after
    env_max      3.54e-07    5.25e-07      6.16e-07                6/6         7
    v65_b32      2.29e-07    5.56e-07      6.88e-07                6/6         2
    v2_b1_T2     1.53e-07    1.17e-07      4.36e-08                6/6         1
    b1_T8        2.60e-07    4.08e-07      2.66e-07                6/6         7 x5, 1 x1
    holes_pad3   2.23e-07    6.73e-07      1.37e-06                8/8         5
    stop_T8      2.58e-07    6.30e-07      9.97e-07                16/16       2 x6, 3 x5, 5 x2, 7 x3
    nomask       env_max's

(hidden states relative to the tensor's largest magnitude over the live positions, logits relative to the
row scale, scores absolute).  A user is certified when every selection gap of the float64 run clears m;
certified users must match the restatement exactly, in order.  A user whose early-stop heuristic is
satisfied after step s runs no further step in the kernel: its later step logits stay zero.
"""
import pytest
import torch

import tiger_cases as tc
import tiger_ref

pytestmark = pytest.mark.gpu


def _binding(c, dev):
    import gr_amd
    tensors = {k: v.to(dev) for k, v in c.sd.items() if k not in tc.TIED}
    for k in tc.TIED:
        tensors[k] = tensors["shared.weight"]
    return gr_amd.ops.TigerBinding(c.cfg, tensors)


_RUNS = {}


def _run(name, dev):
    """One ops call per case with the encoder output and the step logits, shared by the tests."""
    if name not in _RUNS:
        import gr_amd
        c = tc.case(name)
        mask = None if c.mask is None else c.mask.to(dev)
        out = gr_amd.ops.tiger_generate(_binding(c, dev), c.ids.to(dev), mask, c.beams, c.T, with_encoder=True,
                                        with_logits=True)
        _RUNS[name] = tuple(t.cpu() for t in out)
    return _RUNS[name]


@pytest.mark.parametrize("name", tc.NAMES)
def test_encoder_and_step_logits_against_float64(name, dev):
    c, m = tc.case(name), tc.measured(name)
    seqs, scores, enc, logits = _run(name, dev)
    tr = tc.restated(name, torch.float64)[2]
    live = c.live
    e64 = tr["enc"]
    assert enc.shape == e64.shape
    err = ((enc.double() - e64)[live].abs().max() / e64[live].abs().max()).item()
    tol = 4 * m["enc_err32"]
    print(f"{name}: encoder err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    cert = m["certified"]
    tol = 4 * m["logit_err32"]
    worst = 0.0
    stopped = tr["stopped_after"]
    assert logits.shape == (c.B, c.T - 1, c.beams, c.cfg["vocab_size"])
    for t in range(c.T - 1):
        running = (stopped < 0) | (stopped > t)
        assert not logits[~running, t].any(), "a stopped user ran another step"
        if t >= tr["steps"]:
            assert not running.any()
            continue
        l64, nlive = tr["logits"][t], tr["live"][t]
        on = cert & running                                   # the users whose search runs step t
        got = logits[:, t, :nlive].double()
        e = ((got - l64).abs().amax(-1) / l64.abs().amax(-1))[on]
        worst = max(worst, e.max().item())
        assert logits[running, t, :nlive].abs().amax(-1).gt(0).all()
        assert not logits[:, t, nlive:].any()
    print(f"{name}: step-logit err {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol


@pytest.mark.parametrize("name", tc.NAMES)
def test_beam_results(name, dev):
    c, m = tc.case(name), tc.measured(name)
    seqs, scores, _, _ = _run(name, dev)
    s64, c64, _ = tc.restated(name, torch.float64)
    cert = m["certified"]
    assert cert.float().mean() >= 0.9
    bad = [b for b in range(c.B) if cert[b] and not torch.equal(seqs[b], s64[b])]
    d = (scores.double() - c64)[cert].abs().max().item()
    print(f"{name}: {int(cert.sum())}/{c.B} certified, users differing {bad}, score err {d:.3e} (m {m['m']:.3e})")
    assert not bad
    assert d <= m["m"]
    # every user: descending scores, and each hypothesis re-scored by teacher forcing in float64
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    with torch.no_grad():
        r = tiger_ref.rescore(c.cfg, c.sd_as(torch.float64), c.ids, torch.ones_like(c.ids) if c.mask is None else c.mask,
                              seqs)
    d = (r - scores.double()).abs().max().item()
    print(f"{name}: re-scored hypotheses differ by {d:.3e} (m {m['m']:.3e})")
    assert d <= m["m"]
    assert bool((seqs[:, :, 0] == c.cfg["pad_token_id"]).all())


def test_no_mask_is_the_all_ones_mask(dev):
    """attention_mask=None takes the kernels' null-pointer branches: bit for bit the all-ones run."""
    for a, b in zip(_run("nomask", dev), _run("env_max", dev)):
        assert a.shape == b.shape
        assert torch.equal(a, b) if a.dtype == torch.int64 else torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_non_zero_pad_fills_with_the_pad_id(dev):
    """holes_pad3: `pad_token_id or eos_token_id` is the pad id 3, so a hypothesis that ends early reads
    [3, a, EOS, 3, 3, 3] (with pad id 0 the fill is the EOS id)."""
    c = tc.case("holes_pad3")
    seqs = _run("holes_pad3", dev)[0]
    s64 = tc.restated("holes_pad3", torch.float64)[0]
    eos, pad = c.cfg["eos_token_id"], c.cfg["pad_token_id"]
    early = [r for r in seqs.view(-1, c.T).tolist() if eos in r[1:c.T - 1]]
    assert early and early == [r for r in s64.view(-1, c.T).tolist() if eos in r[1:c.T - 1]]
    for r in early:
        assert all(t == pad for t in r[r.index(eos, 1) + 1:])


def test_stops_at_several_steps(dev):
    """stop_T8: the step loop leaves after steps 2, 3, 5 and 7, user by user; every hypothesis is the
    float64 restatement's (all 16 users are certified)."""
    c, m = tc.case("stop_T8"), tc.measured("stop_T8")
    seqs, _, _, logits = _run("stop_T8", dev)
    s64, _, tr = tc.restated("stop_T8", torch.float64)
    ran = logits.abs().amax((-1, -2)).gt(0).sum(1)              # steps with any non-zero logit
    assert torch.equal(ran, tr["stopped_after"])
    assert len(ran.unique()) >= 3
    assert torch.equal(seqs[m["certified"]], s64[m["certified"]])


def test_batch_independence_at_the_edge(dev):
    """User 2 of env_max alone, and at position 3 of a batch of 5: bit-identical to its row of the full run."""
    import gr_amd
    c = tc.case("env_max")
    bind = _binding(c, dev)
    full_s, full_c = _run("env_max", dev)[:2]
    ids, mask = c.ids.to(dev), c.mask.to(dev)
    for B, at in [(1, 0), (5, 3)]:
        order = torch.arange(B) % c.B
        order[at] = 2
        o = order.to(dev)
        s, sc = gr_amd.ops.tiger_generate(bind, ids[o], mask[o], c.beams, c.T)
        s, sc = s.cpu(), sc.cpu()
        assert torch.equal(s[at], full_s[2]) and torch.equal(sc[at].view(torch.int32), full_c[2].view(torch.int32))
        assert torch.equal(s, full_s[order]) and torch.equal(sc.view(torch.int32), full_c[order].view(torch.int32))


@pytest.mark.parametrize("k", [1, 32])
def test_beam_hits_over_several_blocks(k, dev):
    """300 users are three blocks of 128, the last one partial; hits planted in rows 0, 127, 128 and 299."""
    import gr_amd
    B, T = 300, 5
    g = torch.Generator().manual_seed(7 + k)
    preds = torch.randint(1, 60, (B, k, T), generator=g)
    preds[:, :, 0] = 0
    labels = torch.randint(60, 64, (B, T - 1), generator=g)        # no hit unless planted
    planted = {0: 0, 127: k - 1, 128: k // 2, 299: k - 1}
    for b, j in planted.items():
        labels[b] = preds[b, j, 1:]
    labels[5] = preds[5, 0, 1:]
    labels[5, 2] = -100                                             # a padded label never matches
    if k > 1:
        preds[128, k - 1] = preds[128, k // 2]                      # duplicate beams: the first one counts
    want = tiger_ref.pos_index(preds[:, :, 1:], labels)
    got = gr_amd.ops.beam_hits(preds.to(dev), labels.to(dev), skip=1).cpu()
    assert got.dtype == torch.bool and torch.equal(got, want)
    assert all(want[b, j] for b, j in planted.items()) and int(want.sum()) == len(planted) and not want[5].any()
