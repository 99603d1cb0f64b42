"""tests/tiger_ref.py, the plain-torch restatement of TIGER inference, against the fixtures the
reference itself produced (tests/golden/make_golden_tiger.py) and, where ``transformers`` is
importable, against the live library on a freshly seeded model."""
import numpy as np
import pytest
import torch

import tiger_fixtures as tf
import tiger_ref


@pytest.mark.parametrize("name", tf.NAMES)
def test_float32_restatement_reproduces_the_reference(name):
    fx = tf.fixture(name)
    s, c, width, tr = tf.restated(name, torch.float32)
    assert width == fx.T
    assert np.array_equal(s.numpy(), fx.out["sequences"])
    assert np.abs(c.numpy() - fx.out["sequences_scores"]).max() <= 1e-6
    n = fx.meta["enc_users"]
    live = fx.mask[:n].bool()
    assert (tr["enc"][:n][live] - torch.from_numpy(fx.out["encoder_output"])[live]).abs().max() <= 1e-5


@pytest.mark.parametrize("name", tf.NAMES)
def test_float64_restatement_reproduces_its_stored_run(name):
    fx = tf.fixture(name)
    s, c, _, tr = tf.restated(name, torch.float64)
    assert np.array_equal(s.numpy(), fx.out["sequences64"])
    assert np.abs(c.numpy() - fx.out["scores64"]).max() <= 1e-12
    cert = tr["gaps"].numpy() > fx.m
    assert np.array_equal(cert, fx.out["certified"]) and cert.mean() >= 0.9
    # certified users: the float32 reference and the float64 restatement return the same hypotheses
    assert np.array_equal(fx.out["sequences"][cert], fx.out["sequences64"][cert])
    assert np.abs(fx.out["sequences_scores"][cert] - fx.out["scores64"][cert]).max() <= fx.m


def test_unfilled_positions_hold_the_eos_id():
    """The library fills its hypothesis buffers with `pad_token_id or eos_token_id`: with pad id 0 a
    hypothesis that ends early is followed by EOS ids, not by padding."""
    fx = tf.fixture("tiger_eos")
    eos, pad = fx.cfg["eos_token_id"], fx.cfg["pad_token_id"]
    s = tf.restated("tiger_eos", torch.float32)[0].view(-1, fx.T).tolist()
    early = [r for r in s if eos in r[1:fx.T - 1]]
    assert early
    for r in early:
        p = r.index(eos, 1)
        assert all(t == eos for t in r[p:]) and eos != pad
    ref_early = [r for r in fx.out["sequences"].reshape(-1, fx.T).tolist() if eos in r[1:fx.T - 1]]
    assert early == ref_early


def test_early_stop_fixture_stops_early():
    """tiger_stop: most users fill their finished slots and satisfy the stop heuristic at step 2 or 3; the
    finished list then merges old and new hypotheses at every step."""
    fx = tf.fixture("tiger_stop")
    for dtype in (torch.float32, torch.float64):
        st = tf.restated("tiger_stop", dtype)[3]["stopped_after"]
        assert np.array_equal(st.numpy(), fx.out["stopped_after"])
    early = (st > 0) & (st < fx.T - 1)
    assert early.sum() * 4 >= len(st) and (st == 2).any() and (st == 3).any() and (st == fx.T - 1).any()
    eos = fx.cfg["eos_token_id"]
    ends = [r.index(eos, 1) if eos in r[1:] else fx.T for r in fx.out["sequences"].reshape(-1, fx.T).tolist()]
    assert {1, 2, 3} <= set(ends)
    # a batch of users who all stop early comes back cropped from the library
    sub = torch.nonzero(st == 2)[:4, 0]
    with torch.no_grad():
        out = tiger_ref.generate(fx.cfg, fx.sd, fx.ids[sub], fx.mask[sub], fx.beams, fx.T)
    assert out.shape == (4 * fx.beams, 3)


@pytest.mark.parametrize("name", ["tiger_eos", "tiger_stop"])
def test_rescore_matches_the_search_scores(name):
    fx = tf.fixture(name)
    s, c, _, _ = tf.restated(name, torch.float64)
    with torch.no_grad():
        r = tiger_ref.rescore(fx.cfg, fx.sd_as(torch.float64), fx.ids, fx.mask, s)
    assert (r - c).abs().max() <= 1e-10


def test_pos_index_and_metrics_reproduce_the_reference():
    fx = tf.fixture("tiger_main")
    seqs = torch.from_numpy(fx.out["sequences"])
    half = seqs.shape[0] // 2
    rec, nd = {}, {}
    for sl in (slice(0, half), slice(half, None)):
        r, n = tiger_ref.metrics(tiger_ref.pos_index(seqs[sl][:, :, 1:5], fx.labels[sl]), fx.meta["topk_list"])
        for k, v in {**r, **n}.items():
            (rec if k.startswith("Recall") else nd).setdefault(k, []).append(v)
    assert {k: sum(v) / len(v) for k, v in rec.items()} == fx.meta["recall"]
    assert {k: sum(v) / len(v) for k, v in nd.items()} == fx.meta["ndcg"]
    assert fx.meta["recall"]["Recall@20"] > fx.meta["recall"]["Recall@2"] > 0


def test_against_the_live_library():
    transformers = pytest.importorskip("transformers", reason="transformers is not installed")
    cfg = dict(vocab_size=48, num_layers=2, num_decoder_layers=2, d_model=32, d_ff=64, num_heads=2, d_kv=16,
               dropout_rate=0.1, feed_forward_proj="relu", pad_token_id=0, eos_token_id=7)
    torch.manual_seed(5)
    model = transformers.T5ForConditionalGeneration(transformers.T5Config(
        decoder_start_token_id=cfg["pad_token_id"], **cfg)).eval()
    with torch.no_grad():
        model.shared.weight[cfg["eos_token_id"]] *= 3.0
    g = torch.Generator().manual_seed(6)
    B, S, k = 6, 12, 8
    ids = torch.randint(1, cfg["vocab_size"], (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.int64)
    for b in range(B):
        ids[b, :b] = 0
        mask[b, :b] = 0
    with torch.no_grad():
        out = model.generate(input_ids=ids, attention_mask=mask, max_length=5, num_beams=k, num_return_sequences=k,
                             return_dict_in_generate=True, output_scores=True)
        sd = {n: v for n, v in model.state_dict().items()}
        full = dict(cfg, layer_norm_epsilon=model.config.layer_norm_epsilon,
                    scale_decoder_outputs=getattr(model.config, "scale_decoder_outputs", True))
        s, c, width = tiger_ref.beam_search(full, sd, ids, mask, k, 5)
    assert out.sequences.shape[1] == width
    assert torch.equal(s.view(-1, 5)[:, :width], out.sequences)
    assert (c.view(-1) - out.sequences_scores).abs().max() <= 1e-6


# The seeded envelope cases (tests/tiger_cases.py) with more than one beam.  Left out: the one-beam cases
# v2_b1_T2 and b1_T8, because the library switches to greedy decoding at one beam and returns no
# sequences_scores (the kernel's contract there is the restatement's beam search with k = 1); and nomask,
# because without a mask the library infers one from the pad ids among the inputs, while the kernels take
# None as all ones, which is env_max itself.
@pytest.mark.parametrize("name", ["env_max", "v65_b32", "holes_pad3", "stop_T8"])
def test_envelope_cases_against_the_live_library(name):
    transformers = pytest.importorskip("transformers", reason="transformers is not installed")
    import tiger_cases as tc
    c = tc.case(name)
    model = transformers.T5ForConditionalGeneration(transformers.T5Config(
        decoder_start_token_id=c.cfg["pad_token_id"], **c.cfg)).eval()
    model.load_state_dict(c.sd)
    with torch.no_grad():
        out = model.generate(input_ids=c.ids, attention_mask=c.mask, max_length=c.T, num_beams=c.beams,
                             num_return_sequences=c.beams, return_dict_in_generate=True, output_scores=True)
    assert model.config.layer_norm_epsilon == c.cfg["layer_norm_epsilon"]
    assert getattr(model.config, "scale_decoder_outputs", True) is True
    s, sc, tr = tc.restated(name, torch.float32)
    width = out.sequences.shape[1]
    assert width == c.T                                  # a user that never stops early keeps the library from cropping
    assert torch.equal(s.view(-1, c.T), out.sequences)
    assert (sc.view(-1) - out.sequences_scores).abs().max() <= 1e-6
