"""Host-side surface of the TIGER entry points (CPU): the symbols, the workspace query, the envelope
checks of the C ABI (every call passes NULL pointers; the shape checks come first, so nothing reaches
a device) and of the Python layer, and the parameter tree of ``gr_amd.TIGER``."""
import ctypes

import numpy as np
import pytest
import torch

import tiger_fixtures as tf

GR_ERR_ARG, GR_ERR_UNSUPPORTED, GR_ERR_WORKSPACE = -1, -2, -4
MAIN = dict(vocab=64, d_model=64, d_kv=16, n_heads=4, d_ff=256, n_enc=2, n_dec=2, n_buckets=32, pad_id=0, eos_id=31,
            fill_id=31)


def _params(**kw):
    from gr_amd import _lib as L
    p = L.TigerParams()
    for k, v in dict(MAIN, **kw).items():
        setattr(p, k, v)
    return p


def _call(lib, p, B=4, S=80, beams=20, T=5, ws=0):
    return lib.gr_tiger_generate_f32(ctypes.byref(p), None, None, B, S, beams, T, None, None, None, None, None, ws, None)


def test_symbols_are_exported_and_bound():
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    for name in ("gr_tiger_workspace_bytes", "gr_tiger_generate_f32", "gr_beam_hits_i64"):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert ctypes.sizeof(L.TigerParams) == 14 * 4 + 8 * 8 + 4 * 8 * 8 + 4 * 13 * 8
    assert gr_amd.TIGER is gr_amd.tiger.TIGER and callable(gr_amd.ops.tiger_generate) and callable(gr_amd.ops.beam_hits)


def test_workspace_query():
    import gr_amd
    lib = gr_amd.lib()
    p = _params()
    q = lambda *a: lib.gr_tiger_workspace_bytes(ctypes.byref(p), *a)
    one, many = q(1, 80, 20, 5), q(256, 80, 20, 5)
    # cross K/V [n_dec, 2, S, inner] and self K/V [n_dec, 2, T-1, beams, inner] floats per user
    per_user = 4 * (2 * 2 * 80 * 64 + 2 * 2 * 4 * 20 * 64)
    assert per_user <= one <= per_user + 64 and 256 * per_user <= many <= 256 * per_user + 64
    assert q(1, 12, 20, 5) < one and q(1, 80, 5, 5) < one and q(1, 80, 20, 3) < one
    assert q(0, 80, 20, 5) > 0
    for bad in [(1, 0, 20, 5), (1, 129, 20, 5), (1, 80, 33, 5), (1, 80, 0, 5), (1, 80, 20, 9), (1, 80, 20, 1),
                (-1, 80, 20, 5), (2 ** 21 + 1, 80, 20, 5), (2 ** 31, 80, 20, 5)]:
        assert q(*bad) == 0, bad
    assert lib.gr_tiger_workspace_bytes(None, 1, 80, 20, 5) == 0


@pytest.mark.parametrize("kw, call, word", [
    (dict(d_model=48), {}, b"d_model"), (dict(d_model=128), {}, b"d_model"),
    (dict(d_kv=12), {}, b"d_kv"), (dict(d_kv=64, n_heads=1), {}, b"d_kv"),
    (dict(n_heads=8), {}, b"num_heads * d_kv"), (dict(n_heads=1), {}, b"num_heads * d_kv"),
    (dict(d_ff=288), {}, b"d_ff"), (dict(d_ff=100), {}, b"d_ff"), (dict(d_ff=0), {}, b"d_ff"),
    (dict(n_enc=0), {}, b"num_layers"), (dict(n_enc=5), {}, b"num_layers"),
    (dict(n_dec=0), {}, b"num_decoder_layers"), (dict(n_dec=5), {}, b"num_decoder_layers"),
    (dict(n_buckets=16), {}, b"num_buckets"),
    (dict(vocab=129), {}, b"vocab_size"), (dict(vocab=39), {}, b"2 * num_beams"),
    ({}, dict(beams=33), b"num_beams"), ({}, dict(beams=0), b"num_beams"),
    ({}, dict(S=129), b"128 tokens"), ({}, dict(S=0), b"128 tokens"),
    ({}, dict(T=9), b"max_length"), ({}, dict(T=1), b"max_length"),
    ({}, dict(B=2 ** 21 + 1), b"2^21"), ({}, dict(B=2 ** 31), b"2^21"),
])
def test_c_abi_refuses_what_is_outside_the_envelope(kw, call, word):
    import gr_amd
    lib = gr_amd.lib()
    assert _call(lib, _params(**kw), **call) == GR_ERR_UNSUPPORTED
    msg = lib.gr_last_error()
    assert msg.startswith(b"gr_tiger_generate_f32: ") and word in msg, msg


def test_c_abi_argument_order():
    import gr_amd
    lib = gr_amd.lib()
    assert _call(lib, _params(), B=-1) == GR_ERR_ARG
    assert lib.gr_tiger_generate_f32(None, None, None, 1, 80, 20, 5, None, None, None, None, None, 0, None) == GR_ERR_ARG
    assert _call(lib, _params(eos_id=64)) == GR_ERR_ARG and b"[0, vocab)" in lib.gr_last_error()
    assert _call(lib, _params()) == GR_ERR_WORKSPACE
    assert _call(lib, _params(), ws=1 << 40) == GR_ERR_WORKSPACE          # a NULL workspace of any size
    assert _call(lib, _params(vocab=40, eos_id=31)) == GR_ERR_WORKSPACE   # exactly 2 * num_beams is inside
    hits = lib.gr_beam_hits_i64
    assert hits(None, 4, 0, 4, 5, None, 4, None, None) == GR_ERR_ARG
    assert hits(None, 4, 20, 4, 3, None, 4, None, None) == GR_ERR_ARG
    assert hits(None, 4, 20, 4, 5, None, 0, None, None) == GR_ERR_ARG
    assert hits(None, 4, 20, 4, 5, None, 4, None, None) == GR_ERR_ARG and b"null" in lib.gr_last_error()
    assert hits(None, 0, 20, 4, 5, None, 4, None, None) == GR_ERR_ARG


@pytest.mark.parametrize("delta, word", [
    (dict(d_model=128), "d_model"), (dict(d_kv=64, num_heads=1), "d_kv"), (dict(num_heads=8), "num_heads * d_kv"),
    (dict(d_ff=512), "d_ff"), (dict(d_ff=48), "d_ff"), (dict(num_layers=5), "num_layers"),
    (dict(num_decoder_layers=0), "num_decoder_layers"), (dict(vocab_size=200), "vocab_size"),
    (dict(feed_forward_proj="gated-gelu"), "feed_forward_proj"), (dict(eos_token_id=[3, 4]), "one EOS"),
    (dict(relative_attention_num_buckets=16), "relative_attention_num_buckets"),
    (dict(relative_attention_max_distance=64), "relative_attention_max_distance"),
    (dict(tie_word_embeddings=False), "tie_word_embeddings"),
])
def test_module_refuses_what_is_outside_the_envelope(delta, word):
    import gr_amd
    cfg = dict(tf.fixture("tiger_main").cfg, **delta)
    with pytest.raises(NotImplementedError, match="TIGER: ") as e:
        gr_amd.TIGER(cfg)
    assert word in str(e.value) and "no CPU fallback" in str(e.value)


def test_call_time_limits_are_named():
    import gr_amd
    cfg = tf.fixture("tiger_main").cfg
    for kw, word in [(dict(num_beams=33), "num_beams"), (dict(num_beams=40), "num_beams"), (dict(S=129), "128"),
                     (dict(max_length=9), "max_length")]:
        with pytest.raises(NotImplementedError) as e:
            gr_amd.ops.tiger_check_config(cfg, **kw)
        assert word in str(e.value)
    with pytest.raises(NotImplementedError, match="2 \\* num_beams"):
        gr_amd.ops.tiger_check_config(dict(cfg, vocab_size=39), num_beams=20)
    assert gr_amd.ops.tiger_check_config(dict(cfg, vocab_size=40), num_beams=20, S=80, max_length=5) == 31


@pytest.mark.parametrize("name", tf.NAMES)
def test_parameter_tree_is_the_references(name):
    import gr_amd
    fx = tf.fixture(name)
    m = gr_amd.TIGER(fx.cfg)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == fx.meta["keys"]
    m.load_state_dict(fx.state_dict())             # strict
    t5 = m.model
    assert t5.lm_head.weight is t5.shared.weight and t5.encoder.embed_tokens is t5.shared
    assert torch.equal(t5.decoder.block[0].layer[1].EncDecAttention.k.weight,
                       fx.sd["decoder.block.0.layer.1.EncDecAttention.k.weight"])
    assert "transformers" not in type(t5).__module__


def test_training_and_cpu_are_refused():
    import gr_amd
    fx = tf.fixture("tiger_d32_b5")
    m = gr_amd.TIGER(fx.cfg)
    with pytest.raises(NotImplementedError, match="training"):
        m(fx.ids, fx.mask, labels=fx.labels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(fx.ids, fx.mask, num_beams=5)


def test_token_map_and_collate():
    from gr_amd import tiger
    codes = np.array([[0, 7, 3, 1], [5, 0, 0, 2]])
    toks = tiger.codes_to_tokens(codes, 8)
    assert toks.tolist() == [[1, 16, 20, 26], [6, 9, 17, 27]]
    assert tiger.codes_to_tokens(torch.from_numpy(codes), 8).tolist() == toks.tolist()
    hist = [toks[:1], np.concatenate([toks, toks, toks[:1]])]        # 1 item and 5 items, max_len 3
    out = tiger.collate(hist, [toks[1], toks[0][:2]], max_len=3)
    assert out["history"].dtype == out["attention_mask"].dtype == out["target"].dtype == torch.int64
    assert out["history"].tolist() == [[0] * 8 + [1, 16, 20, 26],
                                       [1, 16, 20, 26, 6, 9, 17, 27, 1, 16, 20, 26]]
    assert out["attention_mask"].tolist() == [[0] * 8 + [1] * 4, [1] * 12]
    assert out["target"].tolist() == [[6, 9, 17, 27], [1, 16, -100, -100]]


def test_defaults_named_in_the_config_are_accepted():
    import gr_amd
    cfg = dict(tf.fixture("tiger_d32_b5").cfg, relative_attention_num_buckets=32, relative_attention_max_distance=128,
               tie_word_embeddings=True)
    gr_amd.TIGER(cfg)


def test_library_crop_is_restated_for_the_metric_tail():
    """The library crops its result to the batch's longest hypothesis and evaluate_model zero-pads it
    back: past that width the compared tokens are 0, not the fill.  ``tiger.crop_like_library``
    restates that without a host round trip."""
    from gr_amd import tiger
    eos = 11
    seqs = torch.tensor([[[0, 5, 11, 11, 11], [0, 11, 11, 11, 11]],
                         [[0, 7, 8, 11, 11], [0, 7, 11, 11, 11]]])
    out = tiger.crop_like_library(seqs, eos)           # longest hypothesis: 3 generated tokens
    assert out.tolist() == [[[0, 5, 11, 11, 0], [0, 11, 11, 11, 0]], [[0, 7, 8, 11, 0], [0, 7, 11, 11, 0]]]
    full = seqs.clone()
    full[1, 1] = torch.tensor([0, 7, 9, 3, 11])         # one hypothesis reaches max_length: nothing is cropped
    assert torch.equal(tiger.crop_like_library(full, eos), full)
    noeos = torch.tensor([[[0, 1, 2, 3, 4]]])
    assert torch.equal(tiger.crop_like_library(noeos, eos), noeos)
