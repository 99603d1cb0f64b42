"""Host-side surface of the TIGER prefix entry points (CPU): the symbols, the workspace query, the
envelope and pointer checks of the C ABI (every check comes before anything reaches a device: the calls
pass a NULL workspace, and the adapter / prof "pointers" are made-up addresses that are never read) and of
the Python layer, and the parameter tree of ``gr_amd.tiger_prefix.TIGER``."""
import ctypes

import numpy as np
import pytest
import torch

import tiger_fixtures as tf
import tiger_prefix_fixtures as tpf

GR_ERR_ARG, GR_ERR_UNSUPPORTED, GR_ERR_WORKSPACE = -1, -2, -4
MAIN = dict(vocab=64, d_model=64, d_kv=16, n_heads=4, d_ff=256, n_enc=2, n_dec=2, n_buckets=32, pad_id=0, eos_id=31,
            fill_id=31)
PMAIN = dict(bert_dim=768, n_vec=5, n_heads=4, eps=1e-5)
FAKE = 0x10000          # a 16-byte aligned address that no check dereferences


def _params(**kw):
    from gr_amd import _lib as L
    p = L.TigerParams()
    for k, v in dict(MAIN, **kw).items():
        setattr(p, k, v)
    return p


def _pparams(adapter=FAKE, **kw):
    from gr_amd import _lib as L
    pp = L.TigerPrefixParams()
    for k, v in dict(PMAIN, **kw).items():
        setattr(pp, k, v)
    for lvl in range(3):
        for i in range(14):
            pp.adapter[lvl][i] = adapter + 16 * (lvl * 14 + i) if adapter else None
    return pp


def _call(lib, p, pp, B=4, S=80, beams=20, T=5, prof=(FAKE, FAKE, FAKE), ws=0):
    return lib.gr_tiger_generate_prefix_f32(ctypes.byref(p), ctypes.byref(pp), None, None, *prof, B, S, beams, T, None,
                                            None, None, None, None, None, ws, None)


def test_symbols_are_exported_and_bound():
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    for name in ("gr_tiger_prefix_workspace_bytes", "gr_tiger_generate_prefix_f32"):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert ctypes.sizeof(L.TigerPrefixParams) == 4 * 4 + 2 * 4 + 3 * 14 * 8 == 360
    assert ctypes.sizeof(L.TigerParams) == 14 * 4 + 8 * 8 + 4 * 8 * 8 + 4 * 13 * 8          # unchanged
    assert gr_amd.tiger_prefix.TIGER is not gr_amd.TIGER and issubclass(gr_amd.tiger_prefix.TIGER, torch.nn.Module)
    assert callable(gr_amd.ops.tiger_generate_prefix) and callable(gr_amd.ops.TigerPrefixBinding)
    assert len(gr_amd.ops.TIGER_ADAPTER_KEYS) == 14


def test_workspace_query():
    import gr_amd
    lib = gr_amd.lib()
    p, pp = _params(), _pparams()
    q = lambda *a: lib.gr_tiger_prefix_workspace_bytes(ctypes.byref(p), ctypes.byref(pp), *a)
    plain = lambda *a: lib.gr_tiger_workspace_bytes(ctypes.byref(p), *a)
    for B, S, beams, T in [(1, 80, 20, 5), (256, 80, 20, 5), (3, 125, 32, 8), (7, 1, 5, 2)]:
        want = plain(B, S + 3, beams, T) + B * (S + 3) * 8 + B * 3 * 64 * 4
        assert want <= q(B, S, beams, T) <= want + 32, (B, S, beams, T)
    assert q(0, 80, 20, 5) > 0
    for bad in [(1, 0, 20, 5), (1, 126, 20, 5), (1, 128, 20, 5), (1, 80, 33, 5), (1, 80, 20, 9), (-1, 80, 20, 5),
                (2 ** 21 + 1, 80, 20, 5)]:
        assert q(*bad) == 0, bad
    assert lib.gr_tiger_prefix_workspace_bytes(None, ctypes.byref(pp), 1, 80, 20, 5) == 0
    assert lib.gr_tiger_prefix_workspace_bytes(ctypes.byref(p), None, 1, 80, 20, 5) == 0
    for kw in (dict(bert_dim=770), dict(bert_dim=1028), dict(n_vec=17), dict(n_vec=0), dict(n_heads=3)):
        bad = _pparams(**kw)
        assert lib.gr_tiger_prefix_workspace_bytes(ctypes.byref(p), ctypes.byref(bad), 1, 80, 20, 5) == 0, kw
    deployed = _params(d_model=128, d_ff=512, n_heads=8)
    assert lib.gr_tiger_prefix_workspace_bytes(ctypes.byref(deployed), ctypes.byref(_pparams(n_heads=8)), 1, 80, 20, 5) == 0


@pytest.mark.parametrize("kw, pkw, call, word", [
    ({}, dict(bert_dim=770), {}, b"bert_dim"), ({}, dict(bert_dim=0), {}, b"bert_dim"),
    ({}, dict(bert_dim=1028), {}, b"bert_dim"),
    ({}, dict(n_vec=0), {}, b"n_vec"), ({}, dict(n_vec=17), {}, b"n_vec"),
    ({}, dict(n_heads=3), {}, b"num_heads"), ({}, dict(n_heads=0), {}, b"num_heads"),
    ({}, {}, dict(S=126), b"125 tokens"), ({}, {}, dict(S=0), b"125 tokens"),
    # everything gr_tiger_generate_f32 checks
    (dict(d_model=128, d_ff=512, n_heads=8), dict(n_heads=8), {}, b"d_model"),       # the deployed prefix config
    (dict(d_model=48), {}, {}, b"d_model"), (dict(d_kv=12), {}, {}, b"d_kv"),
    (dict(n_heads=8), {}, {}, b"num_heads * d_kv"), (dict(d_ff=288), {}, {}, b"d_ff"),
    (dict(n_enc=5), {}, {}, b"num_layers"), (dict(n_dec=0), {}, {}, b"num_decoder_layers"),
    (dict(n_buckets=16), {}, {}, b"num_buckets"), (dict(vocab=129), {}, {}, b"vocab_size"),
    (dict(vocab=39), {}, {}, b"2 * num_beams"), ({}, {}, dict(beams=33), b"num_beams"),
    ({}, {}, dict(T=9), b"max_length"), ({}, {}, dict(B=2 ** 21 + 1), b"2^21"),
])
def test_c_abi_refuses_what_is_outside_the_envelope(kw, pkw, call, word):
    import gr_amd
    lib = gr_amd.lib()
    assert _call(lib, _params(**kw), _pparams(**pkw), **call) == GR_ERR_UNSUPPORTED
    msg = lib.gr_last_error()
    assert msg.startswith(b"gr_tiger_generate_prefix_f32: ") and word in msg, msg


def test_c_abi_argument_and_pointer_checks():
    import gr_amd
    lib = gr_amd.lib()
    p, pp = _params(), _pparams()
    fn = lib.gr_tiger_generate_prefix_f32
    tail = (4, 80, 20, 5, None, None, None, None, None, None, 0, None)
    assert fn(None, ctypes.byref(pp), None, None, FAKE, FAKE, FAKE, *tail) == GR_ERR_ARG
    assert fn(ctypes.byref(p), None, None, None, FAKE, FAKE, FAKE, *tail) == GR_ERR_ARG
    assert b"null prefix params" in lib.gr_last_error()
    assert _call(lib, p, pp, B=-1) == GR_ERR_ARG
    assert _call(lib, _params(eos_id=64), pp) == GR_ERR_ARG and b"[0, vocab)" in lib.gr_last_error()
    # every adapter pointer: null, then misaligned
    for lvl in range(3):
        for i in range(14):
            for value in (None, FAKE + 4):
                bad = _pparams()
                bad.adapter[lvl][i] = value
                assert _call(lib, p, bad) == GR_ERR_ARG, (lvl, i, value)
                assert b"adapter weight pointer" in lib.gr_last_error()
    for i in range(3):
        for value in (None, FAKE + 8):
            prof = [FAKE] * 3
            prof[i] = value
            assert _call(lib, p, pp, prof=prof) == GR_ERR_ARG, (i, value)
            assert b"prof_lvl" in lib.gr_last_error()
    # inside the envelope with every pointer plausible: the workspace is asked for next
    assert _call(lib, p, pp) == GR_ERR_WORKSPACE and b"gr_tiger_prefix_workspace_bytes" in lib.gr_last_error()
    assert _call(lib, p, pp, S=125, ws=1 << 40) == GR_ERR_WORKSPACE
    assert _call(lib, p, _pparams(bert_dim=1024, n_vec=16)) == GR_ERR_WORKSPACE
    assert _call(lib, p, _pparams(bert_dim=4, n_vec=1, n_heads=64)) == GR_ERR_WORKSPACE


@pytest.mark.parametrize("name", tpf.NAMES)
def test_parameter_tree_is_the_references(name):
    import gr_amd
    fx = tpf.fixture(name)
    m = gr_amd.tiger_prefix.TIGER(fx.cfg)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == fx.meta["keys"]
    m.load_state_dict(fx.state_dict())             # strict
    assert m.model.lm_head.weight is m.model.shared.weight
    assert torch.equal(m.adapter_lvl2.cross_attn.in_proj_weight, fx.sd["adapter_lvl2.cross_attn.in_proj_weight"])
    assert torch.equal(m.adapter_lvl3.ffn[2].bias, fx.sd["adapter_lvl3.ffn.2.bias"])
    assert m.adapter_lvl1.bert_proj.weight.shape == (fx.cfg["d_model"], fx.cfg["bert_dim"])
    assert m.adapter_lvl1.norm1.eps == gr_amd.tiger_prefix.ADAPTER_LN_EPS == 1e-5


@pytest.mark.parametrize("name", tf.NAMES)
def test_the_plain_modules_tree_is_unchanged(name):
    import gr_amd
    fx = tf.fixture(name)
    m = gr_amd.TIGER(fx.cfg)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == fx.meta["keys"]
    assert not any(k.startswith("adapter") for k in m.state_dict())


def test_bert_dim_defaults_to_768():
    import gr_amd
    cfg = {k: v for k, v in tpf.fixture("tiger_prefix_bert768").cfg.items() if k != "bert_dim"}
    assert gr_amd.tiger_prefix.TIGER(cfg).adapter_lvl1.bert_proj.in_features == 768


def test_training_and_cpu_are_refused():
    import gr_amd
    fx = tpf.fixture("tiger_prefix_bert768")
    m = gr_amd.tiger_prefix.TIGER(fx.cfg)
    with pytest.raises(NotImplementedError, match="training"):
        m(fx.ids, fx.mask, labels=fx.labels, prof_lvl1=fx.prof[0], prof_lvl2=fx.prof[1], prof_lvl3=fx.prof[2])
    with pytest.raises(NotImplementedError, match="training"):
        m(fx.ids, fx.mask, labels=fx.labels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(fx.ids, fx.mask, num_beams=5, prof_lvl1=fx.prof[0], prof_lvl2=fx.prof[1], prof_lvl3=fx.prof[2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(fx.ids, fx.mask, num_beams=5)


@pytest.mark.parametrize("delta, word", [
    (dict(d_model=128, d_ff=512, num_heads=8, d_kv=16), "d_model"),      # RQVAE-T5-prefix/main.py's deployed width
    (dict(d_ff=512), "d_ff"), (dict(num_heads=8), "num_heads * d_kv"), (dict(num_layers=5), "num_layers"),
    (dict(bert_dim=770), "bert_dim"), (dict(bert_dim=2048), "bert_dim"), (dict(bert_dim=0), "bert_dim"),
    (dict(num_heads=3, d_kv=16), "num_heads"),
])
def test_module_refuses_what_is_outside_the_envelope(delta, word):
    import gr_amd
    cfg = dict(tpf.fixture("tiger_prefix_main").cfg, **delta)
    with pytest.raises(NotImplementedError, match="TIGER: ") as e:
        gr_amd.tiger_prefix.TIGER(cfg)
    assert word in str(e.value) and "no CPU fallback" in str(e.value) and gr_amd.ops.TIGER_ENVELOPE in str(e.value)


def test_call_time_limits_are_named():
    import gr_amd
    cfg = tpf.fixture("tiger_prefix_main").cfg
    for kw, word in [(dict(S=126), "125"), (dict(S=0), "125"), (dict(n_vec=17), "n_vec"), (dict(n_vec=0), "n_vec")]:
        with pytest.raises(NotImplementedError) as e:
            gr_amd.ops.tiger_prefix_check(cfg, 96, **kw)
        assert word in str(e.value) and gr_amd.ops.TIGER_PREFIX_ENVELOPE in str(e.value)
    gr_amd.ops.tiger_prefix_check(cfg, 96, n_vec=16, S=125)


def test_collate_with_prof_arrays():
    from gr_amd import tiger_prefix
    toks = np.array([[1, 16, 20, 26], [6, 9, 17, 27]])
    rng = np.random.default_rng(0)
    prof = [[rng.standard_normal((5, 8)) for _ in range(2)] for _ in range(3)]        # float64 arrays per user
    out = tiger_prefix.collate([toks[:1], toks], [toks[1], toks[0]], 3, prof_lvl1=prof[0], prof_lvl2=prof[1],
                               prof_lvl3=prof[2])
    assert out["history"].tolist() == [[0] * 8 + [1, 16, 20, 26], [0] * 4 + [1, 16, 20, 26, 6, 9, 17, 27]]
    for i in range(3):
        t = out[f"prof_lvl{i + 1}"]
        assert t.dtype == torch.float32 and t.shape == (2, 5, 8)
        assert np.array_equal(t.numpy(), np.stack(prof[i]).astype(np.float32))
    plain = tiger_prefix.collate([toks[:1], toks], [toks[1], toks[0]], 3)
    assert sorted(plain) == ["attention_mask", "history", "target"]
    assert torch.equal(plain["history"], out["history"])
