"""Host-side surface of the TIGER teacher-forced forward (CPU): the four symbols, the workspace queries, the
envelope, pointer and alignment checks of the C ABI (every check comes before anything reaches a device: the
pointers are NULL or made-up addresses that are never read) and the mode rules of the two modules' ``forward``."""
import ctypes

import pytest
import torch

import tiger_fixtures as tf
import tiger_prefix_fixtures as tpf

GR_OK, GR_ERR_ARG, GR_ERR_UNSUPPORTED, GR_ERR_WORKSPACE = 0, -1, -2, -4
MAIN = dict(vocab=64, d_model=64, d_kv=16, n_heads=4, d_ff=256, n_enc=2, n_dec=2, n_buckets=32, pad_id=0, eos_id=31,
            fill_id=31)
PMAIN = dict(bert_dim=768, n_vec=5, n_heads=4, eps=1e-5)
FAKE = 0x10000          # a 16-byte aligned address that no check dereferences
PLAIN, PREFIX = "gr_tiger_forward_f32", "gr_tiger_forward_prefix_f32"


def _params(weights=None, **kw):
    from gr_amd import _lib as L
    p = L.TigerParams()
    for k, v in dict(MAIN, **kw).items():
        setattr(p, k, v)
    if weights:
        for k in ("shared", "lm_head", "enc_rel", "dec_rel", "enc_final_ln", "dec_final_ln", "enc_bucket", "dec_bucket"):
            setattr(p, k, weights)
        for l in range(4):
            for i in range(8):
                p.enc[l][i] = weights
            for i in range(13):
                p.dec[l][i] = weights
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


def _call(lib, which, p, pp=None, B=4, S=80, Ld=4, ids=None, labels=None, loss=None, prof=(FAKE, FAKE, FAKE), wsp=None,
          ws=0):
    if which == PLAIN:
        return lib.gr_tiger_forward_f32(ctypes.byref(p), ids, None, labels, B, S, Ld, loss, None, None, None, wsp, ws,
                                        None)
    return lib.gr_tiger_forward_prefix_f32(ctypes.byref(p), ctypes.byref(pp or _pparams()), ids, None, *prof, labels, B, S,
                                           Ld, loss, None, None, None, wsp, ws, None)


def test_symbols_are_exported_and_bound():
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    for name in ("gr_tiger_forward_workspace_bytes", "gr_tiger_forward_f32", "gr_tiger_forward_prefix_workspace_bytes",
                 "gr_tiger_forward_prefix_f32"):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert len(L.SIGNATURES[PLAIN][1]) == 14 and len(L.SIGNATURES[PREFIX][1]) == 18
    assert ctypes.sizeof(L.TigerParams) == 14 * 4 + 8 * 8 + 4 * 8 * 8 + 4 * 13 * 8          # unchanged
    assert callable(gr_amd.ops.tiger_forward) and callable(gr_amd.ops.tiger_forward_prefix)
    assert callable(gr_amd.tiger.eval_loss) and gr_amd.tiger_prefix.eval_loss is gr_amd.tiger.eval_loss


def test_workspace_query():
    import gr_amd
    lib = gr_amd.lib()
    p, pp = _params(), _pparams()
    q = lambda *a: lib.gr_tiger_forward_workspace_bytes(ctypes.byref(p), *a)
    # cross K/V [n_dec, 2, S, inner] floats and one (sum, count) pair of doubles per user
    per_user = 4 * (2 * 2 * 80 * 64) + 16
    one, many = q(1, 80, 4), q(256, 80, 4)
    assert per_user <= one <= per_user + 64 and 256 * per_user <= many <= 256 * per_user + 64
    assert q(1, 12, 4) < one < q(1, 128, 4) and one < q(2, 80, 4)
    deep = _params(n_dec=4)
    assert lib.gr_tiger_forward_workspace_bytes(ctypes.byref(deep), 1, 80, 4) > one
    assert q(1, 80, 1) == q(1, 80, 8) == one              # no self K/V workspace: it stays in LDS
    assert q(0, 80, 4) > 0
    for bad in [(1, 0, 4), (1, 129, 4), (1, 80, 0), (1, 80, 9), (-1, 80, 4), (2 ** 21 + 1, 80, 4), (2 ** 31, 80, 4)]:
        assert q(*bad) == 0, bad
    assert lib.gr_tiger_forward_workspace_bytes(None, 1, 80, 4) == 0
    assert lib.gr_tiger_forward_workspace_bytes(ctypes.byref(_params(d_model=128)), 1, 80, 4) == 0
    assert lib.gr_tiger_forward_workspace_bytes(ctypes.byref(_params(vocab=2, eos_id=1, fill_id=1)), 1, 80, 4) > 0
    qp = lambda *a: lib.gr_tiger_forward_prefix_workspace_bytes(ctypes.byref(p), ctypes.byref(pp), *a)
    for B, S, Ld in [(1, 80, 4), (256, 80, 4), (3, 125, 8), (7, 1, 1)]:
        want = q(B, S + 3, Ld) + B * (S + 3) * 8 + B * 3 * 64 * 4
        assert want <= qp(B, S, Ld) <= want + 32, (B, S, Ld)
    for bad in [(1, 0, 4), (1, 126, 4), (1, 128, 4), (1, 80, 0), (1, 80, 9), (-1, 80, 4), (2 ** 21 + 1, 80, 4)]:
        assert qp(*bad) == 0, bad
    assert lib.gr_tiger_forward_prefix_workspace_bytes(None, ctypes.byref(pp), 1, 80, 4) == 0
    assert lib.gr_tiger_forward_prefix_workspace_bytes(ctypes.byref(p), None, 1, 80, 4) == 0
    for kw in (dict(bert_dim=770), dict(n_vec=17), dict(n_vec=0), dict(n_heads=3)):
        assert lib.gr_tiger_forward_prefix_workspace_bytes(ctypes.byref(p), ctypes.byref(_pparams(**kw)), 1, 80, 4) == 0, kw
    deployed = _params(d_model=128, d_ff=512, n_heads=8)
    assert lib.gr_tiger_forward_prefix_workspace_bytes(ctypes.byref(deployed), ctypes.byref(_pparams(n_heads=8)), 1, 80,
                                                       4) == 0


@pytest.mark.parametrize("which", [PLAIN, PREFIX])
@pytest.mark.parametrize("kw, call, word", [
    ({}, dict(Ld=0), b"Ld"), ({}, dict(Ld=9), b"Ld"), ({}, dict(Ld=-1), b"Ld"),
    (dict(d_model=128), {}, b"d_model"), (dict(d_model=128, d_ff=512, n_heads=8), {}, b"d_model"),
    (dict(d_model=48), {}, b"d_model"), (dict(d_kv=12), {}, b"d_kv"), (dict(n_heads=8), {}, b"num_heads * d_kv"),
    (dict(d_ff=288), {}, b"d_ff"), (dict(n_enc=5), {}, b"num_layers"), (dict(n_dec=0), {}, b"num_decoder_layers"),
    (dict(n_buckets=16), {}, b"num_buckets"), (dict(vocab=129), {}, b"vocab_size"), (dict(vocab=1), {}, b"vocab_size"),
    ({}, dict(S=129), b"tokens"), ({}, dict(S=0), b"tokens"),
    ({}, dict(B=2 ** 21 + 1), b"2^21"), ({}, dict(B=2 ** 31), b"2^21"),
])
def test_c_abi_refuses_what_is_outside_the_envelope(which, kw, call, word):
    import gr_amd
    lib = gr_amd.lib()
    assert _call(lib, which, _params(**kw), **call) == GR_ERR_UNSUPPORTED
    msg = lib.gr_last_error()
    assert msg.startswith(which.encode() + b": ") and word in msg, msg


def test_history_limits_carry_each_entry_s_prefix():
    import gr_amd
    lib = gr_amd.lib()
    assert _call(lib, PLAIN, _params(), S=129) == GR_ERR_UNSUPPORTED
    assert lib.gr_last_error().startswith(b"gr_tiger_forward_f32: ") and b"128 tokens" in lib.gr_last_error()
    assert _call(lib, PLAIN, _params(), S=128) == GR_ERR_WORKSPACE
    assert _call(lib, PREFIX, _params(), S=126) == GR_ERR_UNSUPPORTED
    assert lib.gr_last_error().startswith(b"gr_tiger_forward_prefix_f32: ") and b"125 tokens" in lib.gr_last_error()
    assert _call(lib, PREFIX, _params(), S=125) == GR_ERR_WORKSPACE
    for pkw, word in [(dict(bert_dim=770), b"bert_dim"), (dict(n_vec=17), b"n_vec"), (dict(n_heads=3), b"num_heads")]:
        assert _call(lib, PREFIX, _params(), _pparams(**pkw)) == GR_ERR_UNSUPPORTED
        assert lib.gr_last_error().startswith(b"gr_tiger_forward_prefix_f32: ") and word in lib.gr_last_error()


@pytest.mark.parametrize("which", [PLAIN, PREFIX])
def test_c_abi_argument_pointer_and_alignment_checks(which):
    import gr_amd
    lib = gr_amd.lib()
    who = which.encode() + b": "
    err = lambda: lib.gr_last_error()
    assert _call(lib, which, _params(), B=-1) == GR_ERR_ARG and err().startswith(who)
    if which == PLAIN:
        assert lib.gr_tiger_forward_f32(None, None, None, None, 4, 80, 4, None, None, None, None, None, 0, None) == GR_ERR_ARG
    else:
        tail = (None, 4, 80, 4, None, None, None, None, None, 0, None)
        fn = lib.gr_tiger_forward_prefix_f32
        assert fn(None, ctypes.byref(_pparams()), None, None, FAKE, FAKE, FAKE, *tail) == GR_ERR_ARG
        assert fn(ctypes.byref(_params()), None, None, None, FAKE, FAKE, FAKE, *tail) == GR_ERR_ARG
        assert b"null prefix params" in err()
        bad = _pparams()
        bad.adapter[1][3] = FAKE + 4
        assert _call(lib, which, _params(), bad) == GR_ERR_ARG and b"adapter weight pointer" in err()
        bad.adapter[1][3] = None
        assert _call(lib, which, _params(), bad) == GR_ERR_ARG and b"adapter weight pointer" in err()
        for i in range(3):
            for value in (None, FAKE + 8):
                prof = [FAKE] * 3
                prof[i] = value
                assert _call(lib, which, _params(), prof=tuple(prof)) == GR_ERR_ARG and b"prof_lvl" in err()
    for kw in (dict(eos_id=64), dict(pad_id=-1), dict(fill_id=64)):
        assert _call(lib, which, _params(**kw)) == GR_ERR_ARG and b"[0, vocab)" in err() and err().startswith(who)
    # the workspace: missing, too small, misaligned
    p = _params()
    if which == PLAIN:
        need = lib.gr_tiger_forward_workspace_bytes(ctypes.byref(p), 4, 80, 4)
    else:
        need = lib.gr_tiger_forward_prefix_workspace_bytes(ctypes.byref(p), ctypes.byref(_pparams()), 4, 80, 4)
    query = which.replace("_f32", "_workspace_bytes").encode()
    assert need > 0
    for wsp, ws in [(None, 0), (None, 1 << 40), (FAKE, need - 1), (FAKE + 8, need)]:
        assert _call(lib, which, p, wsp=wsp, ws=ws) == GR_ERR_WORKSPACE, (wsp, ws)
        assert err().startswith(who) and query in err()
    # the required pointers, then the weights; an empty batch is done once every check has passed
    full = dict(ids=FAKE, labels=FAKE, loss=FAKE)
    for k in full:
        assert _call(lib, which, p, wsp=FAKE, ws=need, **dict(full, **{k: None})) == GR_ERR_ARG, k
        assert err() == who + b"null pointer"
    assert _call(lib, which, p, wsp=FAKE, ws=need, **full) == GR_ERR_ARG and b"a weight pointer" in err()
    ok = _params(weights=FAKE)
    ok.lm_head = FAKE + 4
    assert _call(lib, which, ok, wsp=FAKE, ws=need, **full) == GR_ERR_ARG and b"a weight pointer" in err()
    ok.lm_head = FAKE
    ok.dec[1][12] = None
    assert _call(lib, which, ok, wsp=FAKE, ws=need, **full) == GR_ERR_ARG and b"a weight pointer" in err()
    ok.dec[1][12] = FAKE
    assert _call(lib, which, ok, B=0, wsp=FAKE, ws=need, **full) == GR_OK


def _modules():
    import gr_amd
    fx, pfx = tf.fixture("tiger_d32_b5"), tpf.fixture("tiger_prefix_bert768")
    prof = dict(prof_lvl1=pfx.prof[0], prof_lvl2=pfx.prof[1], prof_lvl3=pfx.prof[2])
    return [(gr_amd.TIGER(fx.cfg), fx, {}), (gr_amd.tiger_prefix.TIGER(pfx.cfg), pfx, {}),
            (gr_amd.tiger_prefix.TIGER(pfx.cfg), pfx, prof)]


def test_module_mode_rules():
    for m, fx, prof in _modules():
        assert m.training
        with pytest.raises(NotImplementedError, match="training"):
            m(fx.ids, fx.mask, labels=fx.labels, **prof)
        with torch.no_grad():                          # still in training mode
            with pytest.raises(NotImplementedError, match="training"):
                m(fx.ids, fx.mask, labels=fx.labels, **prof)
        m.eval()
        with pytest.raises(NotImplementedError, match="training"):      # eval mode, gradients enabled
            m(fx.ids, fx.mask, labels=fx.labels, **prof)
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                m(fx.ids, fx.mask, labels=fx.labels, **prof)
            with pytest.raises(ValueError, match="labels"):
                m(fx.ids, fx.mask, **prof)
            with pytest.raises(ValueError, match="labels"):
                m(fx.ids, fx.mask, labels=None, **prof)


def test_label_width_is_checked_before_the_device():
    """ops.tiger_forward refuses CPU tensors first; the Ld limits of the Python layer are in its argument check."""
    import gr_amd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gr_amd.ops.tiger_forward(None, torch.zeros(2, 5, dtype=torch.int64), None, torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gr_amd.ops.tiger_forward_prefix(None, torch.zeros(2, 5, dtype=torch.int64), None, *[torch.zeros(2, 5, 8)] * 3,
                                        torch.zeros(2, 4, dtype=torch.int64))
