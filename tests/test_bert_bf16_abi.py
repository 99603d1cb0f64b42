"""Host-side surface of the BERT encoder's bf16 precision (CPU): the four symbols, the struct, the envelope and argument
checks of gr_bert_embed_bf16 / gr_bert_embed_ragged_bf16 (gr_bert_embed_f32's, in its order: every call passes NULL
pointers, the shape checks come first, nothing reaches a device), the workspace queries, and the module's refusals."""
import ctypes

import pytest
import torch

import bert_embed_fixtures as bf

GR_OK, GR_ERR_ARG, GR_ERR_UNSUPPORTED, GR_ERR_WORKSPACE = 0, -1, -2, -4
BASE = dict(vocab_size=30522, hidden_size=768, num_heads=12, head_dim=64, intermediate_size=3072, num_layers=12,
            max_position=512, type_vocab_size=2, hidden_act=0, position_type=0, eps=1e-12)
NAMES = ("gr_bert_embed_bf16_workspace_bytes", "gr_bert_embed_bf16", "gr_bert_embed_ragged_bf16_workspace_bytes",
         "gr_bert_embed_ragged_bf16")


def _params(cls="BertBf16Params", **kw):
    from gr_amd import _lib as L
    p = getattr(L, cls)()
    for k, v in dict(BASE, **kw).items():
        setattr(p, k, v)
    return p


def _call(lib, p, B=4, S=128, pooling=1, ws=0):
    return lib.gr_bert_embed_bf16(ctypes.byref(p), None, None, None, B, S, pooling, None, None, None, ws, None)


def _call_ragged(lib, p, B=4, S=128, rows=None, pooling=1, ws=0):
    rows = B * S if rows is None else rows
    return lib.gr_bert_embed_ragged_bf16(ctypes.byref(p), None, None, None, B, S, rows, pooling, None, None, None, None,
                                         ws, None)


def test_symbols_and_struct():
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    for name in NAMES:
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    # gr_bert_bf16_params: 10 int32, 2 float, 5 table pointers, 24 x 6 bf16 matrices, 24 x 10 fp32 vectors
    assert ctypes.sizeof(L.BertBf16Params) == 10 * 4 + 2 * 4 + 5 * 8 + 24 * 6 * 8 + 24 * 10 * 8
    assert ctypes.sizeof(L.BertBf16Params) == ctypes.sizeof(L.BertParams)          # 16 pointers per layer both ways
    assert L.BertBf16Params.matrix.offset == L.BertParams.layer.offset
    assert [f for f, _ in L.BertBf16Params._fields_[:-2]] == [f for f, _ in L.BertParams._fields_[:-1]]
    assert len(gr_amd.ops.BertBf16Binding.MATRICES) == 6
    assert [gr_amd.ops.BERT_LAYER_KEYS[i].split(".")[-2] for i in gr_amd.ops.BertBf16Binding.MATRICES] == \
        ["query", "key", "value", "dense", "dense", "dense"]
    assert issubclass(gr_amd.ops.BertBf16Binding, gr_amd.ops.BertBinding)


@pytest.mark.parametrize("kw, call, word", [
    (dict(hidden_size=776), {}, b"hidden_size"), (dict(hidden_size=1088, num_heads=17), {}, b"hidden_size"),
    (dict(hidden_size=0), {}, b"hidden_size"),
    (dict(head_dim=48, num_heads=16), {}, b"head_dim"), (dict(head_dim=128, num_heads=6), {}, b"head_dim"),
    (dict(num_heads=8), {}, b"num_heads * head_dim"), (dict(num_heads=0), {}, b"num_heads * head_dim"),
    (dict(intermediate_size=3080), {}, b"intermediate_size"), (dict(intermediate_size=4128), {}, b"intermediate_size"),
    (dict(intermediate_size=0), {}, b"intermediate_size"),
    (dict(num_layers=0), {}, b"num_layers"), (dict(num_layers=25), {}, b"num_layers"),
    (dict(hidden_act=1), {}, b"hidden_act"), (dict(position_type=1), {}, b"position_embedding_type"),
    (dict(vocab_size=0), {}, b"vocab_size"), (dict(type_vocab_size=0), {}, b"type_vocab_size"),
    (dict(max_position=0), {}, b"max_position_embeddings"),
    ({}, dict(S=0), b"S must be"), ({}, dict(S=513), b"S must be"),
    (dict(max_position=64), dict(S=65), b"max_position_embeddings"),
    ({}, dict(B=2 ** 16 + 1), b"B must be"), ({}, dict(B=2 ** 31), b"B must be"),
])
def test_outside_the_envelope(kw, call, word):
    """The fp32 entry's cases (test_bert_embed_abi.py), its error code and its word, under the new entries' names; the
    workspace queries answer 0."""
    import gr_amd
    lib = gr_amd.lib()
    p = _params(**kw)
    B, S = call.get("B", 4), call.get("S", 128)
    p32 = _params("BertParams", **kw)                                                      # the fp32 entry, for its word
    assert lib.gr_bert_embed_f32(ctypes.byref(p32), None, None, None, B, S, 1, None, None, None, 0, None) == GR_ERR_UNSUPPORTED
    assert word in lib.gr_last_error()
    assert _call(lib, p, **call) == GR_ERR_UNSUPPORTED
    msg = lib.gr_last_error()
    assert msg.startswith(b"gr_bert_embed_bf16: ") and word in msg, msg
    assert _call_ragged(lib, p, **call) == GR_ERR_UNSUPPORTED
    msg = lib.gr_last_error()
    assert msg.startswith(b"gr_bert_embed_ragged_bf16: ") and word in msg, msg
    assert lib.gr_bert_embed_bf16_workspace_bytes(ctypes.byref(p), B, S) == 0
    assert lib.gr_bert_embed_ragged_bf16_workspace_bytes(ctypes.byref(p), B, S, 8) == 0


def test_argument_order():
    import gr_amd
    lib = gr_amd.lib()
    assert lib.gr_bert_embed_bf16(None, None, None, None, 1, 128, 1, None, None, None, 0, None) == GR_ERR_ARG
    assert lib.gr_bert_embed_ragged_bf16(None, None, None, None, 1, 128, 128, 1, None, None, None, None, 0, None) == GR_ERR_ARG
    assert lib.gr_bert_embed_bf16_workspace_bytes(None, 1, 128) == 0
    assert lib.gr_bert_embed_ragged_bf16_workspace_bytes(None, 1, 128, 128) == 0
    for call in (_call, _call_ragged):
        assert call(lib, _params(), B=-1) == GR_ERR_ARG
        assert call(lib, _params(hidden_size=776), B=-1) == GR_ERR_ARG          # ARG before UNSUPPORTED
        assert call(lib, _params(hidden_size=776)) == GR_ERR_UNSUPPORTED        # UNSUPPORTED before WORKSPACE
        for pooling in (-1, 3):
            assert call(lib, _params(), pooling=pooling) == GR_ERR_ARG and b"pooling" in lib.gr_last_error()
        assert call(lib, _params()) == GR_ERR_WORKSPACE                         # a short (here: missing) workspace
        assert call(lib, _params(), ws=1 << 40) == GR_ERR_WORKSPACE
        assert b"_bf16_workspace_bytes" in lib.gr_last_error()
        assert call(lib, _params(), B=0) == GR_OK                               # nothing to do, nothing launched
        assert call(lib, _params(intermediate_size=100), B=0) == GR_ERR_UNSUPPORTED
    assert _call_ragged(lib, _params(), rows=0) == GR_ERR_ARG and b"rows_bound" in lib.gr_last_error()
    assert lib.gr_bert_embed_ragged_bf16_workspace_bytes(ctypes.byref(_params()), 4, 128, 0) == 0


def test_pointer_checks():
    """With a (host) workspace of the right size the pointer checks are reached; they all come before any launch."""
    import gr_amd
    lib = gr_amd.lib()
    p = _params(hidden_size=64, num_heads=1, intermediate_size=32, num_layers=1, vocab_size=8, max_position=8)
    n = lib.gr_bert_embed_bf16_workspace_bytes(ctypes.byref(p), 1, 4)
    assert n == 4 * (18 * 64 + 2 * 32) + 16
    buf = ctypes.create_string_buffer(n + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15
    ids = (ctypes.c_int64 * 4)()
    out = ctypes.create_string_buffer(64 * 4 * 4 + 16)
    outp = (ctypes.addressof(out) + 15) & ~15
    f = lambda ids_, pooling, pooled, hidden, ws_=ws, n_=n: lib.gr_bert_embed_bf16(
        ctypes.byref(p), ids_, None, None, 1, 4, pooling, pooled, hidden, ws_, n_, None)
    assert f(ids, 1, outp, None, ws + 4) == GR_ERR_WORKSPACE                 # misaligned
    assert f(ids, 1, outp, None, ws, n - 1) == GR_ERR_WORKSPACE              # too small
    assert f(None, 1, outp, None) == GR_ERR_ARG and b"input_ids" in lib.gr_last_error()
    assert f(ids, 1, None, None) == GR_ERR_ARG and b"pooled_out" in lib.gr_last_error()
    assert f(ids, 0, None, None) == GR_ERR_ARG and b"hidden_out" in lib.gr_last_error()
    assert f(ids, 0, None, outp + 4) == GR_ERR_ARG and b"hidden_out" in lib.gr_last_error()
    assert f(ids, 1, outp, None) == GR_ERR_ARG and b"weight pointer" in lib.gr_last_error()     # every weight is NULL


def test_workspace_is_smaller_than_fp32():
    import gr_amd
    lib = gr_amd.lib()
    p16, p32 = _params(), _params("BertParams")
    for B, S in [(32, 128), (32, 512), (1, 1), (7, 33)]:
        n16 = lib.gr_bert_embed_bf16_workspace_bytes(ctypes.byref(p16), B, S)
        n32 = lib.gr_bert_embed_workspace_bytes(ctypes.byref(p32), B, S)
        need = B * S * (18 * 768 + 2 * 3072)              # fp32 x and pre-LN sum; bf16 x, q/k/v, context, GELU output
        assert need <= n16 <= need + 128 and n16 < n32, (B, S, n16, n32)
        r16 = lib.gr_bert_embed_ragged_bf16_workspace_bytes(ctypes.byref(p16), B, S, B * S)
        r32 = lib.gr_bert_embed_ragged_workspace_bytes(ctypes.byref(p32), B, S, B * S)
        assert n16 < r16 < r32 and r16 - n16 == r32 - n32
    half = lib.gr_bert_embed_ragged_bf16_workspace_bytes(ctypes.byref(p16), 32, 128, 2048)
    assert half < lib.gr_bert_embed_ragged_bf16_workspace_bytes(ctypes.byref(p16), 32, 128, 4096)
    assert lib.gr_bert_embed_ragged_bf16_workspace_bytes(ctypes.byref(p16), 32, 128, 1 << 40) == \
        lib.gr_bert_embed_ragged_bf16_workspace_bytes(ctypes.byref(p16), 32, 128, 4096)


def test_module_refusals():
    import gr_amd
    fx = bf.fixture("bert_embed_main")
    m = gr_amd.bert_embed.BertEncoder(fx.cfg)
    m.load_state_dict(fx.sd)
    m.eval()
    with pytest.raises(ValueError, match="precision.*not built"):
        m.embed(fx.ids, fx.mask, precision="fp16")
    with pytest.raises(ValueError, match="precision='x'"):
        m.embed(fx.ids, fx.mask, precision="x")
    with pytest.raises(ValueError, match="precision"):
        m.embed(fx.ids, fx.mask, precision=None)
    tok = lambda texts, **kw: dict(input_ids=fx.ids[:len(texts)], attention_mask=fx.mask[:len(texts)])
    with pytest.raises(ValueError, match="precision.*not built"):
        gr_amd.bert_embed.encode_texts(["a", "b"], tok, m, "cpu", 2, 12, precision="fp16")
    with pytest.raises(ValueError, match="precision='int8'"):
        gr_amd.bert_embed.generate_user_profile_embedding({1: "a"}, tok, m, precision="int8")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.embed(fx.ids, fx.mask, precision="bf16")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gr_amd.ops.BertBf16Binding(m.config, fx.sd)
    m.train()
    with pytest.raises(NotImplementedError, match="training"):
        m.embed(fx.ids, fx.mask, precision="bf16")
    with pytest.raises(RuntimeError, match="no CPU fallback"), torch.no_grad():
        m.embed(fx.ids, fx.mask, pooling="cls", precision="bf16")
