"""Host-side surface of the BERT encoder (CPU): the restatement against the recorded ``transformers`` run, the
symbols, the workspace query and the envelope checks of the C ABI (every call passes NULL pointers; the shape checks
come first, so nothing reaches a device), the parameter tree of ``gr_amd.bert_embed.BertEncoder`` and its refusals."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import bert_cases as bc
import bert_embed_fixtures as bf
import bert_embed_ref as ref

GR_OK, GR_ERR_ARG, GR_ERR_UNSUPPORTED, GR_ERR_WORKSPACE = 0, -1, -2, -4
BASE = dict(vocab_size=30522, hidden_size=768, num_heads=12, head_dim=64, intermediate_size=3072, num_layers=12,
            max_position=512, type_vocab_size=2, hidden_act=0, position_type=0, eps=1e-12)
LARGE = dict(hidden_size=1024, num_heads=16, intermediate_size=4096, num_layers=24)
CONFIG = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
              hidden_act="gelu", max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12)
SMALL = dict(vocab_size=48, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
             hidden_act="gelu", max_position_embeddings=24, type_vocab_size=2, layer_norm_eps=1e-12)


def _params(**kw):
    from gr_amd import _lib as L
    p = L.BertParams()
    for k, v in dict(BASE, **kw).items():
        setattr(p, k, v)
    return p


def _call(lib, p, B=4, S=128, pooling=1, ws=0):
    return lib.gr_bert_embed_f32(ctypes.byref(p), None, None, None, B, S, pooling, None, None, None, ws, None)


# ---- the restatement against the recorded transformers run

@pytest.mark.parametrize("name", bf.NAMES)
def test_restatement_against_the_recorded_run(name):
    fx = bf.fixture(name)
    r64 = ref.run(fx.cfg, fx.sd, fx.ids, fx.mask, fx.type_ids, torch.float64)
    r32 = ref.run(fx.cfg, fx.sd, fx.ids, fx.mask, fx.type_ids, torch.float32)
    for k in ("hidden", "mean_no_cls", "cls"):
        on = fx.mask if k == "hidden" else None
        assert ref.live_err(r64[k], fx.r64[k], on) <= 1e-12, k                # the recorded float64 run, another host
        assert ref.live_err(r32[k], fx.hf[k], on) <= 1e-5, k                  # HF's float32 run
    err = ref.measure(r32, fx.r64, fx.mask)
    for k, v in err.items():
        print(f"{name}: {k} {v:.3e} (recorded {fx.meta[k]:.3e})")
        assert v <= 4 * fx.meta[k], (k, v, fx.meta[k])
    # a mean that includes the [CLS] row is far outside what the GPU tests accept
    apart = ref.live_err(ref.pool(fx.r64["hidden"], fx.mask, "mean_with_cls"), fx.r64["mean_no_cls"])
    assert apart > 100 * fx.meta["pooled_err32"]
    # HF's pooling lines on HF's hidden state (T5/item_encode.py:74-75, bert_emb.py:160-165)
    m = fx.mask.float()
    want = (fx.hf["hidden"] * m.unsqueeze(-1))[:, 1:].sum(1) / m[:, 1:].sum(-1, keepdim=True).clamp(min=1e-9)
    assert torch.equal(want, fx.hf["mean_no_cls"]) and torch.equal(fx.hf["hidden"][:, 0], fx.hf["cls"])


def test_one_fixture_has_token_types_and_a_hole():
    fx = bf.fixture("bert_embed_types")
    assert int(fx.type_ids.sum()) > 0
    row = fx.mask[0].tolist()
    assert row[3] == 0 and row[2] == 1 and row[4] == 1                       # a hole, live on both sides
    assert int(fx.mask[1, 0]) == 0 and int(fx.mask[1, 1]) == 1              # a masked [CLS] position


def test_restatement_edge_semantics():
    c = bc.case("tiny")
    r64 = bc.restated("tiny", torch.float64)
    assert c.mask[1].tolist() == [1] + [0] * 32
    assert r64["mean_no_cls"][1].abs().max() == 0 and r64["cls"][1].abs().max() > 0     # [CLS] only: mean 0
    mask = c.mask.clone()
    mask[2] = 0                                                                       # no live key: zeros
    out = ref.run(c.cfg, c.sd, c.ids, mask, None, torch.float64)
    assert out["hidden"][2].abs().max() == 0 and out["cls"][2].abs().max() == 0 and out["mean_no_cls"][2].abs().max() == 0
    keep = [0, 1, 3, 4, 5]
    assert torch.equal(out["hidden"][keep][c.mask[keep] != 0], r64["hidden"][keep][c.mask[keep] != 0])
    assert torch.isfinite(out["hidden"]).all()


# ---- the C ABI

def test_symbols_are_exported_and_bound():
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    for name in ("gr_bert_embed_workspace_bytes", "gr_bert_embed_f32"):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert ctypes.sizeof(L.BertParams) == 10 * 4 + 2 * 4 + 5 * 8 + 24 * 16 * 8
    assert len(gr_amd.ops.BERT_LAYER_KEYS) == 16
    assert "bert_embed" in gr_amd.__all__ and callable(gr_amd.ops.bert_embed)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gr_amd.h")).read()
    declared = {w.split("(")[0] for w in header.replace("\n", " ").split() if w.startswith("gr_") and "(" in w}
    assert {n for n in L.SIGNATURES if "bert" in n} == {n for n in declared if "bert" in n}


def test_workspace_query():
    import gr_amd
    lib = gr_amd.lib()
    p = _params()
    q = lambda *a: lib.gr_bert_embed_workspace_bytes(ctypes.byref(p), *a)
    need = lambda B, S: 4 * B * S * (6 * 768 + 3072)       # x, pre-LN, q/k/v, context: 6 H; the intermediate tile
    for B, S in [(1, 1), (32, 128), (32, 512), (7, 33), (2 ** 16, 512)]:
        assert need(B, S) <= q(B, S) <= need(B, S) + 128, (B, S)
    sizes = [q(B, 64) for B in (1, 2, 3, 17, 256)] + [q(256, S) for S in (65, 128, 511, 512)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))                          # monotone inside the envelope
    assert q(0, 128) > 0
    for bad in [(1, 0), (1, 513), (-1, 128), (2 ** 16 + 1, 128), (2 ** 40, 128)]:
        assert q(*bad) == 0, bad
    assert lib.gr_bert_embed_workspace_bytes(None, 1, 128) == 0
    assert lib.gr_bert_embed_workspace_bytes(ctypes.byref(_params(hidden_size=776)), 1, 128) == 0
    assert lib.gr_bert_embed_workspace_bytes(ctypes.byref(_params(max_position=100)), 1, 101) == 0


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
def test_c_abi_refuses_what_is_outside_the_envelope(kw, call, word):
    import gr_amd
    lib = gr_amd.lib()
    assert _call(lib, _params(**kw), **call) == GR_ERR_UNSUPPORTED
    msg = lib.gr_last_error()
    assert msg.startswith(b"gr_bert_embed_f32: ") and word in msg, msg


@pytest.mark.parametrize("kw", [
    {}, LARGE, dict(hidden_size=32, num_heads=1, head_dim=32), dict(hidden_size=64, num_heads=1), dict(intermediate_size=32),
    dict(intermediate_size=4096), dict(num_layers=1), dict(num_layers=24), dict(vocab_size=21128),
])
def test_envelope_edges_are_inside(kw):
    """bert-base, bert-large, chinese-roberta-wwm-ext's vocabulary and the edges pass the shape checks (they stop at
    the workspace)."""
    import gr_amd
    lib = gr_amd.lib()
    for S in (1, 128, 512):
        for pooling in (0, 1, 2):
            assert _call(lib, _params(**kw), S=S, pooling=pooling) == GR_ERR_WORKSPACE
        assert lib.gr_bert_embed_workspace_bytes(ctypes.byref(_params(**kw)), 2 ** 16, S) > 0


def test_c_abi_argument_order():
    import gr_amd
    lib = gr_amd.lib()
    assert _call(lib, _params(), B=-1) == GR_ERR_ARG
    assert lib.gr_bert_embed_f32(None, None, None, None, 1, 128, 1, None, None, None, 0, None) == GR_ERR_ARG
    assert _call(lib, _params(hidden_size=776), B=-1) == GR_ERR_ARG          # ARG before UNSUPPORTED
    assert _call(lib, _params(hidden_size=776)) == GR_ERR_UNSUPPORTED        # UNSUPPORTED before WORKSPACE
    for pooling in (-1, 3):
        assert _call(lib, _params(), pooling=pooling) == GR_ERR_ARG and b"pooling" in lib.gr_last_error()
    assert _call(lib, _params()) == GR_ERR_WORKSPACE
    assert _call(lib, _params(), ws=1 << 40) == GR_ERR_WORKSPACE             # a NULL workspace of any size
    assert b"gr_bert_embed_workspace_bytes" in lib.gr_last_error()
    assert _call(lib, _params(), B=0) == GR_OK                                # nothing to do, nothing launched
    assert _call(lib, _params(intermediate_size=100), B=0) == GR_ERR_UNSUPPORTED


def test_c_abi_pointer_checks():
    """With a (host) workspace of the right size the pointer checks are reached; they all come before any launch."""
    import gr_amd
    lib = gr_amd.lib()
    p = _params(hidden_size=64, num_heads=1, intermediate_size=32, num_layers=1, vocab_size=8, max_position=8)
    n = lib.gr_bert_embed_workspace_bytes(ctypes.byref(p), 1, 4)
    buf = ctypes.create_string_buffer(n + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15
    ids = (ctypes.c_int64 * 4)()
    out = ctypes.create_string_buffer(64 * 4 * 4 + 16)
    outp = (ctypes.addressof(out) + 15) & ~15
    f = lambda ids_, pooling, pooled, hidden, ws_=ws, n_=n: lib.gr_bert_embed_f32(
        ctypes.byref(p), ids_, None, None, 1, 4, pooling, pooled, hidden, ws_, n_, None)
    assert f(ids, 1, outp, None, ws + 4) == GR_ERR_WORKSPACE                 # misaligned
    assert f(ids, 1, outp, None, ws, n - 1) == GR_ERR_WORKSPACE              # too small
    assert f(None, 1, outp, None) == GR_ERR_ARG and b"input_ids" in lib.gr_last_error()
    assert f(ids, 1, None, None) == GR_ERR_ARG and b"pooled_out" in lib.gr_last_error()
    assert f(ids, 2, None, outp) == GR_ERR_ARG and b"pooled_out" in lib.gr_last_error()
    assert f(ids, 0, None, None) == GR_ERR_ARG and b"hidden_out" in lib.gr_last_error()
    assert f(ids, 0, None, outp + 4) == GR_ERR_ARG and b"hidden_out" in lib.gr_last_error()
    assert f(ids, 1, outp, None) == GR_ERR_ARG and b"weight pointer" in lib.gr_last_error()     # every weight is NULL


# ---- the module

@pytest.mark.parametrize("name", bf.NAMES)
def test_parameter_tree_is_bert_models(name):
    import gr_amd
    fx = bf.fixture(name)
    m = gr_amd.bert_embed.BertEncoder(fx.cfg)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == fx.meta["keys"]
    assert fx.meta["keys"] == ref.state_keys(fx.cfg)
    m.load_state_dict(fx.sd)                                                  # strict
    old = dict(fx.sd, **{"embeddings.position_ids": torch.arange(fx.cfg["max_position_embeddings"]).unsqueeze(0)})
    m.load_state_dict(old)                                                    # an old checkpoint's buffer is ignored
    with pytest.raises(RuntimeError, match="pooler.dense.bias"):
        m.load_state_dict({k: v for k, v in fx.sd.items() if k != "pooler.dense.bias"})
    assert torch.equal(m.encoder.layer[0].attention.self.query.weight, fx.sd["encoder.layer.0.attention.self.query.weight"])
    assert m.embeddings.LayerNorm.eps == 1e-12


def test_config_objects_and_defaults():
    import gr_amd

    class Cfg:
        pass
    c = Cfg()
    for k, v in SMALL.items():
        setattr(c, k, v)
    m = gr_amd.bert_embed.BertEncoder(c)
    assert m.config["hidden_size"] == 64 and m.config["position_embedding_type"] == "absolute"
    with pytest.raises(ValueError, match="hidden_size"):
        gr_amd.bert_embed.BertEncoder({k: v for k, v in SMALL.items() if k != "hidden_size"})


def test_transformers_is_not_imported():
    """A fresh interpreter: other tests of the session may have imported it."""
    code = ("import sys; import gr_amd; from gr_amd.bert_embed import BertEncoder; "
            f"BertEncoder({SMALL!r}); assert 'transformers' not in sys.modules, 'transformers was imported'")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


@pytest.mark.parametrize("delta, word", [
    (dict(hidden_size=776), "hidden_size"), (dict(hidden_size=2048, num_attention_heads=32), "hidden_size"),
    (dict(num_attention_heads=16), "num_attention_heads"), (dict(num_attention_heads=6), "num_attention_heads"),
    (dict(intermediate_size=3080), "intermediate_size"), (dict(intermediate_size=8192), "intermediate_size"),
    (dict(num_hidden_layers=0), "num_hidden_layers"), (dict(num_hidden_layers=25), "num_hidden_layers"),
    (dict(hidden_act="relu"), "hidden_act"), (dict(hidden_act="gelu_new"), "hidden_act"),
    (dict(position_embedding_type="relative_key"), "position_embedding_type"),
    (dict(max_position_embeddings=0), "max_position_embeddings"),
])
def test_module_refuses_what_is_outside_the_envelope(delta, word):
    import gr_amd
    with pytest.raises(NotImplementedError, match="BERT encoder: ") as e:
        gr_amd.bert_embed.BertEncoder(dict(CONFIG, **delta))
    assert word in str(e.value) and "no CPU fallback" in str(e.value)


def test_module_refuses_shapes_outside_the_envelope():
    import gr_amd
    with pytest.raises(NotImplementedError, match="513 positions"):
        gr_amd.ops.bert_check(dict(CONFIG, max_position_embeddings=1024), S=513)
    with pytest.raises(NotImplementedError, match="max_position_embeddings"):
        gr_amd.ops.bert_check(SMALL, S=25)
    with pytest.raises(NotImplementedError, match="65537 sequences"):
        gr_amd.ops.bert_check(CONFIG, S=8, B=2 ** 16 + 1)
    gr_amd.ops.bert_check(CONFIG, S=512, B=2 ** 16)
    gr_amd.ops.bert_check(dict(CONFIG, vocab_size=21128), S=1, B=1)             # chinese-roberta-wwm-ext
    gr_amd.ops.bert_check(dict(CONFIG, hidden_size=1024, num_attention_heads=16, intermediate_size=4096,
                               num_hidden_layers=24), S=512)                     # bert-large


def test_training_and_cpu_are_refused():
    import gr_amd
    fx = bf.fixture("bert_embed_main")
    m = gr_amd.bert_embed.BertEncoder(fx.cfg)
    m.load_state_dict(fx.sd)
    m.train()
    with pytest.raises(NotImplementedError, match="training"):
        m(input_ids=fx.ids, attention_mask=fx.mask)
    with pytest.raises(NotImplementedError, match="training"):
        m.embed(fx.ids, fx.mask)
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(input_ids=fx.ids, attention_mask=fx.mask, token_type_ids=fx.type_ids)
    with pytest.raises(RuntimeError, match="no CPU fallback"), torch.no_grad():
        m.train().embed(fx.ids, fx.mask, pooling="cls")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gr_amd.ops.BertBinding(m.config, fx.sd)
    with pytest.raises(ValueError, match="pooling"):
        m.eval().embed(fx.ids, fx.mask, pooling="mean")
    tok = lambda texts, **kw: dict(input_ids=fx.ids[:len(texts)], attention_mask=fx.mask[:len(texts)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gr_amd.bert_embed.encode_texts(["a", "b"], tok, m, "cpu", 2, 12)
