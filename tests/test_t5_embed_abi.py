"""Host-side surface of the T5 embedding retriever (CPU): the symbols, the workspace query, the envelope checks
of the C ABI (every call passes NULL pointers; the shape checks come first, so nothing reaches a device),
the parameter tree of ``gr_amd.t5_embed.TIGER``, and the metric tail's arithmetic."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest
import torch

import t5_embed_fixtures as tf
import t5_embed_ref as ref

GR_OK, GR_ERR_ARG, GR_ERR_UNSUPPORTED, GR_ERR_WORKSPACE = 0, -1, -2, -4
DEPLOYED = dict(d_model=512, d_kv=16, n_heads=4, d_ff=256, n_layers=6, in_dim=768, out_dim=768, n_buckets=32, eps=1e-6)
PARAMS = dict(d_model=512, d_ff=256, num_heads=4, d_kv=16, dropout_rate=0.1, num_layers=2, input_emb_dim=768,
              target_emb_dim=768, temperature=0.07)


def _params(**kw):
    from gr_amd import _lib as L
    p = L.T5EmbedParams()
    for k, v in dict(DEPLOYED, **kw).items():
        setattr(p, k, v)
    return p


def _call(lib, p, B=4, S=21, ws=0):
    return lib.gr_t5_embed_f32(ctypes.byref(p), None, None, B, S, None, None, None, ws, None)


def test_symbols_are_exported_and_bound():
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    for name in ("gr_t5_embed_workspace_bytes", "gr_t5_embed_f32"):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert ctypes.sizeof(L.T5EmbedParams) == 8 * 4 + 2 * 4 + 7 * 8 + 8 * 8 * 8
    assert gr_amd.t5_embed.TIGER is not gr_amd.TIGER and callable(gr_amd.ops.t5_embed)
    assert "t5_embed" in gr_amd.__all__


def test_workspace_query():
    import gr_amd
    lib = gr_amd.lib()
    p = _params()
    q = lambda *a: lib.gr_t5_embed_workspace_bytes(ctypes.byref(p), *a)
    # per token row x [d_model], q/k/v [3 inner], the feed-forward tile [d_ff]; per user pooled and pred
    need = lambda B, S: 4 * (B * S * (512 + 192 + 256) + B * (512 + 768))
    for B, S in [(1, 21), (256, 21), (7, 32), (3, 1)]:
        assert need(B, S) <= q(B, S) <= need(B, S) + 128, (B, S)
    assert q(0, 21) > 0 and q(2 ** 20, 32) >= need(2 ** 20, 32)
    for bad in [(1, 0), (1, 33), (-1, 21), (2 ** 20 + 1, 21), (2 ** 40, 21)]:
        assert q(*bad) == 0, bad
    assert lib.gr_t5_embed_workspace_bytes(None, 1, 21) == 0
    assert lib.gr_t5_embed_workspace_bytes(ctypes.byref(_params(d_model=520)), 1, 21) == 0


@pytest.mark.parametrize("kw, call, word", [
    (dict(d_model=48), {}, b"d_model"), (dict(d_model=544), {}, b"d_model"), (dict(d_model=0), {}, b"d_model"),
    (dict(d_kv=12), {}, b"d_kv"), (dict(d_kv=128, n_heads=1), {}, b"d_kv"),
    (dict(n_heads=17), {}, b"n_heads * d_kv"), (dict(n_heads=0), {}, b"n_heads * d_kv"),
    (dict(d_ff=1056), {}, b"d_ff"), (dict(d_ff=100), {}, b"d_ff"), (dict(d_ff=0), {}, b"d_ff"),
    (dict(in_dim=770), {}, b"in_dim"), (dict(in_dim=1028), {}, b"in_dim"), (dict(in_dim=0), {}, b"in_dim"),
    (dict(out_dim=6), {}, b"out_dim"), (dict(out_dim=1028), {}, b"out_dim"),
    (dict(n_layers=0), {}, b"n_layers"), (dict(n_layers=9), {}, b"n_layers"),
    (dict(n_buckets=16), {}, b"n_buckets"),
    ({}, dict(S=0), b"S must be"), ({}, dict(S=33), b"S must be"),
    ({}, dict(B=2 ** 20 + 1), b"B must be"), ({}, dict(B=2 ** 31), b"B must be"),
])
def test_c_abi_refuses_what_is_outside_the_envelope(kw, call, word):
    import gr_amd
    lib = gr_amd.lib()
    assert _call(lib, _params(**kw), **call) == GR_ERR_UNSUPPORTED
    msg = lib.gr_last_error()
    assert msg.startswith(b"gr_t5_embed_f32: ") and word in msg, msg


@pytest.mark.parametrize("kw", [
    {}, dict(d_model=32, d_kv=8, n_heads=1), dict(d_model=64, d_kv=64, n_heads=4), dict(d_ff=32), dict(d_ff=1024),
    dict(in_dim=4, out_dim=4), dict(in_dim=1024, out_dim=1024), dict(n_layers=1), dict(n_layers=8),
])
def test_envelope_edges_are_inside(kw):
    """The deployed configuration and the edges of the envelope pass the shape checks (they stop at the workspace)."""
    import gr_amd
    lib = gr_amd.lib()
    for S in (1, 21, 32):
        assert _call(lib, _params(**kw), S=S) == GR_ERR_WORKSPACE
        assert lib.gr_t5_embed_workspace_bytes(ctypes.byref(_params(**kw)), 2 ** 20, S) > 0


def test_c_abi_argument_order():
    import gr_amd
    lib = gr_amd.lib()
    assert _call(lib, _params(), B=-1) == GR_ERR_ARG
    assert lib.gr_t5_embed_f32(None, None, None, 1, 21, None, None, None, 0, None) == GR_ERR_ARG
    assert _call(lib, _params(d_model=48), B=-1) == GR_ERR_ARG              # ARG before UNSUPPORTED
    assert _call(lib, _params(d_model=48)) == GR_ERR_UNSUPPORTED            # UNSUPPORTED before WORKSPACE
    assert _call(lib, _params()) == GR_ERR_WORKSPACE
    assert _call(lib, _params(), ws=1 << 40) == GR_ERR_WORKSPACE            # a NULL workspace of any size
    assert b"gr_t5_embed_workspace_bytes" in lib.gr_last_error()
    assert _call(lib, _params(), B=0) == GR_OK                               # nothing to do, nothing launched
    assert _call(lib, _params(d_ff=100), B=0) == GR_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", tf.NAMES)
def test_parameter_tree_is_the_references(name):
    import gr_amd
    fx = tf.fixture(name)
    m = gr_amd.t5_embed.TIGER(fx.params)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == fx.meta["keys"]
    assert len(fx.meta["keys"]) == 56
    m.load_state_dict(fx.state_dict())             # strict
    assert m.model.encoder.embed_tokens is m.model.shared and m.model.shared.weight.shape == (32128, fx.cfg["d_model"])
    assert len(m.model.encoder.block) == 6 and fx.params["num_layers"] == 2       # six blocks whatever params says
    assert torch.equal(m.model.encoder.block[5].layer[1].DenseReluDense.wo.weight,
                       fx.sd["model.encoder.block.5.layer.1.DenseReluDense.wo.weight"])
    assert m.temperature == 0.07 and m.cosine_eps == 1e-8


def test_n_parameters_and_attributes():
    import gr_amd
    m = gr_amd.t5_embed.TIGER(dict(tf.fixture("t5e_main").params, temperature=0.2))
    assert m.temperature == 0.2
    total = sum(p.numel() for p in m.parameters())
    emb = 32128 * 64
    assert m.n_parameters == (f'#Embedding parameters: {emb}\n#Non-embedding parameters: {total - emb}\n'
                              f'#Total trainable parameters: {total}\n')


def test_transformers_is_not_imported():
    """A fresh interpreter: other tests of the session may have imported it."""
    code = ("import sys; import gr_amd; from gr_amd.t5_embed import TIGER; "
            "TIGER(dict(d_model=32, d_ff=32, num_heads=1, d_kv=8, dropout_rate=0.1, input_emb_dim=4, target_emb_dim=4)); "
            "assert 'transformers' not in sys.modules, 'transformers was imported'")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


@pytest.mark.parametrize("delta, word", [
    (dict(d_model=48), "d_model"), (dict(d_model=1024), "d_model"), (dict(d_kv=12), "d_kv"),
    (dict(num_heads=32), "num_heads * d_kv"), (dict(d_ff=2048), "d_ff"), (dict(input_emb_dim=770), "input_emb_dim"),
    (dict(target_emb_dim=2048), "target_emb_dim"), (dict(feed_forward_proj="gated-gelu"), "feed_forward_proj"),
])
def test_module_refuses_what_is_outside_the_envelope(delta, word):
    import gr_amd
    with pytest.raises(NotImplementedError, match="T5 embedding retriever: ") as e:
        gr_amd.t5_embed.TIGER(dict(PARAMS, **delta))
    assert word in str(e.value) and "no CPU fallback" in str(e.value)


def test_training_and_cpu_are_refused():
    import gr_amd
    fx = tf.fixture("t5e_main")
    m = gr_amd.t5_embed.TIGER(fx.params)
    m.load_state_dict(fx.state_dict())
    m.train()
    with pytest.raises(NotImplementedError, match="training"):
        m(fx.seq, fx.mask, target_emb=fx.target)
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(fx.seq, fx.mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"), torch.no_grad():
        m.train().generate(fx.seq, fx.mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gr_amd.ops.T5EmbedBinding(fx.cfg, fx.sd)
    with pytest.raises(NotImplementedError, match="1..32"):
        gr_amd.ops.t5_embed_check(fx.cfg, S=33)


def test_collate():
    from gr_amd import t5_embed
    rng = np.random.default_rng(0)
    samples = [dict(seq_embs=rng.standard_normal((n, 6)).astype(np.float32), seq_len=n,
                    target_emb=rng.standard_normal(4).astype(np.float32), target_id=10 + n, user_id=100 + n)
               for n in (3, 1, 5)]
    samples[1]["seq_embs"] = torch.from_numpy(samples[1]["seq_embs"])          # tensors are taken too
    out = t5_embed.collate(samples)
    assert out["seq_embs"].shape == (3, 5, 6) and out["seq_embs"].dtype == torch.float32
    assert out["attention_mask"].dtype == out["target_id"].dtype == out["user_id"].dtype == torch.int64
    assert out["attention_mask"].tolist() == [[1, 1, 1, 0, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1]]
    assert torch.equal(out["seq_embs"][0, :3], torch.from_numpy(samples[0]["seq_embs"]))
    assert out["seq_embs"][0, 3:].abs().max() == 0 and out["seq_embs"][1, 1:].abs().max() == 0
    assert out["target_emb"].shape == (3, 4) and out["target_id"].tolist() == [13, 11, 15]
    assert out["user_id"].tolist() == [103, 101, 105]


def test_metric_arithmetic_on_a_hand_made_topk():
    """Recall@k / NDCG@k are per-batch means, then the mean of the batch means (T5/evaluate.py:58-70)."""
    from gr_amd import t5_embed
    topk = [2, 5]
    ids_a = torch.tensor([[7, 3, 9, 1, 0], [4, 5, 6, 2, 8], [1, 2, 3, 4, 5]])
    tgt_a = torch.tensor([3, 8, 6])          # rank 2, rank 5, absent
    ids_b = torch.tensor([[5, 4, 3, 2, 1]])
    tgt_b = torch.tensor([5])                # rank 1
    per = [t5_embed.batch_metrics(ids_a, tgt_a, topk), t5_embed.batch_metrics(ids_b, tgt_b, topk)]
    rec, nd = t5_embed.average_metrics(per, topk)
    f32 = lambda v: float(np.float32(v))
    d = lambda r: np.float32(1.0) / np.log2(np.float32(r + 1))
    assert rec == {"Recall@2": (f32(np.float32(1) / np.float32(3)) + 1.0) / 2,
                   "Recall@5": (f32(np.float32(2) / np.float32(3)) + 1.0) / 2}
    assert nd["NDCG@2"] == pytest.approx((float(d(2)) / 3 + 1.0) / 2, rel=1e-6)
    assert nd["NDCG@5"] == pytest.approx(((float(d(2)) + float(d(5))) / 3 + 1.0) / 2, rel=1e-6)
    for m, (i, t) in zip(per, ((ids_a, tgt_a), (ids_b, tgt_b))):
        assert {k: v.item() for k, v in m.items()} == ref.metrics(i, t, topk)
    assert t5_embed.average_metrics([], topk) == ({"Recall@2": 0.0, "Recall@5": 0.0}, {"NDCG@2": 0.0, "NDCG@5": 0.0})
    with pytest.raises(NotImplementedError, match="1..64"):
        t5_embed.retrieve(torch.zeros(1, 4), torch.zeros(3, 4), 65)
