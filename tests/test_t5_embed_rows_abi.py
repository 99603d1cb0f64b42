"""Host-side surface of the T5 embedding retriever's packed entry (CPU): the three symbols, the workspace query and
its identity with the dense one, the refusals of the C ABI (the shape checks come before any pointer is used, so
nothing reaches a device), and ``collate_ids`` against ``collate`` on the same samples as vectors."""
import ctypes

import numpy as np
import pytest
import torch

import t5_embed_fixtures as tf

GR_OK, GR_ERR_ARG, GR_ERR_UNSUPPORTED, GR_ERR_WORKSPACE = 0, -1, -2, -4
DEPLOYED = dict(d_model=512, d_kv=16, n_heads=4, d_ff=256, n_layers=6, in_dim=768, out_dim=768, n_buckets=32, eps=1e-6)
# every width t5e_check refuses (test_t5_embed_abi.py's list), with the word its message carries
BAD_WIDTHS = [
    (dict(d_model=48), b"d_model"), (dict(d_model=544), b"d_model"), (dict(d_model=0), b"d_model"),
    (dict(d_kv=12), b"d_kv"), (dict(d_kv=128, n_heads=1), b"d_kv"),
    (dict(n_heads=17), b"n_heads * d_kv"), (dict(n_heads=0), b"n_heads * d_kv"),
    (dict(d_ff=1056), b"d_ff"), (dict(d_ff=100), b"d_ff"), (dict(d_ff=0), b"d_ff"),
    (dict(in_dim=770), b"in_dim"), (dict(in_dim=1028), b"in_dim"), (dict(in_dim=0), b"in_dim"),
    (dict(out_dim=6), b"out_dim"), (dict(out_dim=1028), b"out_dim"),
    (dict(n_layers=0), b"n_layers"), (dict(n_layers=9), b"n_layers"), (dict(n_buckets=16), b"n_buckets"),
]
# an address nothing is stored at: the calls below are all refused before they would use it
FAKE = 1 << 20


def _params(**kw):
    from gr_amd import _lib as L
    p = L.T5EmbedParams()
    for k, v in dict(DEPLOYED, **kw).items():
        setattr(p, k, v)
    return p


def _rows(lib, p, B=4, rows=40, R=100, projected=None, ws=None, ws_bytes=0):
    return lib.gr_t5_embed_rows_f32(ctypes.byref(p), projected, R, None, None, B, rows, None, None, ws, ws_bytes, None)


def test_symbols_are_exported_and_bound():
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    for name in ("gr_t5_embed_project_f32", "gr_t5_embed_rows_workspace_bytes", "gr_t5_embed_rows_f32"):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    for name in ("t5_embed_project", "t5_embed_rows"):
        assert callable(getattr(gr_amd.ops, name))
    for name in ("Tables", "collate_ids", "evaluate_ids", "eval_loss_ids"):
        assert callable(getattr(gr_amd.t5_embed, name))
    assert callable(gr_amd.t5_embed.TIGER.embed_rows)


@pytest.mark.parametrize("kw", [{}, dict(d_model=32, d_kv=8, n_heads=1, d_ff=32, in_dim=4, out_dim=4, n_layers=1),
                                dict(d_kv=64, d_ff=1024, in_dim=1024, out_dim=1024, n_layers=8)])
def test_workspace_query(kw):
    import gr_amd
    lib = gr_amd.lib()
    p = _params(**kw)
    q = lambda B, rows: lib.gr_t5_embed_rows_workspace_bytes(ctypes.byref(p), B, rows)
    dense = lambda B, S: lib.gr_t5_embed_workspace_bytes(ctypes.byref(p), B, S)
    for B, S in [(1, 1), (7, 21), (256, 21), (3, 32)]:
        assert q(B, B * S) == dense(B, S) > 0, (B, S)
        if S > 1:
            for rows in (B, B * S - 1):                      # strictly smaller with fewer rows
                assert 0 < q(B, rows) < dense(B, S), (B, S, rows)
    assert q(2 ** 20, 32 * 2 ** 20) == dense(2 ** 20, 32)
    for bad in [(4, 3), (4, 0), (4, -1), (4, 129), (1, 33), (-1, 0), (-1, -1), (2 ** 20 + 1, 2 ** 20 + 1), (2 ** 40, 2 ** 40)]:
        assert q(*bad) == 0, bad
    assert lib.gr_t5_embed_rows_workspace_bytes(None, 4, 40) == 0


@pytest.mark.parametrize("kw, word", BAD_WIDTHS)
def test_refused_widths(kw, word):
    import gr_amd
    lib = gr_amd.lib()
    p = _params(**kw)
    assert lib.gr_t5_embed_rows_workspace_bytes(ctypes.byref(p), 4, 40) == 0
    assert _rows(lib, p) == GR_ERR_UNSUPPORTED
    msg = lib.gr_last_error()
    assert msg.startswith(b"gr_t5_embed_rows_f32: ") and word in msg, msg
    assert lib.gr_t5_embed_project_f32(ctypes.byref(p), None, 10, None, None) == GR_ERR_UNSUPPORTED
    msg = lib.gr_last_error()
    assert msg.startswith(b"gr_t5_embed_project_f32: ") and word in msg, msg


@pytest.mark.parametrize("call, code, word", [
    (dict(B=4, rows=3), GR_ERR_UNSUPPORTED, b"rows"), (dict(B=4, rows=129), GR_ERR_UNSUPPORTED, b"rows"),
    (dict(B=4, rows=-1), GR_ERR_UNSUPPORTED, b"rows"), (dict(B=0, rows=1), GR_ERR_UNSUPPORTED, b"rows"),
    (dict(B=2 ** 20 + 1, rows=2 ** 20 + 1), GR_ERR_UNSUPPORTED, b"B must be"),
    (dict(B=-1, rows=0), GR_ERR_ARG, b"negative batch"),
    (dict(R=0), GR_ERR_ARG, b"R must be"), (dict(R=-5), GR_ERR_ARG, b"R must be"),
    (dict(R=2 ** 24 + 1), GR_ERR_UNSUPPORTED, b"R must be"),
])
def test_rows_refusals(call, code, word):
    import gr_amd
    lib = gr_amd.lib()
    assert _rows(lib, _params(), **call) == code
    msg = lib.gr_last_error()
    assert msg.startswith(b"gr_t5_embed_rows_f32: ") and word in msg, msg


def test_rows_argument_order():
    import gr_amd
    lib = gr_amd.lib()
    p = _params()
    assert lib.gr_t5_embed_rows_f32(None, None, 100, None, None, 4, 40, None, None, None, 0, None) == GR_ERR_ARG
    assert _rows(lib, _params(d_model=48), B=-1, rows=0) == GR_ERR_ARG          # ARG before UNSUPPORTED
    assert _rows(lib, p) == GR_ERR_WORKSPACE                                     # inside the envelope, no workspace
    assert b"gr_t5_embed_rows_workspace_bytes" in lib.gr_last_error()
    assert _rows(lib, p, ws_bytes=1 << 40) == GR_ERR_WORKSPACE                  # a NULL workspace of any size
    need = lib.gr_t5_embed_rows_workspace_bytes(ctypes.byref(p), 4, 40)
    assert _rows(lib, p, ws=FAKE, ws_bytes=need - 1) == GR_ERR_WORKSPACE
    assert _rows(lib, p, ws=FAKE + 4, ws_bytes=need) == GR_ERR_WORKSPACE        # misaligned
    # with a workspace the pointers are looked at: NULL, then projected's alignment
    assert _rows(lib, p, ws=FAKE, ws_bytes=need) == GR_ERR_ARG and b"null pointer" in lib.gr_last_error()
    rc = lib.gr_t5_embed_rows_f32(ctypes.byref(p), FAKE + 4, 100, FAKE, FAKE, 4, 40, FAKE, None, FAKE, need, None)
    assert rc == GR_ERR_ARG and b"projected must be 16-byte aligned" in lib.gr_last_error()
    assert _rows(lib, p, B=0, rows=0) == GR_OK                                   # nothing to do, nothing launched
    assert _rows(lib, _params(d_ff=100), B=0, rows=0) == GR_ERR_UNSUPPORTED


def test_project_refusals():
    import gr_amd
    lib = gr_amd.lib()
    p = _params()
    call = lambda table, R, projected: lib.gr_t5_embed_project_f32(ctypes.byref(p), table, R, projected, None)
    assert lib.gr_t5_embed_project_f32(None, FAKE, 10, FAKE, None) == GR_ERR_ARG
    for R in (0, -3):
        assert call(FAKE, R, FAKE) == GR_ERR_ARG and b"R must be" in lib.gr_last_error()
    assert call(FAKE, 2 ** 24 + 1, FAKE) == GR_ERR_UNSUPPORTED and b"R must be" in lib.gr_last_error()
    assert call(None, 10, FAKE) == GR_ERR_ARG and b"null pointer" in lib.gr_last_error()
    assert call(FAKE, 10, None) == GR_ERR_ARG and b"null pointer" in lib.gr_last_error()
    assert call(FAKE, 10, FAKE + 8) == GR_ERR_ARG and b"projected must be 16-byte aligned" in lib.gr_last_error()
    assert call(FAKE + 4, 10, FAKE) == GR_ERR_ARG and b"16-byte aligned" in lib.gr_last_error()
    assert call(FAKE, 10, FAKE) == GR_ERR_ARG and b"weight pointer" in lib.gr_last_error()     # params hold no weights


def _samples(rng, n_items, n_users, lengths):
    return [dict(history=rng.integers(0, n_items, n - 1).tolist(), user_id=int(rng.integers(1, n_users + 1)),
                 target_id=int(rng.integers(0, n_items))) for n in lengths]


def test_collate_ids_is_collate_without_the_vectors():
    """The reference's __getitem__ on seeded tables, then ``collate``; against ``collate_ids`` gathered densely."""
    from gr_amd import t5_embed
    rng = np.random.default_rng(3)
    n_items, n_users, dim = 50, 9, 8
    items = rng.standard_normal((n_items, dim)).astype(np.float32)
    users = rng.standard_normal((n_users, dim)).astype(np.float32)
    samples = _samples(rng, n_items, n_users, [5, 2, 32, 21, 3])
    vectors = [dict(seq_embs=np.concatenate([users[s["user_id"] - 1][None], items[s["history"]]], axis=0),
                    seq_len=len(s["history"]) + 1, target_emb=items[s["target_id"]], target_id=s["target_id"],
                    user_id=s["user_id"]) for s in samples]
    want = t5_embed.collate(vectors)
    got = t5_embed.collate_ids(samples, n_items)
    assert set(got) == {"tokens", "offsets", "target_id", "user_id"}
    assert all(got[k].dtype == torch.int64 and got[k].dim() == 1 for k in got)
    tokens, offsets = got["tokens"].numpy(), got["offsets"].numpy()
    assert offsets[0] == 0 and offsets[-1] == len(tokens) == 5 + 2 + 32 + 21 + 3
    table = np.concatenate([items, users], axis=0)
    B, S = len(samples), int(np.diff(offsets).max())
    seq, mask = np.zeros((B, S, dim), np.float32), np.zeros((B, S), np.int64)
    for b in range(B):
        n = offsets[b + 1] - offsets[b]
        seq[b, :n] = table[tokens[offsets[b]:offsets[b + 1]]]
        mask[b, :n] = 1
    assert np.array_equal(seq, want["seq_embs"].numpy()) and np.array_equal(mask, want["attention_mask"].numpy())
    assert np.array_equal(items[got["target_id"].numpy()], want["target_emb"].numpy())
    assert torch.equal(got["target_id"], want["target_id"]) and torch.equal(got["user_id"], want["user_id"])
    assert tokens[0] == n_items + samples[0]["user_id"] - 1                 # data_vision.py:135


def test_collate_ids_refuses_on_the_host():
    from gr_amd import t5_embed
    ok = dict(history=[1, 2], user_id=1, target_id=3)
    with pytest.raises(ValueError, match="empty history"):
        t5_embed.collate_ids([ok, dict(history=[], user_id=2, target_id=3)], 10)
    with pytest.raises(ValueError, match="33 rows"):
        t5_embed.collate_ids([dict(history=list(range(32)), user_id=2, target_id=3), ok], 40)
    with pytest.raises(ValueError, match="empty batch"):
        t5_embed.collate_ids([], 10)
    assert t5_embed.collate_ids([dict(history=list(range(31)), user_id=2, target_id=3)], 40)["offsets"].tolist() == [0, 32]


def test_cpu_tensors_are_refused():
    import gr_amd
    fx = tf.fixture("t5e_main")
    m = gr_amd.t5_embed.TIGER(fx.params)
    m.load_state_dict(fx.state_dict())
    m.eval()
    items = torch.randn(10, fx.cfg["input_emb_dim"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gr_amd.t5_embed.Tables(m, items, torch.randn(3, fx.cfg["input_emb_dim"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gr_amd.t5_embed.Tables(m, items.numpy())
