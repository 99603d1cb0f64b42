"""Host-side surface of the ragged BERT entry (CPU): the symbols, the workspace formula, the argument checks of
gr_bert_embed_ragged_f32 (NULL or host pointers only: every check comes before any device call), ``row_bound`` on host
masks and the module's refusals."""
import ctypes
import os
import re

import pytest
import torch

import bert_cases as bc
import bert_embed_fixtures as bf

GR_OK, GR_ERR_ARG, GR_ERR_UNSUPPORTED, GR_ERR_WORKSPACE = 0, -1, -2, -4
BASE = dict(vocab_size=30522, hidden_size=768, num_heads=12, head_dim=64, intermediate_size=3072, num_layers=12,
            max_position=512, type_vocab_size=2, hidden_act=0, position_type=0, eps=1e-12)
PREFIX = b"gr_bert_embed_ragged_f32: "


def _params(**kw):
    from gr_amd import _lib as L
    p = L.BertParams()
    for k, v in dict(BASE, **kw).items():
        setattr(p, k, v)
    return p


def _call(lib, p, B=4, S=128, rows=None, pooling=1, ws=0):
    rows = B * S if rows is None else rows
    return lib.gr_bert_embed_ragged_f32(ctypes.byref(p), None, None, None, B, S, rows, pooling, None, None, None, None,
                                        ws, None)


def _up16(n):
    return (n + 15) // 16 * 16


def _formula(B, S, rows, H=768, I=3072):
    """include/gr_amd.h: 4 R (6 H + intermediate_size) + up16(8 (B + 1)) + 16 + up16(4 B) + 16, R = min(rows, B S)."""
    return 4 * min(rows, B * S) * (6 * H + I) + _up16(8 * (B + 1)) + 16 + _up16(4 * B) + 16


def test_symbols_are_exported_declared_and_bound():
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gr_amd.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S).replace("\n", " ")
    kinds = {"const gr_bert_params*": ctypes.POINTER(L.BertParams), "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
             "size_t": ctypes.c_size_t}
    for name in ("gr_bert_embed_ragged_workspace_bytes", "gr_bert_embed_ragged_f32"):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
        m = re.search(r"(\w+)\s+" + name + r"\(([^)]*)\)", flat)
        assert m, name
        args = [a.strip().rsplit(" ", 1)[0].strip() for a in m.group(2).split(",")]
        want = [kinds.get(a, ctypes.c_void_p) for a in args]          # every other argument is a pointer
        assert all(a in kinds or a.endswith("*") for a in args), args
        assert want == L.SIGNATURES[name][1], (name, args)
        assert L.SIGNATURES[name][0] == (ctypes.c_size_t if m.group(1) == "size_t" else ctypes.c_int)
    assert len(L.SIGNATURES["gr_bert_embed_ragged_f32"][1]) == len(L.SIGNATURES["gr_bert_embed_f32"][1]) + 2
    assert callable(gr_amd.ops.bert_embed_ragged) and callable(gr_amd.bert_embed.row_bound)


def test_workspace_query():
    import gr_amd
    lib = gr_amd.lib()
    p = _params()
    q = lambda *a: lib.gr_bert_embed_ragged_workspace_bytes(ctypes.byref(p), *a)
    padded = lambda B, S: lib.gr_bert_embed_workspace_bytes(ctypes.byref(p), B, S)
    for B, S in [(1, 1), (32, 128), (32, 512), (7, 33), (2 ** 16, 512)]:
        for rows in (1, B * S // 2, B * S - 1, B * S):
            if rows >= 1:
                assert q(B, S, rows) == _formula(B, S, rows), (B, S, rows)
        assert q(B, S, B * S + 1) == q(B, S, B * S) == q(B, S, 2 ** 40)       # a bound above B S counts as B S
    for B, S in [(32, 128), (32, 512), (7, 33)]:
        assert 0 <= q(B, S, B * S) - padded(B, S) <= 2048, (B, S)             # the lengths, the offsets and the flag
        assert q(B, S, B * S // 2) < padded(B, S)
        sizes = [q(B, S, r) for r in (1, 2, 17, B * S // 2, B * S - 1, B * S, B * S + 5)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[3] < sizes[5]
    assert q(0, 128, 0) > 0 and q(0, 128, -3) > 0                              # B = 0 takes any bound
    for bad in [(1, 0, 1), (1, 513, 1), (-1, 128, 1), (2 ** 16 + 1, 128, 1), (4, 128, 0), (4, 128, -1)]:
        assert q(*bad) == 0, bad
    assert lib.gr_bert_embed_ragged_workspace_bytes(None, 1, 128, 1) == 0
    assert lib.gr_bert_embed_ragged_workspace_bytes(ctypes.byref(_params(hidden_size=776)), 1, 128, 128) == 0
    assert lib.gr_bert_embed_ragged_workspace_bytes(ctypes.byref(_params(max_position=100)), 1, 101, 101) == 0


def test_argument_order_and_prefix():
    import gr_amd
    lib = gr_amd.lib()

    def refused(rc, want, word):
        msg = lib.gr_last_error()
        assert rc == want and msg.startswith(PREFIX) and word in msg, (rc, msg)
    refused(lib.gr_bert_embed_ragged_f32(None, None, None, None, 1, 128, 128, 1, None, None, None, None, 0, None),
            GR_ERR_ARG, b"null params")
    refused(_call(lib, _params(), B=-1), GR_ERR_ARG, b"negative batch")
    refused(_call(lib, _params(hidden_size=776), B=-1), GR_ERR_ARG, b"negative batch")     # ARG before UNSUPPORTED
    refused(_call(lib, _params(hidden_size=776)), GR_ERR_UNSUPPORTED, b"hidden_size")
    refused(_call(lib, _params(), S=513), GR_ERR_UNSUPPORTED, b"S must be")
    refused(_call(lib, _params(hidden_size=776), rows=0), GR_ERR_UNSUPPORTED, b"hidden_size")  # the envelope first
    for rows in (0, -1):
        refused(_call(lib, _params(), rows=rows), GR_ERR_ARG, b"rows_bound")
        refused(_call(lib, _params(), rows=rows, pooling=7), GR_ERR_ARG, b"rows_bound")       # before the pooling
    for pooling in (-1, 3):
        refused(_call(lib, _params(), pooling=pooling), GR_ERR_ARG, b"pooling")
    refused(_call(lib, _params()), GR_ERR_WORKSPACE, b"gr_bert_embed_ragged_workspace_bytes")
    refused(_call(lib, _params(), ws=1 << 40), GR_ERR_WORKSPACE, b"workspace")               # a NULL workspace of any size
    assert _call(lib, _params(), B=0) == GR_OK and _call(lib, _params(), B=0, rows=0) == GR_OK
    assert _call(lib, _params(intermediate_size=100), B=0) == GR_ERR_UNSUPPORTED
    assert _call(lib, _params(), rows=2 ** 40) == GR_ERR_WORKSPACE                           # counts as B S


def test_pointer_checks():
    """With a (host) workspace of the right size the pointer checks are reached; they all come before any launch."""
    import gr_amd
    lib = gr_amd.lib()
    p = _params(hidden_size=64, num_heads=1, intermediate_size=32, num_layers=1, vocab_size=8, max_position=8)
    n = lib.gr_bert_embed_ragged_workspace_bytes(ctypes.byref(p), 1, 4, 3)
    assert n == _formula(1, 4, 3, H=64, I=32)
    buf = ctypes.create_string_buffer(n + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15
    ids = (ctypes.c_int64 * 4)()
    offs = (ctypes.c_int64 * 2)()
    out = ctypes.create_string_buffer(64 * 4 * 4 + 16)
    outp = (ctypes.addressof(out) + 15) & ~15
    f = lambda ids_, pooling, pooled, hidden, offsets, ws_=ws, n_=n: lib.gr_bert_embed_ragged_f32(
        ctypes.byref(p), ids_, None, None, 1, 4, 3, pooling, pooled, hidden, offsets, ws_, n_, None)

    def refused(rc, want, word):
        msg = lib.gr_last_error()
        assert rc == want and msg.startswith(PREFIX) and word in msg, (rc, msg)
    refused(f(ids, 1, outp, None, None, ws + 4), GR_ERR_WORKSPACE, b"workspace")              # misaligned
    refused(f(ids, 1, outp, None, None, ws, n - 1), GR_ERR_WORKSPACE, b"workspace")           # too small
    refused(f(ids, 1, outp, None, None, None), GR_ERR_WORKSPACE, b"workspace")                # missing
    refused(f(None, 1, outp, None, None), GR_ERR_ARG, b"input_ids")
    refused(f(ids, 1, None, None, None), GR_ERR_ARG, b"pooled_out")
    refused(f(ids, 2, None, outp, offs), GR_ERR_ARG, b"pooled_out")
    refused(f(ids, 0, None, None, None), GR_ERR_ARG, b"hidden_rows_out")
    refused(f(ids, 0, None, outp, None), GR_ERR_ARG, b"row_offsets_out")
    refused(f(ids, 0, None, None, offs), GR_ERR_ARG, b"hidden_rows_out")
    refused(f(ids, 0, None, outp + 4, offs), GR_ERR_ARG, b"hidden_rows_out")
    refused(f(ids, 1, outp, None, None), GR_ERR_ARG, b"weight pointer")                       # every weight is NULL
    w = ctypes.create_string_buffer(64)
    good = (ctypes.addressof(w) + 15) & ~15
    for name in ("word", "position", "token_type", "emb_ln_w", "emb_ln_b"):
        setattr(p, name, good)
    for i in range(16):
        p.layer[0][i] = good + (4 if i == 11 else 0)
    refused(f(ids, 1, outp, None, None), GR_ERR_ARG, b"weight pointer")                       # one misaligned weight


def _by_hand(mask):
    total = 0
    for row in mask.tolist():
        live = [i for i, v in enumerate(row) if v != 0]
        total += live[-1] + 1 if live else 0
    return total


def test_row_bound_on_host_masks():
    from gr_amd.bert_embed import row_bound
    assert row_bound(None) is None
    tiny = bc.case("tiny")
    assert row_bound(tiny.mask) == 33 + 1 + 2 + 17 + 32 + 5
    for name in bc.NAMES:
        assert row_bound(bc.case(name).mask) == _by_hand(bc.case(name).mask), name
    holes = bc.case("heads32").mask
    assert int(holes[1, 0]) == 0 and int(holes[2, -1]) == 1 and int((holes == 0).sum()) > 0
    lens = [_by_hand(holes[b:b + 1]) for b in range(holes.shape[0])]
    assert lens[0] == 65 and lens[2] == 65 and lens[1] >= 2         # all live; last column live; no position 0
    assert row_bound(holes) == sum(lens) and row_bound(holes) > int((holes != 0).sum())       # the holes stay in
    dead = tiny.mask.clone()
    dead[2] = 0
    assert row_bound(dead) == row_bound(tiny.mask) - 2
    assert row_bound(torch.zeros(3, 9, dtype=torch.int64)) == 0
    assert row_bound(torch.ones(3, 9, dtype=torch.int64)) == 27
    assert row_bound(5 * torch.ones(2, 4, dtype=torch.int32)) == 8              # anything but 0 is live
    assert row_bound(tiny.mask.bool()) == row_bound(tiny.mask)
    assert row_bound(torch.zeros(0, 9, dtype=torch.int64)) == 0


def test_training_and_cpu_are_refused():
    import gr_amd
    fx = bf.fixture("bert_embed_main")
    m = gr_amd.bert_embed.BertEncoder(fx.cfg)
    m.load_state_dict(fx.sd)
    m.train()
    with pytest.raises(NotImplementedError, match="training"):
        m.embed(fx.ids, fx.mask, ragged=True)
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.embed(fx.ids, fx.mask, fx.type_ids, ragged=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.embed(fx.ids, fx.mask, ragged=True, rows_bound=gr_amd.bert_embed.row_bound(fx.mask))
    with pytest.raises(RuntimeError, match="no CPU fallback"), torch.no_grad():
        m.train().embed(fx.ids, fx.mask, pooling="cls", ragged=True)
    with pytest.raises(ValueError, match="pooling"):
        m.eval().embed(fx.ids, fx.mask, pooling="mean", ragged=True)
    tok = lambda texts, **kw: dict(input_ids=fx.ids[:len(texts)], attention_mask=fx.mask[:len(texts)])
    for ragged in (True, False):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gr_amd.bert_embed.encode_texts(["a", "b"], tok, m, "cpu", 2, 12, ragged=ragged)
