"""The BERT encoder's bf16 precision on the GPU (gr_bert_embed_bf16 / gr_bert_embed_ragged_bf16, csrc/bert_embed.hip)
against the float64 restatement tests/bert_embed_ref.py.

The rule is the project's 4 x rule (test_bert_embed_gpu.py) with the bf16 restatement tests/bert_bf16_ref.py in the
float32 one's place: each of hidden (live rows), mean_no_cls and cls within 4 x that restatement's own distance from
float64 on the same inputs (``measured_bf16``: 2.1e-3 .. 8.2e-3 for the hidden state), relative to the tensor's largest
magnitude over live rows.  The hidden error must also lie ABOVE 4 x the float32 restatement's, so a ``precision`` that is
silently ignored fails.  What that tolerance can and cannot tell is shown on the CPU in test_bert_bf16_ref.py.  Bitwise
properties -- repeatability, batch invariance, ragged against padded, every GEMM tile -- are the fp32 call's.
"""
import functools

import numpy as np
import pytest
import torch

import bert_bf16_ref as bref
import bert_cases as bc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _binding(name):
    import gr_amd
    c = bref.case(name)
    return gr_amd.ops.BertBf16Binding(c.cfg, {k: v.to(DEV) for k, v in c.sd.items()})


def _to(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _run(b, ids, mask, tt):
    """(hidden, mean_no_cls, cls) on the CPU: one call per pooling, the hidden state from the first."""
    import gr_amd
    mean, hidden = gr_amd.ops.bert_embed(b, *_to(ids, mask, tt), pooling="mean_no_cls", with_hidden=True)
    cls = gr_amd.ops.bert_embed(b, *_to(ids, mask, tt), pooling="cls")
    assert hidden.dtype == mean.dtype == cls.dtype == torch.float32
    return dict(hidden=hidden.cpu(), mean_no_cls=mean.cpu(), cls=cls.cpu())


@functools.lru_cache(maxsize=None)
def _case_run(name):
    c = bref.case(name)
    return _run(_binding(name), c.ids, c.mask, c.type_ids)


def _lens(mask):
    return [max((i + 1 for i, v in enumerate(row) if v != 0), default=0) for row in mask.tolist()]


def _module(cfg, sd):
    import gr_amd
    m = gr_amd.bert_embed.BertEncoder(cfg)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.mark.parametrize("name", bref.NAMES)
def test_cases_against_float64(name, dev):
    c = bref.case(name)
    got = _case_run(name)
    assert got["hidden"].shape == (c.B, c.S, c.cfg["hidden_size"])
    d, bound, f32 = bref.distance(got, name), bref.measured_bf16(name), bref.measured(name)
    for k in ("hidden", "mean_no_cls", "cls"):
        print(f"{name}: {k} err {d[k]:.3e} (bf16 restatement {bound[k]:.3e}, bound {4 * bound[k]:.3e})")
    print(f"{name}: float32 restatement hidden {f32['hidden_err32']:.3e}")
    for k in ("hidden", "mean_no_cls", "cls"):
        assert d[k] <= 4 * bound[k], (name, k, d[k], 4 * bound[k])
    assert d["hidden"] > 4 * f32["hidden_err32"], (name, d["hidden"], f32["hidden_err32"])     # bf16 did run


def test_repeatable(dev):
    c = bc.case("heads32")
    one, two = _case_run("heads32"), _run(_binding("heads32"), c.ids, c.mask, c.type_ids)
    for k in one:
        assert torch.equal(one[k], two[k]), k


@pytest.mark.parametrize("name", ["tiny", "heads32"])
def test_batch_independent(name, dev):
    """One sequence at several places of batches of 1, 3 and 17: the same bits (live rows and its own pooled row)."""
    c = bc.case(name)
    b = _binding(name)
    u = 3
    live = c.mask[u] != 0
    tt_all = c.type_ids if c.type_ids is not None else torch.zeros_like(c.ids)
    base = _run(b, c.ids, c.mask, tt_all)
    for B, places in ((1, (0,)), (3, (0, 2)), (17, (0, 5, 16))):
        for at in places:
            rows = [(at + 1 + i) % c.B for i in range(B)]
            rows[at] = u
            got = _run(b, c.ids[rows], c.mask[rows], tt_all[rows])
            assert torch.equal(got["hidden"][at] * live[:, None], base["hidden"][u] * live[:, None]), (B, at)
            assert torch.equal(got["mean_no_cls"][at], base["mean_no_cls"][u]), (B, at)
            assert torch.equal(got["cls"][at], base["cls"][u]), (B, at)


@pytest.mark.parametrize("name", ["tiny", "heads32", "base_width", "long"])
def test_ragged_against_padded(name, dev):
    """The pooled vectors and every kept row (rows [0, len_b), holes included) are the padded bf16 call's bits, with
    the exact bound and with B * S; a bound one below the mask's count shows as NaN and -1."""
    import gr_amd
    c = bc.case(name)
    b = _binding(name)
    pad = _case_run(name)
    lens = _lens(c.mask)
    exact = sum(lens)
    assert exact < c.B * c.S
    want_off = np.concatenate([[0], np.cumsum(lens)]).tolist()
    args = _to(c.ids, c.mask, c.type_ids)
    for bound in (exact, c.B * c.S):
        mean, rows, off = gr_amd.ops.bert_embed_ragged(b, *args, pooling="mean_no_cls", rows_bound=bound, with_hidden=True)
        cls = gr_amd.ops.bert_embed_ragged(b, *args, pooling="cls", rows_bound=bound)
        assert rows.shape == (bound, c.cfg["hidden_size"]) and off.tolist() == want_off, (name, bound)
        rows = rows.cpu()
        for i, n in enumerate(lens):
            assert torch.equal(rows[want_off[i]:want_off[i + 1]], pad["hidden"][i, :n]), (name, bound, i)
        assert torch.equal(mean.cpu(), pad["mean_no_cls"]) and torch.equal(cls.cpu(), pad["cls"]), (name, bound)
    pooled, rows, off = gr_amd.ops.bert_embed_ragged(b, *args, pooling="cls", rows_bound=exact - 1, with_hidden=True)
    assert bool(torch.isnan(pooled).all()) and off.tolist() == [0] * c.B + [-1]


@pytest.mark.parametrize("name", ["heads32", "base_width"])
def test_every_gemm_tile_gives_the_same_bits(name, dev):
    """Option "bert_tile" forces 128 x 128, 64 x 128 or 128 x 96 outputs per workgroup on every bf16 GEMM of the call,
    as it does for the fp32 kernel: bitwise the shape-chosen form."""
    from gr_amd import _lib as L
    c = bc.case(name)
    chosen = _case_run(name)
    try:
        for tile in (1, 2, 3):
            L.set_option("bert_tile", tile)
            got = _run(_binding(name), c.ids, c.mask, c.type_ids)
            for k in got:
                assert torch.equal(got[k], chosen[k]), (tile, k)
    finally:
        L.set_option("bert_tile", 0)


def test_cls_is_row_zero_and_cls_only_mean_is_zero(dev):
    got = _case_run("tiny")
    assert torch.equal(got["cls"], got["hidden"][:, 0])
    assert got["mean_no_cls"][1].abs().max() == 0            # lengths[1] = 1: nothing live after position 0
    assert got["mean_no_cls"][2].abs().max() > 0


def test_fp32_is_unchanged(dev):
    import gr_amd
    c = bc.case("heads32")
    m = _module(c.cfg, c.sd)
    ids, mask, tt = _to(c.ids, c.mask, c.type_ids)
    want = gr_amd.ops.bert_embed(gr_amd.ops.BertBinding(c.cfg, {k: v.to(DEV) for k, v in c.sd.items()}), ids, mask, tt)
    m.embed(ids, mask, tt, precision="bf16")                 # a bf16 call in between changes nothing
    assert torch.equal(m.embed(ids, mask, tt), want) and torch.equal(m.embed(ids, mask, tt, precision="fp32"), want)
    assert torch.equal(m(input_ids=ids, attention_mask=mask, token_type_ids=tt).last_hidden_state[:, 0],
                       m.embed(ids, mask, tt, pooling="cls"))


def test_module_path_and_rebuilt_binding(dev):
    c = bc.case("tiny")
    m = _module(c.cfg, c.sd)
    ids, mask = _to(c.ids, c.mask)
    want = _case_run("tiny")
    first = m.embed(ids, mask, precision="bf16")
    assert torch.equal(first.cpu(), want["mean_no_cls"])
    assert torch.equal(m.embed(ids, mask, pooling="cls", precision="bf16").cpu(), want["cls"])
    assert torch.equal(m.embed(ids, mask, precision="bf16", ragged=True).cpu(), want["mean_no_cls"])
    bind = m.binding_bf16()
    assert m.binding_bf16() is bind                                              # nothing changed: kept
    with torch.no_grad():
        m.encoder.layer[0].intermediate.dense.weight.mul_(1.5)                  # in place: same storage, new version
    assert m.binding_bf16() is not bind
    second = m.embed(ids, mask, precision="bf16")
    assert not torch.equal(second, first)
    sd = dict(c.sd)
    sd["encoder.layer.0.intermediate.dense.weight"] = c.sd["encoder.layer.0.intermediate.dense.weight"] * 1.5
    import gr_amd
    fresh = gr_amd.ops.BertBf16Binding(c.cfg, {k: v.to(DEV) for k, v in sd.items()})
    assert torch.equal(second, gr_amd.ops.bert_embed(fresh, ids, mask))
    m.load_state_dict(c.sd)                                                      # copies in place: rebuilt again
    assert torch.equal(m.embed(ids, mask, precision="bf16"), first)


class _Encoded(dict):
    """What an HF tokenizer returns, as far as the reference uses it: a mapping with ``.to(device)``."""

    def to(self, device):
        return _Encoded({k: v.to(device) for k, v in self.items()})


def _stub_tokenizer(table):
    """texts -> ids from ``table``, truncated, padded with 0 to the batch's longest, as HF does with padding=True."""
    def tok(texts, padding=True, truncation=True, max_length=None, return_tensors="pt"):
        assert padding is True and truncation is True and return_tensors == "pt"
        rows = [table[t][:max_length] for t in texts]
        S = max(len(r) for r in rows)
        ids = torch.zeros(len(rows), S, dtype=torch.int64)
        mask = torch.zeros(len(rows), S, dtype=torch.int64)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r)
            mask[i, :len(r)] = 1
        return _Encoded(input_ids=ids, attention_mask=mask, token_type_ids=torch.zeros_like(ids))
    return tok


def test_reference_shaped_entries(dev):
    from gr_amd import bert_embed
    c = bc.case("tiny")
    m = _module(c.cfg, c.sd)
    g = torch.Generator().manual_seed(8)
    lengths = [5, 12, 2, 9, 1, 30, 7]
    table = {f"text {i}": torch.randint(1, c.cfg["vocab_size"], (n,), generator=g).tolist() for i, n in enumerate(lengths)}
    texts = list(table)
    tok = _stub_tokenizer(table)
    out = bert_embed.encode_texts(texts, tok, m, dev, batch_size=3, max_length=16, precision="bf16")
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (len(texts), c.cfg["hidden_size"])
    for start in range(0, len(texts), 3):
        enc = tok(texts[start:start + 3], max_length=16).to(DEV)
        want = m.embed(enc["input_ids"], enc["attention_mask"], enc["token_type_ids"], precision="bf16")
        assert np.array_equal(out[start:start + 3], want.cpu().numpy())
    assert not np.array_equal(out, bert_embed.encode_texts(texts, tok, m, dev, batch_size=3, max_length=16))
    users = {u: t for u, t in zip((7, 3, 11), texts[:3])}
    embs = bert_embed.generate_user_profile_embedding(users, tok, m, precision="bf16")
    enc = tok([users[u] for u in (3, 7, 11)], max_length=64).to(DEV)
    want = m.embed(enc["input_ids"], enc["attention_mask"], enc["token_type_ids"], pooling="cls", precision="bf16").cpu().numpy()
    assert list(embs) == [3, 7, 11]
    for i, u in enumerate((3, 7, 11)):
        assert embs[u].dtype == np.float32 and np.array_equal(embs[u], want[i])
