"""The ragged BERT entry (gr_bert_embed_ragged_f32) on the GPU: bit for bit the padded call (gr_bert_embed_f32) on the
rows it keeps -- rows [0, len_b) of each sequence, len_b one past the last live position -- and on the pooled vectors,
and against the float64 restatement tests/bert_embed_ref.py under the rule of test_bert_embed_gpu.py: 4 x the float32
restatement's own measured distance from float64 on the same inputs.  No tolerance of its own.
"""
import functools

import numpy as np
import pytest
import torch

import bert_cases as bc
import bert_embed_fixtures as bf
import bert_embed_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _binding(key):
    """One binding per seeded case or (config name, seed) state, kept for the session."""
    import gr_amd
    cfg, sd = (bc.case(key).cfg, bc.case(key).sd) if isinstance(key, str) else _state(*key)
    return gr_amd.ops.BertBinding(cfg, {k: v.to(DEV) for k, v in sd.items()})


@functools.lru_cache(maxsize=None)
def _state(config, seed):
    cfg = dict(bc.BASE, **bc.CASES[config][0])
    return cfg, bc.state(cfg, seed)


def _to(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _lens(mask, B, S):
    """Host lengths: one past the last live position, 0 for a sequence with no live key."""
    if mask is None:
        return [S] * B
    return [max((i + 1 for i, v in enumerate(row) if v != 0), default=0) for row in mask.tolist()]


def _padded(b, ids, mask, tt):
    import gr_amd
    mean, hidden = gr_amd.ops.bert_embed(b, *_to(ids, mask, tt), pooling="mean_no_cls", with_hidden=True)
    cls = gr_amd.ops.bert_embed(b, *_to(ids, mask, tt), pooling="cls")
    return dict(hidden=hidden.cpu(), mean_no_cls=mean.cpu(), cls=cls.cpu())


def _ragged(b, ids, mask, tt, bound):
    import gr_amd
    mean, rows, off = gr_amd.ops.bert_embed_ragged(b, *_to(ids, mask, tt), pooling="mean_no_cls", rows_bound=bound,
                                                   with_hidden=True)
    cls = gr_amd.ops.bert_embed_ragged(b, *_to(ids, mask, tt), pooling="cls", rows_bound=bound)
    rows2, off2 = gr_amd.ops.bert_embed_ragged(b, *_to(ids, mask, tt), pooling=None, rows_bound=bound)
    assert torch.equal(off, off2)
    total = int(off[-1])
    assert torch.equal(rows[:total], rows2[:total])
    return dict(rows=rows.cpu(), off=off.cpu(), mean_no_cls=mean.cpu(), cls=cls.cpu())


def _same_bits(got, pad, lens, what):
    """The offsets are the host's prefix sum, the packed rows are the padded hidden state's [b, :len_b] (masked rows
    inside included) and both pooled vectors are the padded call's, bit for bit."""
    off = np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert got["off"].tolist() == off, what
    for b, n in enumerate(lens):
        assert torch.equal(got["rows"][off[b]:off[b + 1]], pad["hidden"][b, :n]), (what, "rows of sequence", b)
    assert torch.equal(got["mean_no_cls"], pad["mean_no_cls"]), (what, "mean_no_cls")
    assert torch.equal(got["cls"], pad["cls"]), (what, "cls")


def _against_float64(got, want64, err, what):
    for k, e in (("mean_no_cls", "pooled_err32"), ("cls", "cls_err32")):
        if want64[k].abs().max() == 0:                 # no scale for a relative distance: exact zeros are the check
            assert got[k].abs().max() == 0, (what, k)
            continue
        d = ref.live_err(got[k], want64[k])
        print(f"{what}: {k} err {d:.3e} (float32 restatement {err[e]:.3e}, bound {4 * err[e]:.3e})")
        assert d <= 4 * err[e], (what, k, d, 4 * err[e])


@functools.lru_cache(maxsize=None)
def _case_padded(name):
    c = bc.case(name)
    return _padded(_binding(name), c.ids, c.mask, c.type_ids)


# ---- 1, 2: the seeded cases

@pytest.mark.parametrize("name", bc.NAMES)
def test_cases_bitwise_against_the_padded_call(name, dev):
    c = bc.case(name)
    lens = _lens(c.mask, c.B, c.S)
    exact = sum(lens)
    assert exact < c.B * c.S
    pad = _case_padded(name)
    for bound in (exact, exact + 1, c.B * c.S):
        got = _ragged(_binding(name), c.ids, c.mask, c.type_ids, bound)
        assert got["rows"].shape == (bound, c.cfg["hidden_size"])
        _same_bits(got, pad, lens, (name, bound))


@pytest.mark.parametrize("name", bc.NAMES)
def test_cases_against_float64(name, dev):
    c = bc.case(name)
    got = _ragged(_binding(name), c.ids, c.mask, c.type_ids, sum(_lens(c.mask, c.B, c.S)))
    _against_float64(got, bc.restated(name, torch.float64), bc.measured(name), name)


# ---- 3: edges the cases do not reach

#  name: config of bert_cases.CASES, S, lengths (None: no mask at all), seed
EDGES = {
    "query_tile_edge": ("long", 129, [128, 129, 127], 311),     # 384 packed rows: three 128-row GEMM tiles, cut mid-sequence
    "one_gemm_tile":   ("long", 64, [64, 1, 63], 312),          # 128 packed rows exactly
    "one_row":         ("tiny", 1, [1], 313),
    "dead_sequences":  ("tiny", 33, [0, 33, 2, 0, 0, 17, 0], 314),   # first, two in the middle, last
    "all_dead":        ("tiny", 9, [0, 0, 0], 315),
    "no_mask":         ("tiny", 33, None, 316),
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_edges(edge, dev):
    config, S, lengths, seed = EDGES[edge]
    cfg, sd = _state(config, seed)
    B = 5 if lengths is None else len(lengths)
    ids, mask, _ = bc.inputs(cfg, B, S, [S] * B if lengths is None else lengths, False, seed)
    if lengths is None:
        mask = None
    lens = _lens(mask, B, S)
    assert lens == ([S] * B if lengths is None else lengths)
    b = _binding((config, seed))
    pad = _padded(b, ids, mask, None)
    exact = sum(lens)
    for bound in sorted({max(exact, 1), min(exact + 1, B * S), B * S}):
        _same_bits(_ragged(b, ids, mask, None, bound), pad, lens, (edge, bound))
    got = _ragged(b, ids, mask, None, max(exact, 1))
    if edge == "dead_sequences":
        off = got["off"].tolist()
        assert off[0] == off[1] == 0 and off[3] == off[4] == off[5] and off[6] == off[7] == exact      # offsets repeat
        live = [i for i, n in enumerate(lengths) if n]
        base = _padded(b, ids[live], mask[live], None)                   # the neighbours alone: the same bits
        for k in ("mean_no_cls", "cls"):
            assert got[k][[i for i, n in enumerate(lengths) if not n]].abs().max() == 0, k
            assert torch.equal(got[k][live], base[k]), k
    if exact == 0:
        # the float64 run is all zeros, so a relative distance has no scale: equality is the check
        assert int(got["off"][-1]) == 0 and got["mean_no_cls"].abs().max() == 0 and got["cls"].abs().max() == 0
        assert ref.run(cfg, sd, ids, mask, None, torch.float64)["mean_no_cls"].abs().max() == 0
        return
    r64 = ref.run(cfg, sd, ids, mask, None, torch.float64)
    r32 = ref.run(cfg, sd, ids, mask, None, torch.float32)
    _against_float64(got, r64, ref.measure(r32, r64, mask), edge)


# ---- 4: placement and repeatability

def test_placement_in_the_batch(dev):
    """One sequence of heads32 at several places of batches of 1, 3 and 17 among neighbours of other lengths: the
    padded base call's bits, as test_bert_embed_gpu.py::test_batch_independent has it for the padded entry."""
    c = bc.case("heads32")
    b = _binding("heads32")
    u = 3
    n_u = _lens(c.mask[u:u + 1], 1, c.S)[0]
    base = _case_padded("heads32")
    for B, places in ((1, (0,)), (3, (0, 2)), (17, (0, 5, 16))):
        for at in places:
            pick = [(at + 1 + i) % c.B for i in range(B)]
            pick[at] = u
            mask = c.mask[pick].clone()
            for i in range(B):                                           # neighbours of other lengths: cut some short
                if i != at and i % 2:
                    mask[i, 7 + 3 * (i % 5):] = 0
            lens = _lens(mask, B, c.S)
            got = _ragged(b, c.ids[pick], mask, c.type_ids[pick], sum(lens))
            off = got["off"].tolist()
            assert off == np.concatenate([[0], np.cumsum(lens)]).tolist()
            assert torch.equal(got["rows"][off[at]:off[at + 1]], base["hidden"][u, :n_u]), (B, at)
            assert torch.equal(got["mean_no_cls"][at], base["mean_no_cls"][u]), (B, at)
            assert torch.equal(got["cls"][at], base["cls"][u]), (B, at)


def test_repeatable(dev):
    c = bc.case("heads32")
    bound = sum(_lens(c.mask, c.B, c.S))
    one = _ragged(_binding("heads32"), c.ids, c.mask, c.type_ids, bound)
    two = _ragged(_binding("heads32"), c.ids, c.mask, c.type_ids, bound)
    total = int(one["off"][-1])
    assert torch.equal(one["rows"][:total], two["rows"][:total]) and torch.equal(one["off"], two["off"])
    assert torch.equal(one["mean_no_cls"], two["mean_no_cls"]) and torch.equal(one["cls"], two["cls"])


# ---- 5: a bound below the mask's row count

def test_a_wrong_bound_is_visible(dev):
    import gr_amd
    c = bc.case("tiny")
    b = _binding("tiny")
    ids, mask = _to(c.ids, c.mask)
    exact = sum(_lens(c.mask, c.B, c.S))
    pad = _case_padded("tiny")
    for pooling in ("mean_no_cls", "cls"):
        pooled, rows, off = gr_amd.ops.bert_embed_ragged(b, ids, mask, pooling=pooling, rows_bound=exact - 1,
                                                         with_hidden=True)
        assert rows.shape[0] == exact - 1
        assert bool(torch.isnan(pooled).all()), pooling
        assert off.tolist() == [0] * c.B + [-1]
        again = gr_amd.ops.bert_embed_ragged(b, ids, mask, pooling=pooling, rows_bound=exact)   # the same workspace
        assert torch.equal(again.cpu(), pad[pooling]), pooling


# ---- 6: no synchronisation

def _module(cfg, sd):
    import gr_amd
    m = gr_amd.bert_embed.BertEncoder(cfg)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def test_no_synchronisation(dev):
    from gr_amd import bert_embed
    c = bc.case("tiny")
    m = _module(c.cfg, c.sd)
    ids, mask = _to(c.ids, c.mask)
    exact = bert_embed.row_bound(c.mask)
    assert bert_embed.row_bound(mask) == c.B * c.S                     # a device mask is not read
    first = m.embed(ids, mask, ragged=True)                           # fills the binding and the workspace sizes
    m.embed(ids, mask, ragged=True, rows_bound=exact)
    m.embed(ids, mask, pooling="cls", ragged=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                           # any device-to-host copy or synchronisation raises
    try:
        second = m.embed(ids, mask, ragged=True)
        third = m.embed(ids, mask, ragged=True, rows_bound=exact)
        cls = m.embed(ids, mask, pooling="cls", ragged=True, rows_bound=bert_embed.row_bound(mask))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    pad = _case_padded("tiny")
    assert torch.equal(first, second) and torch.equal(second, third)
    assert torch.equal(second.cpu(), pad["mean_no_cls"]) and torch.equal(cls.cpu(), pad["cls"])


# ---- 7: the reference-shaped entries

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


class _Recorder:
    """Wraps ``ops.bert_embed`` and ``ops.bert_embed_ragged``: which entry each batch took, and with what bound."""

    def __init__(self, monkeypatch):
        import gr_amd
        self.calls = []
        padded, ragged = gr_amd.ops.bert_embed, gr_amd.ops.bert_embed_ragged

        def rec_padded(binding, input_ids, *a, **kw):
            self.calls.append(("padded", tuple(input_ids.shape), None))
            return padded(binding, input_ids, *a, **kw)

        def rec_ragged(binding, input_ids, *a, **kw):
            self.calls.append(("ragged", tuple(input_ids.shape), kw.get("rows_bound")))
            return ragged(binding, input_ids, *a, **kw)
        monkeypatch.setattr(gr_amd.ops, "bert_embed", rec_padded)
        monkeypatch.setattr(gr_amd.ops, "bert_embed_ragged", rec_ragged)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def test_reference_shaped_entries(dev, monkeypatch):
    from gr_amd import bert_embed
    fx = bf.fixture("bert_embed_main")
    m = _module(fx.cfg, fx.sd)
    g = torch.Generator().manual_seed(8)
    lengths = [5, 12, 2, 9, 1, 30, 7]
    table = {f"text {i}": torch.randint(1, fx.cfg["vocab_size"], (n,), generator=g).tolist() for i, n in enumerate(lengths)}
    texts = list(table)
    tok = _stub_tokenizer(table)
    want = []
    for start in range(0, len(texts), 3):                               # the padded call per batch, before recording
        enc = tok(texts[start:start + 3], max_length=16).to(DEV)
        want.append(m.embed(enc["input_ids"], enc["attention_mask"], enc["token_type_ids"]).cpu().numpy())
    rec = _Recorder(monkeypatch)
    out = bert_embed.encode_texts(texts, tok, m, dev, batch_size=3, max_length=16)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and np.array_equal(out, np.concatenate(want))
    # [5 12 2] and [9 1 16] have padding: the ragged entry with the exact row count; [7] alone has none
    assert rec.take() == [("ragged", (3, 12), 19), ("ragged", (3, 16), 26), ("padded", (1, 7), None)]
    assert np.abs(out[4]).max() == 0                                    # one token: nothing after position 0
    off = bert_embed.encode_texts(texts, tok, m, dev, batch_size=3, max_length=16, ragged=False)
    assert np.array_equal(off, out)
    assert rec.take() == [("padded", (3, 12), None), ("padded", (3, 16), None), ("padded", (1, 7), None)]
    # a tokenizer that answers on the device: the mask is not read, every batch stays on the padded entry
    on_device = lambda *a, **kw: tok(*a, **kw).to(DEV)
    assert np.array_equal(bert_embed.encode_texts(texts[:3], on_device, m, dev, batch_size=3, max_length=16), out[:3])
    assert rec.take() == [("padded", (3, 12), None)]

    users = {u: t for u, t in zip((7, 3, 11), texts[:3])}
    enc = tok([users[u] for u in (3, 7, 11)], max_length=64).to(DEV)
    want_cls = m.embed(enc["input_ids"], enc["attention_mask"], enc["token_type_ids"], pooling="cls").cpu().numpy()
    rec.take()
    embs = bert_embed.generate_user_profile_embedding(users, tok, m)
    assert rec.take() == [("ragged", (3, 12), 19)]
    assert list(embs) == [3, 7, 11]
    for i, u in enumerate((3, 7, 11)):
        assert embs[u].dtype == np.float32 and np.array_equal(embs[u], want_cls[i])
    same = bert_embed.generate_user_profile_embedding(users, tok, m, ragged=False)
    assert rec.take() == [("padded", (3, 12), None)]
    assert all(np.array_equal(same[u], embs[u]) for u in users)
    bert_embed.generate_user_profile_embedding({4: texts[6]}, tok, m)    # one user: no padding
    assert rec.take() == [("padded", (1, 7), None)]
