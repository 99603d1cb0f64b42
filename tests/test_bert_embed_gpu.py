"""The BERT encoder on the GPU (csrc/bert_embed.hip) against the float64 restatement tests/bert_embed_ref.py.

Tolerances are 4 x the float32 restatement's own worst distance from float64 on the same inputs, relative to the
tensor's largest magnitude over live rows (the rule of test_tiger_gpu.py and test_t5_embed_gpu.py).  For the fixtures
the generator measured them and stored them in each fixture's meta (3.1e-07 .. 3.4e-07 for the hidden state, 1.8e-07 ..
2.9e-07 for the pooled vectors); for the seeded cases of tests/bert_cases.py they are measured here, on the CPU, once
per case.  Masked rows of the hidden state are not compared.  Against HF's own recorded float32 run the bound is that
plus HF's recorded distance from float64 (the triangle inequality).
"""
import numpy as np
import pytest
import torch

import bert_cases as bc
import bert_embed_fixtures as bf
import bert_embed_ref as ref

pytestmark = pytest.mark.gpu


def _binding(cfg, sd, dev):
    import gr_amd
    return gr_amd.ops.BertBinding(cfg, {k: v.to(dev) for k, v in sd.items()})


def _module(cfg, sd, dev):
    import gr_amd
    m = gr_amd.bert_embed.BertEncoder(cfg)
    m.load_state_dict(sd)                            # strict
    return m.to(dev).eval()


def _to(dev, *ts):
    return tuple(None if t is None else t.to(dev) for t in ts)


def _run(b, ids, mask, tt):
    """(hidden, mean_no_cls, cls) on the CPU: one call per pooling, the hidden state from the first."""
    import gr_amd
    mean, hidden = gr_amd.ops.bert_embed(b, ids, mask, tt, pooling="mean_no_cls", with_hidden=True)
    cls = gr_amd.ops.bert_embed(b, ids, mask, tt, pooling="cls")
    return dict(hidden=hidden.cpu(), mean_no_cls=mean.cpu(), cls=cls.cpu())


def _check(got, want64, err, mask, what, extra=None):
    extra = extra or {}
    for k, e in (("hidden", "hidden_err32"), ("mean_no_cls", "pooled_err32"), ("cls", "cls_err32")):
        d = ref.live_err(got[k], want64[k], mask if k == "hidden" else None)
        bound = 4 * err[e] + extra.get(k, 0.0)
        print(f"{what}: {k} err {d:.3e} (float32 restatement {err[e]:.3e}, bound {bound:.3e})")
        assert d <= bound, (what, k, d, bound)


@pytest.mark.parametrize("name", bc.NAMES)
def test_cases_against_float64(name, dev):
    c = bc.case(name)
    ids, mask, tt = _to(dev, c.ids, c.mask, c.type_ids)
    got = _run(_binding(c.cfg, c.sd, dev), ids, mask, tt)
    assert got["hidden"].shape == (c.B, c.S, c.cfg["hidden_size"]) and got["cls"].shape == got["mean_no_cls"].shape
    _check(got, bc.restated(name, torch.float64), bc.measured(name), c.mask, name)


def test_cls_is_row_zero_and_cls_only_mean_is_zero(dev):
    c = bc.case("tiny")
    ids, mask, tt = _to(dev, c.ids, c.mask, c.type_ids)
    got = _run(_binding(c.cfg, c.sd, dev), ids, mask, tt)
    assert torch.equal(got["cls"], got["hidden"][:, 0])
    assert got["mean_no_cls"][1].abs().max() == 0            # lengths[1] = 1: nothing live after position 0
    assert got["mean_no_cls"][2].abs().max() > 0


@pytest.mark.parametrize("name", bf.NAMES)
def test_fixtures_against_the_recorded_reference(name, dev):
    fx = bf.fixture(name)
    m = _module(fx.cfg, fx.sd, dev)
    ids, mask, tt = _to(dev, fx.ids, fx.mask, fx.type_ids)
    got = _run(m.binding(), ids, mask, tt)
    _check(got, fx.r64, fx.meta, fx.mask, name + " vs float64")
    hf_err = dict(hidden=fx.meta["hf_hidden_err"], mean_no_cls=fx.meta["hf_pooled_err"], cls=fx.meta["hf_cls_err"])
    _check(got, fx.hf, fx.meta, fx.mask, name + " vs HF float32", extra=hf_err)
    # the reference's lines on the module: outputs = model(**encoded); outputs.last_hidden_state
    encoded = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, special_tokens_mask=mask)
    out = m(**encoded)
    assert torch.equal(out.last_hidden_state.cpu(), got["hidden"]) and out[0] is out.last_hidden_state
    assert torch.equal(m.embed(ids, mask, tt).cpu(), got["mean_no_cls"])
    assert torch.equal(m.embed(ids, mask, tt, pooling="cls").cpu(), got["cls"])


@pytest.mark.parametrize("name", ["heads32", "base_width"])
def test_every_gemm_tile_gives_the_same_bits(name, dev):
    """Option "bert_tile": 128 x 128, 64 x 128 and 128 x 96 outputs per workgroup, each forced on every GEMM of the
    call (heads32: N 96, 160 and 288, none a multiple of a tile; base_width: four 256-deep chains per element and,
    at 390 rows, row tiles with a tail), against the float64 run and bitwise against the shape-chosen form."""
    from gr_amd import _lib as L
    c = bc.case(name)
    ids, mask, tt = _to(dev, c.ids, c.mask, c.type_ids)
    b = _binding(c.cfg, c.sd, dev)
    chosen = _run(b, ids, mask, tt)
    try:
        for tile in (1, 2, 3):
            L.set_option("bert_tile", tile)
            got = _run(b, ids, mask, tt)
            _check(got, bc.restated(name, torch.float64), bc.measured(name), c.mask, f"{name} tile {tile}")
            for k in got:
                assert torch.equal(got[k], chosen[k]), (tile, k)
    finally:
        L.set_option("bert_tile", 0)


def test_repeatable(dev):
    c = bc.case("heads32")
    ids, mask, tt = _to(dev, c.ids, c.mask, c.type_ids)
    b = _binding(c.cfg, c.sd, dev)
    one, two = _run(b, ids, mask, tt), _run(b, ids, mask, tt)
    for k in one:
        assert torch.equal(one[k], two[k]), k


@pytest.mark.parametrize("name", ["tiny", "heads32"])
def test_batch_independent(name, dev):
    """One sequence at several places of batches of 1, 3 and 17: the same bits (live rows and pooled vectors)."""
    c = bc.case(name)
    b = _binding(c.cfg, c.sd, dev)
    u = 3
    live = c.mask[u] != 0
    tt_all = c.type_ids if c.type_ids is not None else torch.zeros_like(c.ids)
    base = _run(b, *_to(dev, c.ids, c.mask, tt_all))
    for B, places in ((1, (0,)), (3, (0, 2)), (17, (0, 5, 16))):
        for at in places:
            rows = [(at + 1 + i) % c.B for i in range(B)]
            rows[at] = u
            got = _run(b, *_to(dev, c.ids[rows], c.mask[rows], tt_all[rows]))
            assert torch.equal(got["hidden"][at][live], base["hidden"][u][live]), (B, at)
            assert torch.equal(got["mean_no_cls"][at], base["mean_no_cls"][u]), (B, at)
            assert torch.equal(got["cls"][at], base["cls"][u]), (B, at)


def test_masked_positions_are_inert(dev):
    c = bc.case("heads32")
    dead = c.mask == 0
    assert int(dead.sum()) > 0
    other = c.ids.clone()
    other[dead] = torch.randint(1, c.cfg["vocab_size"], (int(dead.sum()),), generator=torch.Generator().manual_seed(5))
    assert not torch.equal(other, c.ids)
    b = _binding(c.cfg, c.sd, dev)
    one = _run(b, *_to(dev, c.ids, c.mask, c.type_ids))
    two = _run(b, *_to(dev, other, c.mask, c.type_ids))
    assert torch.equal(one["hidden"][~dead], two["hidden"][~dead])
    assert torch.equal(one["mean_no_cls"], two["mean_no_cls"])
    live0 = c.mask[:, 0] != 0                                  # a masked position 0 is a masked row like any other
    assert torch.equal(one["cls"][live0], two["cls"][live0])


def test_a_sequence_with_no_live_key(dev):
    c = bc.case("tiny")
    mask = c.mask.clone()
    mask[2] = 0
    b = _binding(c.cfg, c.sd, dev)
    base = _run(b, *_to(dev, c.ids, c.mask, None))
    got = _run(b, *_to(dev, c.ids, mask, None))
    for k in got:
        assert got[k][2].abs().max() == 0, k
    keep = [0, 1, 3, 4, 5]
    live = c.mask[keep] != 0
    assert torch.equal(got["hidden"][keep][live], base["hidden"][keep][live])
    assert torch.equal(got["mean_no_cls"][keep], base["mean_no_cls"][keep]) and torch.equal(got["cls"][keep], base["cls"][keep])
    want = ref.run(c.cfg, c.sd, c.ids, mask, None, torch.float64)
    _check(got, want, ref.measure(ref.run(c.cfg, c.sd, c.ids, mask, None, torch.float32), want, mask), mask, "no live key")


def test_token_types(dev):
    c = bc.case("tiny")
    assert c.type_ids is None
    b = _binding(c.cfg, c.sd, dev)
    ids, mask = _to(dev, c.ids, c.mask)
    none = _run(b, ids, mask, None)
    zeros = _run(b, ids, mask, torch.zeros_like(ids))
    for k in none:
        assert torch.equal(none[k], zeros[k]), k
    tt = (torch.arange(c.S)[None, :] >= torch.tensor([[20], [1], [1], [9], [16], [2]])).to(torch.int64)
    got = _run(b, ids, mask, tt.to(dev))
    assert not torch.equal(got["mean_no_cls"], none["mean_no_cls"])
    r64 = ref.run(c.cfg, c.sd, c.ids, c.mask, tt, torch.float64)
    r32 = ref.run(c.cfg, c.sd, c.ids, c.mask, tt, torch.float32)
    _check(got, r64, ref.measure(r32, r64, c.mask), c.mask, "token types")
    # far from the result without them: the type table was read
    assert ref.live_err(none["mean_no_cls"], r64["mean_no_cls"]) > 100 * bc.measured("tiny")["pooled_err32"]


def test_in_place_update_and_no_synchronisation(dev):
    c = bc.case("tiny")
    m = _module(c.cfg, c.sd, dev)
    ids, mask = _to(dev, c.ids, c.mask)
    first = m.embed(ids, mask)                      # fills the binding and the workspace size
    hidden = m(input_ids=ids, attention_mask=mask).last_hidden_state
    bind = m.binding()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")         # any device-to-host copy or synchronisation raises
    try:
        second = m.embed(ids, mask)
        cls = m.embed(ids, mask, pooling="cls")
        again = m(input_ids=ids, attention_mask=mask).last_hidden_state
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first, second) and torch.equal(hidden, again) and torch.equal(cls, hidden[:, 0])
    delta = 0.25 * torch.randn(c.cfg["hidden_size"], generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        m.encoder.layer[1].output.LayerNorm.bias += delta.to(dev)
    assert m.binding() is bind
    third = m.embed(ids, mask)
    assert not torch.equal(third, first)
    sd = dict(c.sd)
    sd["encoder.layer.1.output.LayerNorm.bias"] = c.sd["encoder.layer.1.output.LayerNorm.bias"] + delta
    r64 = ref.run(c.cfg, sd, c.ids, c.mask, None, torch.float64)
    r32 = ref.run(c.cfg, sd, c.ids, c.mask, None, torch.float32)
    d, e = ref.live_err(third.cpu(), r64["mean_no_cls"]), ref.live_err(r32["mean_no_cls"], r64["mean_no_cls"])
    print(f"after the update: pooled err {d:.3e} (float32 restatement {e:.3e})")
    assert d <= 4 * e


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
    fx = bf.fixture("bert_embed_main")
    m = _module(fx.cfg, fx.sd, dev)
    g = torch.Generator().manual_seed(8)
    lengths = [5, 12, 2, 9, 1, 30, 7]
    table = {f"text {i}": torch.randint(1, fx.cfg["vocab_size"], (n,), generator=g).tolist() for i, n in enumerate(lengths)}
    texts = list(table)
    tok = _stub_tokenizer(table)
    out = bert_embed.encode_texts(texts, tok, m, dev, batch_size=3, max_length=16)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (len(texts), fx.cfg["hidden_size"])
    for start in range(0, len(texts), 3):
        enc = tok(texts[start:start + 3], max_length=16).to(dev)
        want = m.embed(enc["input_ids"], enc["attention_mask"], enc["token_type_ids"])
        assert np.array_equal(out[start:start + 3], want.cpu().numpy())
        hidden = m(**enc).last_hidden_state            # the reference's own pooling lines on the module's output
        masked = hidden * enc["attention_mask"].unsqueeze(-1)
        lines = masked[:, 1:, :].sum(dim=1) / enc["attention_mask"][:, 1:].sum(dim=-1, keepdim=True).clamp(min=1e-9)
        # both add at most n = 15 float32 rows, in different orders: each side is within (n - 1) 2^-24 sum|x| of the
        # exact sum, and sum|x| / count <= max|hidden|
        assert (lines - want).abs().max().item() <= 2 * 14 * 2.0 ** -24 * hidden.abs().max().item()
    assert np.abs(out[4]).max() == 0                    # one token: nothing after position 0
    users = {u: t for u, t in zip((7, 3, 11), texts[:3])}
    embs = bert_embed.generate_user_profile_embedding(users, tok, m)
    assert list(embs) == [3, 7, 11]
    enc = tok([users[u] for u in (3, 7, 11)], max_length=64).to(dev)
    want = m(**enc).last_hidden_state[:, 0, :].cpu().numpy()
    for i, u in enumerate((3, 7, 11)):
        assert embs[u].dtype == np.float32 and np.array_equal(embs[u], want[i])
