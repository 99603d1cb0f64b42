"""The T5 embedding retriever's packed entry on the GPU (gr_t5_embed_project_f32, gr_t5_embed_rows_f32): id sequences
on live rows only, against the dense call on the same sequences as zero-padded vectors with the right-padded mask.

The contract is equality of bits: the GEMM gives a row one summation order wherever it sits, a masked key weighs
exactly 0 in the dense attention, and a dead row is never pooled.  Case a is also held to the float64 restatement
at 4 x the float32 restatement's own distance (the rule of test_t5_embed_gpu.py), and the projection to
``table.double() @ W.double().T + b`` at 4 x the distance of torch's CPU float32 ``F.linear`` from it.

    case  weights and widths                                                     B  lengths
    a     fixture t5e_main                                                       7  32 1 21 2 5 17 9
    b     d_model 32, one head of 8, d_ff 32, in 4, out 4, one block             3  9 1 32
    c     d_model 512, 4 heads of 64, d_ff 1024, in 1024, out 1024, eight blocks 3  5 32 2
    d     d_model 64, 2 heads of 16, d_ff 64, in 16, out 16, one block           5  31 32 3 32 30  (128 rows: two
          64-row GEMM tiles, the third user's rows 63..65 across their boundary)
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import t5_embed_fixtures as tf
import t5_embed_ref as ref

pytestmark = pytest.mark.gpu

NARROW = dict(d_model=32, d_ff=32, num_heads=1, d_kv=8, num_layers=1, input_emb_dim=4, target_emb_dim=4,
              layer_norm_epsilon=1e-6)
WIDEST = dict(d_model=512, d_ff=1024, num_heads=4, d_kv=64, num_layers=8, input_emb_dim=1024, target_emb_dim=1024,
              layer_norm_epsilon=1e-6)
SMALL = dict(d_model=64, d_ff=64, num_heads=2, d_kv=16, num_layers=1, input_emb_dim=16, target_emb_dim=16,
             layer_norm_epsilon=1e-6)
LENGTHS = {"a": [32, 1, 21, 2, 5, 17, 9], "b": [9, 1, 32], "c": [5, 32, 2], "d": [31, 32, 3, 32, 30]}
TABLE_ROWS = 40


class Case:
    """Weights, a seeded table, seeded tokens; the dense side (zero-padded gather, right-padded mask) on the CPU."""

    def __init__(self, name):
        if name == "a":
            fx = tf.fixture("t5e_main")
            self.cfg, self.sd = fx.cfg, fx.sd
        else:
            self.cfg = {"b": NARROW, "c": WIDEST, "d": SMALL}[name]
            self.sd = tf.random_state(self.cfg, 400 + ord(name))
        rng = np.random.default_rng(500 + ord(name))
        self.lengths = LENGTHS[name]
        self.table = torch.from_numpy(0.5 * rng.standard_normal((TABLE_ROWS, self.cfg["input_emb_dim"])).astype(np.float32))
        self.tokens = torch.from_numpy(rng.integers(0, TABLE_ROWS, sum(self.lengths)))
        self.offsets = torch.tensor([0] + list(np.cumsum(self.lengths)), dtype=torch.long)
        self.seq, self.mask = dense_side(self.table, self.tokens, self.offsets)


def dense_side(table, tokens, offsets):
    B, S = len(offsets) - 1, int(offsets.diff().max())
    seq, mask = torch.zeros(B, S, table.shape[1]), torch.zeros(B, S, dtype=torch.long)
    for b in range(B):
        n = int(offsets[b + 1] - offsets[b])
        seq[b, :n] = table[tokens[offsets[b]:offsets[b + 1]]]
        mask[b, :n] = 1
    return seq, mask


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def on_device(name, dev):
    """The case's binding and one run of either entry, shared by the tests (computed once, left unchanged)."""
    import gr_amd
    c = case(name)
    binding = gr_amd.ops.T5EmbedBinding(c.cfg, {k: v.to(dev) for k, v in c.sd.items()})
    projected = gr_amd.ops.t5_embed_project(binding, c.table.to(dev))
    tokens, offsets = c.tokens.to(dev), c.offsets.to(dev)
    pred, hidden = gr_amd.ops.t5_embed_rows(binding, projected, tokens, offsets, with_hidden=True)
    dpred, dhidden = gr_amd.ops.t5_embed(binding, c.seq.to(dev), c.mask.to(dev), with_hidden=True)
    return dict(binding=binding, projected=projected, tokens=tokens, offsets=offsets, pred=pred, hidden=hidden,
                dense_pred=dpred, dense_hidden=dhidden)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_bits_of_the_dense_call(name, dev):
    c, r = case(name), on_device(name, dev)
    assert r["pred"].shape == (len(c.lengths), c.cfg["target_emb_dim"])
    assert r["hidden"].shape == (sum(c.lengths), c.cfg["d_model"])
    assert not torch.isnan(r["pred"]).any()
    assert same_bits(r["pred"], r["dense_pred"])
    assert same_bits(r["hidden"], r["dense_hidden"][c.mask.to(dev).bool()])          # live rows, user after user


def test_case_a_against_float64(dev):
    c, r = case("a"), on_device("a", dev)
    want = tf.restate(c.cfg, c.sd, c.seq, c.mask)
    pe = ref.live_err(r["pred"].cpu(), want["pred64"])
    he = ref.live_err(r["hidden"].cpu(), want["hidden64"][c.mask.bool()])
    print(f"case a: pred err {pe:.3e} (float32 restatement {want['pred_err32']:.3e}), hidden err {he:.3e} "
          f"(float32 restatement {want['hidden_err32']:.3e})")
    assert pe <= 4 * want["pred_err32"], (pe, want["pred_err32"])
    assert he <= 4 * want["hidden_err32"], (he, want["hidden_err32"])


@pytest.mark.parametrize("name", ["a", "c"])
def test_projection_against_float64(name, dev):
    c, r = case(name), on_device(name, dev)
    W, b = c.sd["input_proj.weight"], c.sd["input_proj.bias"]
    want = c.table.double() @ W.double().T + b.double()
    err32 = ref.live_err(F.linear(c.table, W, b), want)
    err = ref.live_err(r["projected"].cpu(), want)
    print(f"projection {name}: err {err:.3e} (CPU float32 F.linear {err32:.3e})")
    assert r["projected"].shape == want.shape and err <= 4 * err32, (err, err32)


@pytest.mark.parametrize("R", [1, 65, 130])
def test_projection_row_is_independent_of_its_place(R, dev):
    import gr_amd
    binding = on_device("a", dev)["binding"]
    g = torch.Generator().manual_seed(R)
    table = torch.randn(R, case("a").cfg["input_emb_dim"], generator=g).to(dev)
    perm = torch.randperm(R, generator=g).to(dev)
    whole = gr_amd.ops.t5_embed_project(binding, table)
    assert same_bits(gr_amd.ops.t5_embed_project(binding, table[perm]), whole[perm])
    assert same_bits(gr_amd.ops.t5_embed_project(binding, table), whole)


def _user(c, u):
    return c.tokens[c.offsets[u]:c.offsets[u + 1]]


def test_repeatable_and_independent_of_the_batch(dev):
    import gr_amd
    c, r = case("a"), on_device("a", dev)
    run = lambda tokens, offsets: gr_amd.ops.t5_embed_rows(r["binding"], r["projected"], tokens.to(dev), offsets.to(dev),
                                                           with_hidden=True)
    pred, hidden = run(c.tokens, c.offsets)
    assert same_bits(pred, r["pred"]) and same_bits(hidden, r["hidden"])
    alone, _ = run(_user(c, 2), torch.tensor([0, c.lengths[2]]))
    assert same_bits(alone, r["pred"][2:3])
    order = [5, 0, 6, 2, 1]                                        # user 2 at position 3 of a batch of 5
    tokens = torch.cat([_user(c, u) for u in order])
    offsets = torch.tensor([0] + list(np.cumsum([c.lengths[u] for u in order])))
    moved, moved_hidden = run(tokens, offsets)
    assert same_bits(moved, r["pred"][order])
    assert same_bits(moved_hidden[offsets[3]:offsets[4]], r["hidden"][c.offsets[2]:c.offsets[3]])


def test_tokens_outside_the_table_poison_their_user_only(dev):
    import gr_amd
    c, r = case("a"), on_device("a", dev)
    tokens = c.tokens.clone()
    tokens[c.offsets[3] + 1] = TABLE_ROWS                          # R: one past the table
    tokens[c.offsets[5] + 4] = -1
    pred = gr_amd.ops.t5_embed_rows(r["binding"], r["projected"], tokens.to(dev), r["offsets"])     # raises unless GR_OK
    assert torch.isnan(pred[3]).all() and torch.isnan(pred[5]).all()
    keep = [0, 1, 2, 4, 6]
    assert same_bits(pred[keep], r["pred"][keep])


def test_offsets_that_describe_no_sequence_poison_their_user_only(dev):
    """A length of 0 and one of 40: both users NaN, nothing outside the buffers, the third user's bits its own."""
    import gr_amd
    c, r = case("d"), on_device("d", dev)
    tokens = c.tokens[:45].to(dev)
    pred = gr_amd.ops.t5_embed_rows(r["binding"], r["projected"], tokens, torch.tensor([0, 0, 40, 45]).to(dev))
    assert torch.isnan(pred[0]).all() and torch.isnan(pred[1]).all()
    alone = gr_amd.ops.t5_embed_rows(r["binding"], r["projected"], tokens[40:], torch.tensor([0, 5]).to(dev))
    assert not torch.isnan(alone).any() and same_bits(pred[2:], alone)


# the module's six blocks at one width for the sequences and the catalog, as in the reference (768 -> 768)
MODULE = dict(SMALL, num_layers=6, dropout_rate=0.1, temperature=0.07)


def _module(dev):
    import gr_amd
    m = gr_amd.t5_embed.TIGER(MODULE)
    missing, unexpected = m.load_state_dict(tf.random_state(MODULE, 460), strict=False)
    assert set(missing) <= {"model.shared.weight", "model.encoder.embed_tokens.weight"} and not unexpected
    return m.to(dev).eval()


@functools.lru_cache(maxsize=None)
def _catalog():
    """50 items, 9 users, two batches of 6 samples, as ids and as the reference's vector samples."""
    rng = np.random.default_rng(11)
    dim = MODULE["input_emb_dim"]
    items = rng.standard_normal((50, dim)).astype(np.float32)
    users = rng.standard_normal((9, dim)).astype(np.float32)
    lengths = [[3, 21, 2, 9, 32, 5], [2, 2, 17, 30, 4, 8]]
    ids = [[dict(history=rng.integers(0, 50, n - 1).tolist(), user_id=int(rng.integers(1, 10)),
                 target_id=int(rng.integers(0, 50))) for n in ls] for ls in lengths]
    vectors = [[dict(seq_embs=np.concatenate([users[s["user_id"] - 1][None], items[s["history"]]], axis=0),
                     seq_len=len(s["history"]) + 1, target_emb=items[s["target_id"]], target_id=s["target_id"],
                     user_id=s["user_id"]) for s in batch] for batch in ids]
    return items, users, ids, vectors


def test_evaluate_ids_and_eval_loss_ids(dev):
    from gr_amd import t5_embed
    items, users, ids, vectors = _catalog()
    m = _module(dev)
    tables = t5_embed.Tables(m, items, users)
    assert tables.table.shape[0] == 59 and tables.user_row(1) == 50 and tables.projected().shape[0] == 59
    id_batches = [t5_embed.collate_ids(b, tables.n_items) for b in ids]
    vec_batches = [t5_embed.collate(b) for b in vectors]
    topk = [5, 10, 20]
    assert t5_embed.evaluate_ids(id_batches, m, tables, topk) == t5_embed.evaluate_batches(vec_batches, m, items, topk)
    losses = [m(b["seq_embs"].to(dev), b["attention_mask"].to(dev), target_emb=b["target_emb"].to(dev))[0].item()
              for b in vec_batches]
    got = t5_embed.eval_loss_ids(id_batches, m, tables)
    assert isinstance(got, float) and got == sum(losses) / len(losses), (got, losses)
    for ib, vb in zip(id_batches, vec_batches):
        pred = m.embed_rows(tables, ib["tokens"].to(dev), ib["offsets"].to(dev))
        assert same_bits(pred, m.generate(vb["seq_embs"].to(dev), vb["attention_mask"].to(dev)))


def test_no_host_round_trip(dev):
    from gr_amd import t5_embed
    items, users, ids, _ = _catalog()
    m = _module(dev)
    tables = t5_embed.Tables(m, items, users)
    batch = t5_embed.collate_ids(ids[0], tables.n_items)
    tokens, offsets = batch["tokens"].to(dev), batch["offsets"].to(dev)
    first = m.embed_rows(tables, tokens, offsets)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")       # any device-to-host copy or synchronisation raises
    try:
        second = m.embed_rows(tables, tokens, offsets)
        table = tables.projected()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert same_bits(first, second) and table is tables.projected()


def test_projection_is_a_snapshot_of_input_proj(dev):
    from gr_amd import t5_embed
    items, users, ids, vectors = _catalog()
    m = _module(dev)
    tables = t5_embed.Tables(m, items, users)
    ib, vb = t5_embed.collate_ids(ids[1], tables.n_items), t5_embed.collate(vectors[1])
    tokens, offsets = ib["tokens"].to(dev), ib["offsets"].to(dev)
    seq, mask = vb["seq_embs"].to(dev), vb["attention_mask"].to(dev)
    before = m.embed_rows(tables, tokens, offsets)
    old = tables.projected()
    with torch.no_grad():
        m.input_proj.weight.mul_(1.5)
    after = m.embed_rows(tables, tokens, offsets)
    assert tables.projected() is not old
    assert same_bits(after, m.generate(seq, mask)) and not torch.equal(after, before)
    with torch.no_grad():
        m.input_proj.bias.add_(0.25)
    assert same_bits(m.embed_rows(tables, tokens, offsets), m.generate(seq, mask))
