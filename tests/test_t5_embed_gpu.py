"""The T5 embedding retriever on the GPU (csrc/t5_embed.hip) against the float64 restatement
tests/t5_embed_ref.py.

Tolerances are 4 x the float32 reference's own worst distance from float64 on the same inputs, relative to
the tensor's largest magnitude over live rows (the rule of test_tiger_gpu.py).  For the fixtures the
generator measured them on the reference and stored them in each fixture's meta:

    fixture       pred_err32   hidden_err32
    t5e_main      4.31e-07     5.29e-07
    t5e_h3        3.05e-07     3.29e-07
    t5e_peaked    6.05e-06     2.78e-05

For the shapes no fixture can hold (the deployed width, the envelope's edges) the float32 restatement stands
for the reference: its distance from float64 is computed in the test, on the CPU, on the same inputs.
"""
import functools

import pytest
import torch

import t5_embed_fixtures as tf
import t5_embed_ref as ref

pytestmark = pytest.mark.gpu

DEPLOYED = dict(d_model=512, d_ff=256, num_heads=4, d_kv=16, num_layers=6, input_emb_dim=768, target_emb_dim=768,
                layer_norm_epsilon=1e-6, temperature=0.07)
DEPLOYED_LENGTHS = [21, 1, 2, 5, 20, 13, 21, 8]
SMALL = dict(d_model=64, d_ff=64, num_heads=2, d_kv=16, num_layers=1, input_emb_dim=16, target_emb_dim=16,
             layer_norm_epsilon=1e-6)
RETRIEVAL_SEED = 7


def _binding(cfg, sd, dev):
    import gr_amd
    return gr_amd.ops.T5EmbedBinding(cfg, {k: v.to(dev) for k, v in sd.items()})


def _module(params, sd, dev):
    """gr_amd.t5_embed.TIGER with ``sd`` loaded; only the unused token table may be missing from it."""
    import gr_amd
    m = gr_amd.t5_embed.TIGER(params)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert set(missing) <= {"model.shared.weight", "model.encoder.embed_tokens.weight"} and not unexpected
    return m.to(dev).eval()


def _params(cfg):
    return dict(cfg, dropout_rate=0.1)


def _check(pred, hidden, want, mask, what=""):
    """pred / hidden (CPU) against the float64 restatement at 4 x the float32 distance; prints the figures."""
    pe = ref.live_err(pred, want["pred64"])
    print(f"{what}: pred err {pe:.3e} (float32 restatement {want['pred_err32']:.3e})", end="")
    if hidden is not None:
        he = ref.live_err(hidden, want["hidden64"], mask)
        print(f", hidden err {he:.3e} (float32 restatement {want['hidden_err32']:.3e})")
        assert he <= 4 * want["hidden_err32"], (what, he, want["hidden_err32"])
    else:
        print()
    assert pe <= 4 * want["pred_err32"], (what, pe, want["pred_err32"])


@pytest.mark.parametrize("name", tf.NAMES)
def test_fixtures_against_float64(name, dev):
    import gr_amd
    fx = tf.fixture(name)
    want = dict(pred64=fx.pred64, hidden64=fx.hidden64, pred_err32=fx.meta["pred_err32"],
                hidden_err32=fx.meta["hidden_err32"])
    pred, hidden = gr_amd.ops.t5_embed(_binding(fx.cfg, fx.sd, dev), fx.seq.to(dev), fx.mask.to(dev), with_hidden=True)
    assert pred.shape == fx.pred64.shape and hidden.shape == fx.hidden64.shape
    _check(pred.cpu(), hidden.cpu(), want, fx.mask, name)
    m = gr_amd.t5_embed.TIGER(fx.params)
    m.load_state_dict(fx.state_dict())                  # strict
    m = m.to(dev).eval()
    loss, out = m(fx.seq.to(dev), fx.mask.to(dev))
    assert loss is None and torch.equal(out, pred)
    assert torch.equal(m.generate(fx.seq.to(dev), fx.mask.to(dev), num_beams=3), pred)


@functools.lru_cache(maxsize=None)
def _deployed():
    sd = tf.random_state(DEPLOYED, 101)
    seq, mask = tf.sequences(8, 21, 768, 102, DEPLOYED_LENGTHS)
    return sd, seq, mask, tf.restate(DEPLOYED, sd, seq, mask)


def test_deployed_width_against_float64(dev):
    """d_model 512, d_ff 256, 4 x 16, six blocks, 768 -> 768; B 8, S 21."""
    import gr_amd
    sd, seq, mask, want = _deployed()
    pred, hidden = gr_amd.ops.t5_embed(_binding(DEPLOYED, sd, dev), seq.to(dev), mask.to(dev), with_hidden=True)
    _check(pred.cpu(), hidden.cpu(), want, mask, "deployed width")


def _edge_inputs(B, S, dim, seed, kind):
    seq, mask = tf.sequences(B, S, dim, seed)
    if kind == "none":
        seq, _ = tf.sequences(B, S, dim, seed, [S] * B)
        return seq, None
    if kind == "holes":
        seq, mask = tf.sequences(B, S, dim, seed, [S] * B)
        mask[0, 1::2] = 0
        mask[B - 1, 0] = 0
        mask[B - 1, S - 1] = 0
    return seq, mask


EDGES = [
    # id, config changes, B, S, mask kind
    ("S1", {}, 3, 1, "pad"), ("S2", {}, 3, 2, "pad"), ("S31", {}, 3, 31, "pad"), ("S32", {}, 3, 32, "pad"),
    ("B1", {}, 1, 7, "pad"), ("B3", {}, 3, 7, "pad"), ("B17", {}, 17, 7, "pad"),
    ("d32_h1x8", dict(d_model=32, num_heads=1, d_kv=8), 4, 9, "pad"),
    ("inner256_4x64", dict(num_heads=4, d_kv=64), 4, 32, "pad"),
    ("inner256_8x32", dict(num_heads=8, d_kv=32), 4, 9, "pad"),
    ("ff32", dict(d_ff=32), 4, 9, "pad"), ("ff1024", dict(d_ff=1024), 4, 9, "pad"),
    ("in4_out4", dict(input_emb_dim=4, target_emb_dim=4), 4, 9, "pad"),
    ("layers8", dict(num_layers=8), 4, 9, "pad"),
    ("mask_none", {}, 4, 9, "none"), ("mask_holes", {}, 4, 9, "holes"),
]


@pytest.mark.parametrize("case", EDGES, ids=[e[0] for e in EDGES])
def test_edges_against_float64(case, dev):
    import gr_amd
    name, delta, B, S, kind = case
    cfg = dict(SMALL, **delta)
    sd = tf.random_state(cfg, 200 + len(name))
    seq, mask = _edge_inputs(B, S, cfg["input_emb_dim"], 300 + len(name), kind)
    want = tf.restate(cfg, sd, seq, mask)
    pred, hidden = gr_amd.ops.t5_embed(_binding(cfg, sd, dev), seq.to(dev), None if mask is None else mask.to(dev),
                                       with_hidden=True)
    _check(pred.cpu(), hidden.cpu(), want, mask, name)


def test_a_user_with_no_live_position(dev):
    """pooled = 0, so pred = normalize(out_b); the neighbours' bits are those of a batch without that user."""
    import gr_amd
    sd = tf.random_state(SMALL, 210)
    seq, mask = tf.sequences(5, 9, 16, 310, [9, 4, 6, 1, 7])
    mask[2] = 0
    want = tf.restate(SMALL, sd, seq, mask)
    b = _binding(SMALL, sd, dev)
    pred = gr_amd.ops.t5_embed(b, seq.to(dev), mask.to(dev)).cpu()
    _check(pred, None, want, mask, "empty user")
    bias = sd["output_proj.bias"].double()
    # sixteen squares summed, a square root and a division in float32: a few roundings of 2^-24 each
    assert (pred[2].double() - bias / bias.norm()).abs().max().item() <= 4 * 2.0 ** -23
    keep = [0, 1, 3, 4]
    assert torch.equal(gr_amd.ops.t5_embed(b, seq[keep].to(dev), mask[keep].to(dev)).cpu(), pred[keep])


def test_padding_is_inert(dev):
    """Zeros or random finite values (x 5) in the masked positions: the same bits."""
    import gr_amd
    fx = tf.fixture("t5e_peaked")
    dead = ~fx.mask.bool()
    assert int(dead.sum()) > 0 and int(fx.mask[2, 1]) == 0 and int(fx.mask[5, 0]) == 0       # padding and holes
    zero, noisy = fx.seq.clone(), fx.seq.clone()
    zero[dead] = 0.0
    noisy[dead] = 5.0 * torch.randn(int(dead.sum()), fx.seq.shape[-1], generator=torch.Generator().manual_seed(5))
    b = _binding(fx.cfg, fx.sd, dev)
    a = gr_amd.ops.t5_embed(b, zero.to(dev), fx.mask.to(dev))
    c = gr_amd.ops.t5_embed(b, noisy.to(dev), fx.mask.to(dev))
    assert torch.equal(a, c)
    assert ref.live_err(a.cpu(), fx.pred64) <= 4 * fx.meta["pred_err32"]


@pytest.mark.parametrize("which", ["t5e_main", "deployed"])
def test_repeatable_and_batch_invariant(which, dev):
    import gr_amd
    if which == "deployed":
        sd, seq, mask, _ = _deployed()
        cfg = DEPLOYED
    else:
        fx = tf.fixture(which)
        cfg, sd, seq, mask = fx.cfg, fx.sd, fx.seq, fx.mask
    b = _binding(cfg, sd, dev)
    seq, mask = seq.to(dev), mask.to(dev)
    full, hid = gr_amd.ops.t5_embed(b, seq, mask, with_hidden=True)
    again, hid2 = gr_amd.ops.t5_embed(b, seq, mask, with_hidden=True)
    assert torch.equal(full, again) and torch.equal(hid, hid2)
    assert torch.equal(gr_amd.ops.t5_embed(b, seq[3:7], mask[3:7]), full[3:7])
    for u in (0, 1, seq.shape[0] - 1):
        assert torch.equal(gr_amd.ops.t5_embed(b, seq[u:u + 1], mask[u:u + 1]), full[u:u + 1])
    swapped = torch.arange(seq.shape[0] - 1, -1, -1, device=dev)
    assert torch.equal(gr_amd.ops.t5_embed(b, seq[swapped], mask[swapped]), full[swapped])
    assert gr_amd.ops.t5_embed(b, seq[:0], mask[:0]).shape == (0, full.shape[1])


def test_no_host_round_trip(dev):
    sd, seq, mask, want = _deployed()
    m = _module(_params(DEPLOYED), sd, dev)
    seq, mask = seq.to(dev), mask.to(dev)
    target = torch.randn(8, 768, generator=torch.Generator().manual_seed(9)).to(dev)
    first = m.generate(seq, mask)                 # fills the binding, the bucket table, the workspace size
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")       # any device-to-host copy or synchronisation raises
    try:
        loss, second = m(seq, mask, target_emb=target)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first, second) and loss.dim() == 0
    assert ref.live_err(second.cpu(), want["pred64"]) <= 4 * want["pred_err32"]
    bind = m.binding()
    with torch.no_grad():
        m.output_proj.bias += 0.25                 # an in-place update is seen by the next call
    assert m.binding() is bind and not torch.equal(m.generate(seq, mask), first)


@functools.lru_cache(maxsize=None)
def _retrieval():
    """Deployed-width model, 16 users, a 707 x 768 catalog; the float64 scores and the float32 restatement's
    distance from them; targets: every other user's is one of its own float64 top 20."""
    g = torch.Generator().manual_seed(RETRIEVAL_SEED)
    sd = tf.random_state(DEPLOYED, RETRIEVAL_SEED)
    seq, mask = tf.sequences(16, 21, 768, RETRIEVAL_SEED)
    items = torch.randn(707, 768, generator=g)
    target_emb = torch.randn(16, 768, generator=g)
    want = tf.restate(DEPLOYED, sd, seq, mask)
    s64 = ref.scores(want["pred64"], items)
    s32 = ref.scores(want["pred32"], items)
    score_err = (s32.double() - s64).abs().max().item()
    top = torch.topk(s64, 21, dim=1)
    gaps = -(top.values.diff(dim=1))
    certified = gaps.min(dim=1).values > 4 * score_err
    target_id = torch.randint(0, 707, (16,), generator=g)
    for u in range(0, 16, 2):
        target_id[u] = top.indices[u, (3 * u) % 20]
    loss64 = ref.info_nce(want["pred64"], target_emb, DEPLOYED["temperature"]).item()
    return dict(sd=sd, seq=seq, mask=mask, items=items, target_emb=target_emb, target_id=target_id, ids64=top.indices[:, :20],
                certified=certified, score_err=score_err, loss64=loss64, want=want)


def test_retrieval_against_float64(dev):
    """Catalog 707 x 768, k 20, 16 users at the deployed width.  A user is certified when every gap among its
    top 21 float64 scores exceeds 4 x the float32 restatement's score error; certified users' id lists must
    match the float64 run exactly, in order.  Seed 7: the float64 run alone certifies 16 of 16 users."""
    import gr_amd
    from gr_amd import t5_embed
    r = _retrieval()
    share = r["certified"].float().mean().item()
    print(f"retrieval: score err32 {r['score_err']:.3e}, certified {int(r['certified'].sum())}/16")
    assert share >= 0.9
    m = _module(_params(DEPLOYED), r["sd"], dev)
    seq, mask, items = r["seq"].to(dev), r["mask"].to(dev), r["items"].to(dev)
    pred = m.generate(seq, mask)
    vals, ids = t5_embed.retrieve(pred, items, 20)
    assert ids.shape == (16, 20) and ids.dtype == torch.int64 and (vals.diff(dim=1) <= 0).all()
    ids = ids.cpu()
    for u in range(16):
        if r["certified"][u]:
            assert torch.equal(ids[u], r["ids64"][u]), u
    # the metric tail on two batches of 8 against the restatement's on the float64 lists
    topk = [5, 10, 20]
    cut = (slice(0, 8), slice(8, 16))
    batches = [dict(seq_embs=r["seq"][c], attention_mask=r["mask"][c], target_id=r["target_id"][c]) for c in cut]
    rec, nd = t5_embed.evaluate_batches(batches, m, r["items"], topk)
    per = [ref.metrics(r["ids64"][c], r["target_id"][c], topk) for c in cut]
    for k in topk:      # the hit counts are exact; the discounts 1 / log2(rank + 1) are float32 on either side
        assert rec[f"Recall@{k}"] == sum(p[f"Recall@{k}"] for p in per) / 2
        assert nd[f"NDCG@{k}"] == pytest.approx(sum(p[f"NDCG@{k}"] for p in per) / 2, rel=1e-6)
    assert rec["Recall@20"] >= 0.5
    # eval_loss-style forward
    loss, out = m(seq, mask, target_emb=r["target_emb"].to(dev))
    assert torch.equal(out, pred)
    assert abs(loss.item() - r["loss64"]) <= 1e-5 * abs(r["loss64"]), (loss.item(), r["loss64"])
