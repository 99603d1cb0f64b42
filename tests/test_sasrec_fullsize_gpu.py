"""SASRec at BASELINE's full catalog sizes against the CPU oracle, over the WHOLE bench batch
(every one of the bench's 2,048 C3 users and 512 C5 users, not a sample).

A real ``SASRec`` with the bench's weights (``synth.sasrec_model``) scores the bench's sequences on
the GPU at the bench batch; ``oracle/sasrec_oracle.forward`` (SASRec/model.py:49-96) runs the same
users on the host and the oracle logits (model.py:98-108) are formed in user chunks, so host memory
stays bounded at the 1M-row catalog.  Per user:

* logits: ``|gpu - oracle| <= 1e-5 * max|row|`` (north_star's tolerance, row-scaled), every user;
* ranks (SASRec/evaluate.py:27-32): exact for every user whose oracle target logit has no
  competitor within 2 delta; every user's GPU rank lies in the band
  ``#{l > t + 2 delta} + 1 <= rank <= #{l > t - 2 delta} + 1``.  delta = BAND x row scale, the
  triangle bound of a GPU logit against the fp32 oracle: the kernels' fp64 logits tolerance plus the
  oracle's own worst distance from fp64 (tests/test_sasrec_infer_fp64_gpu.py: 3e-6 + 6.5e-7), about
  a third of the 1e-5 bar; the whole-batch logits error is held to it as well;
* HR@10 and NDCG@10 of the whole batch (evaluate.py:35-47, float64 ``np.mean``) equal the oracle's;
* top-10 (C5, ``dist.sharded_rank_topk`` and an 8-shard merge on one GPU): values within delta of
  the oracle's value for the same id, ids equal to the oracle's top-10 wherever consecutive oracle
  values are more than 2 delta apart, and always inside ``{j : l_j >= v_10 - 2 delta}``.

Half of the users' targets come from the oracle's top-20 (non-trivial HR@10), half are uniform.
"""
import numpy as np
import pytest
import torch

from oracle import sasrec_oracle
from test_sasrec_infer_fp64_gpu import T32_LOGITS, TOL_LOGITS

pytestmark = pytest.mark.gpu
TOL = 1e-5
BAND = TOL_LOGITS + T32_LOGITS   # |gpu - fp64| + |fp64 - fp32 oracle|, row-scaled
CHUNK = 64          # users per host-side oracle logits chunk ([64, 1M] fp32 = 256 MB at C5)


def _sd(model, table=None):
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    if table is not None:
        sd["item_emb.weight"] = table.detach().cpu()
    return sd


def _oracle_hidden(model, seqs_cpu, sd):
    """LN_last(x)[:, -1, :] of the oracle forward (model.py:96, 104)."""
    return sasrec_oracle.forward(seqs_cpu, sd, model.num_blocks, model.num_heads,
                                 model.layernorm_eps)[:, -1, :].contiguous()


def _hr_ndcg(ranks, k=10):
    from gr_amd import evaluate
    return evaluate.hr_ndcg(ranks, k)


class _Batch:
    """Accumulates per-user comparisons of one whole batch, chunk by chunk."""

    def __init__(self, seed):
        self.g = np.random.default_rng(seed)
        self.err = 0.0
        self.targets, self.exact, self.lo, self.hi, self.iso = [], [], [], [], []
        self.topk_exact = 0
        self.topk_checked = 0

    def add(self, got, ref):
        """``got``, ``ref``: [c, rows] fp32 logits of the same users (GPU, oracle).  Returns the
        chunk's targets and per-user delta."""
        scale = ref.abs().amax(1)
        self.err = max(self.err, float(((got - ref).abs().amax(1) / scale).max()))
        delta = (scale * BAND).double()
        lg = ref.double()
        lg[:, 0] = -1e9
        c, rows = lg.shape
        top20 = torch.topk(lg, 20, dim=1).indices.numpy()
        tg = torch.from_numpy(np.where(self.g.random(c) < 0.5, top20[np.arange(c), self.g.integers(0, 20, c)],
                                       self.g.integers(1, rows, c)).astype(np.int64))
        t = lg.gather(1, tg[:, None])
        self.exact.append(((lg > t).sum(1) + 1).numpy())
        lo = ((lg > t + 2 * delta[:, None]).sum(1) + 1).numpy()
        hi = ((lg > t - 2 * delta[:, None]).sum(1) + 1).numpy()   # counts the target itself: +1 slack
        self.lo.append(lo)
        self.hi.append(hi)
        self.iso.append(lo == hi - 1)                                 # only the target in the band
        self.targets.append(tg)
        return tg, delta, lg

    def topk(self, v, i, lg, delta, k=10):
        """GPU top-k (values ``v``, ids ``i``, [c, k]) against the chunk's masked oracle logits."""
        ov, oi = torch.topk(lg, k + 1, dim=1)             # descending; ties only matter where excluded
        v, i = v.double().cpu(), i.cpu()
        vb = lg.gather(1, i)                               # oracle value at the GPU's ids
        assert ((vb - v).abs() <= delta[:, None]).all()
        assert (vb >= ov[:, k - 1:k] - 2 * delta[:, None]).all()     # inside the top-k band
        assert (i.sort(1).values[:, 1:] != i.sort(1).values[:, :-1]).all()   # distinct ids
        gaps = ov[:, :k] - ov[:, 1:k + 1]
        sep = (gaps > 2 * delta[:, None]).all(1)
        assert torch.equal(i[sep], oi[sep, :k])
        self.topk_exact += int(sep.sum())
        self.topk_checked += len(sep)

    def finish(self, ranks, parity_log, **info):
        exact, lo, hi, iso = (np.concatenate(x) for x in (self.exact, self.lo, self.hi, self.iso))
        assert ((ranks >= lo) & (ranks <= hi)).all(), np.nonzero((ranks < lo) | (ranks > hi))
        assert np.array_equal(ranks[iso], exact[iso])
        hr_o, nd_o = _hr_ndcg(exact)
        hr_g, nd_g = _hr_ndcg(ranks)
        rec = dict(users=len(ranks), max_row_scaled_logit_err=self.err,
                   ranks_exact=int((ranks == exact).sum()), ranks_isolated=int(iso.sum()), band=BAND,
                   ranks_in_band=int(((ranks >= lo) & (ranks <= hi)).sum()),
                   hr10_oracle=hr_o, hr10_gpu=hr_g, ndcg10_oracle=nd_o, ndcg10_gpu=nd_g, **info)
        if self.topk_checked:
            rec.update(top10_users_checked=self.topk_checked, top10_exact_users=self.topk_exact)
        parity_log(**rec)
        assert self.err <= TOL
        assert self.err <= BAND      # what the rank / top-k bands above rest on
        assert hr_g == hr_o and nd_g == nd_o, (hr_g, hr_o, nd_g, nd_o)


def test_c3_full_catalog_vs_oracle(dev, parity_log):
    """C3: 2 blocks, d 64, n 50, 100,001-row table; the bench's 2048-user batch, EVERY user through
    the oracle: contiguous predict logits, the rank over materialised logits and the fused rank."""
    from gr_amd import evaluate, ops, synth
    items, n, B = 100_000, 50, 2048
    model = synth.sasrec_model(items, synth.sasrec_params(64, n, 2, 1, 64, dev), dev)
    seqs = synth.sequences(B, n, items, 2000, dev)
    logits = model.predict(seqs)
    sd = _sd(model)
    h_ref = _oracle_hidden(model, seqs.cpu(), sd)
    table = sd["item_emb.weight"]
    acc = _Batch(3)
    for c0 in range(0, B, CHUNK):
        ref = h_ref[c0:c0 + CHUNK].matmul(table.t())             # model.py:107
        acc.add(logits[c0:c0 + CHUNK].cpu(), ref)
    tg = torch.cat(acc.targets).to(dev)
    r_mat = ops.rank(logits, tg).cpu().numpy()
    r_fused = evaluate.rank_batch(model, seqs, tg).cpu().numpy()
    assert np.array_equal(r_fused, r_mat)
    acc.finish(r_mat, parity_log, kind="sasrec_full_size", config="C3 (100,001 rows, d 64, n 50), whole batch")


def test_c5_full_catalog_vs_oracle(dev, parity_log):
    """C5: d 128, n 200, 1,000,001-row table; the bench's 512 users, EVERY user through the oracle;
    predict logits, the single-shard and the 8-shard catalog-sharded rank + top-10."""
    from gr_amd import dist as D, ops, synth
    items, n, B, k = 1_000_000, 200, 512, 10
    model = synth.sasrec_model(items, synth.sasrec_params(128, n, 2, 1, 64, dev), dev, seed=5)
    seqs = synth.sequences(B, n, items, 5000, dev)
    h = model.last_hidden(seqs)
    sd = _sd(model)
    h_ref = _oracle_hidden(model, seqs.cpu(), sd)
    table = model.item_emb.weight.detach()
    table_cpu = sd["item_emb.weight"]
    acc = _Batch(7)
    chunks = []
    for c0 in range(0, B, CHUNK):
        got = model.predict(seqs[c0:c0 + CHUNK])
        if c0 == 0:   # predict = the scoring kernel on the forward's hidden states, bit for bit
            assert torch.equal(ops.score(h[:CHUNK], table), got)
        ref = h_ref[c0:c0 + CHUNK].matmul(table_cpu.t())           # model.py:107
        tg, delta, lg = acc.add(got.cpu(), ref)
        del got, ref
        _, v1, i1 = D.sharded_rank_topk(h[c0:c0 + CHUNK], table, 0, tg.to(dev), k=k)
        acc.topk(v1, i1, lg, delta, k)
        chunks.append((v1, i1))
        del lg
    targets = torch.cat(acc.targets).to(dev)
    rank1, v1, i1 = D.sharded_rank_topk(h, table, 0, targets, k=k)
    assert torch.equal(v1, torch.cat([c[0] for c in chunks])) and torch.equal(i1, torch.cat([c[1] for c in chunks]))
    # 8 catalog shards on one GPU: the per-rank kernels of the 8-GPU run, merged as dist._exchange
    rows = items + 1
    ts = torch.zeros(B, device=dev)
    shards = [D.shard_range(rows, r, 8) for r in range(8)]
    for lo, hi in shards:
        own = (targets >= lo) & (targets < hi)
        loc = torch.where(own, targets - lo, torch.zeros_like(targets))
        ts += torch.where(own, ops.score_pairs(h, table[lo:hi], loc, mask_col0=(lo == 0)), torch.zeros_like(ts))
    cnt = torch.zeros(B, dtype=torch.int64, device=dev)
    vs, is_ = [], []
    for lo, hi in shards:
        v, i, c = ops.score_topk(h, table[lo:hi], k, lo, thresholds=ts, mask_col0=(lo == 0))
        cnt += c
        vs.append(v)
        is_.append(i)
    v8, i8 = D.merge_topk(torch.cat(vs, 1), torch.cat(is_, 1), k)
    assert torch.equal(cnt + 1, rank1) and torch.equal(v8, v1) and torch.equal(i8, i1)
    acc.finish(rank1.cpu().numpy(), parity_log, kind="sasrec_full_size",
               config="C5 (1,000,001 rows, d 128, n 200), whole batch")


def test_c5_per_rank_construction_matches_full_table(dev):
    """bench.py's C5 leg builds, per rank, only its catalog shard and the table rows its own users
    gather (synth.sasrec_rank_model).  The hidden states of every world size's user shards, stitched
    together, equal the full-table model's bit for bit, and so does the merged rank / top-10."""
    import copy
    from gr_amd import dist as D, synth
    items, n, B, d = 1_000_000, 200, 512, 128
    p = synth.sasrec_params(d, n, 2, 1, 64, dev)
    seqs = synth.sequences(B, n, items, 5000, dev)
    table = synth.table_rows(torch.arange(items + 1, device=dev), d, 7, dev)
    m1, s1 = synth.sasrec_rank_model(items, p, seqs, dev, seed=5)
    full = copy.deepcopy(m1)
    full.item_emb = torch.nn.Embedding(items + 1, d, padding_idx=0).to(dev)
    with torch.no_grad():
        full.item_emb.weight.copy_(table)
    full.item_num = items
    h = full.last_hidden(seqs)
    assert torch.equal(m1.last_hidden(s1), h)
    for world in (2, 8):
        hs = []
        for r in range(world):
            lo, hi = D.shard_range(B, r, world)
            mr, sr = synth.sasrec_rank_model(items, p, seqs[lo:hi], dev, seed=5)
            hs.append(mr.last_hidden(sr))
        assert torch.equal(torch.cat(hs), h), world
        shards = [D.shard_range(items + 1, r, world) for r in range(world)]
        parts = [synth.table_rows(torch.arange(lo, hi, device=dev), d, 7, dev) for lo, hi in shards]
        assert torch.equal(torch.cat(parts), table)
