"""Plain-torch restatement of TIGER inference (RQVAE-T5/model.py: a T5 encoder-decoder searched by
``generate(max_length=5, num_beams=k, num_return_sequences=k)``), in the dtype of the state dict it is
given (float32 or float64).  No ``transformers`` import: it restates what the library computes for
this configuration, quirks included.

The T5 stack: shared embedding, pre-RMSNorm blocks (no mean, no bias), attention without the
1/sqrt(d) scale, the bucketed relative-position bias (32 buckets, max distance 128; bidirectional in
the encoder, one-directional in the decoder; the table lives in block 0 and later blocks reuse it),
the additive padding mask on encoder keys and on cross-attention, the ReLU feed-forward, the final
norms and the tied lm_head behind its d_model**-0.5 scale.

The beam search (GenerationMixin._beam_search and its helpers): 2*num_beams continuations kept per
step, running scores [0, -1e9, ...], the -1e9 maskings, the /(cur_len + 1 - prompt_len) length
normalisation of finished hypotheses, the early-stop heuristic and the final selection.

Two things the library does that one would not expect:

* The static-shaped hypothesis buffers are filled with ``pad_token_id or eos_token_id[0]``.  The
  reference's pad id is 0, which is falsy, so the fill is the *EOS* id: a hypothesis that ends early
  reads [pad, a, EOS, EOS, EOS], and when EOS is not token 0 every position after the first EOS
  holds a non-pad token.  (That is the "non-pad tokens follow an EOS token" of the probe.)
* The result is cropped to the longest hypothesis of the whole batch.  ``beam_search`` returns the
  static ``[B, k, max_length]`` buffers and the crop width separately, so a user's rows never depend
  on the rest of the batch.
"""
import math

import torch

NUM_BUCKETS = 32
MAX_DISTANCE = 128
NEG = -1.0e9


def relative_bucket(relative_position, bidirectional, num_buckets=NUM_BUCKETS, max_distance=MAX_DISTANCE):
    """T5Attention._relative_position_bucket (relative_position = key position - query position)."""
    rp = relative_position
    buckets = torch.zeros_like(rp)
    if bidirectional:
        num_buckets //= 2
        buckets = buckets + (rp > 0).to(torch.long) * num_buckets
        rp = rp.abs()
    else:
        rp = -torch.min(rp, torch.zeros_like(rp))
    max_exact = num_buckets // 2
    is_small = rp < max_exact
    large = max_exact + (torch.log(rp.float() / max_exact) / math.log(max_distance / max_exact)
                         * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(is_small, rp, large)


def _norm(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def _heads(x, n_heads):
    return x.view(*x.shape[:-1], n_heads, -1).transpose(-2, -3)       # [..., H, L, d_kv]


def _attend(q, k, v, bias):
    """q [.., H, Lq, dk], k / v [.., H, Lk, dk], bias broadcastable to [.., H, Lq, Lk] (additive)."""
    w = torch.softmax(q @ k.transpose(-1, -2) + bias, dim=-1)
    o = w @ v
    return o.transpose(-2, -3).reshape(*o.shape[:-3], o.shape[-2], -1)


class Model:
    def __init__(self, cfg, sd):
        self.cfg = cfg
        self.sd = sd
        self.H = int(cfg["num_heads"])
        self.eps = float(cfg.get("layer_norm_epsilon", 1e-6))
        self.dtype = sd["shared.weight"].dtype
        self.scale_lm = bool(cfg.get("scale_decoder_outputs", True))

    def w(self, name):
        return self.sd[name]

    def encode(self, input_ids, attention_mask):
        """[B, S] ids and 0/1 mask -> encoder output [B, S, d_model] (after the final norm)."""
        sd, H = self.sd, self.H
        B, S = input_ids.shape
        x = sd["shared.weight"][input_ids]
        pos = torch.arange(S)
        bucket = relative_bucket(pos[None, :] - pos[:, None], True)
        bias = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"][bucket]   # [S, S, H]
        bias = bias.permute(2, 0, 1)[None]
        mask = torch.zeros(B, 1, 1, S, dtype=self.dtype)
        mask = mask.masked_fill(attention_mask[:, None, None, :] == 0, torch.finfo(self.dtype).min)
        bias = bias + mask
        for i in range(int(self.cfg["num_layers"])):
            p = f"encoder.block.{i}.layer."
            h = _norm(x, sd[p + "0.layer_norm.weight"], self.eps)
            q = _heads(h @ sd[p + "0.SelfAttention.q.weight"].T, H)
            k = _heads(h @ sd[p + "0.SelfAttention.k.weight"].T, H)
            v = _heads(h @ sd[p + "0.SelfAttention.v.weight"].T, H)
            x = x + _attend(q, k, v, bias) @ sd[p + "0.SelfAttention.o.weight"].T
            h = _norm(x, sd[p + "1.layer_norm.weight"], self.eps)
            x = x + torch.relu(h @ sd[p + "1.DenseReluDense.wi.weight"].T) @ sd[p + "1.DenseReluDense.wo.weight"].T
        return _norm(x, sd["encoder.final_layer_norm.weight"], self.eps)

    def cross_kv(self, enc):
        out = []
        for i in range(int(self.cfg["num_decoder_layers"])):
            p = f"decoder.block.{i}.layer.1.EncDecAttention."
            out.append((_heads(enc @ self.sd[p + "k.weight"].T, self.H), _heads(enc @ self.sd[p + "v.weight"].T, self.H)))
        return out

    def decode(self, dec_ids, cross, attention_mask):
        """Teacher-forced decoder: dec_ids [N, L], cross K/V and mask of the N rows -> logits [N, L, V]."""
        sd, H = self.sd, self.H
        N, Ld = dec_ids.shape
        x = sd["shared.weight"][dec_ids]
        pos = torch.arange(Ld)
        bucket = relative_bucket(pos[None, :] - pos[:, None], False)
        bias = sd["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"][bucket].permute(2, 0, 1)[None]
        causal = torch.zeros(Ld, Ld, dtype=self.dtype).masked_fill(pos[None, :] > pos[:, None],
                                                                    torch.finfo(self.dtype).min)
        bias = bias + causal
        S = attention_mask.shape[1]
        cmask = torch.zeros(N, 1, 1, S, dtype=self.dtype)
        cmask = cmask.masked_fill(attention_mask[:, None, None, :] == 0, torch.finfo(self.dtype).min)
        for i in range(int(self.cfg["num_decoder_layers"])):
            p = f"decoder.block.{i}.layer."
            h = _norm(x, sd[p + "0.layer_norm.weight"], self.eps)
            q = _heads(h @ sd[p + "0.SelfAttention.q.weight"].T, H)
            k = _heads(h @ sd[p + "0.SelfAttention.k.weight"].T, H)
            v = _heads(h @ sd[p + "0.SelfAttention.v.weight"].T, H)
            x = x + _attend(q, k, v, bias) @ sd[p + "0.SelfAttention.o.weight"].T
            h = _norm(x, sd[p + "1.layer_norm.weight"], self.eps)
            q = _heads(h @ sd[p + "1.EncDecAttention.q.weight"].T, H)
            x = x + _attend(q, cross[i][0], cross[i][1], cmask) @ sd[p + "1.EncDecAttention.o.weight"].T
            h = _norm(x, sd[p + "2.layer_norm.weight"], self.eps)
            x = x + torch.relu(h @ sd[p + "2.DenseReluDense.wi.weight"].T) @ sd[p + "2.DenseReluDense.wo.weight"].T
        x = _norm(x, sd["decoder.final_layer_norm.weight"], self.eps)
        if self.scale_lm:
            x = x * (int(self.cfg["d_model"]) ** -0.5)
        return x @ sd["lm_head.weight"].T


def _decode_step(m, tokens, t, cache, cross, attention_mask):
    """The library's cached decoder step: one query row per beam at position t against the cached keys
    and values of positions 0..t (``cache``: per layer [K, V] of shape [N, H, t, d_kv], extended in
    place).  The same values as ``Model.decode``'s last row, in the library's own operand shapes."""
    sd, H = m.sd, m.H
    x = sd["shared.weight"][tokens][:, None, :]                                   # [N, 1, D]
    rp = torch.arange(t + 1)[None, :] - t
    bias = sd["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"][relative_bucket(rp, False)]
    bias = bias.permute(2, 0, 1)[None]                                             # [1, H, 1, t + 1]
    N, S = attention_mask.shape
    cmask = torch.zeros(N, 1, 1, S, dtype=m.dtype)
    cmask = cmask.masked_fill(attention_mask[:, None, None, :] == 0, torch.finfo(m.dtype).min)
    for i in range(int(m.cfg["num_decoder_layers"])):
        p = f"decoder.block.{i}.layer."
        h = _norm(x, sd[p + "0.layer_norm.weight"], m.eps)
        q = _heads(h @ sd[p + "0.SelfAttention.q.weight"].T, H)
        k = _heads(h @ sd[p + "0.SelfAttention.k.weight"].T, H)
        v = _heads(h @ sd[p + "0.SelfAttention.v.weight"].T, H)
        if cache[i] is not None:
            k, v = torch.cat((cache[i][0], k), -2), torch.cat((cache[i][1], v), -2)
        cache[i] = [k, v]
        x = x + _attend(q, k, v, bias) @ sd[p + "0.SelfAttention.o.weight"].T
        h = _norm(x, sd[p + "1.layer_norm.weight"], m.eps)
        q = _heads(h @ sd[p + "1.EncDecAttention.q.weight"].T, H)
        x = x + _attend(q, cross[i][0], cross[i][1], cmask) @ sd[p + "1.EncDecAttention.o.weight"].T
        h = _norm(x, sd[p + "2.layer_norm.weight"], m.eps)
        x = x + torch.relu(h @ sd[p + "2.DenseReluDense.wi.weight"].T) @ sd[p + "2.DenseReluDense.wo.weight"].T
    x = _norm(x, sd["decoder.final_layer_norm.weight"], m.eps)
    if m.scale_lm:
        x = x * (int(m.cfg["d_model"]) ** -0.5)
    return (x @ sd["lm_head.weight"].T)[:, 0, :]


def _gather(t, idx):
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.take_along_dim(t, idx, dim=1)


def beam_search(cfg, sd, input_ids, attention_mask=None, num_beams=20, max_length=5, trace=None, use_cache=True):
    """-> (sequences [B, k, max_length] int64, scores [B, k], width).  ``width`` is the column count the
    library crops its result to.  ``use_cache=False`` restates the library's cache-less decoding (the same
    values from other operand shapes: the last bits of the scores differ).  ``trace`` (a dict) receives the encoder output, per step the logits of
    the live beams and the selection gaps that the certification reads, and ``stopped_after``: per user
    the number of steps after which the early-stop heuristic was satisfied (-1: never; the search
    kernel runs no further step for that user, the library runs them and ignores their result)."""
    m = Model(cfg, sd)
    B, S = input_ids.shape
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids)
    k, V = int(num_beams), int(cfg["vocab_size"])
    pad, eos = int(cfg["pad_token_id"]), int(cfg["eos_token_id"])
    keep = 2 * k
    fill = pad or eos                       # the library's `pad_token_id or eos_token_id[0]`
    enc = m.encode(input_ids, attention_mask)
    cross = [(kk.repeat_interleave(k, 0), vv.repeat_interleave(k, 0)) for kk, vv in m.cross_kv(enc)]
    mask_k = attention_mask.repeat_interleave(k, 0)
    run_seq = torch.full((B, k, max_length), fill, dtype=torch.int64)
    run_seq[:, :, 0] = pad                  # decoder_start_token_id = pad
    seqs = run_seq.clone()
    run_scores = torch.zeros(B, k, dtype=torch.float32)
    run_scores[:, 1:] = NEG
    scores = torch.full((B, k), NEG, dtype=torch.float32)
    if m.dtype == torch.float64:            # the float64 restatement keeps its scores in float64
        run_scores, scores = run_scores.double(), scores.double()
    finished = torch.zeros(B, k, dtype=torch.bool)
    unsat = torch.ones(B, 1, dtype=torch.bool)
    run_idx = torch.full((B, k, max_length - 1), -1, dtype=torch.int32)
    idx = run_idx.clone()
    top_mask = torch.cat((torch.ones(k, dtype=torch.bool), torch.zeros(keep - k, dtype=torch.bool)))
    if trace is not None:
        trace.update(enc=enc, logits=[], gaps=torch.full((B,), float("inf"), dtype=torch.float64),
                     live=[], steps=0, stopped_after=torch.full((B,), -1, dtype=torch.int64))
    cache = [None] * int(cfg["num_decoder_layers"])
    cur = 1
    while True:
        if use_cache:       # the library's default: one query row per beam, keys and values reordered by parent
            logits = _decode_step(m, run_seq[:, :, cur - 1].reshape(B * k), cur - 1, cache, cross, mask_k)
        else:               # use_cache=False: the whole prefix again at every step
            logits = m.decode(run_seq[:, :, :cur].reshape(B * k, cur), cross, mask_k)[:, -1, :]
        logp = torch.log_softmax(logits if m.dtype == torch.float64 else logits.float(), dim=-1)
        acc = (logp.view(B, k, V) + run_scores[:, :, None]).reshape(B, k * V)
        top, ti = torch.topk(acc, keep)
        parent = ti // V
        top_seq = _gather(run_seq, parent)
        top_seq[:, :, cur] = ti % V
        top_idx = _gather(run_idx, parent)
        top_idx[:, :, cur - 1] = (parent + torch.arange(B)[:, None] * k).to(torch.int32)
        hits = (top_seq[:, :, cur] == eos) | (cur + 1 >= max_length)
        # running beams of the next step
        top_run = top + hits.to(torch.float32) * NEG
        nxt = torch.topk(top_run, k)[1]
        # finished beams
        just = hits & top_mask[None, :]
        fin = top / float(cur + 1 - 1)
        fin = fin + (~unsat).to(torch.float32) * NEG
        fin = fin + (~just) * NEG
        if trace is not None:
            _trace_step(trace, logits.view(B, k, V), acc, top, top_run, nxt, scores, fin, unsat, cur)
        run_seq, run_scores, run_idx = _gather(top_seq, nxt), _gather(top_run, nxt), _gather(top_idx, nxt)
        if use_cache:
            flat_parent = run_idx[:, :, cur - 1].reshape(-1).long()
            cache = [[kv[0].index_select(0, flat_parent), kv[1].index_select(0, flat_parent)] for kv in cache]
        m_seq, m_sc = torch.cat((seqs, top_seq), 1), torch.cat((scores, fin), 1)
        m_idx, m_fin = torch.cat((idx, top_idx), 1), torch.cat((finished, just), 1)
        sel = torch.topk(m_sc, k)[1]
        seqs, scores, idx, finished = _gather(m_seq, sel), _gather(m_sc, sel), _gather(m_idx, sel), _gather(m_fin, sel)
        cur += 1
        best = run_scores[:, :1] / float(cur - 1)
        worst = torch.where(finished, scores.min(1, keepdim=True)[0], torch.full_like(scores, NEG))
        unsat = unsat & (best > worst).any(-1, keepdim=True)
        if trace is not None:       # the number of steps after which the user's heuristic was first satisfied
            first = (~unsat[:, 0]) & (trace["stopped_after"] < 0)
            trace["stopped_after"][first] = cur - 1
        if not (bool(unsat.any()) and not bool(hits.all())):
            break
    width = 1 + int(((idx + 1).bool()).sum(-1).max())
    return seqs, scores, width


def _trace_step(trace, logits, acc, top, top_run, nxt, scores, fin, unsat, cur):
    """Record the live beams' logits and, per user, the smallest gap of this step's selections: between
    adjacent kept scores and between the last kept and the first dropped one, ignoring every entry that
    carries a -1e9 mask.  A user whose search has stopped (heuristic satisfied) adds nothing."""
    B, k, V = logits.shape
    live = 1 if cur == 1 else k
    trace["logits"].append(logits[:, :live].clone())
    trace["live"].append(live)
    trace["steps"] += 1
    big = NEG / 2
    for b in range(B):
        if not bool(unsat[b]):
            continue
        g = float("inf")
        # selection 1: the 2k continuations among k*V candidates
        s = torch.sort(acc[b].double(), descending=True)[0]
        s = s[s > big][: top.shape[1] + 1]
        if s.numel() > 1:
            g = min(g, float((s[:-1] - s[1:]).min()))
        # selection 2: the k running beams among the unmasked continuations
        r = torch.sort(top_run[b].double(), descending=True)[0]
        r = r[r > big][: k + 1]
        if r.numel() > 1:
            g = min(g, float((r[:-1] - r[1:]).min()))
        # selection 3: the k finished hypotheses among old and new
        f = torch.sort(torch.cat((scores[b], fin[b])).double(), descending=True)[0]
        f = f[f > big][: k + 1]
        if f.numel() > 1:
            g = min(g, float((f[:-1] - f[1:]).min()))
        trace["gaps"][b] = min(float(trace["gaps"][b]), g)


def generate(cfg, sd, input_ids, attention_mask=None, num_beams=20, max_length=5):
    """The library's return value: [B * num_beams, width] int64."""
    seqs, _, width = beam_search(cfg, sd, input_ids, attention_mask, num_beams, max_length)
    return seqs.reshape(-1, max_length)[:, :width]


def rescore(cfg, sd, input_ids, attention_mask, sequences):
    """Teacher-forced, length-normalised score of each returned hypothesis: sequences [B, k, T] ->
    [B, k] in the state dict's dtype.  A hypothesis ends at its first EOS after the start token, or at
    T; the sum of its token log-probabilities is divided by the number of generated tokens."""
    m = Model(cfg, sd)
    B, k, T = sequences.shape
    eos = int(cfg["eos_token_id"])
    enc = m.encode(input_ids, attention_mask)
    cross = [(kk.repeat_interleave(k, 0), vv.repeat_interleave(k, 0)) for kk, vv in m.cross_kv(enc)]
    flat = sequences.reshape(B * k, T)
    logits = m.decode(flat[:, :-1], cross, attention_mask.repeat_interleave(k, 0))
    logp = torch.log_softmax(logits, -1).gather(-1, flat[:, 1:, None])[..., 0]       # [N, T-1]
    is_eos = flat[:, 1:] == eos
    first = torch.where(is_eos.any(1), is_eos.float().argmax(1), torch.full((B * k,), T - 2))
    n_gen = first + 1
    keep = torch.arange(T - 1)[None, :] < n_gen[:, None]
    return ((logp * keep).sum(1) / n_gen).view(B, k)


def pos_index(preds, labels):
    """utils.calculate_pos_index: the first beam whose tokens equal the label row."""
    B, k, _ = preds.shape
    out = torch.zeros(B, k, dtype=torch.bool)
    for i in range(B):
        lab = labels[i].tolist()
        for j in range(k):
            if preds[i, j].tolist() == lab:
                out[i, j] = True
                break
    return out


def metrics(pos, topk_list):
    """utils.recall_at_k / ndcg_at_k means of one batch, as Python floats."""
    rec, nd = {}, {}
    ranks = torch.arange(1, pos.shape[-1] + 1)
    dcg = torch.where(pos, 1.0 / torch.log2(ranks + 1), torch.tensor(0.0, dtype=torch.float))
    for kk in topk_list:
        rec[f"Recall@{kk}"] = pos[:, :kk].sum(dim=1).float().mean().item()
        nd[f"NDCG@{kk}"] = dcg[:, :kk].sum(dim=1).float().mean().item()
    return rec, nd
