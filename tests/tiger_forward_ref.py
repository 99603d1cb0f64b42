"""Plain-torch restatement of TIGER's teacher-forced forward (RQVAE-T5/model.py ``TIGER.forward`` with
``labels`` in eval mode, i.e. ``T5ForConditionalGeneration.forward``), in the dtype of the state dict it is
given.  The stack is tests/tiger_ref.py's ``Model`` (``encode``, ``cross_kv``, ``decode``); this file adds
what the library does around it:

* ``_shift_right``: the decoder input row is ``[pad_token_id, labels[:, :-1]]`` with every -100 replaced by
  the pad id (a -100 in the middle of a row is legal);
* the loss is torch's cross-entropy rule with ``ignore_index=-100``: the mean over the counted positions of
  ``-log_softmax(logits)[label]``; no counted position in the whole batch gives NaN (0 / 0);
* a label outside ``[0, vocab)`` that is not -100 is an error in torch; here, as in the kernel, the embedding
  read clamps it and its NLL -- and with it the loss -- is NaN.
"""
import torch

import tiger_prefix_ref as pref
import tiger_ref

IGNORE = -100


def shift_right(labels, pad):
    """[B, Ld] labels -> the decoder input ids."""
    dec = torch.full_like(labels, pad)
    dec[:, 1:] = labels[:, :-1]
    return dec.masked_fill(dec == IGNORE, pad)


def _loss(logits, labels):
    """(loss 0-dim, nll [B, Ld] with 0 where not counted) from logits [B, Ld, V]."""
    V = logits.shape[-1]
    counted = labels != IGNORE
    bad = counted & ((labels < 0) | (labels >= V))
    logp = torch.log_softmax(logits, -1).gather(-1, labels.clamp(0, V - 1)[..., None])[..., 0]
    nll = torch.where(counted, -logp, torch.zeros_like(logp))
    nll = torch.where(bad, torch.full_like(nll, float("nan")), nll)
    return nll.sum() / counted.sum().to(nll.dtype), nll


def _forward(m, input_ids, attention_mask, labels):
    cfg = m.cfg
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids)
    V = int(cfg["vocab_size"])
    enc = m.encode(input_ids, attention_mask)
    dec_ids = shift_right(labels, int(cfg["pad_token_id"])).clamp(0, V - 1)
    logits = m.decode(dec_ids, m.cross_kv(enc), attention_mask)
    loss, nll = _loss(logits, labels)
    return loss, logits, nll


def forward(cfg, sd, input_ids, attention_mask, labels):
    """-> (loss 0-dim, logits [B, Ld, V], nll [B, Ld]) in the state dict's dtype."""
    with torch.no_grad():
        return _forward(tiger_ref.Model(cfg, sd), input_ids, attention_mask, labels)


def forward_prefix(cfg, sd, input_ids, attention_mask, prof, labels):
    """``forward`` on the prefixed input: the three adapter tokens ahead of the history (S + 3 encoder
    positions), as tests/tiger_prefix_ref.py builds them; prof = (prof_lvl1, prof_lvl2, prof_lvl3)."""
    with torch.no_grad():
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        prefix = pref.prefix_tokens(cfg, sd, input_ids, prof)
        ids, mask = pref.extend(input_ids, attention_mask)
        with pref.prefixed(prefix):
            return _forward(tiger_ref.Model(cfg, sd), ids, mask, labels)
