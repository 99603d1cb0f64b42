"""TIGER generative retrieval (RQVAE-T5/model.py): a small T5 encoder-decoder over semantic-ID tokens,
searched by beam search -- inference only, on the gfx950 kernels of csrc/tiger.hip.

``TIGER(config)`` takes the reference's config dict and holds the reference's parameter tree under the
reference's names (``model.shared.weight``, ``model.encoder.block.0.layer.0.SelfAttention.q.weight``,
..., tied entries included), so a reference checkpoint loads unchanged; it does not import
``transformers``.  ``generate`` is the reference's call (``max_length=5``, ``num_return_sequences =
num_beams``) as one C call with no host round trip.  ``forward(input_ids, attention_mask, labels)`` under
``.eval()`` and ``torch.no_grad()`` is the reference's evaluation call: the teacher-forced logits and the mean
cross-entropy over the labels that are not -100 (``eval_loss`` restates RQVAE-T5/train.py:40-51 on it); the
backward and the optimiser step are not built, so the same call in training mode raises.

``codes_to_tokens`` and ``collate`` reproduce the token map and ``GenRecDataLoader.collate_fn`` on
arrays, so the output of ``RQVAE.generate_codes`` feeds ``TIGER`` directly; ``evaluate_model`` restates
RQVAE-T5/utils.py:44-92 with the hit search on the device.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops

MAX_LENGTH = 5      # TIGER.generate's max_length (RQVAE-T5/model.py:77)
NUM_BUCKETS = 32    # T5Config defaults the reference leaves alone
LN_EPS = 1e-6


class _Norm(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))


class _Attention(nn.Module):
    def __init__(self, d_model, inner, n_heads, d_kv, rel_bias):
        super().__init__()
        self.q = nn.Linear(d_model, inner, bias=False)
        self.k = nn.Linear(d_model, inner, bias=False)
        self.v = nn.Linear(d_model, inner, bias=False)
        self.o = nn.Linear(inner, d_model, bias=False)
        if rel_bias:
            self.relative_attention_bias = nn.Embedding(NUM_BUCKETS, n_heads)
        with torch.no_grad():       # T5's initialisation (factor 1)
            self.q.weight.normal_(0.0, (d_model * d_kv) ** -0.5)
            self.k.weight.normal_(0.0, d_model ** -0.5)
            self.v.weight.normal_(0.0, d_model ** -0.5)
            self.o.weight.normal_(0.0, inner ** -0.5)
            if rel_bias:
                self.relative_attention_bias.weight.normal_(0.0, d_model ** -0.5)


class _AttnLayer(nn.Module):
    def __init__(self, name, cfg, rel_bias):
        super().__init__()
        d, H, dkv = cfg["d_model"], cfg["num_heads"], cfg["d_kv"]
        setattr(self, name, _Attention(d, H * dkv, H, dkv, rel_bias))
        self.layer_norm = _Norm(d)


class _Dense(nn.Module):
    def __init__(self, d, dff):
        super().__init__()
        self.wi = nn.Linear(d, dff, bias=False)
        self.wo = nn.Linear(dff, d, bias=False)
        with torch.no_grad():
            self.wi.weight.normal_(0.0, d ** -0.5)
            self.wo.weight.normal_(0.0, dff ** -0.5)


class _FFLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.DenseReluDense = _Dense(cfg["d_model"], cfg["d_ff"])
        self.layer_norm = _Norm(cfg["d_model"])


class _Block(nn.Module):
    def __init__(self, cfg, decoder, rel_bias):
        super().__init__()
        layers = [_AttnLayer("SelfAttention", cfg, rel_bias)]
        if decoder:
            layers.append(_AttnLayer("EncDecAttention", cfg, False))
        layers.append(_FFLayer(cfg))
        self.layer = nn.ModuleList(layers)


class _Stack(nn.Module):
    def __init__(self, cfg, shared, decoder):
        super().__init__()
        self.embed_tokens = shared
        n = cfg["num_decoder_layers"] if decoder else cfg["num_layers"]
        self.block = nn.ModuleList([_Block(cfg, decoder, i == 0) for i in range(n)])
        self.final_layer_norm = _Norm(cfg["d_model"])


class _T5(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.shared = nn.Embedding(cfg["vocab_size"], cfg["d_model"])
        with torch.no_grad():
            self.shared.weight.normal_(0.0, 1.0)
        self.encoder = _Stack(cfg, self.shared, False)
        self.decoder = _Stack(cfg, self.shared, True)
        self.lm_head = nn.Linear(cfg["d_model"], cfg["vocab_size"], bias=False)
        self.lm_head.weight = self.shared.weight          # tied


class TIGER(nn.Module):
    def __init__(self, config):
        super().__init__()
        ops.tiger_check_config(config)
        self.config = dict(config)
        self.model = _T5(self.config)
        self._binding = None
        self._binding_key = None

    @property
    def n_parameters(self):
        total = sum(p.numel() for p in self.parameters() if p.requires_grad)
        emb = self.model.shared.weight.numel()
        return (f'#Embedding parameters: {emb}\n#Non-embedding parameters: {total - emb}\n'
                f'#Total trainable parameters: {total}\n')

    def binding(self):
        """The parameters' device-pointer view, rebuilt when a parameter's storage moves."""
        tensors = {k: v for k, v in self.model.state_dict(keep_vars=True).items()}
        key = tuple(t.data_ptr() for t in tensors.values())
        if self._binding is None or key != self._binding_key:
            cfg = dict(self.config, layer_norm_epsilon=self.config.get("layer_norm_epsilon", LN_EPS))
            self._binding = ops.TigerBinding(cfg, {k: v.detach() for k, v in tensors.items()})
            self._binding_key = key
        return self._binding

    def _forward_guard(self, labels):
        if self.training or torch.is_grad_enabled():
            raise NotImplementedError("TIGER.forward in training mode or with gradients enabled is not built: training "
                                      "of the T5 model (backward and the optimiser step) is out of scope here; call it "
                                      "under .eval() and torch.no_grad() for the evaluation loss, or use generate()")
        if labels is None:
            raise ValueError("TIGER.forward needs labels: it is the teacher-forced evaluation call (loss, logits); "
                             "decoder_input_ids and the library's other keyword arguments are not built")

    def forward(self, input_ids, attention_mask=None, labels=None):
        """The reference's evaluation call (``eval_loss``): -> (loss 0-dim fp32, logits [B, Ld, vocab] fp32), the
        mean NLL over the labels that are not -100, as one C call with no host round trip."""
        self._forward_guard(labels)
        return ops.tiger_forward(self.binding(), input_ids, attention_mask, labels)

    @torch.no_grad()
    def generate_scored(self, input_ids, attention_mask=None, num_beams=20, max_length=MAX_LENGTH):
        """-> (sequences [B, num_beams, max_length] int64 best first, scores [B, num_beams] fp32)."""
        return ops.tiger_generate(self.binding(), input_ids, attention_mask, num_beams, max_length)

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, num_beams=20):
        """The reference's ``generate``: [B * num_beams, max_length] hypotheses, best first per user.  The
        library crops its result to the longest hypothesis of the batch; this one keeps all max_length
        columns (the cropped ones hold the fill token), so nothing waits for the device."""
        seqs, _ = self.generate_scored(input_ids, attention_mask, num_beams)
        return seqs.view(-1, seqs.shape[-1])


def codes_to_tokens(codes, codebook_size):
    """Semantic IDs [..., L] (level l in [0, codebook_size)) -> T5 tokens c + l * codebook_size + 1 (0 is
    the padding token)."""
    if isinstance(codes, torch.Tensor):
        off = torch.arange(codes.shape[-1], device=codes.device, dtype=codes.dtype) * codebook_size
        return codes + off + 1
    codes = np.asarray(codes)
    return codes + np.arange(codes.shape[-1], dtype=codes.dtype) * codebook_size + 1


def collate(histories, targets, max_len, prof_lvl1=None, prof_lvl2=None, prof_lvl3=None):
    """``GenRecDataLoader.collate_fn`` after ``pad_or_truncate``: each history ([n_i, L] tokens) keeps its
    last ``max_len`` items and is left-padded with zero codes, then flattened; the mask is 1 where the
    token is not 0; the flattened targets are right-padded with -100.  -> dict of int64 tensors
    ``history`` [B, max_len * L], ``attention_mask`` and ``target``.  ``prof_lvl1..3`` (the prefix variant,
    RQVAE-T5-prefix/data_vision.py:170-172): per level one (n_vec, bert_dim) array per user, stacked as
    float32 ``prof_lvl1..3`` [B, n_vec, bert_dim]."""
    hs = [np.asarray(h, dtype=np.int64) for h in histories]
    L_ = hs[0].shape[-1]
    hist = np.zeros((len(hs), max_len, L_), np.int64)
    for i, h in enumerate(hs):
        h = h.reshape(-1, L_)[-max_len:]
        if len(h):
            hist[i, max_len - len(h):] = h
    hist = hist.reshape(len(hs), -1)
    ts = [np.asarray(t, dtype=np.int64).reshape(-1) for t in targets]
    width = max(len(t) for t in ts)
    tgt = np.full((len(ts), width), -100, np.int64)
    for i, t in enumerate(ts):
        tgt[i, :len(t)] = t
    out = {"history": torch.from_numpy(hist), "target": torch.from_numpy(tgt),
           "attention_mask": torch.from_numpy((hist != 0).astype(np.int64))}
    for name, prof in (("prof_lvl1", prof_lvl1), ("prof_lvl2", prof_lvl2), ("prof_lvl3", prof_lvl3)):
        if prof is not None:
            out[name] = torch.from_numpy(np.stack([np.asarray(v, dtype=np.float32) for v in prof]))
    return out


def crop_like_library(seqs, eos_id):
    """What the reference's ``evaluate_model`` compares: the library crops ``generate``'s result to the
    longest hypothesis of the batch (a hypothesis ends with its first EOS after the start token, or at
    max_length) and ``evaluate_model`` pads it back with zeros.  seqs [B, k, T] -> the same tensor with 0
    in the columns the library would have cropped; tensor operations only, nothing waits for the device."""
    T = seqs.shape[-1]
    is_eos = seqs[..., 1:] == eos_id
    pos = torch.arange(1, T, device=seqs.device)
    length = torch.where(is_eos, pos, torch.full_like(pos, T - 1)).amin(-1)      # generated tokens per hypothesis
    width = 1 + length.max()
    return torch.where(torch.arange(T, device=seqs.device) < width, seqs, torch.zeros_like(seqs))


def eval_loss(model, test_loader, device):
    """RQVAE-T5/train.py:40-51 (and RQVAE-T5-prefix/train.py:55-76: a batch that carries ``prof_lvl1..3`` passes
    them to the model): eval mode, one teacher-forced forward and one ``loss.item()`` per batch under
    ``torch.no_grad()``, training mode again at the end; the mean over the batches."""
    model.eval()
    total_loss = 0.0
    with torch.no_grad():
        for batch in test_loader:
            args = {k: batch[k].to(device) for k in ("prof_lvl1", "prof_lvl2", "prof_lvl3") if k in batch}
            loss, _ = model(input_ids=batch["history"].to(device), attention_mask=batch["attention_mask"].to(device),
                            labels=batch["target"].to(device), **args)
            total_loss += loss.item()
    model.train()
    return total_loss / len(test_loader)


@torch.no_grad()
def evaluate_model(model, batches, topk_list, beam_size, device=None):
    """RQVAE-T5/utils.py:44-92 (and RQVAE-T5-prefix/utils.py:44-102: a batch that carries ``prof_lvl1..3``
    passes them to the model): one generate per batch at max(max(topk_list), beam_size) beams, the start
    token dropped, hypotheses padded or cut to the label width, the first exact match per user found
    on the device (``gr_beam_hits_i64``; the columns the library would have cropped compare as the zeros
    the reference pads with, ``crop_like_library``), Recall@k and NDCG@k as per-batch means averaged over the
    batches -- the reference's arithmetic on the [B, beams] hit matrix, float for float."""
    recalls = {f"Recall@{k}": [] for k in topk_list}
    ndcgs = {f"NDCG@{k}": [] for k in topk_list}
    beams = max(max(topk_list), beam_size)
    if device is None:
        device = next(model.parameters()).device
    for batch in batches:
        ids = batch["history"].to(device)
        mask = batch["attention_mask"].to(device)
        labels = batch["target"].to(device)
        prof = {}
        if batch.get("prof_lvl1") is not None:      # RQVAE-T5-prefix/utils.py:61-77
            prof = {k: batch[k].to(device) for k in ("prof_lvl1", "prof_lvl2", "prof_lvl3")}
        seqs, _ = model.generate_scored(ids, mask, beams, **prof)
        seqs = crop_like_library(seqs, model.binding().params.eos_id)
        pos = ops.beam_hits(seqs, labels, skip=1).cpu()
        ranks = torch.arange(1, pos.shape[-1] + 1)
        dcg = torch.where(pos, 1.0 / torch.log2(ranks + 1), torch.tensor(0.0, dtype=torch.float))
        for k in topk_list:
            recalls[f"Recall@{k}"].append(pos[:, :k].sum(dim=1).float().mean().item())
            ndcgs[f"NDCG@{k}"].append(dcg[:, :k].sum(dim=1).float().mean().item())
    return ({k: sum(v) / len(v) for k, v in recalls.items()}, {k: sum(v) / len(v) for k, v in ndcgs.items()})
