"""BERT text encoder (the ``AutoModel.from_pretrained(...)`` pass of T5/item_encode.py, major-encode/bert_emb.py and
Baseline/Rec.py): embeddings, the post-LN encoder stack and the reference's two poolings -- inference only, fp32,
on the gfx950 kernels of csrc/bert_embed.hip; ``embed(..., precision="bf16")`` opts into bf16 GEMM operands with
fp32 accumulation (float32 results; the contract is in include/gr_amd.h).

``BertEncoder(config)`` takes a dict or any object with HF's ``BertConfig`` field names and holds ``BertModel``'s
parameter tree under ``BertModel``'s names (``embeddings.word_embeddings.weight``,
``encoder.layer.0.attention.self.query.weight``, ..., ``pooler.dense.bias``), so the ``state_dict()`` of a model
made by ``AutoModel.from_pretrained`` loads strictly; it does not import ``transformers``.  The pooler is held
because every checkpoint holds it and is never evaluated: the reference reads ``last_hidden_state`` only.

``model(**encoded)`` returns an object with ``.last_hidden_state``; ``model.embed(...)`` returns the pooled
``[B, H]`` vectors in one C call without the hidden state leaving the workspace.  ``encode_texts`` and
``generate_user_profile_embedding`` keep the reference's signatures; the tokenizer (any callable with the HF
call convention) stays on the host.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops

_FIELDS = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "hidden_act",
           "max_position_embeddings", "type_vocab_size", "layer_norm_eps", "position_embedding_type", "pad_token_id")
_DEFAULTS = dict(hidden_act="gelu", layer_norm_eps=1e-12, position_embedding_type="absolute", pad_token_id=0,
                 type_vocab_size=2, max_position_embeddings=512)
_IGNORED_KEYS = ("embeddings.position_ids", "embeddings.token_type_ids")    # buffers of older checkpoints


def _config(config):
    get = config.get if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
    cfg = {}
    for k in _FIELDS:
        v = get(k, None)
        if v is None:
            if k not in _DEFAULTS:
                raise ValueError(f"BertEncoder: the config has no {k}")
            v = _DEFAULTS[k]
        cfg[k] = v
    return cfg


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        H = cfg["hidden_size"]
        self.word_embeddings = nn.Embedding(cfg["vocab_size"], H)
        self.position_embeddings = nn.Embedding(cfg["max_position_embeddings"], H)
        self.token_type_embeddings = nn.Embedding(cfg["type_vocab_size"], H)
        self.LayerNorm = nn.LayerNorm(H, eps=cfg["layer_norm_eps"])


class _SelfAttention(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(H, H), nn.Linear(H, H), nn.Linear(H, H)


class _DenseNorm(nn.Module):
    def __init__(self, n_in, H, eps):
        super().__init__()
        self.dense = nn.Linear(n_in, H)
        self.LayerNorm = nn.LayerNorm(H, eps=eps)


class _Attention(nn.Module):
    def __init__(self, H, eps):
        super().__init__()
        self.add_module("self", _SelfAttention(H))
        self.output = _DenseNorm(H, H, eps)


class _Dense(nn.Module):
    def __init__(self, n_in, n_out):
        super().__init__()
        self.dense = nn.Linear(n_in, n_out)


class _Layer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        H, I, eps = cfg["hidden_size"], cfg["intermediate_size"], cfg["layer_norm_eps"]
        self.attention = _Attention(H, eps)
        self.intermediate = _Dense(H, I)
        self.output = _DenseNorm(I, H, eps)


class _Stack(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList(_Layer(cfg) for _ in range(cfg["num_hidden_layers"]))


class BertOutput:
    """What ``model(**encoded)`` returns: ``.last_hidden_state`` ([B, S, H]; also ``out[0]``).  ``pooler_output`` is
    None: the pooler is not evaluated."""

    def __init__(self, last_hidden_state):
        self.last_hidden_state = last_hidden_state
        self.pooler_output = None

    def __getitem__(self, i):
        return (self.last_hidden_state,)[i]


class BertEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        cfg = _config(config)
        ops.bert_check(cfg)
        self.config = cfg
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Stack(cfg)
        self.pooler = _Dense(cfg["hidden_size"], cfg["hidden_size"])
        self._bindings = {}      # precision -> (key, binding)

    def load_state_dict(self, state_dict, strict=True, **kw):
        """``BertModel``'s state dict, strictly; the ``position_ids`` / ``token_type_ids`` buffers that older
        checkpoints carry are accepted and ignored."""
        sd = {k: v for k, v in state_dict.items() if k not in _IGNORED_KEYS}
        return super().load_state_dict(sd, strict=strict, **kw)

    def _binding_for(self, precision):
        """The precision's binding from the one cache: (key, binding) per precision, rebuilt when the key changes."""
        if precision == "fp16":
            raise ValueError("precision='fp16' is not built: 'fp32' or 'bf16'")
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision={precision!r} must be 'fp32' or 'bf16'")
        tensors = self.state_dict(keep_vars=True)
        if precision == "fp32":
            make, key = ops.BertBinding, tuple(t.data_ptr() for t in tensors.values())
        else:
            make, key = ops.BertBf16Binding, tuple((t.data_ptr(), t._version) for t in tensors.values())
        if self._bindings.get(precision, (None, None))[0] != key:
            self._bindings[precision] = (key, make(self.config, {k: v.detach() for k, v in tensors.items()}))
        return self._bindings[precision][1]

    def binding(self):
        """The parameters' device-pointer view, rebuilt when a parameter's storage moves."""
        return self._binding_for("fp32")

    def binding_bf16(self):
        """The bf16 precision's binding (``ops.BertBf16Binding``: a snapshot of the six matrices per layer rounded to
        bf16), rebuilt when a parameter's storage pointer or its ``_version`` changes -- so after an in-place update
        or a ``load_state_dict`` the next call rounds the new weights."""
        return self._binding_for("bf16")

    def _refuse_training(self):
        if self.training and torch.is_grad_enabled():
            raise NotImplementedError("the BERT encoder's training (its backward) is not built: call it under "
                                      "torch.no_grad() or .eval()")

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, **tokenizer_extras):
        """-> ``BertOutput`` with ``.last_hidden_state`` [B, S, H].  Rows at masked positions are what the encoder
        computes there; a sequence with no live key gives zeros."""
        self._refuse_training()
        if input_ids is None:
            raise ValueError("BertEncoder takes input_ids (inputs_embeds is not built)")
        with torch.no_grad():
            return BertOutput(ops.bert_embed(self.binding(), input_ids, attention_mask, token_type_ids, pooling=None))

    def embed(self, input_ids, attention_mask=None, token_type_ids=None, pooling="mean_no_cls", ragged=False,
              rows_bound=None, precision="fp32"):
        """-> [B, H] in one C call.  ``"mean_no_cls"``: ``(hidden * mask)[:, 1:].sum(1) / mask[:, 1:].sum(-1)
        .clamp(min=1e-9)`` (major-encode/bert_emb.py:160-165), which is T5/item_encode.py:74-75 for every sequence
        with a live token after position 0; a sequence with none returns 0 where item_encode.py's unclamped division
        gives NaN.  ``"cls"``: row 0 of the last hidden state (item_encode.py:28).  A mask entry other than 0
        counts as 1.

        ``ragged=True``: the same bits from the ragged entry, which computes only the rows up to each sequence's last
        live position.  ``rows_bound`` is an upper bound on their count (``row_bound(mask)`` of a host-side mask
        gives it exactly); None means B * S, which is always safe.  Neither form synchronises.

        ``precision="bf16"``: the opt-in bf16 precision -- bf16 GEMM operands with fp32 accumulation, fp32 epilogues,
        LayerNorms, softmax and pooling, a float32 result (the contract is in include/gr_amd.h); ``"fp32"``, the
        default, is the call as it always was.  ``forward`` is fp32 only."""
        self._refuse_training()
        if pooling not in ("mean_no_cls", "cls"):
            raise ValueError(f"pooling={pooling!r} must be 'mean_no_cls' or 'cls'")
        with torch.no_grad():
            binding = self._binding_for(precision)             # ValueError, naming the argument, for any other string
            if ragged:
                return ops.bert_embed_ragged(binding, input_ids, attention_mask, token_type_ids, pooling=pooling,
                                             rows_bound=rows_bound)
            return ops.bert_embed(binding, input_ids, attention_mask, token_type_ids, pooling=pooling)


def row_bound(attention_mask, S=None):
    """The packed row count of the ragged entry for ``attention_mask`` [B, S]: the sum over the sequences of one past
    the last live position (0 for a sequence with no live key) -- exact for a mask on the host.  A mask on a device
    is not read (that would synchronise): the answer is B * S, the bound that is always safe.  None (all live) gives
    None, which ``embed`` and ``ops.bert_embed_ragged`` read as B * S.  ``S``: the padded width when it is not the
    mask's own (a mask wider than the ids)."""
    if attention_mask is None:
        return None
    B, width = attention_mask.shape
    S = width if S is None else int(S)
    if attention_mask.is_cuda:
        return B * S
    live = attention_mask[:, :S] != 0
    last = torch.arange(1, live.shape[1] + 1)[None, :] * live
    return int(last.max(dim=1).values.sum()) if live.numel() else 0


def _tokenize(tokenizer, texts, max_length, device):
    """-> (the encoded batch on ``device``, the ragged entry's row bound taken from the mask where the tokenizer left
    it: exact on the host, B * S on a device)."""
    encoded = tokenizer(list(texts), padding=True, truncation=True, max_length=max_length, return_tensors="pt")
    mask = encoded.get("attention_mask")
    B, S = encoded["input_ids"].shape
    bound = B * S if mask is None else row_bound(mask, S)
    if hasattr(encoded, "to"):
        return encoded.to(device), bound
    return {k: v.to(device) for k, v in encoded.items()}, bound


def _embed_encoded(model, encoded, pooling, bound, ragged, precision="fp32"):
    """The ragged entry when it has rows to leave out, the padded one otherwise: the same bits from both."""
    ids = encoded["input_ids"]
    ragged = ragged and bound < ids.shape[0] * ids.shape[1]
    return model.embed(ids, encoded.get("attention_mask"), encoded.get("token_type_ids"), pooling=pooling,
                       ragged=ragged, rows_bound=bound if ragged else None, precision=precision)


@torch.no_grad()
def encode_texts(texts, tokenizer, model, device, batch_size, max_length, *, ragged=True, precision="fp32"):
    """The item pass (T5/item_encode.py:59-78, major-encode/bert_emb.py:131-168): batches of ``batch_size`` texts,
    tokenized with padding to the batch's longest and truncation at ``max_length``, mean-pooled without [CLS] ->
    float32 array [len(texts), H].  A text with no live token after position 0 gives a zero row.  ``ragged``: batches
    with padding go through the ragged entry with the row count taken from the tokenizer's host-side mask (the same
    bits, less work); False keeps every batch on the padded entry.  ``precision``: ``embed``'s."""
    model.eval()
    device = torch.device(device)
    embs = []
    for start in range(0, len(texts), batch_size):
        encoded, bound = _tokenize(tokenizer, texts[start:start + batch_size], max_length, device)
        embs.append(_embed_encoded(model, encoded, "mean_no_cls", bound, ragged, precision))
    if not embs:
        return np.zeros((0, model.config["hidden_size"]), np.float32)
    return torch.cat(embs, dim=0).cpu().numpy().astype(np.float32)


@torch.no_grad()
def generate_user_profile_embedding(user_profile_map, tokenizer, model, *, ragged=True, precision="fp32"):
    """The profile pass (T5/item_encode.py:11-34): users in sorted order, batches of 32, 64 tokens at most, the
    [CLS] row -> {user id: float32 vector [H]}.  Runs on the model's device.  ``ragged``, ``precision``: as in
    ``encode_texts``."""
    device = next(model.parameters()).device
    users = sorted(user_profile_map.items(), key=lambda kv: kv[0])
    out = {}
    for start in range(0, len(users), 32):
        batch = users[start:start + 32]
        encoded, bound = _tokenize(tokenizer, [name for _, name in batch], 64, device)
        vecs = _embed_encoded(model, encoded, "cls", bound, ragged, precision).cpu().numpy()
        for (uid, _), v in zip(batch, vecs):
            out[uid] = v
    return out
