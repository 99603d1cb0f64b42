"""T5 embedding retriever (T5/model.py): a bidirectional T5 encoder over ``[user vector, item vectors...]``
sequences of 768-wide BERT vectors, mean-pooled and projected to one unit vector per user that is
scored against the item catalog by cosine -- inference only, on the gfx950 kernels of csrc/t5_embed.hip.

``TIGER(params)`` takes the reference's dict and holds the reference's parameter tree under the
reference's names (``model.shared.weight``, ``model.encoder.block.0.layer.0.SelfAttention.q.weight``, ...,
``input_proj.weight``, ``output_proj.bias``), so a reference checkpoint loads strictly; it does not import
``transformers``.  Like the reference it never passes ``num_layers`` on: the stack has ``T5Config``'s six
blocks whatever ``params['num_layers']`` says, and the unused ``[32128, d_model]`` token table is there
because every checkpoint holds it.  ``forward`` and ``generate`` are one C call with no host round trip;
the contrastive loss of an evaluation pass is torch arithmetic on the kernel's embedding.  The backward
is not built.

``retrieve`` / ``evaluate_batches`` restate the metric tail of T5/evaluate.py:38-75 (scores through
``gr_linear_f32``, top k through ``gr_topk_f32``), ``collate`` restates ``collate_emb_batch`` on arrays.
Reading the ``.h5`` embedding files stays with the caller.

Every position of every sequence is a row of one of two fixed tables (T5/data_vision.py:119-154), so there is a
second way in that moves no vectors per batch: ``Tables(model, item_embs, user_embs)`` holds the tables and their
``input_proj`` on the device, ``collate_ids`` turns samples into row ids and offsets, ``model.embed_rows`` runs the
encoder on the live rows only and returns ``generate``'s bits, and ``evaluate_ids`` / ``eval_loss_ids`` are the two
loops on top of it.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .tiger import LN_EPS, _Stack

NUM_LAYERS = 6        # T5Config defaults the reference leaves alone (T5/model.py:9-15)
VOCAB = 32128
MAX_K = 64            # gr_topk_f32's list length


class _Encoder(nn.Module):
    """T5EncoderModel's parameter tree: ``shared`` tied to ``encoder.embed_tokens``, then the stack."""

    def __init__(self, cfg):
        super().__init__()
        self.shared = nn.Embedding(VOCAB, cfg["d_model"])
        with torch.no_grad():
            self.shared.weight.normal_(0.0, 1.0)
        self.encoder = _Stack(cfg, self.shared, False)


class TIGER(nn.Module):
    def __init__(self, params):
        super().__init__()
        cfg = dict(d_model=int(params["d_model"]), d_ff=int(params["d_ff"]), num_heads=int(params["num_heads"]),
                   d_kv=int(params["d_kv"]), num_layers=NUM_LAYERS, input_emb_dim=int(params["input_emb_dim"]),
                   target_emb_dim=int(params["target_emb_dim"]), layer_norm_epsilon=LN_EPS,
                   feed_forward_proj=params.get("feed_forward_proj", "relu"))
        ops.t5_embed_check(cfg)
        self.config = cfg
        self.model = _Encoder(cfg)
        self.input_proj = nn.Linear(cfg["input_emb_dim"], cfg["d_model"])
        self.output_proj = nn.Linear(cfg["d_model"], cfg["target_emb_dim"])
        self.cosine_eps = 1e-8
        self.temperature = float(params.get("temperature", 0.07))
        self._binding = None
        self._binding_key = None

    @property
    def n_parameters(self):
        total = sum(p.numel() for p in self.parameters() if p.requires_grad)
        emb = self.model.shared.weight.numel() if self.model.shared.weight.requires_grad else 0
        return (f'#Embedding parameters: {emb}\n#Non-embedding parameters: {total - emb}\n'
                f'#Total trainable parameters: {total}\n')

    def binding(self):
        """The parameters' device-pointer view, rebuilt when a parameter's storage moves."""
        tensors = self.state_dict(keep_vars=True)
        key = tuple(t.data_ptr() for t in tensors.values())
        if self._binding is None or key != self._binding_key:
            self._binding = ops.T5EmbedBinding(self.config, {k: v.detach() for k, v in tensors.items()})
            self._binding_key = key
        return self._binding

    def compute_contrastive_loss(self, pred_emb, target_emb):
        """In-batch InfoNCE, both directions (T5/model.py:33-44)."""
        pred = F.normalize(pred_emb, p=2, dim=1, eps=self.cosine_eps)
        target = F.normalize(target_emb, p=2, dim=1, eps=self.cosine_eps)
        logits = pred @ target.T
        logits = logits / self.temperature
        labels = torch.arange(logits.size(0), device=logits.device)
        return (F.cross_entropy(logits, labels) + F.cross_entropy(logits.T, labels)) / 2.0

    def forward(self, seq_embs, attention_mask=None, target_emb=None):
        """-> (loss or None, pred_emb_norm [B, target_emb_dim]).  The loss is the reference's, evaluated on the
        kernel's unit embedding (the reference normalises the raw projection there: the same vector)."""
        if self.training and torch.is_grad_enabled():
            raise NotImplementedError("the T5 embedding retriever's training (the contrastive backward) is not built: "
                                      "call it under torch.no_grad() or .eval()")
        with torch.no_grad():
            pred = ops.t5_embed(self.binding(), seq_embs, attention_mask)
            loss = self.compute_contrastive_loss(pred, target_emb) if target_emb is not None else None
        return loss, pred

    def generate(self, seq_embs, attention_mask=None, **kwargs):
        return self.forward(seq_embs=seq_embs, attention_mask=attention_mask, target_emb=None)[1]

    @torch.no_grad()
    def embed_rows(self, tables, tokens, offsets):
        """``generate`` on id sequences: ``tokens`` [rows] are rows of ``tables`` (a ``Tables`` of this model), user b
        is tokens[offsets[b]:offsets[b + 1]] -> pred [B, target_emb_dim], the bits ``generate`` returns for the same
        sequences as right-padded vectors.  One C call on the live rows only; nothing is read back."""
        return ops.t5_embed_rows(self.binding(), tables.projected(), tokens, offsets)


class Tables:
    """The two fixed tables every sequence is drawn from (T5/data_vision.py:119-154), on the model's device:
    ``table`` [n_items + n_users, input_emb_dim], item rows first and user rows after, so an item's row is its id
    and ``user_row(user_id) = n_items + user_id - 1``; ``items_normalized``, the L2-normalised catalog ``retrieve``
    scores against; and ``projected()``, ``input_proj`` of ``table``, computed once and kept."""

    def __init__(self, model, item_embs, user_embs=None):
        self.model = model
        dev = model.input_proj.weight.device
        items = torch.as_tensor(item_embs, dtype=torch.float32, device=dev)
        self.n_items = items.shape[0]
        self.n_users = 0
        self.table = items
        if user_embs is not None:
            users = torch.as_tensor(user_embs, dtype=torch.float32, device=dev)
            self.n_users = users.shape[0]
            self.table = torch.cat([items, users], dim=0)
        self.items = self.table[:self.n_items]
        self._projected = None
        self._key = None
        self.projected()                              # refuses a CPU model here, not at the first batch
        self.items_normalized = F.normalize(self.items, p=2, dim=1)

    def user_row(self, user_id):
        return self.n_items + user_id - 1

    def projected(self):
        """``input_proj`` of the table: a snapshot, rebuilt when ``input_proj``'s storage pointer or ``_version``
        changes -- so after an in-place update or a ``load_state_dict`` the next call projects with the new weights."""
        lin = self.model.input_proj
        key = tuple((t.data_ptr(), t._version) for t in (lin.weight, lin.bias))
        if self._projected is None or key != self._key:
            self._projected = ops.t5_embed_project(self.model.binding(), self.table)
            self._key = key
        return self._projected


def collate(batch):
    """``collate_emb_batch`` (T5/train.py:17-35) on arrays: samples with ``seq_embs`` [seq_len, dim], ``seq_len``,
    ``target_emb``, ``target_id``, ``user_id`` -> right-padded float32 ``seq_embs`` [B, max_len, dim], int64
    ``attention_mask``, ``target_emb``, ``target_id``, ``user_id``."""
    lens = [int(b["seq_len"]) for b in batch]
    first = np.asarray(batch[0]["seq_embs"])
    seq = np.zeros((len(batch), max(lens), first.shape[-1]), np.float32)
    mask = np.zeros((len(batch), max(lens)), np.int64)
    for i, (b, n) in enumerate(zip(batch, lens)):
        seq[i, :n] = np.asarray(b["seq_embs"], dtype=np.float32)[:n]
        mask[i, :n] = 1
    return {"seq_embs": torch.from_numpy(seq), "attention_mask": torch.from_numpy(mask),
            "target_emb": torch.from_numpy(np.stack([np.asarray(b["target_emb"], dtype=np.float32) for b in batch])),
            "target_id": torch.tensor([int(b["target_id"]) for b in batch], dtype=torch.long),
            "user_id": torch.tensor([int(b["user_id"]) for b in batch], dtype=torch.long)}


MAX_ROWS = 32         # positions per user


def collate_ids(samples, n_items):
    """The reference's ``__getitem__`` + ``collate_emb_batch`` (T5/data_vision.py:131-154, T5/train.py:17-35)
    without the vectors: samples with ``history`` (item ids), ``user_id``, ``target_id`` -> int64 ``tokens`` [rows]
    (per user its row ``n_items + user_id - 1`` of a ``Tables`` over ``n_items`` items, then the history), ``offsets``
    [B + 1], ``target_id``, ``user_id``.  An empty history (the reference cannot concatenate one either), a
    sequence of more than 32 rows and an empty batch are ValueErrors here, before anything reaches the device."""
    if len(samples) == 0:
        raise ValueError("collate_ids: an empty batch")
    tokens, offsets = [], [0]
    for i, s in enumerate(samples):
        history = [int(t) for t in s["history"]]
        if len(history) == 0:
            raise ValueError(f"collate_ids: sample {i} has an empty history")
        if 1 + len(history) > MAX_ROWS:
            raise ValueError(f"collate_ids: sample {i} has {1 + len(history)} rows (the user's and {len(history)} "
                             f"items); at most {MAX_ROWS} are supported")
        tokens.append(n_items + int(s["user_id"]) - 1)
        tokens.extend(history)
        offsets.append(len(tokens))
    return {"tokens": torch.tensor(tokens, dtype=torch.long), "offsets": torch.tensor(offsets, dtype=torch.long),
            "target_id": torch.tensor([int(s["target_id"]) for s in samples], dtype=torch.long),
            "user_id": torch.tensor([int(s["user_id"]) for s in samples], dtype=torch.long)}


def retrieve(pred, item_embs, k, catalog_normalized=False):
    """T5/evaluate.py:39,52-56: ``pred`` normalised again, the catalog normalised (``catalog_normalized``: it
    already is, as inside a loop), cosine scores through ``gr_linear_f32``, the top ``k`` (<= 64) through
    ``gr_topk_f32``, ties to the lower column -> (values [B, k] descending, ids [B, k] int64)."""
    if not 1 <= k <= MAX_K:
        raise NotImplementedError(f"retrieve: k={k} must be 1..{MAX_K}")
    items = item_embs if catalog_normalized else F.normalize(item_embs, p=2, dim=1)
    scores = ops.linear(F.normalize(pred, p=2, dim=1), items)
    return ops.topk(scores, k)


def batch_metrics(topk_idx, target_id, topk_list):
    """Recall@k and NDCG@k of one batch as 0-d float32 means (T5/evaluate.py:58-67)."""
    out = {}
    match = (topk_idx == target_id.unsqueeze(1))
    for k in topk_list:
        cur = match[:, :k]
        ranks = torch.arange(1, k + 1, device=topk_idx.device).unsqueeze(0)
        out[f"Recall@{k}"] = cur.any(dim=1).float().mean()
        out[f"NDCG@{k}"] = (cur.float() / torch.log2(ranks + 1)).sum(dim=1).mean()
    return out


def average_metrics(per_batch, topk_list):
    """The mean over the batches of the per-batch means (T5/evaluate.py:69-70), in Python floats."""
    rec, nd = {}, {}
    for k in topk_list:
        for name, dst in ((f"Recall@{k}", rec), (f"NDCG@{k}", nd)):
            v = [float(x) for x in torch.stack([m[name] for m in per_batch]).tolist()] if per_batch else []
            dst[name] = sum(v) / len(v) if len(v) > 0 else 0.0
    return rec, nd


@torch.no_grad()
def evaluate_batches(batches, model, item_embs, topk_list, device=None):
    """The metric loop of T5/evaluate.py:38-75 (and T5/train.py:69-97): one forward per batch, the top
    max(topk_list) of the cosine scores against the normalised catalog, Recall@k / NDCG@k as per-batch means
    averaged over the batches.  The per-batch means stay on the device until the end."""
    if device is None:
        device = next(model.parameters()).device
    items = F.normalize(torch.as_tensor(item_embs, dtype=torch.float32, device=device), p=2, dim=1)
    per_batch = []
    for batch in batches:
        _, pred = model(seq_embs=batch["seq_embs"].to(device), attention_mask=batch["attention_mask"].to(device),
                        target_emb=None)
        _, ids = retrieve(pred, items, max(topk_list), catalog_normalized=True)
        per_batch.append(batch_metrics(ids, batch["target_id"].to(device), topk_list))
    return average_metrics(per_batch, topk_list)


@torch.no_grad()
def evaluate_ids(batches, model, tables, topk_list):
    """``evaluate_batches`` on ``collate_ids`` batches: the same loop and the same floats, with only the ids going to
    the device per batch -- the vectors are ``tables``' and the catalog is its ``items_normalized``."""
    device = tables.table.device
    per_batch = []
    for batch in batches:
        pred = model.embed_rows(tables, batch["tokens"].to(device), batch["offsets"].to(device))
        _, ids = retrieve(pred, tables.items_normalized, max(topk_list), catalog_normalized=True)
        per_batch.append(batch_metrics(ids, batch["target_id"].to(device), topk_list))
    return average_metrics(per_batch, topk_list)


@torch.no_grad()
def eval_loss_ids(batches, model, tables):
    """``eval_loss`` (T5/train.py:57-67) on ``collate_ids`` batches: the mean over the batches of the contrastive loss
    of ``forward``, the targets' vectors gathered from ``tables`` on the device.  The per-batch losses stay on the device
    until the end."""
    device = tables.table.device
    losses = []
    for batch in batches:
        pred = model.embed_rows(tables, batch["tokens"].to(device), batch["offsets"].to(device))
        losses.append(model.compute_contrastive_loss(pred, tables.items[batch["target_id"].to(device)]))
    values = [float(v) for v in torch.stack(losses).tolist()] if losses else []
    return sum(values) / len(values) if values else 0.0
