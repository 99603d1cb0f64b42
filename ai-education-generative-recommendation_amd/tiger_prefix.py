"""TIGER's prefix variant (RQVAE-T5-prefix/model.py): the T5 of ``gr_amd.tiger`` plus three
``ProfessionalAdapter`` modules.  Each adapter cross-attends the history's token embeddings to a user's
top-n BERT vectors of one level of the professional hierarchy and yields one prefix token; the three
tokens are prepended to the encoder input and the beam search runs on ``S + 3`` encoder positions --
inference only, as one C call of three launches (csrc/tiger.hip: tiger_adapter_kernel, then the encoder
and search kernels).

``TIGER(config)`` holds the reference's parameter tree under the reference's names (``model.*`` as
``gr_amd.tiger.TIGER``, then ``adapter_lvl1..3.*``), so a prefix checkpoint loads strictly.  The adapters
are built from torch's own modules for their parameters only; their arithmetic runs in the kernel.
``generate`` without all three ``prof_lvl*`` is the plain model's call, as in the reference.  Reading
``prof_lvl*.h5`` is left to the caller (``collate`` takes arrays); ``forward`` with ``labels`` under ``.eval()``
and ``torch.no_grad()`` is the evaluation loss (``eval_loss``: RQVAE-T5-prefix/train.py:55-76), training is not built; the deployed
prefix configuration (d_model 128, d_ff 512, 8 heads of 16) is outside the kernels' envelope and is
refused with that envelope's message.
"""
import torch
import torch.nn as nn

from . import ops, tiger
from .tiger import MAX_LENGTH, codes_to_tokens, collate, crop_like_library, eval_loss, evaluate_model  # noqa: F401

ADAPTER_LN_EPS = 1e-5     # nn.LayerNorm's default, which the reference leaves alone


class ProfessionalAdapter(nn.Module):
    """The parameters of RQVAE-T5-prefix/model.py's adapter, under its names and in its order."""

    def __init__(self, d_model, bert_dim=768, num_heads=4, dropout=0.1):
        super().__init__()
        self.bert_proj = nn.Linear(bert_dim, d_model)
        self.cross_attn = nn.MultiheadAttention(embed_dim=d_model, num_heads=num_heads, dropout=dropout,
                                                batch_first=True)
        self.ffn = nn.Sequential(nn.Linear(d_model, d_model * 4), nn.GELU(), nn.Linear(d_model * 4, d_model))
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)

    def forward(self, student_hidden, bert_vecs):
        raise NotImplementedError("the adapters run inside TIGER.generate (tiger_adapter_kernel); there is no "
                                  "stand-alone or CPU forward")


class TIGER(tiger.TIGER):
    def __init__(self, config):
        super().__init__(config)
        bert_dim = int(config.get("bert_dim", 768))
        ops.tiger_prefix_check(self.config, bert_dim)
        d, heads, drop = int(config["d_model"]), int(config["num_heads"]), float(config["dropout_rate"])
        self.adapter_lvl1 = ProfessionalAdapter(d, bert_dim, heads, drop)
        self.adapter_lvl2 = ProfessionalAdapter(d, bert_dim, heads, drop)
        self.adapter_lvl3 = ProfessionalAdapter(d, bert_dim, heads, drop)
        self._pbinding = None
        self._pbinding_key = None

    def prefix_binding(self):
        """The T5 parameters' and the adapters' device-pointer view, rebuilt when a tensor's storage moves."""
        tensors = dict(self.state_dict(keep_vars=True))
        key = tuple(t.data_ptr() for t in tensors.values())
        if self._pbinding is None or key != self._pbinding_key:
            cfg = dict(self.config, layer_norm_epsilon=self.config.get("layer_norm_epsilon", tiger.LN_EPS))
            t5 = {k[len("model."):]: v.detach() for k, v in tensors.items() if k.startswith("model.")}
            ad = {k: v.detach() for k, v in tensors.items() if k.startswith("adapter_lvl")}
            self._pbinding = ops.TigerPrefixBinding(cfg, t5, ad, ADAPTER_LN_EPS)
            self._pbinding_key = key
        return self._pbinding

    def forward(self, input_ids, attention_mask=None, labels=None, prof_lvl1=None, prof_lvl2=None, prof_lvl3=None):
        """The reference's evaluation call: -> (loss, logits) as ``gr_amd.tiger.TIGER.forward``, on S + 3 encoder
        positions when all three ``prof_lvl*`` are given, else the plain model's call."""
        self._forward_guard(labels)
        if prof_lvl1 is None or prof_lvl2 is None or prof_lvl3 is None:
            return ops.tiger_forward(self.binding(), input_ids, attention_mask, labels)
        return ops.tiger_forward_prefix(self.prefix_binding(), input_ids, attention_mask, prof_lvl1, prof_lvl2,
                                        prof_lvl3, labels)

    @torch.no_grad()
    def generate_scored(self, input_ids, attention_mask=None, num_beams=20, max_length=MAX_LENGTH, prof_lvl1=None,
                        prof_lvl2=None, prof_lvl3=None):
        """-> (sequences [B, num_beams, max_length] int64 best first, scores [B, num_beams] fp32); the plain
        model's result unless all three ``prof_lvl*`` are given."""
        if prof_lvl1 is None or prof_lvl2 is None or prof_lvl3 is None:
            return ops.tiger_generate(self.binding(), input_ids, attention_mask, num_beams, max_length)
        return ops.tiger_generate_prefix(self.prefix_binding(), input_ids, attention_mask, prof_lvl1, prof_lvl2,
                                         prof_lvl3, num_beams, max_length)

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, num_beams=20, prof_lvl1=None, prof_lvl2=None, prof_lvl3=None):
        """The reference's ``generate``: [B * num_beams, max_length] hypotheses, best first per user (never
        cropped, see ``gr_amd.tiger.TIGER.generate``)."""
        seqs, _ = self.generate_scored(input_ids, attention_mask, num_beams, MAX_LENGTH, prof_lvl1, prof_lvl2,
                                       prof_lvl3)
        return seqs.view(-1, seqs.shape[-1])
