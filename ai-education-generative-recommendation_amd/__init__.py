"""gr_amd — MI355X (gfx950) implementation of the two data-parallel hot paths of
CatchMan1/AI-education-generative-recommendation:

* RQ-VAE residual-quantization encode  (``RQVAE.get_indices``)  -> ``gr_amd.rqvae``
* SASRec forward / full-catalog scoring (``SASRec.predict``)     -> ``gr_amd.sasrec``

and of the consumer of the semantic IDs, TIGER's T5 encode + beam search (``TIGER.generate``) -> ``gr_amd.tiger``,
and of the dense retriever of ``T5/`` (T5 encoder, pooled unit embedding, cosine top-k) -> ``gr_amd.t5_embed``,
and of the BERT pass that makes the vectors all of them consume (``encode_texts``) -> ``gr_amd.bert_embed``.

The directory name is not a Python identifier; the repository root's ``gr_amd.py`` registers it
under the import name ``gr_amd``.  Kernels live in ``csrc/`` behind the C ABI of include/gr_amd.h
and are loaded from ``lib/libgr_amd.so`` (built by ``build.py``); there is no CPU fallback.
"""
from . import ops  # noqa: F401
from ._lib import LIB_PATH, lib  # noqa: F401
from .rqvae import RQVAE  # noqa: F401
from .sasrec import SASRec  # noqa: F401
from . import tiger  # noqa: F401
from .tiger import TIGER  # noqa: F401
from . import tiger_prefix  # noqa: F401  (its TIGER is the prefix variant: gr_amd.tiger_prefix.TIGER)
from . import t5_embed  # noqa: F401  (its TIGER is the T5/ embedding retriever: gr_amd.t5_embed.TIGER)
from . import bert_embed  # noqa: F401  (the BERT pass that makes the 768-wide vectors: gr_amd.bert_embed.BertEncoder)

__all__ = ["RQVAE", "SASRec", "TIGER", "tiger", "tiger_prefix", "t5_embed", "bert_embed", "ops", "lib", "LIB_PATH"]
