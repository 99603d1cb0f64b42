"""Loading of tests/golden/bert_embed_*.npz (tests/golden/make_golden_bert_embed.py)."""
import functools

import torch

import golden_lib as gl

NAMES = ["bert_embed_main", "bert_embed_types", "bert_embed_h64"]


class Fixture:
    def __init__(self, name):
        sd, out, meta = gl.load(name)
        self.name, self.meta, self.cfg = name, meta, meta["config"]
        self.sd = {k: torch.from_numpy(v) for k, v in sd.items()}
        self.ids = torch.from_numpy(out["input_ids"])
        self.mask = torch.from_numpy(out["attention_mask"])
        self.type_ids = torch.from_numpy(out["token_type_ids"])
        self.hf = dict(hidden=torch.from_numpy(out["hf_hidden"]), mean_no_cls=torch.from_numpy(out["hf_mean_no_cls"]),
                       cls=torch.from_numpy(out["hf_cls"]))
        self.r64 = dict(hidden=torch.from_numpy(out["hidden64"]), mean_no_cls=torch.from_numpy(out["mean_no_cls64"]),
                        cls=torch.from_numpy(out["cls64"]))


@functools.lru_cache(maxsize=None)
def fixture(name):
    return Fixture(name)
