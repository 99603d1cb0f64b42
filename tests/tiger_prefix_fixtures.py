"""Loading of tests/golden/tiger_prefix_*.npz and the restatement runs the TIGER prefix tests share
(computed once per fixture and dtype, then left unchanged)."""
import functools

import torch

import golden_lib as gl
import tiger_prefix_ref as pref

NAMES = ["tiger_prefix_main", "tiger_prefix_bert768", "tiger_prefix_h2_s125"]


class Fixture:
    def __init__(self, name):
        sd, out, meta = gl.load(name)
        self.name, self.meta, self.out = name, meta, out
        self.cfg = meta["config"]
        self.beams, self.T, self.n_vec = meta["num_beams"], meta["max_length"], meta["n_vec"]
        sd = {k: torch.from_numpy(v) for k, v in sd.items()}
        for k in meta["tied"]:
            sd[k] = sd["shared.weight"]
        self.sd = sd                                     # T5 names without "model.", adapters in full
        self.ids = torch.from_numpy(out["input_ids"])
        self.mask = torch.from_numpy(out["attention_mask"])
        self.prof = [torch.from_numpy(out[f"prof_lvl{i}"]) for i in (1, 2, 3)]
        self.labels = torch.from_numpy(out["labels"])
        self.m = float(meta["m"])

    def state_dict(self):
        """The reference's state dict (every key of meta["keys"], tied entries included)."""
        return {k: self.sd[k[len("model."):] if k.startswith("model.") else k].clone() for k, _ in self.meta["keys"]}

    def sd_as(self, dtype):
        return {k: v.to(dtype) for k, v in self.sd.items()}

    def t5(self):
        return {k: v for k, v in self.sd.items() if not k.startswith("adapter_lvl")}

    def adapters(self):
        return {k: v for k, v in self.sd.items() if k.startswith("adapter_lvl")}


@functools.lru_cache(maxsize=None)
def fixture(name):
    return Fixture(name)


@functools.lru_cache(maxsize=None)
def restated(name, dtype):
    """(sequences, scores, width, trace) of the restatement on the fixture's inputs."""
    fx = fixture(name)
    trace = {}
    with torch.no_grad():
        s, c, w = pref.beam_search(fx.cfg, fx.sd_as(dtype), fx.ids, fx.mask, [p.to(dtype) for p in fx.prof], fx.beams,
                                   fx.T, trace=trace, use_cache=fx.meta.get("use_cache", True))
    return s, c, w, trace
