"""Loading of tests/golden/tiger_*.npz and the restatement runs the TIGER tests share (computed once per
fixture and dtype, then left unchanged)."""
import functools

import torch

import golden_lib as gl
import tiger_ref

NAMES = ["tiger_main", "tiger_eos", "tiger_h2_ff128", "tiger_v40_len3", "tiger_d32_b5", "tiger_stop"]


class Fixture:
    def __init__(self, name):
        sd, out, meta = gl.load(name)
        self.name, self.meta, self.out = name, meta, out
        self.cfg = meta["config"]
        self.beams, self.T = meta["num_beams"], meta["max_length"]
        sd = {k: torch.from_numpy(v) for k, v in sd.items()}
        for k in meta["tied"]:
            sd[k] = sd["shared.weight"]
        self.sd = sd
        self.ids = torch.from_numpy(out["input_ids"])
        self.mask = torch.from_numpy(out["attention_mask"])
        self.labels = torch.from_numpy(out["labels"])
        self.m = float(meta["m"])

    def state_dict(self, prefix="model."):
        """The reference's state dict (every key of meta["keys"], tied entries included)."""
        return {k: self.sd[k[len(prefix):]].clone() for k, _ in self.meta["keys"]}

    def sd_as(self, dtype):
        return {k: v.to(dtype) for k, v in self.sd.items()}


@functools.lru_cache(maxsize=None)
def fixture(name):
    return Fixture(name)


@functools.lru_cache(maxsize=None)
def restated(name, dtype):
    """(sequences, scores, width, trace) of the restatement on the fixture's inputs."""
    fx = fixture(name)
    trace = {}
    with torch.no_grad():
        s, c, w = tiger_ref.beam_search(fx.cfg, fx.sd_as(dtype), fx.ids, fx.mask, fx.beams, fx.T, trace=trace,
                                        use_cache=fx.meta.get("use_cache", True))
    return s, c, w, trace
