"""Fixtures for the TIGER teacher-forced forward tests: the reference's own ``TIGER.forward`` (RQVAE-T5/model.py
and RQVAE-T5-prefix/model.py, imported at run time from a checkout of the reference; needs ``transformers``)
in eval mode under ``torch.no_grad()``, on the weights and inputs of existing fixtures, next to the plain-torch
restatement tests/tiger_forward_ref.py in float32 and float64.

    python tests/golden/make_golden_tiger_forward.py <reference checkout>   ->  tests/golden/tiger_fwd_*.npz

No weights are stored: ``tiger_fwd_<source>.npz`` goes with ``<source>.npz``.  Each file holds the labels (the
source fixture's labels with a fixed -100 pattern: user 0 loses its last label, user 1 keeps only its first,
user 2 is ignored entirely, user 3 has -100 at position 1 followed by real labels), the reference's float32
``loss`` and ``logits``, the float64 restatement's ``loss``, ``logits`` and ``nll``, and in ``meta`` the reference's
own distances from float64 that set the GPU tolerances: ``logit_err32`` (per row, scaled by the row's largest
|logit|) and ``nll_err32`` (absolute, over the counted positions).

Before a file is written the generator asserts that the restatement in float32 equals the reference: logits
within 1e-5 row-scaled, loss within 1e-6 relative.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_tiger as base  # noqa: E402  (puts tests/ on the path)
import make_golden_tiger_prefix as pbase  # noqa: E402
import tiger_fixtures as tf  # noqa: E402
import tiger_forward_ref as fref  # noqa: E402
import tiger_prefix_fixtures as tpf  # noqa: E402

PLAIN = ["tiger_main", "tiger_d32_b5", "tiger_v40_len3", "tiger_eos", "tiger_h2_ff128"]
PREFIX = ["tiger_prefix_main", "tiger_prefix_bert768", "tiger_prefix_h2_s125"]


def holed(labels):
    """The fixed -100 pattern on a copy of the source fixture's labels."""
    out = labels.clone()
    out[0, -1] = -100
    out[1, 1:] = -100
    out[2, :] = -100
    out[3, 1] = -100
    return out


def row_scaled(a, b):
    """max over rows of |a - b| / max|b| of the row."""
    return ((a.double() - b.double()).abs().amax(-1) / b.double().abs().amax(-1)).max().item()


def make(name, prefixed, model_cls):
    fx = (tpf if prefixed else tf).fixture(name)
    model = model_cls(fx.cfg).eval()
    model.load_state_dict(fx.state_dict())
    labels = holed(fx.labels)
    prof = fx.prof if prefixed else None
    kw = dict(prof_lvl1=prof[0], prof_lvl2=prof[1], prof_lvl3=prof[2]) if prefixed else {}
    with torch.no_grad():
        loss_ref, logits_ref = model(input_ids=fx.ids, attention_mask=fx.mask, labels=labels, **kw)
    assert loss_ref.dtype == logits_ref.dtype == torch.float32

    def restate(dtype):
        sd = fx.sd_as(dtype)
        if prefixed:
            return fref.forward_prefix(fx.cfg, sd, fx.ids, fx.mask, [p.to(dtype) for p in prof], labels)
        return fref.forward(fx.cfg, sd, fx.ids, fx.mask, labels)

    loss32, logits32, _ = restate(torch.float32)
    loss64, logits64, nll64 = restate(torch.float64)
    d_logit, d_loss = row_scaled(logits32, logits_ref), abs(loss32.item() - loss_ref.item()) / abs(loss_ref.item())
    assert d_logit <= 1e-5, f"{name}: float32 restatement logits differ from the reference by {d_logit}"
    assert d_loss <= 1e-6, f"{name}: float32 restatement loss differs from the reference by {d_loss}"
    counted = labels != -100
    nll_ref = -torch.log_softmax(logits_ref, -1).gather(-1, labels.clamp(min=0)[..., None])[..., 0]
    logit_err32 = row_scaled(logits_ref, logits64)
    nll_err32 = (nll_ref.double() - nll64)[counted].abs().max().item()
    print(f"{name}: labels {tuple(labels.shape)}, {int(counted.sum())} counted; loss {loss_ref.item():.7f} "
          f"(fp64 {loss64.item():.9f}); restatement32 vs reference: logits {d_logit:.2e}, loss {d_loss:.2e}; "
          f"reference vs fp64: logit_err32 {logit_err32:.3e}, nll_err32 {nll_err32:.3e}")
    import transformers
    meta = dict(name="tiger_fwd_" + name, source=name, prefixed=prefixed, logit_err32=logit_err32, nll_err32=nll_err32,
                counted=int(counted.sum()), torch=torch.__version__, transformers=transformers.__version__)
    out = {"meta": np.array(json.dumps(meta)), "labels": labels.numpy(), "loss": loss_ref.numpy(),
           "logits": logits_ref.numpy(), "loss64": loss64.numpy(), "logits64": logits64.numpy(), "nll64": nll64.numpy()}
    path = os.path.join(HERE, f"tiger_fwd_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{name}: wrote {size} bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    ref = sys.argv[1]
    only = sys.argv[2:]
    plain_cls = base.load_reference(ref)
    prefix_cls = pbase.load_reference(ref)[0].TIGER
    for nm in PLAIN:
        if not only or nm in only:
            make(nm, False, plain_cls)
    for nm in PREFIX:
        if not only or nm in only:
            make(nm, True, prefix_cls)
