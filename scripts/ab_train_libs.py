#!/usr/bin/env python3
"""A/B of the SASRec training kernels of csrc/sasrec_train.hip (one workgroup per sequence) between
two builds of the library, under the rule and driver of scripts/ab_chain_libs.py: fresh child per
build (GR_AMD_LIB), interleaved repetitions, outputs bitwise the parent's, median device time within
the parent's trimmed spread.

    python scripts/ab_train_libs.py lib/libgr_amd_parent.so lib/libgr_amd.so [repetitions = 10]

Cases: the forward (sas_train_fwd_kernel) and the backward (sas_train_bwd_kernel) with dropout 0.2 at
bench.py's training shape (d 64, n 50, mlp 64, 2 blocks) and at an odd one (d 48, n 33, mlp 100, 2
heads, 3 blocks), batches large enough that the kernels and not the host set the time.  The hash
covers the output and every gradient; every item id occurs once in a batch, so each item-table row
gets one atomic add and the result does not depend on their order.
"""
import hashlib
import json
import os
import sys

import ab_chain_libs


def child(out):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gr_amd import ops, synth
    dev = torch.device("cuda:0")
    res = {}

    def timed(fn):
        for _ in range(5):
            r = fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 20 * 1e3, r

    for name, B, n, d, blocks, heads, mlp in (("d64 n50 mlp64", 1024, 50, 64, 2, 1, 64),
                                               ("d48 n33 mlp100 h2", 512, 33, 48, 3, 2, 100)):
        items = B * n + 7
        torch.manual_seed(0)
        m = synth.sasrec_model(items, synth.sasrec_params(d, n, blocks, heads, mlp, dev), dev, seed=d).train()
        m.train_kernels = "sequence"
        seqs = (torch.randperm(items, device=dev)[:B * n] + 1).view(B, n)
        seqs[:, :2] = 0
        dout = torch.randn(B, n, d, device=dev)
        seed = ops.dropout_seed(dev)

        def fwd():
            seed.fill_(1234)
            return ops.sasrec_train_forward(m, seqs)

        t_f, o = timed(fwd)
        params = ops._train_params(m)
        t_b, grads = timed(lambda: torch.autograd.grad(o, params, dout, retain_graph=True))
        hsh = hashlib.sha256()
        for t in (o, *grads):
            hsh.update(t.detach().contiguous().cpu().numpy().tobytes())
        res[f"train_fwd {name}"] = [t_f, hsh.hexdigest()]
        res[f"train_bwd {name}"] = [t_b, hsh.hexdigest()]
    ops.check_errors(dev)
    with open(out, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    ab_chain_libs.main(child, os.path.abspath(__file__))
