"""Tiled SASRec training kernels (csrc/sasrec_train_tiled.hip, ops._SasTrain) against fp64.

The same comparison as test_sasrec_train_gpu.test_train_edge_shapes_vs_fp64, with its helpers: the
train-mode forward (SASRec/model.py:49-96 as called by SASRec/train.py:131) and the gradient of
every parameter (train.py:161-172) against the float64 CPU restatement on the kernels' own dropout
masks.  Per comparison two errors on the same inputs and masks, both scaled by the fp64 tensor's
largest magnitude and recorded through ``parity_log`` (kind ``sasrec_train_tiled_vs_fp64``):
err_t32 (the restatement in fp32 torch on the CPU vs fp64) and err_kernel (kernels vs fp64).  A
class's tolerance is 4 x its worst err_t32 over the cases, rounded up to one significant digit.

The cases (B, n, max_len, d, H, m, nb, p) are the smallest shapes at which a tiled kernel can go
wrong; "auto" cases lie outside the one-workgroup-per-sequence kernels' envelope, "tiled" cases force
the tiled kernels onto shapes the other kernels take:

    (1, 1, 1, 128, 1, 64, 1, 0.0)      auto   one row, full width
    (2, 64, 64, 72, 3, 100, 2, 0.2)    auto   d just past 64, n inside the old range, head width 24
    (3, 65, 80, 128, 2, 128, 1, 0.2)   auto   n just past one wave of keys, n < max_len
    (2, 70, 70, 65, 5, 9, 2, 0.3)      auto   odd d, head width 13, every k tail
    (3, 33, 40, 96, 4, 200, 1, 0.5)    auto   mlp past 128, p 0.5
    (2, 129, 256, 128, 8, 64, 1, 0.1)  auto   n across 128, eight heads of width 16
    (70, 20, 20, 128, 1, 64, 1, 0.2)   auto   row tiles that span sequences, more rows than parts
    (2, 200, 200, 128, 1, 64, 2, 0.2)  auto   the C5 shape
    (2, 256, 256, 128, 2, 256, 1, 0.1) auto   every limit at once
    (4, 17, 64, 7, 7, 9, 1, 0.5)       tiled  head width 1
    (130, 20, 20, 16, 1, 64, 2, 0.2)   tiled  the other kernels' widest batch case
    (2, 64, 64, 64, 4, 128, 3, 0.1)    tiled  the other kernels' limits

err_t32 is a property of the CPU that runs the restatement (its BLAS sums in its own order), so the
rule is applied to the values of the host that runs the GPU suite, below: worst err_t32 per class
over all twelve cases forward 4.5e-07 (C5 shape) -> 2e-06, embedding-table gradients 7.5e-07 (d 72)
-> 4e-06, weight / bias gradients 8.8e-07 (C5 shape) -> 4e-06.  (On another CPU host the nine auto
cases gave 4.5e-07, 7.6e-07 and 1.04e-06 (70 x 20): 2e-06, 4e-06 and 5e-06; the tighter 4e-06 is kept.)

Measured on an MI355X and its host (worst quantity of each class per case):

    case                                kernels  quantity   err_t32  err_kernel  tolerance
    (1, 1, 1, 128, 1, 64, 1, 0.0)       auto     forward    1.3e-07  2.4e-07     2e-06
    (1, 1, 1, 128, 1, 64, 1, 0.0)       auto     d emb      1.9e-07  2.5e-07     4e-06
    (1, 1, 1, 128, 1, 64, 1, 0.0)       auto     dW, db     4.4e-07  5.1e-07     4e-06
    (2, 64, 64, 72, 3, 100, 2, 0.2)     auto     forward    3.4e-07  3.4e-07     2e-06
    (2, 64, 64, 72, 3, 100, 2, 0.2)     auto     d emb      7.5e-07  5.0e-07     4e-06
    (2, 64, 64, 72, 3, 100, 2, 0.2)     auto     dW, db     5.2e-07  7.0e-07     4e-06
    (3, 65, 80, 128, 2, 128, 1, 0.2)    auto     forward    3.8e-07  4.0e-07     2e-06
    (3, 65, 80, 128, 2, 128, 1, 0.2)    auto     d emb      3.8e-07  4.7e-07     4e-06
    (3, 65, 80, 128, 2, 128, 1, 0.2)    auto     dW, db     7.2e-07  8.2e-07     4e-06
    (2, 70, 70, 65, 5, 9, 2, 0.3)       auto     forward    3.6e-07  4.2e-07     2e-06
    (2, 70, 70, 65, 5, 9, 2, 0.3)       auto     d emb      3.5e-07  4.2e-07     4e-06
    (2, 70, 70, 65, 5, 9, 2, 0.3)       auto     dW, db     5.4e-07  6.0e-07     4e-06
    (3, 33, 40, 96, 4, 200, 1, 0.5)     auto     forward    3.3e-07  2.9e-07     2e-06
    (3, 33, 40, 96, 4, 200, 1, 0.5)     auto     d emb      4.3e-07  5.6e-07     4e-06
    (3, 33, 40, 96, 4, 200, 1, 0.5)     auto     dW, db     5.8e-07  6.2e-07     4e-06
    (2, 129, 256, 128, 8, 64, 1, 0.1)   auto     forward    3.0e-07  2.6e-07     2e-06
    (2, 129, 256, 128, 8, 64, 1, 0.1)   auto     d emb      4.5e-07  3.8e-07     4e-06
    (2, 129, 256, 128, 8, 64, 1, 0.1)   auto     dW, db     5.7e-07  5.9e-07     4e-06
    (70, 20, 20, 128, 1, 64, 1, 0.2)    auto     forward    3.0e-07  3.0e-07     2e-06
    (70, 20, 20, 128, 1, 64, 1, 0.2)    auto     d emb      3.6e-07  3.5e-07     4e-06
    (70, 20, 20, 128, 1, 64, 1, 0.2)    auto     dW, db     7.6e-07  6.9e-07     4e-06
    (2, 200, 200, 128, 1, 64, 2, 0.2)   auto     forward    4.5e-07  3.3e-07     2e-06
    (2, 200, 200, 128, 1, 64, 2, 0.2)   auto     d emb      6.8e-07  5.6e-07     4e-06
    (2, 200, 200, 128, 1, 64, 2, 0.2)   auto     dW, db     8.8e-07  6.0e-07     4e-06
    (2, 256, 256, 128, 2, 256, 1, 0.1)  auto     forward    3.0e-07  3.1e-07     2e-06
    (2, 256, 256, 128, 2, 256, 1, 0.1)  auto     d emb      4.5e-07  6.2e-07     4e-06
    (2, 256, 256, 128, 2, 256, 1, 0.1)  auto     dW, db     6.5e-07  1.1e-06     4e-06
    (4, 17, 64, 7, 7, 9, 1, 0.5)        tiled    forward    3.8e-07  3.3e-07     2e-06
    (4, 17, 64, 7, 7, 9, 1, 0.5)        tiled    d emb      6.0e-07  6.0e-07     4e-06
    (4, 17, 64, 7, 7, 9, 1, 0.5)        tiled    dW, db     7.7e-07  1.3e-06     4e-06
    (130, 20, 20, 16, 1, 64, 2, 0.2)    tiled    forward    4.1e-07  3.4e-07     2e-06
    (130, 20, 20, 16, 1, 64, 2, 0.2)    tiled    d emb      4.0e-07  3.8e-07     4e-06
    (130, 20, 20, 16, 1, 64, 2, 0.2)    tiled    dW, db     5.9e-07  5.6e-07     4e-06
    (2, 64, 64, 64, 4, 128, 3, 0.1)     tiled    forward    3.0e-07  3.2e-07     2e-06
    (2, 64, 64, 64, 4, 128, 3, 0.1)     tiled    d emb      5.7e-07  5.7e-07     4e-06
    (2, 64, 64, 64, 4, 128, 3, 0.1)     tiled    dW, db     7.0e-07  7.1e-07     4e-06
"""
import copy

import pytest
import torch

from test_sasrec_train_gpu import EDGE_SEED, NAMES, _edge_inputs, ref_forward64
from test_sasrec_train_gpu import TOL_DEMB as SEQ_TOL_DEMB, TOL_DW as SEQ_TOL_DW, TOL_OUT as SEQ_TOL_OUT

pytestmark = pytest.mark.gpu

TOL_OUT, TOL_DEMB, TOL_DW = 2e-6, 4e-6, 4e-6   # forward output; embedding-row gradients; weight / bias gradients

CASES = [
    ((1, 1, 1, 128, 1, 64, 1, 0.0), "auto"),
    ((2, 64, 64, 72, 3, 100, 2, 0.2), "auto"),
    ((3, 65, 80, 128, 2, 128, 1, 0.2), "auto"),
    ((2, 70, 70, 65, 5, 9, 2, 0.3), "auto"),
    ((3, 33, 40, 96, 4, 200, 1, 0.5), "auto"),
    ((2, 129, 256, 128, 8, 64, 1, 0.1), "auto"),
    ((70, 20, 20, 128, 1, 64, 1, 0.2), "auto"),
    ((2, 200, 200, 128, 1, 64, 2, 0.2), "auto"),
    ((2, 256, 256, 128, 2, 256, 1, 0.1), "auto"),
    ((4, 17, 64, 7, 7, 9, 1, 0.5), "tiled"),
    ((130, 20, 20, 16, 1, 64, 2, 0.2), "tiled"),
    ((2, 64, 64, 64, 4, 128, 3, 0.1), "tiled"),
]


def _model(items, ps, max_len, d, H, m, nb, p, dev, kernels):
    from gr_amd import ops, synth
    prm = synth.sasrec_params(d, max_len, nb, H, m, dev)
    prm["dropout"] = p
    model = synth.sasrec_model(items, prm, dev, seed=3).train()
    model.train_kernels = kernels
    params = ops._train_params(model)
    with torch.no_grad():
        for t, c in zip(params, ps):
            assert t.shape == c.shape
            t.copy_(c)
    return model, params


def _step(model, params, seqs, up, dev):
    """One forward + backward from EDGE_SEED: (output, gradients); the seed word must advance by one."""
    from gr_amd import ops
    seed = ops.dropout_seed(dev)
    seed.fill_(EDGE_SEED)
    out = model(seqs.to(dev))
    assert int(seed.item()) == EDGE_SEED + 1      # the training kernels ran (the module path draws from torch)
    got = torch.autograd.grad((out * up.to(dev)).sum(), params)
    torch.cuda.synchronize()
    ops.check_errors(dev)
    return out.detach(), got


@pytest.mark.parametrize("case,kernels", CASES, ids=[f"{k}-" + "x".join(str(v) for v in c) for c, k in CASES])
def test_tiled_train_vs_fp64(case, kernels, dev, parity_log):
    from gr_amd import ops
    B, n, max_len, d, H, m, nb, p = case
    items, ps, seqs, up = _edge_inputs(B, n, max_len, d, H, m, nb)
    model, params = _model(items, ps, max_len, d, H, m, nb, p, dev, kernels)
    assert ops.sasrec_train_supported(model, n)
    if kernels == "auto":
        assert not ops.sasrec_train_fits_sequence(model, n)   # so "auto" means the tiled kernels here
    out, got = _step(model, params, seqs, up, dev)
    res = {}
    for dtype in (torch.float64, torch.float32):
        ref, leaves = ref_forward64(ps, seqs, EDGE_SEED, p, H, model.layernorm_eps, dtype)
        res[dtype] = [ref.detach()] + list(torch.autograd.grad((ref * up.to(dtype)).sum(), leaves))
    names = ["forward", "item_emb", "pos_emb"] + [f"blk{k}.{x}" for k in range(nb) for x in NAMES] + ["last.w", "last.b"]
    tols = [TOL_OUT, TOL_DEMB, TOL_DEMB] + [TOL_DW] * (12 * nb + 2)
    bad = []
    for name, tol, a, b32, b in zip(names, tols, [out, *got], res[torch.float32], res[torch.float64]):
        assert a.shape == b.shape, name
        a = a.detach().cpu().double()
        assert bool(torch.isfinite(a).all()), name       # the all-padding sequence included
        scale = max(float(b.abs().max()), 1e-6)
        err_kernel = float((a - b).abs().max()) / scale
        err_t32 = float((b32.double() - b).abs().max()) / scale
        parity_log(kind="sasrec_train_tiled_vs_fp64", case=list(case), kernels=kernels, quantity=name,
                   err_t32=err_t32, err_kernel=err_kernel, tol=tol)
        if not err_kernel <= tol:
            bad.append((name, err_kernel, tol))
    assert not bad, bad
    assert float(got[0][0].abs().max()) == 0.0            # padding row of the item table
    assert got[1].shape[0] == max_len
    assert float(got[1][n:].abs().sum()) == 0.0           # positions the batch does not reach
    if B > 1:
        assert bool(torch.isfinite(out[1]).all())         # the all-padding sequence


def test_tiled_and_sequence_kernels_agree(dev):
    """One shape both kernel sets take, the same seed word (so the same masks): outputs and
    gradients within the sum of the two sets' fp64 tolerances; and a forced set refuses a shape
    outside its envelope instead of falling back."""
    B, n, max_len, d, H, m, nb, p = 4, 33, 50, 48, 3, 100, 2, 0.2
    items, ps, seqs, up = _edge_inputs(B, n, max_len, d, H, m, nb)
    runs = {}
    for kernels in ("sequence", "tiled"):
        model, params = _model(items, ps, max_len, d, H, m, nb, p, dev, kernels)
        runs[kernels] = _step(model, params, seqs, up, dev)
    (out_s, got_s), (out_t, got_t) = runs["sequence"], runs["tiled"]
    tols = [SEQ_TOL_OUT + TOL_OUT] + [SEQ_TOL_DEMB + TOL_DEMB] * 2 + [SEQ_TOL_DW + TOL_DW] * (12 * nb + 2)
    names = ["forward", "item_emb", "pos_emb"] + [f"blk{k}.{x}" for k in range(nb) for x in NAMES] + ["last.w", "last.b"]
    for name, tol, a, b in zip(names, tols, [out_s, *got_s], [out_t, *got_t]):
        scale = max(float(a.abs().max()), 1e-6)
        err = float((a.double() - b.double()).abs().max()) / scale
        assert err <= tol, (name, err, tol)
    items, ps, seqs, up = _edge_inputs(2, 20, 20, 128, 1, 64, 1)
    model, params = _model(items, ps, 20, 128, 1, 64, 1, 0.0, dev, "sequence")
    with pytest.raises(RuntimeError, match="sequence"):
        model(seqs.to(dev))


def test_whole_train_step_graph_at_d128(dev):
    """ops.SasTrainGraph captures the whole step at a shape only the tiled kernels take (d 128, n 70,
    2 blocks): three replays against the same three steps issued eagerly on a copy of the model
    (dropout 0, the same negatives), SGD, every parameter within 1e-5 of its scale as in
    test_train_bce.test_whole_train_step_graph_matches_eager."""
    from gr_amd import ops, synth
    B, n, d, items, J = 8, 70, 128, 300, 5
    p = synth.sasrec_params(d, n, 2, 1, 64, dev)
    p["dropout"] = 0.0
    m = synth.sasrec_model(items, p, dev, seed=7).train()
    ref = copy.deepcopy(m)
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    ref_opt = torch.optim.SGD(ref.parameters(), lr=0.05)
    g = torch.Generator(device=dev).manual_seed(9)
    seqs = torch.randint(1, items + 1, (B, n), generator=g, device=dev)
    seqs[:, :3] = 0
    targets = torch.roll(seqs, -1, dims=1)
    targets[:, -1] = torch.randint(1, items + 1, (B,), generator=g, device=dev)
    targets[seqs == 0] = 0
    step = ops.SasTrainGraph(m, opt, seqs, targets, items, J, 1e-24, seed=21)
    assert step.graph is not None
    for a, b in zip(m.parameters(), ref.parameters()):
        assert torch.equal(a, b)   # the warm-up steps were undone
    for _ in range(3):
        key = int(step.seed.item())
        bl, valid = step.replay()
        negs = ops.neg_samples(seqs, items, J, seed_tensor=torch.tensor([key], dtype=torch.int64, device=dev))
        ref_opt.zero_grad()
        bl2, valid2 = ops.sampled_bce_loss(ref(seqs), ref.item_emb.weight, targets, negs, 1e-24)
        (bl2 / valid2).backward()
        ref_opt.step()
        assert float(valid) == float(valid2)
        assert abs(float(bl) - float(bl2.detach())) <= 1e-5 * abs(float(bl2.detach()))
    with torch.no_grad():
        for (name, a), b in zip(m.named_parameters(), ref.parameters()):
            assert (a - b).abs().max() <= 1e-5 * max(float(b.abs().max()), 1e-6), name
    torch.cuda.synchronize()
    ops.check_errors(dev)
