"""What the SASRec training paths share: the g_vec row (csrc/sasrec_train_contract.h) against the
parameters it is sliced by (ops._train_params), and the captured-step protocol (ops._CapturedStep)
under the three graph classes: constructing one leaves no trace of its warm-up."""
import ctypes
import math

import pytest
import torch


@pytest.mark.parametrize("d,mlp,blocks,n", [(8, 8, 1, 1), (48, 100, 2, 33), (128, 256, 8, 256)])
def test_vec_width_is_the_train_params_past_the_tables(d, mlp, blocks, n):
    """gr_sasrec_train_vec_width == the sizes of _train_params' tensors past the two embedding
    tables, plus the n positional rows (CPU: a host-side query, no kernel is launched)."""
    import gr_amd
    from gr_amd import SASRec, _lib as L, ops, synth
    m = SASRec(20, synth.sasrec_params(d, n, blocks, 1, mlp, "cpu"))
    p = L.SasrecParams(d=d, n_blocks=blocks, n_heads=1, mlp=mlp, max_len=n, eps=1e-8, item_rows=21)
    sizes = [math.prod(q.shape) for q in ops._train_params(m)[2:]]
    assert len(sizes) == 12 * blocks + 2
    assert sum(sizes) + n * d == gr_amd.lib().gr_sasrec_train_vec_width(ctypes.byref(p), n)


def _state(opt, module):
    """Every tensor a captured step's warm-up could move."""
    ts = [p for g in opt.param_groups for p in g["params"]]
    ts += [v for p in ts for v in opt.state.get(p, {}).values() if torch.is_tensor(v)]
    ts += [g["lr"] for g in opt.param_groups]
    assert all(torch.is_tensor(t) for t in ts)
    return ts + list(module.buffers())


def _sas_batch(dev, B=4, n=8, items=50):
    g = torch.Generator(device=dev).manual_seed(5)
    seqs = torch.randint(1, items + 1, (B, n), generator=g, device=dev)
    seqs[:, :2] = 0
    targets = torch.roll(seqs, -1, dims=1)
    targets[:, -1] = torch.randint(1, items + 1, (B,), generator=g, device=dev)
    targets[seqs == 0] = 0
    return seqs, targets


@pytest.mark.gpu
def test_graph_constructors_leave_no_trace(dev):
    """B 4, n 8, d 16, one head, one block, mlp 16, 50 items (SasTrainGraph with dropout 0.2, so its
    warm-up steps really move the weights) and the RQ-VAE's smallest fused configuration: after each
    of the three constructors every parameter, optimizer state tensor, tensor learning rate and
    module buffer is torch.equal to its value before; SasTrainGraph's negative-sampler seed is the
    seed passed in.  The optimizers have taken one eager step first, so their state exists and is
    not zero."""
    from gr_amd import ops, synth
    from test_rq_train_gpu import _batches, _model, _opt
    B, n, d, items, J = 4, 8, 16, 50, 1
    seqs, targets = _sas_batch(dev, B, n, items)

    g = torch.Generator(device=dev).manual_seed(1)
    feats = torch.randn(B, n, d, generator=g, device=dev).requires_grad_()
    table = torch.randn(items + 1, d, generator=g, device=dev).requires_grad_()
    before = [t.detach().clone() for t in (feats, table)]
    step = ops.SasTrainStepGraph(feats, table, seqs, targets, items, J, 1e-24, seed=3)
    assert step.graph is not None
    assert all(torch.equal(a, b) for a, b in zip(before, (feats, table)))

    p = synth.sasrec_params(d, n, 1, 1, 16, dev)
    assert p["dropout"] == 0.2
    m = synth.sasrec_model(items, p, dev, seed=7).train()
    opt = torch.optim.Adam(m.parameters(), lr=torch.tensor(1e-3, device=dev), betas=(0.9, 0.98), capturable=True)
    ops.SasTrainGraph(m, opt, seqs, targets, items, J, 1e-24, capture=False).replay()   # one eager step
    before = [t.detach().clone() for t in _state(opt, m)]
    assert len(opt.state) > 0
    step = ops.SasTrainGraph(m, opt, seqs, targets, items, J, 1e-24, seed=21)
    assert step.graph is not None and int(step.seed.item()) == 21
    after = _state(opt, m)
    assert len(after) == len(before) and all(torch.equal(a, b) for a, b in zip(before, after))

    rq = _model(dev, 0.1, False)
    ropt, _ = _opt(rq, dev)
    x = _batches(dev, 1)[0]
    ops.RqTrainGraph(rq, ropt, x.clone(), capture=False).replay()
    before = [t.detach().clone() for t in _state(ropt, rq)]
    assert len(ropt.state) > 0
    step = ops.RqTrainGraph(rq, ropt, x.clone())
    assert step.graph is not None
    after = _state(ropt, rq)
    assert len(after) == len(before) and all(torch.equal(a, b) for a, b in zip(before, after))
    torch.cuda.synchronize()
    ops.check_errors(dev)
