"""Fused SASRec training kernels (csrc/sasrec_train.hip, ops._SasTrain) against torch autograd.

The reference's train-mode forward (SASRec/model.py:49-96 as called by SASRec/train.py:131) and its
backward (train.py:161-172) are restated functionally in torch fp32 with the kernels' dropout masks
(reproduced here from the same counter-based hash), so the forward output and the gradient of every
parameter can be compared on the same masks: dropout 0 (plain module semantics) and 0.2 (main.py).
fp32 sums run in different orders on the two sides: outputs within 2e-5 and gradients within 2e-4
of their tensor's max magnitude.

test_train_edge_shapes_vs_fp64 compares with the same restatement in fp64 on the CPU
(``ref_forward64``) at the shapes those four cases leave out.  Per comparison two errors on the same
inputs and masks, both scaled by the fp64 tensor's largest magnitude and recorded through
``parity_log``: err_t32 (the restatement in fp32 torch on the CPU vs fp64) and err_kernel (kernels vs
fp64).  A class's tolerance is 4 x its worst err_t32 over all cases (room for the MFMA k order and
the atomic order of the item-table rows), rounded up to one significant digit.  Measured on an
MI355X, cases (B, n, max_len, d, H, m, nb, p):

    case                               quantity   err_t32  err_kernel  tolerance
    (3, 1, 1, 16, 1, 64, 1, 0.0)       forward    8.5e-08  1.2e-07  3e-06
    (3, 1, 1, 16, 1, 64, 1, 0.0)       d emb      1.6e-07  1.0e-07  3e-06
    (3, 1, 1, 16, 1, 64, 1, 0.0)       dW, db     3.3e-07  2.7e-07  4e-06
    (4, 33, 50, 48, 3, 100, 2, 0.2)    forward    2.9e-07  2.9e-07  3e-06
    (4, 33, 50, 48, 3, 100, 2, 0.2)    d emb      4.0e-07  4.4e-07  3e-06
    (4, 33, 50, 48, 3, 100, 2, 0.2)    dW, db     6.3e-07  4.4e-07  4e-06
    (5, 20, 20, 20, 5, 1, 2, 0.2)      forward    6.3e-07  8.0e-07  3e-06
    (5, 20, 20, 20, 5, 1, 2, 0.2)      d emb      5.7e-07  4.6e-07  3e-06
    (5, 20, 20, 20, 5, 1, 2, 0.2)      dW, db     9.0e-07  6.6e-07  4e-06
    (4, 17, 64, 7, 7, 9, 1, 0.5)       forward    3.8e-07  3.3e-07  3e-06
    (4, 17, 64, 7, 7, 9, 1, 0.5)       d emb      6.0e-07  6.1e-07  3e-06
    (4, 17, 64, 7, 7, 9, 1, 0.5)       dW, db     7.7e-07  1.3e-06  4e-06
    (130, 20, 20, 16, 1, 64, 2, 0.2)   forward    4.1e-07  3.4e-07  3e-06
    (130, 20, 20, 16, 1, 64, 2, 0.2)   d emb      4.0e-07  3.7e-07  3e-06
    (130, 20, 20, 16, 1, 64, 2, 0.2)   dW, db     5.9e-07  3.8e-07  4e-06
    (2, 64, 64, 64, 4, 128, 3, 0.1)    forward    3.0e-07  2.8e-07  3e-06
    (2, 64, 64, 64, 4, 128, 3, 0.1)    d emb      5.7e-07  5.4e-07  3e-06
    (2, 64, 64, 64, 4, 128, 3, 0.1)    dW, db     7.0e-07  6.9e-07  4e-06

("d emb": the item and positional table gradients; "dW, db": every other parameter.)  Worst err_t32
per class: forward 6.3e-07 -> 3e-06, d emb 6.0e-07 -> 3e-06, dW / db 9.0e-07 -> 4e-06.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(z):
    z = (z + np.uint64(0x9E3779B97F4A7C15)) & M64
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M64
    return z ^ (z >> np.uint64(31))


def keep_mask(seed, B, site, count, p):
    """The kernels' keep factors (sasrec_train.hip keep()): [B, count] of 0 or 1 / (1 - p)."""
    if p <= 0:
        return np.ones((B, count), np.float32)
    with np.errstate(over="ignore"):
        idx = np.arange(count, dtype=np.uint64)
        key = (np.uint64(site) << np.uint64(32)) | idx
        inner = _mix64(key)[None, :]
        b = np.arange(B, dtype=np.uint64)[:, None]
        z = _mix64(np.uint64(seed) ^ _mix64(b ^ inner))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.where(u >= np.float32(p), np.float32(1.0) / np.float32(1.0 - np.float32(p)), 0).astype(np.float32)


def ref_forward(model, seqs, seed, p):
    """model.py:58-96 in torch ops with explicit dropout masks (the kernels' masks)."""
    B, n = seqs.shape
    d, H, m = model.d, model.num_heads, model.mlp_layer
    hd = d // H
    dev = seqs.device
    mk = lambda site, cnt: torch.from_numpy(keep_mask(seed, B, site, cnt, p)).to(dev)   # noqa: E731
    x = F.embedding(seqs, model.item_emb.weight, padding_idx=0) + model.pos_emb.weight[:n][None]
    causal = torch.ones((n, n), dtype=torch.bool, device=dev).triu(1)
    for k, (la, at, lf, ff) in enumerate(zip(model.attention_layernorms, model.attention_layers,
                                             model.forward_layernorms, model.forward_layers)):
        h = F.layer_norm(x, (d,), la.weight, la.bias, model.layernorm_eps)
        qkv = F.linear(h, at.in_proj_weight, at.in_proj_bias)
        q, kk, v = qkv.split(d, dim=-1)
        q = q.view(B, n, H, hd).transpose(1, 2) * (1.0 / hd) ** 0.5
        kk = kk.view(B, n, H, hd).transpose(1, 2)
        v = v.view(B, n, H, hd).transpose(1, 2)
        s = (q @ kk.transpose(-1, -2)).masked_fill(causal, float("-inf"))
        pr = torch.softmax(s, dim=-1) * mk(3 * k, H * n * n).view(B, H, n, n)
        o = (pr @ v).transpose(1, 2).reshape(B, n, d)
        x = x + F.linear(o, at.out_proj.weight, at.out_proj.bias)
        f = F.layer_norm(x, (d,), lf.weight, lf.bias, model.layernorm_eps)
        u = torch.relu(F.linear(f, ff[0].weight, ff[0].bias)) * mk(3 * k + 1, n * m).view(B, n, m)
        x = x + F.linear(u, ff[3].weight, ff[3].bias) * mk(3 * k + 2, n * d).view(B, n, d)
    return F.layer_norm(x, (d,), model.last_layernorm.weight, model.last_layernorm.bias, model.layernorm_eps)


def _close(a, b, tol, what):
    scale = max(float(b.abs().max()), 1e-6)
    err = float((a - b).abs().max())
    assert err <= tol * scale, f"{what}: max |diff| {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("B,n,d,H,m,nb,p", [
    (6, 20, 16, 1, 64, 2, 0.0),     # main.py's configuration, dropout off
    (6, 20, 16, 1, 64, 2, 0.2),     # main.py's configuration (dropout 0.2)
    (3, 50, 64, 2, 64, 2, 0.2),     # C3 shapes, two heads
    (2, 64, 64, 4, 128, 3, 0.1),    # the kernels' limits: n 64, d 64, mlp 128
])
def test_train_forward_backward_matches_autograd(B, n, d, H, m, nb, p, dev):
    from gr_amd import ops, synth
    prm = synth.sasrec_params(d, n, nb, H, m, dev)
    prm["dropout"] = p
    items = 500
    model = synth.sasrec_model(items, prm, dev, seed=3).train()
    g = torch.Generator(device=dev).manual_seed(5)
    seqs = torch.randint(1, items + 1, (B, n), generator=g, device=dev)
    seqs[0, : n // 2] = 0          # left padding (padding row 0 gets no gradient)
    seqs[-1, 3] = seqs[-1, 5]      # a repeated item (its rows' gradients add)
    params = ops._train_params(model)
    seed = int(ops.dropout_seed(dev).item())
    out = model(seqs)
    assert int(ops.dropout_seed(dev).item()) == seed + 1
    ref = ref_forward(model, seqs, seed, p)
    _close(out.detach(), ref.detach(), 2e-5, "forward")
    upstream = torch.randn(out.shape, generator=g, device=dev)
    got = torch.autograd.grad((out * upstream).sum(), params)
    want = torch.autograd.grad((ref * upstream).sum(), params)
    names = ["item_emb", "pos_emb"] + [f"blk{k}.{x}" for k in range(nb) for x in
                                       ("ln_a.w", "ln_a.b", "in_w", "in_b", "out_w", "out_b", "ln_f.w", "ln_f.b",
                                        "ffn1.w", "ffn1.b", "ffn2.w", "ffn2.b")] + ["last.w", "last.b"]
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape, name
        _close(a, b, 2e-4, name)
    assert float(got[0][0].abs().max()) == 0.0   # padding row
    torch.cuda.synchronize()
    ops.check_errors(dev)


def ref_forward64(params, seqs, seed, p, H, eps, dtype=torch.float64):
    """``ref_forward`` on the CPU in ``dtype`` (float64: the reference; float32: the same
    restatement, whose distance from float64 sizes the tolerances).  ``params``: CPU tensors in the
    order of ops._train_params; returns the output and the leaves the gradients are taken in."""
    P = [t.detach().to(dtype).requires_grad_(True) for t in params]
    B, n = seqs.shape
    d = P[0].shape[1]
    nb = (len(P) - 4) // 12
    hd = d // H
    mk = lambda site, cnt: torch.from_numpy(keep_mask(seed, B, site, cnt, p)).to(dtype)   # noqa: E731
    x = F.embedding(seqs, P[0], padding_idx=0) + P[1][:n][None]
    causal = torch.ones((n, n), dtype=torch.bool).triu(1)
    for k in range(nb):
        la_w, la_b, in_w, in_b, out_w, out_b, lf_w, lf_b, w1, b1, w2, b2 = P[2 + 12 * k: 14 + 12 * k]
        m = w1.shape[0]
        h = F.layer_norm(x, (d,), la_w, la_b, eps)
        q, kk, v = F.linear(h, in_w, in_b).split(d, dim=-1)
        q = q.view(B, n, H, hd).transpose(1, 2) * (1.0 / hd) ** 0.5
        kk = kk.view(B, n, H, hd).transpose(1, 2)
        v = v.view(B, n, H, hd).transpose(1, 2)
        s = (q @ kk.transpose(-1, -2)).masked_fill(causal, float("-inf"))
        pr = torch.softmax(s, dim=-1) * mk(3 * k, H * n * n).view(B, H, n, n)
        o = (pr @ v).transpose(1, 2).reshape(B, n, d)
        x = x + F.linear(o, out_w, out_b)
        f = F.layer_norm(x, (d,), lf_w, lf_b, eps)
        u = torch.relu(F.linear(f, w1, b1)) * mk(3 * k + 1, n * m).view(B, n, m)
        x = x + F.linear(u, w2, b2) * mk(3 * k + 2, n * d).view(B, n, d)
    return F.layer_norm(x, (d,), P[-2], P[-1], eps), P


def _cpu_params(items, max_len, d, H, m, nb, g):
    """Seeded CPU parameters in the order of ops._train_params (padding row 0 of the item table zero)."""
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    item = rn(items + 1, d)
    item[0] = 0
    ps = [item, rn(max_len, d)]
    for _ in range(nb):
        ps += [1 + 0.1 * rn(d), 0.1 * rn(d), rn(3 * d, d) * d ** -0.5, 0.1 * rn(3 * d), rn(d, d) * d ** -0.5,
               0.1 * rn(d), 1 + 0.1 * rn(d), 0.1 * rn(d), rn(m, d) * d ** -0.5, 0.1 * rn(m),
               rn(d, m) * m ** -0.5, 0.1 * rn(d)]
    return ps + [1 + 0.1 * rn(d), 0.1 * rn(d)]


def _edge_inputs(B, n, max_len, d, H, m, nb):
    """(parameters, sequences, upstream gradient) of an edge case, on the CPU.  40 items, so ids
    repeat everywhere; in a multi-row batch sequence 1 is all padding, sequence 0 is left-padded,
    and the last sequence repeats an item within itself and shares it with sequence 0."""
    items = 40
    g = torch.Generator().manual_seed(1000 * B + 10 * n + d)
    ps = _cpu_params(items, max_len, d, H, m, nb, g)
    seqs = torch.randint(1, items + 1, (B, n), generator=g)
    seqs[0, : n // 2] = 0
    if B > 1:
        seqs[1] = 0
        seqs[-1, n // 2] = seqs[-1, n - 1]
        seqs[0, n - 1] = seqs[-1, n - 1]
    up = torch.randn(B, n, d, generator=g)
    return items, ps, seqs, up


NAMES = ("ln_a.w", "ln_a.b", "in_w", "in_b", "out_w", "out_b", "ln_f.w", "ln_f.b", "ffn1.w", "ffn1.b", "ffn2.w",
         "ffn2.b")
TOL_OUT, TOL_DEMB, TOL_DW = 3e-6, 3e-6, 4e-6   # forward output; embedding-row gradients; weight / bias gradients
EDGE_SEED = 0x0F1E2D3C4B5A6978


# (B, n, max_len, d, H, m, nb, p): one row of one position; n 33 (two row tiles of mm) below max_len
# with head width 16; five heads of width 4 and a one-wide FFN; head width 1 (every mm k tail) at
# d 7 and p 0.5; 130 sequences (the [B, V] partial sum); the kernels' limits
@pytest.mark.parametrize("B,n,max_len,d,H,m,nb,p", [
    (3, 1, 1, 16, 1, 64, 1, 0.0),
    (4, 33, 50, 48, 3, 100, 2, 0.2),
    (5, 20, 20, 20, 5, 1, 2, 0.2),
    (4, 17, 64, 7, 7, 9, 1, 0.5),
    (130, 20, 20, 16, 1, 64, 2, 0.2),
    (2, 64, 64, 64, 4, 128, 3, 0.1),
])
def test_train_edge_shapes_vs_fp64(B, n, max_len, d, H, m, nb, p, dev, parity_log):
    """The fused forward and every parameter gradient against fp64 on the kernels' masks, at the
    shapes the four cases above leave out (n < max_len: pos_emb rows n.. get exact zeros)."""
    from gr_amd import ops, synth
    items, ps, seqs, up = _edge_inputs(B, n, max_len, d, H, m, nb)
    prm = synth.sasrec_params(d, max_len, nb, H, m, dev)
    prm["dropout"] = p
    model = synth.sasrec_model(items, prm, dev, seed=3).train()
    params = ops._train_params(model)
    with torch.no_grad():
        for t, c in zip(params, ps):
            assert t.shape == c.shape
            t.copy_(c)
    assert ops.sasrec_train_supported(model, n)
    seed = ops.dropout_seed(dev)
    seed.fill_(EDGE_SEED)
    out = model(seqs.to(dev))
    assert int(seed.item()) == EDGE_SEED + 1
    got = torch.autograd.grad((out * up.to(dev)).sum(), params)
    torch.cuda.synchronize()
    ops.check_errors(dev)
    res = {}
    for dtype in (torch.float64, torch.float32):
        ref, leaves = ref_forward64(ps, seqs, EDGE_SEED, p, H, model.layernorm_eps, dtype)
        res[dtype] = [ref.detach()] + list(torch.autograd.grad((ref * up.to(dtype)).sum(), leaves))
    names = ["forward", "item_emb", "pos_emb"] + [f"blk{k}.{x}" for k in range(nb) for x in NAMES] + ["last.w", "last.b"]
    tols = [TOL_OUT, TOL_DEMB, TOL_DEMB] + [TOL_DW] * (12 * nb + 2)
    bad = []
    for name, tol, a, b32, b in zip(names, tols, [out.detach(), *got], res[torch.float32], res[torch.float64]):
        assert a.shape == b.shape, name
        a = a.detach().cpu().double()
        assert bool(torch.isfinite(a).all()), name       # the all-padding sequence included
        scale = max(float(b.abs().max()), 1e-6)
        err_kernel = float((a - b).abs().max()) / scale
        err_t32 = float((b32.double() - b).abs().max()) / scale
        parity_log(kind="sasrec_train_vs_fp64", case=[B, n, max_len, d, H, m, nb, p], quantity=name,
                   err_t32=err_t32, err_kernel=err_kernel, tol=tol)
        if not err_kernel <= tol:
            bad.append((name, err_kernel, tol))
    assert not bad, bad
    assert float(got[0][0].abs().max()) == 0.0            # padding row of the item table
    assert got[1].shape[0] == max_len
    assert float(got[1][n:].abs().sum()) == 0.0           # positions the batch does not reach
    if B > 1:
        assert bool(torch.isfinite(out[1]).all())         # the all-padding sequence


def test_train_module_path_equivalence(dev):
    """fused_train on vs off (the module-by-module autograd path) at dropout 0."""
    import copy
    from gr_amd import synth
    prm = synth.sasrec_params(32, 30, 2, 1, 64, dev)
    prm["dropout"] = 0.0
    a = synth.sasrec_model(300, prm, dev, seed=4).train()
    b = copy.deepcopy(a)
    b.fused_train = False
    seqs = torch.randint(0, 301, (4, 30), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    ya, yb = a(seqs), b(seqs)
    _close(ya.detach(), yb.detach(), 2e-5, "forward")
    ya.square().sum().backward()
    yb.square().sum().backward()
    for (name, pa), pb in zip(a.named_parameters(), b.parameters()):
        if pb.grad is None:
            assert pa.grad is None, name     # W_Q / W_K / W_V feed nothing (model.py:63-65)
            continue
        _close(pa.grad, pb.grad, 2e-4, name)


def test_train_dropout_rate_and_fresh_masks(dev):
    """Each call draws new masks (the seed word advances) at the configured rate."""
    from gr_amd import synth
    prm = synth.sasrec_params(16, 20, 1, 1, 64, dev)
    prm["dropout"] = 0.2
    model = synth.sasrec_model(100, prm, dev, seed=2).train()
    seqs = torch.randint(1, 101, (8, 20), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    y1, y2 = model(seqs), model(seqs)
    assert not torch.equal(y1, y2)
    km = keep_mask(12345, 64, 1, 20 * 64, 0.2)
    assert abs(float((km == 0).mean()) - 0.2) < 0.01
