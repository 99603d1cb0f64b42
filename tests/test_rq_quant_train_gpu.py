"""The fused quantizer's training forward and backward (csrc/rq_sk.hip: gr_rq_quantize_sk_train_f32,
rq_sk_bwd_dz_kernel, rq_sk_bwd_dc_kernel, through ops.rq_quantize_train) against plain fp64.

ResidualVectorQuantizer.forward under autograd (RQ-VAE/models/rq.py:39-56 with vq.py:86-99 per
level) is restated in torch on the CPU, given the assignment ``idx``:

    x_q_l   = C_l[idx_l]
    loss_l  = mse(x_q_l, r_l.detach()) + beta * mse(x_q_l.detach(), r_l)
    x_res_l = r_l + (x_q_l - r_l).detach();  r_{l+1} = r_l - x_res_l;  x_q = sum_l x_res_l
    rq_loss = mean_l loss_l

Inputs are built so the assignment is not in question: z = sum_l C_l[chosen_l] + noise with codebook
scales shrinking per level (1, 0.3, 0.1, 0.03) and noise well below the last level's code spacing
(``_noise_scale``), so on every argmin level the fp64 argmin of the residual chain is ``chosen`` by
a wide margin (asserted) and the kernel's indices must equal it.  On Sinkhorn levels the kernel's assignment is taken as given
(tests/test_rq_sk_gpu.py owns it).  Shapes: unequal K per level (the backward's level walk), e not
32, one and four levels, one row, codes no row selects (their gradient rows must be exactly 0).
Three losses per case: x_q and rq_loss together, rq_loss alone (no x_q gradient reaches the
backward) and x_q alone (no rq_loss gradient).

Tolerances: per comparison err_t32 (the same restatement in fp32 torch on the CPU vs fp64) and
err_kernel (kernels vs fp64), both scaled by the fp64 tensor's largest magnitude and recorded through
``parity_log``; a class's tolerance is 4 x its worst err_t32 over all cases, rounded up to one
significant digit, and never looser than the 1e-6 (outputs, losses) / 1e-5 (gradients) of
tests/test_rq_train_gpu.py.  Measured on an MI355X (worst over the three losses):

    n, e, Ks, sk_eps                          quantity   err_t32  err_kernel  tolerance
    200 32 [8, 256, 64] [0, 0, 0]             x_q, loss  6.2e-08  1.8e-07  6e-07
    200 32 [8, 256, 64] [0, 0, 0]             dz         9.0e-08  7.6e-08  5e-07
    200 32 [8, 256, 64] [0, 0, 0]             dC         6.9e-07  7.0e-07  9e-06
    33 5 [1, 5, 1024] [0, 0, 0]               x_q, loss  5.7e-08  5.7e-08  6e-07
    33 5 [1, 5, 1024] [0, 0, 0]               dz         7.7e-08  8.8e-08  5e-07
    33 5 [1, 5, 1024] [0, 0, 0]               dC         2.2e-06  2.3e-06  9e-06
    1 48 [16] [0]                             x_q, loss  2.5e-08  2.5e-08  6e-07
    1 48 [16] [0]                             dz         6.2e-08  6.2e-08  5e-07
    1 48 [16] [0]                             dC         6.2e-08  6.2e-08  9e-06
    64 64 [8, 8, 8, 8] [0.01, 0, 0.01, 0]     x_q, loss  1.4e-07  1.4e-07  6e-07
    64 64 [8, 8, 8, 8] [0.01, 0, 0.01, 0]     dz         3.5e-08  3.5e-08  5e-07
    64 64 [8, 8, 8, 8] [0.01, 0, 0.01, 0]     dC         1.5e-06  1.5e-06  9e-06
    130 32 [256, 8, 64] [0.01, 0.01, 0.01]    x_q, loss  6.4e-08  6.2e-08  6e-07
    130 32 [256, 8, 64] [0.01, 0.01, 0.01]    dz         1.1e-07  9.8e-08  5e-07
    130 32 [256, 8, 64] [0.01, 0.01, 0.01]    dC         8.7e-07  8.7e-07  9e-06

Worst err_t32 per class: x_q / rq_loss 1.35e-07 -> 6e-07, dz 1.12e-07 -> 5e-07, dC 2.23e-06 -> 9e-06
(the last level's dC is a sum of code - residual ~ noise, and the residual carries the rounding of
|z|: fp32 itself is that far from fp64 there).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BETA = 0.25
SCALES = [1.0, 0.3, 0.1, 0.03]
TOL_OUT, TOL_DZ, TOL_DC = 6e-7, 5e-7, 9e-6   # x_q and rq_loss, dz, every dC_l

# (n, e, Ks, sk_eps)
CASES = [(200, 32, [8, 256, 64], [0.0, 0.0, 0.0]),
         (33, 5, [1, 5, 1024], [0.0, 0.0, 0.0]),
         (1, 48, [16], [0.0]),
         (64, 64, [8, 8, 8, 8], [0.01, 0.0, 0.01, 0.0]),
         (130, 32, [256, 8, 64], [0.01, 0.01, 0.01])]
_INPUTS = {}


def _noise_scale(c, chosen, scale):
    """Per-element noise: 0.3 x the last level's code scale, and a noise vector no longer than ~0.15
    x the distance from a chosen last-level code to its nearest other code (1024 codes in 5
    dimensions sit close).  Not smaller than that: the last level's codebook gradient is a sum of
    (code - residual) ~ noise, and the residual carries the fp32 rounding of |z| ~ 3, so the fp32
    error of that gradient is ~1e-7 / noise of its magnitude whatever computes it."""
    s = 0.3 * scale
    if c.shape[0] > 1:
        d = torch.cdist(c[chosen].double(), c.double())
        d[torch.arange(len(chosen)), chosen] = float("inf")
        s = min(s, 0.15 * float(d.min()) / c.shape[1] ** 0.5)
    return s


def _inputs(n, e, Ks, sk_eps):
    """(z, codebooks, chosen, upstream) of a case, on the CPU, built once.  On Sinkhorn levels
    ``chosen`` is balanced over the codes (row b takes code perm[b] % K), the assignment Sinkhorn's
    equal column sums ask for."""
    key = (n, e, tuple(Ks))
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(100 * n + e)
        cbs = [s * torch.randn(K, e, generator=g) for K, s in zip(Ks, SCALES)]
        chosen = []
        for K, eps in zip(Ks, sk_eps):
            if eps > 0:
                chosen.append(torch.randperm(n, generator=g) % K)
            else:
                chosen.append(torch.randint(0, K, (n,), generator=g))
        chosen = torch.stack(chosen, 1)
        z = sum(c[chosen[:, l]] for l, c in enumerate(cbs))
        z = z + _noise_scale(cbs[-1], chosen[:, -1], SCALES[len(Ks) - 1]) * torch.randn(n, e, generator=g)
        up = torch.randn(n, e, generator=g)
        _INPUTS[key] = (z, cbs, chosen, up)
    return _INPUTS[key]


def _argmin_chain(z, cbs, idx, sk_eps):
    """fp64 residual chain: per argmin level the nearest code and its margin (second-smallest minus
    smallest squared distance, over |r|^2 + max |c|^2); Sinkhorn levels follow ``idx``."""
    r = z.double()
    out = []
    for l, c in enumerate(cbs):
        c = c.double()
        if sk_eps[l] > 0:
            pick = idx[:, l]
            out.append((None, None))
        else:
            d = (r * r).sum(1, keepdim=True) + (c * c).sum(1)[None] - 2.0 * r @ c.t()
            pick = d.argmin(1)
            if c.shape[0] > 1:
                two = d.topk(2, dim=1, largest=False).values
                margin = (two[:, 1] - two[:, 0]) / ((r * r).sum(1) + (c * c).sum(1).max())
            else:
                margin = torch.ones(r.shape[0], dtype=torch.float64)
            out.append((pick, margin))
        r = r - c[pick]
    return out


def _restate(z, cbs, idx, up, form, dtype):
    """(x_q, rq_loss, dz, [dC_l]) of rq.py:39-56 / vq.py:86-99 given ``idx``, autograd in ``dtype``."""
    z = z.detach().to(dtype, copy=True).requires_grad_(True)     # copies: the shared inputs stay unchanged
    cbs = [c.detach().to(dtype, copy=True).requires_grad_(True) for c in cbs]
    x_q, residual, losses = 0, z, []
    for l, c in enumerate(cbs):
        xq = F.embedding(idx[:, l], c)
        commitment_loss = F.mse_loss(xq.detach(), residual)
        codebook_loss = F.mse_loss(xq, residual.detach())
        losses.append(codebook_loss + BETA * commitment_loss)
        xq = residual + (xq - residual).detach()
        residual = residual - xq
        x_q = x_q + xq
    rq_loss = torch.stack(losses).mean()
    grads = torch.autograd.grad(_loss(x_q, rq_loss, up.to(dtype), form), [z, *cbs], allow_unused=True)
    grads = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, [z, *cbs])]
    return x_q.detach(), rq_loss.detach(), grads[0], grads[1:]


def _loss(x_q, rq_loss, up, form):
    if form == "both":
        return (x_q * up).sum() + rq_loss
    if form == "rq_loss":
        return rq_loss
    return (x_q * up).sum()


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("form", ["both", "rq_loss", "x_q"])
@pytest.mark.parametrize("n,e,Ks,sk_eps", CASES)
def test_rq_quantize_train_vs_fp64(n, e, Ks, sk_eps, form, dev, parity_log):
    from gr_amd import ops
    z, cbs, chosen, up = _inputs(n, e, Ks, sk_eps)
    zg = z.to(dev).requires_grad_(True)
    cg = [c.to(dev).requires_grad_(True) for c in cbs]
    x_q, rq_loss, idx = ops.rq_quantize_train(zg, cg, BETA, sk_eps, 50)
    _loss(x_q, rq_loss, up.to(dev), form).backward()
    idx = idx.cpu()
    assert idx.shape == (n, len(Ks)) and idx.dtype == torch.int64
    for l, (pick, margin) in enumerate(_argmin_chain(z, cbs, idx, sk_eps)):
        assert int(idx[:, l].min()) >= 0 and int(idx[:, l].max()) < Ks[l]
        if pick is not None:
            assert torch.equal(pick, chosen[:, l]) and float(margin.min()) > 1e-3, (l, float(margin.min()))
            assert torch.equal(idx[:, l], chosen[:, l]), l
    ref = _restate(z, cbs, idx, up, form, torch.float64)
    t32 = _restate(z, cbs, idx, up, form, torch.float32)
    dz = zg.grad if zg.grad is not None else torch.zeros_like(zg)
    dcs = [c.grad if c.grad is not None else torch.zeros_like(c) for c in cg]
    got = (x_q.detach(), rq_loss.detach(), dz, dcs)
    flat = lambda r: [("x_q", TOL_OUT, r[0]), ("rq_loss", TOL_OUT, r[1]), ("dz", TOL_DZ, r[2])] + \
        [(f"dC{l}", TOL_DC, t) for l, t in enumerate(r[3])]   # noqa: E731
    bad = []
    for (name, tol, a), (_, _, b32), (_, _, b) in zip(flat(got), flat(t32), flat(ref)):
        assert a.shape == b.shape, name
        err_kernel = _rel(a.detach().cpu().double(), b)
        err_t32 = _rel(b32.double(), b)
        parity_log(kind="rq_quant_train_vs_fp64", n=n, e=e, Ks=Ks, sk_eps=sk_eps, form=form, quantity=name,
                   err_t32=err_t32, err_kernel=err_kernel, tol=tol)
        if not err_kernel <= tol:
            bad.append((name, err_kernel, tol))
    assert not bad, bad
    for l, dc in enumerate(dcs):   # a code no row selects has no gradient at all
        absent = torch.ones(Ks[l], dtype=torch.bool)
        absent[idx[:, l]] = False
        assert float(dc.detach().cpu()[absent].abs().sum()) == 0.0, l
    if form == "x_q":              # no rq_loss gradient: every codebook gradient is exactly 0
        assert all(float(dc.abs().max()) == 0.0 for dc in dcs)
