"""The fused MLP training kernels (csrc/rq_mlp_train.hip, ops.mlp_train) against torch autograd.

MLPLayers in train mode (RQ-VAE/models/layers.py:18-43) is [Dropout -> Linear -> ReLU] x (L - 1),
then Dropout -> Linear.  With dropout 0 the fused forward and backward must match the torch modules'
(fp32 sums in other orders: outputs within 1e-5 and gradients within 2e-5 of their tensor's largest
magnitude).  With dropout on, the kernels draw their own masks (a counter-based hash of the device
seed word, not torch's stream); ``keep_mask`` restates that hash in numpy and is tied to the kernels
element for element (identity-weight probes expose the masks of site 0 and site 1), and the fused
forward and gradients of multi-layer MLPs must equal a plain fp64 restatement on those same masks:

    x_{i+1} = relu(drop_i(x_i) W_i^T + b_i),  no ReLU after the last layer,
    drop_i = keep_mask(seed word, site i, M, K = dims[i], p)

Tolerances of the fp64 comparisons (test_fused_mlp_*_vs_fp64): per comparison two errors on the same
inputs and masks, both scaled by the fp64 tensor's largest magnitude -- err_t32 (the same
restatement in fp32 torch on the CPU vs fp64) and err_kernel (kernels vs fp64) -- recorded through
``parity_log``.  The tolerance of a quantity class is 4 x the worst err_t32 of the class over all
cases (fp32 sums in another order: the MFMA k split), rounded up to one significant digit, and never
looser than the 1e-5 / 2e-5 above.  Measured on an MI355X (worst over p in {0, 0.1, 0.5}):

    dims, M                            quantity   err_t32  err_kernel  tolerance
    [768, 256, 128, 32] M 64           y          4.8e-07  3.4e-07  2e-06
    [768, 256, 128, 32] M 64           dX         3.1e-07  2.2e-07  2e-06
    [768, 256, 128, 32] M 64           dW, db     3.5e-07  3.4e-07  2e-06
    [32, 128, 256, 768] M 64           y          2.5e-07  2.0e-07  2e-06
    [32, 128, 256, 768] M 64           dX         4.0e-07  3.6e-07  2e-06
    [32, 128, 256, 768] M 64           dW, db     3.9e-07  3.5e-07  2e-06
    [30, 33, 7, 1] M 33                y          2.8e-07  3.2e-07  2e-06
    [30, 33, 7, 1] M 33                dX         1.6e-07  2.4e-07  2e-06
    [30, 33, 7, 1] M 33                dW, db     2.6e-07  2.6e-07  2e-06
    [5, 3] M 1                         y          7.3e-08  4.4e-08  2e-06
    [5, 3] M 1                         dX         1.2e-07  9.0e-08  2e-06
    [5, 3] M 1                         dW, db     3.3e-08  3.3e-08  2e-06
    [70, 129, 40] M 129                y          2.2e-07  1.5e-07  2e-06
    [70, 129, 40] M 129                dX         3.2e-07  1.8e-07  2e-06
    [70, 129, 40] M 129                dW, db     3.6e-07  2.8e-07  2e-06
    [770, 64, 32] M 31                 y          2.6e-07  2.7e-07  2e-06
    [770, 64, 32] M 31                 dX         2.3e-07  1.8e-07  2e-06
    [770, 64, 32] M 31                 dW, db     3.2e-07  3.8e-07  2e-06

Worst err_t32 per class: y 4.8e-07, dX 4.0e-07, dW / db 3.9e-07; 4 x each rounds up to 2e-06.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
TOL_OUT, TOL_DX, TOL_DW = 2e-6, 2e-6, 2e-6   # outputs, activation gradients, weight / bias gradients


def _mix64(z):
    z = (z + np.uint64(0x9E3779B97F4A7C15)) & M64
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M64
    return z ^ (z >> np.uint64(31))


def keep_mask(seed, site, M, K, p):
    """The kernels' keep factors of a layer input [M, K] (rq_mlp_train.hip Drop::keep): float32 0 or
    1 / (1 - p).  ``seed`` is the snapshotted device word itself."""
    if p <= 0:
        return np.ones((M, K), np.float32)
    with np.errstate(over="ignore"):
        el = np.arange(M * K, dtype=np.uint64).reshape(M, K)
        key = (np.uint64(site) << np.uint64(44)) ^ el
        z = _mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ _mix64(key))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(u >= np.float32(p), scale, np.float32(0)).astype(np.float32)


def _mlp(dims, dropout, dev, seed=0):
    from gr_amd.rqvae import MLPLayers
    torch.manual_seed(seed)
    m = MLPLayers(dims, dropout=dropout).to(dev).train()
    for lin in m.linears():   # non-zero biases exercise the bias gradient
        lin.bias.data.normal_(0.0, 0.1)
    return m


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("dims,M", [([768, 256, 128, 32], 64), ([32, 128, 256, 768], 64),
                                    ([768, 256, 128, 32], 200), ([48, 40, 8], 33)])
def test_fused_mlp_matches_torch_without_dropout(dims, M, dev):
    import copy
    m = _mlp(dims, 0.0, dev)
    ref = copy.deepcopy(m)
    ref.fused_train = False
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(M, dims[0], generator=g, device=dev)
    up = torch.randn(M, dims[-1], generator=g, device=dev)
    outs = []
    for mm in (m, ref):
        xx = x.clone().requires_grad_(True)
        y = mm.train_forward(xx)
        (y * up).sum().backward()
        outs.append((y.detach(), xx.grad))
    assert _rel(outs[0][0], outs[1][0]) <= 1e-5
    assert _rel(outs[0][1], outs[1][1]) <= 2e-5
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert _rel(p.grad, q.grad) <= 2e-5, k


def test_fused_mlp_dropout_gradients_on_the_kernel_mask(dev):
    from gr_amd import ops
    K, M, p = 96, 70, 0.3
    m = _mlp([K, K], p, dev)
    lin = m.linears()[0]
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.rand(M, K, generator=g, device=dev) + 0.5          # positive: the mask is y / x
    seed = ops.dropout_seed(dev)
    s0 = int(seed.item())
    # the mask of this seed word: identity weight, zero bias
    with torch.no_grad():
        w0, b0 = lin.weight.clone(), lin.bias.clone()
        lin.weight.copy_(torch.eye(K, device=dev))
        lin.bias.zero_()
        seed.fill_(s0)
        y0 = ops.mlp_train(x, m)
        keep = y0 / x
        lin.weight.copy_(w0)
        lin.bias.copy_(b0)
    # the numpy replica is the kernel's mask, element for element (x * keep is one fp32 product and
    # the identity product adds zeros to it: exact)
    rep = torch.from_numpy(keep_mask(s0, 0, M, K, p)).to(dev)
    assert torch.equal(keep > 0, rep > 0)
    assert torch.equal(y0, x * rep)
    kept = (keep > 0).float().mean().item()
    assert abs(kept - (1 - p)) < 0.03                               # Bernoulli(1 - p) keeps
    assert torch.allclose(keep[keep > 0], torch.full_like(keep[keep > 0], 1 / (1 - p)))
    up = torch.randn(M, K, generator=g, device=dev)
    seed.fill_(s0)                                                   # the same masks again
    xx = x.clone().requires_grad_(True)
    y = ops.mlp_train(xx, m)
    (y * up).sum().backward()
    x2 = x.clone().requires_grad_(True)
    w2 = lin.weight.detach().clone().requires_grad_(True)
    b2 = lin.bias.detach().clone().requires_grad_(True)
    y2 = F.linear(x2 * keep, w2, b2)
    (y2 * up).sum().backward()
    assert _rel(y.detach(), y2.detach()) <= 1e-5
    assert _rel(xx.grad, x2.grad) <= 2e-5
    assert _rel(lin.weight.grad, w2.grad) <= 2e-5
    assert _rel(lin.bias.grad, b2.grad) <= 2e-5


def test_dropout_mask_replica_site_1(dev):
    """The forward epilogue's mask (site i + 1, keyed on the output pitch N): a two-layer MLP whose
    first weight is a rectangular identity (N = 24 of K = 40 inputs pass), zero bias, positive
    inputs, so the second layer's saved dropped input is Xd_1 = drop_1(drop_0(x)[:, :N]) exactly."""
    from gr_amd import ops
    K, N, M, p = 40, 24, 37, 0.3
    m = _mlp([K, N, 8], p, dev)
    lin = m.linears()[0]
    with torch.no_grad():
        lin.weight.copy_(torch.eye(N, K, device=dev))
        lin.bias.zero_()
    x = torch.rand(M, K, generator=torch.Generator(device=dev).manual_seed(4), device=dev) + 0.5
    seed = ops.dropout_seed(dev)
    s0 = int(seed.item())
    y = ops.mlp_train(x, m)
    assert int(seed.item()) == s0 + 1
    xd0, _snap, xd1 = y.grad_fn.saved_tensors[:3]
    k0 = torch.from_numpy(keep_mask(s0, 0, M, K, p)).to(dev)
    k1 = torch.from_numpy(keep_mask(s0, 1, M, N, p)).to(dev)
    assert torch.equal(xd0, x * k0)
    assert torch.equal(xd1, xd0[:, :N] * k1)
    assert not torch.equal(k0[:, :N], k1)                           # the two sites draw different masks


# (dims, M): main.py's encoder and decoder; widths that are no multiple of 4 (load16's scalar
# branch), K < 32 (one wave of tile_split has work), K = 33, N = 1; M = 1; M = 33 and 129 across
# the 32-row tile edge, 129 with five k groups in the dW product; a 770-wide scalar-load input
SHAPES = [([768, 256, 128, 32], 64), ([32, 128, 256, 768], 64), ([30, 33, 7, 1], 33), ([5, 3], 1),
          ([70, 129, 40], 129), ([770, 64, 32], 31)]
SEED_WORD = 0x1234567887654321


def _restate(x, ws, bs, masks, up, dtype):
    """x_{i+1} = relu(drop_i(x_i) W_i^T + b_i), the last layer without ReLU, and the gradients of
    sum(y * up) in x, every W and every b: torch autograd on the CPU in ``dtype``."""
    x = x.detach().to(dtype, copy=True).requires_grad_(True)
    ws = [w.detach().to(dtype, copy=True).requires_grad_(True) for w in ws]
    bs = [b.detach().to(dtype, copy=True).requires_grad_(True) for b in bs]
    h = x
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = F.linear(h * masks[i].to(dtype), w, b)
        if i + 1 < len(ws):
            h = torch.relu(h)
    grads = torch.autograd.grad((h * up.to(dtype)).sum(), [x, *ws, *bs])
    return [h.detach(), *grads]


def _mlp_case(dims, M, p, seed_word=SEED_WORD):
    """CPU inputs of one case: x, weights, biases, the masks of ``seed_word`` and the upstream
    gradient."""
    g = torch.Generator().manual_seed(1000 + 7 * M + len(dims))
    x = torch.randn(M, dims[0], generator=g)
    ws = [torch.randn(o, i, generator=g) * (2.0 / (i + o)) ** 0.5 for i, o in zip(dims[:-1], dims[1:])]
    bs = [0.1 * torch.randn(o, generator=g) for o in dims[1:]]
    up = torch.randn(M, dims[-1], generator=g)
    masks = [torch.from_numpy(keep_mask(seed_word, i, M, dims[i], p)) for i in range(len(dims) - 1)]
    return x, ws, bs, masks, up


def _fused_vs_fp64(dims, M, p, dev, parity_log):
    from gr_amd import ops
    x, ws, bs, masks, up = _mlp_case(dims, M, p)
    m = _mlp(dims, p, dev)
    with torch.no_grad():
        for lin, w, b in zip(m.linears(), ws, bs):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
    seed = ops.dropout_seed(dev)
    seed.fill_(SEED_WORD)
    xx = x.to(dev).requires_grad_(True)
    y = ops.mlp_train(xx, m)
    (y * up.to(dev)).sum().backward()
    got = [y.detach(), xx.grad] + [lin.weight.grad for lin in m.linears()] + [lin.bias.grad for lin in m.linears()]
    ref = _restate(x, ws, bs, masks, up, torch.float64)
    t32 = _restate(x, ws, bs, masks, up, torch.float32)
    n = len(ws)
    names = ["y", "dX"] + [f"dW{i}" for i in range(n)] + [f"db{i}" for i in range(n)]
    tols = [TOL_OUT, TOL_DX] + [TOL_DW] * (2 * n)
    bad = []
    for name, tol, a, b32, b in zip(names, tols, got, t32, ref):
        assert a.shape == b.shape, name
        err_kernel = _rel(a.detach().cpu().double(), b)
        err_t32 = _rel(b32.double(), b)
        parity_log(kind="mlp_train_vs_fp64", dims=dims, M=M, p=p, quantity=name, err_t32=err_t32,
                   err_kernel=err_kernel, tol=tol)
        if not err_kernel <= tol:
            bad.append((name, err_kernel, tol))
    assert not bad, bad


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dims,M", SHAPES)
def test_fused_mlp_dropout_multilayer_vs_fp64(dims, M, p, dev, parity_log):
    """Multi-layer MLPs with dropout on (main.py runs 0.1): the forward epilogue's next-site mask,
    the backward's folded ReLU-and-dropout mask (dx_mode 1) and the first layer's hash mask
    (dx_mode 2), against fp64 on the replica's masks."""
    _fused_vs_fp64(dims, M, p, dev, parity_log)


@pytest.mark.parametrize("dims,M", SHAPES)
def test_fused_mlp_edge_shapes_vs_fp64(dims, M, dev, parity_log):
    """The same shapes with dropout off: the scalar-load and tile-edge paths against fp64."""
    _fused_vs_fp64(dims, M, 0.0, dev, parity_log)


def test_rqvae_forward_uses_fused_mlps_and_trains(dev):
    """RQVAE.forward in train mode runs the encoder / decoder on the fused kernels (the same
    gradients as the torch modules at dropout 0) and main.py's dropout 0.1 trains."""
    import copy
    from gr_amd import RQVAE
    torch.manual_seed(0)
    m = RQVAE(in_dim=768, num_emb_list=[8, 8, 8], e_dim=32, layers=[256, 128], dropout_prob=0.0,
              quant_loss_weight=0.1, beta=0.25, sk_epsilons=[0.01] * 3, sk_iters=50).to(dev).train()
    for q in m.rq.vq_layers:
        q.embedding.weight.data.normal_(0.0, 0.3)
    ref = copy.deepcopy(m)
    ref.encoder.fused_train = ref.decoder.fused_train = False
    x = torch.randn(64, 768, generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    res = []
    for mm in (m, ref):
        mm.zero_grad(set_to_none=True)
        o, rq_loss, idx = mm(x)
        loss, _ = mm.compute_loss(o, rq_loss, xs=x)
        loss.backward()
        res.append((loss.item(), idx))
    assert torch.equal(res[0][1], res[1][1])
    assert abs(res[0][0] - res[1][0]) <= 1e-5 * abs(res[1][0])
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert _rel(p.grad, q.grad) <= 5e-5, k
