"""CPU restatement of RQ-VAE ``get_indices`` (test infrastructure only, see oracle/__init__.py).

Every function follows the reference ATen sequence so that, on the same host, the
outputs are bit-identical to the reference (pinned by tests/test_oracle_golden.py).
"""
import numpy as np
import torch


def mlp_encode(x, weights, biases):
    """MLPLayers.forward in eval mode (RQ-VAE/models/layers.py:18-33, 42-43).

    ``[Dropout -> Linear -> ReLU] * (len-2)`` then ``Dropout -> Linear`` (no activation after the
    last Linear, layers.py:28-30).  Dropout is the identity in eval mode.  ``nn.Linear`` is
    ``addmm(b, x, W^T)`` (torch.nn.functional.linear).
    """
    h = x
    n = len(weights)
    for i, (w, b) in enumerate(zip(weights, biases)):
        h = torch.nn.functional.linear(h, w, b)
        if i != n - 1:
            h = torch.relu(h)
    return h


def vq_level(latent, codebook):
    """VectorQuantizer.forward(x, use_sk=False) (RQ-VAE/models/vq.py:63-99).

    Returns (x_q, indices, d) where ``d`` is the distance matrix exactly as vq.py:71-73 forms it:
    ``(sum(r**2) + sum(C**2).t()) - 2 * (r @ C.t())``; ``argmin`` returns the first minimum (vq.py:75);
    ``x_q = r + (C[idx] - r)`` is the straight-through expression of vq.py:95.
    """
    d = torch.sum(latent ** 2, dim=1, keepdim=True) + \
        torch.sum(codebook ** 2, dim=1, keepdim=True).t() - \
        2 * torch.matmul(latent, codebook.t())
    indices = torch.argmin(d, dim=-1)
    x_q = torch.nn.functional.embedding(indices, codebook)
    x_q = latent + (x_q - latent)
    return x_q, indices, d


def rq_quantize(z, codebooks, return_detail=False):
    """ResidualVectorQuantizer.forward(x, use_sk=False) (RQ-VAE/models/rq.py:39-56).

    ``residual <- residual - x_res`` per level (rq.py:47); indices stacked on the last dim (rq.py:54).
    With ``return_detail`` also returns per-level residual inputs and the per-row gap between the best
    and second-best fp32 distance at every level (used to certify near-ties).
    """
    residual = z
    idx, residuals, gaps = [], [], []
    for cb in codebooks:
        x_res, ind, d = vq_level(residual, cb)
        if return_detail:
            residuals.append(residual.clone())
            top2 = torch.topk(d, k=min(2, d.shape[1]), dim=1, largest=False).values
            gap = (top2[:, 1] - top2[:, 0]) if d.shape[1] > 1 else torch.full_like(top2[:, 0], float("inf"))
            gaps.append(gap)
        residual = residual - x_res
        idx.append(ind)
    out = torch.stack(idx, dim=-1)
    if return_detail:
        return out, residuals, torch.stack(gaps, dim=-1)
    return out


@torch.no_grad()
def get_indices(x, weights, biases, codebooks, batch_size=None):
    """RQVAE.get_indices(xs, use_sk=False) (RQ-VAE/models/rqvae.py:67-71).

    ``batch_size`` reproduces the caller's DataLoader chunking (RQ-VAE/infer.py:84-95 uses 64):
    the CPU bits of the encoder GEMM depend on the batch size for tiny batches.
    """
    if batch_size is None:
        return rq_quantize(mlp_encode(x, weights, biases), codebooks)
    outs = [rq_quantize(mlp_encode(x[i:i + batch_size], weights, biases), codebooks)
            for i in range(0, x.shape[0], batch_size)]
    return torch.cat(outs, 0)


def state_to_lists(state_dict, n_levels):
    """Split an ``RQVAE.state_dict()`` into encoder weights/biases and codebooks.

    Keys follow RQ-VAE/models/layers.py:18-33 (``encoder.mlp_layers.{1,4,7,..}``: Dropout sits at the
    even indices, ReLU after each non-final Linear) and vq.py:22 (``rq.vq_layers.{l}.embedding.weight``).
    """
    lin = sorted({int(k.split('.')[2]) for k in state_dict if k.startswith('encoder.mlp_layers.')
                  and k.endswith('.weight')})
    ws = [state_dict[f'encoder.mlp_layers.{i}.weight'] for i in lin]
    bs = [state_dict[f'encoder.mlp_layers.{i}.bias'] for i in lin]
    cbs = [state_dict[f'rq.vq_layers.{l}.embedding.weight'] for l in range(n_levels)]
    return ws, bs, cbs


# ----------------------------------------------------------------------------- use_sk=True
def center_distance(d):
    """VectorQuantizer.center_distance_for_constraint (RQ-VAE/models/vq.py:52-61)."""
    mx, mn = d.max(), d.min()
    middle = (mx + mn) / 2
    amplitude = mx - middle + 1e-5
    assert amplitude > 0
    return (d - middle) / amplitude


@torch.no_grad()
def sinkhorn(distances, epsilon, iters):
    """sinkhorn_algorithm (RQ-VAE/models/layers.py:85-108), float64 input."""
    Q = torch.exp(- distances / epsilon)
    B, K = Q.shape
    Q /= Q.sum(-1, keepdim=True).sum(-2, keepdim=True)
    for _ in range(iters):
        Q /= torch.sum(Q, dim=1, keepdim=True)
        Q /= B
        Q /= torch.sum(Q, dim=0, keepdim=True)
        Q /= K
    Q *= B
    return Q


def vq_level_sk(latent, codebook, sk_epsilon, sk_iters, dot=None):
    """VectorQuantizer.forward(x, use_sk=True) (vq.py:63-99): Sinkhorn assignment when
    sk_epsilon > 0 (vq.py:76-84), else the argmin path.  ``dot(latent, codebook) -> [B, K]``
    replaces this host's ``latent @ codebook.t()`` on a Sinkhorn level (see quantize_sk)."""
    if sk_epsilon <= 0:
        x_q, ind, _ = vq_level(latent, codebook)
        return x_q, ind
    d = torch.sum(latent ** 2, dim=1, keepdim=True) + \
        torch.sum(codebook ** 2, dim=1, keepdim=True).t() - \
        2 * (torch.matmul(latent, codebook.t()) if dot is None else dot(latent, codebook))
    d = center_distance(d).double()
    Q = sinkhorn(d, sk_epsilon, sk_iters)
    ind = torch.argmax(Q, dim=-1)
    x_q = torch.nn.functional.embedding(ind, codebook)
    return latent + (x_q - latent), ind


@torch.no_grad()
def get_indices_sk(x, weights, biases, codebooks, sk_epsilons, sk_iters):
    """RQVAE.get_indices(xs, use_sk=True) (rqvae.py:67-71 -> rq.py:39-56 with vq_level_sk)."""
    residual = mlp_encode(x, weights, biases)
    idx = []
    for cb, eps in zip(codebooks, sk_epsilons):
        x_res, ind = vq_level_sk(residual, cb, eps, sk_iters)
        residual = residual - x_res
        idx.append(ind)
    return torch.stack(idx, dim=-1)


@torch.no_grad()
def quantize_sk(z, codebooks, sk_epsilons, sk_iters, dot=None):
    """ResidualVectorQuantizer.forward(z, use_sk=True) indices (rq.py:39-56) for ONE group of rows:
    the level chain of ``vq_level_sk`` with the residual update of rq.py:47 -> idx [B, L].

    The exact reference: torch's own CPU fp32 distances and the float64 Sinkhorn of
    layers.py:85-108, in this host's summation order.  The host's sgemm order is part of it: MKL
    on another CPU may round r . C^T differently, even differently for two equal rows of one call
    (a 6-row call on an AVX-512 AMD host: rows 0-3 and rows 4-5 come out of different kernels).  ``dot``
    puts a stated order in its place on the Sinkhorn levels, e.g. oracle.rq_exact.linear, the
    restatement of the fixture host's MKL order that the kernels follow."""
    residual, idx = z, []
    for cb, eps in zip(codebooks, sk_epsilons):
        x_res, ind = vq_level_sk(residual, cb, eps, sk_iters, dot)
        residual = residual - x_res
        idx.append(ind)
    return torch.stack(idx, dim=-1)


SK_LOG_MARGIN = 1e-2      # certified Sinkhorn level: log Q_top1 - log Q_top2 above this
SK_ARGMIN_MARGIN = 1e-4   # certified argmin level: relative distance gap above this


@torch.no_grad()
def quantize_sk_fp64(z, codebooks, sk_epsilons, sk_iters):
    """The same chain in float64 from the inputs on: distances, the centring with its ``+ 1e-5``,
    the Sinkhorn and the residual ``r - C[idx]`` -> (idx [B, L], margin [B, L]).

    It depends on no BLAS or vectorised-sum order, so it is the same on every host.  ``margin`` says
    how far a row's choice is from its runner-up, in the units in which an fp32 distance error acts:
      Sinkhorn level   log Q_top1 - log Q_top2 (Q is monotone in -d'/eps, so a distance error moves
                       log Q by about |delta d'| / eps);
      argmin level     (d_2nd - d_1st) / (|r|^2 + max |c|^2), the gap relative to the magnitude
                       whose rounding an fp32 distance carries;
      K = 1            infinity (nothing to choose).
    A row whose Q is NaN or all zero has margin 0."""
    r = z.double()
    idx, margins = [], []
    for cb, eps in zip(codebooks, sk_epsilons):
        c = cb.double()
        d = (r * r).sum(1, keepdim=True) + (c * c).sum(1)[None] - 2.0 * (r @ c.t())
        if eps > 0:
            mx, mn = d.max(), d.min()
            middle = (mx + mn) / 2
            Q = sinkhorn((d - middle) / (mx - middle + 1e-5), eps, sk_iters)
            ind = torch.argmax(Q, dim=-1)
            if c.shape[0] > 1:
                two = torch.topk(Q, 2, dim=1).values
                m = torch.log(two[:, 0]) - torch.log(two[:, 1])
                m = torch.where(torch.isnan(m), torch.zeros_like(m), m)
            else:
                m = torch.full((r.shape[0],), float("inf"), dtype=torch.float64)
        else:
            ind = torch.argmin(d, dim=-1)
            if c.shape[0] > 1:
                two = torch.topk(d, 2, dim=1, largest=False).values
                m = (two[:, 1] - two[:, 0]) / ((r * r).sum(1) + (c * c).sum(1).max())
            else:
                m = torch.full((r.shape[0],), float("inf"), dtype=torch.float64)
        r = r - c[ind]
        idx.append(ind)
        margins.append(m)
    return torch.stack(idx, dim=-1), torch.stack(margins, dim=-1)


def sk_certified(margin, sk_epsilons):
    """Rows of ``quantize_sk_fp64`` whose margin exceeds its level's threshold on EVERY level:
    SK_LOG_MARGIN where the level runs the Sinkhorn, SK_ARGMIN_MARGIN where it is the argmin."""
    thr = torch.tensor([SK_LOG_MARGIN if eps > 0 else SK_ARGMIN_MARGIN for eps in sk_epsilons],
                       dtype=torch.float64)
    return (margin > thr).all(1)


def collision_groups(codes):
    """get_collision_item (RQ-VAE/infer.py:29-41): rows sharing a code, groups in order of the
    code's first appearance, members in row order."""
    index2id = {}
    for i, c in enumerate(map(tuple, np.asarray(codes).tolist())):
        index2id.setdefault(c, []).append(i)
    return [g for g in index2id.values() if len(g) > 1]


def dedup_codes(codes):
    """infer.py:139-162: append a zero column, then number the members of every duplicate code."""
    codes_array = np.hstack((np.asarray(codes), np.zeros((len(codes), 1), dtype=int)))
    unique_codes, counts = np.unique(codes_array, axis=0, return_counts=True)
    for duplicate in unique_codes[counts > 1]:
        for i, idx in enumerate(np.where((codes_array == duplicate).all(axis=1))[0]):
            codes_array[idx, -1] = i
    return codes_array


@torch.no_grad()
def infer_codes(x, weights, biases, codebooks, sk_epsilons, sk_iters, batch_size=64, max_rounds=30,
                re_encode=None):
    """infer.py:88-162 without the file writes: codes (batch_size chunks, use_sk=False), collision
    rounds (every level but the last with sk_epsilon 0, infer.py:108-130), dedup digit.
    ``re_encode(rows) -> [g, L]`` overrides the group re-encode (default: get_indices_sk)."""
    codes = get_indices(x, weights, biases, codebooks, batch_size=batch_size).numpy()
    eps = [0.0] * (len(codebooks) - 1) + [sk_epsilons[-1]]
    rounds = []
    for _ in range(max_rounds):
        groups = collision_groups(codes)
        if not groups:
            break
        rounds.append(groups)
        for g in groups:
            out = (re_encode(g) if re_encode is not None else
                   get_indices_sk(x[g], weights, biases, codebooks, eps, sk_iters).numpy())
            codes[g] = out
    return codes, dedup_codes(codes), rounds
