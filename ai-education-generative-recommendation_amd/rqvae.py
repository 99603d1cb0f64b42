"""Drop-in RQ-VAE module whose encode path runs on the gfx950 kernels.

Same constructor, submodule tree and ``state_dict`` keys as the reference
(RQ-VAE/models/rqvae.py:10-53, rq.py:13-30, vq.py:9-27, layers.py:9-40), so reference checkpoints
load unchanged and ``RQ-VAE/infer.py`` / ``generate_code.py`` can swap the import:

    from models.rqvae import RQVAE            ->   from gr_amd.rqvae import RQVAE

``get_indices(xs, use_sk=False)`` (rqvae.py:67-71) is one C-ABI call, ``gr_rq_encode_f32``.
``forward(x, use_sk)`` (rqvae.py:60-65, the training call of RQ-VAE/train.py:113) is differentiable,
with every level's codebook assignment (argmin or Sinkhorn) on the kernels.
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.init import xavier_normal_

from . import ops

# Near-tie certificate (SURVEY §7 hard part 1).  The encoder output of any fp32 implementation
# differs from the reference's CPU/MKL bits by |dz| <= Z_TAU |z| (per row).  Z_TAU = 3x the largest
# ratio measured in round 2, before the encoder became exact, on HELD-OUT fixtures
# (tests/golden/make_golden_calib.py: rq_calib_3x256 + rq_calib_wide_3x256, 20,480 rows, two encoder
# shapes, both kernel paths; max 1.165e-6, profiles/r02_parity_counts.json).  Since round 3 the GPU
# encoder reproduces those fixtures' z bit for bit (tests/test_rq_gpu.py), so the certificate now
# bounds another CPU's MKL order instead: the bench host's |z_host - z_gpu| / |z| is reported against
# Z_TAU in every RQ cpu_baseline (bench.rq_agreement; 9.2e-7 at most on the EPYC box, round 6).
# A moved z moves every level's residual by ~dz, so
# d = |r - c|^2 moves by <= 2 sqrt(d) |dz|; the fp32 evaluation (|r|^2 + |c|^2) - 2 r.c rounds at
# ~eps (|r| + |c|)^2 <= eps (|z| + sqrt(d))^2.  A level whose best/second-best gap is below the sum
# of both bounds (for the two distances) can legitimately resolve either way; every other row
# must match the reference bit for bit.
Z_TAU = 3.5e-6
D_EPS = 2.4e-7     # 4 x 2^-24


def near_tie_bound(best, gap, znorm2):
    """Upper bound of the fp32 disagreement on (second-best - best) at each level; tensors or
    numpy arrays: best/gap [n, L], znorm2 = ||z||^2 [n]."""
    zn = znorm2[:, None] ** 0.5
    d2 = (best + gap).clip(0) ** 0.5 if hasattr(best, "clip") else (best + gap).clamp_min(0) ** 0.5
    return 4 * d2 * Z_TAU * zn + 2 * D_EPS * (zn + d2) ** 2


def near_tie_rows(best, gap, znorm2):
    """Rows with at least one level whose argmin is within the fp32 certificate."""
    return (gap <= near_tie_bound(best, gap, znorm2)).any(1)


_ACTS = {"sigmoid": nn.Sigmoid, "tanh": nn.Tanh, "relu": nn.ReLU, "leakyrelu": nn.LeakyReLU}


def _act_name(activation):
    """activation_layer of RQ-VAE/models/layers.py:45-67 -> the kernel epilogue name (None: none)."""
    if activation is None:
        return None
    if isinstance(activation, str):
        a = activation.lower()
        if a == "none":
            return None
        if a in _ACTS:
            return a
        raise NotImplementedError(f"activation function {activation} is not implemented")
    for name, cls in _ACTS.items():
        if isinstance(activation, type) and issubclass(activation, cls):
            return name
    raise NotImplementedError(f"gr_amd kernels implement sigmoid / tanh / relu / leakyrelu, not {activation}")


class MLPLayers(nn.Module):
    """Module tree of RQ-VAE/models/layers.py:9-40 (Dropout, Linear, [BatchNorm1d], activation per
    layer; none after the last Linear), xavier_normal_ weights and zero biases.

    Eval forward on the kernels in the reference's CPU order, bit for bit (gr_mlp_exact_f32): ReLU,
    LeakyReLU and activation-free MLPs, with or without the eval BatchNorm1d (torch's CPU formula,
    not folded); in -> 256 -> 128 -> 32 ReLU MLPs on the fused encoder kernel.  Sigmoid / Tanh run
    the gr_linear_f32 epilogues (fp32-close, not bitwise: torch's CPU exp / tanh are its own)."""

    def __init__(self, layers, dropout=0.0, activation="relu", bn=False):
        super().__init__()
        self.layers = layers
        self.dropout = dropout
        self.activation = activation
        self.use_bn = bn
        self.act = _act_name(activation)
        mods = []
        last = len(layers) - 2
        for idx, (i, o) in enumerate(zip(layers[:-1], layers[1:])):
            mods.append(nn.Dropout(p=dropout))
            mods.append(nn.Linear(i, o))
            if bn and idx != last:
                mods.append(nn.BatchNorm1d(num_features=o))
            if self.act is not None and idx != last:
                mods.append(_ACTS[self.act]() if isinstance(activation, str) else activation())
        self.mlp_layers = nn.Sequential(*mods)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(module):
        if isinstance(module, nn.Linear):
            xavier_normal_(module.weight.data)
            if module.bias is not None:
                module.bias.data.fill_(0.0)

    def linears(self):
        return [m for m in self.mlp_layers if isinstance(m, nn.Linear)]

    def folded(self):
        """(weights, biases) of the eval-mode layers with each BatchNorm1d folded into its Linear."""
        lin = self.linears()
        bns = [m for m in self.mlp_layers if isinstance(m, nn.BatchNorm1d)]
        ws, bs = [], []
        for i, m in enumerate(lin):
            w, b = m.weight.detach(), m.bias.detach()
            if self.use_bn and i < len(lin) - 1:
                bn = bns[i]
                s = torch.rsqrt(bn.running_var + bn.eps)
                if bn.weight is not None:
                    s = s * bn.weight.detach()
                w = w * s[:, None]
                b = (b - bn.running_mean) * s
                if bn.bias is not None:
                    b = b + bn.bias.detach()
            ws.append(w.contiguous())
            bs.append(b.contiguous())
        return ws, bs

    def eval_forward(self, x):
        """layers.py:42-43 in eval mode on ``gr_linear_f32`` layer by layer (any widths; the
        activation after every Linear but the last) — the decoder of the no-grad forward."""
        ws, bs = self.folded() if self.use_bn else ([m.weight.detach() for m in self.linears()],
                                                   [m.bias.detach() for m in self.linears()])
        for i, (w, b) in enumerate(zip(ws, bs)):
            x = ops.linear(x, w, b, act=(self.act or "none") if i + 1 < len(ws) else "none")
        return x

    # train-mode forward under autograd on the fused training kernels (ops.mlp_train: one launch per
    # layer and direction); False keeps the torch modules
    fused_train = True

    def train_forward(self, x):
        """layers.py:42-43 under autograd (the RQVAE.forward call of RQ-VAE/train.py:113): ReLU MLPs
        without BatchNorm on ``ops.mlp_train``, anything else on the torch modules."""
        if self.fused_train and ops.mlp_train_supported(self, x):
            return ops.mlp_train(x, self)
        return self.mlp_layers(x)

    def bn_params(self):
        """(means, vars, weights, biases, eps) of the BatchNorm1d layers (``bn=True``), else None."""
        bns = [m for m in self.mlp_layers if isinstance(m, nn.BatchNorm1d)]
        if not bns:
            return None
        d = lambda t: None if t is None else t.detach()   # noqa: E731
        return ([b.running_mean for b in bns], [b.running_var for b in bns], [d(b.weight) for b in bns],
                [d(b.bias) for b in bns], float(bns[0].eps))

    def forward(self, x, group_sizes=None):
        """Eval forward in the reference's CPU order for ONE call of ``len(x)`` rows (MKL's order
        depends on the call's row count), or, with ``group_sizes``, for consecutive row groups
        that are one reference call each (the collision re-encode of RQ-VAE/infer.py:116-127)."""
        if self.training and (self.dropout > 0 or self.use_bn):
            raise RuntimeError("gr_amd MLPLayers runs the eval-mode encoder: call .eval() (dropout / "
                               "BatchNorm batch statistics are train-mode only)")
        if self.act not in ("relu", "leakyrelu", None):
            return self.eval_forward(x)
        lin = self.linears()
        return ops.rq_mlp(x, [m.weight.detach() for m in lin],
                          [m.bias.detach() if m.bias is not None else torch.zeros(m.out_features, device=x.device)
                           for m in lin], bn=self.bn_params(), act=self.act or "none", group_sizes=group_sizes)


class VectorQuantizer(nn.Module):
    """Parameter holder of RQ-VAE/models/vq.py:9-27 (``embedding`` [n_e, e_dim]).  Initialised
    uniform(-1/n_e, 1/n_e), or zeros when ``kmeans_init`` (vq.py:21-27)."""

    def __init__(self, n_e, e_dim, beta=0.25, kmeans_init=False, kmeans_iters=10,
                 sk_epsilon=0.003, sk_iters=100):
        super().__init__()
        self.n_e = n_e
        self.e_dim = e_dim
        self.beta = beta
        self.kmeans_init = kmeans_init
        self.kmeans_iters = kmeans_iters
        self.sk_epsilon = sk_epsilon
        self.sk_iters = sk_iters
        self.embedding = nn.Embedding(n_e, e_dim)
        if not kmeans_init:
            self.initted = True
            self.embedding.weight.data.uniform_(-1.0 / n_e, 1.0 / n_e)
        else:
            self.initted = False
            self.embedding.weight.data.zero_()

    def get_codebook(self):
        return self.embedding.weight

    def get_codebook_entry(self, indices, shape=None):
        z_q = self.embedding(indices)
        return z_q.view(shape) if shape is not None else z_q

    # "host": scikit-learn on the host, the reference's own call (the default); "device": ops.kmeans
    # on the kernels, seeded by kmeans_seed (None: torch's default generator).  RQVAE.set_kmeans sets both.
    kmeans_backend = "host"
    kmeans_seed = None

    def init_emb(self, data):
        """vq.py:39-47 + layers.py:69-82: codebook <- KMeans(n_e, max_iter) centres of the first
        training batch's latents.  ``kmeans_backend`` "host": scikit-learn (host, once; the
        reference's own call); "device": ``ops.kmeans``, the centres copied into the codebook on
        the device without a synchronisation."""
        if self.kmeans_backend == "device":
            res = ops.kmeans(data.detach(), self.n_e, max_iter=self.kmeans_iters, seed=self.kmeans_seed,
                             with_labels=False)
            self.embedding.weight.data.copy_(res.centers)
            self.initted = True
            return
        if self.kmeans_backend != "host":
            raise ValueError(f"kmeans_backend must be 'host' or 'device', got {self.kmeans_backend!r}")
        from sklearn.cluster import KMeans
        centers = KMeans(n_clusters=self.n_e, max_iter=self.kmeans_iters).fit(
            data.detach().cpu().numpy()).cluster_centers_
        self.embedding.weight.data.copy_(torch.from_numpy(centers).to(self.embedding.weight.device))
        self.initted = True


class ResidualVectorQuantizer(nn.Module):
    """Module tree of RQ-VAE/models/rq.py:13-30."""

    def __init__(self, n_e_list, e_dim, sk_epsilons, beta=0.25, kmeans_init=False,
                 kmeans_iters=100, sk_iters=100):
        super().__init__()
        self.n_e_list = n_e_list
        self.e_dim = e_dim
        self.num_quantizers = len(n_e_list)
        self.beta = beta
        self.kmeans_init = kmeans_init
        self.kmeans_iters = kmeans_iters
        self.sk_epsilons = sk_epsilons
        self.sk_iters = sk_iters
        self.vq_layers = nn.ModuleList([
            VectorQuantizer(n_e, e_dim, beta=beta, kmeans_init=kmeans_init,
                            kmeans_iters=kmeans_iters, sk_epsilon=eps, sk_iters=sk_iters)
            for n_e, eps in zip(n_e_list, sk_epsilons)])

    def get_codebook(self):
        return torch.stack([q.get_codebook() for q in self.vq_layers])

    def codebooks(self):
        return [q.embedding.weight.detach() for q in self.vq_layers]

    # every level's assignment, x_q and the losses in one launch (ops.rq_quantize_train), backward
    # in two; False (or a level still waiting for its k-means init) keeps the level-by-level path
    fused_train = True

    def quantize_forward(self, x, use_sk=True, training=False):
        """rq.py:39-56 with vq.py:63-99 per level.  Fused path: one launch assigns every level
        (Sinkhorn over the batch where ``use_sk`` and ``sk_epsilon > 0``, else the argmin), forms
        x_q and the mse numerators; a custom backward gives dz and every codebook's gradient.
        Level-by-level path (k-means init pending: a level's init needs the residual it sees,
        vq.py:66-67): indices from the kernels, values and losses under autograd."""
        if (self.fused_train and x.is_cuda and all(q.initted for q in self.vq_layers)
                and all(q.n_e <= 1024 for q in self.vq_layers)):
            eps = [float(q.sk_epsilon) if use_sk else 0.0 for q in self.vq_layers]
            z = x.reshape(-1, self.e_dim)
            xq, rq_loss, idx = ops.rq_quantize_train(z, [q.embedding.weight for q in self.vq_layers],
                                                     self.beta, eps, self.sk_iters)
            return xq.view(x.shape), rq_loss, idx.view(tuple(x.shape[:-1]) + (self.num_quantizers,))
        losses, idxs = [], []
        x_q = 0
        residual = x
        for q in self.vq_layers:
            latent = residual.reshape(-1, self.e_dim)
            if not q.initted and training:
                q.init_emb(latent.detach())
            cb = q.embedding.weight.detach()
            eps = q.sk_epsilon if use_sk else 0.0
            if eps > 0:
                idx = ops.rq_quantize_sk(latent.detach(), [cb], [eps], q.sk_iters)[:, 0]
            else:
                idx = ops.rq_quantize(latent.detach(), [cb])[:, 0]
            xq = q.embedding(idx).view(residual.shape)
            commitment_loss = F.mse_loss(xq.detach(), residual)
            codebook_loss = F.mse_loss(xq, residual.detach())
            losses.append(codebook_loss + q.beta * commitment_loss)
            xq = residual + (xq - residual).detach()
            residual = residual - xq
            x_q = x_q + xq
            idxs.append(idx.view(residual.shape[:-1]))
        return x_q, torch.stack(losses).mean(), torch.stack(idxs, dim=-1)


class RQVAE(nn.Module):
    """Drop-in for RQ-VAE/models/rqvae.py:RQVAE (same arguments, same ``state_dict``)."""

    def __init__(self, in_dim=768, num_emb_list=None, e_dim=64, layers=None, dropout_prob=0.0,
                 bn=False, loss_type="mse", quant_loss_weight=1.0, beta=0.25, kmeans_init=False,
                 kmeans_iters=100, sk_epsilons=None, sk_iters=100):
        super().__init__()
        self.in_dim = in_dim
        self.num_emb_list = num_emb_list
        self.e_dim = e_dim
        self.layers = layers
        self.dropout_prob = dropout_prob
        self.bn = bn
        self.loss_type = loss_type
        self.quant_loss_weight = quant_loss_weight
        self.beta = beta
        self.kmeans_init = kmeans_init
        self.kmeans_iters = kmeans_iters
        self.sk_epsilons = sk_epsilons
        self.sk_iters = sk_iters
        self.encode_layer_dims = [in_dim] + list(layers) + [e_dim]
        self.encoder = MLPLayers(layers=self.encode_layer_dims, dropout=dropout_prob, bn=bn)
        self.rq = ResidualVectorQuantizer(num_emb_list, e_dim, beta=beta, kmeans_init=kmeans_init,
                                          kmeans_iters=kmeans_iters, sk_epsilons=sk_epsilons,
                                          sk_iters=sk_iters)
        self.decode_layer_dims = self.encode_layer_dims[::-1]
        self.decoder = MLPLayers(layers=self.decode_layer_dims, dropout=dropout_prob, bn=bn)

    def forward(self, x, use_sk=True):
        """rqvae.py:60-65 -> ``(out, rq_loss, indices)``, differentiable (the RQ-VAE/train.py:113 call;
        SURVEY §8f row 4), on the gfx950 kernels end to end:
        * encoder and decoder: ``MLPLayers.train_forward`` (dropout in train mode, Linear, ReLU;
          one launch per layer forward and backward, ``ops.mlp_train``);
        * the quantizer: every level's assignment -- vq.py:69-84, the fp32 distance matrix and its
          argmin, or the batch-coupled Sinkhorn when ``use_sk`` and ``sk_epsilon > 0`` (main.py
          trains with eps 0.01 at every level) -- on the residual exactly as the reference forms
          it, with x_q and the codebook / commitment losses (vq.py:88-95) in the same launch and a
          two-launch backward (``ops.rq_quantize_train``).
        With grad disabled in eval mode the encoder and decoder run the inference kernels
        (``gr_rq_mlp_f32`` / ``gr_linear_f32``)."""
        fast = not torch.is_grad_enabled() and not self.training
        z = self.encoder(x) if fast else self.encoder.train_forward(x)
        x_q, rq_loss, indices = self.rq.quantize_forward(z, use_sk, self.training)
        out = self.decoder.eval_forward(x_q) if fast else self.decoder.train_forward(x_q)
        return out, rq_loss, indices

    def compute_loss(self, out, quant_loss, xs=None):
        """rqvae.py:73-84: reconstruction (mse or l1, mean) + quant_loss_weight * quant_loss."""
        if self.loss_type == "mse":
            loss_recon = F.mse_loss(out, xs, reduction="mean")
        elif self.loss_type == "l1":
            loss_recon = F.l1_loss(out, xs, reduction="mean")
        else:
            raise ValueError("incompatible loss type")
        return loss_recon + self.quant_loss_weight * quant_loss, loss_recon

    def _check_encode(self, xs, use_sk):
        if self.training and self.bn:
            raise RuntimeError("gr_amd RQVAE.get_indices runs the eval-mode encoder: call .eval() "
                               "(BatchNorm uses batch statistics in train mode)")
        if self.training and self.dropout_prob > 0:
            raise RuntimeError("gr_amd RQVAE.get_indices runs the eval-mode encoder: call .eval() "
                               "(dropout is active in train mode)")
        if xs.dim() != 2 or xs.shape[1] != self.in_dim:
            raise RuntimeError(f"get_indices expects [B, {self.in_dim}] inputs, got {tuple(xs.shape)}")

    def get_indices(self, xs, use_sk=False):
        """rqvae.py:67-71: ``[B, in_dim]`` fp32 -> ``[B, L]`` int64 semantic IDs (one C-ABI call).

        ``use_sk=True`` with a level whose ``sk_epsilon > 0`` assigns that level by Sinkhorn over the
        whole batch (vq.py:76-84), as the reference does; the batch is one group.  The reference's
        eval call (no Sinkhorn, no BatchNorm, eval mode) goes straight to the cached binding's
        ``encode_fast`` -- its outputs never carry autograd history, so it needs no no_grad scope."""
        if not use_sk and not self.bn and not self.training:
            c = self.__dict__.get("_gr_rq_binding")
            if c is not None and c[2].direct and tuple(t.data_ptr() for t in c[0]) == c[1]:
                b = c[2]
                b.frozen = self.__dict__.get("_gr_frozen", True)
                idx = b.encode_fast(xs)
                if idx is not None:
                    return idx
        with torch.no_grad():
            return self._get_indices(xs, use_sk)

    def _get_indices(self, xs, use_sk):
        self._check_encode(xs, use_sk)
        if use_sk and any(q.sk_epsilon > 0 for q in self.rq.vq_layers):
            return ops.rq_quantize_sk(self.encoder(xs), self.rq.codebooks(), self.sk_eps(), self.rq.sk_iters)
        if self.bn:   # the eval BatchNorm in torch's CPU formula, then the quantizer
            return ops.rq_quantize(self.encoder(xs), self.rq.codebooks())
        return ops.rq_encode(xs, binding=self.encode_binding())

    def encode_binding(self):
        """The cached device-pointer view of the encoder and codebooks (ops.rq_binding).  With
        BatchNorm the folded weights are recomputed per call (the running statistics may change
        in place), so that binding is never cached."""
        if self.bn:
            ws, bs = self.encoder.folded()
            return ops.RqBinding(ws, bs, self.rq.codebooks())
        b = ops.rq_binding(self, self._encode_params)
        b.frozen = self.__dict__.get("_gr_frozen", True)
        return b

    def freeze_encoder(self, frozen=True):
        """True (default): keep the fused encoder's packed weight image across get_indices calls,
        re-packed when a weight's version counter or the graph-replay epoch moves
        (ops.weights_changed(); every training-graph replay bumps it).  False: pack the current
        weights on every call -- for callers that write weights through ``.data`` without calling
        ops.weights_changed()."""
        self.__dict__["_gr_frozen"] = bool(frozen)
        return self

    def set_kmeans(self, backend="device", seed=None):
        """Where every level's k-means init (``kmeans_init=True``) runs: "host" (default: scikit-learn,
        the reference's call) or "device" (``ops.kmeans`` on the kernels: no host round trip in the
        first forward).  With ``seed``, level l is seeded ``seed + l``, so the same seed gives the
        same codebooks; without, each level draws its seed from torch's default generator."""
        if backend not in ("host", "device"):
            raise ValueError(f"kmeans backend must be 'host' or 'device', got {backend!r}")
        for l, q in enumerate(self.rq.vq_layers):
            q.kmeans_backend = backend
            q.kmeans_seed = None if seed is None else int(seed) + l
        return self

    def call_plans(self, n):
        """MKL's order for a reference call of ``n`` rows: [(kind, kb, pinned)] per encoder Linear,
        then per quantizer level (ops.mkl_plan)."""
        dims = self.encode_layer_dims
        plans = [ops.mkl_plan(n, k, o) for k, o in zip(dims[:-1], dims[1:])]
        return plans + [ops.mkl_plan(n, self.e_dim, q.n_e) for q in self.rq.vq_layers]

    def parity_pinned(self, n):
        """True when every sgemm order of a get_indices call of ``n`` rows is in the envelope
        checked bit for bit against the reference's CPU run (gr_mkl_plan)."""
        return all(p[2] for p in self.call_plans(n))

    @torch.no_grad()
    def get_indices_batched(self, xs, batch_size=64):
        """``torch.cat([get_indices(xs[i:i + batch_size]) for i in range(0, len(xs), batch_size)])``
        -- the reference's DataLoader loop (RQ-VAE/infer.py:84-95, generate_code.py:78-88) -- in at
        most two launches when the full batches share one MKL order with a single call over them
        (true for the reference's widths): the full batches together, then the short tail batch
        as its own call (1-15 rows take MKL's small-call orders)."""
        n = xs.shape[0]
        tail = n % batch_size
        main = n - tail
        parts = []
        if main:
            order = lambda m: [p[:2] for p in self.call_plans(m)]   # noqa: E731
            if main == batch_size or order(batch_size) == order(main):
                parts.append(self.get_indices(xs[:main]))
            else:
                parts += [self.get_indices(xs[i:i + batch_size]) for i in range(0, main, batch_size)]
        if tail:
            parts.append(self.get_indices(xs[main:]))
        if not parts:
            return torch.empty((0, len(self.rq.vq_layers)), dtype=torch.int64, device=xs.device)
        return torch.cat(parts) if len(parts) > 1 else parts[0]

    def _encode_params(self):
        lin = self.encoder.linears()
        return [m.weight for m in lin], [m.bias for m in lin], [q.embedding.weight for q in self.rq.vq_layers]

    def sk_eps(self):
        return [float(q.sk_epsilon) for q in self.rq.vq_layers]

    @torch.no_grad()
    def get_indices_groups(self, xs, group_sizes):
        """``torch.cat([get_indices(g, use_sk=True) for g in groups])`` for consecutive row groups
        of ``xs`` in one launch — the per-group loop of RQ-VAE/infer.py:116-127."""
        self._check_encode(xs, True)
        return ops.rq_quantize_sk(self.encoder(xs, group_sizes=group_sizes), self.rq.codebooks(), self.sk_eps(),
                                  self.rq.sk_iters, group_sizes)

    @torch.no_grad()
    def get_indices_certified(self, xs):
        """``get_indices`` plus a per-row near-tie flag: ``(idx [B, L], flags [B] bool)``.

        A flagged row has a level whose best/second-best fp32 distance gap is within the rounding
        certificate (``near_tie_bound``): it may legitimately differ from a CPU run of the reference.
        Every unflagged row is the reference's answer."""
        self._check_encode(xs, False)
        if self.bn:
            z = self.encoder(xs)
            idx, best, gap = ops.rq_quantize(z, self.rq.codebooks(), with_gap=True)
        else:
            idx, best, gap, z = ops.rq_encode(xs, binding=self.encode_binding(), with_gap=True, with_z=True)
        return idx, near_tie_rows(best, gap, (z * z).sum(1))
