"""The bound E of the filtered quantizer (csrc/rq.hip rq_filter_kernel, csrc/rq_quant.h
rq_filter_bound), checked on the CPU with the constants the kernel uses: E comes from the library's
host entry point gr_rq_filter_bound_f32.

The kernel's approximate value is restated with torch: a_k = cn_k - 2 r.c_k from split-bf16 operands
(x = hi + lo by ``.to(torch.bfloat16)``, the products hi.hi + hi.lo + lo.hi), once summed in float64
and rounded to fp32, once accumulated term by term in fp32 (one order the MFMA could take).  The
exact distance D_k = fl(fl(rn + cn_k) - 2 chain_k) is the torch restatement of the exact kernel's
formula (an fp32 fma chain over k in order, ATen's row sums); where oracle/rq_exact builds, its IDs
must equal the restatement's.  For every item, level and code with a finite bound:

    |a_k - (D_k - rn)| <= E        and        a_k* <= fl(min a + 2E)  for the exact winner k*

and where E or min a is not finite the kernel re-scores every code, which the test records.  The
candidate statistics (codes within 2E of the minimum) are printed per family.
"""
import pytest
import torch

E_DIM = 32


def _split(x):
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def _approx(r, cb, cn, fp32_order):
    rh, rl = _split(-2.0 * r)
    ch, cl = _split(cb)
    if not fp32_order:
        d = rh.double() @ ch.double().T + rh.double() @ cl.double().T + rl.double() @ ch.double().T
        return (d + cn.double()[None, :]).to(torch.float32)
    acc = cn[None, :].expand(r.shape[0], -1).clone()
    for a, b in ((rh, ch), (rh, cl), (rl, ch)):
        for k in range(r.shape[1]):
            acc = acc + a[:, k:k + 1] * b[None, :, k]   # bf16 x bf16: exact in fp32
    return acc


def _exact(r, cb, rn, cn):
    chain = torch.zeros((r.shape[0], cb.shape[0]), dtype=torch.float32)
    for k in range(r.shape[1]):   # fma: the product is exact in float64
        chain = (r[:, k:k + 1].double() * cb[None, :, k].double() + chain.double()).to(torch.float32)
    return ((rn[:, None] + cn[None, :]).double() - 2.0 * chain.double()).to(torch.float32)


def _bound(rn, cmax2):
    from gr_amd import _lib
    f = _lib.lib().gr_rq_filter_bound_f32
    return torch.tensor([f(float(v), float(cmax2)) for v in rn.tolist()], dtype=torch.float32)


def _levels(z, cbs, name):
    """Checks every level; returns the restated IDs [n, L]."""
    r = z.clone()
    ids, stats = [], []
    for l, cb in enumerate(cbs):
        rn, cn = (r * r).sum(1), (cb * cb).sum(1)
        D = _exact(r, cb, rn, cn)
        win = torch.argmin(torch.where(torch.isnan(D), torch.full_like(D, float("inf")), D), dim=1)
        E = _bound(rn, cn[~torch.isnan(cn)].max() if (~torch.isnan(cn)).any() else 0.0)
        for fp32_order in (False, True):
            a = _approx(r, cb, cn, fp32_order)
            m = torch.where(torch.isnan(a), torch.full_like(a, float("inf")), a).min(1).values
            thr = m + 2.0 * E                                   # fp32, as the kernel forms it
            fin = torch.isfinite(thr)                           # else: the kernel marks every code
            err = (a.double() - (D.double() - rn.double()[:, None])).abs()
            ok = (err <= E.double()[:, None]) | ~fin[:, None] | torch.isnan(D)
            assert bool(ok.all()), f"{name} level {l}: |a - (D - rn)| exceeds E " \
                                   f"(worst ratio {float((err / E.double()[:, None])[fin].max()):.3f})"
            aw = a.gather(1, win[:, None])[:, 0]
            assert bool(((aw <= thr) | ~fin).all()), f"{name} level {l}: the exact winner is not marked"
            ties = (D == D.gather(1, win[:, None])) & fin[:, None]
            assert bool((a <= thr[:, None])[ties].all()), f"{name} level {l}: a code tying with the winner is not marked"
            if not fp32_order:
                cand = torch.where(fin[:, None], a <= thr[:, None], torch.ones_like(a, dtype=torch.bool)).sum(1)
                ratio = float((err / E.double()[:, None])[fin].max()) if bool(fin.any()) else float("nan")
                stats.append(f"level {l}: candidates mean {float(cand.float().mean()):.3f} max {int(cand.max())}, "
                             f"all-marked items {int((~fin).sum())}, worst error / E {ratio:.3f}")
        ids.append(win)
        c = cb[win]
        r = r - (r + (c - r))
    print(f"\nRQ_FILTER_BOUND {name}: " + "; ".join(stats))
    return torch.stack(ids, 1)


def _check(z, cbs, name, oracle=True):
    ids = _levels(z, cbs, name)
    if oracle and z.shape[0] >= 2:
        try:
            from oracle import rq_exact
            ref = rq_exact.quantize(z.numpy(), [c.numpy() for c in cbs])
        except Exception:   # the oracle is not built here: the restatement stands alone
            return
        assert int((torch.from_numpy(ref) != ids).any(1).sum()) == 0, f"{name}: the restated IDs differ from the oracle"


def _rand(n, Ks, seed, scale_z=1.0, scale_c=1.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((n, E_DIM), generator=g) * scale_z
    return z, [torch.randn((K, E_DIM), generator=g) * (0.5 ** l) * scale_c for l, K in enumerate(Ks)]


@pytest.mark.parametrize("Ks", [[1], [2], [31], [33], [256, 33, 1024], [255, 256, 257, 32]])
def test_bound_random_shapes(Ks):
    z, cbs = _rand(257, Ks, 11 + len(Ks) + Ks[0])
    _check(z, cbs, f"random K {Ks}")


def test_bound_exact_ties():
    g = torch.Generator().manual_seed(3)
    z, cbs = _rand(257, [128, 128], 4)
    _check(z, [torch.cat([c, c]) for c in cbs], "every row twice")
    _check(z, [cbs[0][:1].expand(64, -1).contiguous()], "all rows identical")
    zq = torch.randint(-16, 17, (257, E_DIM), generator=g).float() / 8
    cq = [torch.randint(-16, 17, (256, E_DIM), generator=g).float() / 8 for _ in range(3)]
    _check(zq, cq, "multiples of 1/8")
    _check(cbs[0][torch.randint(0, 128, (257,), generator=g)].clone(), cbs, "z is a code row")


@pytest.mark.parametrize("first", ["a", "b"])
def test_bound_one_ulp_near_ties(first):
    g = torch.Generator().manual_seed(5)
    z, (cb,) = _rand(257, [64], 6)
    b = cb.clone()
    col = torch.randint(0, E_DIM, (64,), generator=g)
    rows = torch.arange(64)
    b[rows, col] = torch.nextafter(b[rows, col], torch.full((64,), float("inf")))
    pair = torch.stack([cb, b] if first == "a" else [b, cb], 1).reshape(128, E_DIM)
    _check(z, [pair], f"one-ulp pairs, {first} first")
    _check(cb[torch.randint(0, 64, (257,), generator=g)] * 1.0001, [pair], f"one-ulp pairs near z, {first} first")


@pytest.mark.parametrize("ez,ec", [(-100, -100), (-60, -60), (40, 40), (63, 63), (12, -12), (-12, 12)])
def test_bound_magnitudes(ez, ec):
    z, cbs = _rand(257, [256, 256], 7, 2.0 ** ez, 2.0 ** ec)
    _check(z, cbs, f"z x 2^{ez}, codes x 2^{ec}")


def _synth_latents(L, K, n, seed=0):
    """synth.rqvae_model's construction restated on the CPU: a seeded xavier 768 -> 256 -> 128 -> 32
    ReLU encoder with small biases over synth.items, codebooks = residual rows of a sample plus 1 %
    noise, level by level."""
    from gr_amd import synth
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    dims = [768, 256, 128, E_DIM]
    lins = [torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:])]
    with torch.no_grad():
        for lin in lins:
            torch.nn.init.xavier_normal_(lin.weight)
            lin.bias.copy_(0.01 * torch.randn(lin.bias.shape, generator=g))

        def enc(x):
            for i, lin in enumerate(lins):
                x = lin(x)
                x = torch.relu(x) if i + 1 < len(lins) else x
            return x
        r = enc(synth.items(4096, seed + 2, "cpu"))
        cbs = []
        for _ in range(L):
            pick = torch.randint(0, r.shape[0], (K,), generator=g)
            cb = r[pick] + 0.01 * r.std() * torch.randn((K, E_DIM), generator=g)
            cbs.append(cb)
            d = (r * r).sum(1, keepdim=True) + (cb * cb).sum(1)[None, :] - 2.0 * (r @ cb.T)
            c = cb[d.argmin(1)]
            r = r - (r + (c - r))
        return enc(synth.items(n, seed + 3, "cpu")), cbs


@pytest.mark.parametrize("L,K", [(3, 256), (4, 1024)])
def test_bound_synthetic_latents(L, K):
    z, cbs = _synth_latents(L, K, 4096)
    _check(z, cbs, f"synthetic latents L {L} K {K}, 4096 items")


def test_bound_entry_point_non_finite():
    from gr_amd import _lib
    f = _lib.lib().gr_rq_filter_bound_f32
    inf = float("inf")
    assert f(0.0, 0.0) > 0.0
    for rn, c2 in ((inf, 1.0), (1.0, inf), (float("nan"), 1.0), (3e38, 3e38)):
        assert not torch.isfinite(torch.tensor(f(rn, c2)))
