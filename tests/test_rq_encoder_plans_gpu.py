"""Every partition plan of the fused RQ encoder (csrc/rq_fused.hip), at the smallest batch that
reaches it on the device the test runs on (the CU count is read, not assumed).

With C compute units and 32-item tiles, a call of T tiles gives every workgroup T // C whole tiles
(two-tile passes, an odd last tile as a k-split pass) and runs the T % C tiles past that as
feature pieces -- quarters while 4 (T % C) <= C, halves after that, a workgroup taking two half
pieces once 2 (T % C) > C -- with rq_leftover_kernel finishing their layers 2-3.  Every n is
checked for z bitwise equal to oracle/rq_exact.mlp, IDs equal to rq_exact.encode, and both equal to
the layer-wise path (rq_fused=0).  No tolerance anywhere.

Models: the C2 model of synth.rqvae_model (in = 768, MKL splits layer 1's K in two), in = 512 (MKL
splits it at 256: kb = 256 in gr_common.h's mkl_plan, so the k-split pass and the pieces run there
too, at four chunks per block), and in = 256, the width at which MKL runs ONE k block (csplit ==
NC): no k-split pass and no pieces, an odd last tile runs the one-tile pass.
"""
import numpy as np
import pytest
import torch

from oracle import rq_exact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.fixture(scope="module")
def c2_model(dev):
    from gr_amd import synth
    return synth.rqvae_model(3, 256, dev)


def _narrow_model(in_dim, dev, seed=5):
    """synth.rqvae_model's construction (seeded xavier encoder, small random biases, data-derived
    codebooks) at another input width; the items are the first ``in_dim`` columns of synth.items."""
    from gr_amd import RQVAE, ops, synth
    torch.manual_seed(seed)
    m = RQVAE(in_dim=in_dim, num_emb_list=[256] * 3, e_dim=32, layers=[256, 128], dropout_prob=0.1,
              sk_epsilons=[0.0] * 3).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    with torch.no_grad():
        for lin in m.encoder.linears():
            lin.bias.copy_(0.01 * torch.randn(lin.bias.shape, generator=g, device=dev))
        r = m.encoder(synth.items(4096, seed + 2, dev)[:, :in_dim].contiguous())
        for q in m.rq.vq_layers:
            pick = torch.randint(0, r.shape[0], (256,), generator=g, device=dev)
            q.embedding.weight.copy_(r[pick] + 0.01 * r.std() * torch.randn((256, 32), generator=g, device=dev))
            c = q.embedding.weight[ops.rq_quantize(r, [q.embedding.weight])[:, 0]]
            r = r - (r + (c - r))
    return m


def _check(m, x, parity_log, shape):
    """z and IDs of the fused path and of the layer-wise path, all four against the oracle."""
    from gr_amd import _lib, ops
    lin = m.encoder.linears()
    ws, bs, cbs = [l.weight for l in lin], [l.bias for l in lin], m.rq.codebooks()
    idx, z = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    _lib.set_option("rq_fused", 0)
    try:
        idx_lw, z_lw = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    finally:
        _lib.set_option("rq_fused", 1)
    cw, cb = [w.detach().cpu() for w in ws], [b.detach().cpu() for b in bs]
    xc = x.cpu().numpy()
    zref = rq_exact.mlp(xc, cw, cb)
    iref = rq_exact.encode(xc, cw, cb, [c.cpu() for c in cbs])
    zd = int((z.cpu().numpy() != zref).any(1).sum())
    idd = int((idx.cpu().numpy() != iref).any(1).sum())
    parity_log(kind="rq_encoder_plan", shape=shape, rows=len(xc), z_rows_differ=zd, rows_differ=idd,
               z_rows_differ_from_layerwise=int((z != z_lw).any(1).sum()),
               rows_differ_from_layerwise=int((idx != idx_lw).any(1).sum()))
    assert zd == 0, f"{zd} z rows differ from the oracle"
    assert idd == 0, f"{idd} ID rows differ from the oracle"
    assert torch.equal(z, z_lw) and torch.equal(idx, idx_lw)
    return idx, z


# n as a function of the CU count C
PLANS = {
    "two_tile_passes_only": lambda C: 32 * 2 * C,
    "two_tile_pass_and_k_split_pass": lambda C: 32 * 3 * C,
    "one_ragged_leftover_tile": lambda C: 32 * (2 * C + 1) + 5,
    "last_quarter_piece_count": lambda C: 32 * (2 * C + C // 4),
    "first_half_piece_count": lambda C: 32 * (2 * C + C // 4 + 1),
    "workgroup_with_two_pieces": lambda C: 32 * (2 * C + C // 2 + 1),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_plan_vs_oracle_and_layerwise(plan, dev, cus, c2_model, parity_log):
    from gr_amd import synth
    n = PLANS[plan](cus)
    x = synth.items(n, 77, dev)
    _check(c2_model, x, parity_log, f"C2 model, {cus} CUs, n {n} ({plan})")


@pytest.mark.parametrize("in_dim,tiles", [
    (512, lambda C: 3 * C + 1),   # MKL block edge at 256: two-tile + k-split passes, a quarter-piece tile
    (256, lambda C: 3 * C),       # one MKL block (csplit == NC): two-tile pass + one-tile pass
    (256, lambda C: 2 * C + 3),   # ... and uneven whole-tile ranges instead of pieces
], ids=["in512_split", "in256_unsplit", "in256_unsplit_uneven"])
def test_other_input_widths(in_dim, tiles, dev, cus, parity_log):
    from gr_amd import synth
    n = 32 * tiles(cus) - 3
    m = _narrow_model(in_dim, dev)
    x = synth.items(n, 78, dev)[:, :in_dim].contiguous()
    _check(m, x, parity_log, f"in {in_dim}, {cus} CUs, n {n}")


def test_back_to_back_calls_equal(dev, cus, c2_model):
    """Two calls with no host sync in between (the second reuses the leftover pieces' scratch and
    the packed weights while the first may still run): equal, z included."""
    from gr_amd import ops, synth
    n = 32 * (2 * cus + 1) + 5
    x = synth.items(n, 79, dev)
    lin = c2_model.encoder.linears()
    ws, bs, cbs = [l.weight for l in lin], [l.bias for l in lin], c2_model.rq.codebooks()
    a = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    b = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    i1, i2 = c2_model.get_indices(x), c2_model.get_indices(x)
    assert torch.equal(i1, i2) and torch.equal(i1, a[0])
