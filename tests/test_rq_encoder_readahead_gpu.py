"""The fused RQ encoder (csrc/rq_fused.hip) reads its MFMA operands from LDS one step ahead: layer
1's item-tile-0 x fragments a 32-deep group early -- across the chunk barrier, the MKL k-block edge
and the pass boundary, the last read of a workgroup being one nobody uses -- and layer 2's first h1
fragments a 64-deep block early.  These are the shapes where a read-ahead can go wrong: chunk counts
around the read-ahead distance (one chunk per pass: every read-ahead crosses a pass boundary), pass
sequences that change the x image's layout under a fragment already read (two-tile pass -> one-tile
or k-split pass -> pieces), and a workgroup's last pass.

Every case is bitwise, with no tolerance: z against oracle/rq_exact.mlp, IDs against
rq_exact.encode, and both against the layer-wise path (rq_fused = 0).  The CU count C is read from
the device.  The model construction and the check are those of test_rq_encoder_plans_gpu.py
(restated: the test modules do not import each other).
"""
import pytest
import torch

from oracle import rq_exact

pytestmark = pytest.mark.gpu

# in_dim -> 64-wide chunks per pass: 64: 1, 128: 2, 192: 3, 320: 5 (one MKL block, odd), 384: 6 (one
# block for calls of >= 256 rows), 640: 5 + 5 (MKL splits at 320: k-split pass of five chunk
# iterations, and pieces)
WIDTHS = [64, 128, 192, 320, 384, 640]
# rows as a function of the CU count C
ROWS = {
    "one_tile_pass_ragged": lambda C: 32 * C - 3,               # a one-tile pass only, ragged last tile
    "two_two_tile_passes_then_odd_tile": lambda C: 32 * 5 * C - 3,
}
C2_ROWS = {
    "leftover_tile_as_pieces_after_two_tile_passes": lambda C: 32 * (2 * C + 1) + 5,
    "k_split_pass_then_piece": lambda C: 32 * (C + C // 4),
    "short_call_pieces_only": lambda C: 40,
}


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


@pytest.fixture(scope="module")
def narrow_models(dev):
    """One model per width, built on first use and shared by the module's tests."""
    cache = {}

    def get(in_dim):
        if in_dim not in cache:
            cache[in_dim] = _narrow_model(in_dim, dev)
        return cache[in_dim]
    return get


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
    parity_log(kind="rq_encoder_readahead", shape=shape, rows=len(xc), z_rows_differ=zd, rows_differ=idd,
               z_rows_differ_from_layerwise=int((z != z_lw).any(1).sum()),
               rows_differ_from_layerwise=int((idx != idx_lw).any(1).sum()))
    assert zd == 0, f"{zd} z rows differ from the oracle"
    assert idd == 0, f"{idd} ID rows differ from the oracle"
    assert torch.equal(z, z_lw) and torch.equal(idx, idx_lw)
    return idx, z


@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("in_dim", WIDTHS)
def test_chunk_counts_around_the_readahead_distance(in_dim, rows, dev, cus, narrow_models, parity_log):
    from gr_amd import synth
    n = ROWS[rows](cus)
    x = synth.items(n, 81, dev)[:, :in_dim].contiguous()
    _check(narrow_models(in_dim), x, parity_log, f"in {in_dim}, {cus} CUs, n {n} ({rows})")


@pytest.mark.parametrize("case", list(C2_ROWS))
def test_last_pass_dead_prefetch_and_pieces_handover(case, dev, cus, c2_model, parity_log):
    from gr_amd import synth
    n = C2_ROWS[case](cus)
    x = synth.items(n, 82, dev)
    _check(c2_model, x, parity_log, f"C2 model, {cus} CUs, n {n} ({case})")


def test_back_to_back_calls_equal(dev, cus, narrow_models):
    """Two calls with no host sync in between on the largest case (in = 640, two two-tile passes, a
    k-split pass and no pieces per workgroup): equal, z included."""
    from gr_amd import ops, synth
    in_dim, n = 640, 32 * 5 * cus - 3
    m = narrow_models(in_dim)
    x = synth.items(n, 83, dev)[:, :in_dim].contiguous()
    lin = m.encoder.linears()
    ws, bs, cbs = [l.weight for l in lin], [l.bias for l in lin], m.rq.codebooks()
    a = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    b = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
