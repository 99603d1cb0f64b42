"""The fused RQ encoder (csrc/rq_fused.hip) stages layer 1's x chunks through per-pass buffer
resources: a scalar base (the pass's first row), a byte count that ends at the last row that exists
and belongs to the pass (rows past it read as zeros by the hardware's range check), one per-thread
byte offset for the whole kernel, and the chunk's offset as a scalar.  The two LDS addresses of the
double-buffered x image are carried and flipped, not rebuilt from a parity.  These are the shapes
where that can go wrong: a ragged last tile in every pass type (two-tile, one-tile, k-split, piece),
every chunk count per pass (odd and even, so every buffer parity at a pass boundary), rows that must
not be swapped or repeated, an x that is a view into a larger tensor, and a call whose x is larger
than a 32-bit byte count.

Every case is bitwise, with no tolerance: z against oracle/rq_exact.mlp, IDs against
rq_exact.encode, and both against the layer-wise path (rq_fused = 0).  The CU count C is read from
the device.  The model construction and the check are those of test_rq_encoder_readahead_gpu.py
(restated: the test modules do not import each other).
"""
import pytest
import torch

from oracle import rq_exact

pytestmark = pytest.mark.gpu

# rows as a function of the CU count C
RAGGED = {
    "one_tile_pass_one_valid_row_in_last_tile": lambda C: 32 * C - 31,
    "two_tile_pass_ragged": lambda C: 32 * 2 * C - 1,
    "k_split_pass_then_one_row_piece": lambda C: 32 * 3 * C + 1,
    "two_tile_pass_then_ragged_piece": lambda C: 32 * (2 * C + 1) + 5,
    "pieces_only": lambda C: 40,
    "k_split_pass_then_pieces": lambda C: 32 * (C + C // 4),
}
# in_dim -> 64-wide chunks per pass: 1, 2, 3, 5 and 6 (one MKL block each at these row counts)
PARITY_WIDTHS = [64, 128, 192, 320, 384]


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _model(in_dim, dev, seed=5):
    """synth.rqvae_model's construction (seeded xavier encoder, small random biases, data-derived
    codebooks) at another input width; the items are the first ``in_dim`` columns of synth.items."""
    from gr_amd import RQVAE, ops, synth
    if in_dim == 768:
        return synth.rqvae_model(3, 256, dev)
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
def models(dev):
    """One model per width (768: the C2 model), built on first use and shared by the module's tests."""
    cache = {}

    def get(in_dim):
        if in_dim not in cache:
            cache[in_dim] = _model(in_dim, dev)
        return cache[in_dim]
    return get


def _both_paths(m, x):
    """(IDs, z) of the fused path and of the layer-wise path."""
    from gr_amd import _lib, ops
    lin = m.encoder.linears()
    ws, bs, cbs = [l.weight for l in lin], [l.bias for l in lin], m.rq.codebooks()
    idx, z = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    _lib.set_option("rq_fused", 0)
    try:
        idx_lw, z_lw = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    finally:
        _lib.set_option("rq_fused", 1)
    return (idx, z), (idx_lw, z_lw), (ws, bs, cbs)


def _check(m, x, parity_log, shape):
    """z and IDs of the fused path and of the layer-wise path, all four against the oracle."""
    (idx, z), (idx_lw, z_lw), (ws, bs, cbs) = _both_paths(m, x)
    cw, cb = [w.detach().cpu() for w in ws], [b.detach().cpu() for b in bs]
    xc = x.cpu().numpy()
    zref = rq_exact.mlp(xc, cw, cb)
    iref = rq_exact.encode(xc, cw, cb, [c.cpu() for c in cbs])
    zd = int((z.cpu().numpy() != zref).any(1).sum())
    idd = int((idx.cpu().numpy() != iref).any(1).sum())
    parity_log(kind="rq_encoder_staging", shape=shape, rows=len(xc), z_rows_differ=zd, rows_differ=idd,
               z_rows_differ_from_layerwise=int((z != z_lw).any(1).sum()),
               rows_differ_from_layerwise=int((idx != idx_lw).any(1).sum()))
    assert zd == 0, f"{zd} z rows differ from the oracle"
    assert idd == 0, f"{idd} ID rows differ from the oracle"
    assert torch.equal(z, z_lw) and torch.equal(idx, idx_lw)
    return idx, z


def _items(n, seed, in_dim, dev):
    from gr_amd import synth
    x = synth.items(n, seed, dev)
    return x if in_dim == x.shape[1] else x[:, :in_dim].contiguous()


@pytest.mark.parametrize("rows", list(RAGGED))
@pytest.mark.parametrize("in_dim", [768, 640])
def test_ragged_last_tile_in_every_pass_type(in_dim, rows, dev, cus, models, parity_log):
    n = RAGGED[rows](cus)
    _check(models(in_dim), _items(n, 91, in_dim, dev), parity_log, f"in {in_dim}, {cus} CUs, n {n} ({rows})")


@pytest.mark.parametrize("in_dim", PARITY_WIDTHS)
def test_chunk_count_parities(in_dim, dev, cus, models, parity_log):
    """1, 2, 3, 5 and 6 chunks per pass over two two-tile passes and a one-tile pass: odd and even
    counts, and both x buffers at a pass boundary."""
    n = 32 * 5 * cus - 3
    _check(models(in_dim), _items(n, 92, in_dim, dev), parity_log,
           f"in {in_dim} ({in_dim // 64} chunks), {cus} CUs, n {n}")


def test_row_offsets_are_per_row(dev, cus, models, parity_log):
    """Row i = synth.items row (i * 7919 mod n): a swapped or repeated staged row changes z."""
    n = 32 * (2 * cus + 1) + 5
    src = _items(n, 93, 768, dev)
    x = src[(torch.arange(n, device=dev) * 7919) % n].contiguous()
    _check(models(768), x, parity_log, f"C2 model, {cus} CUs, n {n} (permuted rows)")


def test_x_is_a_view_into_a_larger_tensor(dev, cus, models, parity_log):
    """x = big[s : s + n] with s no multiple of 32, big itself 16 bytes into its allocation: the x
    pointer is 16-byte aligned (what the ABI asks for) and not 32-byte aligned."""
    n, s, tail = 32 * 2 * cus - 1, 13, 7
    flat = torch.zeros(4 + (s + n + tail) * 768, device=dev)
    big = flat[4:].view(s + n + tail, 768)
    big.copy_(_items(s + n + tail, 94, 768, dev))
    x = big[s:s + n]
    assert x.is_contiguous() and x.data_ptr() % 32 == 16 and s % 32 != 0
    _check(models(768), x, parity_log, f"C2 model, {cus} CUs, n {n} (rows {s}.. of a larger tensor)")


def test_one_call_past_4_gib_of_input(dev, models):
    """n x 768 x 4 bytes > 2^32: the smallest shape at which one 32-bit byte count over the whole of
    x goes wrong.  Fused against layer-wise only (the CPU oracle would take minutes)."""
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 24 * 2 ** 30:
        pytest.skip("needs 24 GiB of free device memory")
    n = 1_400_000 + 17
    g = torch.Generator(device=dev).manual_seed(95)
    x = torch.randn((n, 768), generator=g, device=dev)
    x *= 0.05
    (idx, z), (idx_lw, z_lw), _ = _both_paths(models(768), x)
    assert torch.equal(z, z_lw)
    assert torch.equal(idx, idx_lw)


def test_back_to_back_calls_equal(dev, cus, models):
    """Two calls with no host sync in between on the largest ragged case (in = 768: two-tile passes,
    a k-split pass and a one-row piece): equal, z included."""
    from gr_amd import ops
    n = 32 * 3 * cus + 1
    m = models(768)
    x = _items(n, 96, 768, dev)
    lin = m.encoder.linears()
    ws, bs, cbs = [l.weight for l in lin], [l.bias for l in lin], m.rq.codebooks()
    a = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    b = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
