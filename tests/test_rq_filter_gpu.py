"""The filtered quantizer (csrc/rq.hip rq_filter_kernel, option "rq_filter"): a split-bf16 pass
bounds every distance and the exact fp32 formula runs only on the codes within the bound of the
minimum.  The IDs must be what the exact kernel gives, bit for bit, exact ties included.

Every case runs ops.rq_quantize with rq_filter at 1 and at 0.  Finite inputs: both results equal
oracle.rq_exact.quantize with 0 rows differing.  Non-finite inputs (the oracle is not pinned there):
the two settings agree with each other.  No tolerance anywhere.
"""
import pytest
import torch

from oracle import rq_exact

pytestmark = pytest.mark.gpu

E_DIM = 32


def _both(z, cbs):
    """IDs with rq_filter 1 and 0, and the number of filtered launches each setting made."""
    from gr_amd import _lib, ops
    launches = _lib.lib().gr_rq_filter_launches
    old = _lib.get_option("rq_filter")
    try:
        _lib.set_option("rq_filter", 1)
        c0 = launches()
        on = ops.rq_quantize(z, cbs)
        c1 = launches()
        _lib.set_option("rq_filter", 0)
        off = ops.rq_quantize(z, cbs)
        c2 = launches()
    finally:
        _lib.set_option("rq_filter", old)
    return on, off, c1 - c0, c2 - c1


def _check(z, cbs, parity_log, shape, finite=True):
    on, off, _, _ = _both(z, cbs)
    differ = int((on != off).any(1).sum())
    rec = dict(kind="rq_filter", shape=shape, rows=z.shape[0], rows_differ_filter_vs_exact_kernel=differ)
    if finite:
        ref = torch.from_numpy(rq_exact.quantize(z.cpu().numpy(), [c.cpu().numpy() for c in cbs]))
        d_on = int((on.cpu() != ref).any(1).sum())
        d_off = int((off.cpu() != ref).any(1).sum())
        parity_log(rows_differ=d_on, rows_differ_exact_kernel=d_off, **rec)
        assert d_on == 0, f"{shape}: {d_on} rows differ from the oracle with rq_filter = 1"
        assert d_off == 0, f"{shape}: {d_off} rows differ from the oracle with rq_filter = 0"
    else:
        parity_log(**rec)
    assert differ == 0, f"{shape}: {differ} rows differ between rq_filter = 1 and 0"
    return on


def _rand(n, Ks, seed, dev, e=E_DIM, scale_z=1.0, scale_c=1.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((n, e), generator=g) * scale_z
    cbs = [torch.randn((K, e), generator=g) * (0.5 ** l) * scale_c for l, K in enumerate(Ks)]
    return z.to(dev), [c.to(dev) for c in cbs]


def test_option_selects_the_filtered_kernel(dev):
    from gr_amd import _lib
    assert _lib.get_option("rq_filter") == 1
    z, cbs = _rand(257, [256, 256, 256], 1, dev)
    _, _, ran_on, ran_off = _both(z, cbs)
    assert ran_on == 1 and ran_off == 0
    z5, cbs5 = _rand(257, [256], 2, dev, e=5)
    _, _, ran_on, ran_off = _both(z5, cbs5)
    assert ran_on == 0 and ran_off == 0   # e != 32 stays on the exact kernel


@pytest.mark.parametrize("n", [1, 31, 32, 33, 257, 8193])
def test_item_counts_mixed_codebooks(n, dev, parity_log):
    z, cbs = _rand(n, [256, 33, 1024], 10 + n, dev)
    _check(z, cbs, parity_log, f"n {n}, K [256, 33, 1024]")


@pytest.mark.parametrize("K", [1, 2, 31, 32, 33, 255, 256, 257, 1024])
def test_codebook_sizes_one_level(K, dev, parity_log):
    z, cbs = _rand(257, [K], 40 + K, dev)
    _check(z, cbs, parity_log, f"n 257, K [{K}]")


@pytest.mark.parametrize("Ks", [[256, 256, 256], [255, 256, 257, 32], [1024, 1024, 1024, 1024], [1025, 256]])
def test_levels(Ks, dev, parity_log):
    z, cbs = _rand(8193 if Ks[0] == 256 else 257, Ks, 70 + len(Ks), dev)
    _check(z, cbs, parity_log, f"K {Ks}")


@pytest.mark.parametrize("e", [5, 16, 64])
def test_other_widths_stay_intact(e, dev, parity_log):
    z, cbs = _rand(257, [256, 33], 90 + e, dev, e=e)
    _check(z, cbs, parity_log, f"e {e}, K [256, 33]")


def test_exact_ties_first_index_wins(dev, parity_log):
    g = torch.Generator().manual_seed(3)
    z, cbs = _rand(257, [128, 128], 4, dev)
    _check(z, [torch.cat([c, c]) for c in cbs], parity_log, "every row twice")
    ids = _check(z, [cbs[0][:1].expand(64, -1).contiguous()], parity_log, "all rows identical")
    assert int(ids.abs().sum()) == 0
    zq = (torch.randint(-16, 17, (257, E_DIM), generator=g).float() / 8).to(dev)
    cq = [(torch.randint(-16, 17, (256, E_DIM), generator=g).float() / 8).to(dev) for _ in range(3)]
    _check(zq, cq, parity_log, "multiples of 1/8 in [-2, 2]")
    pick = torch.randint(0, 128, (257,), generator=g).to(dev)
    _check(cbs[0][pick].clone(), cbs, parity_log, "z is a code row")


@pytest.mark.parametrize("first", ["a", "b"])
def test_one_ulp_near_ties(first, dev, parity_log):
    g = torch.Generator().manual_seed(5)
    z, (cb,) = _rand(257, [64], 6, "cpu")
    b = cb.clone()
    col = torch.randint(0, E_DIM, (64,), generator=g)
    rows = torch.arange(64)
    b[rows, col] = torch.nextafter(b[rows, col], torch.full((64,), float("inf")))
    pair = torch.stack([cb, b] if first == "a" else [b, cb], 1).reshape(128, E_DIM).to(dev)
    _check(z.to(dev), [pair], parity_log, f"one-ulp pairs, {first} first")
    near = (cb[torch.randint(0, 64, (257,), generator=g)] * 1.0001).to(dev)
    _check(near, [pair], parity_log, f"one-ulp pairs with z next to a pair, {first} first")


@pytest.mark.parametrize("ez,ec", [(-100, -100), (-60, -60), (40, 40), (63, 63), (12, -12), (-12, 12)])
def test_magnitudes(ez, ec, dev, parity_log):
    z, cbs = _rand(257, [256, 256], 7, dev, scale_z=2.0 ** ez, scale_c=2.0 ** ec)
    _check(z, cbs, parity_log, f"z x 2^{ez}, codes x 2^{ec}")


@pytest.mark.parametrize("case", ["z_nan", "z_inf", "code_nan", "level_nan"])
def test_non_finite_inputs_agree(case, dev, parity_log):
    z, cbs = _rand(257, [256, 256, 33], 8, dev)
    if case == "z_nan":
        z[5, 3] = float("nan")
    elif case == "z_inf":
        z[70, 31] = float("inf")
    elif case == "code_nan":
        cbs[0][17, 9] = float("nan")
    else:
        cbs[1].fill_(float("nan"))
    _check(z, cbs, parity_log, case, finite=False)


@pytest.fixture(scope="module")
def c2_model(dev):
    from gr_amd import synth
    return synth.rqvae_model(3, 256, dev)


@pytest.mark.parametrize("n", [8193, 65537])
def test_get_indices_through_the_fused_encoder(n, dev, c2_model, parity_log):
    from gr_amd import _lib, synth
    x = synth.items(n, 91, dev)
    m = c2_model
    on = m.get_indices(x)
    _lib.set_option("rq_filter", 0)
    try:
        off = m.get_indices(x)
    finally:
        _lib.set_option("rq_filter", 1)
    lin = m.encoder.linears()
    ref = rq_exact.encode(x.cpu().numpy(), [l.weight.detach().cpu() for l in lin], [l.bias.detach().cpu() for l in lin],
                          [c.detach().cpu() for c in m.rq.codebooks()])
    differ = int((on.cpu().numpy() != ref).any(1).sum())
    parity_log(kind="rq_filter_get_indices", rows=n, rows_differ=differ,
               rows_differ_filter_vs_exact_kernel=int((on != off).any(1).sum()))
    assert differ == 0
    assert torch.equal(on, off)


def test_with_gap_is_unchanged(dev):
    from gr_amd import _lib, ops
    z, cbs = _rand(257, [256, 33, 1024], 9, dev)
    launches = _lib.lib().gr_rq_filter_launches
    c0 = launches()
    a = ops.rq_quantize(z, cbs, with_gap=True)
    assert launches() == c0   # the calls that return distances stay on the exact kernel
    _lib.set_option("rq_filter", 0)
    try:
        b = ops.rq_quantize(z, cbs, with_gap=True)
    finally:
        _lib.set_option("rq_filter", 1)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(a[0], ops.rq_quantize(z, cbs))
