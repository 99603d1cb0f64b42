"""An encode call is two launches: the filtered quantizer's workgroups finish the fused encoder's
leftover tiles themselves (csrc/rq.hip rq_filter_kernel<LIVE, true>, option "rq_tail_merge";
csrc/rq_fused.h rq_leftover_tile and rq_filter_range), rq_leftover_kernel is not launched.

With C compute units and 32-item tiles, a call of T tiles has T % C leftover tiles (every tile when
4 T <= C, the short-call plan).  Every plan is run at the smallest n that reaches it on the device
the test runs on: IDs equal to oracle/rq_exact.encode, z equal to rq_exact.mlp, both equal to the
three-launch path (rq_tail_merge = 0), and the launch counters say which kernels ran.  No tolerance
anywhere: IDs and z are compared bitwise.

The codebook-update cases at the end run through RQVAE.get_indices, whose binding caches the
filtered quantizer's packed codebook image (ops.RqBinding.cb_image_ptr) under the codebooks' version
counters and the graph-replay epoch: the quantizer must see the codebooks a call is made with,
however they were changed since the call before, and a capture with a stale image must raise.
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


def _leftover_tiles(n, C):
    T = (n + 31) // 32
    if 4 * T <= C:
        return T
    return T % min(T, C)


def _encode_both(x, ws, bs, cbs):
    """(idx, z) with rq_tail_merge 1 and 0, and what each call added to the filter / leftover
    launch counters."""
    from gr_amd import _lib, ops
    lib = _lib.lib()
    out = {}
    old = _lib.get_option("rq_tail_merge")
    try:
        for opt in (1, 0):
            _lib.set_option("rq_tail_merge", opt)
            f0, l0 = lib.gr_rq_filter_launches(), lib.gr_rq_leftover_launches()
            idx, z = ops.rq_encode(x, ws, bs, cbs, with_z=True)
            out[opt] = (idx, z, lib.gr_rq_filter_launches() - f0, lib.gr_rq_leftover_launches() - l0)
    finally:
        _lib.set_option("rq_tail_merge", old)
    return out


def _params(m):
    lin = m.encoder.linears()
    return [l.weight for l in lin], [l.bias for l in lin]


def _oracle(x, ws, bs, cbs):
    cw, cb = [w.detach().cpu() for w in ws], [b.detach().cpu() for b in bs]
    xc = x.cpu().numpy()
    return rq_exact.mlp(xc, cw, cb), rq_exact.encode(xc, cw, cb, [c.detach().cpu() for c in cbs])


# n as a function of the CU count C
PLANS = {
    "no_leftover_tile": lambda C: 32 * 2 * C,
    "one_ragged_leftover_tile": lambda C: 32 * (2 * C + 1) + 5,
    "last_quarter_piece_count": lambda C: 32 * (2 * C + C // 4),
    "first_half_piece_count": lambda C: 32 * (2 * C + C // 4 + 1),
    "workgroup_with_two_pieces": lambda C: 32 * (2 * C + C // 2 + 1),
    "all_but_one_workgroup_owns_a_tile": lambda C: 32 * (3 * C - 1),
    "short_call_every_tile_leftover": lambda C: 32 * (C // 4) - 3,
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_plan_two_launches_vs_oracle_and_three_launches(plan, dev, cus, c2_model, parity_log):
    from gr_amd import _lib, synth
    assert _lib.get_option("rq_tail_merge") == 1
    n = PLANS[plan](cus)
    if plan == "short_call_every_tile_leftover" and n <= 1024:
        pytest.skip("the short-call plan of the whole-tile kernels starts past 1,024 rows")
    x = synth.items(n, 81, dev)
    ws, bs = _params(c2_model)
    cbs = c2_model.rq.codebooks()
    out = _encode_both(x, ws, bs, cbs)
    zref, iref = _oracle(x, ws, bs, cbs)
    (idx, z, f_on, l_on), (idx3, z3, f_off, l_off) = out[1], out[0]
    zd = int((z.cpu().numpy() != zref).any(1).sum())
    idd = int((idx.cpu().numpy() != iref).any(1).sum())
    parity_log(kind="rq_two_launch_plan", shape=f"C2 model, {cus} CUs, n {n} ({plan})", rows=n, z_rows_differ=zd,
               rows_differ=idd, z_rows_differ_from_three_launch=int((z != z3).any(1).sum()),
               rows_differ_from_three_launch=int((idx != idx3).any(1).sum()))
    assert zd == 0, f"{zd} z rows differ from the oracle"
    assert idd == 0, f"{idd} ID rows differ from the oracle"
    assert torch.equal(z, z3) and torch.equal(idx, idx3)
    left = _leftover_tiles(n, cus)
    assert (f_on, l_on) == (1, 0), "merged path: one filter launch, no leftover launch"
    assert (f_off, l_off) == (1, 1 if left else 0), "three-launch path: the leftover kernel runs when tiles are left"


def _codebooks(m, x, Ks, dev, seed=9):
    """Codebooks of the given sizes drawn from the model's own residuals (rows of z, then of what
    the level before leaves), so the distances have the scale of real ones."""
    from gr_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    ws, bs = _params(m)
    r = ops.rq_mlp(x[:4096], ws, bs)
    cbs = []
    for K in Ks:
        pick = torch.randint(0, r.shape[0], (K,), generator=g, device=dev)
        cb = (r[pick] + 0.01 * r.std() * torch.randn((K, 32), generator=g, device=dev)).contiguous()
        c = cb[ops.rq_quantize(r, [cb])[:, 0]]
        r = r - (r + (c - r))
        cbs.append(cb)
    return cbs


@pytest.mark.parametrize("Ks,merged", [([255, 256, 32], True), ([1024, 1024], True), ([1025, 256], False)],
                         ids=["K255_256_32", "K1024_1024", "K1025_256_exact_kernel"])
def test_codebook_sizes_at_one_ragged_leftover_tile(Ks, merged, dev, cus, c2_model):
    """K <= 256 (the kernel's register-resident form), K up to 1024 (the recomputing form), and a
    level past 1024 codes, which stays on the exact kernel behind rq_leftover_kernel."""
    from gr_amd import synth
    n = 32 * (2 * cus + 1) + 5
    x = synth.items(n, 82, dev)
    ws, bs = _params(c2_model)
    cbs = _codebooks(c2_model, x, Ks, dev)
    out = _encode_both(x, ws, bs, cbs)
    zref, iref = _oracle(x, ws, bs, cbs)
    (idx, z, f_on, l_on), (idx3, z3, f_off, l_off) = out[1], out[0]
    assert np.array_equal(z.cpu().numpy(), zref) and np.array_equal(idx.cpu().numpy(), iref)
    assert torch.equal(z, z3) and torch.equal(idx, idx3)
    assert (f_on, l_on) == ((1, 0) if merged else (0, 1))
    assert (f_off, l_off) == ((1, 1) if merged else (0, 1))


def test_back_to_back_calls_equal(dev, cus, c2_model):
    """Two calls with no host synchronisation between them (the second encoder writes the leftover
    pieces' scratch right behind the first quantizer's read of it): equal, z included."""
    from gr_amd import ops, synth
    n = 32 * (2 * cus + cus // 4 + 1)
    x = synth.items(n, 83, dev)
    ws, bs = _params(c2_model)
    cbs = c2_model.rq.codebooks()
    a = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    b = ops.rq_encode(x, ws, bs, cbs, with_z=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    i1, i2 = c2_model.get_indices(x), c2_model.get_indices(x)
    assert torch.equal(i1, i2) and torch.equal(i1, a[0])


# ---- the codebooks a call sees, through RQVAE.get_indices ----

def _fresh_model(dev):
    """A model of its own (the C2 model's construction again), for the tests that change codebooks."""
    from gr_amd import synth
    return synth.rqvae_model(3, 256, dev)


def _model_oracle(m, x):
    ws, bs = _params(m)
    return _oracle(x, ws, bs, m.rq.codebooks())[1]


@pytest.fixture(scope="module")
def x_ragged(dev, cus):
    from gr_amd import synth
    return synth.items(32 * (2 * cus + 1) + 5, 84, dev)


def test_in_place_codebook_update_is_seen(dev, x_ragged):
    m = _fresh_model(dev)
    before = m.get_indices(x_ragged)
    with torch.no_grad():
        for l, q in enumerate(m.rq.vq_layers):
            q.embedding.weight.mul_(1.0 + 0.25 * (l + 1))
    after = m.get_indices(x_ragged)
    assert np.array_equal(after.cpu().numpy(), _model_oracle(m, x_ragged))
    assert not torch.equal(before, after)


def test_data_write_then_weights_changed_is_seen(dev, x_ragged):
    from gr_amd import ops
    m = _fresh_model(dev)
    m.get_indices(x_ragged)
    for q in m.rq.vq_layers:
        q.embedding.weight.data[::2] *= 1.5
    ops.weights_changed()
    assert np.array_equal(m.get_indices(x_ragged).cpu().numpy(), _model_oracle(m, x_ragged))


def test_unfrozen_model_reads_the_live_codebooks(dev, x_ragged):
    m = _fresh_model(dev).freeze_encoder(False)
    m.get_indices(x_ragged)
    for q in m.rq.vq_layers:
        q.embedding.weight.data[1::2] *= 0.75
    assert np.array_equal(m.get_indices(x_ragged).cpu().numpy(), _model_oracle(m, x_ragged))


def test_two_models_called_alternately(dev, c2_model, x_ragged):
    a, b = c2_model, _fresh_model(dev)
    with torch.no_grad():
        for q in b.rq.vq_layers:
            q.embedding.weight.copy_(q.embedding.weight.flip(0) * 1.25)
    ra, rb = _model_oracle(a, x_ragged), _model_oracle(b, x_ragged)
    for _ in range(2):
        assert np.array_equal(a.get_indices(x_ragged).cpu().numpy(), ra)
        assert np.array_equal(b.get_indices(x_ragged).cpu().numpy(), rb)
    assert not np.array_equal(ra, rb)


def test_image_and_in_kernel_staging_agree(dev, c2_model, x_ragged):
    """The cached image is in use for a frozen model, and the kernel that copies it returns what the
    kernel that derives the images from the codebooks returns (and the oracle)."""
    from gr_amd import _lib
    with_image = c2_model.get_indices(x_ragged)
    c2_model.freeze_encoder(False)
    try:
        derived = c2_model.get_indices(x_ragged)
    finally:
        c2_model.freeze_encoder(True)
    assert torch.equal(with_image, derived)
    assert np.array_equal(with_image.cpu().numpy(), _model_oracle(c2_model, x_ragged))
    nf = _lib.lib().gr_rq_codebook_image_floats(32, 3, _lib.i32_array([256] * 3))
    per_level = 2 * 256 * 32 + 256 + 16            # hi|lo image, fp32 image, norms, the maximum's slots
    assert nf == 3 * ((per_level + 255) // 256 * 256)   # each level rounded up to 1 KiB
    b = c2_model.encode_binding()
    assert b.cb_image is not None and b.cb_image.numel() == nf and b._cb_key is not None


def test_capture_with_a_stale_codebook_image_raises(dev, x_ragged):
    m = _fresh_model(dev)
    m.get_indices(x_ragged)
    with torch.no_grad():
        m.rq.vq_layers[1].embedding.weight.mul_(1.125)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="packed codebook image is out of date"):
        with torch.cuda.graph(g, stream=s):
            _ = x_ragged[:4] * 1.0
            m.get_indices(x_ragged)
    torch.cuda.synchronize()
    # one eager call after the change, then the capture is allowed and replays the new codebooks
    ref = m.get_indices(x_ragged)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=s):
        out = m.get_indices(x_ragged)
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert np.array_equal(ref.cpu().numpy(), _model_oracle(m, x_ragged))
