"""C ABI of the tiled SASRec training path (csrc/sasrec_train_tiled.hip), host side only: the size
queries, and the launchers' argument / envelope checks, which run before any device work (the
pointers handed over here are never dereferenced: no GPU is needed)."""
import ctypes

import pytest

GR_ERR_ARG, GR_ERR_UNSUPPORTED, GR_ERR_WORKSPACE = -1, -2, -4
FAKE = 0x10000   # a non-null "device address"


def _params(L, d=128, nb=2, H=1, mlp=64, max_len=256):
    return L.SasrecParams(d=d, n_blocks=nb, n_heads=H, mlp=mlp, max_len=max_len, eps=1e-8, item_rows=100,
                          **{f: FAKE for f, _ in L.SasrecParams._fields_[7:]})


def _bufs(L, **over):
    vals = {f: FAKE for f, _ in L.SasrecTrainBufs._fields_}
    vals.update(over)
    return L.SasrecTrainBufs(**vals)


def _call(lib, which, p, bufs, B=4, n=200, p_drop=0.2, seqs=FAKE, io=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.gr_sasrec_train_tiled_workspace_bytes(ctypes.byref(p), B, n) if p is not None else 0
    fn = lib.gr_sasrec_train_tiled_fwd_f32 if which == "fwd" else lib.gr_sasrec_train_tiled_bwd_f32
    pp = ctypes.byref(p) if p is not None else None
    bb = ctypes.byref(bufs) if bufs is not None else None
    # fwd: (..., out, err_flag, ws, bytes, stream); bwd: (..., d_out, g_item, ws, bytes, stream)
    rc = fn(pp, seqs, B, n, p_drop, 0, None, bb, io, None, ws, ws_bytes, None)
    return rc, lib.gr_last_error()


def test_size_queries():
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    p = _params(L)
    w1 = lib.gr_sasrec_train_tiled_workspace_bytes(ctypes.byref(p), 1, 200)
    w8 = lib.gr_sasrec_train_tiled_workspace_bytes(ctypes.byref(p), 8, 200)
    w128 = lib.gr_sasrec_train_tiled_workspace_bytes(ctypes.byref(p), 128, 200)
    # at least the residual-stream gradient, a [rows, d] temporary, dQ|dK|dV and P', dS of one block
    assert w1 >= 4 * (200 * (2 * 128 + 3 * 128) + 2 * 200 * 200)
    assert w1 < w8 < w128
    assert w128 < 2 ** 30                                   # the C5 batch: well under a GiB
    assert lib.gr_sasrec_train_tiled_workspace_bytes(None, 8, 200) == 0
    for B, n in ((1, 1), (2, 64), (70, 20), (128, 200), (4096, 256)):
        s = lib.gr_sasrec_train_tiled_parts(ctypes.byref(p), B, n)
        assert 1 <= s <= max(1, B * n)                      # never more partial rows than rows
        assert s <= 64                                      # and never one per sequence at scale
    assert lib.gr_sasrec_train_tiled_parts(ctypes.byref(p), 1, 1) == 1
    assert lib.gr_sasrec_train_tiled_parts(ctypes.byref(p), 128, 200) > 1
    assert lib.gr_sasrec_train_tiled_parts(None, 8, 200) == 0


def test_supported_is_the_union_of_both_envelopes():
    """ops.sasrec_train_supported: the per-sequence kernels' envelope, the tiled kernels' beyond it,
    nothing outside; a forced ``train_kernels`` narrows it to that set."""
    from gr_amd import SASRec, ops

    def model(d, max_len, H=1, mlp=64, nb=2):
        return SASRec(10, {"device": "cpu", "d": d, "max_len": max_len, "num_blocks": nb, "num_heads": H,
                           "dropout": 0.2, "mlp_layer": mlp, "layernorm_eps": 1e-8})

    small, large = model(64, 64, mlp=128), model(128, 256, mlp=256)
    assert ops.sasrec_train_supported(small, 64) and ops.sasrec_train_fits_sequence(small, 64)
    assert ops.sasrec_train_supported(large, 256) and not ops.sasrec_train_fits_sequence(large, 256)
    assert ops.sasrec_train_supported(large, 200)
    for bad, n in ((model(129, 20, H=1), 20), (model(128, 300), 257), (model(128, 50), 51),
                   (model(128, 50, mlp=257), 50), (model(128, 50, nb=9), 50)):
        assert not ops.sasrec_train_supported(bad, n)
    large.train_kernels = "sequence"
    assert not ops.sasrec_train_supported(large, 200)
    small.train_kernels = "tiled"
    assert ops.sasrec_train_supported(small, 64)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("what,kw,n,p_drop,code", [
    ("d 129", dict(d=129, H=1), 200, 0.2, GR_ERR_UNSUPPORTED),
    ("n 257", dict(max_len=300), 257, 0.2, GR_ERR_UNSUPPORTED),
    ("n > max_len", dict(max_len=50), 51, 0.2, GR_ERR_UNSUPPORTED),
    ("mlp 257", dict(mlp=257), 200, 0.2, GR_ERR_UNSUPPORTED),
    ("d % H", dict(d=128, H=3), 200, 0.2, GR_ERR_UNSUPPORTED),
    ("0 blocks", dict(nb=0), 200, 0.2, GR_ERR_UNSUPPORTED),
    ("9 blocks", dict(nb=9), 200, 0.2, GR_ERR_UNSUPPORTED),
    ("p_drop 1", dict(), 200, 1.0, GR_ERR_ARG),
])
def test_launchers_refuse_shapes_outside_the_envelope(which, what, kw, n, p_drop, code):
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    rc, msg = _call(lib, which, _params(L, **kw), _bufs(L), n=n, p_drop=p_drop, ws_bytes=1 << 40)
    assert rc == code, (what, rc, msg)
    assert msg and b"gr_sasrec_train_tiled" in msg, (what, msg)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_launchers_refuse_null_buffers_and_short_workspace(which):
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    p = _params(L)
    cases = [dict(p=None, bufs=_bufs(L)), dict(p=p, bufs=None), dict(p=p, bufs=_bufs(L), seqs=None),
             dict(p=p, bufs=_bufs(L), io=None), dict(p=p, bufs=_bufs(L), ws=None),
             dict(p=p, bufs=_bufs(L, prob=None)), dict(p=p, bufs=_bufs(L, xl=None))]
    if which == "bwd":
        cases.append(dict(p=p, bufs=_bufs(L, g_vec=None)))
    for kw in cases:
        rc, msg = _call(lib, which, kw.pop("p"), kw.pop("bufs"), **kw)
        assert rc == GR_ERR_ARG and msg, (kw, rc, msg)
    need = lib.gr_sasrec_train_tiled_workspace_bytes(ctypes.byref(p), 4, 200)
    for short in (0, need - 1):
        rc, msg = _call(lib, which, p, _bufs(L), ws_bytes=short)
        assert rc == GR_ERR_WORKSPACE and b"workspace" in msg, (short, rc, msg)
    # B * n past 2^31 rows is an argument error, not an overflow
    rc, msg = _call(lib, which, p, _bufs(L), B=2 ** 31, n=200, ws_bytes=1 << 60)
    assert rc == GR_ERR_ARG and msg
