"""gr_kmeans_f32's host-side surface (CPU) and the module opt-in.  Every call here passes NULL for
every pointer: the shape, argument and workspace checks come before the pointer check, and the
pointer check before any launch, so nothing can reach the device."""
import pytest
import torch

GR_ERR_ARG, GR_ERR_UNSUPPORTED, GR_ERR_WORKSPACE = -1, -2, -4


def _call(lib, n, e, K, ws_bytes=0, trials=0, max_iter=1, tol=1e-4):
    return lib.gr_kmeans_f32(None, n, e, K, None, 0, trials, max_iter, tol, None, None, None, None, None,
                             ws_bytes, None)


def test_workspace_query_and_envelope():
    import gr_amd
    lib = gr_amd.lib()
    small = lib.gr_kmeans_workspace_bytes(64, 32, 8)
    big = lib.gr_kmeans_workspace_bytes(100000, 32, 256)
    assert 0 < small < big
    assert big >= 3 * 4 * 100000                 # D^2, labels and distances per row
    for n, e, K in [(64, 0, 8), (64, 65, 8), (64, 32, 0), (2000, 32, 1025), (7, 32, 8), (2 ** 31, 8, 8), (0, 8, 1)]:
        assert lib.gr_kmeans_workspace_bytes(n, e, K) == 0, (n, e, K)
        assert lib.gr_kmeans_form(n, e, K) == -1
    assert lib.gr_kmeans_workspace_bytes(1025, 64, 1024) > 0
    assert lib.gr_kmeans_workspace_bytes(2 ** 31 - 1, 1, 1) > 0      # K <= n < 2^31


def test_launch_form_query():
    import gr_amd
    from gr_amd import _lib as L
    lib = gr_amd.lib()
    assert lib.gr_kmeans_form(64, 32, 8) == 1            # the reference's batch: one workgroup
    assert lib.gr_kmeans_form(256, 32, 32) == 1
    assert lib.gr_kmeans_form(257, 32, 8) == 0           # more than one tile of rows
    assert lib.gr_kmeans_form(100000, 32, 256) == 0
    L.set_option("kmeans_small", 0)
    try:
        assert lib.gr_kmeans_form(64, 32, 8) == 0
    finally:
        L.set_option("kmeans_small", 1)


def test_argument_checks_precede_the_pointers():
    import gr_amd
    lib = gr_amd.lib()
    assert _call(lib, 7, 32, 8) == GR_ERR_ARG and b"n_samples < n_clusters" in lib.gr_last_error()
    assert _call(lib, 64, 65, 8) == GR_ERR_UNSUPPORTED and b"1 <= e <= 64" in lib.gr_last_error()
    assert _call(lib, 2000, 32, 1025) == GR_ERR_UNSUPPORTED
    assert _call(lib, 2 ** 31, 8, 8) == GR_ERR_UNSUPPORTED
    assert _call(lib, 64, 32, 8, trials=17) == GR_ERR_UNSUPPORTED
    assert _call(lib, 64, 32, 8, max_iter=-1) == GR_ERR_ARG
    assert _call(lib, 64, 32, 8, tol=-1.0) == GR_ERR_ARG
    assert _call(lib, 64, 32, 8) == GR_ERR_WORKSPACE
    assert _call(lib, 64, 32, 8, ws_bytes=1 << 40) == GR_ERR_WORKSPACE      # a NULL workspace of any size


def test_option_kmeans_small():
    from gr_amd import _lib as L
    assert L.get_option("kmeans_small") == 1
    L.set_option("kmeans_small", 0)
    assert L.get_option("kmeans_small") == 0
    L.set_option("kmeans_small", 1)
    with pytest.raises(RuntimeError):
        L.set_option("kmeans_small", 2)


def test_module_opt_in_and_no_cpu_fallback():
    from gr_amd import RQVAE, ops
    m = RQVAE(in_dim=16, num_emb_list=[8, 8, 8], e_dim=16, layers=[32], kmeans_init=True, kmeans_iters=5,
              sk_epsilons=[0.0] * 3)
    assert all(q.kmeans_backend == "host" and q.kmeans_seed is None for q in m.rq.vq_layers)
    assert m.set_kmeans("device", seed=10) is m
    assert [(q.kmeans_backend, q.kmeans_seed) for q in m.rq.vq_layers] == [("device", 10), ("device", 11), ("device", 12)]
    m.set_kmeans("device")
    assert all(q.kmeans_seed is None for q in m.rq.vq_layers)
    with pytest.raises(ValueError):
        m.set_kmeans("gpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans(torch.zeros(20, 8), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.rq.vq_layers[0].init_emb(torch.zeros(20, 16))
    m.set_kmeans("host")
    assert all(q.kmeans_backend == "host" for q in m.rq.vq_layers)
    assert set(m.state_dict()) == set(RQVAE(in_dim=16, num_emb_list=[8, 8, 8], e_dim=16, layers=[32],
                                            sk_epsilons=[0.0] * 3).state_dict())
