"""gr_kmeans_f32 / ops.kmeans / RQVAE.set_kmeans("device") against the float64 restatement of
tests/kmeans_ref.py (itself pinned to scikit-learn by tests/test_kmeans_ref.py).

Every case runs in the tiled form (option ``kmeans_small`` 0) and, where ``gr_kmeans_form`` says the
shape fits it, in the one-workgroup form (option 1) as well.

Bars.  Labels: a device label is admissible when its fp64 squared distance exceeds the row's fp64
minimum by at most 2 (e + 4) 2^-24 (|x| + max_k |c_k|)^2, the fp32 dot-product bound for any
summation order; rows with more than one admissible label are asserted to be under 1 % of a case on
the reference side.  Centres: against the fp64 M step (relocation included) on the device's own
labels, within 4x the worst error of the plain fp32 numpy restatement of the same sums, measured
per case as a fraction of max |centre|."""
import functools
import os

import numpy as np
import pytest
import torch

import kmeans_ref as kr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans_sklearn.npz")
FORMS = ["one_workgroup", "tiled"]


def _fits(n, e, K):
    """True when the one-workgroup form takes the shape (asked of the library, default option)."""
    try:
        import gr_amd
        return gr_amd.lib().gr_kmeans_form(n, e, K) == 1
    except (RuntimeError, OSError):   # no library at collection time (gr_amd.lib() / CDLL): list both forms;
        return True                    # the tests then assert the form that runs, so a wrong guess fails


def _with_forms(shapes):
    """[(key, form)] over the launch forms each shape {key: (n, e, K)} can take."""
    return [(k, f) for k, v in shapes.items() for f in FORMS if f == "tiled" or _fits(*v)]


@pytest.fixture(params=FORMS)
def form(request):
    from gr_amd import _lib as L
    old = L.get_option("kmeans_small")
    L.set_option("kmeans_small", 1 if request.param == FORMS[0] else 0)
    yield request.param
    L.set_option("kmeans_small", old)


def _skip_form(form, n, e, K):
    """Inside a test that loops over shapes: the one-workgroup pass leaves out what it cannot take."""
    return form == FORMS[0] and not _fits(n, e, K)


def _rows(x, K, seed):
    return x[np.random.default_rng(seed).choice(len(x), K, replace=False)].astype(np.float64)


def _normal(n, e, seed):
    return np.random.default_rng(seed).standard_normal((n, e)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x float32, c0 float64) of a lockstep case."""
    if name.startswith("normal"):
        n, e, K = LOCKSTEP[name]
        x = _normal(n, e, 11)
        return x, _rows(x, K, 5)
    if name == "blobs_300x16_k16":     # two initial centres far from all rows: they start empty
        x, _, _ = kr.blobs(300, 16, 16, 0)
        c0 = _rows(x, 16, 1)
        c0[7] = c0[2] + 100.0
        c0[11] = c0[3] - 100.0
        return x, c0
    if name == "blobs_240x16_k16":     # the same within the one-workgroup form's reach
        x, _, _ = kr.blobs(240, 16, 16, 0)
        c0 = _rows(x, 16, 1)
        c0[7] = c0[2] + 30.0
        c0[11] = c0[3] - 30.0
        return x, c0
    if name == "blobs_2048x32_k64":    # random rows of 64 blobs: 3 then 2 empty clusters
        x, _, _ = kr.blobs(2048, 32, 64, 1)
        return x, _rows(x, 64, 2)
    raise KeyError(name)


LOCKSTEP = {"normal_64x32_k8": (64, 32, 8), "normal_1000x5_k7": (1000, 5, 7),
            "normal_513x64_k256": (513, 64, 256), "normal_4099x48_k33": (4099, 48, 33),
            "blobs_300x16_k16": (300, 16, 16), "blobs_2048x32_k64": (2048, 32, 64),
            "blobs_240x16_k16": (240, 16, 16), "normal_256x5_k7": (256, 5, 7),
            "normal_n_eq_k": (40, 8, 40), "normal_k1": (100, 8, 1), "normal_e1": (200, 1, 5),
            "normal_1025x64_k1024": (1025, 64, 1024)}


def _band(x, c32, e):
    xn = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    cn = np.sqrt((c32.astype(np.float64) ** 2).sum(1)).max()
    return 2.0 * (e + 4) * 2.0 ** -24 * (xn + cn) ** 2


@functools.lru_cache(maxsize=None)
def _trajectory(name, max_steps=12):
    """The restatement's walk from c0, each step taken from the fp32 cast of its centres (what the
    device is given): [(c32, D, labels, dmin, band)]; computed once per case and left unchanged."""
    x, c0 = _case(name)
    c = c0
    prev, steps = None, []
    for _ in range(max_steps):
        c32 = c.astype(np.float32)
        D = kr.sqdist(x, c32)
        labels = D.argmin(1)
        dmin = D[np.arange(len(x)), labels]
        steps.append((c32, D, labels, dmin, _band(x, c32, x.shape[1])))
        if prev is not None and np.array_equal(labels, prev):
            break
        c, _ = kr.m_step(x, labels, dmin, c32.astype(np.float64))
        prev = labels
    return steps


def _run(xt, K, **kw):
    from gr_amd import ops
    r = ops.kmeans(xt, K, **kw)
    return (r.centers.cpu().numpy(), r.labels.cpu().numpy(), float(r.inertia.item()), int(r.n_iter.item()))


@pytest.mark.parametrize("name,form", _with_forms(LOCKSTEP), indirect=["form"])
def test_lockstep_lloyd_against_float64(name, form, dev):
    import gr_amd
    x, c0 = _case(name)
    n, e = x.shape
    K = len(c0)
    assert (n, e, K) == LOCKSTEP[name]
    assert gr_amd.lib().gr_kmeans_form(n, e, K) == (1 if form == FORMS[0] else 0)   # the form under test runs
    xt = torch.from_numpy(x).to(dev)
    worst_c, worst_tol, ambiguous, empties, moved = 0.0, 0.0, 0, 0, 0
    for c32, D, ref_labels, ref_dmin, band in _trajectory(name):
        # reference side: rows with more than one admissible label are rare
        multi = ((D - ref_dmin[:, None]) <= band[:, None]).sum(1) > 1
        ambiguous = max(ambiguous, int(multi.sum()))
        assert multi.mean() <= 0.01
        ct = torch.from_numpy(c32).to(dev)
        _, lab, inertia, it0 = _run(xt, K, max_iter=0, init=ct)          # the E step alone
        assert it0 == 0
        d_dev = D[np.arange(n), lab]
        assert (d_dev - ref_dmin <= band).all(), "a device label outside the fp32 band of the minimum"
        moved += int((lab != ref_labels).sum())
        assert abs(inertia - d_dev.sum()) <= 1e-5 * max(d_dev.sum(), 1e-30)
        cen, _, _, it1 = _run(xt, K, max_iter=1, tol=0.0, init=ct)       # E + M (+ relocation)
        assert it1 == 1
        c64, n_empty = kr.m_step(x, lab, d_dev, c32.astype(np.float64))
        c_np32, _ = kr.m_step(x, lab, d_dev, c32, dtype=np.float32)
        scale = np.abs(c64).max()
        tol = 4.0 * np.abs(c_np32.astype(np.float64) - c64).max() / scale
        err = np.abs(cen.astype(np.float64) - c64).max() / scale
        empties += n_empty
        worst_c, worst_tol = max(worst_c, err), max(worst_tol, tol)
        assert err <= tol, (err, tol)
    print(f"\n{name} [{form}]: {len(_trajectory(name))} steps, centre error {worst_c:.3g} (bar up to {worst_tol:.3g}), "
          f"{empties} empty clusters relocated, {moved} labels moved inside the band, "
          f"at most {ambiguous} ambiguous rows")
    if name.startswith("blobs"):
        assert empties >= 1, "the case is meant to meet empty clusters"


def test_common_offset(form, dev):
    """512 x 32, 8 blobs (spread 1, noise 0.1) plus 1e4: the labels are the planted ones at every
    step (the |x|^2 + |c|^2 - 2 x.c form mislabels most rows here) and the centres hold the bar."""
    x, planted, _ = kr.blobs(512, 32, 8, 4, spread=1.0, noise=0.1, offset=1e4)
    xt = torch.from_numpy(x).to(dev)
    c = x[:8].astype(np.float64)               # one row of each blob (row i belongs to blob i % 8)
    for step in range(3):
        c32 = c.astype(np.float32)
        D = kr.sqdist(x, c32)
        ref_labels = D.argmin(1)
        dmin = D[np.arange(512), ref_labels]
        margin = np.partition(D, 1, axis=1)
        assert (margin[:, 1] - margin[:, 0]).min() > 0.5 and np.array_equal(ref_labels, planted)
        ct = torch.from_numpy(c32).to(dev)
        _, lab, _, _ = _run(xt, 8, max_iter=0, init=ct)
        assert np.array_equal(lab, planted), f"step {step}: {(lab != planted).sum()} of 512 rows mislabelled"
        cen, _, _, _ = _run(xt, 8, max_iter=1, tol=0.0, init=ct)
        c64, _ = kr.m_step(x, lab, dmin, c32.astype(np.float64))
        c_np32, _ = kr.m_step(x, lab, dmin, c32, dtype=np.float32)
        scale = np.abs(c64).max()
        tol = 4.0 * np.abs(c_np32.astype(np.float64) - c64).max() / scale
        assert np.abs(cen.astype(np.float64) - c64).max() / scale <= tol
        c = c64


# (n, e, K, spread, data seed, init seed): margins above 1e-3 at every step of the fp64 run
# (the two low-dimensional cases are where the shift rule fires first; (256, 1, 2) fits one workgroup)
WHOLE = [(300, 16, 16, 4.0, 0, 0), (2048, 32, 64, 4.0, 0, 1), (1024, 2, 2, 1.0, 2, 0), (256, 1, 2, 1.0, 2, 0)]


@functools.lru_cache(maxsize=None)
def _whole(i):
    n, e, K, spread, ds, s = WHOLE[i]
    x, _, _ = kr.blobs(n, e, K, ds, spread=spread)
    c0 = _rows(x, K, s)
    return x, c0, kr.lloyd(x, c0, 50, 0.0), kr.lloyd(x, c0, 50, 1e-4)


def test_whole_run_from_init(form, dev):
    fired = []
    for i in range(len(WHOLE)):
        if _skip_form(form, *WHOLE[i][:3]):
            continue
        x, c0, ref, ref_tol = _whole(i)
        K = len(c0)
        assert min(s.margin.min() for s in ref.steps) > 1e-3
        xt = torch.from_numpy(x).to(dev)
        ct = torch.from_numpy(c0.astype(np.float32)).to(dev)
        cen, lab, inertia, n_iter = _run(xt, K, max_iter=50, tol=0.0, init=ct)
        assert n_iter == ref.n_iter and np.array_equal(lab, ref.labels)
        assert abs(inertia - ref.inertia) <= 1e-5 * ref.inertia
        # iterations past convergence leave everything untouched
        cen2, lab2, inertia2, n2 = _run(xt, K, max_iter=n_iter, tol=0.0, init=ct)
        assert n2 == n_iter and np.array_equal(cen2.view(np.uint32), cen.view(np.uint32))
        assert np.array_equal(lab2, lab) and inertia2 == inertia
        _, _, _, n_tol = _run(xt, K, max_iter=50, tol=1e-4, init=ct)
        assert n_tol <= n_iter and n_tol == ref_tol.n_iter
        fired.append(ref_tol.rule)
        print(f"\n{WHOLE[i][:3]} [{form}]: n_iter {n_iter} (tol 0), {n_tol} (tol 1e-4, rule '{ref_tol.rule}'), "
              f"inertia {inertia:.6g}")
    assert "shift" in fired


def _match_rows(cen, x):
    """Row index of each centre in x by exact bits (-1: none)."""
    eq = (cen[:, None, :].view(torch.int32) == x[None, :, :].view(torch.int32)).all(-1)
    return torch.where(eq.any(1), eq.float().argmax(1), torch.full_like(eq[:, 0], -1, dtype=torch.int64))


SEEDING = {"64x32_k8": (64, 32, 8), "250x5_k7": (250, 5, 7), "1000x5_k7": (1000, 5, 7), "513x64_k256": (513, 64, 256),
           "4099x48_k33": (4099, 48, 33)}


@pytest.mark.parametrize("shape,form", _with_forms(SEEDING), indirect=["form"])
def test_seeding_contract_rows_distinct_reproducible(shape, form, dev):
    from gr_amd import ops
    n, e, K = SEEDING[shape]
    xt = torch.from_numpy(_normal(n, e, 21)).to(dev)
    a = ops.kmeans(xt, K, max_iter=0, seed=7)
    rows = _match_rows(a.centers, xt)
    assert (rows >= 0).all(), "a seeded centre is not a data row"
    assert len(set(rows.tolist())) == K, "seeded centres repeat a row"
    b = ops.kmeans(xt, K, max_iter=0, seed=7)
    assert torch.equal(a.centers, b.centers) and torch.equal(a.labels, b.labels)
    c = ops.kmeans(xt, K, max_iter=0, seed=8)
    assert not torch.equal(a.centers, c.centers)
    # the whole run: same seed, same bits (an order-dependent reducer fails here)
    runs = [ops.kmeans(xt, K, max_iter=8, seed=3) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r.centers, runs[0].centers) and torch.equal(r.labels, runs[0].labels)
        assert torch.equal(r.n_iter, runs[0].n_iter) and torch.equal(r.inertia, runs[0].inertia)


def test_forms_agree_bitwise(dev):
    """Both launch forms run the same phase code in the same order."""
    from gr_amd import _lib as L, ops
    old = L.get_option("kmeans_small")
    try:
        for n, e, K in [(64, 32, 8), (256, 5, 7), (200, 16, 16), (128, 32, 64)]:
            xt = torch.from_numpy(_normal(n, e, 2)).to(dev)
            out = []
            for v in (1, 0):
                L.set_option("kmeans_small", v)
                assert L.lib().gr_kmeans_form(n, e, K) == v
                out.append(ops.kmeans(xt, K, max_iter=10, seed=5))
            assert torch.equal(out[0].centers, out[1].centers) and torch.equal(out[0].labels, out[1].labels)
            assert torch.equal(out[0].n_iter, out[1].n_iter) and torch.equal(out[0].inertia, out[1].inertia)
    finally:
        L.set_option("kmeans_small", old)


def test_seeding_never_draws_a_chosen_row_again(form, dev):
    """40 rows with 5 distinct values, K = 8: the first five centres are the five values (a row with
    D^2 = 0 is never drawn while one with D^2 > 0 exists), the rest repeat them; all finite."""
    from gr_amd import ops
    vals = _normal(5, 6, 1)
    x = vals[np.arange(40) % 5]
    xt = torch.from_numpy(x).to(dev)
    for seed in range(8):
        r = ops.kmeans(xt, 8, max_iter=3, seed=seed)
        cen = r.centers.cpu().numpy()
        assert np.isfinite(cen).all()
        d = np.abs(cen[:, None, :] - vals[None]).max(-1)
        assert (d.min(1) <= 1e-6).all()
        assert len(set(d.argmin(1).tolist())) == 5, "fewer than the five distinct values were found"
        s = ops.kmeans(xt, 8, max_iter=0, seed=seed).centers.cpu().numpy()
        first5 = np.abs(s[:5, None, :] - vals[None]).max(-1).argmin(1)
        assert sorted(first5.tolist()) == [0, 1, 2, 3, 4]


def test_d2_sampling_distribution(form, dev):
    """trials = 1, K = 2 on 64 planted rows: over 2,000 fixed seeds the second centre's frequency
    follows D^2 / sum D^2 given the first centre (chi-square, significance 1e-4)."""
    from scipy import stats
    from gr_amd import ops
    x, _, _ = kr.blobs(64, 4, 4, 9, spread=2.0)
    xt = torch.from_numpy(x).to(dev)
    cens = torch.stack([ops.kmeans(xt, 2, max_iter=0, seed=s, trials=1).centers for s in range(2000)])
    rows = _match_rows(cens.reshape(-1, 4), xt).reshape(2000, 2).cpu().numpy()
    assert (rows >= 0).all()
    first, second = rows[:, 0], rows[:, 1]
    D = kr.sqdist(x, x)                                   # D[i] = D^2 of every row given first = i
    P = D / D.sum(1, keepdims=True)
    expected = P[first].sum(0)
    observed = np.bincount(second, minlength=64).astype(np.float64)
    assert expected.min() >= 5.0                          # every bin is large enough for the test
    chi2 = ((observed - expected) ** 2 / expected).sum()
    p = stats.chi2.sf(chi2, df=63)
    # the first centre is uniform over the rows
    f_obs = np.bincount(first, minlength=64).astype(np.float64)
    p_first = stats.chi2.sf(((f_obs - 2000 / 64) ** 2 / (2000 / 64)).sum(), df=63)
    print(f"\nD^2 sampling [{form}]: chi2 {chi2:.1f} (63 dof), p = {p:.3g}; first centre uniform p = {p_first:.3g}")
    assert p >= 1e-4 and p_first >= 1e-4


def test_quality_against_sklearn(form, dev):
    """Mean final inertia over 32 seeds against scikit-learn's over 32 random_states on the same
    data (tests/golden/make_golden_kmeans.py), max_iter = 50: not worse by more than 3 standard
    errors of the difference."""
    from gr_amd import ops
    g = np.load(GOLDEN)
    for tag, K in (("a", 8), ("b", 64)):
        x = g[f"x_{tag}"]
        if _skip_form(form, x.shape[0], x.shape[1], K):
            continue
        sk = g[f"inertia_{tag}"].astype(np.float64)
        xt = torch.from_numpy(x).to(dev)
        ours = torch.stack([ops.kmeans(xt, K, max_iter=50, seed=s).inertia for s in range(32)]).cpu().numpy()
        se = np.sqrt(ours.var(ddof=1) / len(ours) + sk.var(ddof=1) / len(sk))
        print(f"\nquality {x.shape} K={K} [{form}]: device mean inertia {ours.mean():.6g}, "
              f"scikit-learn {sk.mean():.6g}, standard error of the difference {se:.3g}")
        assert ours.mean() <= sk.mean() + 3.0 * se


# ---------------------------------------------------------------------------------------------------
# module level

def _rqvae(dev, seed=0, kmeans_seed=0):
    from gr_amd import RQVAE
    torch.manual_seed(seed)
    m = RQVAE(in_dim=768, num_emb_list=[8, 8, 8], e_dim=32, layers=[256, 128], dropout_prob=0.0,
              kmeans_init=True, kmeans_iters=10, sk_epsilons=[0.01] * 3, sk_iters=50).to(dev).train()
    return m.set_kmeans("device", seed=kmeans_seed)


def test_module_device_backend(dev):
    from gr_amd import ops
    m = _rqvae(dev)
    x = torch.randn(64, 768, generator=torch.Generator().manual_seed(1)).to(dev)
    assert all(not q.initted and q.kmeans_backend == "device" for q in m.rq.vq_layers)
    assert [q.kmeans_seed for q in m.rq.vq_layers] == [0, 1, 2]
    with torch.no_grad():
        z = m.encoder.train_forward(x)
    _rqvae(dev)(x)    # another model's first forward fills the per-shape host-side caches (group offsets)
    host = _rqvae(dev).set_kmeans("host")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")      # any device-to-host copy or synchronisation raises
    try:
        o, rq_loss, idx = m(x)
        # positive control: the mode does fire here -- the host backend's copy of the latents raises
        with pytest.raises(RuntimeError, match="synchronizing"):
            host(x)
        assert not host.rq.vq_layers[0].initted
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(q.initted for q in m.rq.vq_layers)
    want = ops.kmeans(z, 8, max_iter=10, seed=0).centers
    assert torch.equal(m.rq.vq_layers[0].embedding.weight.detach(), want)
    assert o.shape == x.shape and idx.shape == (64, 3) and int(idx.min()) >= 0 and int(idx.max()) < 8
    m2 = _rqvae(dev)
    m2(x)
    for a, b in zip(m.rq.vq_layers, m2.rq.vq_layers):
        assert torch.equal(a.embedding.weight, b.embedding.weight)
        assert torch.count_nonzero(a.embedding.weight) > 0


def test_module_train_graph_with_device_init(dev):
    from gr_amd import ops
    m = _rqvae(dev)
    opt = torch.optim.AdamW(m.parameters(), lr=torch.tensor(1e-3, device=dev), weight_decay=1e-4, capturable=True)
    x = torch.randn(64, 768, generator=torch.Generator().manual_seed(1)).to(dev)
    step = ops.RqTrainGraph(m, opt, x.clone())
    assert step.graph is not None and all(q.initted for q in m.rq.vq_layers)
    for _ in range(3):
        loss, recon, idx = step.replay()
    assert torch.isfinite(loss).item() and idx.shape == (64, 3)


def test_module_default_backend_is_sklearn(dev, monkeypatch):
    from gr_amd import RQVAE, ops

    def boom(*a, **k):
        raise AssertionError("the default k-means backend must not call ops.kmeans")
    monkeypatch.setattr(ops, "kmeans", boom)
    torch.manual_seed(0)
    m = RQVAE(in_dim=768, num_emb_list=[8, 8, 8], e_dim=32, layers=[256, 128], dropout_prob=0.0,
              kmeans_init=True, kmeans_iters=10, sk_epsilons=[0.01] * 3, sk_iters=50).to(dev).train()
    assert all(q.kmeans_backend == "host" for q in m.rq.vq_layers)
    m(torch.randn(64, 768, device=dev))
    assert all(q.initted for q in m.rq.vq_layers)
    with pytest.raises(AssertionError, match="must not call"):
        m2 = RQVAE(in_dim=768, num_emb_list=[8], e_dim=32, layers=[256, 128], kmeans_init=True, kmeans_iters=10,
                   sk_epsilons=[0.01]).to(dev).train().set_kmeans("device")
        m2(torch.randn(64, 768, device=dev))


def test_argument_errors(dev):
    from gr_amd import RQVAE, ops
    with pytest.raises(ValueError, match="n_clusters"):
        ops.kmeans(torch.zeros(4, 8, device=dev), 8)
    with pytest.raises(RuntimeError, match="envelope"):
        ops.kmeans(torch.zeros(200, 65, device=dev), 8)
    with pytest.raises(RuntimeError, match="envelope"):
        ops.kmeans(torch.zeros(2000, 8, device=dev), 1025)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans(torch.zeros(20, 8), 4)
    # a workspace that is not 16-byte aligned is refused (real device memory: the check precedes any launch)
    from gr_amd import _lib as L
    lib = L.lib()
    x, cen = torch.zeros(64, 8, device=dev), torch.empty(4, 8, device=dev)
    nbytes = lib.gr_kmeans_workspace_bytes(64, 8, 4)
    wsp = L.workspace(nbytes + 16, dev)
    rc = lib.gr_kmeans_f32(L.ptr(x), 64, 8, 4, None, 0, 0, 1, 1e-4, L.ptr(cen), None, None, None,
                           wsp.data_ptr() + 4, nbytes, None)
    assert rc == -1 and b"aligned" in lib.gr_last_error()
    assert ops.kmeans(x, 4, with_labels=False).labels is None
    m = RQVAE(in_dim=768, num_emb_list=[8], e_dim=32, layers=[256, 128], kmeans_init=True, kmeans_iters=10,
              sk_epsilons=[0.01]).to(dev).train().set_kmeans("device", seed=0)
    with pytest.raises(ValueError, match="n_clusters"):
        m(torch.randn(4, 768, device=dev))
