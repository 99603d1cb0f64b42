"""tests/kmeans_ref.py -- the float64 restatement the GPU k-means is held to -- against scikit-learn
itself (the reference's own call, RQ-VAE/models/layers.py:69-82), and its relocation rule on a
planted case.  CPU only."""
import warnings

import numpy as np
import pytest

import kmeans_ref as kr

# (n, e, K, data seed, blob spread, init seed): inits are K distinct random rows, or (None) one row
# of each blob where random rows of 64 overlapping blobs always leave a cluster empty; these runs
# meet no empty cluster (scikit-learn leaves the pairing of several empties to argpartition's order)
CASES = [(64, 32, 8, 0, 4.0, 0), (300, 16, 16, 1, 4.0, 0), (2048, 32, 64, 2, 1.0, None)]


def _init_rows(x, K, seed):
    if seed is None:
        return x[:K].copy()
    return x[np.random.default_rng(seed).choice(len(x), K, replace=False)].copy()


@pytest.mark.parametrize("n,e,K,dseed,spread,iseed", CASES)
def test_restatement_equals_sklearn_from_the_same_init(n, e, K, dseed, spread, iseed):
    from sklearn.cluster import KMeans
    x, _, _ = kr.blobs(n, e, K, dseed, spread=spread)
    c0 = _init_rows(x, K, iseed)
    ref = kr.lloyd(x, c0, max_iter=50, tol=0.0)
    assert all(s.n_empty == 0 for s in ref.steps), "pick a seed whose run meets no empty cluster"
    sk = KMeans(K, init=c0, n_init=1, max_iter=50, tol=0).fit(x)
    err = np.abs(sk.cluster_centers_.astype(np.float64) - ref.centers).max()
    print(f"\n({n}, {e}, {K}): n_iter {ref.n_iter} / sklearn {sk.n_iter_}, centres within {err:.3g}")
    assert ref.n_iter == sk.n_iter_
    assert np.array_equal(ref.labels, sk.labels_)
    assert err <= 1e-5
    assert abs(ref.inertia - sk.inertia_) <= 1e-4 * ref.inertia


def test_tolerance_is_sklearns():
    from sklearn.cluster import _kmeans
    x, _, _ = kr.blobs(300, 16, 16, 1)
    assert np.isclose(kr.tolerance(x, 1e-4), _kmeans._tolerance(x, 1e-4), rtol=1e-6)


def test_shift_rule_stops_no_later_than_label_rule():
    x, _, _ = kr.blobs(2048, 32, 64, 5, spread=1.0)
    c0 = _init_rows(x, 64, 3)
    a = kr.lloyd(x, c0, max_iter=50, tol=0.0)
    b = kr.lloyd(x, c0, max_iter=50, tol=1e-4)
    assert b.n_iter <= a.n_iter


def test_relocation_planted_outlier():
    """One initial centre far from all data, one clear outlier row: the empty cluster takes the
    outlier, and the donor's mean excludes it."""
    rng = np.random.default_rng(0)
    a = rng.standard_normal((20, 4)) * 0.1
    b = rng.standard_normal((20, 4)) * 0.1 + 5.0
    out = np.full((1, 4), 9.0)                       # nearest to blob b's centre, far from it
    x = np.concatenate([a, b, out]).astype(np.float32)
    c0 = np.array([[0.0] * 4, [5.0] * 4, [-100.0] * 4])
    labels, dmin, _, _ = kr.e_step(x, c0)
    assert (labels != 2).all() and labels[40] == 1 and dmin.argmax() == 40
    c1, n_empty = kr.m_step(x, labels, dmin, c0)
    assert n_empty == 1
    assert np.allclose(c1[2], x[40])                                   # the empty cluster took the outlier
    assert np.allclose(c1[1], x[20:40].astype(np.float64).mean(0))     # the donor's mean excludes it
    assert np.allclose(c1[0], x[:20].astype(np.float64).mean(0))
    # scikit-learn agrees where its pairing is determined (one empty cluster)
    from sklearn.cluster import KMeans
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = KMeans(3, init=c0, n_init=1, max_iter=1, tol=0).fit(x)
    assert np.abs(sk.cluster_centers_ - c1).max() <= 1e-5


def test_relocation_several_empties_pairing_and_emptied_donor():
    """Two empties take the two farthest rows in order (ties to the lower row); a donor left with
    no member keeps its old centre; nothing divides by zero."""
    x = np.array([[0.0], [0.0], [10.0], [4.0], [4.0]], np.float32)
    c0 = np.array([[0.0], [9.0], [50.0], [60.0]])     # clusters 2 and 3 start empty
    labels, dmin, _, _ = kr.e_step(x, c0)
    assert labels.tolist() == [0, 0, 1, 0, 0]
    assert dmin.tolist() == [0.0, 0.0, 1.0, 16.0, 16.0]
    c1, n_empty = kr.m_step(x, labels, dmin, c0)
    assert n_empty == 2
    assert c1[2, 0] == 4.0 and c1[3, 0] == 4.0          # rows 3 then 4 (tie: lower row first)
    assert c1[0, 0] == 0.0 and c1[1, 0] == 10.0
    c2, _ = kr.m_step(x[2:3], np.array([0]), np.array([1.0]), np.array([[9.0], [70.0]]))
    assert c2[1, 0] == 10.0 and c2[0, 0] == 9.0         # the donor emptied: it keeps its old centre
    assert np.isfinite(c2).all()
