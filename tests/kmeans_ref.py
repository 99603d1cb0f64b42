"""float64 restatement of the k-means that ``gr_kmeans_f32`` computes (include/gr_amd.h): scikit-learn's
``KMeans(n_clusters, init=c0, n_init=1, max_iter, tol)`` Lloyd loop -- E step, M step, empty-cluster
relocation with the pairing fixed, both stop rules.  numpy only; shared by tests/test_kmeans_ref.py
(against scikit-learn itself) and tests/test_kmeans_gpu.py (against the kernels)."""
import collections

import numpy as np

Run = collections.namedtuple("Run", "centers labels inertia n_iter rule steps")
Step = collections.namedtuple("Step", "c_old labels dmin margin n_empty c_new shift")


def sqdist(x, c, chunk=256):
    """[n, K] squared distances in the direct form sum((x - c)^2), float64."""
    x = np.asarray(x, np.float64)
    c = np.asarray(c, np.float64)
    out = np.empty((len(x), len(c)))
    for i in range(0, len(x), chunk):
        d = x[i:i + chunk, None, :] - c[None, :, :]
        out[i:i + chunk] = np.einsum("nkf,nkf->nk", d, d)
    return out


def e_step(x, c):
    """(labels, dmin, margin, D): first index of the minimum; margin = second smallest - smallest
    (inf when K = 1)."""
    D = sqdist(x, c)
    labels = D.argmin(1)
    dmin = D[np.arange(len(D)), labels]
    if D.shape[1] > 1:
        part = np.partition(D, 1, axis=1)
        margin = part[:, 1] - part[:, 0]
    else:
        margin = np.full(len(D), np.inf)
    return labels, dmin, margin, D


def m_step(x, labels, dmin, c_old, dtype=np.float64):
    """Means of the members with scikit-learn's relocation (_relocate_empty_clusters_dense), the
    pairing fixed: the empty clusters in ascending id, the j-th taking the j-th farthest row (dmin
    descending, ties to the lower row), which leaves its donor's sum and count; labels stay; a
    cluster whose count ends at 0 keeps its old centre.  ``dtype`` float32 gives the plain fp32
    restatement of the same sums (the tolerance yardstick of the GPU tests).
    Returns (c_new, n_empty)."""
    x = np.asarray(x, dtype)
    K = len(c_old)
    sums = np.zeros((K, x.shape[1]), dtype)
    np.add.at(sums, labels, x)
    cnt = np.bincount(labels, minlength=K).astype(np.int64)
    empty = np.flatnonzero(cnt == 0)
    if len(empty):
        order = np.lexsort((np.arange(len(dmin)), -np.asarray(dmin, np.float64)))   # dmin desc, row asc
        for j, k in enumerate(empty):
            far = order[j]
            donor = labels[far]
            sums[donor] -= x[far]
            cnt[donor] -= 1
            sums[k] = x[far]
            cnt[k] = 1
    c_new = np.array(c_old, dtype)
    live = cnt > 0
    c_new[live] = sums[live] / cnt[live, None].astype(dtype)
    return c_new, len(empty)


def tolerance(x, tol):
    """scikit-learn's _tolerance: tol * mean over features of var(x)."""
    return tol * np.mean(np.var(np.asarray(x, np.float64), axis=0))


def lloyd(x, c0, max_iter, tol=0.0):
    """The whole run from the centres ``c0``: stop when an E step repeats the previous labels
    (rule "labels") or when the summed squared centre shift is <= tolerance(x, tol) (rule "shift");
    labels and inertia of the rows against the returned centres.  ``steps`` keeps every iteration
    (centres before, labels, distances, margins, empties, centres after, shift)."""
    x = np.asarray(x, np.float64)
    c = np.asarray(c0, np.float64).copy()
    thr = tolerance(x, tol)
    prev = np.full(len(x), -1)
    steps, rule, n_iter = [], None, 0
    for it in range(max_iter):
        labels, dmin, margin, _ = e_step(x, c)
        c_new, n_empty = m_step(x, labels, dmin, c)
        shift = float(((c_new - c) ** 2).sum())
        steps.append(Step(c, labels, dmin, margin, n_empty, c_new, shift))
        c = c_new
        n_iter = it + 1
        if np.array_equal(labels, prev):
            rule = "labels"
            break
        if shift <= thr:
            rule = "shift"
            break
        prev = labels
    labels, dmin, _, _ = e_step(x, c)
    return Run(c, labels, float(dmin.sum()), n_iter, rule, steps)


def blobs(n, e, K, seed, spread=4.0, noise=1.0, offset=0.0):
    """Planted blobs: K centres ~ spread * N(0, 1), rows = centre[i % K] + noise * N(0, 1) + offset,
    float32.  Returns (x, planted labels, centres)."""
    rng = np.random.default_rng(seed)
    cen = spread * rng.standard_normal((K, e))
    lab = np.arange(n) % K
    x = cen[lab] + noise * rng.standard_normal((n, e)) + offset
    return x.astype(np.float32), lab, cen
