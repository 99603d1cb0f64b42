"""Fixture for tests/test_kmeans_gpu.py::test_quality_against_sklearn: two standard-normal data sets
and scikit-learn's final inertia on each for 32 values of random_state, as the reference calls it
(RQ-VAE/models/layers.py:69-82: KMeans(n_clusters, max_iter), everything else default), max_iter 50.

    python tests/golden/make_golden_kmeans.py   ->  tests/golden/kmeans_sklearn.npz
"""
import os

import numpy as np
import sklearn
from sklearn.cluster import KMeans

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for tag, (n, e, K, seed) in {"a": (64, 32, 8, 100), "b": (2048, 32, 64, 101)}.items():
        x = np.random.default_rng(seed).standard_normal((n, e)).astype(np.float32)
        out[f"x_{tag}"] = x
        out[f"inertia_{tag}"] = np.array([KMeans(n_clusters=K, max_iter=50, random_state=s).fit(x).inertia_
                                          for s in range(32)], np.float64)
        print(tag, x.shape, K, out[f"inertia_{tag}"].mean(), out[f"inertia_{tag}"].std(ddof=1))
    np.savez_compressed(os.path.join(HERE, "kmeans_sklearn.npz"), **out)


if __name__ == "__main__":
    main()
