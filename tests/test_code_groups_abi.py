"""Semantic-ID emission on the device, host side (CPU: no kernel is launched here): the C-ABI entry
points of csrc/codes.hip, their argument checks, the ``grouping`` switch of ``generate_codes``, and
the vectorised numpy reference that tests/test_code_groups_gpu.py uses where ``infer.dedup_codes``
(quadratic in the number of shared codes) is too slow."""
import ctypes

import numpy as np
import pytest

NAMES = ["gr_code_groups_workspace_bytes", "gr_code_groups_i64", "gr_code_segments_i64"]
EDGE_N = [0, 1, 2, 63, 64, 65, 257, 4099]
EDGE_L = [1, 3, 8]


def group_reference(codes):
    """(leader, count, digit) per row of ``codes`` [n, L]: a stable argsort of the inverse index of
    ``np.unique(axis=0)`` lists every code's rows in row order, so a row's digit is its position in
    that list minus the list's start and its leader is the list's first row."""
    codes = np.asarray(codes)
    n = len(codes)
    if n == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z.copy(), z.copy()
    _, inv, cnt = np.unique(codes, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    starts = np.cumsum(cnt) - cnt
    digit = np.empty(n, dtype=np.int64)
    digit[order] = np.arange(n) - np.repeat(starts, cnt)
    return order[starts][inv].astype(np.int64), cnt[inv].astype(np.int64), digit


def dedup_reference(codes):
    """``infer.dedup_codes`` from ``group_reference``."""
    codes = np.asarray(codes)
    return np.hstack((codes, group_reference(codes)[2][:, None]))


def edge_codes(n, L, dense, seed=0):
    """Random codes for one edge shape: ``dense`` K^L ~ n / 2 (most rows collide), else K^L ~ 64 n."""
    target = max(n / 2, 1) if dense else 64 * max(n, 1)
    K = max(1, int(target ** (1.0 / L))) if dense else int(np.ceil(target ** (1.0 / L))) + 1
    rng = np.random.default_rng(1000 * n + 10 * L + int(dense) + seed)
    return rng.integers(0, K, size=(n, L)).astype(np.int64)


def test_symbols_exported_and_bound():
    import gr_amd
    from gr_amd import _lib
    handle = ctypes.CDLL(gr_amd.LIB_PATH)
    for name in NAMES:
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES, name
    assert hasattr(gr_amd.ops, "code_groups")
    from gr_amd import infer
    for name in ("collision_groups_device", "dedup_codes_device", "collision_rate"):
        assert callable(getattr(infer, name))


def test_workspace_query():
    import gr_amd
    lib = gr_amd.lib()
    last = 0
    for n in (0, 1, 2, 511, 512, 513, 4099, 100_000, 10_000_000, (1 << 31) - 1):
        nb = lib.gr_code_groups_workspace_bytes(n, 3)
        assert nb > 0 and nb >= last, (n, nb, last)
        assert nb >= 2 * n * 4                        # at least 2 n slots of a 32-bit row index
        assert nb >= 8 * ((n + 255) // 256)           # serves gr_code_segments_i64 too
        last = nb
    assert lib.gr_code_groups_workspace_bytes(100, 1) == lib.gr_code_groups_workspace_bytes(100, 16)
    for n, levels in ((-1, 3), (1 << 31, 3), (10, 0), (10, 17)):
        assert lib.gr_code_groups_workspace_bytes(n, levels) == 0


def test_bad_arguments_fail_on_the_host():
    import gr_amd
    lib = gr_amd.lib()
    p = 4096    # a non-null, aligned address: every call below returns before any device work
    need = lib.gr_code_groups_workspace_bytes(100, 3)
    ok = [p, 100, 3, p, p, p, p, p, p, need, None]
    for pos in (0, 3, 4, 5, 6, 7, 8):                 # each pointer in turn
        args = list(ok)
        args[pos] = None
        assert lib.gr_code_groups_i64(*args) == -1 and b"null" in lib.gr_last_error()
    for n, levels in ((100, 0), (100, -1), (100, 17), (1 << 31, 3), (-1, 3)):
        assert lib.gr_code_groups_i64(p, n, levels, p, p, p, p, p, p, 1 << 40, None) == -1
        assert b"bad shape" in lib.gr_last_error()
    assert lib.gr_code_groups_i64(p, 100, 3, p, p, p, p, p, p, need - 1, None) == -4
    assert b"workspace" in lib.gr_last_error()
    assert lib.gr_code_groups_i64(p, 100, 3, p, p, p, p, p, p + 4, need, None) == -1
    # n = 0: success, nothing launched, no pointer looked at
    assert lib.gr_code_groups_i64(None, 0, 3, None, None, None, None, None, None, 0, None) == 0
    assert lib.gr_last_error() == b""

    ok = [p, 100, p, p, p, p, p, p, 8, None]
    for pos in (0, 2, 3, 4, 5, 6, 7):
        args = list(ok)
        args[pos] = None
        assert lib.gr_code_segments_i64(*args) == -1 and b"null" in lib.gr_last_error()
    assert lib.gr_code_segments_i64(p, 1 << 31, p, p, p, p, p, p, 1 << 40, None) == -1
    assert lib.gr_code_segments_i64(p, -1, p, p, p, p, p, p, 1 << 40, None) == -1
    assert lib.gr_code_segments_i64(p, 257, p, p, p, p, p, p, 15, None) == -4
    assert lib.gr_code_segments_i64(None, 0, None, None, None, None, None, None, 0, None) == 0


def test_device_entry_points_refuse_cpu_tensors():
    import torch
    from gr_amd import infer, ops
    codes = torch.zeros((4, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.code_groups(codes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        infer.dedup_codes_device(codes)


def test_generate_codes_rejects_unknown_grouping():
    import inspect
    from gr_amd import infer
    with pytest.raises(ValueError, match="grouping"):
        infer.generate_codes(None, np.zeros((2, 4), dtype=np.float32), "cpu", grouping="gpu")
    assert inspect.signature(infer.generate_codes).parameters["grouping"].default == "host"
    assert inspect.signature(infer.infer).parameters["grouping"].default == "host"


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("L", EDGE_L)
def test_numpy_reference_equals_host_functions(L, dense):
    from gr_amd.infer import collision_groups, dedup_codes
    for n in EDGE_N:
        codes = edge_codes(n, L, dense)
        leader, count, digit = group_reference(codes)
        assert np.array_equal(dedup_reference(codes), dedup_codes(codes)), n
        groups = collision_groups(codes)
        got = {}
        for r in np.flatnonzero(count > 1):
            got.setdefault(int(leader[r]), []).append(int(r))
        assert [got[k] for k in sorted(got)] == groups, n
        assert all(count[g[0]] == len(g) and leader[g[-1]] == g[0] for g in groups)
    if dense:
        assert len(groups) > 100      # the dense shapes do collide
