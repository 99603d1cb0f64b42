"""The filtered quantizer's tile plan (csrc/rq_fused.h rq_filter_range, exported as
gr_rq_filter_plan): host arithmetic, checked without a GPU.

T tiles, of which the last ``left`` are the fused encoder's leftover tiles, over G workgroups:
workgroup b < left owns leftover tile T - left + b plus a contiguous range of main tiles, the other
workgroups split the remaining main tiles evenly in contiguous ranges, and no workgroup holds more
than RQ_W x GR_FMAXT = 16 tiles (the grid grows until that holds).  left = 0 is the plan the kernel
had before leftover tiles were merged into it: workgroup b takes [b T / G, (b + 1) T / G).

Swept: T in 1 .. 4 G + 3 for G in {4, 8, 256, 304}, every left in 0 .. min(G, T).
"""
import ctypes

import numpy as np
import pytest

CAP = 16   # RQ_W x GR_FMAXT


def _plans(T, G):
    """(grid[nl], begins[nl, M], counts[nl, M]) for left = 0 .. min(G, T); entries past a row's
    grid are zero."""
    from gr_amd import _lib
    f = _lib.lib().gr_rq_filter_plan
    nl, M = min(G, T) + 1, max(G, T)
    begins = np.zeros((nl, M), np.int32)
    counts = np.zeros((nl, M), np.int32)
    grid = np.zeros(nl, np.int32)
    pb, pc, pg = begins.ctypes.data, counts.ctypes.data, grid.ctypes.data
    for left in range(nl):
        rc = f(T, G, left, pb + 4 * M * left, pc + 4 * M * left, pg + 4 * left)
        assert rc == 0, (T, G, left, _lib.lib().gr_last_error())
    return grid, begins, counts


@pytest.mark.parametrize("G", [4, 8, 256, 304])
def test_plan_sweep(G):
    for T in range(1, 4 * G + 4):
        grid, begins, counts = _plans(T, G)
        nl, M = counts.shape
        left = np.arange(nl)[:, None]
        b = np.arange(M)[None, :]
        live = b < grid[:, None]
        tag = f"T {T}, G {G}"
        assert (grid >= G).all() and (grid <= M).all(), tag
        assert (counts.sum(1) == T).all(), tag
        assert (counts[~live] == 0).all(), tag
        assert (counts <= CAP).all(), tag
        owner = live & (b < left)
        assert (counts[owner] >= 1).all(), tag
        main = counts - owner            # main tiles per workgroup
        assert (main >= 0).all(), tag
        # contiguous, disjoint, covering [0, T - left): every range starts where the one before ends
        ends = np.cumsum(main, 1)
        assert (begins[:, 0] == 0).all(), tag
        assert (begins[:, 1:][live[:, 1:]] == ends[:, :-1][live[:, 1:]]).all(), tag
        assert (ends[np.arange(nl), grid - 1] == T - np.arange(nl)).all(), tag
        # left = 0: the ranges the kernel had before
        g0 = int(grid[0])
        assert g0 == G, tag   # T <= 4 G + 3: nobody exceeds 16 tiles
        edges = (np.arange(g0 + 1, dtype=np.int64) * T) // g0
        assert (begins[0, :g0] == edges[:-1]).all() and (counts[0, :g0] == np.diff(edges)).all(), tag


def test_grid_grows_to_keep_sixteen_tiles():
    """More than 16 tiles per workgroup: the grid grows, as the launcher did before (ceil(T / 16) when
    there are no leftover tiles), and with leftover tiles until no range exceeds 16."""
    from gr_amd import _lib
    f = _lib.lib().gr_rq_filter_plan
    g = ctypes.c_int32()
    assert f(16 * 256 + 1, 256, 0, None, None, ctypes.byref(g)) == 0 and g.value == 257
    for T, G, left in [(16 * 256 + 40, 256, 40), (5000, 256, 255), (16 * 8, 8, 7)]:
        assert f(T, G, left, None, None, ctypes.byref(g)) == 0
        c = np.zeros(g.value, np.int32)
        bg = np.zeros(g.value, np.int32)
        assert f(T, G, left, bg.ctypes.data, c.ctypes.data, ctypes.byref(g)) == 0
        assert c.sum() == T and c.max() <= CAP and c[:left].min() >= 1 and g.value >= G


def test_invalid_left_is_refused():
    from gr_amd import _lib
    f = _lib.lib().gr_rq_filter_plan
    g = ctypes.c_int32()
    assert f(3, 8, 4, None, None, ctypes.byref(g)) != 0    # more leftover tiles than tiles
    assert f(0, 8, 0, None, None, ctypes.byref(g)) != 0
    assert f(10, 8, -1, None, None, ctypes.byref(g)) != 0
