"""Collision groups and dedup digit on the GPU (csrc/codes.hip, ops.code_groups) against the host
functions they stand in for: ``infer.collision_groups`` (RQ-VAE/infer.py:29-41) and
``infer.dedup_codes`` (infer.py:139-162).  Pure integer work: every comparison is array_equal."""
import collections

import numpy as np
import pytest
import torch

import golden_lib as gl
from test_code_groups_abi import EDGE_L, EDGE_N, dedup_reference, edge_codes, group_reference
from test_rq_sk_oracle import _case

pytestmark = pytest.mark.gpu


def host_groups(codes):
    from gr_amd.infer import collision_groups
    groups = collision_groups(codes)
    rows = np.concatenate(groups).astype(np.int64) if groups else np.zeros(0, dtype=np.int64)
    return rows, np.array([len(g) for g in groups], dtype=np.int64)


def host_stats(codes):
    c = collections.Counter(map(tuple, np.asarray(codes).tolist()))
    shared = [v for v in c.values() if v > 1]
    return [len(c), max(c.values()) if c else 0, sum(shared), len(shared)]


def check(codes, dev, digits="host"):
    """One device run of ``codes`` against the host functions; returns the CodeGroups."""
    from gr_amd import infer, ops
    t = torch.from_numpy(codes).to(dev)
    g = ops.code_groups(t)
    rows, sizes = host_groups(codes)
    assert g.rows.dtype == g.sizes.dtype == g.digit.dtype == g.leader.dtype == g.count.dtype == torch.int64
    assert np.array_equal(g.rows.cpu().numpy(), rows)
    assert np.array_equal(g.sizes.cpu().numpy(), sizes)
    final = infer.dedup_codes(codes) if digits == "host" else dedup_reference(codes)
    assert np.array_equal(g.digit.cpu().numpy(), final[:, -1])
    leader, count, _ = group_reference(codes)
    assert np.array_equal(g.leader.cpu().numpy(), leader)
    assert np.array_equal(g.count.cpu().numpy(), count)
    hs = host_stats(codes)
    assert g.stats.cpu().tolist() == hs
    st, host_sizes = g.host()
    assert list(st) == hs and np.array_equal(host_sizes, sizes)
    # the thin wrappers of infer
    r2, s2 = infer.collision_groups_device(t)
    assert np.array_equal(r2.cpu().numpy(), rows) and np.array_equal(s2.cpu().numpy(), sizes)
    assert np.array_equal(infer.dedup_codes_device(t).cpu().numpy(), final)
    n = len(codes)
    assert infer.collision_rate(t) == ((n - hs[0]) / n if n else 0.0)
    return g


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("L", EDGE_L)
@pytest.mark.parametrize("n", EDGE_N)
def test_edge_shapes(n, L, dense, dev):
    check(edge_codes(n, L, dense), dev)


def test_all_rows_equal(dev):
    n = 4099
    g = check(np.full((n, 3), 7, dtype=np.int64), dev)
    assert g.sizes.cpu().tolist() == [n]
    assert np.array_equal(g.digit.cpu().numpy(), np.arange(n))
    assert np.array_equal(g.rows.cpu().numpy(), np.arange(n))


def test_all_rows_distinct(dev):
    n = 4099
    codes = np.stack([np.arange(n) // 64, np.arange(n) % 64, np.zeros(n, dtype=np.int64)], 1).astype(np.int64)
    g = check(codes[np.random.default_rng(3).permutation(n)], dev)
    assert g.rows.numel() == 0 and g.sizes.numel() == 0
    assert not g.digit.any().item()


@pytest.mark.parametrize("offset", [0, 1 << 40])
def test_no_packing_shortcut(offset, dev):
    """L = 8 with values up to 1023 is 80 bits of code: rows that differ only in the first level, only
    in the last level, or only above bit 32 of one level must stay apart, exact copies must meet."""
    rng = np.random.default_rng(5)
    base = rng.integers(0, 1024, size=(300, 8)).astype(np.int64)
    base[0, :] = 1023                                   # the largest value at every level
    first, last, high = base.copy(), base.copy(), base.copy()
    first[:, 0] = (first[:, 0] + 1 + rng.integers(0, 1023, 300)) % 1024
    last[:, 7] = (last[:, 7] + 1 + rng.integers(0, 1023, 300)) % 1024
    high[:, 3] += np.int64(1) << 32
    codes = np.concatenate([base, first, last, high, base[:100], first[50:120], last[200:]]) + np.int64(offset)
    codes = codes[rng.permutation(len(codes))]
    g = check(codes, dev)
    assert g.host()[0][1] == 2                          # the copies pair up, nothing else meets


def test_many_workgroups_and_long_probe_chains(dev):
    """200,000 rows over 64,000 codes: 782 workgroups, nearly every row shared, clusters in the table."""
    from gr_amd import ops
    codes = np.random.default_rng(7).integers(0, 40, size=(200_000, 3)).astype(np.int64)
    g = check(codes, dev, digits="numpy")
    assert g.host()[0][2] > 0.9 * len(codes)
    h = ops.code_groups(torch.from_numpy(codes).to(dev))
    for a, b in ((g.rows, h.rows), (g.sizes, h.sizes), (g.digit, h.digit), (g.leader, h.leader),
                 (g.count, h.count), (g.stats, h.stats)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["rq_sk_csv_3x8", "rq_sk_syn_3x16"])
def test_generate_codes_device_grouping_end_to_end(name, dev):
    from gr_amd import RQVAE
    from gr_amd.infer import collision_rate, generate_codes
    x, _, _, _, out, meta = _case(name)
    sd, _, _ = gl.load(name)

    def model():
        m = RQVAE(in_dim=768, num_emb_list=[meta["K"]] * meta["L"], e_dim=32, layers=[256, 128],
                  dropout_prob=0.1, sk_epsilons=[0.01] * meta["L"], sk_iters=meta["sk_iters"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        return m.to(dev).eval()

    logs = {"host": [], "device": []}
    h_codes, h_final, h_stats = generate_codes(model(), x, dev, log=logs["host"].append)
    d_codes, d_final, d_stats = generate_codes(model(), x, dev, log=logs["device"].append, grouping="device")
    assert type(d_codes) is type(h_codes) and type(d_final) is type(h_final)
    assert d_codes.dtype == h_codes.dtype and d_final.dtype == h_final.dtype
    assert np.array_equal(d_codes, h_codes) and np.array_equal(d_final, h_final)
    assert d_stats == h_stats
    assert logs["device"] == logs["host"]
    # the reference's own outputs
    assert np.array_equal(d_codes, out["codes"]) and np.array_equal(d_final, out["final"])
    assert d_stats["rounds"] == meta["rounds"]
    assert sum(int(s.split()[3]) for s in logs["device"]) == meta["groups"]
    assert collision_rate(torch.from_numpy(d_codes).to(dev)) == d_stats["collision_rate"]
