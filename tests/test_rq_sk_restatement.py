"""The two Sinkhorn references of oracle/rq_oracle.py against each other, on the CPU, at every shape
tests/test_rq_sk_shapes_gpu.py runs the kernel at (this module owns the case list and the cached
references; the GPU module imports them).

``quantize_sk`` is the exact bar: torch's CPU fp32 distances and the float64 Sinkhorn of
layers.py:85-108 in this host's order.  ``quantize_sk_fp64`` is the host-independent bar: float64
from the inputs on, with a per-row, per-level margin; a row is certified when its margin exceeds
rq_oracle.SK_LOG_MARGIN (1e-2, Sinkhorn levels) / SK_ARGMIN_MARGIN (1e-4, argmin levels) on every
level.  The thresholds come from the formats, not from any result: an fp32 distance of e <= 64
terms carries at most about (e + 2) 2^-24 (|r|^2 + |c|^2) < 1e-5 relative error, a tenth of the
argmin threshold; on a Sinkhorn level that error, centred (amplitude of order |d|) and divided by
eps >= 0.003, moves log Q by about 1e-4 or less, a hundredth of the log threshold.

Groups with fewer rows than codes (B < K, the production collision re-encode: 2..5 rows against
256 codes) are a regime of their own: after a column normalisation most rows hold several entries
equal to within an ulp of a double, the top-two margin is 0 or ~1e-15, and the argmax is decided by
the first-index rule and the exact order of the float64 sums and divisions.  No row is certified
there, so only the exact bar speaks; this module asserts that the regime is what it claims to be.

Certified share per case, a CPU measurement of the two oracles alone on the committed seeds; each
floor is the worst share over three seeds of the same measurement, rounded down (a floor keeps the
certificate from hiding a failure, it is not a tolerance).  On every case both oracles agree on
EVERY row, certified or not.

  case                                             rows  certified  share   floor
  B64_e32_K8x8x8                                     64         64  1.000   0.95
  B65_e32_K8x12x256                                  65         50  0.769   0.60
  B64_e32_K256x5x9                                   64         34  0.531   0.35
  B17_e48_K33x16x1 (eps .01/0/.01)                   17         15  0.882   0.80
  B15_e32_K5x7x12                                    15         15  1.000   0.95
  B512_e32_K8x64 (eps .003)                         512        512  1.000   0.95
  B513_e5_K7x1024                                   513        505  0.984   0.90
  B1023_e32_K16                                    1023       1021  0.998   0.95
  B1024_e32_K16x9                                  1024       1022  0.998   0.95
  B1025_e32_K16x9                                  1025       1020  0.995   0.95
  B300_e32_K256x8x64 (eps .05/1/.003, 100 it)       300        271  0.903   0.85
  B130_e33_K100x24 (1 it)                           130        130  1.000   0.90
  B130_e33_K100x24 (0 it)                           130        130  1.000   0.90
  B2048_e32_K8                                     2048       2045  0.999   0.95
  B1500_e32_K64                                    1500       1499  0.999   0.95
  B64_e32_K8x8x8, inputs scaled by 3e-4              64         63  0.984   0.90
  B3_e32_K8x24x256 / B2_e64_K256x8 / B1_e32_K8x256 /
  B16_e32_K1024 / B64_e32_K1024                       -          0  0.000   none: exact bar only
  mixed groups, the 64-, 300- and 65-row groups      429        359  0.837   0.75
  pitch groups 1000 + 7 x 1 + 300                   1307       1293  0.989   0.95
"""
import functools

import pytest
import torch

from oracle import rq_oracle

SCALES = (0.8, 0.5, 0.3)


class Case:
    def __init__(self, B, e, Ks, eps=0.01, iters=50, floor=None, seed=None, scale=1.0, near_tie=False):
        self.B, self.e, self.Ks, self.iters, self.floor = B, e, list(Ks), iters, floor
        self.scale = scale          # z and the codebooks times this
        self.near_tie = near_tie    # B < K, yet most margins above 1e-9 (test_tie_regime_is_a_tie_regime)
        self.eps = [float(eps)] * len(Ks) if isinstance(eps, (int, float)) else [float(v) for v in eps]
        self.seed = seed if seed is not None else 7919 * B + 31 * e + sum(Ks) + iters
        self.id = f"B{B}_e{e}_K{'x'.join(map(str, Ks))}" + ("" if iters == 50 else f"_it{iters}") + \
            ("" if scale == 1.0 else f"_x{scale:g}")

    @property
    def tie_regime(self):       # fewer rows than codes on every Sinkhorn level
        return self.floor is None


# (B, e, Ks; eps 0.01 and 50 iterations unless noted) with the certified-share floor
CASES = [
    Case(64, 32, [8, 8, 8], floor=0.95),
    Case(65, 32, [8, 12, 256], floor=0.6),
    Case(64, 32, [256, 5, 9], floor=0.35),
    Case(17, 48, [33, 16, 1], eps=[0.01, 0.0, 0.01], floor=0.8),
    Case(15, 32, [5, 7, 12], floor=0.95),
    Case(512, 32, [8, 64], eps=0.003, floor=0.95),
    Case(513, 5, [7, 1024], floor=0.9),
    Case(1023, 32, [16], floor=0.95),
    Case(1024, 32, [16, 9], floor=0.95),
    Case(1025, 32, [16, 9], floor=0.95),
    Case(300, 32, [256, 8, 64], eps=[0.05, 1.0, 0.003], iters=100, floor=0.85),
    Case(130, 33, [100, 24], iters=1, floor=0.9),
    Case(130, 33, [100, 24], iters=0, floor=0.9),
    # the two big shapes of test_rq_sk_gpu.py: 2048 * 8 == lds_elems, and the workspace-resident matrix
    Case(2048, 32, [8], floor=0.95),
    Case(1500, 32, [64], floor=0.95),
    # distances of order 1e-6: the only inputs at which the + 1e-5 of the centring's amplitude is
    # more than an ulp of it (it is 90 % of it here; at |d| ~ 10..100 it moves d' by 3e-7)
    Case(64, 32, [8, 8, 8], floor=0.9, scale=3e-4),
    # B < K: the tie regime, exact bar only
    Case(3, 32, [8, 24, 256]),
    Case(2, 64, [256, 8]),
    Case(1, 32, [8, 256]),
    Case(16, 32, [1024]),
    Case(64, 32, [1024], near_tie=True),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def make_inputs(B, e, Ks, seed):
    """z = randn(B, e), codebooks randn(K, e) * (0.8, 0.5, 0.3) per level."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, e, generator=g)
    cbs = [torch.randn(K, e, generator=g) * SCALES[l % len(SCALES)] for l, K in enumerate(Ks)]
    return z, cbs


class Ref:
    """Both references of one group of rows: exact idx, fp64 idx, margin, certified rows."""

    def __init__(self, z, cbs, eps, iters):
        self.exact = rq_oracle.quantize_sk(z, cbs, eps, iters)
        self.fp64, self.margin = rq_oracle.quantize_sk_fp64(z, cbs, eps, iters)
        self.certified = rq_oracle.sk_certified(self.margin, eps)

    @property
    def share(self):
        return float(self.certified.double().mean())


@functools.lru_cache(maxsize=None)
def case_data(case_id):
    """(z, codebooks, Ref) of a case: computed once per session, shared, never written to."""
    c = BY_ID[case_id]
    z, cbs = make_inputs(c.B, c.e, c.Ks, c.seed)
    z, cbs = z * c.scale, [cb * c.scale for cb in cbs]
    return z, cbs, Ref(z, cbs, c.eps, c.iters)


def test_oracle_quantize_sk_is_the_level_chain():
    """quantize_sk = vq_level_sk level by level with rq.py:47's residual update."""
    c = BY_ID["B17_e48_K33x16x1"]
    z, cbs, ref = case_data(c.id)
    r, out = z.clone(), []
    for cb, eps in zip(cbs, c.eps):
        xq, ind = rq_oracle.vq_level_sk(r, cb, eps, c.iters)
        out.append(ind)
        r = r - xq
    assert torch.equal(ref.exact, torch.stack(out, -1))
    assert ref.exact.shape == (c.B, 3) and ref.exact.dtype == torch.int64
    assert bool(torch.isinf(ref.margin[:, 2]).all())                  # K = 1: nothing to choose
    assert bool((ref.exact[:, 2] == 0).all())


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_fp64_oracle_agrees_with_exact_oracle(cid):
    c = BY_ID[cid]
    _, _, ref = case_data(cid)
    differ = (ref.exact != ref.fp64).any(1)
    cert = ref.certified
    print(f"\n{cid}: rows {c.B} certified {int(cert.sum())} share {ref.share:.3f} floor {c.floor} "
          f"differ {int(differ.sum())} certified_differ {int((differ & cert).sum())}")
    assert int((differ & cert).sum()) == 0
    assert int(ref.exact.min()) >= 0 and all(int(ref.exact[:, l].max()) < K for l, K in enumerate(c.Ks))
    if c.floor is not None:
        assert ref.share >= c.floor, (ref.share, c.floor)


@pytest.mark.parametrize("cid", [c.id for c in CASES if c.tie_regime])
def test_tie_regime_is_a_tie_regime(cid):
    """B < K: the top-two margin of log Q is below 1e-9 on most rows of every Sinkhorn level with
    more codes than rows.  Were that to stop holding, the exact-order cases would no longer test
    the order of the float64 sums and the first-index rule.

    64 rows against 1024 codes is the exception, and is asserted as what it is: 16 codes per row
    leave its margins small but mostly above 1e-9 (six seeds: smallest 3e-11 .. 1.5e-8, median
    6e-6 .. 4e-5, largest below 1e-2; below 1e-9 on 0 to 5 % of the rows).  No row is certified, so
    the exact bar is still the only one that speaks there, but it is a near-tie regime, not a tie
    regime: every margin below the certificate's threshold, the smallest below 1e-7."""
    c = BY_ID[cid]
    _, _, ref = case_data(cid)
    levels = [l for l, K in enumerate(c.Ks) if c.eps[l] > 0 and K > c.B]
    assert levels
    for l in levels:
        tight = float((ref.margin[:, l] < 1e-9).double().mean())
        print(f"\n{cid} level {l}: margin < 1e-9 on {tight:.3f} of the rows, min {float(ref.margin[:, l].min()):.2e} "
              f"max {float(ref.margin[:, l].max()):.2e}")
        if not c.near_tie:
            assert tight > 0.5, (l, tight)
        else:
            assert float(ref.margin[:, l].max()) < rq_oracle.SK_LOG_MARGIN and float(ref.margin[:, l].min()) < 1e-7
    assert int(ref.certified.sum()) == 0


def test_one_row_group_takes_code_zero():
    """A group of one row: the Sinkhorn makes every entry of the single row the same value, so the
    first-index argmax is code 0 on every Sinkhorn level -- whatever the row is."""
    c = BY_ID["B1_e32_K8x256"]
    _, _, ref = case_data(c.id)
    assert ref.exact.tolist() == [[0, 0]] and ref.fp64.tolist() == [[0, 0]]
    assert float(ref.margin.max()) == 0.0
    z, cbs = make_inputs(1, 32, [8, 256], seed=5)
    assert rq_oracle.quantize_sk(z * 3.0, cbs, [0.01, 0.01], 50).tolist() == [[0, 0]]
    # an argmin level is not affected
    got = rq_oracle.quantize_sk(z, cbs, [0.0, 0.01], 50)
    assert int(got[0, 0]) == int(rq_oracle.rq_quantize(z, cbs)[0, 0]) and int(got[0, 1]) == 0


def dup_codebook(K, e, pairs, seed, scale=0.8):
    """randn(K, e) * scale with C[hi] = C[lo] for every (lo, hi) of ``pairs``."""
    c = torch.randn(K, e, generator=torch.Generator().manual_seed(seed)) * scale
    for lo, hi in pairs:
        c[hi] = c[lo]
    return c


DUP_PAIRS = {48: [(5, 37), (6, 7)], 256: [(3, 67), (10, 74), (100, 164), (191, 255)]}


@pytest.mark.parametrize("K", [48, 256])
@pytest.mark.parametrize("B", [3, 17, 64, 600])
def test_duplicate_codes_take_the_lower_index(B, K):
    """Two equal codes have equal distances and equal Q in every row: first-index argmax / argmin
    never returns the higher index of a pair, on Sinkhorn and on argmin levels."""
    z, cbs, eps, ref = dup_case(B, K)
    hi = torch.tensor([h for _, h in DUP_PAIRS[K]])
    for l in range(2):
        assert not bool(torch.isin(ref.exact[:, l], hi).any()), l
        assert not bool(torch.isin(ref.fp64[:, l], hi).any()), l
    lo = torch.tensor([a for a, _ in DUP_PAIRS[K]])
    if B >= 64:   # the case means something only if the pairs are chosen at all
        assert bool(torch.isin(ref.exact, lo).any())
    assert int(((ref.exact != ref.fp64).any(1) & ref.certified).sum()) == 0


@functools.lru_cache(maxsize=None)
def dup_case(B, K):
    """Level 0 Sinkhorn, level 1 argmin, both codebooks with the duplicate pairs of DUP_PAIRS[K]."""
    z = torch.randn(B, 32, generator=torch.Generator().manual_seed(100 * B + K))
    cbs = [dup_codebook(K, 32, DUP_PAIRS[K], seed=K + 1, scale=0.8),
           dup_codebook(K, 32, DUP_PAIRS[K], seed=K + 2, scale=0.5)]
    eps = [0.01, 0.0]
    return z, cbs, eps, Ref(z, cbs, eps, 50)


# ------------------------------------------------------------------ groups of mixed size (one launch)
MIXED_SIZES = [1, 2, 3, 64, 300, 7, 1, 65]
MIXED_KS = [256, 8, 64]
MIXED_EPS = [0.01, 0.01, 0.01]
MIXED_FLOOR = 0.75  # certified share over the rows of the 64-, 300- and 65-row groups (measured 0.837)


@functools.lru_cache(maxsize=None)
def mixed_data():
    """(z, codebooks, [Ref per group]): each group is its own reference call on its rows alone."""
    z, cbs = make_inputs(sum(MIXED_SIZES), 32, MIXED_KS, seed=4242)
    refs, r0 = [], 0
    for s in MIXED_SIZES:
        refs.append(Ref(z[r0:r0 + s], cbs, MIXED_EPS, 50))
        r0 += s
    return z, cbs, refs


def test_mixed_groups_oracles_agree():
    z, cbs, refs = mixed_data()
    big = [r for s, r in zip(MIXED_SIZES, refs) if s >= 64]
    for s, r in zip(MIXED_SIZES, refs):
        assert int(((r.exact != r.fp64).any(1) & r.certified).sum()) == 0, s
        if s == 1:
            assert r.exact.tolist() == [[0, 0, 0]]
    share = sum(int(r.certified.sum()) for r in big) / sum(len(r.certified) for r in big)
    print(f"\nmixed groups: certified share of the large groups {share:.3f}")
    assert share >= MIXED_FLOOR
    # grouping matters: the same rows as one group choose differently somewhere
    one = rq_oracle.quantize_sk(z, cbs, MIXED_EPS, 50)
    assert bool((one != torch.cat([r.exact for r in refs])).any())


def stated_dot(r, c):
    """r . C^T in the MKL order of the fixture host as oracle/rq_exact.c states it (the order the
    kernels follow), whatever sgemm this host's torch runs."""
    from oracle import rq_exact
    return torch.from_numpy(rq_exact.linear(r.numpy(), c.numpy()))


# Few rows against more codes, at seeds where the float64 order decides one row: a restatement of
# the kernel's order on the CPU (index-order sums, ``(Q / s) / B``) gives torch's answer, while
#   ``(Q / s) * (1 / B)`` in place of the division (B = 3, 5, 6: no power of two)   -- the K = 24 cases
#   pairwise instead of index-order row and column sums                              -- the others
# moves one row, and 1-ulp noise on exp() moves none.  The last one pins the order of the column
# sum: torch's CPU sum over dim 0 is not in index order (columns past the last multiple of 16 go
# through four interleaved partial sums, and from 18 rows on the rows are summed in blocks of 16);
# at 17 rows x 40 codes row 13 sits on an exact tie between codes 32 and 33 (fp64 margin 0.0) that
# this order decides: index-order column sums give 33, torch gives 32.
# (B, K, eps, seed) of make_inputs.
ORDER_CASES = [(3, 24, 0.01, 6), (3, 24, 0.01, 14), (5, 24, 0.01, 20), (6, 24, 0.01, 30),
               (5, 136, 0.01, 361), (6, 64, 0.01, 164), (6, 136, 0.01, 92), (6, 40, 0.003, 50),
               (17, 40, 0.003, 59)]

@functools.lru_cache(maxsize=None)
def order_data(B, K, eps, seed):
    z, cbs = make_inputs(B, 32, [K], seed)
    return z, cbs, rq_oracle.quantize_sk(z, cbs, [eps], 50, dot=stated_dot)


@pytest.mark.parametrize("B,K,eps,seed", ORDER_CASES)
def test_order_cases_are_ties(B, K, eps, seed):
    z, cbs, exact = order_data(B, K, eps, seed)
    idx, margin = rq_oracle.quantize_sk_fp64(z, cbs, [eps], 50)
    assert float(margin.min()) < 1e-9          # decided by rounding: the fp64 bar is silent here
    assert exact.shape == (B, 1) and int(exact.max()) < K


PITCH_SIZES = [1000, 1, 1, 1, 1, 1, 1, 1, 300]
PITCH_KS = [256, 64]
PITCH_FLOOR = 0.95  # measured over all rows (the one-row groups certify nothing)


@functools.lru_cache(maxsize=None)
def pitch_data():
    """Two workspace-resident groups at Kmax = 256 and then at K = 64 < Kmax (both matrices exceed
    the 16384 LDS elements on both levels).  The short group finishes level 0 in a third of the long
    one's time (measured 5 ms against 16.5 ms), so a workspace offset that used the level's K
    instead of the pitch Kmax would put the short group's level-1 matrix (rows 1007..1307 x 64)
    inside the long group's live one (its rows 251..327).  The seven one-row groups between them
    make the two workgroups numbers 0 and 8: workgroups go round the eight XCDs in turn, each XCD
    has an L2 of its own, and only two workgroups on one XCD see each other's writes while the
    kernel runs (as workgroups 0 and 1 the overlap changed nothing, measured)."""
    z, cbs = make_inputs(sum(PITCH_SIZES), 32, PITCH_KS, seed=909)
    refs, r0 = [], 0
    for s in PITCH_SIZES:
        refs.append(Ref(z[r0:r0 + s], cbs, [0.01, 0.01], 50))
        r0 += s
    return z, cbs, refs


def test_pitch_groups_oracles_agree():
    _, _, refs = pitch_data()
    for r in refs:
        assert int(((r.exact != r.fp64).any(1) & r.certified).sum()) == 0
    share = sum(int(r.certified.sum()) for r in refs) / sum(PITCH_SIZES)
    print(f"\npitch groups: certified share {share:.3f}")
    assert share >= PITCH_FLOOR


PROD_GROUPS = 600
PROD_KS = [256, 256, 256]
PROD_EPS = [0.0, 0.0, 0.003]      # infer.py:109-110: only the last level runs the Sinkhorn


@functools.lru_cache(maxsize=None)
def prod_data():
    """About 600 collision-sized groups (sizes cycle 1..5) at the production K: (z, cbs, sizes,
    exact idx of every group's own call)."""
    sizes = [1 + i % 5 for i in range(PROD_GROUPS)]
    z, cbs = make_inputs(sum(sizes), 32, PROD_KS, seed=777)
    out, r0 = [], 0
    for s in sizes:
        out.append(rq_oracle.quantize_sk(z[r0:r0 + s], cbs, PROD_EPS, 50))
        r0 += s
    return z, cbs, sizes, torch.cat(out)


def test_production_groups_are_all_ties():
    """The infer.py form is entirely in the B < K regime: no row of a sample of groups certified."""
    z, cbs, sizes, exact = prod_data()
    assert exact.shape == (sum(sizes), 3)
    r0 = 0
    for s in sizes[:25]:
        idx, margin = rq_oracle.quantize_sk_fp64(z[r0:r0 + s], cbs, PROD_EPS, 50)
        assert float(margin[:, 2].max()) < 1e-9
        assert torch.equal(idx[:, :2], exact[r0:r0 + s, :2])     # the argmin levels agree outright
        if s == 1:
            assert int(exact[r0, 2]) == 0
        r0 += s
