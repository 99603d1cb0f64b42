"""rq_sk_kernel (csrc/rq_sk.hip) on every branch, against the two references of oracle/rq_oracle.py
(tests/test_rq_sk_restatement.py owns the cases, the cached references and the CPU test of the
references against each other).

Two bars per case:
  exact   idx == rq_oracle.quantize_sk on every row (torch's CPU fp32 distances, the float64
          Sinkhorn of layers.py:85-108), cap 0, wherever every level's r.C^T order is inside
          mkl_plan_pinned's envelope (oracle.rq_exact.plan(B, e, K)[2]); outside it -- only
          B15_e32_K5x7x12: fewer than 16 rows, K no multiple of 8 -- rows_differ is recorded;
  fp64    every certified row == rq_oracle.quantize_sk_fp64 (float64 from the inputs on; a row is
          certified when its margin exceeds 1e-2 in log Q / 1e-4 relative distance gap on every
          level), and the certified share meets the case's floor.
A certified row that differs is a kernel bug; an uncertified one is a question of summation order.
Groups with fewer rows than codes certify nothing (top-two margins of 0 or an ulp): there the
exact bar alone speaks, and it pins the order of the float64 sums (rows in index order, columns
in torch's blocked CPU order), the / s / dB division sequence and the first-index rule.

What the cases reach (SK_T = 1024 threads, lds_elems = min(n Kmax, 16384)):
  division path             any B or K that is no power of two (65, 12, 5, 9, 33, 7, 100, 24, ...)
  seq_sum<8> / <16> tails   K = 5, 7, 8, 9, 12, 16, 24, 33, 100
  LDS <-> workspace         65 x [8, 12, 256] and 300 x [256, 8, 64] switch between levels; the mixed
                            launch has groups on both sides at K = 256 and Kmax != K on two levels
  lane groups               Gr 64 (B 1..3, 15, 16), 32 (17), 16 (64), 4 (130), 2 (300, 512), 1 (513+)
  B, K <= 1024 edge         B = 1023, 1024, 1025; K = 1024
  parameters                e = 5, 33, 48, 64; 0, 1, 50, 100 iterations; eps 0.003 .. 1.0; an argmin
                            level between Sinkhorn levels; K = 1

Measured on an MI355X (rows_differ against the exact oracle, certified_differ against the fp64 one):

  case                                  rows  rows_differ  certified  share  certified_differ
  B64_e32_K8x8x8                          64            0         64  1.000                 0
  B65_e32_K8x12x256                       65            0         50  0.769                 0
  B64_e32_K256x5x9                        64            0         34  0.531                 0
  B17_e48_K33x16x1                        17            0         15  0.882                 0
  B15_e32_K5x7x12 (not pinned)            15            0         15  1.000                 0
  B512_e32_K8x64                         512            0        512  1.000                 0
  B513_e5_K7x1024                        513            0        505  0.984                 0
  B1023_e32_K16                         1023            0       1021  0.998                 0
  B1024_e32_K16x9                       1024            0       1022  0.998                 0
  B1025_e32_K16x9                       1025            0       1020  0.995                 0
  B300_e32_K256x8x64_it100               300            0        271  0.903                 0
  B130_e33_K100x24_it1                   130            0        130  1.000                 0
  B130_e33_K100x24_it0                   130            0        130  1.000                 0
  B2048_e32_K8                          2048            0       2045  0.999                 0
  B1500_e32_K64                         1500            0       1499  0.999                 0
  B64_e32_K8x8x8_x0.0003                  64            0         63  0.984                 0
  B3_e32_K8x24x256                         3            0          0  0.000                 0
  B2_e64_K256x8                            2            0          0  0.000                 0
  B1_e32_K8x256                            1            0          0  0.000                 0
  B16_e32_K1024                           16            0          0  0.000                 0
  B64_e32_K1024                           64            0          0  0.000                 0
  mixed groups [1,2,3,64,300,7,1,65]     443            0        359  0.810                 0
  pitch groups 1000 + 7 x 1 + 300       1307            0       1293  0.989                 0
  600 production groups (1..5 rows)     1800            0          -      -                 -
  duplicate codes, B 3/17/64/600 x K 48/256: rows_differ 0 on all eight, no higher twin returned
  duplicate rows (4 equal rows; two equal pairs of 6): rows_differ 0 on the stated sgemm order
      (against the host's own sgemm, which rounds equal rows of a 6-row call differently: 2 and 5)
  float64 order cases (R.ORDER_CASES), eight groups of 3..6 rows and 17 x 40: rows_differ 0

Mutants of rq_sk.hip (scratch builds) and the tests that fail on them:
  pairwise seq_sum                 test_float64_order_cases[5-136, 6-64, 6-136, 6-40] while the column
                                   sums still went through seq_sum; confined to the row sums (the
                                   columns now follow torch_col_sum) it passes every case: the row
                                   order is not pinned (torch's own is vectorised and not restated;
                                   a row sum scales a whole row and acts only through rounding
                                   ties: 0 of 2800 groups of 3..9 rows moved in a CPU restatement)
  index-order column sums          test_float64_order_cases[17-40] (the kernel before torch_col_sum)
  * invB / * invK for the division test_float64_order_cases[3-24 (two seeds), 5-24, 6-24]
  no ``oi < best`` in the combine  duplicate codes B3 K48/K256 and B64 K48, duplicate rows (all 4),
                                   single groups B3 / B2 / B1, mixed and production groups, the model
                                   test; and the fixtures of test_rq_sk_gpu.py (5 tests)
  K <= 8 sum without its tail      single groups B64_K256x5x9, B15_K5x7x12, B513_K7x1024
  amplitude without + 1e-5         single group B64_e32_K8x8x8_x0.0003 (inputs scaled by 3e-4: the
                                   1e-5 is most of the amplitude there; invisible at |d| ~ 10..100)
  workspace offset r0 * K[l]       test_workspace_pitch_two_large_groups (243 certified rows of the
                                   long group move) once the two groups share an XCD; as workgroups
                                   0 and 1, on two XCDs with an L2 each, the overlap changed nothing
"""
import ctypes
import itertools

import pytest
import torch

import test_rq_sk_restatement as R
from oracle import rq_exact

pytestmark = pytest.mark.gpu


def _pinned(B, e, Ks):
    """Every level's r.C^T order inside the envelope in which rq_exact.c's statement of MKL's order
    is checked bit for bit -- on the fixture host.  It says nothing about the sgemm of the host the
    tests run on: MKL on an AMD host takes other kernels for calls of 1-7, 16 and 17 rows."""
    return all(rq_exact.plan(B, e, K)[2] for K in Ks)


def _bars(got, ref, pinned, floor, what, parity_log, **extra):
    """Log, then hold ``got`` [rows, L] (CPU) to both bars of ``ref`` (R.Ref)."""
    differ = (got != ref.exact).any(1)
    differ64 = (got != ref.fp64).any(1)
    cert = ref.certified
    rec = dict(kind="rq_sinkhorn_shapes", case=what, rows=len(differ), rows_differ=int(differ.sum()),
               certified=int(cert.sum()), certified_differ=int((differ64 & cert).sum()),
               share=round(ref.share, 4), floor=floor, pinned=pinned, cap=0 if pinned else None, **extra)
    parity_log(**rec)
    assert rec["certified_differ"] == 0, f"{what}: {rec['certified_differ']} certified rows differ from the fp64 oracle"
    if floor is not None:
        assert ref.share >= floor, (what, ref.share, floor)
    if pinned:
        assert rec["rows_differ"] == 0, (f"{what}: {rec['rows_differ']} rows differ from the exact oracle, "
                                         f"{int((differ & cert).sum())} of them certified (a kernel bug; "
                                         f"the others are a question of order)")


def _dev(ts, dev):
    return [t.to(dev) for t in ts]


# ------------------------------------------------------------------------------ (a) one group
@pytest.mark.parametrize("cid", [c.id for c in R.CASES])
def test_single_group_shapes(cid, dev, parity_log):
    from gr_amd import ops
    c = R.BY_ID[cid]
    z, cbs, ref = R.case_data(cid)
    got = ops.rq_quantize_sk(z.to(dev), _dev(cbs, dev), c.eps, c.iters).cpu()
    assert got.shape == (c.B, len(c.Ks)) and got.dtype == torch.int64
    _bars(got, ref, _pinned(c.B, c.e, c.Ks), c.floor, cid, parity_log, Ks=c.Ks, eps=c.eps, iters=c.iters)
    if cid == "B1_e32_K8x256":      # the one-row quirk, literally
        assert got.tolist() == [[0, 0]]
    if cid == "B15_e32_K5x7x12":
        assert not _pinned(c.B, c.e, c.Ks)
    else:
        assert _pinned(c.B, c.e, c.Ks)


# ------------------------------------------------------------------------------ (b) many groups
def _mixed(dev):
    from gr_amd import ops
    z, cbs, refs = R.mixed_data()
    return ops.rq_quantize_sk(z.to(dev), _dev(cbs, dev), R.MIXED_EPS, 50, R.MIXED_SIZES).cpu()


def test_mixed_groups_one_launch(dev, parity_log):
    """Sizes [1, 2, 3, 64, 300, 7, 1, 65] against K [256, 8, 64]: lds_elems = 16384, so at K = 256 the
    300- and 65-row groups sit in the workspace (65 * 256 = 16640) and the 64-row one just fits
    LDS (16384); at K = 8 all are in LDS; at K = 64 the 300-row group is back in the workspace
    (19200) with K != Kmax, the 65-row one in LDS.  Each group against its own reference call."""
    from gr_amd import ops
    z, cbs, refs = R.mixed_data()
    got = _mixed(dev)
    r0, bad, tot = 0, [], dict(rows=0, rows_differ=0, certified=0, certified_differ=0)
    for s, ref in zip(R.MIXED_SIZES, refs):
        g = got[r0:r0 + s]
        differ, differ64 = (g != ref.exact).any(1), (g != ref.fp64).any(1)
        assert _pinned(s, 32, R.MIXED_KS)
        row = dict(rows=s, rows_differ=int(differ.sum()), certified=int(ref.certified.sum()),
                   certified_differ=int((differ64 & ref.certified).sum()))
        for k, v in row.items():
            tot[k] += v
        if row["rows_differ"] or row["certified_differ"]:
            bad.append((r0, row, int((differ & ref.certified).sum())))
        r0 += s
    parity_log(kind="rq_sinkhorn_shapes", case="mixed_groups", sizes=R.MIXED_SIZES, Ks=R.MIXED_KS, cap=0, **tot)
    assert not bad, f"(first row, counts, certified among the rows that differ): {bad}"
    big = [r for s, r in zip(R.MIXED_SIZES, refs) if s >= 64]
    assert sum(int(r.certified.sum()) for r in big) / sum(len(r.certified) for r in big) >= R.MIXED_FLOOR
    # group_sizes is not ignored: the same rows as ONE group choose differently somewhere
    one = ops.rq_quantize_sk(z.to(dev), _dev(cbs, dev), R.MIXED_EPS, 50).cpu()
    assert bool((one != got).any())


def test_workspace_pitch_two_large_groups(dev, parity_log):
    """Groups of 1000 and 300 rows (workgroups 0 and 8, on one XCD: R.pitch_data) against K [256, 64]:
    their matrices are workspace-resident, level 1 at K < Kmax.  Each group owns rows [r0, r1) x
    Kmax of the workspace whatever the level's K."""
    from gr_amd import ops
    z, cbs, refs = R.pitch_data()
    got = ops.rq_quantize_sk(z.to(dev), _dev(cbs, dev), [0.01, 0.01], 50, R.PITCH_SIZES).cpu()
    r0 = 0
    for g, (s, ref) in enumerate(zip(R.PITCH_SIZES, refs)):
        _bars(got[r0:r0 + s], ref, _pinned(s, 32, R.PITCH_KS), None, f"pitch_group{g}_{s}_rows", parity_log)
        r0 += s
    assert sum(int(r.certified.sum()) for r in refs) / sum(R.PITCH_SIZES) >= R.PITCH_FLOOR


def test_production_groups_one_launch(dev, parity_log):
    """infer.py's form at the production K: 600 groups of 1..5 rows against 256 codes, argmin on
    the first two levels and the Sinkhorn (eps 0.003) on the last.  Entirely B < K: exact bar."""
    from gr_amd import ops
    z, cbs, sizes, exact = R.prod_data()
    assert all(_pinned(s, 32, R.PROD_KS) for s in range(1, 6))
    got = ops.rq_quantize_sk(z.to(dev), _dev(cbs, dev), R.PROD_EPS, 50, sizes).cpu()
    differ = (got != exact).any(1)
    parity_log(kind="rq_sinkhorn_shapes", case="production_groups", groups=len(sizes), rows=len(differ),
               rows_differ=int(differ.sum()), rows_differ_sinkhorn_level=int((got[:, 2] != exact[:, 2]).sum()), cap=0)
    assert int(differ.sum()) == 0
    starts = torch.tensor([0] + sizes[:-1]).cumsum(0)
    ones = starts[torch.tensor(sizes) == 1]
    assert bool((got[ones, 2] == 0).all())          # one-row groups: code 0 on the Sinkhorn level


# ------------------------------------------------------------------------------ (c) ties
@pytest.mark.parametrize("K", [48, 256])
@pytest.mark.parametrize("B", [3, 17, 64, 600])
def test_duplicate_codes_take_the_lower_index(B, K, dev, parity_log):
    """C[5] == C[37], C[6] == C[7] (K = 48) / C[k] == C[k + 64] (K = 256): with Gr = 64, 32, 16 and 1
    lanes per row the twins fall into the same lane (k = k' mod Gr) or into different lanes, where
    only the ``oi < best`` rule of the shuffle combine keeps the lower one."""
    from gr_amd import ops
    z, cbs, eps, ref = R.dup_case(B, K)
    got = ops.rq_quantize_sk(z.to(dev), _dev(cbs, dev), eps, 50).cpu()
    hi = torch.tensor([h for _, h in R.DUP_PAIRS[K]])
    for l in range(2):                                   # level 0 Sinkhorn, level 1 argmin
        assert not bool(torch.isin(got[:, l], hi).any()), (l, got[:, l].tolist())
    _bars(got, ref, _pinned(B, 32, [K, K]), None, f"dup_codes_B{B}_K{K}", parity_log)
    assert _pinned(B, 32, [K, K])


def _dup_rows(kind):
    g = torch.Generator().manual_seed(31)
    if kind == "all_equal":
        z = torch.randn(1, 32, generator=g).repeat(4, 1)
    else:                                                # rows 0 == 3 and 1 == 4 among 6 rows
        z = torch.randn(6, 32, generator=g)
        z[3], z[4] = z[0], z[1]
    cbs = [torch.randn(8, 32, generator=g) * 0.8, torch.randn(256, 32, generator=g) * 0.5]
    return z, cbs


@pytest.mark.parametrize("kind", ["all_equal", "two_pairs"])
@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_duplicate_rows_equal_oracle(kind, order, dev, parity_log):
    """Identical rows of a collision group (K = 8 and K = 256, either first): their Q rows differ, if
    at all, by the rounding order of the sums alone, and every entry of such a row has a twin an
    ulp away in the other.  Exact bar, on the distances of the stated MKL order (rq_exact.linear):
    the host's own sgemm may round two equal rows of one call differently (measured: the 6-row
    call on an AVX-512 AMD host gives rows 1 and 4 different distances and then different codes, 2 and
    5 rows of 6 off), which the reference's fixture host and the kernel do not.  The count against
    the host's own distances is recorded, not asserted.  Equal rows get equal codes."""
    from gr_amd import ops
    from oracle import rq_oracle
    z, cbs = _dup_rows(kind)
    cbs = [cbs[i] for i in order]
    ref = rq_oracle.quantize_sk(z, cbs, [0.01, 0.01], 50, dot=R.stated_dot)
    host = rq_oracle.quantize_sk(z, cbs, [0.01, 0.01], 50)
    got = ops.rq_quantize_sk(z.to(dev), _dev(cbs, dev), [0.01, 0.01], 50).cpu()
    assert _pinned(z.shape[0], 32, [8, 256])
    differ = int((got != ref).any(1).sum())
    parity_log(kind="rq_sinkhorn_shapes", case=f"dup_rows_{kind}_K{cbs[0].shape[0]}first", rows=z.shape[0],
               rows_differ=differ, rows_differ_host_sgemm=int((got != host).any(1).sum()), cap=0)
    assert differ == 0, (got.tolist(), ref.tolist())
    if kind == "all_equal":
        assert bool((got == got[0]).all())
    else:
        assert torch.equal(got[0], got[3]) and torch.equal(got[1], got[4])


def _order_case(B, K, eps, seed, dev, parity_log, what):
    from gr_amd import ops
    from oracle import rq_oracle
    z, cbs, ref = R.order_data(B, K, eps, seed)
    got = ops.rq_quantize_sk(z.to(dev), _dev(cbs, dev), [eps], 50).cpu()
    assert _pinned(B, 32, [K])
    differ = int((got != ref).any(1).sum())
    host = rq_oracle.quantize_sk(z, cbs, [eps], 50)
    f64 = R.Ref(z, cbs, [eps], 50)
    certified_differ = int(((got != f64.fp64).any(1) & f64.certified).sum())
    parity_log(kind="rq_sinkhorn_shapes", case=f"{what}_B{B}_K{K}_seed{seed}", rows=B, rows_differ=differ,
               rows_differ_host_sgemm=int((got != host).any(1).sum()), certified=int(f64.certified.sum()),
               certified_differ=certified_differ, cap=0)
    assert certified_differ == 0
    return differ, got, ref


@pytest.mark.parametrize("B,K,eps,seed", R.ORDER_CASES)
def test_float64_order_cases(B, K, eps, seed, dev, parity_log):
    """Few rows against 24..136 codes at seeds where the division sequence ``(Q / s) / B`` or the
    order of the sums decides a row, and 17 x 40, where torch's blocked column-sum order decides
    an exact tie (R.ORDER_CASES).  Exact bar on the stated sgemm order; the count against the
    host's own sgemm is recorded."""
    differ, got, ref = _order_case(B, K, eps, seed, dev, parity_log, "float64_order")
    assert differ == 0, (got.tolist(), ref.tolist())


# ------------------------------------------------------------------------------ (d) overflow
def test_overflow_every_entry_nan(dev):
    """eps = 0.001: exp(-d'/eps) overflows for d' < -0.71, the total is inf and every entry ends as
    NaN -- in the reference too, whose argmax over an all-NaN row is 0."""
    from gr_amd import ops
    from oracle import rq_oracle
    z, cbs = R.make_inputs(64, 32, [8], seed=11)
    ref = rq_oracle.quantize_sk(z, cbs, [0.001], 50)
    assert bool((ref == 0).all())
    got = ops.rq_quantize_sk(z.to(dev), _dev(cbs, dev), [0.001], 50).cpu()
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------ (e) workspace, ABI
GUARD = 4096


def test_workspace_discipline_and_return_codes(dev):
    """gr_rq_encode_sk_f32 on exactly gr_rq_encode_sk_workspace_bytes bytes between two guard bands,
    everything filled with 0xFF (NaN patterns): the kernel neither reads what the workspace held
    nor writes outside it (the workspace starts 8 bytes off a 256-byte boundary, so the kernel's
    own align-up uses the slack the byte count includes).  Then the refusals, none of which
    launches anything."""
    from gr_amd import _lib as L
    z, cbs, _ = R.mixed_data()
    want = _mixed(dev)
    lib = L.lib()
    zd, cd = z.to(dev), _dev(cbs, dev)
    n, e, nl = z.shape[0], z.shape[1], len(cbs)
    ks = L.i32_array(R.MIXED_KS)
    eps = (ctypes.c_double * nl)(*R.MIXED_EPS)
    ptr = torch.tensor([0] + list(itertools.accumulate(R.MIXED_SIZES)), dtype=torch.int64).to(dev)
    need = lib.gr_rq_encode_sk_workspace_bytes(n, e, nl, ks)
    assert need >= n * e * 4 + n * max(R.MIXED_KS) * 8
    buf = torch.full((GUARD + 8 + need + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    ws = buf.data_ptr() + GUARD + 8
    st = L.stream_of(dev)
    cbp = L.ptr_array(cd)

    def call(idx, n_=n, ks_=ks, iters=50, nbytes=need, groups=len(R.MIXED_SIZES)):
        return lib.gr_rq_encode_sk_f32(L.ptr(zd), n_, e, nl, ks_, cbp, eps, iters, L.ptr(ptr), groups,
                                       L.ptr(idx), ws, ctypes.c_size_t(nbytes), st)

    for _ in range(2):                # the second run finds the first one's leavings, not NaN
        idx = torch.full((n, nl), -7, dtype=torch.int64, device=dev)
        L.check(call(idx), "gr_rq_encode_sk_f32")
        assert torch.equal(idx.cpu(), want)
        assert bool((buf[:GUARD + 8] == 0xFF).all()) and bool((buf[GUARD + 8 + need:] == 0xFF).all())
    idx = torch.full((n, nl), -7, dtype=torch.int64, device=dev)
    assert call(idx, nbytes=need - 1) == -4                              # GR_ERR_WORKSPACE
    assert b"workspace" in lib.gr_last_error()
    assert call(idx, ks_=L.i32_array([256, 8, 1025])) == -2                 # GR_ERR_UNSUPPORTED
    assert call(idx, iters=-1) == -1                                     # GR_ERR_ARG
    assert call(idx, n_=0) == 0                                          # GR_OK, nothing written
    torch.cuda.synchronize()
    assert bool((idx == -7).all())


def test_group_sizes_are_checked(dev):
    from gr_amd import ops
    z, cbs = R.make_inputs(10, 32, [8], seed=3)
    zd, cd = z.to(dev), _dev(cbs, dev)
    for sizes in ([4, 5], [4, 7], [5, 0, 5], [10, 0]):
        with pytest.raises(RuntimeError, match="group sizes must be positive and sum to the batch"):
            ops.rq_quantize_sk(zd, cd, [0.01], 50, sizes)
    assert ops.rq_quantize_sk(zd, cd, [0.01], 50, [4, 6]).shape == (10, 1)


# ------------------------------------------------------------------------------ (f) shared kernel
@pytest.mark.parametrize("cid,eps", [("B64_e32_K8x8x8", [0.01, 0.0, 0.01]),
                                     ("B65_e32_K8x12x256", [0.01, 0.05, 0.003]),
                                     ("B300_e32_K256x8x64_it100", [0.05, 1.0, 0.003])])
def test_training_entry_shares_the_assignment(cid, eps, dev):
    """gr_rq_quantize_sk_train_f32 (ops.rq_quantize_train) launches the same kernel: its indices
    are ops.rq_quantize_sk's, bit for bit."""
    from gr_amd import ops
    c = R.BY_ID[cid]
    z, cbs, _ = R.case_data(cid)
    zd, cd = z.to(dev), _dev(cbs, dev)
    want = ops.rq_quantize_sk(zd, cd, eps, c.iters)
    x_q, rq_loss, idx = ops.rq_quantize_train(zd, cd, 0.25, eps, c.iters)
    assert idx.dtype == torch.int64 and torch.equal(idx, want)
    assert x_q.shape == z.shape and bool(torch.isfinite(rq_loss))


def test_model_get_indices_is_one_group_of_the_grouped_call(dev):
    """RQVAE.get_indices(use_sk=True) on a group's rows = those rows of get_indices_groups, at
    unequal K with a K that is no power of two."""
    from gr_amd import RQVAE
    torch.manual_seed(5)
    m = RQVAE(in_dim=256, num_emb_list=[8, 12, 256], e_dim=32, layers=[128], dropout_prob=0.0,
              sk_epsilons=[0.01, 0.01, 0.003], sk_iters=50).to(dev).eval()
    x = torch.randn(70, 256, generator=torch.Generator().manual_seed(6)).to(dev)
    sizes = [3, 40, 1, 26]
    got = m.get_indices_groups(x, sizes)
    r0 = 0
    for s in sizes:
        assert torch.equal(m.get_indices(x[r0:r0 + s], use_sk=True), got[r0:r0 + s]), s
        r0 += s
    assert int(got[43, 0]) == 0 and int(got[43, 2]) == 0     # the one-row group
    assert not torch.equal(got, m.get_indices(x, use_sk=True))


# ------------------------------------------------------------------------------ (g) determinism
def test_deterministic_across_calls_and_streams(dev):
    from gr_amd import ops
    z, cbs, _ = R.mixed_data()
    zd, cd = z.to(dev), _dev(cbs, dev)
    a = ops.rq_quantize_sk(zd, cd, R.MIXED_EPS, 50, R.MIXED_SIZES)
    b = ops.rq_quantize_sk(zd, cd, R.MIXED_EPS, 50, R.MIXED_SIZES)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        c = ops.rq_quantize_sk(zd, cd, R.MIXED_EPS, 50, R.MIXED_SIZES)
    s.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
