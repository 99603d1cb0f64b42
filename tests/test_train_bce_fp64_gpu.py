"""Training-side scoring (csrc/train_bce.hip) against float64, and the negative sampler
(csrc/neg_sample.hip) against an exact restatement of its stream.

Sampled BCE vs fp64
-------------------
Reference: ``oracle/sasrec_oracle.train_loss_grads_scores`` (train.py:134-167 verbatim, the dense score
matrix S kept with ``retain_grad``) on float64 copies of the inputs.  Its dS is non-zero only at the
gathered entries and gives elementwise magnitude bounds, so a table row with a small gradient is held
as tightly as the largest: ``bound_dF = |dS| . |M|``, ``bound_dM = |dS|^T . |F|``, ``bound_loss`` = the
sum of the absolute loss terms.  The kernel is held to ``|got - ref| <= TOL x bound + 1.2e-38``;
entries whose bound is 0 must be exactly 0; ``valid`` is exact.  err_t32 is the same normalised error
of the fp32 CPU restatement; TOL of a class is 4 x its worst err_t32 over all cases, rounded up to one
digit, and was fixed before the kernels were run.

Every case keeps its gathered logits inside |s| <= 4 (asserted on the fp64 scores): the restatement
forms ``1 - sigmoid(s)`` in fp32, which is quantised above s ~ 5 and 0 above s ~ 17, and there fp32
semantics and the fp64 value part company.  Inputs are ``scale x randn`` with scale = min(0.3,
sqrt(0.75 / sqrt(d))); left padding of random length per user, user 0 all padding and user 1 unpadded
where B allows; the padded positions' features are random, not zero.

Cases (B, n, d, items, J) and what they reach in bce_fwd_kernel / the two backward kernels:

* J0 .. J64: no negatives (gr_sampled_bce_bwd_f32 returns before the negatives kernel; an empty negs
  pointer); the BCE_RB = 16 group edge (1 + J = 16, 17, 18); three and five groups;
* d65, d63, d130, d1: d around the 64-lane stride, d = 1;
* B1n1, B1, n1: B = 1, n = 1, a block of four positions with fewer than four (and six in two blocks);
* collide: for users 1-3 one negative is also one of the user's targets, item 11 is among every user's
  negatives and is user 4's target, so its dtable row takes atomics from both backward kernels;
* hot: all 128 positions valid with target 3, 128 atomic adds into one row (no padding in this case).

Measured on an MI355X, per class ``err_t32 err_kernel`` (dtable moves in its last digit from run to
run with the atomic order):

    case     (B, n, d, items, J)    max|s|  batch_loss        dfeats            dtable
    J0       (5, 3, 48, 80, 0)      1.13   1.2e-08 1.2e-08  1.9e-07 2.5e-07  1.9e-07 2.5e-07
    J15      (5, 3, 48, 80, 15)     1.71   5.1e-08 3.6e-08  1.2e-07 1.2e-07  2.3e-07 2.1e-07
    J16      (5, 3, 48, 80, 16)     1.62   9.4e-08 4.4e-09  1.0e-07 1.2e-07  2.2e-07 2.9e-07
    J17      (5, 3, 48, 80, 17)     1.71   4.0e-10 4.0e-10  1.2e-07 1.1e-07  3.5e-07 2.2e-07
    J33      (5, 3, 48, 80, 33)     2.39   2.5e-08 5.9e-08  1.1e-07 1.5e-07  8.6e-07 8.1e-07
    J64      (5, 3, 48, 80, 64)     2.18   5.6e-08 5.8e-09  1.2e-07 1.3e-07  2.0e-07 2.2e-07
    d65      (9, 7, 65, 40, 33)     2.78   2.3e-08 2.3e-08  1.4e-07 1.6e-07  1.5e-07 1.4e-07
    d63      (3, 4, 63, 40, 20)     2.06   3.1e-08 3.1e-08  1.2e-07 1.1e-07  2.0e-07 1.6e-07
    d130     (2, 5, 130, 40, 17)    1.97   6.7e-08 6.7e-08  1.5e-07 1.4e-07  2.0e-07 1.9e-07
    d1       (4, 6, 1, 30, 16)      0.40   3.9e-08 3.9e-08  4.4e-08 5.1e-08  6.9e-08 1.7e-07
    B1n1     (1, 1, 16, 20, 3)      0.20   1.0e-07 1.0e-07  6.5e-08 6.5e-08  1.4e-07 1.4e-07
    B1       (1, 9, 32, 20, 16)     1.34   2.8e-08 2.8e-08  1.0e-07 1.5e-07  1.3e-07 1.6e-07
    n1       (6, 1, 64, 20, 17)     1.84   1.7e-08 1.7e-08  1.2e-07 8.9e-08  2.0e-07 3.8e-07
    collide  (6, 4, 48, 60, 16)     1.92   1.8e-08 7.4e-08  1.5e-07 2.3e-07  2.0e-07 4.6e-07
    hot      (16, 8, 32, 10, 4)     1.87   7.9e-09 7.9e-09  3.4e-07 4.4e-07  9.2e-08 7.8e-08

Worst err_t32 per class -> tolerance (worst err_kernel): batch_loss 1.0e-07 -> 5e-07 (1.0e-07), dfeats
3.4e-07 -> 2e-06 (4.4e-07), dtable 8.6e-07 -> 4e-06 (8.1e-07).  Every class fits 4 x; the 8 x ceiling is
not used.  The hot row's 128 atomics into one row measured 7.8e-08 of the row's bound, below the
restatement's own 9.2e-08 there.

Exact zeros in every case: dfeats at padded positions; dtable rows outside {targets at valid
positions} + {negatives of users with a valid position}; dtable[0].

Saturation (fp32 semantics, never fp64)
---------------------------------------
Logits are exact: feats +-1 along axis 0, table rows v e_0.  A negative at s >= 20 and a positive at
s <= -110 sit on the plateaus where the fp32 sigmoid is exactly 1 / 0: each such term is -log(1e-24) =
55.262043 with coefficient 0; a positive at s >= 20 and a negative at s <= -110 give an exactly zero term.
Users holding only such terms must give count x 55.262043 within two fp32 roundings of the sum (one for
logf's last bit on each term, one for the sum) and exactly zero gradients, also where the padded
positions' own row-0 logit is +-30.

Between the plateaus, s in +-[6, 16], the kernel's ``1 / (1 + expf(-s))`` and torch.sigmoid may round
the sigmoid to neighbouring fp32 values.  One quantum U = 2^-24 (the fp32 spacing under 1) moves a
positive's term -log(sigmoid) by at most about U (|term| + 1) (relative rounding of the term plus the
quantum itself), a negative's term -log(1 - sigmoid) by U (|term| + 1 / (1 - sigmoid)) because 1 -
sigmoid cancels for s > 0, and a coefficient (|c| <= 1) by U.  test_sampled_bce_band_terms measures, one
term per launch over 14 magnitudes x 2 signs x {positive, negative} against the fp32 restatement, how
many such allowances the two are apart.  Measured on an MI355X against torch's CPU sigmoid: worst 1.6
for a loss term (one ulp of logf at s = -9), worst 1.0 for a coefficient.  The tests bound them at 4 x
that, K_TERM = 7 (6.4 rounded up) and K_COEF = 4: the factor 4 is the project's margin over a measured
distance between two fp32 evaluations of the same formula, here for another host's sigmoid or another
expf landing on the other neighbour.  The composite batch (plateau users, band users, 16 valid
positions) is then held to the fp32 restatement with K_TERM / K_COEF allowances on its band entries
plus one fp32 rounding per term; measured there: loss one ulp apart (1.2e-4 of 1963.66), dfeats 1.3
coefficient quanta, dtable 3.0e-08.

Negative sampler
----------------
``oracle/sasrec_oracle.neg_samples_replica`` restates neg_sample_kernel in Python integers (mix64, the
row key, the 128-bit range reduction, rejection by history / earlier rounds / earlier lanes, survivors
in lane order, 4096 rounds, -1 rows); tests/test_train_bce.py tests it alone on the CPU.  Here
``ops.neg_samples`` must equal it id for id: three workgroups with a one-wave tail, heavy rejection,
many rounds, num_neg = NS_MAX_NEG, more draws than 4096 shortened rounds would reach, n = 0 with
num_neg = item_num, item_num = 2^40, histories with repeats and zeros, seeds masked to 64 bits, the
seed_tensor form, an unfillable row, and num_neg = 1025 refused.  Nothing here is a rate: equality is
total.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import sasrec_oracle

pytestmark = pytest.mark.gpu

EPS = 1e-24
FLOOR = 1.2e-38          # the smallest normal fp32: below it a result may be flushed
TOL = {"batch_loss": 5e-7, "dfeats": 2e-6, "dtable": 4e-6}   # 4 x the worst err_t32 (docstring)
S_MAX = 4.0              # every gathered logit of an fp64 case stays inside, far from saturation

# name -> (B, n, d, items, J)
CASES = {f"J{J}": (5, 3, 48, 80, J) for J in (0, 15, 16, 17, 33, 64)}
CASES.update({
    "d65": (9, 7, 65, 40, 33), "d63": (3, 4, 63, 40, 20), "d130": (2, 5, 130, 40, 17), "d1": (4, 6, 1, 30, 16),
    "B1n1": (1, 1, 16, 20, 3), "B1": (1, 9, 32, 20, 16), "n1": (6, 1, 64, 20, 17),
    "collide": (6, 4, 48, 60, 16), "hot": (16, 8, 32, 10, 4),
})


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Seeded fp32 inputs of a case.  Left padding of random length per user: with B >= 3 user 0 is
    all padding and user 1 unpadded, with B = 2 user 1 is unpadded, with B = 1 the user keeps at least
    one position; "hot" has no padding (its 128 positions all add into one row).  The scale keeps the
    logits' standard deviation at or under 0.75."""
    B, n, d, items, J = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 1000 + d)
    scale = min(0.3, (0.75 / d ** 0.5) ** 0.5)
    feats = torch.randn(B, n, d, generator=g) * scale
    table = torch.randn(items + 1, d, generator=g) * scale
    table[0] = 0
    targets = torch.randint(1, items + 1, (B, n), generator=g)
    lens = torch.randint(1 if B == 1 else 0, n + 1, (B,), generator=g)
    if B >= 3:
        lens[0] = 0
    if B >= 2:
        lens[1] = n
    if name == "hot":
        lens[:] = n
        targets[:] = 3
    targets[torch.arange(n)[None, :] < (n - lens)[:, None]] = 0
    negs = sasrec_oracle.neg_samples(np.zeros((B, 1), np.int64), items, J, np.random.RandomState(B + J))
    negs = negs.reshape(B, J).to(torch.int64)
    if name == "collide":
        for b in (1, 2, 3):                                  # a negative that is also the user's target
            negs[b, b] = targets[b, -1]
        negs[:, 7] = 11                                      # one id among every user's negatives
        targets[4, -1] = 11                                  # ... which user 4 also has as a target
    return dict(feats=feats, table=table, targets=targets, negs=negs)


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The fp64 reference of a case (computed once, shared, never modified): results, the magnitude
    bounds from the fp64 dS, the gathered fp64 logits, and err_t32 of the fp32 CPU restatement."""
    t = _inputs(name)
    f, w, tg, ng = t["feats"], t["table"], t["targets"], t["negs"]
    bl, valid, gf, gw, S, dS = sasrec_oracle.train_loss_grads_scores(f.double(), w.double(), tg, ng, EPS)
    r = dict(bl=bl, valid=valid.item(), gf=gf, gw=gw)
    r["bound_gf"] = dS.abs() @ w.double().abs()
    r["bound_gw"] = torch.einsum("btr,btd->rd", dS.abs(), f.double().abs())
    m = (tg != 0).double()
    pos = torch.gather(S, 2, tg.unsqueeze(-1)).squeeze(-1)
    neg = torch.gather(S, 2, ng.unsqueeze(1).expand(-1, f.shape[1], -1))
    r["bound_bl"] = ((torch.log(torch.sigmoid(pos) + EPS) * m).abs().sum()
                     + (torch.log(1 - torch.sigmoid(neg) + EPS) * m.unsqueeze(-1)).abs().sum())
    r["s_max"] = max(pos[tg != 0].abs().max().item() if m.any() else 0.0,
                     neg[tg != 0].abs().max().item() if neg.numel() and m.any() else 0.0)
    # rows of the table that receive gradient: targets at valid positions, negatives of users with one
    live = torch.zeros(w.shape[0], dtype=torch.bool)
    live[tg[tg != 0]] = True
    live[ng[(tg != 0).any(1)].reshape(-1)] = True
    r["live_rows"] = live
    bl32, _, gf32, gw32 = sasrec_oracle.train_loss_grads(f, w, tg, ng, EPS)
    r["err_t32"] = _errs(r, bl32, gf32, gw32)
    return r


def _nerr(got, ref, bound):
    """max |got - ref| / bound over the entries with a bound (inf if an entry without one differs)."""
    diff = ((got.detach().cpu().double() - ref).abs() - FLOOR).clamp_min(0)
    bound = torch.as_tensor(bound)
    if (diff[bound == 0] > 0).any():
        return float("inf")
    nz = bound > 0
    return (diff[nz] / bound[nz]).max().item() if nz.any() else 0.0


def _errs(r, bl, gf, gw, scale=1.0):
    return {"batch_loss": _nerr(bl, r["bl"], r["bound_bl"]),
            "dfeats": _nerr(gf, r["gf"] * scale, r["bound_gf"] * abs(scale)),
            "dtable": _nerr(gw, r["gw"] * scale, r["bound_gw"] * abs(scale))}


def _run(t, dev, scale=None):
    """loss = batch_loss / valid, backward (train.py:161-167); ``scale``: (batch_loss * scale).backward()."""
    from gr_amd import ops
    f = t["feats"].to(dev).requires_grad_(True)
    w = t["table"].to(dev).requires_grad_(True)
    bl, valid = ops.sampled_bce_loss(f, w, t["targets"].to(dev), t["negs"].to(dev), EPS)
    v = valid.item()
    if scale is not None:
        (bl * scale).backward()
    elif v > 0:
        (bl / v).backward()
    else:
        (bl * 0.0).backward()
    return bl.detach(), v, f.grad, w.grad


def _assert_exact_zeros(name, gf, gw):
    t, r = _inputs(name), _ref(name)
    assert torch.count_nonzero(gf.cpu()[t["targets"] == 0]) == 0
    assert torch.count_nonzero(gw.cpu()[~r["live_rows"]]) == 0
    assert not r["live_rows"][0] and torch.count_nonzero(gw[0]) == 0


@pytest.mark.parametrize("name", list(CASES))
def test_sampled_bce_vs_fp64(name, dev, parity_log):
    t, r = _inputs(name), _ref(name)
    assert 0 < r["s_max"] <= S_MAX, r["s_max"]                # the case is out of saturation
    if name == "collide":
        tg, ng = t["targets"], t["negs"]
        assert sum(bool(set(ng[b].tolist()) & set(tg[b][tg[b] != 0].tolist())) for b in range(len(tg))) >= 3
        assert all(11 in ng[b].tolist() for b in range(len(tg))) and 11 in tg[tg != 0].tolist()
    if name == "hot":
        assert (t["targets"] == 3).all() and t["targets"].numel() == 128
    bl, valid, gf, gw = _run(t, dev)
    errs = _errs(r, bl, gf, gw)
    parity_log(case=name, shape=CASES[name], s_max=r["s_max"], err_t32=r["err_t32"], err_kernel=errs, tol=TOL)
    assert valid == r["valid"]
    assert torch.isfinite(gf).all() and torch.isfinite(gw).all()
    _assert_exact_zeros(name, gf, gw)
    for k in TOL:
        assert errs[k] <= TOL[k], (k, errs[k], r["err_t32"][k])


@pytest.mark.parametrize("name", ["J17", "collide"])
def test_sampled_bce_gradient_scale(name, dev):
    """An incoming gradient other than 1 / valid: (bl * 3.5).backward() and (-bl).backward() against
    the fp64 gradients scaled likewise (the reference's are of bl / valid); a second backward through
    the same graph is the first bit for bit, except dtable (free atomic order: held to its tolerance)."""
    from gr_amd import ops
    t, r = _inputs(name), _ref(name)
    for scale in (3.5, -1.0):
        bl, valid, gf, gw = _run(t, dev, scale=scale)
        errs = _errs(r, bl, gf, gw, scale=scale * r["valid"])
        _assert_exact_zeros(name, gf, gw)
        for k in TOL:
            assert errs[k] <= TOL[k], (scale, k, errs[k])
    f = t["feats"].to(dev).requires_grad_(True)
    w = t["table"].to(dev).requires_grad_(True)
    bl, valid = ops.sampled_bce_loss(f, w, t["targets"].to(dev), t["negs"].to(dev), EPS)
    g1 = torch.autograd.grad(bl, [f, w], retain_graph=True)
    g2 = torch.autograd.grad(bl, [f, w], retain_graph=True)
    assert torch.equal(g1[0], g2[0])
    for g in (g1, g2):
        errs = _errs(r, bl, g[0], g[1], scale=r["valid"])
        assert errs["dfeats"] <= TOL["dfeats"] and errs["dtable"] <= TOL["dtable"], errs


def test_sampled_bce_wrapper_views(dev):
    """Non-contiguous views of feats and table and int32 ids give the results of their contiguous
    int64 copies: loss, valid and dfeats bit for bit, dtable within its tolerance of fp64."""
    name = "d65"
    t, r = _inputs(name), _ref(name)
    B, n, d, items, J = CASES[name]
    bl0, valid0, gf0, gw0 = _run(t, dev)
    fh = torch.zeros(B, n, 2 * d, device=dev)
    fh[..., ::2] = t["feats"].to(dev)
    wh = torch.full((items + 1, d + 3), 7.0, device=dev)
    wh[:, :d] = t["table"].to(dev)
    f = fh[..., ::2].detach().requires_grad_(True)
    w = wh[:, :d].detach().requires_grad_(True)
    assert not f.is_contiguous() and not w.is_contiguous()
    from gr_amd import ops
    bl, valid = ops.sampled_bce_loss(f, w, t["targets"].to(dev, torch.int32), t["negs"].to(dev, torch.int32), EPS)
    (bl / valid.item()).backward()
    assert torch.equal(bl.detach(), bl0) and valid.item() == valid0 == r["valid"]
    assert torch.equal(f.grad, gf0)
    assert _nerr(w.grad, r["gw"], r["bound_gw"]) <= TOL["dtable"]
    _assert_exact_zeros(name, f.grad, w.grad)


# ------------------------------------------------------------------ saturation (fp32 semantics)

U = 2.0 ** -24            # the spacing of fp32 in [0.5, 1): the quantum of a sigmoid near 1
T_PLATEAU = 55.262043     # -log(1e-24) as rounded in fp32
K_TERM = 7.0             # 4 x 1.6, the worst measured loss-term distance (docstring), rounded up
K_COEF = 4.0             # 4 x 1.0, the worst measured coefficient distance
BAND = [6.0, 6.5, 7.0, 7.5, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0, 13.25, 14.0, 15.0, 16.0]


def _term_allowance(s, is_neg):
    """What one quantum U of the fp32 sigmoid moves a loss term by, in units of U (module docstring):
    |term| + 1 for a positive, |term| + 1 / (1 - sigmoid) for a negative."""
    s = torch.as_tensor(s, dtype=torch.float64)
    sg = torch.sigmoid(s)
    if is_neg:
        return -torch.log(1 - sg) + 1 / (1 - sg)
    return -torch.log(sg) + 1.0


def _one_term(s, is_neg, dev):
    """The kernel's and the fp32 restatement's loss term and coefficient d term / d s at the exact
    logit ``s``: one position, feats e_0, the row under test s e_0 (a negative rides on a target at
    s = 40, whose own term and coefficient are exactly 0)."""
    from gr_amd import ops
    f = torch.zeros(1, 1, 4)
    f[0, 0, 0] = 1.0
    w = torch.zeros(3, 4)
    w[1, 0], w[2, 0] = s, 40.0
    tg = torch.tensor([[2 if is_neg else 1]])
    ng = torch.tensor([[1]]) if is_neg else torch.zeros(1, 0, dtype=torch.long)
    fd, wd = f.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bl, _ = ops.sampled_bce_loss(fd, wd, tg.to(dev), ng.to(dev), EPS)
    bl.backward()
    rbl, _, _, rgw = sasrec_oracle.train_loss_grads(f, w, tg, ng, EPS)      # valid = 1: gradients of bl
    return bl.item(), wd.grad[1, 0].item(), rbl.item(), rgw[1, 0].item()


def test_sampled_bce_band_terms(dev, parity_log):
    """Between the plateaus, s in +-[6, 16], term by term against the fp32 restatement (never fp64:
    1 - sigmoid is quantised here): how far the kernel's 1 / (1 + expf(-s)) and torch.sigmoid put a
    loss term and its coefficient apart, in units of the allowance of one sigmoid quantum."""
    worst_t = worst_c = 0.0
    for s in [x * sign for x in BAND for sign in (1.0, -1.0)]:
        for is_neg in (False, True):
            kt, kc, rt, rc = _one_term(s, is_neg, dev)
            assert np.isfinite([kt, kc]).all()
            et = abs(kt - rt) / (U * _term_allowance(s, is_neg).item())
            ec = abs(kc - rc) / U
            worst_t, worst_c = max(worst_t, et), max(worst_c, ec)
            print(f"\nBAND s {s:+7.2f} {'neg' if is_neg else 'pos'} term {kt:.9g} vs {rt:.9g} ({et:.3f}) "
                  f"coef {kc:.9g} vs {rc:.9g} ({ec:.3f})", end="")
    parity_log(worst_term=worst_t, worst_coef=worst_c, k_term=K_TERM, k_coef=K_COEF)
    assert worst_t <= K_TERM and worst_c <= K_COEF


def _saturation_inputs():
    """Exact logits s = a v: feats a e_0 + (anything in the other axes), table rows v e_0.  Users 0
    and 1 hold only plateau terms, users 2 and 3 only band terms; 16 valid positions, so the 1 / valid
    of the backward is exact.  Row 0 has v = 30: the padded positions' own logit is saturated.  The
    band's negatives stay at |s| <= 11 and rows 15 and 16 (16, 13.25) are targets only: a negative's
    term at s = 16 moves by 0.5 per sigmoid quantum, which would leave the batch loss no resolution
    (test_sampled_bce_band_terms holds those terms one by one)."""
    v = torch.tensor([30, 6, 7.5, 9, 11, 10, 8, 20, 25, -110, -120, 40, -6.5, 110, -30, 16, 13.25])
    B, n, d = 4, 6, 4
    g = torch.Generator().manual_seed(1)
    table = torch.zeros(len(v), d)
    table[:, 0] = v
    feats = torch.randn(B, n, d, generator=g)
    a = torch.tensor([[1, -1, 1, 1, 1, 1], [1, -1, -1, -1, -1, -1],
                      [1, -1, 1, -1, 1, -1], [-1, 1, -1, 1, -1, 1.0]])
    feats[..., 0] = a
    targets = torch.tensor([[0, 0, 9, 7, 10, 11], [0, 13, 9, 13, 9, 13],
                            [1, 2, 3, 4, 15, 16], [0, 0, 0, 0, 0, 12]])
    negs = torch.tensor([[7, 8, 11, 9, 10], [9, 10, 14, 13, 13], [1, 2, 3, 5, 6], [2, 4, 6, 12, 3]])
    return dict(feats=feats, table=table, targets=targets, negs=negs)


def test_sampled_bce_saturation(dev):
    """fp32 semantics on and between the plateaus (module docstring, "Saturation")."""
    t = _saturation_inputs()
    f64, w64, tg, ng = t["feats"].double(), t["table"].double(), t["targets"], t["negs"]
    m = tg != 0
    s_pos = (f64[..., 0] * w64[tg, 0])                                     # exact: a in {1, -1}
    s_neg = f64[..., 0].unsqueeze(-1) * w64[ng, 0].unsqueeze(1)            # [B, n, J]
    plateau = (((s_pos <= -110) & m).sum() + ((s_neg >= 20) & m.unsqueeze(-1)).sum()).item()
    zero_terms = (((s_pos >= 20) & m).sum() + ((s_neg <= -110) & m.unsqueeze(-1)).sum()).item()
    band_pos = (s_pos.abs() >= 6) & (s_pos.abs() <= 16) & m
    band_neg = (s_neg.abs() >= 6) & (s_neg.abs() <= 16) & m.unsqueeze(-1)
    assert plateau == 32 and zero_terms == 22
    assert plateau + zero_terms + band_pos.sum() + band_neg.sum() == m.sum() * (1 + ng.shape[1])
    assert not band_pos[:2].any() and not band_neg[:2].any() and m.sum() == 16

    # users 0 and 1 alone: plateau terms only (32 of them at 55.262043, 22 exactly 0)
    sub = {k: (x if k == "table" else x[:2]) for k, x in t.items()}
    n_sub = (((s_pos <= -110) & m)[:2].sum() + ((s_neg >= 20) & m.unsqueeze(-1))[:2].sum()).item()
    bl, valid, gf, gw = _run(sub, dev)
    assert valid == 9 and np.isfinite(bl.item())
    assert round(bl.item() / T_PLATEAU) == n_sub == plateau
    assert abs(bl.item() - n_sub * T_PLATEAU) <= 2 * 2.0 ** -23 * n_sub * T_PLATEAU    # logf and the sum: an ulp each
    assert torch.count_nonzero(gf) == 0 and torch.count_nonzero(gw) == 0              # no gradient from a plateau

    # the whole batch against the fp32 restatement
    bl, valid, gf, gw = _run(t, dev)
    rbl, rvalid, rgf, rgw, _, dS = sasrec_oracle.train_loss_grads_scores(t["feats"], t["table"], tg, ng, EPS)
    assert valid == rvalid.item() == 16
    assert torch.isfinite(bl) and torch.isfinite(gf).all() and torch.isfinite(gw).all()
    allow = (_term_allowance(s_pos, False)[band_pos].sum() + _term_allowance(s_neg, True)[band_neg].sum()).item()
    slack = K_TERM * U * allow + 2 * 2.0 ** -23 * rbl.item()
    print(f"\nSATURATION loss {bl.item():.9g} vs fp32 restatement {rbl.item():.9g}: apart {abs(bl.item() - rbl.item()):.3g}, "
          f"allowed {slack:.3g} (band allowance {allow:.4g} U)")
    assert abs(bl.item() - rbl.item()) <= slack, (bl.item(), rbl.item(), slack)
    # gradients: K_COEF quanta per band coefficient (times g = 1 / 16) and an fp32 rounding per term
    hits = torch.zeros(dS.shape, dtype=torch.float64)
    hits.scatter_add_(2, tg.unsqueeze(-1), band_pos.double().unsqueeze(-1))
    hits.scatter_add_(2, ng.unsqueeze(1).expand(-1, tg.shape[1], -1), band_neg.double())
    per = K_COEF * U / 16 * hits + 2.0 ** -22 * dS.double().abs()
    bound_gf = per @ w64.abs()
    bound_gw = torch.einsum("btr,btd->rd", per, f64.abs())
    dgf, dgw = (gf.cpu().double() - rgf.double()).abs(), (gw.cpu().double() - rgw.double()).abs()
    print(f"SATURATION dfeats apart {dgf.max():.3g} (in U / 16 per band hit: {(dgf / (U / 16 * (hits @ w64.abs())).clamp_min(1e-300)).max():.3g}), "
          f"dtable apart {dgw.max():.3g}")
    assert ((gf.cpu().double() - rgf.double()).abs() <= bound_gf).all()
    assert ((gw.cpu().double() - rgw.double()).abs() <= bound_gw).all()
    # padded positions (their row-0 logit is +-30) and rows fed by plateau terms only: exact zeros
    assert torch.count_nonzero(gf.cpu()[~m]) == 0
    assert torch.count_nonzero(gw.cpu()[[0, 7, 8, 9, 10, 11, 13, 14]]) == 0
    assert (gw.cpu()[[1, 2, 3, 4, 5, 6, 12, 15, 16]] != 0).any(1).all()


# ------------------------------------------------------------------ the sampler's exact stream

def _history(B, n, items, seed):
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(1, items + 1, (B, n), generator=g)
    seq[:, : n // 3] = 0
    return seq


def _draws(seq, items, J, seed):
    """How many counters of its stream each row consumes: the sampler is a walk over the counters
    0, 1, 2, ... (64 per round, in lane order) that keeps a draw unless it was seen before."""
    out = []
    for row, hist in enumerate(seq.tolist()):
        rkey = sasrec_oracle.mix64(seed ^ sasrec_oracle.mix64(row))
        seen, t = set(hist), 0
        while len(seen) < len(set(hist)) + J:
            seen.add(1 + ((sasrec_oracle.mix64((rkey + t) % 2 ** 64) * items) >> 64))
            t += 1
        out.append(t)
    return out


@pytest.mark.parametrize("B,n,items,J", [(9, 7, 50, 4), (5, 20, 30, 10), (3, 200, 300, 64), (2, 5, 1100, 1024),
                                         (2, 3, 1027, 1024), (4, 0, 64, 64), (3, 6, 2 ** 40, 8)])
def test_neg_samples_equal_replica(B, n, items, J, dev):
    """(2, 3, 1027, 1024) is here for the round counter: a round that advanced the counter by less
    than 64 would walk the same counters more slowly and give the same ids, until a row needs more
    counters than 4096 such rounds reach (64 + 4095); both of its rows do."""
    from gr_amd import ops
    seq = _history(B, n, items, B + n)
    if items == 1027:
        assert min(_draws(seq, items, J, 7)) > 64 + 4095
    out = ops.neg_samples(seq.to(dev), items, J, seed=7).cpu()
    assert out.shape == (B, J) and torch.equal(out, sasrec_oracle.neg_samples_replica(seq, items, J, 7))
    if n == 0:
        assert all(sorted(r) == list(range(1, items + 1)) for r in out.tolist())


def test_neg_samples_history_duplicates_and_zeros(dev):
    from gr_amd import ops
    seq = torch.tensor([[0, 0, 3, 3, 7, 0, 7, 1], [5, 5, 5, 5, 5, 5, 5, 5], [0] * 8, [2, 0, 4, 0, 6, 0, 8, 0]])
    for seed in (1, 2, 3):
        out = ops.neg_samples(seq.to(dev), 12, 6, seed=seed).cpu()
        assert torch.equal(out, sasrec_oracle.neg_samples_replica(seq, 12, 6, seed))


@pytest.mark.parametrize("seed", [0, 2 ** 63 + 5, -12345, 2 ** 64 + 9])
def test_neg_samples_seed_masking(seed, dev):
    from gr_amd import ops
    seq = _history(9, 7, 50, 16)
    out = ops.neg_samples(seq.to(dev), 50, 4, seed=seed).cpu()
    assert torch.equal(out, sasrec_oracle.neg_samples_replica(seq, 50, 4, seed))
    assert torch.equal(out, sasrec_oracle.neg_samples_replica(seq, 50, 4, seed & (2 ** 64 - 1)))


def test_neg_samples_seed_tensor_equal_replica(dev):
    from gr_amd import ops
    seq = _history(9, 7, 50, 16)
    st = torch.tensor([123], dtype=torch.int64, device=dev)
    a = ops.neg_samples(seq.to(dev), 50, 4, seed=5, seed_tensor=st).cpu()
    b = ops.neg_samples(seq.to(dev), 50, 4, seed=5, seed_tensor=st).cpu()
    c = ops.neg_samples(seq.to(dev), 50, 4, seed_tensor=st).cpu()            # seed defaults to 0
    assert int(st.item()) == 126
    assert torch.equal(a, sasrec_oracle.neg_samples_replica(seq, 50, 4, 5, seed_word=123))
    assert torch.equal(b, sasrec_oracle.neg_samples_replica(seq, 50, 4, 5, seed_word=124))
    assert torch.equal(c, sasrec_oracle.neg_samples_replica(seq, 50, 4, 0, seed_word=125))
    assert not torch.equal(a, b)


def test_neg_samples_unfillable_row(dev):
    """Row 0 has 2 valid items for 3 negatives: the replica's row is -1, ops.neg_samples raises
    ValueError, and the kernel's own output (through the C ABI, as ops calls it) has the -1 row and the
    other row's draws."""
    from gr_amd import _lib as L, ops
    seq = torch.tensor([[1, 2, 3, 4], [0, 0, 0, 1]])
    rep = sasrec_oracle.neg_samples_replica(seq, 6, 3, 9)
    assert rep[0].tolist() == [-1, -1, -1] and rep[1].min() >= 2
    with pytest.raises(ValueError):
        ops.neg_samples(seq.to(dev), 6, 3, seed=9)
    s = seq.to(dev)
    out = torch.zeros((2, 3), dtype=torch.int64, device=dev)
    err = ops.err_flag(dev)
    with L.on(dev):
        L.check(L.lib().gr_neg_samples(L.ptr(s), 2, 4, 6, 3, 9, L.ptr(out), L.ptr(err), L.stream_of(dev)),
                "gr_neg_samples")
    with pytest.raises(ValueError):
        ops.check_errors(dev)
    ops.check_errors(dev)                                                    # cleared by the raise
    assert torch.equal(out.cpu(), rep)


def test_neg_samples_too_many(dev):
    from gr_amd import ops
    seq = _history(2, 5, 5000, 1).to(dev)
    with pytest.raises(RuntimeError):
        ops.neg_samples(seq, 5000, 1025, seed=1)
    assert ops.neg_samples(seq, 5000, 1024, seed=1).shape == (2, 1024)
    ops.check_errors(dev)
