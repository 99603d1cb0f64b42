"""SASRec inference kernels (csrc/sasrec*.hip, attn.hip) against an fp64 reference on every forward path.

Reference: ``oracle/sasrec_oracle.forward`` (SASRec/model.py:49-96) on the model's state dict cast to
float64; logits ``h[:, -1] @ item_emb.T`` (model.py:107) in float64; ranks from the fp64 logits as
SASRec/evaluate.py:27-32 (column 0 at -1e9, strict ``>``, plus one).  The same restatement on the
float32 state dict gives err_t32, the distance of an fp32 evaluation of the same math from fp64.  Per
case, kernel path and quantity two errors are recorded through ``parity_log``: err_t32 and err_kernel
(kernels vs fp64).  Hidden states (``forward``: all positions; ``last_hidden``) are scaled by the
fp64 tensor's largest magnitude, logits (``predict``) per row by the fp64 row's largest magnitude.

A class's tolerance is 4 x its worst err_t32 over all cases of the class (room for the MFMA k order
and the reassociated sums), rounded up to one significant digit; it is never sized from err_kernel.
The cases with peaked attention (the q and k rows of every in_proj_weight times 4: the online-softmax
rescales of attn_k16_kernel, attn_persist_kernel, sas_tail_h2_kernel and the fused kernel carry
weight) are conditioned differently and form classes of their own.

Inputs: 600 items (a 601-row table, a ragged last scoring tile); ``synth.sequences`` with row 0 all
padding, row 1 only its last position set, row 2 unpadded and one row repeating an item; every
output finite.  Cases are (d, heads, mlp, n, blocks, B); the branches of csrc/sasrec.hip they reach:

* fused kernel, sas_fused 1 / 3 (bitwise equal) and 0 (layer-wise): FUSED; (64, 1, 64, 20, 0, 5) is
  num_blocks = 0; (64, 1, 64, 50, 2, 600) runs under the default option 2 (wave count by batch size);
* d = 128 row-tile and per-op (sas_rowtile 1 / 0 x attn_k16 1 / 0): D128; the two B = CUs + 40 cases
  take sas_tail_h2_kernel's ds_bpermute reduction form (4 heads; 8 heads, head width 16, which also
  is d = 128 per-op with causal_attn_kernel);
* per-op with the H-form tail: HFORM ((128, 2, 256, 40, 1, 4): d = 128 with mlp_layer outside
  {32, 64, 128}, so not the row-tile path, tail accepted);
* the tail refused (d/4, head width/4 or mlp/4 no power of two), so run_layerwise's pruned final block
  (``last_tile_only = 1``, the gathers, out-proj / LN / FFN on B rows inside the FFN buffer): PRUNED;
  (48, 2, 100, 70, 2, 9) and (20, 5, 12, 70, 2, 5) take causal_attn_kernel (head widths 24 and 4),
  (128, 2, 100, 77, 2, 7) attn_persist_kernel<64>, (128, 1, 100, 70, 2, 5) attn_k16_kernel and
  attn_persist_kernel<128>, (128, 4, 100, 40, 1, 4) attn_mfma_kernel<32> from the last query tile,
  (128, 1, 100, 1, 2, 3) n = 1 (``prune`` false); all of them are d = 128 / d <= 64 per-op forwards
  for ``forward``;
* n < max_len, layernorm_eps 1e-3 and peaked attention: VARIANTS, on one fused, one row-tile and one
  pruned case each.

Ranks: per case at least 32 users (extra ``synth.sequences`` rows where B is smaller); half the
targets from the fp64 top-20, half uniform.  With delta = the logits tolerance x row scale a user is
certified when no fp64 competitor lies within 2 delta of the fp64 target logit; certified users'
ranks equal the fp64 rank, every rank lies in [#{l > t + 2 delta} + 1, #{l > t - 2 delta} + 1], and at
least 90 % of a case's users must be certified.

Measured on an MI355X (its host ran the restatements: err_t32 moves by a few 1e-8 with the host's
fp32 sum order).  Per quantity ``err_t32 err_kernel``; "fwd[-1]" is err_kernel of ``forward(...)[:, -1]``
against last_hidden's reference, scale and tolerance; "certified" the certified users of the case;
paths joined by "=" measured the same figures:

    case, variant                      path                       forward          last_hidden      logits           fwd[-1]  certified
    (64,1,64,50,2,37)                  fused1 = fused3            1.7e-07 1.9e-07  2.0e-07 1.6e-07  4.7e-07 3.7e-07  2.1e-07  37/37
                                       layerwise                  1.7e-07 1.6e-07  2.0e-07 1.6e-07  4.7e-07 3.7e-07  1.6e-07  37/37
    (48,2,96,33,3,9)                   fused1 = fused3            1.8e-07 2.0e-07  1.9e-07 1.7e-07  3.8e-07 3.3e-07  1.6e-07  32/32
                                       layerwise                  1.8e-07 2.2e-07  1.9e-07 1.9e-07  3.8e-07 3.0e-07  1.9e-07  32/32
    (16,2,32,1,1,4)                    fused1 = fused3            9.5e-08 8.0e-08  9.5e-08 9.5e-08  2.8e-07 2.2e-07  8.0e-08  32/32
                                       layerwise                  9.5e-08 1.0e-07  9.5e-08 7.7e-08  2.8e-07 2.6e-07  1.0e-07  32/32
    (64,8,128,64,8,3)                  fused1 = fused3            2.9e-07 2.4e-07  2.0e-07 1.7e-07  4.1e-07 4.1e-07  2.2e-07  31/32
                                       layerwise                  2.9e-07 2.9e-07  2.0e-07 1.9e-07  4.1e-07 2.8e-07  1.9e-07  31/32
    (64,1,64,20,0,5)                   fused1 = fused3            1.3e-07 1.5e-07  8.2e-08 1.1e-07  3.4e-07 4.2e-07  1.1e-07  32/32
                                       layerwise                  1.3e-07 1.4e-07  8.2e-08 8.2e-08  3.4e-07 3.4e-07  8.2e-08  32/32
    (64,1,64,50,2,600)                 default = fused1           2.0e-07 2.3e-07  2.1e-07 2.1e-07  4.6e-07 3.9e-07  2.0e-07  597/600
    (128,1,64,200,2,6)                 rowtile_k16                2.0e-07 2.0e-07  1.3e-07 1.7e-07  4.9e-07 4.9e-07  1.4e-07  32/32
                                       rowtile_k32                2.0e-07 2.0e-07  1.3e-07 1.3e-07  4.9e-07 3.9e-07  1.3e-07  32/32
                                       per_op_k16                 2.0e-07 2.0e-07  1.3e-07 1.8e-07  4.9e-07 4.9e-07  1.8e-07  32/32
                                       per_op_k32                 2.0e-07 1.8e-07  1.3e-07 1.7e-07  4.9e-07 4.5e-07  1.5e-07  32/32
    (128,2,32,77,3,5)                  rowtile_k16 = rowtile_k32  2.0e-07 1.9e-07  2.3e-07 1.5e-07  3.9e-07 3.9e-07  1.5e-07  32/32
                                       per_op_k16 = per_op_k32    2.0e-07 2.0e-07  2.3e-07 1.7e-07  3.9e-07 4.2e-07  1.7e-07  32/32
    (128,4,128,33,1,4)                 rowtile_k16 = rowtile_k32  1.4e-07 1.4e-07  1.2e-07 1.1e-07  5.5e-07 6.5e-07  1.2e-07  32/32
                                       per_op_k16 = per_op_k32    1.4e-07 1.5e-07  1.2e-07 1.2e-07  5.5e-07 6.5e-07  7.5e-08  32/32
    (128,1,64,1,2,3)                   rowtile_k16 = rowtile_k32  2.0e-07 2.2e-07  2.0e-07 2.2e-07  5.6e-07 4.6e-07  2.2e-07  31/32
                                       per_op_k16 = per_op_k32    2.0e-07 2.3e-07  2.0e-07 1.8e-07  5.6e-07 3.5e-07  2.3e-07  31/32
    (128,1,64,209,1,3)                 rowtile_k16 = rowtile_k32  1.6e-07 1.4e-07  7.2e-08 1.1e-07  3.8e-07 3.7e-07  1.1e-07  31/32
                                       per_op_k16                 1.6e-07 1.4e-07  7.2e-08 1.1e-07  3.8e-07 3.5e-07  1.2e-07  31/32
                                       per_op_k32                 1.6e-07 1.6e-07  7.2e-08 1.1e-07  3.8e-07 3.5e-07  1.2e-07  31/32
    (128,4,64,33,2,296)                all four paths             2.1e-07 2.1e-07  2.1e-07 1.8e-07  6.5e-07 6.2e-07  1.8e-07  293/296
    (128,8,64,33,2,296)                all four paths             1.9e-07 1.8e-07  2.0e-07 2.0e-07  5.7e-07 4.5e-07  2.0e-07  294/296
    (64,2,128,100,2,17)                per_op                     2.2e-07 2.2e-07  1.4e-07 1.5e-07  2.5e-07 2.9e-07  1.5e-07  32/32
    (32,8,64,90,1,6)                   per_op                     2.0e-07 1.5e-07  1.0e-07 1.1e-07  2.4e-07 2.4e-07  1.0e-07  32/32
    (128,2,256,40,1,4)                 per_op                     1.4e-07 1.3e-07  1.6e-07 1.6e-07  4.5e-07 4.5e-07  1.0e-07  32/32
    (48,2,100,70,2,9)                  per_op                     2.3e-07 2.3e-07  1.2e-07 1.2e-07  3.1e-07 3.1e-07  1.2e-07  32/32
    (128,2,100,77,2,7)                 per_op                     2.0e-07 1.7e-07  1.5e-07 1.3e-07  5.2e-07 4.6e-07  1.3e-07  31/32
    (20,5,12,70,2,5)                   per_op                     2.0e-07 2.0e-07  1.2e-07 1.2e-07  2.3e-07 2.6e-07  1.2e-07  31/32
    (128,1,100,1,2,3)                  per_op_k16 = per_op_k32    2.6e-07 1.9e-07  2.6e-07 1.9e-07  4.7e-07 5.8e-07  1.9e-07  32/32
    (128,1,100,70,2,5)                 per_op_k16                 1.8e-07 1.8e-07  2.1e-07 2.1e-07  4.9e-07 3.6e-07  2.1e-07  31/32
                                       per_op_k32                 1.8e-07 1.6e-07  2.1e-07 1.4e-07  4.9e-07 4.6e-07  1.4e-07  31/32
    (128,4,100,40,1,4)                 per_op                     1.7e-07 1.4e-07  1.0e-07 1.8e-07  4.4e-07 4.3e-07  1.8e-07  32/32
    (64,1,64,50,2,37) eps1e-3          fused1 = fused3            2.0e-07 2.1e-07  1.4e-07 1.4e-07  3.8e-07 3.3e-07  1.6e-07  37/37
                                       layerwise                  2.0e-07 1.6e-07  1.4e-07 1.5e-07  3.8e-07 3.3e-07  1.6e-07  37/37
    (128,1,64,200,2,6) eps1e-3         rowtile_k16                2.0e-07 1.9e-07  1.6e-07 1.4e-07  4.2e-07 4.1e-07  1.4e-07  32/32
                                       rowtile_k32                2.0e-07 2.0e-07  1.6e-07 1.4e-07  4.2e-07 4.1e-07  1.6e-07  32/32
                                       per_op_k16                 2.0e-07 1.9e-07  1.6e-07 1.2e-07  4.2e-07 3.6e-07  1.2e-07  32/32
                                       per_op_k32                 2.0e-07 1.9e-07  1.6e-07 1.4e-07  4.2e-07 3.6e-07  1.4e-07  32/32
    (128,2,100,77,2,7) eps1e-3         per_op                     1.8e-07 1.9e-07  1.8e-07 1.8e-07  6.1e-07 3.4e-07  1.8e-07  31/32
    (64,1,64,50,2,37) max_len+17       fused1 = fused3            1.7e-07 2.1e-07  1.9e-07 1.2e-07  3.4e-07 3.1e-07  1.8e-07  37/37
                                       layerwise                  1.7e-07 2.0e-07  1.9e-07 1.7e-07  3.4e-07 3.4e-07  1.4e-07  37/37
    (128,1,64,200,2,6) max_len+17      rowtile_k16                2.0e-07 2.1e-07  1.4e-07 1.6e-07  4.4e-07 4.4e-07  2.1e-07  32/32
                                       rowtile_k32                2.0e-07 2.0e-07  1.4e-07 1.4e-07  4.4e-07 4.4e-07  1.8e-07  32/32
                                       per_op_k16                 2.0e-07 2.0e-07  1.4e-07 1.6e-07  4.4e-07 4.4e-07  1.6e-07  32/32
                                       per_op_k32                 2.0e-07 2.0e-07  1.4e-07 1.6e-07  4.4e-07 4.4e-07  1.8e-07  32/32
    (128,2,100,77,2,7) max_len+17      per_op                     1.8e-07 1.7e-07  1.5e-07 1.9e-07  3.2e-07 3.2e-07  1.9e-07  32/32
    (64,1,64,50,2,37) peaked           fused1 = fused3            1.3e-06 1.1e-06  9.0e-07 6.7e-07  6.2e-07 9.0e-07  8.4e-07  37/37
                                       layerwise                  1.3e-06 1.5e-06  9.0e-07 8.3e-07  6.2e-07 7.5e-07  8.4e-07  37/37
    (128,1,64,200,2,6) peaked          rowtile_k16                2.4e-06 4.2e-06  1.5e-06 9.9e-07  9.9e-07 1.2e-06  9.6e-07  32/32
                                       rowtile_k32                2.4e-06 3.2e-06  1.5e-06 7.6e-07  9.9e-07 4.8e-07  1.5e-06  32/32
                                       per_op_k16                 2.4e-06 3.3e-06  1.5e-06 1.3e-06  9.9e-07 5.7e-07  5.1e-07  32/32
                                       per_op_k32                 2.4e-06 2.1e-06  1.5e-06 7.5e-07  9.9e-07 6.4e-07  6.9e-07  32/32
    (128,2,100,77,2,7) peaked          per_op                     1.3e-06 9.8e-07  9.1e-07 7.0e-07  1.0e-06 9.7e-07  7.0e-07  31/32

Worst err_t32 per class -> tolerance (worst err_kernel): forward 2.9e-07 -> 2e-06 (2.9e-07),
last_hidden 2.6e-07 -> 2e-06 (2.3e-07), logits 6.5e-07 -> 3e-06 (6.5e-07); peaked: forward 2.4e-06 ->
1e-05 (4.2e-06), last_hidden 1.5e-06 -> 7e-06 (1.5e-06), logits 1.0e-06 -> 5e-06 (1.2e-06).  Every path
fits 4 x, the H-form tail included, so no class takes the 8 x its reassociated sums could have asked.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import sasrec_oracle

ITEMS = 600
RANK_B = 32          # users of the rank part, at least
CUS = "CUs+40"       # B of the cases sized from the device's CU count

# 4 x the worst err_t32 of the class, rounded up to one significant digit (table above)
TOL_FWD, TOL_LAST, TOL_LOGITS = 2e-6, 2e-6, 3e-6
TOL_FWD_PEAK, TOL_LAST_PEAK, TOL_LOGITS_PEAK = 1e-5, 7e-6, 5e-6
# worst logits err_t32 of the unpeaked class: with TOL_LOGITS the triangle bound of a GPU logit
# against the fp32 oracle (tests/test_sasrec_fullsize_gpu.py)
T32_LOGITS = 6.5e-7

FUSED = [(64, 1, 64, 50, 2, 37), (48, 2, 96, 33, 3, 9), (16, 2, 32, 1, 1, 4), (64, 8, 128, 64, 8, 3),
         (64, 1, 64, 20, 0, 5)]
FUSED_DEFAULT = [(64, 1, 64, 50, 2, 600)]
D128 = [(128, 1, 64, 200, 2, 6), (128, 2, 32, 77, 3, 5), (128, 4, 128, 33, 1, 4), (128, 1, 64, 1, 2, 3),
        (128, 1, 64, 209, 1, 3), (128, 4, 64, 33, 2, CUS), (128, 8, 64, 33, 2, CUS)]
HFORM = [(64, 2, 128, 100, 2, 17), (32, 8, 64, 90, 1, 6), (128, 2, 256, 40, 1, 4)]
PRUNED = [(48, 2, 100, 70, 2, 9), (128, 2, 100, 77, 2, 7), (20, 5, 12, 70, 2, 5), (128, 1, 100, 1, 2, 3),
          (128, 1, 100, 70, 2, 5), (128, 4, 100, 40, 1, 4)]
VARIANT_BASES = [("fused", (64, 1, 64, 50, 2, 37)), ("d128", (128, 1, 64, 200, 2, 6)),
                 ("pruned", (128, 2, 100, 77, 2, 7))]
# (layernorm_eps, max_len - n, factor on the q and k rows of in_proj_weight)
PLAIN = (1e-8, 0, 1)
VARIANTS = {"eps1e-3": (1e-3, 0, 1), "max_len+17": (1e-8, 17, 1), "peaked": (1e-8, 0, 4)}

CASES = ([("fused", s, "plain") for s in FUSED] + [("fused_default", s, "plain") for s in FUSED_DEFAULT]
         + [("d128", s, "plain") for s in D128] + [("hform", s, "plain") for s in HFORM]
         + [("pruned", s, "plain") for s in PRUNED]
         + [(g, s, v) for v in VARIANTS for g, s in VARIANT_BASES])

DEFAULTS = {"sas_fused": 2, "sas_rowtile": 1, "attn_k16": 1}


def paths(group, shape):
    """(name, options) of every kernel path a case runs through."""
    d, heads = shape[0], shape[1]
    if group == "fused":
        return [("fused1", {"sas_fused": 1}), ("fused3", {"sas_fused": 3}), ("layerwise", {"sas_fused": 0})]
    if group == "fused_default":
        return [("default", {}), ("fused1", {"sas_fused": 1})]
    if group == "d128":
        return [(f"{'rowtile' if rt else 'per_op'}_k{16 if k16 else 32}", {"sas_rowtile": rt, "attn_k16": k16})
                for rt in (1, 0) for k16 in (1, 0)]
    if group == "pruned" and d // heads == 128:
        return [("per_op_k16", {"attn_k16": 1}), ("per_op_k32", {"attn_k16": 0})]
    return [("per_op", {})]


def assert_plan(binding, group, name, shape):
    """The label of a run is the plan under its options (``gr_sasrec_plan``), for the full forward and
    the last-position one: pipeline, attention kernel, and the final block's tail / pruned form."""
    from gr_amd import _lib as L
    d, heads, mlp, n, blocks, B = shape
    hd = d // heads
    for last_only in (0, 1):
        m = binding.plan(B, n, last_only)
        assert m >= 0, (name, m)
        pipe = m & (L.GR_SAS_FUSED | L.GR_SAS_ROWTILE | L.GR_SAS_LAYERWISE)
        attn = m & (L.GR_SAS_ATTN_SCALAR | L.GR_SAS_ATTN_MFMA | L.GR_SAS_ATTN_PERSIST | L.GR_SAS_ATTN_K16)
        tail, pruned = bool(m & L.GR_SAS_TAIL), bool(m & L.GR_SAS_PRUNED)
        what = (name, last_only, hex(m))
        assert not m & L.GR_SAS_FUSED_MISALIGNED, what
        if name in ("fused1", "fused3", "default"):
            assert pipe == L.GR_SAS_FUSED, what
            if name != "default":   # two waves need two 32-token tiles
                assert bool(m & L.GR_SAS_FUSED_TWO_WAVES) == (name == "fused3" and n > 32), what
            continue
        # (128, 8, 64, 33, 2, CUs + 40), head width 16, is per-op under sas_rowtile 1 as well
        rowtile = name.startswith("rowtile") and hd in (32, 64, 128)
        assert pipe == (L.GR_SAS_ROWTILE if rowtile else L.GR_SAS_LAYERWISE), what
        # the final block of a last-position forward: the tail everywhere but in the pruned group, where
        # it is the pruned block (n = 1 has nothing to prune: the full block); the layer-wise run of a
        # fused shape takes whichever of the two its widths give
        if group == "fused":
            assert tail + pruned == (last_only == 1 and blocks >= 1 and (tail or n >= 2)), what
        else:
            assert tail == (last_only == 1 and group != "pruned"), what
            assert pruned == (last_only == 1 and group == "pruned" and n >= 2), what
        if blocks - tail == 0:
            assert attn == 0, what
        elif hd == 128:
            k16 = name.endswith("_k16") or not name.endswith("_k32")   # unnamed: the default, 16-key steps
            assert attn == (L.GR_SAS_ATTN_K16 if k16 else L.GR_SAS_ATTN_PERSIST), what
        else:
            assert attn == {64: L.GR_SAS_ATTN_PERSIST, 32: L.GR_SAS_ATTN_MFMA}.get(hd, L.GR_SAS_ATTN_SCALAR), what
        assert bool(m & L.GR_SAS_ATTN_LAST_TILE) == (pruned and attn != L.GR_SAS_ATTN_SCALAR), what


def build_sequences(B, n, seed):
    """max(B, RANK_B) rows of synth.sequences with the rows no draw of it gives: all padding, only the
    last position set, no padding, an item repeated within the row.  The first B rows are the case's
    batch, all of them the rank part's."""
    from gr_amd import synth
    s = synth.sequences(max(B, RANK_B), n, ITEMS, seed, "cpu")
    g = torch.Generator().manual_seed(seed + 1)
    s[0] = 0
    s[1, :-1] = 0
    s[2] = torch.randint(1, ITEMS + 1, (n,), generator=g)
    if n >= 2:
        r = min(3, B - 1)
        s[r, -1] = s[r, -2]     # lengths are >= 2: both set
    return s


def oracle(sd, seqs, blocks, heads, eps, dtype):
    """(forward [B, n, d], logits [B, rows]) of the restatement in ``dtype``."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    f = sasrec_oracle.forward(seqs, sd, blocks, heads, eps)
    return f, f[:, -1, :] @ sd["item_emb.weight"].t()


def scaled_err(a, ref):
    """max |a - ref| over the fp64 tensor's largest magnitude."""
    return float((a.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def row_err(a, ref):
    """max over rows of max |a - ref| over the fp64 row's largest magnitude."""
    return float(((a.double() - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-30)).max())


def tolerances(variant):
    if variant == "peaked":
        return {"forward": TOL_FWD_PEAK, "last_hidden": TOL_LAST_PEAK, "logits": TOL_LOGITS_PEAK}
    return {"forward": TOL_FWD, "last_hidden": TOL_LAST, "logits": TOL_LOGITS}


@functools.lru_cache(maxsize=None)
def reference(shape, variant):
    """A case's CPU side, computed once and left unchanged: fp32 state dict, sequences, the fp64
    reference and the fp32 restatement's errors against it.  ``shape``'s B is a number here."""
    from gr_amd import synth
    d, heads, mlp, n, blocks, B = shape
    eps, extra, peak = VARIANTS.get(variant, PLAIN)
    p = synth.sasrec_params(d, n + extra, blocks, heads, mlp, "cpu")
    p["layernorm_eps"] = eps
    m = synth.sasrec_model(ITEMS, p, "cpu", seed=d + heads + n + blocks)
    with torch.no_grad():
        for a in m.attention_layers:
            a.in_proj_weight[:2 * d] *= peak
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    seqs = build_sequences(B, n, 11 + n + B)
    f64, l64 = oracle(sd, seqs, blocks, heads, eps, torch.float64)
    f32, l32 = oracle(sd, seqs, blocks, heads, eps, torch.float32)
    assert f64.dtype == torch.float64 and l64.dtype == torch.float64
    t32 = {"forward": scaled_err(f32[:B], f64[:B]), "last_hidden": scaled_err(f32[:B, -1], f64[:B, -1]),
           "logits": row_err(l32, l64)}
    return dict(params=p, sd=sd, seqs=seqs, f64=f64, l64=l64, t32=t32, eps=eps)


def rank_reference(l64, tol, seed):
    """Targets (half from the fp64 top-20, half uniform in [1, items]), the fp64 ranks
    (evaluate.py:27-32), the band a logits error of delta = tol x row scale allows, and the users
    whose target has no competitor within 2 delta."""
    delta = (l64.abs().amax(1) * tol)[:, None]
    lg = l64.clone()
    lg[:, 0] = -1e9
    c = lg.shape[0]
    rng = np.random.default_rng(seed)
    top20 = torch.topk(lg, 20, dim=1).indices.numpy()
    tg = np.where(rng.random(c) < 0.5, top20[np.arange(c), rng.integers(0, 20, c)], rng.integers(1, ITEMS + 1, c))
    tg = torch.from_numpy(tg.astype(np.int64))
    t = lg.gather(1, tg[:, None])
    exact = ((lg > t).sum(1) + 1).numpy()
    lo = ((lg > t + 2 * delta).sum(1) + 1).numpy()
    hi = ((lg > t - 2 * delta).sum(1) + 1).numpy()      # counts the target itself
    return tg, exact, lo, hi, lo == hi - 1


@contextlib.contextmanager
def options(opts):
    from gr_amd import _lib
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            _lib.set_option(k, v)


def _id(c):
    g, s, v = c
    return f"{g}-{'-'.join(str(x) for x in s)}-{v}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_infer_paths_vs_fp64(case, dev, parity_log):
    """forward, last_hidden, predict and the ranks of every kernel path of a case against fp64."""
    from gr_amd import SASRec, evaluate, ops
    group, shape, variant = case
    if shape[5] == CUS:   # above the CU count: the tail's ds_bpermute reduction form
        shape = shape[:5] + (torch.cuda.get_device_properties(dev).multi_processor_count + 40,)
    d, heads, mlp, n, blocks, B = shape
    ref = reference(shape, variant)
    tol = tolerances(variant)
    model = SASRec(ITEMS, dict(ref["params"], device=str(dev)))
    model.load_state_dict(ref["sd"])
    model = model.to(dev).eval()
    assert model.pos_emb.weight.shape[0] == n + VARIANTS.get(variant, PLAIN)[1]
    seqs = ref["seqs"].to(dev)
    f64, l64 = ref["f64"], ref["l64"]
    tg, exact, lo, hi, cert = rank_reference(l64, tol["logits"], 1000 * d + n)
    assert cert.mean() >= 0.9, f"only {cert.sum()} of {len(cert)} users certified"
    bad, outs = [], {}
    for name, opts in paths(group, shape):
        with options(opts):
            assert_plan(model._binding(seqs[:B]), group, name, shape)
            fwd = model.forward(seqs[:B]).cpu()
            last = model.last_hidden(seqs[:B]).cpu()
            lg_b = model.predict(seqs[:B]).cpu()
            lg_dev = model.predict(seqs)
            r_mat = ops.rank(lg_dev, tg.to(dev)).cpu().numpy()
            r_fused = evaluate.rank_batch(model, seqs, tg.to(dev)).cpu().numpy()
        torch.cuda.synchronize()
        ops.check_errors(dev)
        lg = lg_dev.cpu()
        outs[name] = (fwd, last, lg)
        assert fwd.shape == (B, n, d) and last.shape == (B, d) and lg.shape == l64.shape
        for t in (fwd, last, lg_b, lg):                     # the all-padding row included
            assert bool(torch.isfinite(t).all()), name
        errs = {"forward": scaled_err(fwd, f64[:B]), "last_hidden": scaled_err(last, f64[:B, -1]),
                "logits": max(row_err(lg, l64), row_err(lg_b, l64[:B])),
                # the full forward's last row is held to last_hidden's bar as well
                "forward[:, -1]": scaled_err(fwd[:, -1], f64[:B, -1])}
        for q, e in errs.items():
            cls = "last_hidden" if q == "forward[:, -1]" else q
            parity_log(kind="sasrec_infer_vs_fp64", case=list(shape), variant=variant, path=name, quantity=q,
                       err_t32=ref["t32"][cls], err_kernel=e, tol=tol[cls])
            if not e <= tol[cls]:
                bad.append((name, q, e, tol[cls]))
        assert np.array_equal(r_fused, r_mat), name           # the fused rank and rank over predict's logits
        in_band = (r_mat >= lo) & (r_mat <= hi)
        parity_log(kind="sasrec_infer_ranks_vs_fp64", case=list(shape), variant=variant, path=name,
                   users=len(r_mat), certified=int(cert.sum()), ranks_exact=int((r_mat == exact).sum()),
                   ranks_in_band=int(in_band.sum()))
        if not in_band.all() or not np.array_equal(r_mat[cert], exact[cert]):
            bad.append((name, "ranks", int((~in_band).sum()), int((r_mat[cert] != exact[cert]).sum())))
    assert not bad, bad
    if "fused3" in outs or "default" in outs:   # one or two waves per sequence: the same instruction sequence
        other = outs["fused3"] if "fused3" in outs else outs["default"]
        for a, b in zip(outs["fused1"], other):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_path_switch_on_a_model_that_has_run(dev):
    """Regression: SasrecBinding cached a shape's workspace size across ``set_option`` calls, so a
    model whose first call took the fused kernel (a [B, d] workspace) failed with "workspace too
    small" once ``sas_fused`` 0 sent the same shape layer-wise.  The smallest fused shape, forward
    and the one-call rank, in both orders of the switch."""
    from gr_amd import SASRec, evaluate
    shape = (16, 2, 32, 1, 1, 4)
    ref = reference(shape, "plain")
    seqs = ref["seqs"].to(dev)
    tg = torch.ones(len(seqs), dtype=torch.int64, device=dev)
    for order in ((1, 0), (0, 1)):
        model = SASRec(ITEMS, dict(ref["params"], device=str(dev)))
        model.load_state_dict(ref["sd"])
        model = model.to(dev).eval()
        res = []
        for opt in order:
            with options({"sas_fused": opt}):
                res.append((model.last_hidden(seqs).cpu(), evaluate.rank_batch(model, seqs, tg).cpu()))
        for last, ranks in res:
            assert scaled_err(last, ref["f64"][:, -1]) <= TOL_LAST
            assert bool(((ranks >= 1) & (ranks <= ITEMS)).all())


# one fused and one pruned-block shape: CPU only, so the constants are pinned wherever the suite runs
@pytest.mark.parametrize("shape", [(64, 1, 64, 50, 2, 37), (128, 2, 100, 77, 2, 7)])
def test_tolerances_have_teeth(shape):
    """The fp32 restatement meets the class tolerances against fp64; the fp64 restatement with a
    LayerNorm epsilon off by 1e-5, or with block 0's out-projection bias off by one part in a
    thousand, misses every one of them.  A tolerance loosened until a kernel that hard-coded its
    epsilon passed would fail here."""
    d, heads, mlp, n, blocks, B = shape
    ref = reference(shape, "plain")
    tol = tolerances("plain")
    for q, e in ref["t32"].items():
        assert e <= tol[q], (q, e)
    sd, seqs, f64, l64 = ref["sd"], ref["seqs"], ref["f64"], ref["l64"]
    bias = dict(sd)
    bias["attention_layers.0.out_proj.bias"] = sd["attention_layers.0.out_proj.bias"] * (1 - 1e-3)
    for what, (sd_p, eps_p) in {"eps + 1e-5": (sd, ref["eps"] + 1e-5), "out_proj.bias x (1 - 1e-3)": (bias, ref["eps"])}.items():
        f, lg = oracle(sd_p, seqs, blocks, heads, eps_p, torch.float64)
        errs = {"forward": scaled_err(f[:B], f64[:B]), "last_hidden": scaled_err(f[:B, -1], f64[:B, -1]),
                "logits": row_err(lg, l64)}
        print(f"\n{shape} {what}: " + ", ".join(f"{q} {e:.2e} (tol {tol[q]:.0e})" for q, e in errs.items()))
        for q, e in errs.items():
            assert e > tol[q], (what, q, e)
