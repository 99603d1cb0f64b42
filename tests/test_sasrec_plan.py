"""``gr_sasrec_plan`` (csrc/sasrec.hip ``sas_plan``): which kernels a SASRec inference forward runs, decided on
the host before anything is enqueued -- so none of this needs a GPU.  The per-block fields of
``gr_sasrec_params`` are host arrays the plan reads; here they hold fake device addresses (0x10000: 16-byte
aligned, 0x10004: not), which no call below ever hands to a kernel.

(a) the plan of every path of the inference fp64 tests, derived from the launchers' rules: shapes are
    (d, heads, mlp, n, blocks), B = 37 unless a row says otherwise;
(b) the workspace sizes of the commit before the plan existed (its build, B = 37, aligned pointers);
(c) the error paths that return before any launch.
"""
import ctypes

import pytest

GR_ERR_ARG, GR_ERR_UNSUPPORTED, GR_ERR_WORKSPACE = -1, -2, -4
OK, ODD = 0x10000, 0x10004
BLOCK_FIELDS = ("attn_ln_w", "attn_ln_b", "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b",
                "ffn_ln_w", "ffn_ln_b", "ffn1_w", "ffn1_b", "ffn2_w", "ffn2_b")
DEFAULTS = {"sas_fused": 2, "sas_rowtile": 1, "attn_k16": 1, "emb_proj": 1}


class Model:
    """A ``SasrecParams`` over fake addresses; ``odd``: {(field, block)} given the misaligned one."""

    def __init__(self, shape, odd=(), max_len=None, **over):
        from gr_amd import _lib as L
        d, heads, mlp, n, blocks = shape
        self.arrays = {f: (ctypes.c_void_p * max(1, blocks))(*[ODD if (f, i) in odd else OK for i in range(blocks)])
                       for f in BLOCK_FIELDS}
        vals = dict(d=d, n_blocks=blocks, n_heads=heads, mlp=mlp, max_len=n if max_len is None else max_len,
                    eps=1e-8, item_rows=601, item_emb=OK, pos_emb=OK, last_ln_w=OK, last_ln_b=OK)
        vals.update({f: ctypes.cast(a, ctypes.c_void_p) for f, a in self.arrays.items()})
        vals.update(over)
        self.p = L.SasrecParams(**vals)
        self.n = n

    def plan(self, last_only, B=37):
        import gr_amd
        return gr_amd.lib().gr_sasrec_plan(ctypes.byref(self.p), B, self.n, last_only)


@pytest.fixture
def options():
    from gr_amd import _lib as L

    def put(**opts):
        for k, v in opts.items():
            L.set_option(k, v)
    yield put
    for k, v in DEFAULTS.items():
        L.set_option(k, v)


def bits(names):
    from gr_amd import _lib as L
    m = 0
    for nm in names.split():
        m |= getattr(L, "GR_SAS_" + nm)
    return m


C3, C5 = (64, 1, 64, 50, 2), (128, 1, 64, 200, 2)
LAST, FULL = 1, 0
# (shape, options, last_only, B, misaligned, the whole expected mask); TAIL_VALU: 37 <= the CU count (256
# where no device answers)
TABLE = [
    (C3, dict(sas_fused=1), LAST, 37, (), "FUSED"),
    (C3, dict(sas_fused=3), LAST, 37, (), "FUSED FUSED_TWO_WAVES"),
    (C3, dict(sas_fused=2), LAST, 1, (), "FUSED FUSED_TWO_WAVES"),          # k2 == 1 on any CU count
    (C3, dict(sas_fused=0), LAST, 37, (), "LAYERWISE ATTN_PERSIST TAIL TAIL_VALU"),   # hd 64
    (C3, dict(sas_fused=0), FULL, 37, (), "LAYERWISE ATTN_PERSIST"),
    # defaults (sas_fused 2): 37 sequences are one round of the two-wave form wherever 2 CUs >= 37; n <= 32: one wave
    ((48, 2, 96, 33, 3), {}, LAST, 37, (), "FUSED FUSED_TWO_WAVES"),
    ((64, 8, 128, 64, 8), {}, FULL, 37, (), "FUSED FUSED_TWO_WAVES"),
    ((64, 1, 64, 20, 0), {}, FULL, 37, (), "FUSED"),
    (C5, {}, LAST, 37, (), "ROWTILE B0_EMBED_PROJ ATTN_K16 TAIL TAIL_VALU"),
    (C5, {}, FULL, 37, (), "ROWTILE B0_EMBED_PROJ ATTN_K16"),
    (C5, dict(attn_k16=0), LAST, 37, (), "ROWTILE B0_EMBED_PROJ ATTN_PERSIST TAIL TAIL_VALU"),
    (C5, dict(emb_proj=0), LAST, 37, (), "ROWTILE B0_EMBED_LN_LINEAR ATTN_K16 TAIL TAIL_VALU"),
    (C5, dict(sas_rowtile=0), LAST, 37, (), "LAYERWISE ATTN_K16 TAIL TAIL_VALU"),
    ((128, 2, 32, 77, 3), {}, LAST, 37, (), "ROWTILE B0_EMBED_PROJ ATTN_PERSIST TAIL TAIL_VALU"),   # hd 64
    ((128, 4, 128, 33, 1), {}, FULL, 37, (), "ROWTILE B0_EMBED_PROJ ATTN_MFMA"),                      # hd 32
    ((128, 4, 128, 33, 1), {}, LAST, 37, (), "ROWTILE B0_EMBED_LN TAIL TAIL_VALU"),                   # no attention
    ((128, 8, 64, 33, 2), {}, LAST, 37, (), "LAYERWISE ATTN_SCALAR TAIL TAIL_VALU"),                  # hd 16
    # mlp / 4 = 25 is no power of two: no tail
    ((128, 2, 100, 77, 2), {}, LAST, 37, (), "LAYERWISE ATTN_PERSIST ATTN_LAST_TILE PRUNED"),
    ((20, 5, 12, 70, 2), {}, LAST, 37, (), "LAYERWISE ATTN_SCALAR PRUNED"),
    ((128, 1, 100, 1, 2), {}, LAST, 37, (), "LAYERWISE ATTN_K16"),                                    # n < 2
    ((128, 2, 256, 40, 1), {}, LAST, 37, (), "LAYERWISE TAIL TAIL_VALU"),          # mlp 256: not row-tile
    ((64, 2, 128, 100, 2), {}, LAST, 37, (), "LAYERWISE ATTN_MFMA TAIL TAIL_VALU"),   # n > 64, hd 32
    # a LayerNorm weight a row-tile kernel reads as float4: layer-wise from the start.  Block 1's FFN
    # LayerNorm is read by the final block's post_attn kernel, which a last-position forward replaces
    # with the tail (that kernel has no aligned read of it): only the full forward leaves the row tiles
    (C5, {}, LAST, 37, {("attn_ln_w", 0)}, "LAYERWISE ATTN_K16 TAIL TAIL_VALU"),
    (C5, {}, FULL, 37, {("attn_ln_w", 0)}, "LAYERWISE ATTN_K16"),
    (C5, {}, FULL, 37, {("ffn_ln_w", 1)}, "LAYERWISE ATTN_K16"),
    (C5, {}, LAST, 37, {("ffn_ln_w", 1)}, "ROWTILE B0_EMBED_PROJ ATTN_K16 TAIL TAIL_VALU"),
    # a weight the tail needs aligned: no tail, and so no row tiles for a last-position forward
    (C5, {}, LAST, 37, {("ffn2_w", 1)}, "LAYERWISE ATTN_K16 ATTN_LAST_TILE PRUNED"),
    (C5, {}, LAST, 1, (), "ROWTILE B0_EMBED_PROJ ATTN_K16 TAIL TAIL_VALU"),
    (C5, {}, LAST, 2 ** 20, (), "ROWTILE B0_EMBED_PROJ ATTN_K16 TAIL"),
    # a fused shape the kernel cannot read: still the fused plan (its workspace), flagged
    (C3, dict(sas_fused=1), LAST, 37, {("ffn1_b", 0)}, "FUSED FUSED_MISALIGNED"),
]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{'-'.join(map(str, r[0]))}-{r[1]}-{r[2]}-B{r[3]}-{sorted(r[4])}")
def test_plan_table(row, options):
    shape, opts, last_only, B, odd, want = row
    options(**opts)
    got = Model(shape, odd).plan(last_only, B)
    assert got == bits(want), (hex(got), hex(bits(want)))


WORKSPACES = [
    (C3, dict(sas_fused=2), 9728, 10240),
    (C3, dict(sas_fused=0), 3315456, 3315968),
    (C5, dict(sas_rowtile=1), 24627456, 24627968),
    (C5, dict(sas_rowtile=0), 24627456, 24627968),
    ((128, 2, 100, 77, 2), {}, 9892096, 9892608),
    ((48, 2, 100, 70, 2), {}, 4020480, 4020992),
    ((64, 2, 128, 100, 2), {}, 7577856, 7578368),
]


@pytest.mark.parametrize("shape,opts,ws,rank_ws", WORKSPACES)
def test_workspace_sizes_have_not_moved(shape, opts, ws, rank_ws, options):
    import gr_amd
    lib = gr_amd.lib()
    options(**opts)
    m = Model(shape)
    assert lib.gr_sasrec_workspace_bytes(ctypes.byref(m.p), 37, m.n) == ws
    assert lib.gr_sasrec_rank_workspace_bytes(ctypes.byref(m.p), 37, m.n) == rank_ws


def test_errors_come_before_any_launch():
    """The pointers are fake: a launch would not return."""
    import gr_amd
    lib = gr_amd.lib()
    m = Model(C3)
    rc = lib.gr_sasrec_forward_f32(ctypes.byref(m.p), OK, 4, m.n, OK, 1, OK, 16, None, None)
    assert rc == GR_ERR_WORKSPACE and lib.gr_last_error() == b"sasrec: workspace too small (need 1280 bytes)"
    m = Model(C3, {("ffn1_b", 0)})
    for last_only in (0, 1):
        rc = lib.gr_sasrec_forward_f32(ctypes.byref(m.p), OK, 4, m.n, OK, last_only, OK, 1 << 20, None, None)
        msg = lib.gr_last_error()
        assert rc == GR_ERR_UNSUPPORTED and b"aligned" in msg and b"refused a shape" not in msg, (rc, msg)
    rc = lib.gr_sasrec_predict_f32(ctypes.byref(m.p), OK, 4, m.n, OK, OK, 1 << 20, None, None)
    assert rc == GR_ERR_UNSUPPORTED and b"aligned" in lib.gr_last_error()
    rc = lib.gr_sasrec_rank_f32(ctypes.byref(m.p), OK, 4, m.n, OK, 1, OK, OK, 1 << 20, None, 0, None, None)
    assert rc == GR_ERR_UNSUPPORTED and b"aligned" in lib.gr_last_error()


def test_plan_returns_the_parameter_checks_codes():
    import gr_amd
    lib = gr_amd.lib()
    cases = [(Model((64, 3, 64, 50, 2)), GR_ERR_UNSUPPORTED, b"multiple of 4 and of num_heads"),
             (Model(C3, max_len=49), GR_ERR_ARG, b"outside [1, max_len]"),
             (Model(C3, item_emb=None), GR_ERR_ARG, b"null embedding")]
    for m, code, text in cases:
        assert m.plan(1) == code and text in lib.gr_last_error(), (m.plan(1), lib.gr_last_error())
    assert lib.gr_sasrec_plan(None, 37, 50, 1) == GR_ERR_ARG
    assert Model(C3).plan(1) >= 0 and lib.gr_last_error() == b""
