"""Per-stage float64 checks of the BERT encoder's bf16 precision (``gr_bert_embed_bf16``, ``gr_bert_embed_ragged_bf16``)
on the call's OWN operands: the helper of test_bert_bf16_stages_gpu.py (the kernels) and test_bert_bf16_stages_ref.py
(an emulated device, with and without injected mistakes).  No test lives here.

End to end the bf16 call can only be held to about 1e-2 of float64: a value that float32 and float64 place on different
sides of a bf16 tie moves by a whole bf16 ulp, and attention spreads that over the sequence.  Stage by stage there is no
such ambiguity.  The caller owns the call's workspace, and on return it still holds the last layer's intermediates (the
layout is in include/gr_amd.h: x, t fp32; x16, qkv, ctx, ff bf16), so each stage's output can be compared with the
float64 value of that stage ON THE OPERANDS THE KERNEL ITSELF READ, and must be its correct rounding up to fp32 noise.
Two bindings over the same weights -- ``A`` with layer 0 alone, ``B`` with both layers -- give every operand exactly:
the call is bitwise deterministic, so ``A``'s hidden_out and x16 are the residual and the GEMM operand that ``B``'s
second layer consumed.

Stage restatements, generic in dtype (float64: the oracle; float32: measures delta):
    gemm        a16 @ W16^T + bias; the float32 run is the kernel's single chain, k ascending in 16-deep steps
    attention   the kernel's online softmax over 32-key tiles in ascending order from its own bf16 q, k, v: tiles with
                no live key skipped; mn = max(m, live max), alpha = exp(m - mn), p = bf16(exp(s - mn)) (0 when masked),
                l = l alpha + sum(p) of the ROUNDED values, o = o alpha + p v; ctx = o / l, 0 when l = 0
    LayerNorm, exact-erf GELU, the poolings: tests/bert_embed_ref.py

Criteria (delta = 4 x the largest distance between the stage's float32 and float64 restatements on the same operands:
the project's 4 x rule, measured against the restatement, never against the kernel):
    rounded     |got - y64| <= 1/2 ulp_bf16(|y64| + delta) + delta, every element
    close32     max |got - y64| <= delta
    attention   has one rounding point inside it, the weights, where a flip is legitimate.  delta is taken over the
                (sequence, head, query) rows whose float32 weights equal the float64 ones bit for bit; at most 5 % of the
                rows may hold an element outside ``rounded``, and those must lie within
                1/2 ulp + delta + 2^-8 sum_j p_ij |v_jd| (every weight rounded the wrong way).  The float32
                restatement's own flipped-row share must stay <= 2.5 %: the cap is a condition on the case, not a
                measurement.

Cases: the shapes of tests/bert_cases.py and ``bert_bf16_ref.WIDE`` at two layers each, seeds 321-325; ``tiny`` with a
dead sequence (lengths 33 1 2 17 0 5).
"""
import functools
import math

import torch

import bert_bf16_ref as bref
import bert_cases as bc
import bert_embed_ref as ref

PARTS = ("x", "t", "x16", "qkv", "ctx", "ff")
KT = 32                      # keys per tile of be_attn_bf16_kernel
FLIP_CAP, REF_FLIP_CAP = 0.05, 0.025

#  name         shape from                     B    S   mask                     types  seed
CASES = {
    "tiny":       (bc.CASES["tiny"][0],        6,  33, [33, 1, 2, 17, 0, 5],     False, 321),
    "heads32":    (bc.CASES["heads32"][0],     5,  65, "holes",                  True,  322),
    "base_width": (bc.CASES["base_width"][0],  3, 130, [130, 64, 7],             False, 323),
    "long":       (bc.CASES["long"][0],        2, 512, [512, 257],               False, 324),
    "wide":       (bref.WIDE[0],               1,  48, [48],                     False, 325),
}
NAMES = list(CASES)


class Case:
    def __init__(self, name):
        delta, B, S, recipe, types, seed = CASES[name]
        self.name = name
        self.cfg = dict(bc.BASE, **dict(delta, num_hidden_layers=2))
        self.cfg1 = dict(self.cfg, num_hidden_layers=1)          # binding A: layer 0 alone, the same tensors
        self.B, self.S = B, S
        self.sd = bc.state(self.cfg, seed)
        self.ids, self.mask, self.type_ids = bc.inputs(self.cfg, B, S, recipe, types, seed)
        self.H, self.I = int(self.cfg["hidden_size"]), int(self.cfg["intermediate_size"])
        self.nh = int(self.cfg["num_attention_heads"])
        self.hd = self.H // self.nh
        self.eps = float(self.cfg["layer_norm_eps"])
        self.live = self.mask != 0
        self.alive = self.live.any(dim=1)                        # [B]: the sequence has a live key
        self.lens = [max((i + 1 for i, v in enumerate(row) if v != 0), default=0) for row in self.mask.tolist()]

    def w16(self, layer, key):
        """The matrix as ``BertBf16Binding`` rounds it."""
        return self.sd[f"encoder.layer.{layer}.{key}.weight"].to(torch.bfloat16)

    def vec(self, layer, key):
        return self.sd[f"encoder.layer.{layer}.{key}"]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---------------------------------------------------------------------------------------------- the workspace

def up16(n):
    return (n + 15) // 16 * 16


def layout(cfg, R):
    """Byte offsets of the six parts and their total, by include/gr_amd.h's formula."""
    H, I = int(cfg["hidden_size"]), int(cfg["intermediate_size"])
    sizes = dict(x=R * H * 4, t=R * H * 4, x16=R * H * 2, qkv=R * 3 * H * 2, ctx=R * H * 2, ff=R * I * 2)
    off, o = {}, 0
    for k in PARTS:
        off[k] = o
        o += up16(sizes[k])
    return off, sizes, o


def views(ws_uint8, cfg, R):
    """The six parts of a bf16 call's workspace as torch views: x, t float32 [R, H]; x16, ctx bfloat16 [R, H]; qkv
    bfloat16 [R, 3H]; ff bfloat16 [R, I]."""
    H, I = int(cfg["hidden_size"]), int(cfg["intermediate_size"])
    off, sizes, total = layout(cfg, R)
    assert ws_uint8.dtype == torch.uint8 and ws_uint8.numel() >= total
    cols = dict(x=H, t=H, x16=H, qkv=3 * H, ctx=H, ff=I)
    out = {}
    for k in PARTS:
        raw = ws_uint8[off[k]:off[k] + sizes[k]]
        out[k] = raw.view(torch.float32 if k in ("x", "t") else torch.bfloat16).view(R, cols[k])
    return out


def _dev(t, dev):
    return None if t is None else t.to(dev)


def call(binding, ids, mask, tt, pooling):
    """The padded C entry as ``ops.bert_embed`` calls it, on a workspace this helper owns, 0xFF-filled before the call
    so that stale or unwritten data reads as NaN.  -> pooled [B, H], hidden [B, S, H], the six views (on the device)."""
    from gr_amd import _lib as L
    from gr_amd import ops
    dev = binding.device
    B, S = ids.shape
    H = binding.params.hidden_size
    ids, mask, tt = _dev(ids, dev), _dev(mask, dev), _dev(tt, dev)
    nbytes = binding.workspace_bytes(B, S)
    assert layout(binding.cfg, B * S)[2] + 16 == nbytes, "the bf16 workspace layout changed"
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    pooled = torch.full((B, H), float("nan"), dtype=torch.float32, device=dev)
    hidden = torch.full((B, S, H), float("nan"), dtype=torch.float32, device=dev)
    with L.on(dev):
        L.check(getattr(L.lib(), binding.ENTRY)(binding.ref, L.ptr(ids), L.ptr(mask), L.ptr(tt), B, S,
                                                ops.BERT_POOLINGS[pooling], L.ptr(pooled), L.ptr(hidden), L.ptr(ws),
                                                nbytes, L.stream_of(dev)), binding.ENTRY)
    return pooled, hidden, views(ws, binding.cfg, B * S)


def call_ragged(binding, ids, mask, tt, pooling, rows):
    """The ragged C entry likewise, with ``rows`` as its row bound.  -> pooled, hidden_rows [rows, H], offsets [B + 1],
    the six views over ``rows`` packed rows."""
    from gr_amd import _lib as L
    from gr_amd import ops
    dev = binding.device
    B, S = ids.shape
    H = binding.params.hidden_size
    ids, mask, tt = _dev(ids, dev), _dev(mask, dev), _dev(tt, dev)
    nbytes = binding.ragged_workspace_bytes(B, S, rows)
    assert layout(binding.cfg, rows)[2] + up16(8 * (B + 1)) + 16 + up16(4 * B) + 16 == nbytes, \
        "the ragged bf16 workspace layout changed"
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    pooled = torch.full((B, H), float("nan"), dtype=torch.float32, device=dev)
    hidden = torch.full((rows, H), float("nan"), dtype=torch.float32, device=dev)
    offsets = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    with L.on(dev):
        L.check(getattr(L.lib(), binding.RAGGED_ENTRY)(binding.ref, L.ptr(ids), L.ptr(mask), L.ptr(tt), B, S, rows,
                                                       ops.BERT_POOLINGS[pooling], L.ptr(pooled), L.ptr(hidden),
                                                       L.ptr(offsets), L.ptr(ws), nbytes, L.stream_of(dev)),
                binding.RAGGED_ENTRY)
    return pooled, hidden, offsets, views(ws, binding.cfg, rows)


def device_run(binding, c):
    """One run of case ``c`` on ``binding``, on the CPU: the six parts, hidden [B, S, H], mean_no_cls, cls.  Two calls
    (one per pooling); the second must leave the first's bits in every part."""
    mean, hidden, v = call(binding, c.ids, c.mask, c.type_ids, "mean_no_cls")
    run = {k: t.cpu() for k, t in v.items()}
    run["hidden"], run["mean_no_cls"] = hidden.cpu(), mean.cpu()
    cls, hidden2, v2 = call(binding, c.ids, c.mask, c.type_ids, "cls")
    run["cls"] = cls.cpu()
    for k in PARTS:
        assert torch.equal(bits(v2[k].cpu()), bits(run[k])), k
    assert torch.equal(bits(hidden2.cpu()), bits(run["hidden"]))
    return run


def bits(t):
    """The tensor's bytes as int16, for comparisons that NaN cannot confuse."""
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------ stage restatements

def rne(t):
    """Round-to-nearest-even to bf16.  float64 goes through float32 first: exp(s - mn) of the float64 attention run is
    rounded twice, which differs from one rounding only within 2^-24 (relative) of a bf16 tie -- where float32 and
    float64 disagree anyway: a flip like any other, and counted with them."""
    return t.to(torch.float32).to(torch.bfloat16)


def gemm(a16, w16, bias, dtype, k_stop=None, step=16):
    """a16 [R, K] bf16, w16 [N, K] bf16, bias [N] float32 -> a16 @ w16^T + bias in ``dtype``.  float32: the kernel's
    single accumulation chain, k ascending in ``step``-deep steps.  ``k_stop``: the chain ends there (a mistake)."""
    K = a16.shape[1] if k_stop is None else k_stop
    a, w = a16.to(dtype), w16.to(dtype)
    if dtype == torch.float64:
        return a[:, :K] @ w[:, :K].T + bias.to(dtype)
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=dtype)
    for k in range(0, K, step):
        e = min(k + step, K)
        acc = acc + (a[:, k:e] @ w[:, k:e].T)
    return acc + bias


def attention(qkv16, live, nh, dtype, noise=None, mistake=None):
    """qkv16 [B, S, 3H] bf16 (the kernel's own q | k | v), live [B, S] bool -> (ctx [B, S, H] in ``dtype``, unrounded;
    the rounded un-normalised weights [B, nh, S, S] float32, 0 where masked or skipped; sum_j p_ij |v_jd| / l
    [B, S, H]).  ``noise`` [B, nh, S, S]: relative perturbation of the scores (the emulated device).
    ``mistake``: "trunc_weights", "fp32_row_sum" or "normalise_then_round"."""
    B, S, H3 = qkv16.shape
    H = H3 // 3
    hd = H // nh
    q, k, v = (qkv16[..., i * H:(i + 1) * H].to(dtype).view(B, S, nh, hd).transpose(1, 2) for i in range(3))
    scale = torch.tensor(1.0 / hd, dtype=torch.float64).sqrt().to(dtype)
    s = (q @ k.transpose(-1, -2)) * scale
    if noise is not None:
        s = s * (1 + noise.to(dtype))
    s = s.masked_fill(~live[:, None, None, :], float("-inf"))
    if mistake == "normalise_then_round":
        pr = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
        pr = rne(pr).to(dtype)
        return (pr @ v).transpose(1, 2).reshape(B, S, H), pr.float(), None
    m = torch.full((B, nh, S, 1), float("-inf"), dtype=dtype)
    l = torch.zeros(B, nh, S, 1, dtype=dtype)
    o = torch.zeros(B, nh, S, hd, dtype=dtype)
    oabs = torch.zeros(B, nh, S, hd, dtype=dtype)
    weights = torch.zeros(B, nh, S, S, dtype=torch.float32)
    for t0 in range(0, S, KT):
        visit = live[:, t0:t0 + KT].any(dim=1)                       # [B]: the tile has a live key
        if not bool(visit.any()):
            continue
        vis = visit[:, None, None, None]
        st = s[..., t0:t0 + KT]
        mn = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
        mn = torch.where(vis, mn, torch.zeros_like(mn))               # a skipped tile: any finite value, unused
        alpha = torch.exp(m - mn)
        e = torch.exp(st - mn)
        p = (_truncate(e) if mistake == "trunc_weights" else rne(e)).to(dtype)
        terms = e if mistake == "fp32_row_sum" else p
        if noise is not None:
            terms = terms.flip(-1)                                    # the emulated device adds in the other order
        total = terms.sum(dim=-1, keepdim=True)
        vt = v[:, :, t0:t0 + KT]
        l = torch.where(vis, l * alpha + total, l)
        o = torch.where(vis, o * alpha + p @ vt, o)
        oabs = torch.where(vis, oabs * alpha + p @ vt.abs(), oabs)
        m = torch.where(vis, mn, m)
        weights[..., t0:t0 + KT] = torch.where(vis, p, torch.zeros_like(p)).float()
    some = l > 0
    safe = torch.where(some, l, torch.ones_like(l))
    ctx = torch.where(some, o / safe, torch.zeros_like(o))
    spread = torch.where(some, oabs / safe, torch.zeros_like(o))
    back = lambda t: t.transpose(1, 2).reshape(B, S, H)
    return back(ctx), weights, back(spread)


def _truncate(t):
    """Round-toward-zero to bf16: what dropping the low 16 bits of the fp32 gives (a mistake)."""
    return (t.to(torch.float32).contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def embeddings(c, dtype):
    """The embedding LayerNorm from the tables, [B * S, H]."""
    w = lambda k: c.sd["embeddings." + k].to(dtype)
    tt = torch.zeros_like(c.ids) if c.type_ids is None else c.type_ids
    x = (w("word_embeddings.weight")[c.ids] + w("token_type_embeddings.weight")[tt]) \
        + w("position_embeddings.weight")[:c.S]
    return ref.layer_norm(x, w("LayerNorm.weight"), w("LayerNorm.bias"), c.eps).reshape(c.B * c.S, c.H)


def tanh_gelu(t):
    return 0.5 * t * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (t + 0.044715 * t ** 3)))


# ------------------------------------------------------------------------------------------------- criteria

def half_ulp_bf16(a):
    """1/2 ulp of bf16 at magnitude ``a`` (float64, >= 0): 2^(e - 8) for a in [2^e, 2^(e + 1)), e >= -126."""
    _, ex = torch.frexp(a)                                   # a = m 2^ex, m in [0.5, 1): e = ex - 1
    e = torch.where(a > 0, ex - 1, torch.full_like(ex, -126)).clamp(min=-126)
    return torch.ldexp(torch.ones_like(a), e - 8)


class Stage:
    """One stage's float64 value on the device's own operands, and its delta.  kind: "rounded", "close32" or
    "attention"; ``rows`` [R] bool: the rows compared (None: all); ``extra``: the attention stage's spread and the
    rows that must be exactly 0."""

    def __init__(self, name, kind, y64, y32, rows=None, extra=None, on32=None):
        self.name, self.kind, self.y64, self.rows, self.extra = name, kind, y64, rows, extra or {}
        d = (y32.double() - y64).abs()
        if rows is not None:
            d = d[rows]
        if on32 is not None:                                   # attention: only rows without a flip measure delta
            d = d[on32 if rows is None else on32[rows]]
        self.delta = 4.0 * (d.max().item() if d.numel() else 0.0)


class Verdict:
    def __init__(self, stage, ok, text, **figures):
        self.stage, self.ok, self.text, self.figures = stage, ok, text, figures

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return ("ok   " if self.ok else "FAIL ") + self.text


def rounded(got16, y64, delta):
    """-> (outside [..] bool, excess = max(|got - y64| - 1/2 ulp, 0) [..]) for bf16 ``got16``."""
    err = (got16.double() - y64).abs()
    hu = half_ulp_bf16(y64.abs() + delta)
    return ~(err <= hu + delta), (err - hu).clamp(min=0.0)


def judge(st, got):
    """Compare the device's part ``got`` (rows as the stage's y64) with the stage.  Prints nothing; the Verdict's text
    holds the figures: the device's own fp32 noise next to delta."""
    y64, rows = st.y64, st.rows
    g = got if rows is None else got[rows]
    y = y64 if rows is None else y64[rows]
    if bool(torch.isnan(g.float()).any()):
        return Verdict(st.name, False, f"{st.name}: NaN in the compared rows (a part that was not written)")
    if st.kind == "close32":
        err = (g.double() - y).abs().max().item() if g.numel() else 0.0
        return Verdict(st.name, err <= st.delta, f"{st.name}: device max |got - y64| {err:.3e}, delta {st.delta:.3e}",
                       noise=err, delta=st.delta)
    if st.kind == "rounded":
        out, excess = rounded(g, y, st.delta)
        n, worst = int(out.sum()), (excess.max().item() if g.numel() else 0.0)
        return Verdict(st.name, n == 0, f"{st.name}: device noise beyond 1/2 ulp {worst:.3e}, delta {st.delta:.3e}, "
                       f"{n} of {out.numel()} elements outside ({100.0 * n / max(out.numel(), 1):.2f} %)",
                       noise=worst, delta=st.delta, outside=n / max(out.numel(), 1))
    assert st.kind == "attention"
    zero = st.extra["zero_rows"]
    dead_ok = bool((got[zero].float() == 0).all())
    spread = st.extra["spread"] if rows is None else st.extra["spread"][rows]
    hd = st.extra["hd"]
    out, excess = rounded(g, y, st.delta)
    err = (g.double() - y).abs()
    loose = err <= half_ulp_bf16(y.abs() + st.delta) + st.delta + 2.0 ** -8 * spread
    per_row = out.view(out.shape[0], -1, hd).any(dim=-1)                  # (row, head)
    share = per_row.double().mean().item() if per_row.numel() else 0.0
    inside = excess[~out]
    worst = inside.max().item() if inside.numel() else 0.0
    units = (err / half_ulp_bf16(y.abs() + st.delta) / 2.0).max().item() if g.numel() else 0.0
    ok = dead_ok and share <= FLIP_CAP and bool(loose.all())
    return Verdict(st.name, ok, f"{st.name}: device noise beyond 1/2 ulp {worst:.3e} on the rows inside, delta "
                   f"{st.delta:.3e}, {100.0 * share:.2f} % of (sequence, head, query) rows outside (cap "
                   f"{100.0 * FLIP_CAP:.0f} %, the float32 restatement's flipped share "
                   f"{100.0 * st.extra['ref_flipped']:.2f} %), {int((~loose).sum())} elements past the every-weight-"
                   f"flipped bound, worst error {units:.1f} ulp, dead sequences {'zero' if dead_ok else 'NOT zero'}",
                   noise=worst, delta=st.delta, outside=share)


# ------------------------------------------------------------------------------------------- what to expect

def _both(f):
    return f(torch.float64), f(torch.float32)


def _seq_rows(c, keep):
    """[B * S] bool: the rows of the sequences ``keep`` [B] bool."""
    return keep[:, None].expand(c.B, c.S).reshape(-1)


def stages(c, layer, run, prev):
    """name -> Stage for the ``layer`` whose intermediates ``run`` holds (its last one), from ``run``'s own parts.
    ``prev``: the run of the binding that ends one layer earlier (its hidden and x16 are this layer's inputs), or None
    for layer 0, whose input is the embedding LayerNorm from the tables (no rounding upstream)."""
    with torch.no_grad():
        return _stages(c, layer, run, prev)


def _stages(c, layer, run, prev):
    S, H, out = c.S, c.H, {}
    alive_rows = _seq_rows(c, c.alive)

    def vec(k, dtype):
        return c.vec(layer, k).to(dtype)

    # 1. q | k | v from the previous run's x16 (layer 1 only: layer 0's operand is overwritten)
    if prev is not None:
        w = torch.cat([c.w16(layer, "attention.self." + n) for n in ("query", "key", "value")])
        b = torch.cat([c.vec(layer, f"attention.self.{n}.bias") for n in ("query", "key", "value")])
        y64, y32 = _both(lambda dt: gemm(prev["x16"], w, b, dt))
        out["qkv"] = Stage("qkv", "rounded", y64, y32)

    # 2. the context from the run's own qkv
    qkv = run["qkv"].view(c.B, S, 3 * H)
    c64, w64, spread = attention(qkv, c.live, c.nh, torch.float64)
    c32, w32, _ = attention(qkv, c.live, c.nh, torch.float32)
    same = (w32 == w64).all(dim=-1)                                        # [B, nh, S]
    counted = same[c.alive]
    flipped = 1.0 - counted.double().mean().item()
    assert flipped <= REF_FLIP_CAP, (c.name, layer, "the float32 restatement's own flipped rows", flipped)
    on32 = same.transpose(1, 2)[..., None].expand(c.B, S, c.nh, c.hd).reshape(c.B * S, H)
    out["ctx"] = Stage("ctx", "attention", c64.reshape(c.B * S, H), c32.reshape(c.B * S, H), rows=alive_rows,
                       extra=dict(spread=spread.reshape(c.B * S, H), zero_rows=~alive_rows, hd=c.hd,
                                  ref_flipped=flipped), on32=on32)

    # 3. x = LN(residual + attention.output.dense(ctx)); the residual: prev's hidden (zeroed for a dead sequence:
    #    those rows are skipped) or the embeddings
    def post_attention(dt):
        resid = embeddings(c, dt) if prev is None else prev["hidden"].reshape(c.B * S, H).to(dt)
        g = gemm(run["ctx"], c.w16(layer, "attention.output.dense"), vec("attention.output.dense.bias", dt), dt)
        return ref.layer_norm(resid + g, vec("attention.output.LayerNorm.weight", dt),
                              vec("attention.output.LayerNorm.bias", dt), c.eps)
    y64, y32 = _both(post_attention)
    out["x"] = Stage("x", "close32", y64, y32, rows=None if prev is None else alive_rows)

    # 4. ff = gelu(intermediate.dense(RNE(x)))
    x16 = rne(run["x"])
    y64, y32 = _both(lambda dt: ref.gelu(gemm(x16, c.w16(layer, "intermediate.dense"),
                                              vec("intermediate.dense.bias", dt), dt)))
    out["ff"] = Stage("ff", "rounded", y64, y32)

    # 5. t = x + output.dense(ff)
    y64, y32 = _both(lambda dt: run["x"].to(dt) + gemm(run["ff"], c.w16(layer, "output.dense"),
                                                       vec("output.dense.bias", dt), dt))
    out["t"] = Stage("t", "close32", y64, y32)

    # 6. hidden = LN(t) (live sequences: hidden_out is zeroed for a dead one; its x16 is not, and must be the rounding)
    y64, y32 = _both(lambda dt: ref.layer_norm(run["t"].to(dt), vec("output.LayerNorm.weight", dt),
                                               vec("output.LayerNorm.bias", dt), c.eps))
    out["hidden"] = Stage("hidden", "close32", y64, y32, rows=alive_rows)
    out["x16_dead"] = Stage("x16_dead", "rounded", y64, y32, rows=~alive_rows)

    # 7. the poolings of the run's own hidden state
    for k in ("mean_no_cls", "cls"):
        y64, y32 = _both(lambda dt: ref.pool(run["hidden"].to(dt), c.mask, k))
        out[k] = Stage(k, "close32", y64, y32)
    return out


def judge_all(c, st, run):
    """Every check of one run against its stages -> [Verdict]."""
    R, H = c.B * c.S, c.H
    alive_rows = _seq_rows(c, c.alive)
    vs = []
    for k in PARTS + ("hidden", "mean_no_cls", "cls"):
        bad = bool(torch.isnan(run[k].float()).any())
        vs.append(Verdict("written", not bad, f"written: {k} {'holds NaN' if bad else 'has no NaN'}"))
    for name, part in (("qkv", "qkv"), ("ctx", "ctx"), ("x", "x"), ("ff", "ff"), ("t", "t"), ("x16_dead", "x16")):
        if name in st:
            vs.append(judge(st[name], run[part]))
    hidden = run["hidden"].reshape(R, H)
    vs.append(judge(st["hidden"], hidden))
    dead_zero = bool((hidden[~alive_rows] == 0).all())
    vs.append(Verdict("hidden", dead_zero, f"hidden: dead sequences {'zero' if dead_zero else 'NOT zero'}"))
    vs.append(x16_is_rne(c, run))
    vs.append(judge(st["mean_no_cls"], run["mean_no_cls"]))
    vs.append(judge(st["cls"], run["cls"]))
    return vs


def x16_is_rne(c, run):
    """x16 == RNE(hidden_out) bit for bit on the live sequences."""
    alive_rows = _seq_rows(c, c.alive)
    want = rne(run["hidden"].reshape(c.B * c.S, c.H))[alive_rows].view(torch.int16)
    n = int((run["x16"][alive_rows].view(torch.int16) != want).sum())
    return Verdict("x16", n == 0, f"x16: {n} of {want.numel()} elements differ from RNE(hidden_out)")


def report(name, layer, verdicts):
    for v in verdicts:
        if v.stage != "written" or not v.ok:
            print(f"{name} layer {layer}: {v!r}")
    return [v for v in verdicts if not v.ok]


# ------------------------------------------------------------------------------------------ the emulated device

def emulate(c, layers, seed=7):
    """The call in float32 on the CPU, as an honest device would run it but not as the restatement does: GEMM chains
    in 64-deep steps, scores perturbed by relative 2^-23 noise (so its weight flips differ from the restatement's), the
    row sum added in the other order.  -> the same dict ``device_run`` gives."""
    g = torch.Generator().manual_seed(seed)
    f32 = torch.float32
    B, S, H = c.B, c.S, c.H
    with torch.no_grad():
        x = embeddings(c, f32)
        x16 = rne(x)
        for layer in range(layers):
            vec = lambda k: c.vec(layer, k)
            w = torch.cat([c.w16(layer, "attention.self." + n) for n in ("query", "key", "value")])
            b = torch.cat([vec(f"attention.self.{n}.bias") for n in ("query", "key", "value")])
            qkv = rne(gemm(x16, w, b, f32, step=64))
            noise = (2 * torch.rand(B, c.nh, S, S, generator=g) - 1) * 2.0 ** -23
            ctx = rne(attention(qkv.view(B, S, 3 * H), c.live, c.nh, f32, noise=noise)[0]).reshape(B * S, H)
            t = x + gemm(ctx, c.w16(layer, "attention.output.dense"), vec("attention.output.dense.bias"), f32, step=64)
            x = ref.layer_norm(t, vec("attention.output.LayerNorm.weight"), vec("attention.output.LayerNorm.bias"), c.eps)
            x16 = rne(x)
            ff = rne(ref.gelu(gemm(x16, c.w16(layer, "intermediate.dense"), vec("intermediate.dense.bias"), f32, step=64)))
            t = x + gemm(ff, c.w16(layer, "output.dense"), vec("output.dense.bias"), f32, step=64)
            last = ref.layer_norm(t, vec("output.LayerNorm.weight"), vec("output.LayerNorm.bias"), c.eps)
            x16 = rne(last)
            if layer + 1 < layers:
                x = last
        hidden = (last * _seq_rows(c, c.alive)[:, None].float()).view(B, S, H)
        return dict(x=x, t=t, x16=x16, qkv=qkv, ctx=ctx, ff=ff, hidden=hidden,
                    mean_no_cls=ref.pool(hidden, c.mask, "mean_no_cls"), cls=ref.pool(hidden, c.mask, "cls"))


MISTAKES = ("tanh_gelu", "trunc_qkv", "trunc_ctx", "trunc_ff", "trunc_weights", "fp32_row_sum", "normalise_then_round",
            "drop_k_qkv", "drop_k_attention_output", "drop_k_intermediate", "drop_k_output", "x16_not_rne")
#: the stage whose check must fail under each mistake
CAUGHT_BY = dict(tanh_gelu="ff", trunc_qkv="qkv", trunc_ctx="ctx", trunc_ff="ff", trunc_weights="ctx",
                 fp32_row_sum="ctx", normalise_then_round="ctx", drop_k_qkv="qkv", drop_k_attention_output="x",
                 drop_k_intermediate="ff", drop_k_output="t", x16_not_rne="x16")


def mistaken(c, layer, run, prev, mistake, seed=11):
    """(part name, its value) as a device with ONE wrong step would have left it, computed from the honest run's own
    operands (every stage is checked on its own operands, so nothing downstream of the wrong stage matters)."""
    f32 = torch.float32
    B, S, H = c.B, c.S, c.H
    vec = lambda k: c.vec(layer, k)
    with torch.no_grad():
        if mistake in ("trunc_qkv", "drop_k_qkv"):
            w = torch.cat([c.w16(layer, "attention.self." + n) for n in ("query", "key", "value")])
            b = torch.cat([vec(f"attention.self.{n}.bias") for n in ("query", "key", "value")])
            y = gemm(prev["x16"], w, b, f32, step=64, k_stop=H - 16 if mistake == "drop_k_qkv" else None)
            return "qkv", (_truncate(y) if mistake == "trunc_qkv" else rne(y))
        if mistake in ("trunc_ctx", "trunc_weights", "fp32_row_sum", "normalise_then_round"):
            g = torch.Generator().manual_seed(seed)
            noise = (2 * torch.rand(B, c.nh, S, S, generator=g) - 1) * 2.0 ** -23
            y = attention(run["qkv"].view(B, S, 3 * H), c.live, c.nh, f32, noise=noise,
                          mistake=None if mistake == "trunc_ctx" else mistake)[0].reshape(B * S, H)
            return "ctx", (_truncate(y) if mistake == "trunc_ctx" else rne(y))
        if mistake == "drop_k_attention_output":
            resid = embeddings(c, f32) if prev is None else prev["hidden"].reshape(B * S, H)
            t = resid + gemm(run["ctx"], c.w16(layer, "attention.output.dense"), vec("attention.output.dense.bias"),
                             f32, step=64, k_stop=H - 16)
            return "x", ref.layer_norm(t, vec("attention.output.LayerNorm.weight"),
                                       vec("attention.output.LayerNorm.bias"), c.eps)
        if mistake in ("tanh_gelu", "trunc_ff", "drop_k_intermediate"):
            y = gemm(rne(run["x"]), c.w16(layer, "intermediate.dense"), vec("intermediate.dense.bias"), f32, step=64,
                     k_stop=H - 16 if mistake == "drop_k_intermediate" else None)
            y = tanh_gelu(y) if mistake == "tanh_gelu" else ref.gelu(y)
            return "ff", (_truncate(y) if mistake == "trunc_ff" else rne(y))
        if mistake == "drop_k_output":
            return "t", run["x"] + gemm(run["ff"], c.w16(layer, "output.dense"), vec("output.dense.bias"), f32,
                                        step=64, k_stop=c.I - 16)
        assert mistake == "x16_not_rne"
        return "x16", _truncate(run["hidden"].reshape(B * S, H))
