"""Tensor-level wrappers of the C ABI (include/gr_amd.h).

Each function takes/returns torch tensors on a ROCm device, enqueues on the current stream and
never synchronises.  Argument checking mirrors the ATen errors the reference would raise.
"""
import collections
import ctypes
import itertools
import math
import os

import torch

from . import _lib as L

# Input errors the kernels detect (an item id outside the table, a row whose negatives cannot be
# drawn) are OR-ed into a per-device sticky error word instead of synchronising the stream.
# ``check_errors()`` synchronises and raises (evaluate() calls it once per evaluation; a training
# loop calls it once per epoch).  GR_AMD_CHECK=1 checks after every call instead.
CHECK = os.environ.get("GR_AMD_CHECK", "0") == "1"
ERR_BAD_ID = 1        # item id outside [0, rows): the reference raises IndexError (nn.Embedding / gather)
ERR_NEG_POPULATION = 2  # get_neg_samples population smaller than num_neg: numpy raises ValueError
_ERR = {}


def err_flag(device):
    """The device's sticky error word (int32, 0 = clean); kernels only ever write a nonzero code."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    t = _ERR.get(idx)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
        _ERR[idx] = t
    return t


def check_errors(device=None):
    """Synchronise ``device`` and raise the error the kernels flagged since the last check (then
    clear it): IndexError for out-of-range item ids, ValueError for an unfillable negative row."""
    devs = [device] if device is not None else [torch.device("cuda", i) for i in list(_ERR)]
    for d in devs:
        t = err_flag(torch.device(d))
        code = int(t.item())              # .item() synchronises the stream the flag was written on
        if code:
            t.zero_()
            if code == ERR_NEG_POPULATION:
                raise ValueError("Cannot take a larger sample than population when 'replace=False'")
            raise IndexError("index out of range in self (item id outside the embedding table)")


def linear(x, weight, bias=None, act="none", residual=None, out=None):
    """``act(x @ weight.T + bias) (+ residual)`` — F.linear (+ the activations of
    RQ-VAE/models/layers.py:45-67: relu, sigmoid, tanh, leakyrelu) on the matrix cores."""
    L.require_gpu(x, weight)
    x2 = L.as_f32(x).reshape(-1, x.shape[-1])
    w = L.as_f32(weight)
    m, k = x2.shape
    n = w.shape[0]
    if w.shape[1] != k:
        raise RuntimeError(f"linear: shape mismatch x[..., {k}] vs weight{tuple(w.shape)}")
    b = L.as_f32(bias) if bias is not None else None
    r = L.as_f32(residual).reshape(m, n) if residual is not None else None
    y = out if out is not None else torch.empty((m, n), dtype=torch.float32, device=x.device)
    a = {"none": L.GR_ACT_NONE, "relu": L.GR_ACT_RELU, "sigmoid": L.GR_ACT_SIGMOID, "tanh": L.GR_ACT_TANH,
         "leakyrelu": L.GR_ACT_LEAKYRELU}[act]
    with L.on(x.device):
        L.check(L.lib().gr_linear_f32(L.ptr(x2), m, k, L.ptr(w), n, L.ptr(b), L.ptr(r),
                                      n if r is not None else 0, a, L.ptr(y), n,
                                      L.stream_of(x.device)), "gr_linear_f32")
    return y.reshape(*x.shape[:-1], n)


def score(h, table, out=None):
    """Full-catalog logits ``h @ table.T`` (SASRec/model.py:107)."""
    L.require_gpu(h, table)
    h = L.as_f32(h)
    t = L.as_f32(table)
    B, d = h.shape
    rows = t.shape[0]
    y = out if out is not None else logits_buffer(B, rows, h.device)
    with L.on(h.device):
        L.check(L.lib().gr_score_f32(L.ptr(h), B, d, L.ptr(t), rows, L.ptr(y), y.stride(0),
                                     L.stream_of(h.device)), "gr_score_f32")
    return y


def rank(logits, targets, mask_col0=True):
    """Strict rank of each target (SASRec/evaluate.py:27-32) without mutating ``logits``."""
    L.require_gpu(logits, targets)
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    t = targets.reshape(-1).to(torch.int64).contiguous()
    B, cols = logits.shape
    out = torch.empty(B, dtype=torch.int64, device=logits.device)
    with L.on(logits.device):
        L.check(L.lib().gr_rank_f32(L.ptr(logits), B, cols, logits.stride(0), L.ptr(t),
                                    1 if mask_col0 else 0, L.ptr(out),
                                    L.stream_of(logits.device)), "gr_rank_f32")
    return out


def count_gt(logits, thresholds):
    """``#{j : logits[b, j] > thresholds[b]}`` per row (strict, SASRec/evaluate.py:32)."""
    L.require_gpu(logits, thresholds)
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    th = L.as_f32(thresholds.reshape(-1))
    B, cols = logits.shape
    out = torch.empty(B, dtype=torch.int64, device=logits.device)
    with L.on(logits.device):
        L.check(L.lib().gr_count_gt_f32(L.ptr(logits), B, cols, logits.stride(0), L.ptr(th),
                                        L.ptr(out), L.stream_of(logits.device)), "gr_count_gt_f32")
    return out


def topk(logits, k, id_offset=0, thresholds=None):
    """Per-row top-k: (values [B,k] descending, ids [B,k] = column + id_offset); ties -> lower id.
    With ``thresholds`` the same pass also returns the strict counts ``#{j : l[b,j] > thr[b]}``."""
    L.require_gpu(logits)
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    B, cols = logits.shape
    dev = logits.device
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    th = L.as_f32(thresholds.reshape(-1)) if thresholds is not None else None
    cnt = torch.empty(B, dtype=torch.int64, device=dev) if th is not None else None
    nbytes = L.lib().gr_topk_workspace_bytes(B, cols, k)
    wsp = L.workspace(nbytes, dev)
    with L.on(dev):
        L.check(L.lib().gr_topk_f32(L.ptr(logits), B, cols, logits.stride(0), k, id_offset,
                                    L.ptr(vals), L.ptr(ids), L.ptr(th), L.ptr(cnt), L.ptr(wsp), nbytes,
                                    L.stream_of(dev)), "gr_topk_f32")
    return (vals, ids) if th is None else (vals, ids, cnt)


def score_pairs(h, table, ids, mask_col0=True):
    """Target logits ``h[b] . table[ids[b]]`` with the scoring kernel's exact fp32 chain (-1e9 for
    id 0 when ``mask_col0``, SASRec/evaluate.py:27)."""
    L.require_gpu(h, table, ids)
    h, t = L.as_f32(h), L.as_f32(table)
    ids = ids.reshape(-1).to(torch.int64).contiguous()
    B, d = h.shape
    out = torch.empty(B, dtype=torch.float32, device=h.device)
    err = err_flag(h.device)
    with L.on(h.device):
        L.check(L.lib().gr_score_pairs_f32(L.ptr(h), B, d, L.ptr(t), t.shape[0], L.ptr(ids),
                                           1 if mask_col0 else 0, L.ptr(out), L.ptr(err),
                                           L.stream_of(h.device)), "gr_score_pairs_f32")
    _check_err(err)
    return out


_COUNT_WS = {}   # (device, stream) -> zeroed workspace of gr_score_count_gt_ws_f32 (left zero by every call)
_SCRATCH = {}    # (device index, stream) -> scratch workspace of the short calls (no contents carried)
SCRATCH_CACHE_BYTES = 16 << 20


def scratch(nbytes, device):
    """Caller-owned scratch for one call (``L.workspace``), reused across the calls of one stream when
    small: a call's kernels finish with it before any later call on the same stream starts (stream
    order), and the library never keeps pointers.  Saves an allocation per call at the reference's
    batch sizes (get_indices(x[64]), rank of 128 users).  Under graph capture: a fresh allocation
    (the graph's pool owns it)."""
    if nbytes > SCRATCH_CACHE_BYTES or torch.cuda.is_current_stream_capturing():
        return L.workspace(nbytes, device)
    key = (device.index, L.stream_of(device))
    ws = _SCRATCH.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = L.workspace(max(nbytes, 1 << 16), device)
        _SCRATCH[key] = ws
    return ws


def _count_workspace(device, nbytes):
    """The count kernel's workspace, which it expects zero on entry and leaves zero on exit.
    Eager calls reuse one cached, once-zeroed buffer per (device, stream).  Under graph capture a
    fresh buffer is allocated and zeroed by a node of the graph itself, and never cached: a cached
    buffer first zeroed inside a capture holds zeros only after a replay, and the capture stream's
    key is reused by later captures."""
    if torch.cuda.is_current_stream_capturing():
        # zeroed by a fill KERNEL node of the graph (torch.zeros), so every replay starts from zeros
        return torch.zeros(nbytes, dtype=torch.uint8, device=device), None
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _COUNT_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        _COUNT_WS[key] = ws
    return ws, key


def score_count_gt(h, table, thresholds, mask_col0=True):
    """``#{j : (h . table^T)[b, j] > thresholds[b]}`` without materialising the logits."""
    L.require_gpu(h, table, thresholds)
    h, t = L.as_f32(h), L.as_f32(table)
    th = L.as_f32(thresholds.reshape(-1))
    B, d = h.shape
    out = torch.empty(B, dtype=torch.int64, device=h.device)
    with L.on(h.device):
        nb = L.lib().gr_score_count_workspace_bytes(B)
        ws, key = _count_workspace(h.device, nb)
        try:
            L.check(L.lib().gr_score_count_gt_ws_f32(L.ptr(h), B, d, L.ptr(t), t.shape[0], L.ptr(th),
                                                     1 if mask_col0 else 0, L.ptr(out), L.ptr(ws), nb,
                                                     L.stream_of(h.device)), "gr_score_count_gt_ws_f32")
        except Exception:
            if key is not None:   # a failed call may leave non-zero words: never reuse the buffer
                _COUNT_WS.pop(key, None)
            raise
    return out


def score_rank(h, table, targets, mask_col0=True):
    """Strict rank of each target over the full catalog (SASRec/evaluate.py:27-32) without
    writing the [B, rows] logits: count_gt(h, table, pairs(h, table, targets)) + 1."""
    return score_count_gt(h, table, score_pairs(h, table, targets, mask_col0), mask_col0) + 1


def score_topk(h, table, k, id_offset=0, thresholds=None, mask_col0=True):
    """Top-k of ``h @ table.T`` per user without writing the logits: (values [B,k] descending,
    ids [B,k] = column + id_offset; ties -> lower id), column 0 taken as -1e9 when ``mask_col0``
    (SASRec/evaluate.py:27).  With ``thresholds`` also the strict counts ``#{j : l[b,j] > thr[b]}``.
    Same values, bit for bit, as ``topk(score(h, table))`` after the column-0 mask."""
    L.require_gpu(h, table)
    h, t = L.as_f32(h), L.as_f32(table)
    B, d = h.shape
    rows = t.shape[0]
    dev = h.device
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    th = L.as_f32(thresholds.reshape(-1)) if thresholds is not None else None
    cnt = torch.empty(B, dtype=torch.int64, device=dev) if th is not None else None
    nbytes = L.lib().gr_score_topk_workspace_bytes(B, d, rows, k)
    wsp = L.workspace(nbytes, dev)
    with L.on(dev):
        L.check(L.lib().gr_score_topk_f32(L.ptr(h), B, d, L.ptr(t), rows, id_offset,
                                          1 if mask_col0 else 0, k, L.ptr(th), L.ptr(cnt),
                                          L.ptr(vals), L.ptr(ids), L.ptr(wsp), nbytes,
                                          L.stream_of(dev)), "gr_score_topk_f32")
    return (vals, ids) if th is None else (vals, ids, cnt)


def merge_topk(vals, ids, k):
    """Top-k of candidate lists [B, C] (values, global ids) by (value desc, id asc), ids < 0 padding
    (emitted as (-inf, -1)): the merge of the catalog shards' lists (gr_merge_topk_f32)."""
    L.require_gpu(vals, ids)
    B, C = vals.shape
    v = L.as_f32(vals)
    i = ids.to(torch.int64).contiguous()
    out_v = torch.empty((B, k), dtype=torch.float32, device=vals.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=vals.device)
    with L.on(vals.device):
        L.check(L.lib().gr_merge_topk_f32(L.ptr(v), v.stride(0), L.ptr(i), i.stride(0), B, C, k,
                                          L.ptr(out_v), L.ptr(out_i), L.stream_of(vals.device)),
                "gr_merge_topk_f32")
    return out_v, out_i


def merge_topk_packed(packed, world, kk, k):
    """The merge straight from the exchange's all-gathered int64 buffer [world, B, 2 kk] (per rank
    and row kk ids, then kk value bit patterns; dist._exchange)."""
    L.require_gpu(packed)
    packed = packed.contiguous()
    B = packed.numel() // (world * 2 * kk)
    out_v = torch.empty((B, k), dtype=torch.float32, device=packed.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=packed.device)
    with L.on(packed.device):
        L.check(L.lib().gr_merge_topk_packed(L.ptr(packed), world, B, kk, k, L.ptr(out_v), L.ptr(out_i),
                                             L.stream_of(packed.device)), "gr_merge_topk_packed")
    return out_v, out_i


def rq_quantize(z, codebooks, with_gap=False):
    """Residual quantization of latents (RQ-VAE/models/rq.py:39-56, use_sk=False).

    With ``with_gap`` also returns the best distance and the best/second-best gap per level."""
    L.require_gpu(z, *codebooks)
    z = L.as_f32(z)
    n, e = z.shape
    cbs = [L.as_f32(c) for c in codebooks]
    Ks = [c.shape[0] for c in cbs]
    for c in cbs:
        if c.shape[1] != e:
            raise RuntimeError("rq_quantize: codebook width != latent width")
    dev = z.device
    idx = torch.empty((n, len(cbs)), dtype=torch.int64, device=dev)
    gap = torch.empty((n, len(cbs)), dtype=torch.float32, device=dev) if with_gap else None
    best = torch.empty((n, len(cbs)), dtype=torch.float32, device=dev) if with_gap else None
    lib = L.lib()
    st = L.stream_of(dev)
    with L.on(dev):
        # code_norms = NULL: the kernel recomputes the norms from its LDS image of each codebook
        L.check(lib.gr_rq_quantize_f32(L.ptr(z), n, e, len(cbs), L.i32_array(Ks), L.ptr_array(cbs),
                                       None, L.ptr(idx), L.ptr(best), L.ptr(gap), st),
                "gr_rq_quantize_f32")
    return (idx, best, gap) if with_gap else idx


class RqBinding:
    """The encoder weights / biases and codebooks of one RQ-VAE as the ctypes arrays
    ``gr_rq_encode_f32`` takes (device pointers, dims, K per level), built once per parameter set
    (:func:`rq_binding`) so a ``get_indices`` call at the reference's batch 64 (RQ-VAE/infer.py:84-95)
    pays only the launch."""

    def __init__(self, weights, biases, codebooks):
        weights, biases, codebooks = ([t.detach() for t in ts] for ts in (weights, biases, codebooks))
        self.ws = [L.as_f32(w) for w in weights]
        self.bs = [L.as_f32(b) for b in biases]
        self.cbs = [L.as_f32(c) for c in codebooks]
        L.require_gpu(*self.ws, *self.cbs)
        self.direct = all(a.data_ptr() == b.data_ptr() for a, b in
                          zip(self.ws + self.bs + self.cbs, list(weights) + list(biases) + list(codebooks)))
        self.in_dim = self.ws[0].shape[1]
        self.dims = [self.in_dim] + [w.shape[0] for w in self.ws]
        for i, w in enumerate(self.ws):
            if w.shape[1] != self.dims[i]:
                raise RuntimeError(f"rq_encode: Linear {i} expects {w.shape[1]} inputs, got {self.dims[i]}")
        self.Ks = [c.shape[0] for c in self.cbs]
        self.n_linear = len(self.ws)
        self.dims_c, self.ks_c = L.i32_array(self.dims), L.i32_array(self.Ks)
        self.w_arr, self.b_arr, self.c_arr = L.ptr_array(self.ws), L.ptr_array(self.bs), L.ptr_array(self.cbs)
        self.device = self.ws[0].device
        self.dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._ws_bytes = {}
        # the fused encoder's packed weight image (frozen weights only, see packed_ptr)
        nf = L.lib().gr_rq_encoder_pack_floats(len(self.ws), self.dims_c)
        self.packed = torch.empty(nf, dtype=torch.float32, device=self.device) if nf else None
        self._pack_key = None
        # the filtered quantizer's packed codebook image (frozen codebooks only, see cb_image_ptr)
        nc = L.lib().gr_rq_codebook_image_floats(self.dims[-1], len(self.cbs), self.ks_c)
        self.cb_image = torch.empty(nc, dtype=torch.float32, device=self.device) if nc else None
        self._cb_key = None

    # Re-use one packed encoder image across calls, re-packed whenever a weight's version counter
    # (load_state_dict, optimizer steps, any in-place op) or the graph-replay epoch moves (a
    # replayed training graph updates the weights without a version bump: ops.weights_changed).
    # A write that bypasses both (``param.data[...] = ...``) must call weights_changed(), or the
    # owner runs with ``RQVAE.freeze_encoder(False)``: every call then packs the current weights
    # into its workspace (one extra launch, 4 us per C2 call, profiles/r04/ab_rq_pack.txt).
    frozen = True

    def packed_ptr(self):
        """Device pointer of the up-to-date packed encoder image; None: pack per call
        (``frozen = False``, or not the fused encoder shape)."""
        if self.packed is None or not self.frozen:
            return None

        def pack(image):
            L.check(L.lib().gr_rq_encoder_pack_f32(len(self.ws), self.dims_c, self.w_arr, L.ptr(image),
                                                   L.stream_of(self.device)), "gr_rq_encoder_pack_f32")
        return self._image_ptr("packed", "_pack_key", "_streams", self.ws, pack, "packed encoder image")

    def cb_image_ptr(self):
        """Device pointer of the up-to-date packed codebook image (the filtered quantizer's per-level
        LDS images, ``gr_rq_codebook_pack_f32``), cached like the encoder image under the codebooks'
        version counters and the graph-replay epoch; None: the kernel derives the images from the
        codebooks on every call (``frozen = False``, or codebooks the filtered quantizer does not take)."""
        if self.cb_image is None or not self.frozen:
            return None

        def pack(image):
            L.check(L.lib().gr_rq_codebook_pack_f32(self.dims[-1], len(self.cbs), self.ks_c, self.c_arr, L.ptr(image),
                                                    L.stream_of(self.device)), "gr_rq_codebook_pack_f32")
        return self._image_ptr("cb_image", "_cb_key", "_cb_streams", self.cbs, pack, "packed codebook image")

    def _image_ptr(self, attr, key_attr, streams_attr, params, pack, what):
        """The cached image ``attr`` of ``params``, re-packed into a fresh tensor when its key moved."""
        image = getattr(self, attr)
        key = tuple(w._version for w in params) + (_WEIGHT_EPOCH[0],)
        capturing = torch.cuda.is_current_stream_capturing()
        if key != getattr(self, key_attr) and capturing:
            # a pack recorded into a graph would run only at replay, leaving the eager image stale
            raise RuntimeError(f"rq_encode: the {what} is out of date inside a graph capture; "
                               "run one eager get_indices after the last weight change, then capture "
                               "(graphs that encode must be re-captured after weight changes)")
        if capturing:
            # a captured graph bakes in this image's pointer: keep the image alive for the binding's
            # lifetime, so replays after a later re-pack read the old weights, never freed memory
            refs = self.__dict__.setdefault("_graph_images", [])
            if not any(r is image for r in refs):
                refs.append(image)
        if key != getattr(self, key_attr):
            if getattr(self, key_attr) is not None:
                # a re-pack writes a fresh image on this stream; the previous one goes back to the
                # caching allocator, which does not hand it out again before the work of every
                # stream recorded on it (below) has finished
                image = torch.empty_like(image)
                setattr(self, attr, image)
                setattr(self, streams_attr, set())
            with L.on(self.device):
                pack(image)
            setattr(self, key_attr, key)
        st = L.stream_of(self.device)
        streams = getattr(self, streams_attr, None)
        if streams is None:
            streams = set()
            setattr(self, streams_attr, streams)
        if st not in streams:   # an encode on another stream than the allocating one
            image.record_stream(torch.cuda.current_stream(self.device))
            streams.add(st)
        return image.data_ptr()

    def encode_fast(self, x):
        """rq_encode's common call -- fp32 contiguous [n, in_dim] rows on the binding's (current)
        device, eager, semantic IDs only -- with the per-call host work cut to the checks and the
        launch (the reference's get_indices(x[64]) is host-bound).  None: not that case; the
        general path (which also raises the errors) runs instead.  Same C call, same results."""
        if (x.dtype is not torch.float32 or x.dim() != 2 or x.shape[1] != self.in_dim or not x.is_cuda
                or not x.is_contiguous() or x.get_device() != self.dev_index
                or self.dev_index != torch.cuda.current_device() or torch.cuda.is_current_stream_capturing()):
            return None
        pk, ci = self.packed_ptr(), self.cb_image_ptr()
        n = x.shape[0]
        st = L.stream_of(self.device)
        nbytes = self._ws_bytes.get(n) or self.workspace_bytes(n)
        ws = _SCRATCH.get((self.dev_index, st))
        if ws is None or ws.numel() < nbytes:
            ws = scratch(nbytes, self.device)
        idx = torch.empty((n, len(self.cbs)), dtype=torch.int64, device=self.device)
        rc = L.lib().gr_rq_encode_image_f32(x.data_ptr(), n, self.n_linear, self.dims_c, self.w_arr, self.b_arr,
                                            pk, len(self.cbs), self.ks_c, self.c_arr, ci, idx.data_ptr(), None, None,
                                            None, ws.data_ptr(), nbytes, st)
        if rc:
            L.check(rc, "gr_rq_encode_image_f32")
        return idx

    def workspace_bytes(self, n):
        nb = self._ws_bytes.get(n)
        if nb is None:
            nb = L.lib().gr_rq_encode_workspace_bytes(n, len(self.ws), self.dims_c, len(self.cbs), self.ks_c)
            if nb == 0:
                raise RuntimeError("rq_encode: bad encoder description")
            if len(self._ws_bytes) < 64:
                self._ws_bytes[n] = nb
        return nb


# Bumped by every replay of a captured training step (its optimizer updates parameters in place
# without touching their version counters), so cached weight images re-pack after it.
_WEIGHT_EPOCH = [0]


def weights_changed():
    """Tell the cached kernel bindings that parameters changed behind torch's version counters."""
    _WEIGHT_EPOCH[0] += 1


def mkl_plan(m, k, n):
    """MKL's accumulation order for one reference CPU sgemm call of ``m`` rows, inner size ``k``,
    ``n`` outputs (``gr_mkl_plan``): (kind, block width, pinned), kind in chain / gemv16 / small16."""
    kind, kb = ctypes.c_int32(0), ctypes.c_int32(0)
    pinned = L.lib().gr_mkl_plan(int(m), int(k), int(n), ctypes.byref(kind), ctypes.byref(kb))
    return ("chain", "gemv16", "small16")[kind.value], kb.value, bool(pinned)


def rq_binding(owner, weights_fn):
    """Cached :class:`RqBinding` on ``owner`` (an RQVAE): rebuilt when any parameter's storage moved
    (``.to()``, ``param.data = ...``); in-place updates (``load_state_dict``, optimiser steps) are
    seen through the same pointers.  ``weights_fn() -> (weights, biases, codebooks)``, the LIVE
    parameters (not detached copies: their pointers are the cache key)."""
    c = owner.__dict__.get("_gr_rq_binding")
    if c is not None:
        tensors, key, b = c
        if b.direct and tuple(t.data_ptr() for t in tensors) == key:
            return b
    ws, bs, cbs = weights_fn()
    tensors = list(ws) + list(bs) + list(cbs)
    b = RqBinding(ws, bs, cbs)
    owner.__dict__["_gr_rq_binding"] = (tensors, tuple(t.data_ptr() for t in tensors), b)
    return b


def rq_encode(x, weights=None, biases=None, codebooks=None, with_gap=False, with_z=False, binding=None):
    """RQVAE.get_indices(xs, use_sk=False): encoder MLP + residual quantization (rqvae.py:67-71).

    Returns ``idx`` [n, L] int64, plus ``best`` and ``gap`` [n, L] (best distance and second-best
    minus best) and the encoder output ``z`` when requested.  ``binding`` (an :class:`RqBinding`)
    replaces ``weights`` / ``biases`` / ``codebooks``.
    """
    if binding is not None and not with_gap and not with_z:
        idx = binding.encode_fast(x)
        if idx is not None:
            return idx
    b = binding if binding is not None else RqBinding(weights, biases, codebooks)
    L.require_gpu(x)
    x2 = L.as_f32(x)
    if x2.dim() != 2 or x2.shape[1] != b.in_dim:
        raise RuntimeError(f"rq_encode: expected [n, {b.in_dim}] inputs, got {tuple(x2.shape)}")
    dev = x2.device
    if dev != b.device:
        raise RuntimeError(f"rq_encode: inputs on {dev}, parameters on {b.device}")
    n = x2.shape[0]
    nbytes = b.workspace_bytes(n)
    wsp = scratch(nbytes, dev)
    nl = len(b.cbs)
    idx = torch.empty((n, nl), dtype=torch.int64, device=dev)
    gap = torch.empty((n, nl), dtype=torch.float32, device=dev) if with_gap else None
    best = torch.empty((n, nl), dtype=torch.float32, device=dev) if with_gap else None
    z = torch.empty((n, b.dims[-1]), dtype=torch.float32, device=dev) if with_z else None
    with L.on(dev):
        L.check(L.lib().gr_rq_encode_image_f32(x2.data_ptr(), n, b.n_linear, b.dims_c, b.w_arr, b.b_arr,
                                               b.packed_ptr(), nl, b.ks_c, b.c_arr, b.cb_image_ptr(), idx.data_ptr(),
                                               L.ptr(best), L.ptr(gap), L.ptr(z), wsp.data_ptr(), nbytes,
                                               L.stream_of(dev)),
                "gr_rq_encode_image_f32")
    out = [idx]
    if with_gap:
        out += [best, gap]
    if with_z:
        out.append(z)
    return out[0] if len(out) == 1 else tuple(out)


_EXACT_ACTS = {"relu": 1, "none": 0, None: 0, "leakyrelu": 4}


def rq_mlp(x, weights, biases, bn=None, act="relu", group_sizes=None):
    """MLPLayers.forward (RQ-VAE/models/layers.py:18-43, eval): the encoder output ``z`` alone, in
    the reference's CPU order bit for bit (``gr_mlp_exact_f32``: the fused kernel for in -> 256 ->
    128 -> 32 ReLU MLPs, exact layer-wise launches otherwise, the per-row kernel for 1-15-row
    calls).  ``bn``: None, or (means, vars, weights, biases, eps) of the eval BatchNorm1d after every
    Linear but the last (weights / biases entries may be None: affine off); ``act``: relu /
    leakyrelu / none.  ``group_sizes``: consecutive row groups, each ONE reference call (MKL's order
    depends on the call's row count; ``gr_mlp_exact_groups_f32``)."""
    L.require_gpu(x, *weights)
    x2 = L.as_f32(x)
    n = x2.shape[0]
    ws = [L.as_f32(w) for w in weights]
    bs = [L.as_f32(b) for b in biases] if biases is not None else None
    dims = [x2.shape[1]] + [w.shape[0] for w in ws]
    for i, w in enumerate(ws):
        if w.shape[1] != dims[i]:
            raise RuntimeError(f"rq_mlp: Linear {i} expects {w.shape[1]} inputs, got {dims[i]}")
    if act not in _EXACT_ACTS:
        raise RuntimeError(f"rq_mlp: activation {act} has no exact kernel (relu / leakyrelu / none)")
    dev = x.device
    lib = L.lib()
    dims_c = L.i32_array(dims)
    nbytes = lib.gr_rq_mlp_workspace_bytes(n, len(ws), dims_c)
    wsp = L.workspace(nbytes, dev)
    z = torch.empty((n, dims[-1]), dtype=torch.float32, device=dev)
    bn_arrs = [None] * 4
    eps = 0.0
    keep = []
    if bn is not None:
        means, vars_, bws, bbs, eps = bn
        for j, group in enumerate((means, vars_, bws, bbs)):
            if group is None or all(t is None for t in group):
                continue
            ts = [L.as_f32(t) for t in group]
            keep.append(ts)
            bn_arrs[j] = L.ptr_array(ts)
    with L.on(dev):
        if group_sizes is not None:
            sizes = [int(g) for g in group_sizes]
            if sum(sizes) != n or any(g < 1 for g in sizes):
                raise RuntimeError("rq_mlp: group sizes must be positive and sum to the batch")
            # Groups MKL runs as k-block chains (>= 16 rows) whose per-layer blocks match those of ONE
            # call over all of them produce the same bits in that call: they go through the MFMA
            # kernels together; the rest (1-15-row orders) through the per-row kernel, group by group.
            plans = {}

            def plan(m):
                if m not in plans:
                    plans[m] = tuple(mkl_plan(m, dims[i], dims[i + 1])[:2] for i in range(len(ws)))
                return plans[m]

            big = [i for i, g in enumerate(sizes) if all(k == "chain" for k, _ in plan(g))]
            while big:   # the kept groups' one call must have every kept group's own order
                pb = plan(sum(sizes[i] for i in big))
                kept = [i for i in big if plan(sizes[i]) == pb]   # (``keep`` holds the BN tensors alive)
                if kept == big:
                    break
                big = kept
            small = [i for i in range(len(sizes)) if i not in set(big)]
            offs = [0]
            for g in sizes:
                offs.append(offs[-1] + g)

            def rows_of(sel):
                return torch.cat([torch.arange(offs[i], offs[i + 1], device=dev) for i in sel])

            if small:
                rs = rows_of(small) if big else None
                xs = x2 if rs is None else x2.index_select(0, rs).contiguous()
                zs = z if rs is None else torch.empty((xs.shape[0], dims[-1]), dtype=torch.float32, device=dev)
                ptr = _group_ptr([sizes[i] for i in small], dev)
                L.check(lib.gr_mlp_exact_groups_f32(L.ptr(xs), xs.shape[0], len(ws), dims_c, L.ptr_array(ws),
                                                    L.ptr_array(bs) if bs is not None else None, *bn_arrs,
                                                    float(eps), _EXACT_ACTS[act], L.ptr(ptr), len(small),
                                                    L.ptr(zs), L.stream_of(dev)), "gr_mlp_exact_groups_f32")
                if rs is not None:
                    z.index_copy_(0, rs, zs)
            if big:
                rb = rows_of(big) if small else None
                xb = x2 if rb is None else x2.index_select(0, rb).contiguous()
                nb2 = xb.shape[0]
                zb = z if rb is None else torch.empty((nb2, dims[-1]), dtype=torch.float32, device=dev)
                nbytes2 = lib.gr_rq_mlp_workspace_bytes(nb2, len(ws), dims_c)
                wsp2 = L.workspace(nbytes2, dev)
                L.check(lib.gr_mlp_exact_f32(L.ptr(xb), nb2, len(ws), dims_c, L.ptr_array(ws),
                                             L.ptr_array(bs) if bs is not None else None, *bn_arrs, float(eps),
                                             _EXACT_ACTS[act], L.ptr(zb), L.ptr(wsp2), nbytes2, L.stream_of(dev)),
                        "gr_mlp_exact_f32")
                if rb is not None:
                    z.index_copy_(0, rb, zb)
            return z
        L.check(lib.gr_mlp_exact_f32(L.ptr(x2), n, len(ws), dims_c, L.ptr_array(ws),
                                     L.ptr_array(bs) if bs is not None else None, *bn_arrs, float(eps),
                                     _EXACT_ACTS[act], L.ptr(z), L.ptr(wsp), nbytes, L.stream_of(dev)),
                "gr_mlp_exact_f32")
    return z


def rq_encode_sk(x, weights, biases, codebooks, sk_eps, sk_iters, group_sizes=None):
    """RQVAE.get_indices(xs, use_sk=True) (RQ-VAE/models/rqvae.py:67-71 with vq.py:76-84) for
    independent row groups in ONE launch: ``group_sizes`` partitions the rows of ``x`` into
    consecutive groups, each one reference call (default: the whole batch is one group)."""
    L.require_gpu(x, *weights, *codebooks)
    return rq_quantize_sk(rq_mlp(x, weights, biases, group_sizes=group_sizes), codebooks, sk_eps, sk_iters,
                          group_sizes)


def rq_encode_z(z, codebooks, with_gap=False):
    """``get_indices`` from encoder outputs computed elsewhere (e.g. a BatchNorm encoder)."""
    return rq_quantize(z, codebooks, with_gap=with_gap)


_GROUP_PTRS = {}


def _group_ptr(sizes, dev):
    """Device copy of the group offsets [0, s0, s0+s1, ...].  The one-group form (a training batch)
    is cached per (n, device) and never freed, so a captured training step (RqTrainGraph) replays
    the Sinkhorn launch with no host-to-device copy and a pointer that stays valid."""
    if len(sizes) != 1:
        return torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int64).to(dev)
    key = (sizes[0], str(dev))
    t = _GROUP_PTRS.get(key)
    if t is None:
        t = torch.tensor([0, sizes[0]], dtype=torch.int64).to(dev)
        _GROUP_PTRS[key] = t
    return t


def rq_quantize_sk(z, codebooks, sk_eps, sk_iters, group_sizes=None):
    """ResidualVectorQuantizer.forward(z, use_sk=True) indices (rq.py:39-56, vq.py:63-84): per level,
    Sinkhorn over the group's distances where ``sk_eps[l] > 0``, plain argmin otherwise."""
    L.require_gpu(z, *codebooks)
    z = L.as_f32(z)
    n = z.shape[0]
    cbs = [L.as_f32(c) for c in codebooks]
    e = z.shape[1]
    Ks = [c.shape[0] for c in cbs]
    sizes = [n] if group_sizes is None else [int(s) for s in group_sizes]
    if sum(sizes) != n or any(s < 1 for s in sizes):
        raise RuntimeError("rq_encode_sk: group sizes must be positive and sum to the batch")
    dev = z.device
    ptr = _group_ptr(sizes, dev)
    lib = L.lib()
    ks_c = L.i32_array(Ks)
    eps_c = (ctypes.c_double * len(cbs))(*[float(v) for v in sk_eps])
    nbytes = lib.gr_rq_encode_sk_workspace_bytes(n, e, len(cbs), ks_c)
    wsp = L.workspace(nbytes, dev)
    idx = torch.empty((n, len(cbs)), dtype=torch.int64, device=dev)
    with L.on(dev):
        L.check(lib.gr_rq_encode_sk_f32(L.ptr(z), n, e, len(cbs), ks_c, L.ptr_array(cbs), eps_c,
                                        int(sk_iters), L.ptr(ptr), len(sizes), L.ptr(idx), L.ptr(wsp),
                                        nbytes, L.stream_of(dev)), "gr_rq_encode_sk_f32")
    return idx


class CodeGroups:
    """Result of ``code_groups``: everything is on the device and nothing has been synchronised.

    ``leader`` / ``count`` / ``digit`` [n] int64 per row; ``stats`` [4] int64 = (distinct codes,
    largest count, M = rows of shared codes, G = shared codes).  ``rows`` [M] and ``sizes`` [G] are
    slices of buffers padded to n and n // 2 entries: taking them needs M and G on the host, so the
    first access reads ``stats`` back (``host()``: the one device-to-host read, cached)."""
    SIZES_HEAD = 8192   # group sizes that ride along with the stats in host()'s one read

    def __init__(self, n, leader, count, digit, rows_buf, meta):
        self.n, self.leader, self.count, self.digit = n, leader, count, digit
        self._rows, self._meta, self._host = rows_buf, meta, None

    @property
    def stats(self):
        return self._meta[:4]

    def host(self):
        """``((distinct, max_count, M, G), sizes)`` on the host (ints; sizes a numpy int64 array, None
        without a listing): one read of the stats with the first ``SIZES_HEAD`` sizes behind them,
        and a second read only when there are more groups than that."""
        if self._host is None:
            listing = self._rows is not None
            head = self._meta[:4 + self.SIZES_HEAD if listing else 4].cpu()
            st = tuple(int(v) for v in head[:4])
            sizes = None
            if listing:
                g = st[3]
                sizes = (head[4:4 + g] if g <= self.SIZES_HEAD else self._meta[4:4 + g].cpu()).numpy()
            self._host = (st, sizes)
        return self._host

    @property
    def rows(self):
        if self._rows is None:
            raise RuntimeError("code_groups(listing=False) has no group listing")
        return self._rows[:self.host()[0][2]]

    @property
    def sizes(self):
        if self._rows is None:
            raise RuntimeError("code_groups(listing=False) has no group listing")
        return self._meta[4:4 + self.host()[0][3]]


def code_groups(codes, listing=True):
    """Collision groups and dedup digit of ``codes`` [n, L] (RQ-VAE/infer.py:29-41 and :139-162) as a
    ``CodeGroups``.  The hash build, the lookup and the segment pass over the sorted keys are HIP
    (codes.hip); the sort of the packed ``leader << 32 | row`` keys between them is ``torch.sort``
    on the device (the keys past M hold INT64_MAX, so no size has to reach the host).  Performs no
    synchronisation.  ``listing=False``: leader / count / stats only (digit stays zero)."""
    L.require_gpu(codes)
    if codes.dim() != 2 or codes.dtype != torch.int64:
        raise TypeError(f"code_groups takes an int64 [n, L] tensor, got {codes.dtype} {tuple(codes.shape)}")
    codes = codes.contiguous()
    n, levels = codes.shape
    dev = codes.device
    lib = L.lib()
    leader, count, digit = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    meta = (torch.empty if n else torch.zeros)(4 + max(n // 2, 1), dtype=torch.int64, device=dev)
    rows_buf = torch.empty(n, dtype=torch.int64, device=dev) if listing else None
    if n == 0:
        if levels < 1:
            raise RuntimeError("code_groups: codes need at least one level")
        return CodeGroups(n, leader, count, digit, rows_buf, meta)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    nbytes = lib.gr_code_groups_workspace_bytes(n, levels)
    wsp = L.workspace(nbytes, dev)
    with L.on(dev):
        L.check(lib.gr_code_groups_i64(L.ptr(codes), n, levels, L.ptr(leader), L.ptr(count), L.ptr(digit),
                                       L.ptr(keys), L.ptr(meta), L.ptr(wsp), nbytes, L.stream_of(dev)),
                "gr_code_groups_i64")
        if listing:
            keys = torch.sort(keys).values
            L.check(lib.gr_code_segments_i64(L.ptr(keys), n, L.ptr(meta), L.ptr(count), L.ptr(rows_buf),
                                             L.ptr(meta[4:]), L.ptr(digit), L.ptr(wsp), nbytes,
                                             L.stream_of(dev)), "gr_code_segments_i64")
    return CodeGroups(n, leader, count, digit, rows_buf, meta)


KMeansResult = collections.namedtuple("KMeansResult", "centers labels inertia n_iter")
KMEANS_ENVELOPE = "1 <= e <= 64 features, 1 <= n_clusters <= 1024, n_clusters <= n < 2**31 rows"


def kmeans(x, n_clusters, max_iter=10, tol=1e-4, seed=None, init=None, trials=None, with_labels=True):
    """scikit-learn's ``KMeans(n_clusters, max_iter=max_iter, tol=tol).fit(x)`` as the reference calls
    it (RQ-VAE/models/layers.py:69-82: greedy k-means++ seeding, one initialisation, Lloyd with
    empty-cluster relocation and both stop rules) in one C-ABI call, ``gr_kmeans_f32``: a
    ``KMeansResult`` of ``centers`` [K, e] fp32, ``labels`` [n] int64 and ``inertia`` (fp64 scalar)
    against those centres, and ``n_iter`` (int32 scalar), all on the device; nothing synchronises.

    ``seed``: the k-means++ draws are a function of it and of ``x`` only, and the sums are taken in a
    fixed order, so the same seed gives the same bits.  ``None`` draws one from torch's default
    generator (``torch.manual_seed`` makes the run repeatable).  ``init`` [K, e] skips the seeding;
    with ``max_iter=0`` the call returns the labels and inertia of ``init``.  ``trials``: candidates
    per seeding round (default scikit-learn's ``2 + floor(ln K)``; 1 is plain D^2 sampling).
    ``with_labels=False`` leaves ``labels`` None (no [n] int64 buffer; the codebook init needs none)."""
    L.require_gpu(x)
    if x.dim() != 2:
        raise RuntimeError(f"kmeans takes [n, e] rows, got {tuple(x.shape)}")
    x = L.as_f32(x.detach())
    n, e = x.shape
    K = int(n_clusters)
    if n < K:
        raise ValueError(f"n_samples={n} should be >= n_clusters={K}.")
    lib = L.lib()
    nbytes = lib.gr_kmeans_workspace_bytes(n, e, K)
    if nbytes == 0:
        raise RuntimeError(f"kmeans: x {tuple(x.shape)} with n_clusters={K} is outside the kernels' envelope "
                           f"({KMEANS_ENVELOPE}); there is no CPU fallback")
    dev = x.device
    if init is not None:
        L.require_gpu(init)
        init = L.as_f32(init.detach())
        if tuple(init.shape) != (K, e):
            raise RuntimeError(f"kmeans: init must be [{K}, {e}], got {tuple(init.shape)}")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    centers = torch.empty((K, e), dtype=torch.float32, device=dev)
    labels = torch.empty(n, dtype=torch.int64, device=dev) if with_labels else None
    inertia = torch.empty((), dtype=torch.float64, device=dev)
    n_iter = torch.empty((), dtype=torch.int32, device=dev)
    wsp = L.workspace(nbytes, dev)
    with L.on(dev):
        L.check(lib.gr_kmeans_f32(L.ptr(x), n, e, K, L.ptr(init), int(seed) & (2 ** 64 - 1),
                                  0 if trials is None else int(trials), int(max_iter), float(tol), L.ptr(centers),
                                  L.ptr(labels), L.ptr(inertia), L.ptr(n_iter), L.ptr(wsp), nbytes,
                                  L.stream_of(dev)), "gr_kmeans_f32")
    return KMeansResult(centers, labels, inertia, n_iter)


class SasrecBinding:
    """Device-pointer view of a SASRec module's parameters (``gr_sasrec_params``).

    Built once per parameter set and cached on the module (:func:`sasrec_binding`); the pointers
    are the parameters' own storage, so in-place weight updates and ``load_state_dict`` are seen.
    """

    def __init__(self, model):
        self.keep = []
        self.direct = True           # every pointer is the parameter's own storage (no copies)
        f = self._f
        nb = model.num_blocks
        p = L.SasrecParams()
        p.d, p.n_blocks, p.n_heads, p.mlp = model.d, nb, model.num_heads, model.mlp_layer
        p.max_len = model.pos_emb.weight.shape[0]
        p.eps = float(model.layernorm_eps)
        p.item_rows = model.item_emb.weight.shape[0]
        p.item_emb = f(model.item_emb.weight)
        p.pos_emb = f(model.pos_emb.weight)
        arr = self._arr
        p.attn_ln_w = arr([m.weight for m in model.attention_layernorms])
        p.attn_ln_b = arr([m.bias for m in model.attention_layernorms])
        p.in_proj_w = arr([m.in_proj_weight for m in model.attention_layers])
        p.in_proj_b = arr([m.in_proj_bias for m in model.attention_layers])
        p.out_proj_w = arr([m.out_proj.weight for m in model.attention_layers])
        p.out_proj_b = arr([m.out_proj.bias for m in model.attention_layers])
        p.ffn_ln_w = arr([m.weight for m in model.forward_layernorms])
        p.ffn_ln_b = arr([m.bias for m in model.forward_layernorms])
        p.ffn1_w = arr([m[0].weight for m in model.forward_layers])
        p.ffn1_b = arr([m[0].bias for m in model.forward_layers])
        p.ffn2_w = arr([m[3].weight for m in model.forward_layers])
        p.ffn2_b = arr([m[3].bias for m in model.forward_layers])
        p.last_ln_w = f(model.last_layernorm.weight)
        p.last_ln_b = f(model.last_layernorm.bias)
        self.p = p
        self.p_ref = ctypes.byref(p)
        self.device = model.item_emb.weight.device
        self._ws = {}
        self._ws_epoch = L.OPTION_EPOCH

    def _f(self, t):
        L.require_gpu(t)
        t2 = L.as_f32(t.detach())
        self.direct &= t2.data_ptr() == t.data_ptr()
        self.keep.append(t2)
        return t2.data_ptr()

    def _arr(self, ts):
        a = (ctypes.c_void_p * max(1, len(ts)))(*[self._f(t) for t in ts])
        self.keep.append(a)
        return ctypes.cast(a, ctypes.c_void_p)

    def _sizes(self):
        """The per-shape size cache, emptied when a path switch has moved since it was filled (the
        fused and the layer-wise forward of one shape need different workspaces)."""
        if self._ws_epoch != L.OPTION_EPOCH:
            self._ws.clear()
            self._ws_epoch = L.OPTION_EPOCH
        return self._ws

    def workspace_bytes(self, B, n):
        key = (0, B, n)
        nb = self._sizes().get(key)
        if nb is None:
            nb = L.lib().gr_sasrec_workspace_bytes(self.p_ref, B, n)
            if len(self._ws) < 256:
                self._ws[key] = nb
        return nb

    def rank_workspace_bytes(self, B, n):
        key = (1, B, n)
        nb = self._sizes().get(key)
        if nb is None:
            nb = (L.lib().gr_sasrec_rank_workspace_bytes(self.p_ref, B, n),
                  L.lib().gr_score_count_workspace_bytes(B))
            if len(self._ws) < 256:
                self._ws[key] = nb
        return nb

    def plan(self, B, n, last_only):
        """``gr_sasrec_plan``: the GR_SAS_* mask of the kernels a forward of this shape runs now."""
        return L.lib().gr_sasrec_plan(self.p_ref, B, n, 1 if last_only else 0)


def sasrec_binding(model):
    """Cached :class:`SasrecBinding` of ``model``: reused while every parameter's storage pointer
    is unchanged (checked per call, ~5 us for SASRec's 34 tensors); rebuilt after ``.to()`` or a
    ``param.data = ...`` swap, and on every call when a parameter is not contiguous fp32 (then the
    binding holds copies).  This is what makes a ``predict`` at the reference's eval batch of 128
    (SASRec/evaluate.py:13, 26) cost one launch on the host."""
    c = model.__dict__.get("_gr_sas_binding")
    if c is not None:
        params, key, b = c
        if b.direct and tuple(q.data_ptr() for q in params) == key:
            return b
    params = list(model.parameters())
    b = SasrecBinding(model)
    model.__dict__["_gr_sas_binding"] = (params, tuple(q.data_ptr() for q in params), b)
    return b


def _sas_ids(log_seqs, binding):
    L.require_gpu(log_seqs)
    if log_seqs.dim() != 2:
        raise RuntimeError("SASRec expects log_seqs of shape [B, n]")
    if log_seqs.device != binding.device:
        raise RuntimeError(f"log_seqs on {log_seqs.device}, model on {binding.device}")
    return log_seqs.to(torch.int64).contiguous()


def _check_err(err):
    if CHECK:
        check_errors(err.device)


def sasrec_forward(binding, log_seqs, last_only=False):
    ids = _sas_ids(log_seqs, binding)
    B, n = ids.shape
    dev = ids.device
    d = binding.p.d
    out = torch.empty((B, d) if last_only else (B, n, d), dtype=torch.float32, device=dev)
    nbytes = binding.workspace_bytes(B, n)
    wsp = scratch(nbytes, dev)
    err = err_flag(dev)
    with L.on(dev):
        L.check(L.lib().gr_sasrec_forward_f32(binding.p_ref, L.ptr(ids), B, n, L.ptr(out),
                                              1 if last_only else 0, L.ptr(wsp), nbytes, L.ptr(err),
                                              L.stream_of(dev)), "gr_sasrec_forward_f32")
    _check_err(err)
    return out


def sasrec_rank(binding, log_seqs, targets, mask_col0=True):
    """One batch of SASRec/evaluate.py:26-32 in ONE C-ABI call (``gr_sasrec_rank_f32``): the 1-based
    strict rank of each target over the full catalog, column 0 taken as -1e9 when ``mask_col0``,
    from the forward's last hidden states -- the logits are never written.  Bitwise the ranks of
    ``ops.rank(predict(seqs), targets)`` (the same fp32 scoring chain)."""
    ids = _sas_ids(log_seqs, binding)
    B, n = ids.shape
    t = targets.reshape(-1)
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    if not t.is_contiguous():
        t = t.contiguous()
    if t.shape[0] != B:
        raise RuntimeError(f"sasrec_rank: {t.shape[0]} targets for {B} sequences")
    dev = ids.device
    nbytes, cnb = binding.rank_workspace_bytes(B, n)
    wsp = scratch(nbytes, dev)
    out = torch.empty(B, dtype=torch.int64, device=dev)
    err = err_flag(dev)
    cws, key = _count_workspace(dev, cnb)
    with L.on(dev):
        try:
            L.check(L.lib().gr_sasrec_rank_f32(binding.p_ref, ids.data_ptr(), B, n, t.data_ptr(),
                                               1 if mask_col0 else 0, out.data_ptr(), wsp.data_ptr(), nbytes,
                                               L.ptr(cws), cnb, err.data_ptr(),
                                               L.stream_of(dev)), "gr_sasrec_rank_f32")
        except Exception:
            if key is not None:
                _COUNT_WS.pop(key, None)
            raise
    _check_err(err)
    return out


LOGITS_ROW_ALIGN = 32  # floats: one 128-byte line


def logits_buffer(B, rows, device):
    """A fresh ``[B, rows]`` fp32 logits tensor whose rows are ``rows`` rounded up to 32 floats apart
    (a view of a ``[B, ld]`` allocation), so every row starts on a 128-byte line and the scoring
    kernel stores whole lines straight from its accumulators.  The reference's callers
    (evaluate.py:27-32, train.py:45-48: in-place ``[:, 0]`` mask, ``gather``, ``>`` + ``sum``) work on
    it unchanged; ``.contiguous()`` gives a packed copy."""
    ld = -(-rows // LOGITS_ROW_ALIGN) * LOGITS_ROW_ALIGN
    return torch.empty((B, ld), dtype=torch.float32, device=device)[:, :rows]


def sasrec_predict(binding, log_seqs, out=None):
    """model.py:98-108 through ``gr_sasrec_predict_ld_f32``.  ``out`` (optional) may be any
    ``[B, item_rows]`` fp32 tensor with unit column stride; by default a row-padded
    :func:`logits_buffer` is returned."""
    ids = _sas_ids(log_seqs, binding)
    B, n = ids.shape
    dev = ids.device
    rows = binding.p.item_rows
    logits = out if out is not None else logits_buffer(B, rows, dev)
    if (logits.shape != (B, rows) or logits.dtype != torch.float32 or logits.device != dev
            or (B > 1 and logits.stride(1) != 1) or logits.stride(0) < rows):
        raise ValueError("sasrec_predict: out must be fp32 [B, item_rows] on the ids' device with unit column stride")
    ld = logits.stride(0) if B > 1 else rows
    nbytes = binding.workspace_bytes(B, n)
    wsp = scratch(nbytes, dev)
    err = err_flag(dev)
    with L.on(dev):
        L.check(L.lib().gr_sasrec_predict_ld_f32(binding.p_ref, L.ptr(ids), B, n,
                                                 L.ptr(logits), ld, L.ptr(wsp), nbytes, L.ptr(err),
                                                 L.stream_of(dev)), "gr_sasrec_predict_ld_f32")
    _check_err(err)
    return logits


# --------------------------------------------------------------------------------------------
# Training-side scoring (SASRec/train.py:131-160)

class _SampledBCE(torch.autograd.Function):
    """``(batch_loss, batch_valid_t)`` of train.py:134-158 with the score matrix never formed;
    differentiable in ``feats`` and ``table`` (gr_sampled_bce_fwd_f32 / gr_sampled_bce_bwd_f32)."""

    @staticmethod
    def forward(ctx, feats, table, targets, negs, eps):
        B, n, d = feats.shape
        rows = table.shape[0]
        J = negs.shape[1]
        dev = feats.device
        row_loss = torch.empty(B * n, dtype=torch.float32, device=dev)
        coef = torch.empty(B * n * (J + 1), dtype=torch.float32, device=dev)
        sums = torch.empty(2, dtype=torch.float32, device=dev)
        err = err_flag(dev)
        with L.on(dev):
            L.check(L.lib().gr_sampled_bce_fwd_f32(L.ptr(feats), B, n, d, L.ptr(table), rows,
                                                   L.ptr(targets), L.ptr(negs), J, float(eps),
                                                   L.ptr(row_loss), L.ptr(coef), L.ptr(sums),
                                                   L.ptr(err), L.stream_of(dev)),
                    "gr_sampled_bce_fwd_f32")
        _check_err(err)
        ctx.save_for_backward(feats, table, targets, negs, coef)
        valid = sums[1]
        ctx.mark_non_differentiable(valid)
        return sums[0], valid

    @staticmethod
    def backward(ctx, g_loss, g_valid):
        feats, table, targets, negs, coef = ctx.saved_tensors
        B, n, d = feats.shape
        rows = table.shape[0]
        dev = feats.device
        g = g_loss.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        dfeats = torch.empty_like(feats)
        dtable = torch.empty_like(table)
        with L.on(dev):
            L.check(L.lib().gr_sampled_bce_bwd_f32(L.ptr(feats), B, n, d, L.ptr(table), rows,
                                                   L.ptr(targets), L.ptr(negs), negs.shape[1],
                                                   L.ptr(coef), L.ptr(g), L.ptr(dfeats),
                                                   L.ptr(dtable), L.stream_of(dev)),
                    "gr_sampled_bce_bwd_f32")
        return dfeats, dtable, None, None, None


def sampled_bce_loss(seq_features, item_emb_weight, target_o_t, neg_samples, eps):
    """train.py:134-158 in one fused op: returns ``(batch_loss, batch_valid_t)`` as device scalars,
    equal to the reference's ``(pos_loss + neg_loss).sum()`` and ``mask.sum()`` over the
    ``[B, n, item_num+1]`` score matrix it forms (this op never forms it).  ``batch_loss`` is
    differentiable in ``seq_features`` [B, n, d] and ``item_emb_weight`` [item_num+1, d]; the caller
    divides by ``batch_valid_t`` (train.py:161-164) and calls ``backward()`` as before."""
    L.require_gpu(seq_features, item_emb_weight, target_o_t, neg_samples)
    if seq_features.dim() != 3 or item_emb_weight.dim() != 2 or seq_features.shape[2] != item_emb_weight.shape[1]:
        raise RuntimeError("sampled_bce_loss: seq_features [B, n, d] and item_emb_weight [rows, d] expected")
    B, n, _ = seq_features.shape
    if tuple(target_o_t.shape) != (B, n) or neg_samples.dim() != 2 or neg_samples.shape[0] != B:
        raise RuntimeError("sampled_bce_loss: target_o_t [B, n] and neg_samples [B, num_neg] expected")
    return _SampledBCE.apply(L.as_f32(seq_features), L.as_f32(item_emb_weight),
                             target_o_t.to(torch.int64).contiguous(),
                             neg_samples.to(torch.int64).contiguous(), eps)


_NEG_CALLS = itertools.count()


def neg_samples(seq, item_num, num_neg=1, seed=None, seed_tensor=None):
    """train.py:15-30 ``get_neg_samples(seq, item_num, num_neg)`` on the GPU: ``[B, num_neg]`` int64,
    per row distinct items uniform over ``[1, item_num]`` minus the row's non-zero history (the
    reference's distribution; not numpy's random stream).  ``seed`` defaults to a fresh value per
    call drawn from torch's global generator, so ``torch.manual_seed`` makes runs repeatable.

    A row whose population (``item_num`` minus its distinct history) is smaller than ``num_neg``
    raises ValueError, as numpy's ``choice(replace=False)`` does.  That can only happen when
    ``n + num_neg > item_num`` (the history holds at most ``n`` distinct items), and only then does
    this call synchronise to check; otherwise every candidate is accepted with probability
    >= 1/2 and the kernel's 4096 rounds of 64 draws cannot fall short.  Unfilled rows hold -1.

    ``seed_tensor`` (a CUDA int64 tensor of one element): the stream is keyed by ``seed ^
    seed_tensor`` read on the device, and ``seed_tensor`` is advanced by one on the stream after
    the draw -- the form a captured graph replays with fresh negatives (``SasTrainStepGraph``)."""
    L.require_gpu(seq)
    s = seq.to(torch.int64).contiguous()
    if s.dim() != 2:
        raise RuntimeError("neg_samples: seq must be [B, n]")
    B, n = s.shape
    if seed is None:
        seed = 0 if seed_tensor is not None else int(torch.randint(0, 2 ** 62, (1,)).item()) ^ next(_NEG_CALLS)
    out = torch.empty((B, num_neg), dtype=torch.int64, device=s.device)
    err = err_flag(s.device)
    with L.on(s.device):
        if seed_tensor is not None:
            if seed_tensor.dtype != torch.int64 or seed_tensor.numel() != 1 or seed_tensor.device != s.device:
                raise RuntimeError("neg_samples: seed_tensor must be one int64 element on the sequences' device")
            L.check(L.lib().gr_neg_samples_dseed(L.ptr(s), B, n, int(item_num), int(num_neg),
                                                 int(seed) & (2 ** 64 - 1), L.ptr(seed_tensor), L.ptr(out),
                                                 L.ptr(err), L.stream_of(s.device)), "gr_neg_samples_dseed")
            seed_tensor.add_(1)
        else:
            L.check(L.lib().gr_neg_samples(L.ptr(s), B, n, int(item_num), int(num_neg), int(seed) & (2 ** 64 - 1),
                                           L.ptr(out), L.ptr(err), L.stream_of(s.device)), "gr_neg_samples")
    # a short population is possible only when 2 (n + num_neg) > item_num; never synchronise inside a
    # graph capture (the captured step classes check once per replay instead)
    if (CHECK or 2 * (n + num_neg) > item_num) and not torch.cuda.is_current_stream_capturing():
        check_errors(s.device)
    return out


# --------------------------------------------------------------------------------------------
# Transformer training forward / backward (SASRec/model.py:49-96 under train.py:131 and :161-172)

_DROP_SEED = {}


def dropout_seed(device):
    """The device's dropout seed word: every train-mode forward snapshots it and advances it by one
    on the stream (a captured step therefore replays with fresh masks).  Initialised from torch's
    global generator, so ``torch.manual_seed`` makes runs repeatable."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    t = _DROP_SEED.get(idx)
    if t is None:
        t = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).to(torch.device("cuda", idx))
        _DROP_SEED[idx] = t
    return t


def _sas_train_fits(model, n, n_max, d_max, mlp_max):
    return (1 <= n <= n_max and n <= model.pos_emb.weight.shape[0] and 1 <= model.d <= d_max
            and model.d % model.num_heads == 0 and 1 <= model.mlp_layer <= mlp_max
            and 1 <= model.num_blocks <= 8)


def sasrec_train_fits_sequence(model, n):
    """One workgroup per sequence (sasrec_train.hip): n, d <= 64, mlp_layer <= 128."""
    return _sas_train_fits(model, n, 64, 64, 128)


def sasrec_train_fits_tiled(model, n):
    """The tiled kernels (sasrec_train_tiled.hip): n <= 256, d <= 128, mlp_layer <= 256."""
    return _sas_train_fits(model, n, 256, 128, 256)


def sasrec_train_supported(model, n):
    """Whether the train-mode forward / backward of this shape runs on the training kernels (either
    set); honours ``model.train_kernels`` ("sequence" / "tiled" restrict it to that set)."""
    mode = getattr(model, "train_kernels", "auto")
    seq = mode in ("auto", "sequence") and sasrec_train_fits_sequence(model, n)
    return seq or (mode in ("auto", "tiled") and sasrec_train_fits_tiled(model, n))


def _train_params(model):
    """The parameters the transformer's forward reads, in the order _SasTrain returns gradients."""
    ps = [model.item_emb.weight, model.pos_emb.weight]
    for la, at, lf, ff in zip(model.attention_layernorms, model.attention_layers, model.forward_layernorms,
                              model.forward_layers):
        ps += [la.weight, la.bias, at.in_proj_weight, at.in_proj_bias, at.out_proj.weight, at.out_proj.bias,
               lf.weight, lf.bias, ff[0].weight, ff[0].bias, ff[3].weight, ff[3].bias]
    return ps + [model.last_layernorm.weight, model.last_layernorm.bias]


class _SasTrain(torch.autograd.Function):
    """Train-mode SASRec forward (dropout on) and its backward on one of the two kernel sets (same
    saved activations, dropout masks and g_vec layout: csrc/sasrec_train_contract.h).  ``tiled``
    False: sasrec_train.hip, one launch each, one workgroup and one partial row of g_vec per sequence
    (n, d <= 64, mlp_layer <= 128).  True: sasrec_train_tiled.hip (n <= 256, d <= 128, mlp_layer <=
    256), tiled launches over all B * n rows, ``gr_sasrec_train_tiled_parts`` partial rows (split-k
    chunks of the rows) and a workspace, allocated like the saved buffers (inside a captured step:
    from the graph's pool).  Every parameter gradient but the item table's is the sum of g_vec's
    rows, sliced in ``_train_params`` order; item-table rows are scattered in the kernel."""

    @staticmethod
    def _launch(which, ctx, cb, *tensors):
        """gr_sasrec_train[_tiled]_{fwd,bwd}_f32 on ctx's step."""
        seqs, p = ctx.seqs, ctx.binding.p
        B, n = seqs.shape
        dev = seqs.device
        name = f"gr_sasrec_train_{'tiled_' if ctx.tiled else ''}{which}_f32"
        args = [L.ptr(t) for t in tensors]
        with L.on(dev):
            if ctx.tiled:
                nbytes = L.lib().gr_sasrec_train_tiled_workspace_bytes(ctypes.byref(p), B, n)
                ws = L.workspace(nbytes, dev)
                args += [L.ptr(ws), nbytes]
            L.check(getattr(L.lib(), name)(ctypes.byref(p), L.ptr(seqs), B, n, float(ctx.p_drop), 0, L.ptr(ctx.seed),
                                           ctypes.byref(cb), *args, L.stream_of(dev)), name)

    @staticmethod
    def forward(ctx, seqs, binding, tiled, p_drop, seed_snap, *params):
        B, n = seqs.shape
        p = binding.p
        d, m, nb, H = p.d, p.mlp, p.n_blocks, p.n_heads
        R = B * n
        e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=seqs.device)   # noqa: E731
        bufs = {"xin": e(nb, R, d), "hs": e(nb, R, d), "qkv": e(nb, R, 3 * d), "prob": e(nb, B, H, n, n),
                "os": e(nb, R, d), "x1": e(nb, R, d), "fs": e(nb, R, d), "zs": e(nb, R, m), "us": e(nb, R, m),
                "xl": e(R, d)}
        out = e(B, n, d)
        err = err_flag(seqs.device)
        ctx.binding, ctx.tiled, ctx.p_drop, ctx.bufs, ctx.seqs, ctx.seed = binding, tiled, p_drop, bufs, seqs, seed_snap
        ctx.shapes = [q.shape for q in params]   # item table, positions, then g_vec's order
        vw = L.lib().gr_sasrec_train_vec_width(ctypes.byref(p), n)
        if sum(math.prod(shp) for shp in ctx.shapes[2:]) + n * d != vw:
            raise RuntimeError(f"_SasTrain: the parameters do not fill a g_vec row of {vw} floats")
        _SasTrain._launch("fwd", ctx, L.SasrecTrainBufs(**{k: v.data_ptr() for k, v in bufs.items()}), out, err)
        _check_err(err)
        return out

    @staticmethod
    def backward(ctx, dout):
        seqs, p = ctx.seqs, ctx.binding.p
        B, n = seqs.shape
        dev = seqs.device
        vw = L.lib().gr_sasrec_train_vec_width(ctypes.byref(p), n)
        parts = L.lib().gr_sasrec_train_tiled_parts(ctypes.byref(p), B, n) if ctx.tiled else B
        g_vec = torch.empty((parts, vw), dtype=torch.float32, device=dev)
        g_item = torch.zeros((p.item_rows, p.d), dtype=torch.float32, device=dev)
        cb = L.SasrecTrainBufs(g_vec=g_vec.data_ptr(), **{k: v.data_ptr() for k, v in ctx.bufs.items()})
        _SasTrain._launch("bwd", ctx, cb, dout.contiguous().float(), g_item)
        vec = g_vec.sum(0)
        grads, off = [], 0
        for shp in ctx.shapes[2:]:
            grads.append(vec[off:off + math.prod(shp)].view(shp))
            off += math.prod(shp)
        # rows n.. of pos_emb get zeros (a pad kernel rather than a copy into a zeros tensor, which
        # keeps memset / memcpy nodes out of a captured step's graph)
        dpos = torch.nn.functional.pad(vec[off:].view(n, p.d), (0, 0, 0, ctx.shapes[1][0] - n))
        return (None, None, None, None, None, g_item, dpos, *grads)


def sasrec_train_forward(model, log_seqs):
    """``model.forward(log_seqs)`` in train mode with grad (SASRec/train.py:131): the transformer
    forward with dropout on the kernels, differentiable in every parameter it reads."""
    seqs = log_seqs.to(torch.int64).contiguous()
    L.require_gpu(seqs)
    n = seqs.shape[1]
    mode = getattr(model, "train_kernels", "auto")
    if mode not in ("auto", "sequence", "tiled"):
        raise ValueError(f"train_kernels must be 'auto', 'sequence' or 'tiled', got {mode!r}")
    if mode == "sequence" and not sasrec_train_fits_sequence(model, n):
        raise RuntimeError("train_kernels = 'sequence': the one-workgroup-per-sequence kernels take n, d <= 64 and "
                           f"mlp_layer <= 128 (got n {n}, d {model.d}, mlp_layer {model.mlp_layer})")
    tiled = mode == "tiled" or (mode == "auto" and not sasrec_train_fits_sequence(model, n))
    if tiled and not sasrec_train_fits_tiled(model, n):
        raise RuntimeError("the tiled training kernels take n <= 256, d <= 128 and mlp_layer <= 256 "
                           f"(got n {n}, d {model.d}, mlp_layer {model.mlp_layer})")
    seed = dropout_seed(seqs.device)
    snap = seed + 0              # this step's masks (forward and backward read the same word); a kernel, not a copy
    seed.add_(1)
    return _SasTrain.apply(seqs, sasrec_binding(model), tiled, float(model.dropout), snap, *_train_params(model))


class _CapturedStep:
    """A training step (``self._body()``: forward, loss, backward and, with ``self.opt``, the optimizer
    step) captured once as a graph (hipGraph via ``torch.cuda.graph``) and replayed.  ``_capture``
    owns the protocol: snapshot what the warm-up moves (the optimizer's parameters, its state tensors
    and tensor learning rates, the module's buffers), run ``warmup`` steps on a side stream
    (allocator, autograd and the optimizer's lazily created state), clear the gradients, capture the
    detached outputs as ``self.out`` (the captured autograd graph and its AccumulateGrad nodes,
    created on the capture stream, are released, so later eager backwards into the same leaves stay
    on their own stream), restore the snapshot: the first replay is the first real step.  State the
    warm-up created starts from zero.

    A subclass that leaves ``graph`` None runs ``_body`` eagerly in ``replay``: that is the path with
    the transformer / MLPs under torch autograd.  Back-to-back replays of that graph faulted (HSA
    memory aperture violation) in rocPRIM's unique-by-key partition kernel of the item-embedding
    backward (profiles/r02_train_graph_diag.txt); a graph of captured memsets and kernels replays
    correctly back to back (profiles/r03_graph_memset.txt), so round 2's memset-node explanation
    does not hold, and the fault stays inside that rocPRIM kernel.  Round 2 synchronised the device
    after every replay; not capturing that path at all makes every path run without a host
    synchronisation and without the faulting configuration."""

    graph = opt = None
    _check = False   # a row whose negative population may be short: the reference raises

    def _clear_grads(self):
        self.opt.zero_grad(set_to_none=True)

    def _capture(self, dev, warmup, module=None):
        opt = self.opt
        params = [p for g in opt.param_groups for p in g["params"]] if opt else []
        state = lambda: [v for p in params for v in opt.state.get(p, {}).values() if torch.is_tensor(v)]   # noqa: E731
        keep = params + state() + [g["lr"] for g in (opt.param_groups if opt else []) if torch.is_tensor(g["lr"])]
        keep += list(module.buffers()) if module is not None else []
        saved = [t.detach().clone() for t in keep]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._clear_grads()
                self._body()
        torch.cuda.current_stream(dev).wait_stream(side)
        self._clear_grads()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = tuple(x.detach() for x in self._body())
        with torch.no_grad():
            known = {id(t) for t in keep}
            for v in state():
                if id(v) not in known:
                    v.zero_()
            for t, old in zip(keep, saved):
                t.copy_(old)

    def replay(self):
        """Run one step; returns the step's outputs (captured: its static tensors), with no host
        synchronisation between replays."""
        if self.graph is None:
            out = tuple(x.detach() for x in self._body())
        else:
            self.graph.replay()
            if self.opt is not None:
                weights_changed()   # the captured optimizer step moved the weights without a version bump
            out = self.out
        if self._check:
            check_errors(self.inputs.device)
        return out


class SasTrainStepGraph(_CapturedStep):
    """The training-side scoring step of SASRec/train.py:131-167 -- negatives (train.py:142),
    scores + sampled BCE (134-158), ``loss = batch_loss / batch_valid_t`` (161-164) and its backward
    into ``feats.grad`` / ``table.grad`` -- captured once as a graph (hipGraph via
    ``torch.cuda.graph``) and replayed: one launch per step instead of ~20 host-issued ones.

    ``feats`` [B, n, d] and ``table`` [rows, d] are leaf tensors with ``requires_grad``; ``inputs``
    (the sequences the negatives avoid) and ``targets`` are the step's static inputs: copy a new
    batch into them before ``replay()``.  Each replay draws fresh negatives (device-side seed).
    ``replay()`` returns the static ``(batch_loss, batch_valid_t)`` device scalars and leaves the
    gradients in ``.grad`` (overwritten, not accumulated, as with ``zero_grad(set_to_none=True)``
    before each reference step).  A step with no valid position gives loss 0 and zero gradients,
    as the reference's ``if batch_valid_t > 0`` does."""

    def __init__(self, feats, table, inputs, targets, item_num, num_neg, eps, seed=0, warmup=3):
        L.require_gpu(feats, table, inputs, targets)
        if not (feats.is_leaf and table.is_leaf and feats.requires_grad and table.requires_grad):
            raise RuntimeError("SasTrainStepGraph: feats and table must be leaf tensors requiring grad")
        self.feats, self.table, self.inputs, self.targets = feats, table, inputs, targets
        self.item_num, self.num_neg, self.eps = int(item_num), int(num_neg), float(eps)
        self._check = CHECK or 2 * (inputs.shape[1] + self.num_neg) > self.item_num
        self.seed = torch.tensor([int(seed)], dtype=torch.int64, device=feats.device)
        self._capture(feats.device, warmup)

    def _clear_grads(self):
        self.feats.grad = self.table.grad = None

    def _body(self):
        negs = neg_samples(self.inputs, self.item_num, self.num_neg, seed_tensor=self.seed)
        bl, valid = sampled_bce_loss(self.feats, self.table, self.targets, negs, self.eps)
        (bl / valid.clamp(min=1.0)).backward()   # batch_loss is 0 when nothing is valid
        return bl, valid


class SasTrainGraph(_CapturedStep):
    """The whole SASRec training step of SASRec/train.py:131-173 -- the transformer forward in
    train mode (dropout on, the drop-in's autograd path), GPU negatives (device-seeded), the fused
    sampled BCE, ``loss = batch_loss / batch_valid_t``, backward and ``optimizer.step()`` --
    captured once as a graph (hipGraph via ``torch.cuda.graph``) and replayed: one launch per step
    instead of ~150 host-issued kernels at the reference's batch of 128.

    ``optimizer`` must be capturable (``torch.optim.Adam(..., capturable=True)``: its step counter
    lives on the device).  ``inputs`` [B, n] and ``targets`` [B, n] are the static batch tensors:
    copy each batch into them before ``replay()``, which returns the static ``(batch_loss,
    batch_valid_t)`` device scalars.  The warm-up steps are undone (``_CapturedStep``) and the negative
    sampler's seed is reset, so the first replay is the first real training step.  Of what is
    restored, the warm-up moves the parameters and Adam's state; tensor learning rates and module
    buffers it does not move, so restoring them changes nothing here.  Dropout draws from torch's
    graph-safe generator (fresh masks each replay)."""

    def __init__(self, model, optimizer, inputs, targets, item_num, num_neg, eps, seed=0, warmup=3,
                 capture=None):
        L.require_gpu(inputs, targets)
        self.model, self.opt = model, optimizer
        if capture is None:   # capture the fused-kernel step; the autograd fallback runs eagerly
            capture = bool(getattr(model, "fused_train", False) and sasrec_train_supported(model, inputs.shape[1]))
        self.inputs, self.targets = inputs, targets
        self.item_num, self.num_neg, self.eps = int(item_num), int(num_neg), float(eps)
        self._check = CHECK or 2 * (inputs.shape[1] + self.num_neg) > self.item_num
        dev = inputs.device
        self.seed = torch.tensor([int(seed)], dtype=torch.int64, device=dev)
        if capture:
            self._capture(dev, warmup, model)
            self.seed.fill_(int(seed))   # the warm-up advanced the negative sampler

    def _body(self):
        self.opt.zero_grad(set_to_none=True)
        feats = self.model(self.inputs)                                            # train.py:131
        negs = neg_samples(self.inputs, self.item_num, self.num_neg, seed_tensor=self.seed)   # :142
        bl, valid = sampled_bce_loss(feats, self.model.item_emb.weight, self.targets, negs, self.eps)
        (bl / valid.clamp(min=1.0)).backward()   # :161-172 (batch_loss is 0 when nothing is valid)
        self.opt.step()                                                            # :173
        return bl, valid


class RqTrainGraph(_CapturedStep):
    """One RQ-VAE training step of RQ-VAE/train.py:108-119 -- ``out, rq_loss, indices =
    model(data)`` (every level's Sinkhorn / argmin assignment on the kernels, dropout on),
    ``compute_loss``, ``loss.backward()``, ``clip_grad_norm_(params, 1.0)`` and ``optimizer.step()``
    -- captured once as a graph (hipGraph via ``torch.cuda.graph``) and replayed: one launch per
    step instead of ~200 host-issued kernels at the reference's batch of 64 (main.py:26).

    ``optimizer`` must be capturable with a tensor learning rate (``torch.optim.AdamW(params,
    lr=torch.tensor(1e-3, device=dev), weight_decay=1e-4, capturable=True)``): its step counter
    and lr live on the device, and a scheduler built on it (``get_linear_schedule_with_warmup``,
    train.py:81-89) writes the new lr in place, so ``scheduler.step()`` after ``replay()`` reaches
    the captured step.  ``inputs`` [B, in_dim] is the static batch: copy each batch into it before
    ``replay()``, which returns the static ``(loss, loss_recon, indices)`` device tensors
    (train.py:120-121's ``.item()`` becomes a device-side sum the caller reads once per epoch).

    A model with ``kmeans_init`` and codebooks not yet initialised is initialised here on
    ``inputs`` -- the reference's first training batch does the same (vq.py:66-67) -- before the
    capture.  The warm-up steps are undone afterwards (``_CapturedStep``), so the first replay is the
    first real training step.  Dropout draws from torch's graph-safe generator (fresh masks each
    replay).  On the kernel path (fused MLPs and quantizer) replays run back to back
    (tests/test_rq_train_gpu.py); with the torch modules (``fused_train = False``, BatchNorm) the step
    runs eagerly (``_CapturedStep`` explains why).  ``capture`` overrides the choice."""

    def __init__(self, model, optimizer, inputs, max_norm=1.0, use_sk=True, warmup=3, capture=None):
        L.require_gpu(inputs)
        for g in optimizer.param_groups:
            if not g.get("capturable", False) or not torch.is_tensor(g["lr"]):
                raise RuntimeError("RqTrainGraph: the optimizer must be capturable with a tensor lr "
                                   "(e.g. AdamW(params, lr=torch.tensor(1e-3, device=dev), capturable=True))")
        self.model, self.opt, self.inputs = model, optimizer, inputs
        if capture is None:   # capture the kernel path; the torch-module fallback runs eagerly
            capture = bool(getattr(model.encoder, "fused_train", False) and getattr(model.decoder, "fused_train", False)
                           and getattr(model.rq, "fused_train", False) and mlp_train_supported(model.encoder, inputs)
                           and not model.bn)
        self.max_norm, self.use_sk = float(max_norm), bool(use_sk)
        dev = inputs.device
        if model.training and any(not q.initted for q in model.rq.vq_layers):
            with torch.no_grad():   # vq.py:66-67: k-means init on the first batch's residuals
                model(inputs, use_sk=self.use_sk)
        if capture:   # buffers too: with bn=True every train-mode BatchNorm forward moves its running statistics
            self._capture(dev, warmup, model)

    def _body(self):
        self.opt.zero_grad(set_to_none=True)
        out, rq_loss, indices = self.model(self.inputs, use_sk=self.use_sk)           # train.py:113
        loss, loss_recon = self.model.compute_loss(out, rq_loss, xs=self.inputs)     # :114
        loss.backward()                                                              # :116
        torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_norm)       # :117
        self.opt.step()                                                              # :118
        return loss, loss_recon, indices


class _RqQuantTrain(torch.autograd.Function):
    """ResidualVectorQuantizer.forward under autograd (rq.py:39-56, vq.py:63-99) in one launch
    forward and two backward: the assignment of every level (Sinkhorn or argmin), x_q and the mse
    numerators (gr_rq_quantize_sk_train_f32); dz and every codebook's gradient
    (gr_rq_quantize_sk_train_bwd_f32)."""

    @staticmethod
    def forward(ctx, z, beta, sk_eps, sk_iters, *codebooks):
        n, e = z.shape
        dev = z.device
        Ks = [c.shape[0] for c in codebooks]
        lib = L.lib()
        ks_c = L.i32_array(Ks)
        eps_c = (ctypes.c_double * len(codebooks))(*[float(v) for v in sk_eps])
        nbytes = lib.gr_rq_encode_sk_workspace_bytes(n, e, len(codebooks), ks_c)
        wsp = L.workspace(nbytes, dev)
        idx = torch.empty((n, len(codebooks)), dtype=torch.int64, device=dev)
        xq = torch.empty((n, e), dtype=torch.float32, device=dev)
        sq = torch.empty((n, len(codebooks)), dtype=torch.float32, device=dev)
        with L.on(dev):
            L.check(lib.gr_rq_quantize_sk_train_f32(L.ptr(z), n, e, len(codebooks), ks_c, L.ptr_array(codebooks),
                                                    eps_c, int(sk_iters), L.ptr(_group_ptr([n], dev)), 1,
                                                    L.ptr(idx), L.ptr(xq), L.ptr(sq), L.ptr(wsp), nbytes,
                                                    L.stream_of(dev)), "gr_rq_quantize_sk_train_f32")
        m = sq.sum(0) / float(n * e)                       # vq.py:88-89: mse per level
        rq_loss = (m + beta * m).mean()                    # vq.py:90, rq.py:51
        ctx.save_for_backward(z, idx, *codebooks)
        ctx.beta = float(beta)
        ctx.mark_non_differentiable(idx)
        return xq, rq_loss, idx

    @staticmethod
    def backward(ctx, g_xq, g_rq, _g_idx):
        z, idx, *codebooks = ctx.saved_tensors
        n, e = z.shape
        dev = z.device
        g_rq = (g_rq if g_rq is not None else torch.zeros((), device=dev)).to(torch.float32).contiguous()
        g_xq = g_xq.contiguous() if g_xq is not None else None
        dz = torch.empty_like(z)
        dcs = [torch.empty_like(c) for c in codebooks]
        with L.on(dev):
            L.check(L.lib().gr_rq_quantize_sk_train_bwd_f32(
                L.ptr(z), n, e, len(codebooks), L.i32_array([c.shape[0] for c in codebooks]),
                L.ptr_array(codebooks), L.ptr(idx), L.ptr(g_xq) if g_xq is not None else None, L.ptr(g_rq),
                ctypes.c_float(ctx.beta), L.ptr(dz), L.ptr_array(dcs), L.stream_of(dev)),
                "gr_rq_quantize_sk_train_bwd_f32")
        return (dz, None, None, None, *dcs)


def rq_quantize_train(z, codebooks, beta, sk_eps, sk_iters):
    """``(x_q, rq_loss, indices)`` of ResidualVectorQuantizer.forward(z, use_sk) in training
    (rq.py:39-56): differentiable in ``z`` and every codebook, the whole batch one Sinkhorn group
    per level where ``sk_eps[l] > 0`` (vq.py:76-84), the plain argmin elsewhere."""
    L.require_gpu(z, *codebooks)
    if z.dtype != torch.float32 or any(c.dtype != torch.float32 for c in codebooks):
        raise TypeError("rq_quantize_train takes float32 tensors")
    if any(c.shape[0] > 1024 for c in codebooks):
        raise RuntimeError("rq_quantize_train: codebooks of at most 1024 codes")
    return _RqQuantTrain.apply(z.contiguous(), float(beta), [float(v) for v in sk_eps], int(sk_iters),
                               *[c.contiguous() if not c.is_contiguous() else c for c in codebooks])


class _MlpTrain(torch.autograd.Function):
    """MLPLayers.forward in train mode (RQ-VAE/models/layers.py:18-43) and its backward on the
    kernels of rq_mlp_train.hip: the input dropout, then one launch per layer forward (bias, ReLU,
    and the next layer's dropout in the epilogue) and one per layer backward (weight and bias
    gradients and the input gradient with the ReLU and dropout masks folded in)."""

    @staticmethod
    def forward(ctx, x, p, snap, *params):
        ws, bs = params[0::2], params[1::2]
        n = len(ws)
        M = x.shape[0]
        dev = x.device
        dims = [x.shape[1]] + [w.shape[0] for w in ws]
        outs = [torch.empty((M, dd), dtype=torch.float32, device=dev) for dd in dims[1:]]
        xd0 = torch.empty_like(x) if p > 0 else x
        with L.on(dev):
            L.check(L.lib().gr_mlp_train_fwd_f32(L.ptr(x), M, n, L.i32_array(dims), L.ptr_array(ws),
                                                 L.ptr_array(bs), float(p), L.ptr(snap),
                                                 L.ptr(xd0) if p > 0 else None, L.ptr_array(outs),
                                                 L.stream_of(dev)), "gr_mlp_train_fwd_f32")
        ctx.save_for_backward(xd0, snap, *outs[:-1], *ws)
        ctx.p, ctx.n = float(p), n
        return outs[-1]

    @staticmethod
    def backward(ctx, dout):
        xd0, snap, *rest = ctx.saved_tensors
        n = ctx.n
        acts, ws = [xd0] + rest[:n - 1], rest[n - 1:]
        M = xd0.shape[0]
        dev = xd0.device
        dz = dout.contiguous().float()
        gw, gb = [None] * n, [None] * n
        with L.on(dev):
            for i in reversed(range(n)):
                K, N = acts[i].shape[1], ws[i].shape[0]
                dW = torch.empty_like(ws[i])
                db = torch.empty((N,), dtype=torch.float32, device=dev)
                dX = (torch.empty((M, K), dtype=torch.float32, device=dev)
                      if i > 0 or ctx.needs_input_grad[0] else None)
                L.check(L.lib().gr_mlp_train_bwd_layer_f32(
                    L.ptr(acts[i]), M, K, L.ptr(ws[i]), N, L.ptr(dz), 1 if i > 0 else 2, ctx.p, L.ptr(snap), 0,
                    L.ptr(dW), L.ptr(db), L.ptr(dX), L.stream_of(dev)), "gr_mlp_train_bwd_layer_f32")
                gw[i], gb[i] = dW, db
                dz = dX
        grads = [dz if ctx.needs_input_grad[0] else None, None, None]
        for w, b in zip(gw, gb):
            grads += [w, b]
        return tuple(grads)


def mlp_train_supported(mlp, x):
    lin = mlp.linears()
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and not mlp.use_bn
            and (mlp.act == "relu" or len(lin) == 1) and all(m.bias is not None for m in lin)
            and x.shape[1] == lin[0].weight.shape[1])


def mlp_train(x, mlp):
    """``mlp.mlp_layers(x)`` under autograd (RQ-VAE/models/layers.py:42-43 as RQVAE.forward calls it
    in training, RQ-VAE/train.py:113): dropout (train mode), Linear, ReLU on the fused training
    kernels, differentiable in ``x`` and every Linear's weight and bias.  Dropout masks come from the
    device's seed word (``dropout_seed``), so a captured step replays with fresh masks."""
    L.require_gpu(x)
    p = float(mlp.dropout) if mlp.training else 0.0
    seed = dropout_seed(x.device)
    snap = seed + 0              # this call's masks (its backward reads the same word)
    seed.add_(1)
    params = []
    for m in mlp.linears():
        params += [m.weight, m.bias]
    return _MlpTrain.apply(x.contiguous(), p, snap, *params)


TIGER_ENVELOPE = ("d_model in {32, 64}; num_heads * d_kv in {32, 64} with d_kv in {8, 16, 32}; d_ff <= 256 and a "
                  "multiple of 32; 1..4 layers on each side; 2 * num_beams <= vocab_size <= 128; at most 128 history "
                  "tokens; num_beams <= 32; max_length <= 8; at most 2**21 users per call; 32 relative-attention "
                  "buckets over distance 128; tied embeddings; feed_forward_proj 'relu'; one EOS id")
TIGER_ENC_KEYS = ("layer.0.layer_norm", "layer.0.SelfAttention.q", "layer.0.SelfAttention.k", "layer.0.SelfAttention.v",
                  "layer.0.SelfAttention.o", "layer.1.layer_norm", "layer.1.DenseReluDense.wi",
                  "layer.1.DenseReluDense.wo")
TIGER_DEC_KEYS = ("layer.0.layer_norm", "layer.0.SelfAttention.q", "layer.0.SelfAttention.k", "layer.0.SelfAttention.v",
                  "layer.0.SelfAttention.o", "layer.1.layer_norm", "layer.1.EncDecAttention.q",
                  "layer.1.EncDecAttention.k", "layer.1.EncDecAttention.v", "layer.1.EncDecAttention.o",
                  "layer.2.layer_norm", "layer.2.DenseReluDense.wi", "layer.2.DenseReluDense.wo")
TIGER_REL = "layer.0.SelfAttention.relative_attention_bias"


def t5_relative_bucket(relative_position, bidirectional, num_buckets=32, max_distance=128):
    """T5's bucket of a relative position (key position - query position), in the library's own
    arithmetic (float32 log, truncation), so that the tables the kernels index are the library's."""
    import math
    rp = relative_position
    buckets = torch.zeros_like(rp)
    if bidirectional:
        num_buckets //= 2
        buckets = buckets + (rp > 0).to(torch.long) * num_buckets
        rp = rp.abs()
    else:
        rp = -torch.min(rp, torch.zeros_like(rp))
    max_exact = num_buckets // 2
    large = max_exact + (torch.log(rp.float() / max_exact) / math.log(max_distance / max_exact)
                         * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(rp < max_exact, rp, large)


def tiger_check_config(cfg, num_beams=None, S=None, max_length=None):
    """Raise NotImplementedError, naming the limit, for a configuration outside the kernels' envelope."""
    def no(msg):
        raise NotImplementedError(f"TIGER: {msg} (the gfx950 kernels cover: {TIGER_ENVELOPE}); there is no CPU "
                                  "fallback")
    if cfg.get("feed_forward_proj", "relu") != "relu":
        no(f"feed_forward_proj={cfg['feed_forward_proj']!r} is not built, only 'relu'")
    if int(cfg.get("relative_attention_num_buckets", 32)) != 32:
        no(f"relative_attention_num_buckets={cfg['relative_attention_num_buckets']} is not built, only 32")
    if int(cfg.get("relative_attention_max_distance", 128)) != 128:
        no(f"relative_attention_max_distance={cfg['relative_attention_max_distance']} is not built, only 128")
    if cfg.get("tie_word_embeddings", True) is False:
        no("tie_word_embeddings=False is not built: lm_head is the shared embedding")
    eos = cfg["eos_token_id"]
    if isinstance(eos, (list, tuple)):
        if len(eos) != 1:
            no("only one EOS id is supported")
        eos = eos[0]
    d, dkv, H, dff, V = (int(cfg[k]) for k in ("d_model", "d_kv", "num_heads", "d_ff", "vocab_size"))
    if d not in (32, 64):
        no(f"d_model={d} must be 32 or 64")
    if dkv not in (8, 16, 32):
        no(f"d_kv={dkv} must be 8, 16 or 32")
    if H * dkv not in (32, 64):
        no(f"num_heads * d_kv = {H * dkv} must be 32 or 64")
    if dff > 256 or dff < 32 or dff % 32:
        no(f"d_ff={dff} must be a multiple of 32, at most 256")
    for k in ("num_layers", "num_decoder_layers"):
        if not 1 <= int(cfg[k]) <= 4:
            no(f"{k}={cfg[k]} must be 1..4")
    if V > 128:
        no(f"vocab_size={V} must be at most 128")
    if not (0 <= int(eos) < V and 0 <= int(cfg["pad_token_id"]) < V):
        raise ValueError("TIGER: pad_token_id and eos_token_id must lie in [0, vocab_size)")
    if num_beams is not None:
        if not 1 <= num_beams <= 32:
            no(f"num_beams={num_beams} must be 1..32")
        if V < 2 * num_beams:
            no(f"vocab_size={V} must be at least 2 * num_beams = {2 * num_beams}: below that the -1e9-masked dead "
               "beams reach the selection as exact fp32 ties")
    if S is not None and not 1 <= S <= 128:
        no(f"a history of {S} tokens; at most 128 are supported")
    if max_length is not None and not 2 <= max_length <= 8:
        no(f"max_length={max_length} must be 2..8")
    return int(eos)


class TigerBinding:
    """Device-pointer view of a T5 parameter set (``gr_tiger_params``).  ``tensors``: name -> tensor with the
    reference's T5 names (``shared.weight``, ``encoder.block.0.layer.0.SelfAttention.q.weight``, ...).  The
    pointers are the tensors' own storage, so in-place weight updates are seen by the next call."""

    def __init__(self, cfg, tensors):
        eos = tiger_check_config(cfg)
        self.cfg = cfg
        self.keep = []
        dev = tensors["shared.weight"].device
        self.device = dev
        p = L.TigerParams()
        p.vocab, p.d_model, p.d_kv, p.n_heads = (int(cfg[k]) for k in ("vocab_size", "d_model", "d_kv", "num_heads"))
        p.d_ff, p.n_enc, p.n_dec, p.n_buckets = int(cfg["d_ff"]), int(cfg["num_layers"]), int(cfg["num_decoder_layers"]), 32
        p.pad_id, p.eos_id = int(cfg["pad_token_id"]), eos
        p.fill_id = p.pad_id or eos          # the library's `pad_token_id or eos_token_id[0]`
        p.eps = float(cfg.get("layer_norm_epsilon", 1e-6))
        p.lm_scale = float(p.d_model ** -0.5) if cfg.get("scale_decoder_outputs", True) else 1.0
        f = self._f
        p.shared, p.lm_head = f(tensors["shared.weight"]), f(tensors["lm_head.weight"])
        p.enc_rel = f(tensors[f"encoder.block.0.{TIGER_REL}.weight"])
        p.dec_rel = f(tensors[f"decoder.block.0.{TIGER_REL}.weight"])
        p.enc_final_ln = f(tensors["encoder.final_layer_norm.weight"])
        p.dec_final_ln = f(tensors["decoder.final_layer_norm.weight"])
        for l in range(p.n_enc):
            for i, k in enumerate(TIGER_ENC_KEYS):
                p.enc[l][i] = f(tensors[f"encoder.block.{l}.{k}.weight"])
        for l in range(p.n_dec):
            for i, k in enumerate(TIGER_DEC_KEYS):
                p.dec[l][i] = f(tensors[f"decoder.block.{l}.{k}.weight"])
        r = torch.arange(-127, 128)
        self.enc_bucket = t5_relative_bucket(r, True).to(torch.int32).to(dev)
        self.dec_bucket = t5_relative_bucket(-torch.arange(8), False).to(torch.int32).to(dev)
        p.enc_bucket, p.dec_bucket = self.enc_bucket.data_ptr(), self.dec_bucket.data_ptr()
        self.params = p
        self.ref = ctypes.byref(p)
        self._ws = {}

    def _f(self, t):
        L.require_gpu(t)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("TIGER kernels take contiguous float32 parameters")
        self.keep.append(t)
        return t.data_ptr()

    def workspace_bytes(self, B, S, num_beams, max_length):
        key = (B, S, num_beams, max_length)
        n = self._ws.get(key)
        if n is None:
            n = self._ws[key] = L.lib().gr_tiger_workspace_bytes(self.ref, B, S, num_beams, max_length)
        return n

    def forward_workspace_bytes(self, B, S, Ld):
        key = ("forward", B, S, Ld)
        n = self._ws.get(key)
        if n is None:
            n = self._ws[key] = L.lib().gr_tiger_forward_workspace_bytes(self.ref, B, S, Ld)
        return n


def tiger_generate(binding, input_ids, attention_mask=None, num_beams=20, max_length=5, with_encoder=False,
                   with_logits=False):
    """``gr_tiger_generate_f32``: T5 encode and the whole beam search in one C call, nothing synchronises.
    -> (sequences [B, num_beams, max_length] int64, scores [B, num_beams] fp32[, encoder output
    [B, S, d_model]][, step logits [B, max_length - 1, num_beams, vocab]])."""
    L.require_gpu(input_ids)
    if input_ids.dim() != 2 or input_ids.dtype != torch.int64:
        raise RuntimeError(f"tiger_generate takes [B, S] int64 token ids, got {tuple(input_ids.shape)} {input_ids.dtype}")
    B, S = input_ids.shape
    num_beams, max_length = int(num_beams), int(max_length)
    tiger_check_config(binding.cfg, num_beams, S, max_length)
    input_ids = input_ids.contiguous()
    if attention_mask is not None:
        L.require_gpu(attention_mask)
        if tuple(attention_mask.shape) != (B, S):
            raise RuntimeError(f"attention_mask must be [{B}, {S}], got {tuple(attention_mask.shape)}")
        if attention_mask.dtype != torch.int64:
            attention_mask = attention_mask.to(torch.int64)
        attention_mask = attention_mask.contiguous()
    dev = input_ids.device
    V, D = binding.params.vocab, binding.params.d_model
    seqs = torch.empty((B, num_beams, max_length), dtype=torch.int64, device=dev)
    scores = torch.empty((B, num_beams), dtype=torch.float32, device=dev)
    enc = torch.empty((B, S, D), dtype=torch.float32, device=dev) if with_encoder else None
    logits = torch.empty((B, max_length - 1, num_beams, V), dtype=torch.float32, device=dev) if with_logits else None
    nbytes = binding.workspace_bytes(B, S, num_beams, max_length)
    wsp = L.workspace(nbytes, dev)
    with L.on(dev):
        L.check(L.lib().gr_tiger_generate_f32(binding.ref, L.ptr(input_ids), L.ptr(attention_mask), B, S, num_beams,
                                              max_length, L.ptr(seqs), L.ptr(scores), L.ptr(enc), L.ptr(logits),
                                              L.ptr(wsp), nbytes, L.stream_of(dev)), "gr_tiger_generate_f32")
    out = (seqs, scores)
    if with_encoder:
        out += (enc,)
    if with_logits:
        out += (logits,)
    return out


TIGER_ADAPTER_KEYS = ("bert_proj.weight", "bert_proj.bias", "cross_attn.in_proj_weight", "cross_attn.in_proj_bias",
                      "cross_attn.out_proj.weight", "cross_attn.out_proj.bias", "ffn.0.weight", "ffn.0.bias",
                      "ffn.2.weight", "ffn.2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
TIGER_PREFIX_ENVELOPE = ("with prof_lvl1..3: at most 125 history tokens (128 encoder positions with the three prefix "
                         "tokens); bert_dim a multiple of 4 in [4, 1024]; 1..16 vectors per level; d_model a multiple "
                         "of num_heads")


def tiger_prefix_check(cfg, bert_dim, n_vec=None, S=None):
    """Raise NotImplementedError, naming the limit, for what the adapter kernel does not cover."""
    def no(msg):
        raise NotImplementedError(f"TIGER: {msg} (the gfx950 kernels cover: {TIGER_ENVELOPE}; {TIGER_PREFIX_ENVELOPE}); "
                                  "there is no CPU fallback")
    if not 4 <= int(bert_dim) <= 1024 or int(bert_dim) % 4:
        no(f"bert_dim={bert_dim} must be a multiple of 4 in [4, 1024]")
    if int(cfg["d_model"]) % int(cfg["num_heads"]):
        no(f"d_model={cfg['d_model']} must be a multiple of num_heads={cfg['num_heads']} (the adapters' head width)")
    if n_vec is not None and not 1 <= n_vec <= 16:
        no(f"n_vec={n_vec} vectors per level; 1..16 are supported")
    if S is not None and not 1 <= S <= 125:
        no(f"a history of {S} tokens; with the three prefix tokens at most 125 are supported")


class TigerPrefixBinding:
    """Device-pointer view of a prefix model: the T5 parameters (``.t5``, a ``TigerBinding``) and the three
    adapters (``gr_tiger_prefix_params``).  ``adapters``: name -> tensor with the reference's names
    (``adapter_lvl1.bert_proj.weight``, ...).  The pointers are the tensors' own storage, so in-place
    weight updates are seen by the next call."""

    def __init__(self, cfg, tensors, adapters, ln_eps=1e-5):
        self.t5 = TigerBinding(cfg, tensors)
        self.cfg = cfg
        self.device = self.t5.device
        self.bert_dim = int(adapters["adapter_lvl1.bert_proj.weight"].shape[1])
        tiger_prefix_check(cfg, self.bert_dim)
        self.keep = []
        d = int(cfg["d_model"])
        shapes = {"bert_proj.weight": (d, self.bert_dim), "cross_attn.in_proj_weight": (3 * d, d),
                  "cross_attn.in_proj_bias": (3 * d,), "cross_attn.out_proj.weight": (d, d),
                  "ffn.0.weight": (4 * d, d), "ffn.0.bias": (4 * d,), "ffn.2.weight": (d, 4 * d)}
        pp = L.TigerPrefixParams()
        pp.bert_dim, pp.n_heads, pp.eps = self.bert_dim, int(cfg["num_heads"]), float(ln_eps)
        for lvl in range(3):
            for i, k in enumerate(TIGER_ADAPTER_KEYS):
                t = adapters[f"adapter_lvl{lvl + 1}.{k}"]
                if tuple(t.shape) != shapes.get(k, (d,)):
                    raise RuntimeError(f"adapter_lvl{lvl + 1}.{k} must be {shapes.get(k, (d,))}, got {tuple(t.shape)}")
                if t.device != self.device:
                    raise RuntimeError("the adapters and the T5 parameters must be on one device")
                pp.adapter[lvl][i] = self.t5._f(t)
        self.params = pp
        self._ws = {}

    def ref(self, n_vec):
        self.params.n_vec = n_vec
        return ctypes.byref(self.params)

    def workspace_bytes(self, n_vec, B, S, num_beams, max_length):
        key = (n_vec, B, S, num_beams, max_length)
        n = self._ws.get(key)
        if n is None:
            n = self._ws[key] = L.lib().gr_tiger_prefix_workspace_bytes(self.t5.ref, self.ref(n_vec), B, S, num_beams,
                                                                        max_length)
        return n

    def forward_workspace_bytes(self, n_vec, B, S, Ld):
        key = ("forward", n_vec, B, S, Ld)
        n = self._ws.get(key)
        if n is None:
            n = self._ws[key] = L.lib().gr_tiger_forward_prefix_workspace_bytes(self.t5.ref, self.ref(n_vec), B, S, Ld)
        return n


def tiger_generate_prefix(binding, input_ids, attention_mask, prof_lvl1, prof_lvl2, prof_lvl3, num_beams=20,
                          max_length=5, with_prefix=False, with_encoder=False, with_logits=False):
    """``gr_tiger_generate_prefix_f32``: the three adapters, T5 encode on S + 3 positions and the whole beam
    search in one C call (three launches), nothing synchronises.  prof_lvl1..3 [B, n_vec, bert_dim] fp32.
    -> (sequences [B, num_beams, max_length] int64, scores [B, num_beams] fp32[, prefix tokens
    [B, 3, d_model]][, encoder output [B, S + 3, d_model]][, step logits [B, max_length - 1, num_beams,
    vocab]])."""
    prof = [prof_lvl1, prof_lvl2, prof_lvl3]
    L.require_gpu(input_ids, *prof)
    if input_ids.dim() != 2 or input_ids.dtype != torch.int64:
        raise RuntimeError(f"tiger_generate_prefix takes [B, S] int64 token ids, got {tuple(input_ids.shape)} "
                           f"{input_ids.dtype}")
    B, S = input_ids.shape
    num_beams, max_length = int(num_beams), int(max_length)
    n_vec = int(prof[0].shape[1]) if prof[0].dim() == 3 else -1
    for i, t in enumerate(prof):
        if t.dtype != torch.float32 or tuple(t.shape) != (B, n_vec, binding.bert_dim):
            raise RuntimeError(f"prof_lvl{i + 1} must be float32 [{B}, n_vec, {binding.bert_dim}], got {t.dtype} "
                               f"{tuple(t.shape)}")
    tiger_prefix_check(binding.cfg, binding.bert_dim, n_vec, S)
    tiger_check_config(binding.cfg, num_beams, S + 3, max_length)
    prof = [t.contiguous() for t in prof]
    input_ids = input_ids.contiguous()
    if attention_mask is not None:
        L.require_gpu(attention_mask)
        if tuple(attention_mask.shape) != (B, S):
            raise RuntimeError(f"attention_mask must be [{B}, {S}], got {tuple(attention_mask.shape)}")
        if attention_mask.dtype != torch.int64:
            attention_mask = attention_mask.to(torch.int64)
        attention_mask = attention_mask.contiguous()
    dev = input_ids.device
    V, D = binding.t5.params.vocab, binding.t5.params.d_model
    seqs = torch.empty((B, num_beams, max_length), dtype=torch.int64, device=dev)
    scores = torch.empty((B, num_beams), dtype=torch.float32, device=dev)
    prefix = torch.empty((B, 3, D), dtype=torch.float32, device=dev) if with_prefix else None
    enc = torch.empty((B, S + 3, D), dtype=torch.float32, device=dev) if with_encoder else None
    logits = torch.empty((B, max_length - 1, num_beams, V), dtype=torch.float32, device=dev) if with_logits else None
    nbytes = binding.workspace_bytes(n_vec, B, S, num_beams, max_length)
    wsp = L.workspace(nbytes, dev)
    with L.on(dev):
        L.check(L.lib().gr_tiger_generate_prefix_f32(
            binding.t5.ref, binding.ref(n_vec), L.ptr(input_ids), L.ptr(attention_mask), L.ptr(prof[0]), L.ptr(prof[1]),
            L.ptr(prof[2]), B, S, num_beams, max_length, L.ptr(seqs), L.ptr(scores), L.ptr(prefix), L.ptr(enc),
            L.ptr(logits), L.ptr(wsp), nbytes, L.stream_of(dev)), "gr_tiger_generate_prefix_f32")
    out = (seqs, scores)
    for on, t in ((with_prefix, prefix), (with_encoder, enc), (with_logits, logits)):
        if on:
            out += (t,)
    return out


def _tiger_forward_args(what, input_ids, attention_mask, labels):
    """The shape and dtype checks both forward calls share -> (ids, mask, labels, B, S, Ld), contiguous."""
    L.require_gpu(input_ids, labels)
    if input_ids.dim() != 2 or input_ids.dtype != torch.int64:
        raise RuntimeError(f"{what} takes [B, S] int64 token ids, got {tuple(input_ids.shape)} {input_ids.dtype}")
    B, S = input_ids.shape
    if labels.dim() != 2 or labels.shape[0] != B or labels.dtype != torch.int64:
        raise RuntimeError(f"{what} takes [{B}, Ld] int64 labels, got {tuple(labels.shape)} {labels.dtype}")
    Ld = int(labels.shape[1])
    if not 1 <= Ld <= 8:
        raise NotImplementedError(f"TIGER: labels of {Ld} positions; 1..8 are supported (the gfx950 kernels cover: "
                                  f"{TIGER_ENVELOPE}); there is no CPU fallback")
    if attention_mask is not None:
        L.require_gpu(attention_mask)
        if tuple(attention_mask.shape) != (B, S):
            raise RuntimeError(f"attention_mask must be [{B}, {S}], got {tuple(attention_mask.shape)}")
        if attention_mask.dtype != torch.int64:
            attention_mask = attention_mask.to(torch.int64)
        attention_mask = attention_mask.contiguous()
    return input_ids.contiguous(), attention_mask, labels.contiguous(), B, S, Ld


def _tiger_forward_outputs(B, S_enc, Ld, V, D, dev, with_logits, with_nll, with_encoder):
    loss = torch.empty((), dtype=torch.float32, device=dev)
    logits = torch.empty((B, Ld, V), dtype=torch.float32, device=dev) if with_logits else None
    nll = torch.empty((B, Ld), dtype=torch.float32, device=dev) if with_nll else None
    enc = torch.empty((B, S_enc, D), dtype=torch.float32, device=dev) if with_encoder else None
    return loss, logits, nll, enc


def _tiger_forward_result(loss, logits, nll, enc):
    return (loss,) + tuple(t for t in (logits, nll, enc) if t is not None)


def tiger_forward(binding, input_ids, attention_mask, labels, with_logits=True, with_nll=False, with_encoder=False):
    """``gr_tiger_forward_f32``: T5ForConditionalGeneration.forward with ``labels`` in eval mode (the call of
    the reference's ``eval_loss``) as one C call, nothing synchronises.  labels [B, Ld] int64, -100 = not counted.
    -> (loss 0-dim fp32[, logits [B, Ld, vocab]][, per-position NLL [B, Ld], 0 where not counted][, encoder
    output [B, S, d_model]])."""
    input_ids, attention_mask, labels, B, S, Ld = _tiger_forward_args("tiger_forward", input_ids, attention_mask, labels)
    tiger_check_config(binding.cfg, None, S, None)
    dev = input_ids.device
    loss, logits, nll, enc = _tiger_forward_outputs(B, S, Ld, binding.params.vocab, binding.params.d_model, dev,
                                                    with_logits, with_nll, with_encoder)
    if B == 0:          # an empty tensor has no address to pass: torch's mean over no element
        return _tiger_forward_result(loss.fill_(float("nan")), logits, nll, enc)
    nbytes = binding.forward_workspace_bytes(B, S, Ld)
    wsp = L.workspace(nbytes, dev)
    with L.on(dev):
        L.check(L.lib().gr_tiger_forward_f32(binding.ref, L.ptr(input_ids), L.ptr(attention_mask), L.ptr(labels), B, S,
                                             Ld, L.ptr(loss), L.ptr(logits), L.ptr(nll), L.ptr(enc), L.ptr(wsp), nbytes,
                                             L.stream_of(dev)), "gr_tiger_forward_f32")
    return _tiger_forward_result(loss, logits, nll, enc)


def tiger_forward_prefix(binding, input_ids, attention_mask, prof_lvl1, prof_lvl2, prof_lvl3, labels, with_logits=True,
                         with_nll=False, with_encoder=False):
    """``gr_tiger_forward_prefix_f32``: ``tiger_forward`` on the S + 3 encoder positions of ``tiger_generate_prefix``
    (the adapter launch first); the encoder output then is [B, S + 3, d_model]."""
    prof = [prof_lvl1, prof_lvl2, prof_lvl3]
    L.require_gpu(*prof)
    input_ids, attention_mask, labels, B, S, Ld = _tiger_forward_args("tiger_forward_prefix", input_ids, attention_mask,
                                                                      labels)
    n_vec = int(prof[0].shape[1]) if prof[0].dim() == 3 else -1
    for i, t in enumerate(prof):
        if t.dtype != torch.float32 or tuple(t.shape) != (B, n_vec, binding.bert_dim):
            raise RuntimeError(f"prof_lvl{i + 1} must be float32 [{B}, n_vec, {binding.bert_dim}], got {t.dtype} "
                               f"{tuple(t.shape)}")
    tiger_prefix_check(binding.cfg, binding.bert_dim, n_vec, S)
    tiger_check_config(binding.cfg, None, S + 3, None)
    prof = [t.contiguous() for t in prof]
    dev = input_ids.device
    loss, logits, nll, enc = _tiger_forward_outputs(B, S + 3, Ld, binding.t5.params.vocab, binding.t5.params.d_model,
                                                    dev, with_logits, with_nll, with_encoder)
    if B == 0:
        return _tiger_forward_result(loss.fill_(float("nan")), logits, nll, enc)
    nbytes = binding.forward_workspace_bytes(n_vec, B, S, Ld)
    wsp = L.workspace(nbytes, dev)
    with L.on(dev):
        L.check(L.lib().gr_tiger_forward_prefix_f32(
            binding.t5.ref, binding.ref(n_vec), L.ptr(input_ids), L.ptr(attention_mask), L.ptr(prof[0]), L.ptr(prof[1]),
            L.ptr(prof[2]), L.ptr(labels), B, S, Ld, L.ptr(loss), L.ptr(logits), L.ptr(nll), L.ptr(enc), L.ptr(wsp),
            nbytes, L.stream_of(dev)), "gr_tiger_forward_prefix_f32")
    return _tiger_forward_result(loss, logits, nll, enc)


def beam_hits(preds, labels, skip=0):
    """``calculate_pos_index`` (RQVAE-T5/utils.py:6-32) on the device: preds [B, k, T] int64 (the first
    ``skip`` tokens of each hypothesis dropped, the rest zero-padded or cut to the labels' width), labels
    [B, W] int64 -> bool [B, k] marking the first beam whose tokens equal the label row."""
    L.require_gpu(preds, labels)
    if preds.dim() != 3 or labels.dim() != 2 or preds.shape[0] != labels.shape[0]:
        raise RuntimeError(f"beam_hits takes preds [B, k, T] and labels [B, W], got {tuple(preds.shape)} and "
                           f"{tuple(labels.shape)}")
    if preds.dtype != torch.int64 or labels.dtype != torch.int64:
        raise TypeError("beam_hits takes int64 tokens")
    preds, labels = preds.contiguous(), labels.contiguous()
    B, k, T = preds.shape
    skip = int(skip)
    if not 0 <= skip <= T:
        raise ValueError(f"skip={skip} outside [0, {T}]")
    hits = torch.empty((B, k), dtype=torch.uint8, device=preds.device)
    with L.on(preds.device):
        L.check(L.lib().gr_beam_hits_i64(preds.data_ptr() + 8 * skip, B, k, T - skip, T, L.ptr(labels),
                                         labels.shape[1], L.ptr(hits), L.stream_of(preds.device)), "gr_beam_hits_i64")
    return hits.view(torch.bool)


T5E_LAYER_KEYS = TIGER_ENC_KEYS
T5E_ENVELOPE = ("d_model a multiple of 32 in [32, 512]; d_kv in {8, 16, 32, 64} with num_heads * d_kv <= 256; d_ff a "
                "multiple of 32 in [32, 1024]; input and target widths multiples of 4 in [4, 1024]; 1..8 blocks; "
                "32 relative-attention buckets; 1..32 positions; at most 2^20 users per call")


def t5_embed_check(cfg, S=None, B=None):
    """Raise NotImplementedError, naming the limit, for what gr_t5_embed_f32 does not cover.  ``cfg``: d_model,
    d_kv, num_heads, d_ff, num_layers, input_emb_dim, target_emb_dim (the widths of gr_t5_embed_params)."""
    def no(msg):
        raise NotImplementedError(f"T5 embedding retriever: {msg} (the gfx950 kernels cover: {T5E_ENVELOPE}); there is "
                                  "no CPU fallback")
    d, dkv, H, dff, nl, din, dout = (int(cfg[k]) for k in ("d_model", "d_kv", "num_heads", "d_ff", "num_layers",
                                                           "input_emb_dim", "target_emb_dim"))
    if cfg.get("feed_forward_proj", "relu") != "relu":
        no(f"feed_forward_proj={cfg['feed_forward_proj']!r} is not built, only 'relu'")
    if d < 32 or d > 512 or d % 32:
        no(f"d_model={d} must be a multiple of 32 in [32, 512]")
    if dkv not in (8, 16, 32, 64):
        no(f"d_kv={dkv} must be 8, 16, 32 or 64")
    if H < 1 or H * dkv > 256:
        no(f"num_heads * d_kv = {H * dkv} must be at most 256")
    if dff < 32 or dff > 1024 or dff % 32:
        no(f"d_ff={dff} must be a multiple of 32 in [32, 1024]")
    for name, v in (("input_emb_dim", din), ("target_emb_dim", dout)):
        if v < 4 or v > 1024 or v % 4:
            no(f"{name}={v} must be a multiple of 4 in [4, 1024]")
    if not 1 <= nl <= L.GR_T5E_MAX_LAYERS:
        no(f"num_layers={nl} must be 1..{L.GR_T5E_MAX_LAYERS}")
    if S is not None and not 1 <= S <= 32:
        no(f"a sequence of {S} positions; 1..32 are supported")
    if B is not None and B > (1 << 20):
        no(f"a batch of {B} users; at most 2^20 per call")


class T5EmbedBinding:
    """Device-pointer view of the retriever's parameters (``gr_t5_embed_params``).  ``tensors``: name -> tensor
    with the reference's names below ``TIGER`` (``input_proj.weight``, ``output_proj.bias``,
    ``model.encoder.block.0.layer.0.SelfAttention.q.weight``, ...).  The pointers are the tensors' own
    storage, so in-place weight updates are seen by the next call."""

    def __init__(self, cfg, tensors):
        t5_embed_check(cfg)
        self.cfg = cfg
        self.keep = []
        dev = tensors["input_proj.weight"].device
        self.device = dev
        p = L.T5EmbedParams()
        p.d_model, p.d_kv, p.n_heads, p.d_ff = (int(cfg[k]) for k in ("d_model", "d_kv", "num_heads", "d_ff"))
        p.n_layers, p.in_dim, p.out_dim = int(cfg["num_layers"]), int(cfg["input_emb_dim"]), int(cfg["target_emb_dim"])
        p.n_buckets = 32
        p.eps = float(cfg.get("layer_norm_epsilon", 1e-6))
        f = self._f
        p.in_w, p.in_b = f(tensors["input_proj.weight"]), f(tensors["input_proj.bias"])
        p.out_w, p.out_b = f(tensors["output_proj.weight"]), f(tensors["output_proj.bias"])
        p.rel = f(tensors[f"model.encoder.block.0.{TIGER_REL}.weight"])
        p.final_ln = f(tensors["model.encoder.final_layer_norm.weight"])
        for l in range(p.n_layers):
            for i, k in enumerate(T5E_LAYER_KEYS):
                p.layer[l][i] = f(tensors[f"model.encoder.block.{l}.{k}.weight"])
        self.bucket = t5_relative_bucket(torch.arange(-127, 128), True).to(torch.int32).to(dev)
        p.bucket = self.bucket.data_ptr()
        self.params = p
        self.ref = ctypes.byref(p)
        self._ws = {}

    def _f(self, t):
        L.require_gpu(t)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("the T5 embedding kernels take contiguous float32 parameters")
        self.keep.append(t)
        return t.data_ptr()

    def workspace_bytes(self, B, S):
        n = self._ws.get((B, S))
        if n is None:
            n = self._ws[(B, S)] = L.lib().gr_t5_embed_workspace_bytes(self.ref, B, S)
        return n


def t5_embed(binding, seq_embs, attention_mask=None, with_hidden=False):
    """``gr_t5_embed_f32``: input_proj, the T5 encoder stack, masked mean pooling, output_proj and the L2
    normalisation in one C call, nothing synchronises.  seq_embs [B, S, in_dim] fp32, attention_mask [B, S]
    (0 = not a key, not pooled; None: all live) -> pred [B, out_dim] unit rows[, hidden [B, S, d_model]: the
    final-norm states, unspecified where the mask is 0]."""
    L.require_gpu(seq_embs)
    p = binding.params
    if seq_embs.dim() != 3 or seq_embs.shape[-1] != p.in_dim:
        raise RuntimeError(f"t5_embed takes [B, S, {p.in_dim}] vectors, got {tuple(seq_embs.shape)}")
    seq_embs = L.as_f32(seq_embs)
    B, S, _ = seq_embs.shape
    t5_embed_check(binding.cfg, S, B)
    if attention_mask is not None:
        L.require_gpu(attention_mask)
        if tuple(attention_mask.shape) != (B, S):
            raise RuntimeError(f"attention_mask must be [{B}, {S}], got {tuple(attention_mask.shape)}")
        if attention_mask.dtype != torch.int64:
            attention_mask = attention_mask.to(torch.int64)
        attention_mask = attention_mask.contiguous()
    dev = seq_embs.device
    pred = torch.empty((B, p.out_dim), dtype=torch.float32, device=dev)
    hidden = torch.empty((B, S, p.d_model), dtype=torch.float32, device=dev) if with_hidden else None
    if B > 0:
        nbytes = binding.workspace_bytes(B, S)
        wsp = L.workspace(nbytes, dev)
        with L.on(dev):
            L.check(L.lib().gr_t5_embed_f32(binding.ref, L.ptr(seq_embs), L.ptr(attention_mask), B, S, L.ptr(pred),
                                            L.ptr(hidden), L.ptr(wsp), nbytes, L.stream_of(dev)), "gr_t5_embed_f32")
    return (pred, hidden) if with_hidden else pred


T5E_MAX_TABLE = 1 << 24


def t5_embed_project(binding, table):
    """``gr_t5_embed_project_f32``: input_proj over a whole table, once.  table [R, in_dim] fp32 (R 1..2^24) ->
    projected [R, d_model]: row r holds the bits ``t5_embed`` puts into x for that vector."""
    L.require_gpu(table)
    p = binding.params
    if table.dim() != 2 or table.shape[-1] != p.in_dim:
        raise RuntimeError(f"t5_embed_project takes a [R, {p.in_dim}] table, got {tuple(table.shape)}")
    R = table.shape[0]
    if not 1 <= R <= T5E_MAX_TABLE:
        raise NotImplementedError(f"T5 embedding retriever: a table of {R} rows; 1..2^24 are supported; there is no CPU "
                                  "fallback")
    table = L.as_f32(table)
    projected = torch.empty((R, p.d_model), dtype=torch.float32, device=table.device)
    with L.on(table.device):
        L.check(L.lib().gr_t5_embed_project_f32(binding.ref, L.ptr(table), R, L.ptr(projected),
                                                L.stream_of(table.device)), "gr_t5_embed_project_f32")
    return projected


def t5_embed_rows(binding, projected, tokens, offsets, with_hidden=False):
    """``gr_t5_embed_rows_f32``: the encoder on packed live rows, one C call, nothing synchronises.  projected
    [R, d_model] from ``t5_embed_project``; tokens [rows] int64 rows of it, user after user; offsets [B + 1] int64,
    user b is tokens[offsets[b]:offsets[b + 1]] (1..32 of them) -> pred [B, out_dim] unit rows[, hidden [rows,
    d_model]]: the bits ``t5_embed`` gives for the same sequences right-padded.  The values of tokens and offsets
    are not read on the host: a user with a token outside the table or with bad offsets gets a NaN row."""
    L.require_gpu(projected, tokens, offsets)
    p = binding.params
    if projected.dim() != 2 or projected.shape[-1] != p.d_model:
        raise RuntimeError(f"t5_embed_rows takes a projected [R, {p.d_model}] table, got {tuple(projected.shape)}")
    projected = L.as_f32(projected)
    if tokens.dim() != 1 or offsets.dim() != 1 or offsets.shape[0] < 1:
        raise RuntimeError(f"t5_embed_rows takes tokens [rows] and offsets [B + 1], got {tuple(tokens.shape)} and "
                           f"{tuple(offsets.shape)}")
    if tokens.dtype != torch.int64 or offsets.dtype != torch.int64:
        raise TypeError(f"tokens and offsets must be int64, got {tokens.dtype} and {offsets.dtype}")
    tokens, offsets = tokens.contiguous(), offsets.contiguous()
    R, rows, B = projected.shape[0], tokens.shape[0], offsets.shape[0] - 1
    t5_embed_check(binding.cfg, None, B)
    if not B <= rows <= 32 * B:
        raise NotImplementedError(f"T5 embedding retriever: {rows} rows for {B} users; every user has 1..32 rows; there is "
                                  "no CPU fallback")
    if B > 0 and not 1 <= R <= T5E_MAX_TABLE:
        raise NotImplementedError(f"T5 embedding retriever: a table of {R} rows; 1..2^24 are supported; there is no CPU "
                                  "fallback")
    dev = projected.device
    pred = torch.empty((B, p.out_dim), dtype=torch.float32, device=dev)
    hidden = torch.empty((rows, p.d_model), dtype=torch.float32, device=dev) if with_hidden else None
    if B > 0:
        nbytes = L.lib().gr_t5_embed_rows_workspace_bytes(binding.ref, B, rows)
        wsp = L.workspace(nbytes, dev)
        with L.on(dev):
            L.check(L.lib().gr_t5_embed_rows_f32(binding.ref, L.ptr(projected), R, L.ptr(tokens), L.ptr(offsets), B, rows,
                                                 L.ptr(pred), L.ptr(hidden), L.ptr(wsp), nbytes, L.stream_of(dev)),
                    "gr_t5_embed_rows_f32")
    return (pred, hidden) if with_hidden else pred


BERT_LAYER_KEYS = ("attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight",
                   "attention.self.key.bias", "attention.self.value.weight", "attention.self.value.bias",
                   "attention.output.dense.weight", "attention.output.dense.bias",
                   "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias",
                   "intermediate.dense.weight", "intermediate.dense.bias", "output.dense.weight", "output.dense.bias",
                   "output.LayerNorm.weight", "output.LayerNorm.bias")
BERT_MAX_B = 1 << 16
BERT_ENVELOPE = ("hidden_size a multiple of 32 up to 1024, = num_attention_heads * head width with the head width 32 "
                 "or 64; intermediate_size a multiple of 32 up to 4096; 1..24 layers; hidden_act 'gelu'; absolute "
                 "positions; 1..min(512, max_position_embeddings) positions; at most 65536 sequences per call")
BERT_POOLINGS = {None: L.GR_BERT_POOL_NONE, "none": L.GR_BERT_POOL_NONE, "mean_no_cls": L.GR_BERT_POOL_MEAN_NO_CLS,
                 "cls": L.GR_BERT_POOL_CLS}


def bert_check(cfg, S=None, B=None):
    """Raise NotImplementedError, naming the field, for what gr_bert_embed_f32 does not cover.  ``cfg``: HF's
    ``BertConfig`` field names."""
    def no(msg):
        raise NotImplementedError(f"BERT encoder: {msg} (the gfx950 kernels cover: {BERT_ENVELOPE}); there is no CPU "
                                  "fallback")
    H, nh, I, nl = (int(cfg[k]) for k in ("hidden_size", "num_attention_heads", "intermediate_size",
                                          "num_hidden_layers"))
    if cfg.get("hidden_act", "gelu") != "gelu":
        no(f"hidden_act={cfg['hidden_act']!r} is not built, only 'gelu'")
    if cfg.get("position_embedding_type", "absolute") not in (None, "absolute"):
        no(f"position_embedding_type={cfg['position_embedding_type']!r} is not built, only 'absolute'")
    if H < 32 or H > 1024 or H % 32:
        no(f"hidden_size={H} must be a multiple of 32 in [32, 1024]")
    if nh < 1 or H % nh or H // nh not in (32, 64):
        no(f"num_attention_heads={nh} must split hidden_size={H} into heads of 32 or 64")
    if I < 32 or I > 4096 or I % 32:
        no(f"intermediate_size={I} must be a multiple of 32 in [32, 4096]")
    if not 1 <= nl <= L.GR_BERT_MAX_LAYERS:
        no(f"num_hidden_layers={nl} must be 1..{L.GR_BERT_MAX_LAYERS}")
    for k in ("vocab_size", "type_vocab_size", "max_position_embeddings"):
        if int(cfg[k]) < 1:
            no(f"{k}={cfg[k]} must be positive")
    top = min(512, int(cfg["max_position_embeddings"]))
    if S is not None and not 1 <= S <= top:
        no(f"a sequence of {S} positions; 1..{top} are supported (max_position_embeddings="
           f"{cfg['max_position_embeddings']})")
    if B is not None and B > BERT_MAX_B:
        no(f"a batch of {B} sequences; at most {BERT_MAX_B} per call")


class BertBinding:
    """Device-pointer view of a BERT encoder's parameters (``gr_bert_params``).  ``tensors``: name -> tensor with
    ``BertModel``'s names (``embeddings.word_embeddings.weight``, ``encoder.layer.0.attention.self.query.weight``,
    ...; the pooler is not read).  The pointers are the tensors' own storage, so in-place weight updates are
    seen by the next call."""
    ENTRY, WS_QUERY = "gr_bert_embed_f32", "gr_bert_embed_workspace_bytes"
    RAGGED_ENTRY, RAGGED_WS_QUERY = "gr_bert_embed_ragged_f32", "gr_bert_embed_ragged_workspace_bytes"

    def __init__(self, cfg, tensors):
        bert_check(cfg)
        self.cfg = cfg
        self.keep = []
        self.device = tensors["embeddings.word_embeddings.weight"].device
        H, nh, I = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["intermediate_size"])
        p = L.BertParams()
        p.vocab_size, p.hidden_size, p.num_heads, p.head_dim = int(cfg["vocab_size"]), H, nh, H // nh
        p.intermediate_size, p.num_layers = I, int(cfg["num_hidden_layers"])
        p.max_position, p.type_vocab_size = int(cfg["max_position_embeddings"]), int(cfg["type_vocab_size"])
        p.hidden_act = p.position_type = 0
        p.eps = float(cfg.get("layer_norm_eps", 1e-12))
        f = self._f
        e = "embeddings."
        p.word = f(tensors[e + "word_embeddings.weight"], (p.vocab_size, H))
        p.position = f(tensors[e + "position_embeddings.weight"], (p.max_position, H))
        p.token_type = f(tensors[e + "token_type_embeddings.weight"], (p.type_vocab_size, H))
        p.emb_ln_w, p.emb_ln_b = f(tensors[e + "LayerNorm.weight"], (H,)), f(tensors[e + "LayerNorm.bias"], (H,))
        shapes = {"intermediate.dense.weight": (I, H), "intermediate.dense.bias": (I,), "output.dense.weight": (H, I)}
        for k in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"):
            shapes[k + ".weight"] = (H, H)
        for l in range(p.num_layers):
            for i, k in enumerate(BERT_LAYER_KEYS):
                p.layer[l][i] = f(tensors[f"encoder.layer.{l}.{k}"], shapes.get(k, (H,)), f"encoder.layer.{l}.{k}")
        self.params = p
        self.ref = ctypes.byref(p)
        self._ws = {}

    def _f(self, t, shape, name="an embedding parameter"):
        L.require_gpu(t)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("the BERT kernels take contiguous float32 parameters")
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
        if t.device != self.device:
            raise RuntimeError("the BERT parameters must be on one device")
        self.keep.append(t)
        return t.data_ptr()

    def workspace_bytes(self, B, S):
        n = self._ws.get((B, S))
        if n is None:
            n = self._ws[(B, S)] = getattr(L.lib(), self.WS_QUERY)(self.ref, B, S)
        return n

    def ragged_workspace_bytes(self, B, S, rows_bound):
        n = self._ws.get((B, S, rows_bound))
        if n is None:
            n = self._ws[(B, S, rows_bound)] = getattr(L.lib(), self.RAGGED_WS_QUERY)(self.ref, B, S, rows_bound)
        return n


class BertBf16Binding(BertBinding):
    """``gr_bert_bf16_params``: the bf16 precision of the same encoder (bf16 GEMM operands, fp32 accumulation and
    epilogues; the contract is in include/gr_amd.h).  ``tensors``: the float32 tensors ``BertBinding`` takes.  The six
    matrices per layer are rounded once, here, with ``tensor.to(torch.bfloat16)`` (round-to-nearest-even) and kept
    alive by the binding: it is a SNAPSHOT of them, so a later in-place change to a matrix is not seen until a new
    binding is made (``BertEncoder.binding_bf16`` does that).  Tables, biases and LayerNorm parameters stay the
    tensors' own float32 storage.  ``ops.bert_embed`` and ``ops.bert_embed_ragged`` take it in ``BertBinding``'s
    place and call ``gr_bert_embed_bf16`` / ``gr_bert_embed_ragged_bf16``."""
    ENTRY, WS_QUERY = "gr_bert_embed_bf16", "gr_bert_embed_bf16_workspace_bytes"
    RAGGED_ENTRY, RAGGED_WS_QUERY = "gr_bert_embed_ragged_bf16", "gr_bert_embed_ragged_bf16_workspace_bytes"
    MATRICES = tuple(i for i, k in enumerate(BERT_LAYER_KEYS) if k.endswith(".weight") and "LayerNorm" not in k)

    def __init__(self, cfg, tensors):
        super().__init__(cfg, tensors)
        f32 = self.params
        p = L.BertBf16Params()
        for name, _ in L.BertParams._fields_[:-1]:
            setattr(p, name, getattr(f32, name))
        vectors = [i for i in range(len(BERT_LAYER_KEYS)) if i not in self.MATRICES]
        for l in range(p.num_layers):
            for j, i in enumerate(self.MATRICES):
                m = tensors[f"encoder.layer.{l}.{BERT_LAYER_KEYS[i]}"].to(torch.bfloat16).contiguous()
                self.keep.append(m)
                p.matrix[l][j] = m.data_ptr()
            for j, i in enumerate(vectors):
                p.vector[l][j] = f32.layer[l][i]
        self.params = p
        self.ref = ctypes.byref(p)


def _bert_ids(name, t, B, S):
    L.require_gpu(t)
    if tuple(t.shape) != (B, S):
        raise RuntimeError(f"{name} must be [{B}, {S}], got {tuple(t.shape)}")
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    return t.contiguous()


def _bert_args(fn, binding, input_ids, attention_mask, token_type_ids, pooling):
    """What ``bert_embed`` and ``bert_embed_ragged`` (``fn``: the one named in the shape message) open with -> the
    checked [B, S] int64 tensors, the pooling mode and ``pooled`` [B, H] (None without pooling)."""
    if pooling not in BERT_POOLINGS:
        raise ValueError(f"pooling={pooling!r} must be 'mean_no_cls', 'cls' or None")
    mode = BERT_POOLINGS[pooling]
    if input_ids.dim() != 2:
        raise RuntimeError(f"{fn} takes [B, S] token ids, got {tuple(input_ids.shape)}")
    B, S = input_ids.shape
    input_ids = _bert_ids("input_ids", input_ids, B, S)
    bert_check(binding.cfg, S, B)
    if attention_mask is not None:
        attention_mask = _bert_ids("attention_mask", attention_mask, B, S)
    if token_type_ids is not None:
        token_type_ids = _bert_ids("token_type_ids", token_type_ids, B, S)
    pooled = None
    if mode != L.GR_BERT_POOL_NONE:
        pooled = torch.empty((B, binding.params.hidden_size), dtype=torch.float32, device=input_ids.device)
    return input_ids, attention_mask, token_type_ids, mode, pooled


def bert_embed(binding, input_ids, attention_mask=None, token_type_ids=None, pooling="mean_no_cls", with_hidden=False):
    """``gr_bert_embed_f32``: embeddings, the encoder stack and the pooling in one C call, nothing synchronises.
    The binding's type picks the precision: a ``BertBf16Binding`` calls ``gr_bert_embed_bf16`` (the outputs are
    float32 either way).
    input_ids [B, S]; attention_mask [B, S] (0 = not a key, not pooled; None: all live); token_type_ids [B, S] or
    None (zeros).  pooling "mean_no_cls" (the live rows after position 0, 0 when there is none), "cls" (row 0) or
    None -> pooled [B, H][, hidden [B, S, H] with ``with_hidden``], or hidden alone when pooling is None.  A
    sequence with no live key gives zeros."""
    input_ids, attention_mask, token_type_ids, mode, pooled = _bert_args("bert_embed", binding, input_ids, attention_mask,
                                                                         token_type_ids, pooling)
    (B, S), dev, H = input_ids.shape, input_ids.device, binding.params.hidden_size
    want_hidden = with_hidden or pooled is None
    hidden = torch.empty((B, S, H), dtype=torch.float32, device=dev) if want_hidden else None
    if B > 0:
        nbytes = binding.workspace_bytes(B, S)
        wsp = L.workspace(nbytes, dev)
        with L.on(dev):
            L.check(getattr(L.lib(), binding.ENTRY)(binding.ref, L.ptr(input_ids), L.ptr(attention_mask),
                                                    L.ptr(token_type_ids), B, S, mode, L.ptr(pooled), L.ptr(hidden),
                                                    L.ptr(wsp), nbytes, L.stream_of(dev)), binding.ENTRY)
    if pooled is None:
        return hidden
    return (pooled, hidden) if with_hidden else pooled


def bert_embed_ragged(binding, input_ids, attention_mask=None, token_type_ids=None, pooling="mean_no_cls", rows_bound=None,
                      with_hidden=False):
    """``gr_bert_embed_ragged_f32``: ``bert_embed`` over rows ``[0, len_b)`` of each sequence only (``len_b``: one past
    its last live position), packed; the pooled vectors and the kept rows have ``bert_embed``'s bits (a
    ``BertBf16Binding`` calls ``gr_bert_embed_ragged_bf16``: the bits of ``bert_embed`` on that binding).  ``rows_bound``:
    an upper bound on the packed row count ``sum(len_b)`` -- ``bert_embed.row_bound`` gives it for a host-side mask;
    None means B * S, which is always safe; 0 (no sequence has a live key) is passed on as 1.  Nothing synchronises: the row count stays on the device, and a bound
    below it shows as NaN in every pooled element and -1 in the last offset.
    -> pooled [B, H], or with ``with_hidden`` (pooled, hidden_rows [rows_bound, H], row_offsets [B + 1] int64):
    ``hidden_rows[row_offsets[b] + s]`` is position s of sequence b, rows from ``row_offsets[B]`` on are unset.
    ``pooling=None`` returns (hidden_rows, row_offsets)."""
    input_ids, attention_mask, token_type_ids, mode, pooled = _bert_args("bert_embed_ragged", binding, input_ids,
                                                                         attention_mask, token_type_ids, pooling)
    (B, S), dev, H = input_ids.shape, input_ids.device, binding.params.hidden_size
    if rows_bound is not None and int(rows_bound) < 0:
        raise ValueError(f"rows_bound={rows_bound} must not be negative")
    rows = B * S if rows_bound is None else max(min(int(rows_bound), B * S), min(B, 1))   # the C entry takes >= 1
    want_hidden = with_hidden or pooled is None
    hidden = torch.empty((rows, H), dtype=torch.float32, device=dev) if want_hidden else None
    offsets = torch.zeros((B + 1,), dtype=torch.int64, device=dev) if want_hidden else None
    if B > 0:
        nbytes = binding.ragged_workspace_bytes(B, S, rows)
        wsp = L.workspace(nbytes, dev)
        with L.on(dev):
            L.check(getattr(L.lib(), binding.RAGGED_ENTRY)(binding.ref, L.ptr(input_ids), L.ptr(attention_mask),
                                                           L.ptr(token_type_ids), B, S, rows, mode, L.ptr(pooled),
                                                           L.ptr(hidden), L.ptr(offsets), L.ptr(wsp), nbytes,
                                                           L.stream_of(dev)), binding.RAGGED_ENTRY)
    if pooled is None:
        return hidden, offsets
    return (pooled, hidden, offsets) if with_hidden else pooled
