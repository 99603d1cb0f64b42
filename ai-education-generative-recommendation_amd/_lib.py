"""ctypes binding of libgr_amd.so (the C ABI declared in include/gr_amd.h).

The library is built in-tree by ``build.py`` (``__graft_entry__.build()``).  There is no CPU or
PyTorch fallback: if the library is missing, or a tensor is not on a ROCm device, the call raises.
"""
import ctypes
import os

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# GR_AMD_LIB: another in-tree build of the same ABI (A/B variants from scripts/build_variant.sh)
LIB_PATH = os.environ.get("GR_AMD_LIB") or os.path.join(_PKG, "lib", "libgr_amd.so")

GR_ACT_NONE = 0
GR_ACT_RELU = 1
GR_ACT_SIGMOID = 2
GR_ACT_TANH = 3
GR_ACT_LEAKYRELU = 4
GR_MAX_LEVELS = 8
GR_MAX_LINEAR = 8
# bits of gr_sasrec_plan's mask
GR_SAS_FUSED, GR_SAS_ROWTILE, GR_SAS_LAYERWISE = 0x1, 0x2, 0x4
GR_SAS_FUSED_TWO_WAVES, GR_SAS_FUSED_MISALIGNED = 0x8, 0x10
GR_SAS_B0_EMBED_PROJ, GR_SAS_B0_EMBED_LN_LINEAR, GR_SAS_B0_EMBED_LN = 0x20, 0x40, 0x80
GR_SAS_ATTN_SCALAR, GR_SAS_ATTN_MFMA, GR_SAS_ATTN_PERSIST, GR_SAS_ATTN_K16 = 0x100, 0x200, 0x400, 0x800
GR_SAS_ATTN_LAST_TILE, GR_SAS_TAIL, GR_SAS_TAIL_VALU, GR_SAS_PRUNED = 0x1000, 0x2000, 0x4000, 0x8000

_c_int_p = ctypes.POINTER(ctypes.c_int32)
_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_i32 = ctypes.c_int32
_sz = ctypes.c_size_t
_f32 = ctypes.c_float


class SasrecParams(ctypes.Structure):
    """Mirror of ``gr_sasrec_params`` (include/gr_amd.h)."""
    _fields_ = [("d", _i32), ("n_blocks", _i32), ("n_heads", _i32), ("mlp", _i32),
                ("max_len", _i32), ("eps", _f32), ("item_rows", _i64),
                ("item_emb", _vp), ("pos_emb", _vp),
                ("attn_ln_w", _vp), ("attn_ln_b", _vp), ("in_proj_w", _vp), ("in_proj_b", _vp),
                ("out_proj_w", _vp), ("out_proj_b", _vp), ("ffn_ln_w", _vp), ("ffn_ln_b", _vp),
                ("ffn1_w", _vp), ("ffn1_b", _vp), ("ffn2_w", _vp), ("ffn2_b", _vp),
                ("last_ln_w", _vp), ("last_ln_b", _vp)]


class SasrecTrainBufs(ctypes.Structure):
    """Mirror of ``gr_sasrec_train_bufs`` (include/gr_amd.h)."""
    _fields_ = [(f, _vp) for f in ("xin", "hs", "qkv", "prob", "os", "x1", "fs", "zs", "us", "xl", "g_vec")]


GR_TIGER_MAX_LAYERS = 4


class TigerParams(ctypes.Structure):
    """Mirror of ``gr_tiger_params`` (include/gr_amd.h)."""
    _fields_ = [(f, _i32) for f in ("vocab", "d_model", "d_kv", "n_heads", "d_ff", "n_enc", "n_dec", "n_buckets",
                                    "pad_id", "eos_id", "fill_id", "reserved")] + \
               [("eps", _f32), ("lm_scale", _f32)] + \
               [(f, _vp) for f in ("shared", "lm_head", "enc_rel", "dec_rel", "enc_final_ln", "dec_final_ln",
                                   "enc_bucket", "dec_bucket")] + \
               [("enc", (_vp * 8) * GR_TIGER_MAX_LAYERS), ("dec", (_vp * 13) * GR_TIGER_MAX_LAYERS)]


class TigerPrefixParams(ctypes.Structure):
    """Mirror of ``gr_tiger_prefix_params`` (include/gr_amd.h)."""
    _fields_ = [(f, _i32) for f in ("bert_dim", "n_vec", "n_heads", "reserved")] + \
               [("eps", _f32), ("reserved_f", _f32), ("adapter", (_vp * 14) * 3)]


GR_T5E_MAX_LAYERS = 8


class T5EmbedParams(ctypes.Structure):
    """Mirror of ``gr_t5_embed_params`` (include/gr_amd.h)."""
    _fields_ = [(f, _i32) for f in ("d_model", "d_kv", "n_heads", "d_ff", "n_layers", "in_dim", "out_dim",
                                    "n_buckets")] + \
               [("eps", _f32), ("reserved", _f32)] + \
               [(f, _vp) for f in ("in_w", "in_b", "out_w", "out_b", "rel", "bucket", "final_ln")] + \
               [("layer", (_vp * 8) * GR_T5E_MAX_LAYERS)]


GR_BERT_MAX_LAYERS = 24
GR_BERT_POOL_NONE, GR_BERT_POOL_MEAN_NO_CLS, GR_BERT_POOL_CLS = 0, 1, 2


class BertParams(ctypes.Structure):
    """Mirror of ``gr_bert_params`` (include/gr_amd.h)."""
    _fields_ = [(f, _i32) for f in ("vocab_size", "hidden_size", "num_heads", "head_dim", "intermediate_size",
                                    "num_layers", "max_position", "type_vocab_size", "hidden_act", "position_type")] + \
               [("eps", _f32), ("reserved", _f32)] + \
               [(f, _vp) for f in ("word", "position", "token_type", "emb_ln_w", "emb_ln_b")] + \
               [("layer", (_vp * 16) * GR_BERT_MAX_LAYERS)]


class BertBf16Params(ctypes.Structure):
    """Mirror of ``gr_bert_bf16_params`` (include/gr_amd.h): ``matrix`` bf16, everything else fp32."""
    _fields_ = BertParams._fields_[:-1] + [("matrix", (_vp * 6) * GR_BERT_MAX_LAYERS),
                                           ("vector", (_vp * 10) * GR_BERT_MAX_LAYERS)]


# (name, restype, argtypes) for every entry point of include/gr_amd.h
SIGNATURES = {
    "gr_version": (ctypes.c_char_p, []),
    "gr_last_error": (ctypes.c_char_p, []),
    "gr_set_option": (ctypes.c_int, [ctypes.c_char_p, _i64]),
    "gr_get_option": (_i64, [ctypes.c_char_p]),
    "gr_linear_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _i64, _i32, _vp, _i64, _vp]),
    "gr_rq_codebook_norms_f32": (ctypes.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "gr_rq_quantize_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gr_rq_encode_workspace_bytes": (_sz, [_i64, _i32, _vp, _i32, _vp]),
    "gr_rq_encode_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _sz, _vp]),
    "gr_rq_encoder_pack_floats": (_sz, [_i32, _vp]),
    "gr_rq_encoder_pack_f32": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp]),
    "gr_rq_encode_packed_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                               _vp, _vp, _vp, _vp, _sz, _vp]),
    "gr_rq_codebook_image_floats": (_sz, [_i32, _i32, _vp]),
    "gr_rq_codebook_pack_f32": (ctypes.c_int, [_i32, _i32, _vp, _vp, _vp, _vp]),
    "gr_rq_encode_image_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp,
                                              _vp, _vp, _vp, _vp, _sz, _vp]),
    "gr_rq_mlp_workspace_bytes": (_sz, [_i64, _i32, _vp]),
    "gr_rq_mlp_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gr_mlp_exact_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i32,
                                        _vp, _vp, _sz, _vp]),
    "gr_mlp_exact_groups_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32,
                                               _i32, _vp, _i64, _vp, _vp]),
    "gr_mkl_plan": (_i32, [_i64, _i32, _i32, _c_int_p, _c_int_p]),
    "gr_rq_filter_bound_f32": (_f32, [_f32, _f32]),
    "gr_rq_filter_launches": (_i64, []),
    "gr_rq_filter_diag_counts": (None, [_vp]),
    "gr_rq_leftover_launches": (_i64, []),
    "gr_rq_filter_plan": (ctypes.c_int, [_i64, _i32, _i32, _vp, _vp, _vp]),
    "gr_rq_encode_sk_workspace_bytes": (_sz, [_i64, _i32, _i32, _vp]),
    "gr_rq_encode_sk_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i64,
                                           _vp, _vp, _sz, _vp]),
    "gr_mlp_train_fwd_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp]),
    "gr_mlp_train_bwd_layer_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _i32, _f32, _vp, _i32,
                                                  _vp, _vp, _vp, _vp]),
    "gr_rq_quantize_sk_train_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i64,
                                                   _vp, _vp, _vp, _vp, _sz, _vp]),
    "gr_rq_quantize_sk_train_bwd_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _f32,
                                                       _vp, _vp, _vp]),
    "gr_sasrec_workspace_bytes": (_sz, [ctypes.POINTER(SasrecParams), _i64, _i32]),
    "gr_sasrec_forward_f32": (ctypes.c_int, [ctypes.POINTER(SasrecParams), _vp, _i64, _i32, _vp,
                                             _i32, _vp, _sz, _vp, _vp]),
    "gr_sasrec_predict_f32": (ctypes.c_int, [ctypes.POINTER(SasrecParams), _vp, _i64, _i32, _vp,
                                             _vp, _sz, _vp, _vp]),
    "gr_sasrec_predict_ld_f32": (ctypes.c_int, [ctypes.POINTER(SasrecParams), _vp, _i64, _i32, _vp,
                                                _i64, _vp, _sz, _vp, _vp]),
    "gr_sasrec_rank_workspace_bytes": (_sz, [ctypes.POINTER(SasrecParams), _i64, _i32]),
    "gr_sasrec_rank_f32": (ctypes.c_int, [ctypes.POINTER(SasrecParams), _vp, _i64, _i32, _vp, _i32, _vp, _vp,
                                          _sz, _vp, _sz, _vp, _vp]),
    "gr_sasrec_plan": (_i32, [ctypes.POINTER(SasrecParams), _i64, _i32, _i32]),
    "gr_sasrec_train_vec_width": (_i32, [ctypes.POINTER(SasrecParams), _i32]),
    "gr_sasrec_train_fwd_f32": (ctypes.c_int, [ctypes.POINTER(SasrecParams), _vp, _i64, _i32, _f32,
                                               ctypes.c_uint64, _vp, ctypes.POINTER(SasrecTrainBufs), _vp,
                                               _vp, _vp]),
    "gr_sasrec_train_bwd_f32": (ctypes.c_int, [ctypes.POINTER(SasrecParams), _vp, _i64, _i32, _f32,
                                               ctypes.c_uint64, _vp, ctypes.POINTER(SasrecTrainBufs), _vp,
                                               _vp, _vp]),
    "gr_sasrec_train_tiled_workspace_bytes": (_sz, [ctypes.POINTER(SasrecParams), _i64, _i32]),
    "gr_sasrec_train_tiled_parts": (_i32, [ctypes.POINTER(SasrecParams), _i64, _i32]),
    "gr_sasrec_train_tiled_fwd_f32": (ctypes.c_int, [ctypes.POINTER(SasrecParams), _vp, _i64, _i32, _f32,
                                                     ctypes.c_uint64, _vp, ctypes.POINTER(SasrecTrainBufs), _vp,
                                                     _vp, _vp, _sz, _vp]),
    "gr_sasrec_train_tiled_bwd_f32": (ctypes.c_int, [ctypes.POINTER(SasrecParams), _vp, _i64, _i32, _f32,
                                                     ctypes.c_uint64, _vp, ctypes.POINTER(SasrecTrainBufs), _vp,
                                                     _vp, _vp, _sz, _vp]),
    "gr_score_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp]),
    "gr_sampled_bce_fwd_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _i32, _f32,
                                              _vp, _vp, _vp, _vp, _vp]),
    "gr_neg_samples": (ctypes.c_int, [_vp, _i64, _i32, _i64, _i32, ctypes.c_uint64, _vp, _vp, _vp]),
    "gr_neg_samples_dseed": (ctypes.c_int, [_vp, _i64, _i32, _i64, _i32, ctypes.c_uint64, _vp, _vp, _vp, _vp]),
    "gr_sampled_bce_bwd_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _i32, _vp,
                                              _vp, _vp, _vp, _vp]),
    "gr_rank_f32": (ctypes.c_int, [_vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp]),
    "gr_count_gt_f32": (ctypes.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "gr_topk_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "gr_topk_f32": (ctypes.c_int, [_vp, _i64, _i64, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gr_score_pairs_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i64, _vp, _i32, _vp, _vp, _vp]),
    "gr_score_count_gt_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i64, _vp, _i32, _vp, _vp]),
    "gr_score_count_workspace_bytes": (_sz, [_i64]),
    "gr_score_count_gt_ws_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i64, _vp, _i32, _vp, _vp, _sz, _vp]),
    "gr_merge_topk_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp]),
    "gr_merge_topk_packed": (ctypes.c_int, [_vp, _i32, _i64, _i32, _i32, _vp, _vp, _vp]),
    "gr_score_topk_workspace_bytes": (_sz, [_i64, _i32, _i64, _i32]),
    "gr_score_topk_f32": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp,
                                         _vp, _vp, _sz, _vp]),
    "gr_code_groups_workspace_bytes": (_sz, [_i64, _i32]),
    "gr_code_groups_i64": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gr_code_segments_i64": (ctypes.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gr_kmeans_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "gr_kmeans_form": (_i32, [_i64, _i32, _i32]),
    "gr_kmeans_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, ctypes.c_uint64, _i32, _i32, ctypes.c_double,
                                     _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gr_tiger_workspace_bytes": (_sz, [ctypes.POINTER(TigerParams), _i64, _i32, _i32, _i32]),
    "gr_tiger_generate_f32": (ctypes.c_int, [ctypes.POINTER(TigerParams), _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp,
                                             _vp, _vp, _vp, _sz, _vp]),
    "gr_tiger_prefix_workspace_bytes": (_sz, [ctypes.POINTER(TigerParams), ctypes.POINTER(TigerPrefixParams), _i64,
                                              _i32, _i32, _i32]),
    "gr_tiger_generate_prefix_f32": (ctypes.c_int, [ctypes.POINTER(TigerParams), ctypes.POINTER(TigerPrefixParams),
                                                    _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp,
                                                    _vp, _vp, _vp, _sz, _vp]),
    "gr_tiger_forward_workspace_bytes": (_sz, [ctypes.POINTER(TigerParams), _i64, _i32, _i32]),
    "gr_tiger_forward_f32": (ctypes.c_int, [ctypes.POINTER(TigerParams), _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp,
                                            _vp, _vp, _sz, _vp]),
    "gr_tiger_forward_prefix_workspace_bytes": (_sz, [ctypes.POINTER(TigerParams), ctypes.POINTER(TigerPrefixParams),
                                                      _i64, _i32, _i32]),
    "gr_tiger_forward_prefix_f32": (ctypes.c_int, [ctypes.POINTER(TigerParams), ctypes.POINTER(TigerPrefixParams),
                                                   _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp,
                                                   _vp, _sz, _vp]),
    "gr_beam_hits_i64": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i64, _vp, _i32, _vp, _vp]),
    "gr_t5_embed_workspace_bytes": (_sz, [ctypes.POINTER(T5EmbedParams), _i64, _i32]),
    "gr_t5_embed_f32": (ctypes.c_int, [ctypes.POINTER(T5EmbedParams), _vp, _vp, _i64, _i32, _vp, _vp, _vp, _sz, _vp]),
    "gr_t5_embed_project_f32": (ctypes.c_int, [ctypes.POINTER(T5EmbedParams), _vp, _i64, _vp, _vp]),
    "gr_t5_embed_rows_workspace_bytes": (_sz, [ctypes.POINTER(T5EmbedParams), _i64, _i64]),
    "gr_t5_embed_rows_f32": (ctypes.c_int, [ctypes.POINTER(T5EmbedParams), _vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp,
                                            _vp, _sz, _vp]),
    "gr_bert_embed_workspace_bytes": (_sz, [ctypes.POINTER(BertParams), _i64, _i32]),
    "gr_bert_embed_f32": (ctypes.c_int, [ctypes.POINTER(BertParams), _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp,
                                         _sz, _vp]),
    "gr_bert_embed_ragged_workspace_bytes": (_sz, [ctypes.POINTER(BertParams), _i64, _i32, _i64]),
    "gr_bert_embed_ragged_f32": (ctypes.c_int, [ctypes.POINTER(BertParams), _vp, _vp, _vp, _i64, _i32, _i64, _i32, _vp,
                                                _vp, _vp, _vp, _sz, _vp]),
    "gr_bert_embed_bf16_workspace_bytes": (_sz, [ctypes.POINTER(BertBf16Params), _i64, _i32]),
    "gr_bert_embed_bf16": (ctypes.c_int, [ctypes.POINTER(BertBf16Params), _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp,
                                          _sz, _vp]),
    "gr_bert_embed_ragged_bf16_workspace_bytes": (_sz, [ctypes.POINTER(BertBf16Params), _i64, _i32, _i64]),
    "gr_bert_embed_ragged_bf16": (ctypes.c_int, [ctypes.POINTER(BertBf16Params), _vp, _vp, _vp, _i64, _i32, _i64, _i32,
                                                 _vp, _vp, _vp, _vp, _sz, _vp]),
}

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if the library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"gr_amd: {LIB_PATH} is missing - run __graft_entry__.build() "
                               "(there is no CPU fallback)")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().gr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def require_gpu(*tensors):
    """The product path runs only on a ROCm device: refuse CPU tensors loudly."""
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("gr_amd kernels run on a ROCm GPU only (tensor on "
                               f"{t.device}); there is no CPU fallback")


def ptr(t):
    """Device address of ``t`` as a plain int (the argtypes convert it; None: NULL)."""
    return t.data_ptr() if t is not None else None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(device):
    """Handle of ``device``'s current stream (int) -- the stream every call enqueues on."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if _raw_stream is not None:
        return _raw_stream(idx)
    return torch.cuda.current_stream(idx).cuda_stream


class _NoGuard:
    __slots__ = ()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def on(device):
    """Device guard for a launch on ``device``: a no-op when it is already the current device (the
    common case; torch.cuda.device's set / restore costs microseconds per call at the reference's
    batch sizes), torch.cuda.device otherwise."""
    if device.index is None or device.index == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(device)


def ptr_array(tensors):
    """Host array of device pointers (``const float* const*``)."""
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def i32_array(values):
    return (ctypes.c_int32 * len(values))(*values)


def workspace(nbytes, device):
    """Caller-owned scratch from the PyTorch caching allocator (the library never allocates)."""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def as_f32(t):
    """Contiguous fp32 view (the kernels are fp32 end to end, like the reference)."""
    if t.dtype != torch.float32:
        raise TypeError(f"gr_amd kernels take float32 tensors, got {t.dtype}")
    return t.contiguous()


# Counts set_option calls: a switch can change what a shape needs (sas_fused: a [B, d] workspace or the
# layer-wise buffers), so sizes cached per shape (ops.SasrecBinding) are dropped when it moves.
OPTION_EPOCH = 0


def set_option(name, value):
    """gr_set_option (include/gr_amd.h): process-wide path / tuning switches."""
    global OPTION_EPOCH
    check(lib().gr_set_option(name.encode(), int(value)), "gr_set_option")
    OPTION_EPOCH += 1


def get_option(name):
    return int(lib().gr_get_option(name.encode()))
