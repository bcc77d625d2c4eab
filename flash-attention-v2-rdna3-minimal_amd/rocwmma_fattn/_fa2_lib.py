"""ctypes binding of libfa2_gfx950.so — the C-ABI declared in include/fa2_gfx950.h.

There is deliberately NO fallback: if the shared library is missing and cannot be built, or a call is
made with tensors that are not on a ROCm device, this module raises.  (The CPU restatement under
oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes
import importlib.util
import os

# PyTorch-ROCm must be loaded first: it brings its own libamdhip64.so.7, and the kernel library has
# to bind to that SAME runtime instance (it is handed torch's streams and device pointers).  Loading
# libfa2_gfx950.so before torch would pull in the system runtime under the same soname instead.
import torch  # noqa: F401

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
LIB_PATH = os.path.join(_PKG_DIR, "libfa2_gfx950.so")
_OVERRIDE = os.environ.get("FA2_GFX950_LIB")      # developer A/B: load this build of the library instead (never built here)

FA2_DTYPE_F16 = 0
FA2_DTYPE_BF16 = 1
FA2_DTYPE_F32 = 2                                  # the rotary tables of fa2_kvcache_append only
FA2_CACHE_16BIT, FA2_CACHE_E4M3 = 0, 1             # cache_format of fa2_kvcache_append
FA2_BIAS_NONE, FA2_BIAS_IO_DTYPE, FA2_BIAS_F32, FA2_BIAS_BOOL = 0, 1, 2, 3     # bias_kind of fa2_fwd_bias

FA2_KERNEL_HIP_256, FA2_KERNEL_HIP_128, FA2_KERNEL_ASM, FA2_KERNEL_HIP_BIAS = 1, 2, 3, 4              # fa2_fwd_plan_t.kernel
FA2_KERNEL_HIP_WINDOW = 5                                                                               # ... of fa2_fwd_window_plan (an enumerator in the header)
FA2_KERNEL_HIP_VARLEN = 6                                                                               # ... of fa2_fwd_varlen_plan (an enumerator, too)
FA2_KERNEL_HIP_VARLEN_DV = 10                                                                           # ... of fa2_fwd_varlen_dv_plan (an enumerator, too)
FA2_CONTRACT_PRESCALE_Q, FA2_CONTRACT_LSUM_P16 = 1, 2                                                 # fa2_fwd_plan_t.contract bits

_i64p = ctypes.POINTER(ctypes.c_int64)
_vpp = ctypes.POINTER(ctypes.c_void_p)      # a host array of device pointers (fa2_merge_*)


class FwdPlan(ctypes.Structure):
    """fa2_fwd_plan_t (include/fa2_gfx950.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("kernel", "contract", "rows", "heads_main", "kernel_tail", "contract_tail", "rows_tail",
                                             "nsplit", "split_items")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BwdPlan(ctypes.Structure):
    """fa2_bwd_plan_t (include/fa2_gfx950.h)."""
    _fields_ = [("dq_kernel", ctypes.c_int), ("dkv_kernel", ctypes.c_int)]


class DecodePlan(ctypes.Structure):
    """fa2_decode_plan_t (include/fa2_gfx950.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("kernel", "nsplit", "row_tiles", "key_tile")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DecodeMlaPlan(ctypes.Structure):
    """fa2_decode_mla_plan_t (include/fa2_gfx950.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("kernel", "nsplit", "row_blocks", "key_tile", "max_split")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


FA2_KERNEL_HIP_DECODE_MLA = 9                                                                           # fa2_decode_mla_plan_t.kernel (an enumerator in the header)
FA2_KERNEL_HIP_PREFILL = 8                                                                              # fa2_fwd_prefill_plan's kernel (an enumerator in the header)
FA2_KERNEL_HIP_DECODE = 7                                                                               # fa2_decode_plan_t.kernel (an enumerator in the header)
FA2_BWD_KERNEL_HIP, FA2_BWD_KERNEL_ASM, FA2_BWD_KERNEL_SHORT = 1, 2, 3                                  # fa2_bwd_plan_t.dq_kernel / .dkv_kernel
FA2_BIAS_FORM_SCALAR, FA2_BIAS_FORM_VEC4, FA2_BIAS_FORM_TILE, FA2_BIAS_FORM_TILE_DMA, FA2_BIAS_FORM_ROW = 0, 1, 2, 3, 4     # fa2_fwd_bias_form


_FWD_ARGTYPES = [
    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,  # q k v o lse
    ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,                  # B H Nq Nkv D
    _i64p, _i64p, _i64p, _i64p, _i64p,                                                     # strides
    ctypes.c_float, ctypes.c_int, ctypes.c_void_p,                                         # scale causal stream
]

_FWD_BIAS_ARGTYPES = [ctypes.c_int] + _FWD_ARGTYPES[:-1] + [ctypes.c_void_p, ctypes.c_int, _i64p, ctypes.c_void_p]  # ... bias kind strides stream

_BWD_ARGTYPES = [ctypes.c_void_p] * 10 + [ctypes.c_int] * 5 + [_i64p] * 9 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p]

# every symbol include/fa2_gfx950.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "fa2_bwd_f16": (ctypes.c_int, _BWD_ARGTYPES),
    "fa2_bwd_bf16": (ctypes.c_int, _BWD_ARGTYPES),
    "fa2_bwd": (ctypes.c_int, [ctypes.c_int] + _BWD_ARGTYPES),
    "fa2_fwd_f16": (ctypes.c_int, _FWD_ARGTYPES),
    "fa2_fwd_bf16": (ctypes.c_int, _FWD_ARGTYPES),
    "fa2_fwd": (ctypes.c_int, [ctypes.c_int] + _FWD_ARGTYPES),
    "fa2_fwd_bias": (ctypes.c_int, _FWD_BIAS_ARGTYPES),
    "fa2_fwd_ws": (ctypes.c_int, [ctypes.c_int] + _FWD_ARGTYPES[:-1] + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),   # ... workspace bytes stream
    "fa2_fwd_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 7),
    "fa2_bwd_ws": (ctypes.c_int, [ctypes.c_int] + _BWD_ARGTYPES[:-1] + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "fa2_bwd_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 7),
    "fa2_bwd_bias": (ctypes.c_int, [ctypes.c_int] + _BWD_ARGTYPES[:-1] + [ctypes.c_void_p, ctypes.c_int, _i64p, ctypes.c_void_p]),
    "fa2_bwd_bias_ws": (ctypes.c_int, [ctypes.c_int] + _BWD_ARGTYPES[:-1] + [ctypes.c_void_p, ctypes.c_int, _i64p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "fa2_bwd_bias_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 7),
    "fa2_supported_head_dims": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "fa2_padded_head_dim": (ctypes.c_int, [ctypes.c_int]),
    "fa2_tile_rows": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "fa2_fwd_prescales_q": (ctypes.c_int, [ctypes.c_int, ctypes.c_float]),
    "fa2_fwd_plan": (ctypes.c_int, [ctypes.c_int] * 6 + [_i64p, _i64p, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(FwdPlan)]),
    "fa2_bwd_plan": (ctypes.c_int, [ctypes.c_int] * 7 + [_i64p] * 5 + [ctypes.c_float, ctypes.c_int, ctypes.c_int, _i64p, ctypes.POINTER(BwdPlan)]),
    "fa2_fwd_bias_form": (ctypes.c_int, [ctypes.c_int] * 6 + [_i64p]),
    # grouped-query / multi-query attention: the MHA argument lists with Hkv after H (fa2_fwd_gqa: fa2_fwd_ws's, fa2_bwd_gqa: fa2_bwd_ws's)
    "fa2_fwd_gqa": (ctypes.c_int, [ctypes.c_int] + _FWD_ARGTYPES[:7] + [ctypes.c_int] + _FWD_ARGTYPES[7:-1] + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "fa2_fwd_gqa_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 8),
    "fa2_fwd_gqa_plan": (ctypes.c_int, [ctypes.c_int] * 7 + [_i64p, _i64p, ctypes.c_float, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(FwdPlan)]),
    "fa2_bwd_gqa": (ctypes.c_int, [ctypes.c_int] + _BWD_ARGTYPES[:12] + [ctypes.c_int] + _BWD_ARGTYPES[12:-1] + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "fa2_bwd_gqa_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 8),
    # sliding-window attention: fa2_fwd_gqa's / fa2_bwd's argument lists with (window_left, window_right, q_offset) in place of the workspace / before the stream
    "fa2_fwd_window": (ctypes.c_int, [ctypes.c_int] + _FWD_ARGTYPES[:7] + [ctypes.c_int] + _FWD_ARGTYPES[7:-1] + [ctypes.c_int] * 3 + [ctypes.c_void_p]),
    "fa2_bwd_window": (ctypes.c_int, [ctypes.c_int] + _BWD_ARGTYPES[:-1] + [ctypes.c_int] * 3 + [ctypes.c_void_p]),
    "fa2_fwd_window_plan": (ctypes.c_int, [ctypes.c_int] * 7 + [_i64p, _i64p, ctypes.c_float] + [ctypes.c_int] * 4 + [ctypes.c_size_t, ctypes.POINTER(FwdPlan)]),
    "fa2_window_tile_range": (ctypes.c_int, [ctypes.c_int] * 9 + [ctypes.POINTER(ctypes.c_int)] * 2),
    "fa2_window_row_range": (ctypes.c_int, [ctypes.c_int] * 9 + [ctypes.POINTER(ctypes.c_int)] * 2),
    # packed (variable-length) attention: [total, heads, D] tensors with {head, row} strides, cu_seqlens in device memory, the stated maximum lengths
    "fa2_fwd_varlen": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2 + [_i64p] * 4 +
                       [ctypes.c_int64, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.c_void_p]),
    "fa2_bwd_varlen": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2 + [_i64p] * 8 +
                       [ctypes.c_int64, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.c_void_p]),
    "fa2_fwd_varlen_plan": (ctypes.c_int, [ctypes.c_int] * 7 + [_i64p, _i64p, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.POINTER(FwdPlan)]),
    # ... with v / o of head dim Dv < D (the non-absorbed MLA prefill): fa2_fwd_varlen's / fa2_fwd_varlen_plan's lists with Dv after D
    "fa2_fwd_varlen_dv": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 7 + [ctypes.c_void_p] * 2 + [_i64p] * 4 +
                          [ctypes.c_int64, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.c_void_p]),
    "fa2_fwd_varlen_dv_plan": (ctypes.c_int, [ctypes.c_int] * 8 + [_i64p, _i64p, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.POINTER(FwdPlan)]),
    "fa2_varlen_tile_range": (ctypes.c_int, [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_int)] * 2),
    "fa2_varlen_row_range": (ctypes.c_int, [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_int)] * 2),
    # attention dropout: the windowed / packed argument lists, then (float dropout_p, uint64_t seed); and the host side of the mask contract
    "fa2_fwd_dropout": (ctypes.c_int, [ctypes.c_int] + _FWD_ARGTYPES[:7] + [ctypes.c_int] + _FWD_ARGTYPES[7:-1] + [ctypes.c_int] * 3 + [ctypes.c_void_p] +
                        [ctypes.c_float, ctypes.c_uint64]),
    "fa2_bwd_dropout": (ctypes.c_int, [ctypes.c_int] + _BWD_ARGTYPES[:-1] + [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_float, ctypes.c_uint64]),
    "fa2_fwd_varlen_dropout": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2 + [_i64p] * 4 +
                               [ctypes.c_int64, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_float, ctypes.c_uint64]),
    "fa2_bwd_varlen_dropout": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2 + [_i64p] * 8 +
                               [ctypes.c_int64, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_float, ctypes.c_uint64]),
    # score modifiers (logit soft-capping, ALiBi slopes): the windowed / packed argument lists, then (float softcap, const float* alibi_slopes, int64_t stride)
    "fa2_fwd_scoremod": (ctypes.c_int, [ctypes.c_int] + _FWD_ARGTYPES[:7] + [ctypes.c_int] + _FWD_ARGTYPES[7:-1] + [ctypes.c_int] * 3 + [ctypes.c_void_p] +
                         [ctypes.c_float, ctypes.c_void_p, ctypes.c_int64]),
    "fa2_bwd_scoremod": (ctypes.c_int, [ctypes.c_int] + _BWD_ARGTYPES[:-1] + [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_float, ctypes.c_void_p, ctypes.c_int64]),
    "fa2_fwd_varlen_scoremod": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2 + [_i64p] * 4 +
                                [ctypes.c_int64, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_float, ctypes.c_void_p, ctypes.c_int64]),
    "fa2_bwd_varlen_scoremod": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2 + [_i64p] * 8 +
                                [ctypes.c_int64, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_float, ctypes.c_void_p, ctypes.c_int64]),
    # a gradient for the LSE: a family's backward argument list, then (for the windowed / packed ones) dropout_p, seed, softcap, slopes, stride, then dlse and its strides
    "fa2_bwd_lse": (ctypes.c_int, [ctypes.c_int] + _BWD_ARGTYPES[:-1] + [ctypes.c_void_p, ctypes.c_int, _i64p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p] +
                    [ctypes.c_void_p, _i64p]),
    "fa2_bwd_window_lse": (ctypes.c_int, [ctypes.c_int] + _BWD_ARGTYPES[:-1] + [ctypes.c_int] * 3 + [ctypes.c_void_p] +
                           [ctypes.c_float, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _i64p]),
    "fa2_bwd_varlen_lse": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2 + [_i64p] * 8 +
                           [ctypes.c_int64, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.c_void_p] +
                           [ctypes.c_float, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]),
    "fa2_bwd_lse_plan": (ctypes.c_int, [ctypes.c_int] * 7 + [_i64p] * 5 + [ctypes.c_float, ctypes.c_int, ctypes.c_int, _i64p, ctypes.c_int, ctypes.POINTER(BwdPlan)]),
    # merge of partial attention results: host arrays of device pointers, shared stride sets
    "fa2_merge_fwd": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vpp, _vpp, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [_i64p] * 4 +
                      [ctypes.c_int, ctypes.c_void_p]),
    "fa2_merge_bwd": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vpp, _vpp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _vpp, _vpp] + [ctypes.c_int] * 4 +
                      [_i64p] * 7 + [ctypes.c_int, ctypes.c_void_p]),
    # KV-cache decode attention: q k_cache v_cache o lse cache_seqlens block_table, B H Hkv Nq D capacity page_size num_pages, four stride triples, the lse
    # pair, the block-table row stride, scale, num_splits, workspace, bytes, stream
    "fa2_fwd_decode": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 7 + [ctypes.c_int] * 8 + [_i64p] * 5 +
                       [ctypes.c_int64, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "fa2_fwd_decode_plan": (ctypes.c_int, [ctypes.c_int] * 9 + [ctypes.POINTER(DecodePlan)]),
    "fa2_fwd_decode_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 9),
    "fa2_decode_part_range": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int)] * 2),
    # ... on e4m3 caches: the same list with k_descale v_descale descale_strides after scale
    "fa2_fwd_decode_fp8": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 7 + [ctypes.c_int] * 8 + [_i64p] * 5 +
                           [ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, _i64p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                            ctypes.c_void_p]),
    "fa2_fwd_decode_fp8_plan": (ctypes.c_int, [ctypes.c_int] * 9 + [ctypes.POINTER(DecodePlan)]),
    "fa2_fwd_decode_fp8_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 9),
    # ... with a sliding window, soft-capping and ALiBi slopes: cache_format after dtype, fa2_fwd_decode_fp8's list up to descale_strides, then
    # window_left softcap alibi_slopes alibi_stride, then num_splits workspace bytes stream; the queries take window_left last (before the plan)
    "fa2_fwd_decode_window": (ctypes.c_int, [ctypes.c_int] * 2 + [ctypes.c_void_p] * 7 + [ctypes.c_int] * 8 + [_i64p] * 5 +
                              [ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, _i64p, ctypes.c_int, ctypes.c_float, ctypes.c_void_p,
                               ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "fa2_fwd_decode_window_plan": (ctypes.c_int, [ctypes.c_int] * 10 + [ctypes.POINTER(DecodePlan)]),
    "fa2_fwd_decode_window_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 10),
    "fa2_decode_window_part_range": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)] * 2),
    # decode on a latent (MLA) cache: q kv_cache o lse cache_seqlens block_table, B H Nq D Dv capacity page_size num_pages, the q kv o stride triples, the
    # lse pair, the block-table row stride, scale, num_splits, workspace, bytes, stream
    "fa2_fwd_decode_mla": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_int] * 8 + [_i64p] * 4 +
                           [ctypes.c_int64, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "fa2_fwd_decode_mla_plan": (ctypes.c_int, [ctypes.c_int] * 9 + [ctypes.POINTER(DecodeMlaPlan)]),
    "fa2_fwd_decode_mla_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 9),
    "fa2_decode_mla_part_range": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 2),
    "fa2_decode_mla_tile": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)] * 3),
    # KV-cache append: dtype cache_format, k_new v_new k_cache v_cache cache_seqlens block_table, B Hkv Nnew D capacity page_size num_pages, four stride
    # triples, the block-table row stride, q q_out H Nq and their stride triples, cos sin rotary_dtype rotary_dim seqlen_ro row-stride interleaved,
    # k_descale v_descale descale_strides, stream
    "fa2_kvcache_append": (ctypes.c_int, [ctypes.c_int] * 2 + [ctypes.c_void_p] * 6 + [ctypes.c_int] * 7 + [_i64p] * 4 + [ctypes.c_int64] +
                           [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [_i64p] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_int64, ctypes.c_int] +
                           [ctypes.c_void_p] * 2 + [_i64p, ctypes.c_void_p]),
    # chunked prefill against a KV cache: dtype cache_format, q k_cache v_cache o lse cu_seqlens_q cache_seqlens block_table, B H Hkv max_seqlen_q D capacity
    # page_size num_pages, q k v o strides, the lse and block-table row strides, scale, window_left, softcap slopes slope-stride, stream
    "fa2_fwd_prefill": (ctypes.c_int, [ctypes.c_int] * 2 + [ctypes.c_void_p] * 8 + [ctypes.c_int] * 8 + [_i64p] * 4 + [ctypes.c_int64] * 2 +
                        [ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "fa2_fwd_prefill_plan": (ctypes.c_int, [ctypes.c_int] * 8 + [ctypes.POINTER(FwdPlan)]),
    # ... on e4m3 caches: no cache_format, k_descale v_descale descale_strides after scale
    "fa2_fwd_prefill_fp8": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 8 + [ctypes.c_int] * 8 + [_i64p] * 4 + [ctypes.c_int64] * 2 +
                            [ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, _i64p, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64,
                             ctypes.c_void_p]),
    "fa2_fwd_prefill_fp8_plan": (ctypes.c_int, [ctypes.c_int] * 8 + [ctypes.POINTER(FwdPlan)]),
    "fa2_prefill_tile": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)] * 3),
    "fa2_kvappend_slot": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    # ... packed (ragged): cu_seqlens before cache_seqlens, B total(int64) Hkv D capacity page_size num_pages, stride PAIRS {head, row} for k_new v_new q
    # q_out, no Nq; the rest as above
    "fa2_kvcache_append_varlen": (ctypes.c_int, [ctypes.c_int] * 2 + [ctypes.c_void_p] * 7 + [ctypes.c_int, ctypes.c_int64] + [ctypes.c_int] * 5 + [_i64p] * 4 +
                                  [ctypes.c_int64] + [ctypes.c_void_p] * 2 + [ctypes.c_int] + [_i64p] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 +
                                  [ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 2 + [_i64p, ctypes.c_void_p]),
    "fa2_kvappend_varlen_token": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int64] + [ctypes.POINTER(ctypes.c_int)] * 3),
    # the append for a latent (MLA) cache: dtype, kv_c k_pe kv_cache cache_seqlens block_table, B Nnew D Dv capacity page_size num_pages, the kv_c / k_pe
    # stride pairs and the cache's triple, the block-table row stride, q q_out H Nq and their triples, cos sin rotary_dtype rotary_dim seqlen_ro row-stride
    # interleaved, stream
    "fa2_kvcache_append_mla": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 7 + [_i64p] * 3 + [ctypes.c_int64] +
                               [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [_i64p] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 +
                               [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    # ... packed: cu_seqlens before cache_seqlens, B total(int64) D Dv ..., one row stride each for kv_c / k_pe, {head, row} pairs for q / q_out, no Nq
    "fa2_kvcache_append_mla_varlen": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_int64] + [ctypes.c_int] * 5 + [_i64p] * 3 +
                                      [ctypes.c_int64] + [ctypes.c_void_p] * 2 + [ctypes.c_int] + [_i64p] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 +
                                      [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "fa2_kvappend_mla_chunks": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 2),
    "fa2_rotary_eval": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)] + [ctypes.c_int] * 3 +
                        [ctypes.c_void_p]),
    "fa2_scoremod_eval": (ctypes.c_int, [ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(ctypes.c_float)] * 2),
    "fa2_dropout_keep_mask": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]),
    "fa2_dropout_threshold": (ctypes.c_int, [ctypes.c_float, ctypes.POINTER(ctypes.c_float)]),
    "fa2_philox4x32_10": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint32)] * 3),
    "fa2_set_option": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "fa2_get_option": (ctypes.c_int, [ctypes.c_char_p]),
    "fa2_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fa2_version": (ctypes.c_char_p, []),
}

_lib = None
WS_CACHE = {}        # FlashAttn.py: shape -> workspace bytes, valid for the current option values (dropped whenever an option is set here)


def _build_module():
    spec = importlib.util.spec_from_file_location("_fa2_build", os.path.join(_PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load(build_if_missing=True):
    """dlopen the in-tree library (building it with hipcc first when absent) and type its symbols."""
    global _lib
    if _lib is not None:
        return _lib
    # build() compiles only when the library is missing or older than its sources (stamp = digest of sources + flags),
    # so a stale .so is never used silently after a kernel edit.
    if _OVERRIDE:
        lib_path = _OVERRIDE
    elif build_if_missing:
        lib_path = _build_module().build()
    else:
        lib_path = LIB_PATH
    if not os.path.exists(lib_path):
        raise RuntimeError("fa2: %s is missing; run `python %s`" % (LIB_PATH, os.path.join(_PKG_DIR, "build.py")))
    lib = ctypes.CDLL(lib_path)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def error_string(code):
    return load().fa2_error_string(int(code)).decode()


def check(code):
    if code != 0:
        raise RuntimeError("fa2 call failed (%d): %s" % (code, error_string(code)))


def set_option(name, value):
    """fa2_set_option, and forget what was planned under the old value."""
    check(load().fa2_set_option(name.encode(), int(value)))
    WS_CACHE.clear()


class options:
    """with _fa2_lib.options(rows=256, persist=0): ... — set tuning switches of the library (fa2_set_option) and restore
    them on exit.  Process-wide: for A/B measurements and tests, not for concurrent use."""

    def __init__(self, **kw):
        self.kw = kw
        self.saved = {}

    def __enter__(self):
        lib = load()
        for k, v in self.kw.items():
            old = lib.fa2_get_option(k.encode())
            if old < 0:
                raise ValueError("fa2: unknown option %r" % k)
            self.saved[k] = old
            check(lib.fa2_set_option(k.encode(), int(v)))
        WS_CACHE.clear()
        return self

    def __exit__(self, *exc):
        lib = load()
        for k, v in self.saved.items():
            lib.fa2_set_option(k.encode(), v)
        WS_CACHE.clear()
        return False


FA2_FLAG_CAUSAL, FA2_FLAG_EXACT_SCALE = 1, 2       # bits of the `causal` argument (include/fa2_gfx950.h)
FA2_MERGE_NATURAL_LSE = 1                          # `flags` of fa2_merge_fwd / fa2_merge_bwd (an enumerator in the header)
FA2_FLAG_BOTTOM_RIGHT = 4                          # ... of the packed (varlen) entry points' `flags` only


def call_flags(causal):
    """The `causal` argument of the C-ABI from what a caller of the operator passed: a bool (the reference's argument), or the flags themselves —
    bit 1, FA2_FLAG_EXACT_SCALE, marks the forward of a call that will be differentiated."""
    if isinstance(causal, bool) or causal is None:
        return FA2_FLAG_CAUSAL if causal else 0
    c = int(causal)
    if c & ~(FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE):
        raise ValueError("fa2: `causal` is a bool or the flag word FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE (0 .. 3), got %r" % (causal,))
    return c


def fwd_plan(q, k, causal, scale=None, bias_kind=FA2_BIAS_NONE, workspace_bytes=0):
    """fa2_fwd_plan for the call fa2_fwd*(q, k, ...) would be: which kernel(s) serve it and under which numerical contract.  `causal`: bool, or the
    call's flags (FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE)."""
    B, H, Nq, D = q.shape
    dt = FA2_DTYPE_F16 if q.dtype == torch.float16 else FA2_DTYPE_BF16
    plan = FwdPlan()
    check(load().fa2_fwd_plan(dt, B, H, Nq, k.shape[2], D, strides3(q.stride(0), q.stride(1), q.stride(2)),
                              strides3(k.stride(0), k.stride(1), k.stride(2)), float(D ** -0.5 if scale is None else scale),
                              call_flags(causal), int(bias_kind), int(workspace_bytes), ctypes.byref(plan)))
    return plan


def gqa_plan(q, k, causal, scale=None, workspace_bytes=0):
    """fa2_fwd_gqa_plan for the call fa2_fwd_gqa(q, k, ...) would be (k: [B, Hkv, Nkv, D])."""
    B, H, Nq, D = q.shape
    dt = FA2_DTYPE_F16 if q.dtype == torch.float16 else FA2_DTYPE_BF16
    plan = FwdPlan()
    check(load().fa2_fwd_gqa_plan(dt, B, H, k.shape[1], Nq, k.shape[2], D, strides3(q.stride(0), q.stride(1), q.stride(2)),
                                  strides3(k.stride(0), k.stride(1), k.stride(2)), float(D ** -0.5 if scale is None else scale),
                                  call_flags(causal), int(workspace_bytes), ctypes.byref(plan)))
    return plan


WINDOW_MESSAGE = "fa2: window is None, an int W (= (W, W)) or (left, right), each -1 / None (unbounded) or >= 0, and q_offset is an int >= 0"


def parse_window(window, q_offset=0):
    """The operator's `window` / `q_offset` arguments -> (window_left, window_right, q_offset) of the C-ABI, -1 = unbounded.  Bad values raise
    ValueError(WINDOW_MESSAGE) — the compiled front end refuses them with the same text."""
    def one(x):
        if x is None:
            return -1
        if isinstance(x, bool) or not isinstance(x, int) or x < -1 or x >= 2 ** 31:
            raise ValueError(WINDOW_MESSAGE + ", got window=%r q_offset=%r" % (window, q_offset))
        return x
    if window is None:
        left = right = -1
    elif isinstance(window, (tuple, list)):
        if len(window) != 2:
            raise ValueError(WINDOW_MESSAGE + ", got window=%r q_offset=%r" % (window, q_offset))
        left, right = one(window[0]), one(window[1])
    else:
        left = right = one(window)
        if left < 0:                                  # (-1 is spelled None or (-1, -1))
            raise ValueError(WINDOW_MESSAGE + ", got window=%r q_offset=%r" % (window, q_offset))
    if isinstance(q_offset, bool) or not isinstance(q_offset, int) or q_offset < 0 or q_offset >= 2 ** 31:
        raise ValueError(WINDOW_MESSAGE + ", got window=%r q_offset=%r" % (window, q_offset))
    return left, right, q_offset


def window_plan(q, k, causal, window_left, window_right, q_offset, scale=None, workspace_bytes=0):
    """fa2_fwd_window_plan for the call fa2_fwd_window(q, k, ...) would be (k: [B, Hkv, Nkv, D])."""
    B, H, Nq, D = q.shape
    dt = FA2_DTYPE_F16 if q.dtype == torch.float16 else FA2_DTYPE_BF16
    plan = FwdPlan()
    check(load().fa2_fwd_window_plan(dt, B, H, k.shape[1], Nq, k.shape[2], D, strides3(q.stride(0), q.stride(1), q.stride(2)),
                                     strides3(k.stride(0), k.stride(1), k.stride(2)), float(D ** -0.5 if scale is None else scale),
                                     call_flags(causal), int(window_left), int(window_right), int(q_offset), int(workspace_bytes), ctypes.byref(plan)))
    return plan


def window_tile_range(Nq, Nkv, window_left, window_right, q_offset, causal, row0, rows, tile=64, transpose=False):
    """fa2_window_tile_range (transpose: fa2_window_row_range, row0 / rows then name a block of keys) -> (first_tile, ntiles)."""
    first, n = ctypes.c_int(), ctypes.c_int()
    fn = load().fa2_window_row_range if transpose else load().fa2_window_tile_range
    check(fn(int(Nq), int(Nkv), int(window_left), int(window_right), int(q_offset), int(bool(causal)), int(row0), int(rows), int(tile),
             ctypes.byref(first), ctypes.byref(n)))
    return first.value, n.value


def varlen_plan(q, k, max_seqlen_q, max_seqlen_k, B, flags=0, window_left=-1, window_right=-1, scale=None):
    """fa2_fwd_varlen_plan for the call fa2_fwd_varlen(q, k, ...) would be (q: [total_q, H, D], k: [total_k, Hkv, D], B sequences; flags: FA2_FLAG_*)."""
    _, H, D = q.shape
    dt = FA2_DTYPE_F16 if q.dtype == torch.float16 else FA2_DTYPE_BF16
    plan = FwdPlan()
    check(load().fa2_fwd_varlen_plan(dt, int(B), H, k.shape[1], int(max_seqlen_q), int(max_seqlen_k), D, strides2(q.stride(1), q.stride(0)),
                                     strides2(k.stride(1), k.stride(0)), float(D ** -0.5 if scale is None else scale), int(flags),
                                     int(window_left), int(window_right), ctypes.byref(plan)))
    return plan


def varlen_tile_range(Nq_s, Nkv_s, window_left, window_right, flags, row0, rows, tile=64, transpose=False):
    """fa2_varlen_tile_range (transpose: fa2_varlen_row_range, row0 / rows then name a block of keys) -> (first_tile, ntiles)."""
    first, n = ctypes.c_int(), ctypes.c_int()
    fn = load().fa2_varlen_row_range if transpose else load().fa2_varlen_tile_range
    check(fn(int(Nq_s), int(Nkv_s), int(window_left), int(window_right), int(flags), int(row0), int(rows), int(tile), ctypes.byref(first), ctypes.byref(n)))
    return first.value, n.value


def decode_plan(dtype, B, H, Hkv, Nq, D, capacity, page_size=0, num_splits=0):
    """fa2_fwd_decode_plan: the split, the row tiles per K / V head, the key tile and the kernel of a decode call (dtype: an FA2_DTYPE_* code)."""
    plan = DecodePlan()
    check(load().fa2_fwd_decode_plan(int(dtype), int(B), int(H), int(Hkv), int(Nq), int(D), int(capacity), int(page_size), int(num_splits), ctypes.byref(plan)))
    return plan


def decode_fp8_plan(dtype, B, H, Hkv, Nq, D, capacity, page_size=0, num_splits=0):
    """fa2_fwd_decode_fp8_plan: the plan of the call on e4m3 caches (dtype: the FA2_DTYPE_* code of q and o)."""
    plan = DecodePlan()
    check(load().fa2_fwd_decode_fp8_plan(int(dtype), int(B), int(H), int(Hkv), int(Nq), int(D), int(capacity), int(page_size), int(num_splits),
                                         ctypes.byref(plan)))
    return plan


def decode_part_range(length, capacity_keys, Nq, tile, nsplit, part):
    """fa2_decode_part_range -> (first_tile, ntiles): the key tiles part `part` of `nsplit` sweeps for a sequence of `length` keys."""
    first, n = ctypes.c_int(), ctypes.c_int()
    check(load().fa2_decode_part_range(int(length), int(capacity_keys), int(Nq), int(tile), int(nsplit), int(part), ctypes.byref(first), ctypes.byref(n)))
    return first.value, n.value


def decode_window_plan(dtype, B, H, Hkv, Nq, D, capacity, page_size=0, num_splits=0, window_left=-1):
    """fa2_fwd_decode_window_plan: the plan of a decode call with a sliding window of `window_left` keys (-1: none; the 16-bit and e4m3 caches share it)."""
    plan = DecodePlan()
    check(load().fa2_fwd_decode_window_plan(int(dtype), int(B), int(H), int(Hkv), int(Nq), int(D), int(capacity), int(page_size), int(num_splits),
                                            int(window_left), ctypes.byref(plan)))
    return plan


def decode_window_part_range(length, capacity_keys, Nq, window_left, tile, nsplit, part):
    """fa2_decode_window_part_range -> (first_tile, ntiles): the key tiles part `part` of `nsplit` sweeps under a window of `window_left` keys."""
    first, n = ctypes.c_int(), ctypes.c_int()
    check(load().fa2_decode_window_part_range(int(length), int(capacity_keys), int(Nq), int(window_left), int(tile), int(nsplit), int(part),
                                              ctypes.byref(first), ctypes.byref(n)))
    return first.value, n.value


def decode_mla_plan(dtype, B, H, Nq, capacity, page_size=0, num_splits=0, D=576, Dv=512):
    """fa2_fwd_decode_mla_plan: the split, the row blocks, the key tile, the split cap and the kernel of a latent-cache decode call."""
    plan = DecodeMlaPlan()
    check(load().fa2_fwd_decode_mla_plan(int(dtype), int(B), int(H), int(Nq), int(D), int(Dv), int(capacity), int(page_size), int(num_splits), ctypes.byref(plan)))
    return plan


def decode_mla_part_range(length, capacity_keys, nsplit, part):
    """fa2_decode_mla_part_range -> (first_tile, ntiles): the 32-key tiles part `part` of `nsplit` sweeps for a sequence of `length` keys."""
    first, n = ctypes.c_int(), ctypes.c_int()
    check(load().fa2_decode_mla_part_range(int(length), int(capacity_keys), int(nsplit), int(part), ctypes.byref(first), ctypes.byref(n)))
    return first.value, n.value


def decode_mla_tile(length, capacity, page_size, tile):
    """fa2_decode_mla_tile -> (page_slot, row_in_page, valid_rows) of 32-key tile `tile` of a sequence of `length` keys (capacity: key slots, or
    block-table entries per sequence when page_size > 0)."""
    slot, row, rows = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(load().fa2_decode_mla_tile(int(length), int(capacity), int(page_size), int(tile), ctypes.byref(slot), ctypes.byref(row), ctypes.byref(rows)))
    return slot.value, row.value, rows.value


def kvappend_slot(length, capacity_keys, Nnew, i):
    """fa2_kvappend_slot -> the key position new token `i` of `Nnew` is written at for a sequence of `length` keys after the append, or -1 (skipped)."""
    pos = ctypes.c_int64()
    check(load().fa2_kvappend_slot(int(length), int(capacity_keys), int(Nnew), int(i), ctypes.byref(pos)))
    return pos.value


def kvappend_varlen_token(cu_seqlens, t):
    """fa2_kvappend_varlen_token on a host sequence of B + 1 ints -> (seq, i, nnew) of packed token `t`, or None when no sequence owns it."""
    cu = (ctypes.c_int * len(cu_seqlens))(*[int(c) for c in cu_seqlens])
    seq, i, nnew = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(load().fa2_kvappend_varlen_token(cu, len(cu_seqlens) - 1, int(t), ctypes.byref(seq), ctypes.byref(i), ctypes.byref(nnew)))
    return None if seq.value < 0 else (seq.value, i.value, nnew.value)


def prefill_plan(dtype, B, H, Hkv, max_seqlen_q, D, capacity, page_size=0):
    """fa2_fwd_prefill_plan: the kernel, the contract and the rows per workgroup of a prefill call (dtype: an FA2_DTYPE_* code)."""
    plan = FwdPlan()
    check(load().fa2_fwd_prefill_plan(int(dtype), int(B), int(H), int(Hkv), int(max_seqlen_q), int(D), int(capacity), int(page_size), ctypes.byref(plan)))
    return plan.as_dict()


def prefill_fp8_plan(dtype, B, H, Hkv, max_seqlen_q, D, capacity, page_size=0):
    """fa2_fwd_prefill_fp8_plan: prefill_plan's answer for the call on an e4m3 cache (head dims: multiples of 16 up to 256)."""
    plan = FwdPlan()
    check(load().fa2_fwd_prefill_fp8_plan(int(dtype), int(B), int(H), int(Hkv), int(max_seqlen_q), int(D), int(capacity), int(page_size), ctypes.byref(plan)))
    return plan.as_dict()


def prefill_tile(length, capacity, page_size, tile):
    """fa2_prefill_tile -> (page_slot, row_in_page, valid_rows) of 64-key tile `tile` of a sequence of `length` keys (capacity: key slots, or block-table
    entries per sequence when page_size > 0)."""
    slot, row, rows = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(load().fa2_prefill_tile(int(length), int(capacity), int(page_size), int(tile), ctypes.byref(slot), ctypes.byref(row), ctypes.byref(rows)))
    return slot.value, row.value, rows.value


def kvappend_mla_chunks(unit, halves):
    """fa2_kvappend_mla_chunks -> (chunk a, chunk b): the two 16-byte chunks unit `unit` (0 .. 35) of a 576-wide row moves in the latent-cache append."""
    a, b = ctypes.c_int(), ctypes.c_int()
    check(load().fa2_kvappend_mla_chunks(int(unit), int(bool(halves)), ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def strides3(a, b, c):
    return (ctypes.c_int64 * 3)(a, b, c)


def strides2(a, b):
    return (ctypes.c_int64 * 2)(a, b)
