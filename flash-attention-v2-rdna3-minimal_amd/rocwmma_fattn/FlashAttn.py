"""FlashAttention-2 forward operator for MI355X — same entry point as the reference's
rocwmma_fattn/FlashAttn.py (class FlashAttentionFunction, positional signature
`apply(q, k, v, mask, causal, scale, BNHD_fmt)`, FlashAttn.py:45-49), so bench_with_sdpa.py:99,
precision_test.py:63 and the external ComfyUI / sd-webui hooks keep working unchanged.

Layers (reference counterpart in brackets):
  FlashAttentionFunction.forward   [FlashAttn.py:47-76]      operator: shapes, default scale, save for bwd
  flash_attn_wmma.forward          [host.cpp:30-45 +
                                    kernel_fp16.cu:744-876]  dtype switch, D padding, O/L allocation,
                                                             6-tensor return, calls the C-ABI
  libfa2_gfx950.so : fa2_fwd_*     [fwd_kernel, kernel_fp16.cu:306-544]  hand-written gfx950 kernel

  FlashAttentionFunction.backward  [FlashAttn.py:78-92]      operator: dQ, dK, dV through flash_attn_wmma.backward
  libfa2_gfx950.so : fa2_bwd_*     [bwd_kernel, kernel_fp16.cu:547-740]  gfx950 backward kernels

The host is PyTorch-ROCm for memory and streams only; the compute is the C-ABI library
(include/fa2_gfx950.h).  There is no CPU path: tensors must live on a ROCm device.
"""
import collections
import ctypes
import math
import os

import torch

from . import _fa2_lib

__all__ = ["FlashAttentionFunction", "flash_attn_wmma", "flash_attention", "flash_attention_varlen", "merge_attention", "flash_attention_prefill", "flash_attention_prefill_fp8",
           "kvcache_append_varlen", "flash_attention_decode_mla", "kvcache_append_mla", "kvcache_append_mla_varlen"]


class _FlashAttnWmma:
    """Stand-in for the reference's JIT-built pybind module `flash_attn_wmma` (FlashAttn.py:23-41):
    same attribute names, argument order and return contract (host.cpp:60-64)."""

    @staticmethod
    def forward(q, k, v, Br, Bc, causal, scale, permute_NH):
        """forward() of the reference's module: the compiled front end (csrc/frontend.cpp, same logic in C++: ~6 us of host
        time per call instead of ~11) when it was built, else forward_py below."""
        # A caller of the reference's module-level API who pairs forward() with backward() himself (host.cpp:30-58) passes a plain bool: when an input
        # requires a gradient the forward is flagged FA2_FLAG_EXACT_SCALE for him — the backward recomputes P from scores scaled in f32, and an L formed
        # from a folded / rounded-P forward would not match them (2-4x the gradient tolerance at |logit| > 30: ADVICE r5).  Anyone else sets the flag.
        flags = _fa2_lib.call_flags(causal)
        if q.requires_grad or k.requires_grad or v.requires_grad:
            flags |= _fa2_lib.FA2_FLAG_EXACT_SCALE
        fe = _frontend()
        if fe is not None:
            return fe.forward(q, k, v, int(Br), int(Bc), flags, float(scale), bool(permute_NH))
        return _FlashAttnWmma.forward_py(q, k, v, Br, Bc, flags, scale, permute_NH)

    @staticmethod
    def forward_bias(q, k, v, bias, Br, Bc, causal, scale, permute_NH):
        """forward() with an attention bias / mask (extension: the reference reserves `mask` but ignores it, FlashAttn.py:49, :74,
        README.md:45).  `bias` broadcasts against [B, H, Nq, Nkv] like torch SDPA's attn_mask: bool = keep-mask, float = additive.
        Same 6-tensor return as forward()."""
        return _FlashAttnWmma.forward_py(q, k, v, Br, Bc, causal, scale, permute_NH, bias=bias)

    @staticmethod
    def forward_window(q, k, v, Br, Bc, causal, scale, permute_NH, window):
        """forward() under a sliding window (extension: C-ABI fa2_fwd_window).  window = (window_left, window_right, q_offset), -1 = unbounded;
        `causal`: a bool or the C-ABI's call flags.  Same 6-tensor return; grouped k / v run without expansion."""
        fe = _frontend()
        if fe is not None and hasattr(fe, "forward_window"):
            return fe.forward_window(q, k, v, int(Br), int(Bc), _fa2_lib.call_flags(causal), float(scale), bool(permute_NH), *(int(x) for x in window))
        return _FlashAttnWmma.forward_py(q, k, v, Br, Bc, causal, scale, permute_NH, window=window)

    @staticmethod
    def backward_window(Q, K, V, O, dO, L, act_n, act_nkv, act_d, Br, Bc, causal, scale, permute_NH, window):
        """backward() of forward_window (C-ABI fa2_bwd_window; grouped K / V: expanded, dK / dV summed per group in f32)."""
        fe = _frontend()
        if fe is not None and hasattr(fe, "backward_window"):
            return fe.backward_window(Q, K, V, O, dO, L, int(act_n), int(act_nkv), int(act_d), int(Br), int(Bc), bool(causal), float(scale), bool(permute_NH),
                                      *(int(x) for x in window))
        return _FlashAttnWmma.backward_py(Q, K, V, O, dO, L, act_n, act_nkv, act_d, Br, Bc, causal, scale, permute_NH, window=window)

    @staticmethod
    def forward_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, flags, scale, window, dropout=None, scoremod=None):
        """Packed, variable-length forward (extension: C-ABI fa2_fwd_varlen).  q [total_q, H, D], k / v [total_k, Hkv, D] (grouped K / V are addressed
        through the group), cu_seqlens_* int32 [B + 1] on q's device, the maxima host ints; flags = FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE |
        FA2_FLAG_BOTTOM_RIGHT; window = (window_left, window_right), -1 = unbounded.  Returns [O_fwd, q, k, v, O, L] like forward(): the tensors the
        backward wants (D padded to a multiple of 8 if need be; O_fwd a view of O), L = f32 [H, total_q] in log2 units.
        dropout = (p, seed): attention dropout (C-ABI fa2_fwd_varlen_dropout).
        scoremod = (softcap, slopes): logit soft-capping / ALiBi slopes [H] or [num_sequences, H] (C-ABI fa2_fwd_varlen_scoremod); not with dropout."""
        if dropout is not None and scoremod is not None:
            raise RuntimeError("fa2: the score modifiers do not combine with dropout")
        lib = _fa2_lib.load()
        h, h_kv, d = _check_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k)
        if q.dtype == torch.float16:
            dtype_code = _fa2_lib.FA2_DTYPE_F16
            if k.dtype != q.dtype or v.dtype != q.dtype:
                raise RuntimeError("fa2: q, k, v must share one dtype")
        else:
            dtype_code = _fa2_lib.FA2_DTYPE_BF16
            if q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
                q, k, v = q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)
        d_pad = -d % 8
        if d_pad:
            q, k, v = (torch.nn.functional.pad(t, (0, d_pad)) for t in (q, k, v))
        q, k, v = (_packed_ready(t) for t in (q, k, v))
        total_q = q.shape[0]
        O = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        L = torch.empty((h, total_q), dtype=torch.float32, device=q.device)
        if total_q and k.shape[0] == 0:            # no keys at all: every row is dead (and the library wants non-null pointers)
            O.zero_()
            L.fill_(float("-inf"))
        elif total_q:
            dev = q.device.index
            args = (dtype_code, q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr(), L.data_ptr(), cu_seqlens_q.numel() - 1, h, h_kv,
                    max(int(max_seqlen_q), 1), max(int(max_seqlen_k), 1), d + d_pad, cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(),
                    _s2(q), _s2(k), _s2(v), _s2(O), L.stride(0), float(scale), int(flags), int(window[0]), int(window[1]), _raw_stream(dev))
            with torch.cuda.device(dev):
                if scoremod is not None:
                    rc = lib.fa2_fwd_varlen_scoremod(*args, *_scoremod_args(scoremod))
                else:
                    rc = lib.fa2_fwd_varlen(*args) if dropout is None else lib.fa2_fwd_varlen_dropout(*args, float(dropout[0]), int(dropout[1]))
            if rc:
                _fa2_lib.check(rc)
        return [O[..., :d] if d_pad else O, q, k, v, O, L]

    @staticmethod
    def forward_varlen_dv(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, flags, scale, window):
        """forward_varlen with v [total_k, Hkv, Dv] narrower than k (C-ABI fa2_fwd_varlen_dv; forward only).  v keeps its strides — a column slice of a
        wider buffer is addressed in place.  Returns (O [total_q, H, Dv], L f32 [H, total_q] in log2 units)."""
        lib = _fa2_lib.load()
        h, h_kv, d = _check_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, dv=True)
        if q.dtype not in (torch.float16, torch.bfloat16) or k.dtype != q.dtype or v.dtype != q.dtype:
            raise RuntimeError("fa2: q, k, v of a call with v narrower than k must share one dtype, float16 or bfloat16")
        dtype_code = _fa2_lib.FA2_DTYPE_F16 if q.dtype == torch.float16 else _fa2_lib.FA2_DTYPE_BF16
        q, k, v = (_packed_ready(t) for t in (q, k, v))
        total_q, d_v = q.shape[0], v.shape[2]
        O = torch.empty((total_q, h, d_v), dtype=q.dtype, device=q.device)
        L = torch.empty((h, total_q), dtype=torch.float32, device=q.device)
        if total_q and k.shape[0] == 0:            # no keys at all: every row is dead (and the library wants non-null pointers)
            O.zero_()
            L.fill_(float("-inf"))
        elif total_q:
            dev = q.device.index
            with torch.cuda.device(dev):
                rc = lib.fa2_fwd_varlen_dv(dtype_code, q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr(), L.data_ptr(), cu_seqlens_q.numel() - 1, h,
                                           h_kv, max(int(max_seqlen_q), 1), max(int(max_seqlen_k), 1), d, d_v, cu_seqlens_q.data_ptr(),
                                           cu_seqlens_k.data_ptr(), _s2(q), _s2(k), _s2(v), _s2(O), L.stride(0), float(scale), int(flags), int(window[0]),
                                           int(window[1]), _raw_stream(dev))
            if rc:
                _fa2_lib.check(rc)
        return O, L

    @staticmethod
    def backward_varlen(Q, K, V, O, dO, L, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, act_d, flags, scale, window, dropout=None, scoremod=None,
                        dlse=None):
        """backward() of forward_varlen (C-ABI fa2_bwd_varlen; grouped K / V: expanded, dK / dV summed per group in f32).  Returns [dQ, dK, dV].
        dropout = (p, seed) of the forward: the mask is regenerated (fa2_bwd_varlen_dropout; it is keyed by the query head, so expansion changes nothing).
        scoremod = (softcap, slopes) of the forward (fa2_bwd_varlen_scoremod; the slopes belong to the query heads, so expansion changes nothing either).
        dlse: None, or the gradient of the natural-log LSE, f32 [H, total_q] (fa2_bwd_varlen_lse; it belongs to the query heads as well)."""
        lib = _fa2_lib.load()
        if not (Q.is_cuda and dO.is_cuda):
            raise RuntimeError("fa2: tensors must be on a ROCm device (no CPU path in this operator)")
        h, h_kv, dk = Q.size(1), K.size(1), Q.size(2)
        _check_groups(h, h_kv)
        if h_kv != h:
            def mha(Q4, K4, V4, O4, dO4, L_, *rest):
                return [t.unsqueeze(0) for t in _FlashAttnWmma.backward_varlen(Q4[0], K4[0], V4[0], O4[0], dO4[0], L_, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                                                                               max_seqlen_k, act_d, flags, scale, window, dropout, scoremod, dlse)]
            return [t[0] for t in _grouped_backward(mha, Q.unsqueeze(0), K.unsqueeze(0), V.unsqueeze(0), O.unsqueeze(0), dO.unsqueeze(0), L, 0, 0, act_d,
                                                    128, 128, False, scale, True)]
        dtype_code = _fa2_lib.FA2_DTYPE_F16 if Q.dtype == torch.float16 else _fa2_lib.FA2_DTYPE_BF16
        if dO.dtype != Q.dtype:
            dO = dO.to(Q.dtype)
        if dO.size(2) != dk:
            dO = torch.nn.functional.pad(dO, (0, dk - dO.size(2)))
        dO = _packed_ready(dO)
        dQ = torch.empty(Q.shape, dtype=Q.dtype, device=Q.device)       # every element is written by its owner
        dK = torch.empty(K.shape, dtype=K.dtype, device=K.device)
        dV = torch.empty(V.shape, dtype=V.dtype, device=V.device)
        if Q.shape[0] == 0 or K.shape[0] == 0:         # no queries or no keys at all: no gradient anywhere
            return [dQ.zero_()[..., :act_d], dK.zero_()[..., :act_d], dV.zero_()[..., :act_d]]
        L = L.contiguous()
        delta = torch.empty_like(L)
        dev = Q.device.index
        args = (dtype_code, Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), L.data_ptr(), dQ.data_ptr(),
                dK.data_ptr(), dV.data_ptr(), delta.data_ptr(), cu_seqlens_q.numel() - 1, h, max(int(max_seqlen_q), 1),
                max(int(max_seqlen_k), 1), dk, cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(), _s2(Q), _s2(K), _s2(V), _s2(O), _s2(dO),
                _s2(dQ), _s2(dK), _s2(dV), L.stride(0), float(scale), int(flags), int(window[0]), int(window[1]), _raw_stream(dev))
        with torch.cuda.device(dev):
            if dlse is not None:
                g = _dlse_log2(dlse)
                rc = lib.fa2_bwd_varlen_lse(*args, *((0.0, 0) if dropout is None else (float(dropout[0]), int(dropout[1]))),
                                            *((0.0, None, 0) if scoremod is None else _scoremod_args(scoremod)), g.data_ptr(), g.stride(0))
            elif scoremod is not None:
                rc = lib.fa2_bwd_varlen_scoremod(*args, *_scoremod_args(scoremod))
            else:
                rc = lib.fa2_bwd_varlen(*args) if dropout is None else lib.fa2_bwd_varlen_dropout(*args, float(dropout[0]), int(dropout[1]))
        if rc:
            _fa2_lib.check(rc)
        return [dQ[..., :act_d], dK[..., :act_d], dV[..., :act_d]]

    @staticmethod
    def forward_py(q, k, v, Br, Bc, causal, scale, permute_NH, bias=None, window=None, dropout=None, scoremod=None):
        """Returns [O_fwd, q_pad, k_pad, v_pad, O, L] like forward_fp16/forward_bf16 (kernel_fp16.cu:744-876).
        O and L keep the reference's shapes — rows padded to a multiple of Br with a zero tail, O_fwd a view into
        O (kernel_fp16.cu:761, :793-796, :865-875) — but nothing is COPIED to get there: the gfx950 kernels mask
        ragged Nq / Nkv and any D that is a multiple of 8 in-kernel, so q_pad, k_pad, v_pad are the inputs
        themselves (made contiguous if their strides require it; the reference returns padded copies,
        kernel_fp16.cu:767-779).  Only a D that is not a multiple of 8 is zero-padded, to the next multiple of 8.
        Br sizes the N padding of O and L; Bc is accepted for signature compatibility.  `causal`: the reference's bool, or the C-ABI's call flags
        (_fa2_lib.FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE: the operator marks the forward of calls that will be differentiated).
        dropout = (p, seed), with a window (which may be (-1, -1, 0)): attention dropout (C-ABI fa2_fwd_dropout).
        scoremod = (softcap, slopes), with a window likewise: logit soft-capping / ALiBi slopes [H] or [B, H] (C-ABI fa2_fwd_scoremod); not with dropout."""
        if dropout is not None and (window is None or bias is not None):
            raise RuntimeError("fa2: the dropout forward is the windowed one (pass window=(-1, -1, 0) for full attention) and takes no bias")
        if scoremod is not None and (window is None or bias is not None or dropout is not None):
            raise RuntimeError("fa2: the score-modifier forward is the windowed one (pass window=(-1, -1, 0) for full attention) and takes neither bias nor dropout")
        if window is not None:
            window = _fa2_lib.parse_window((window[0], window[1]), window[2])
        lib = _fa2_lib.load()
        flags = _fa2_lib.call_flags(causal)
        causal = bool(flags & _fa2_lib.FA2_FLAG_CAUSAL)
        if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
            raise RuntimeError("fa2: q, k, v must be 4-D ([B,H,N,D] or [B,N,H,D] with BNHD_fmt)")
        if not q.is_cuda or not k.is_cuda or not v.is_cuda:
            raise RuntimeError("fa2: q, k, v must be on a ROCm device (no CPU path in this operator)")
        if k.device != q.device or v.device != q.device:
            raise RuntimeError("fa2: q, k, v must be on the same device")
        # dtype switch (host.cpp:30-45): half stays half, everything else runs (and returns) as bf16
        if q.dtype == torch.float16:
            dtype_code = _fa2_lib.FA2_DTYPE_F16
            if k.dtype != q.dtype or v.dtype != q.dtype:
                raise RuntimeError("fa2: q, k, v must share one dtype")
        else:
            dtype_code = _fa2_lib.FA2_DTYPE_BF16
            if q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
                q, k, v = q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)

        n_ax, h_ax = (1, 2) if permute_NH else (2, 1)
        qsh, ksh = q.shape, k.shape
        b, h, n, d = qsh[0], qsh[h_ax], qsh[n_ax], qsh[3]
        n_kv, h_kv = ksh[n_ax], ksh[h_ax]
        if ksh[0] != b or ksh[3] != d or v.shape != ksh:
            raise RuntimeError("fa2: inconsistent q/k/v shapes %s %s %s" % (tuple(q.shape), tuple(k.shape), tuple(v.shape)))
        _check_groups(h, h_kv)
        if d > _MAX_HEAD_DIM:
            raise RuntimeError("fa2: head dim %d is larger than the largest gfx950 kernel" % d)
        d_pad = -d % 8
        d_kernel = d + d_pad                     # the head dim handed to the C-ABI (columns up to the kernel's are masked there)

        q_pad, k_pad, v_pad = q, k, v
        if d_pad:
            q_pad, k_pad, v_pad = (torch.nn.functional.pad(t, (0, d_pad)) for t in (q, k, v))
        q_pad, k_pad, v_pad = (_kernel_ready(t) for t in (q_pad, k_pad, v_pad))

        # outputs on q's device (kernel_fp16.cu:793-796): rows padded to a multiple of Br like the reference's, only
        # the padding tail is zero-filled (the kernel writes every real row)
        nq_pad = -n % int(Br)
        if nq_pad:
            oshape = (b, n + nq_pad, h, d_kernel) if permute_NH else (b, h, n + nq_pad, d_kernel)
            O = torch.empty(oshape, dtype=q_pad.dtype, device=q_pad.device)
            O.narrow(n_ax, n, nq_pad).zero_()
            L = torch.empty((b, h, n + nq_pad), dtype=torch.float32, device=q.device)
            L[:, :, n:].zero_()
        else:
            O = torch.empty_like(q_pad)
            if not _strides_ok(O):
                O = torch.empty(q_pad.shape, dtype=q_pad.dtype, device=q_pad.device)
            L = torch.empty((b, h, n), dtype=torch.float32, device=q.device)

        def s3(t):
            st = t.stride()
            key = (st[0], st[h_ax], st[n_ax])
            arr = _STRIDE_CACHE.get(key)
            if arr is None:
                if len(_STRIDE_CACHE) > 4096:
                    _STRIDE_CACHE.clear()
                arr = _STRIDE_CACHE[key] = _fa2_lib.strides3(*key)
            return arr

        dev = q.device.index
        args = (dtype_code, q_pad.data_ptr(), k_pad.data_ptr(), v_pad.data_ptr(), O.data_ptr(), L.data_ptr(),
                b, h, n, n_kv, d_kernel, s3(q_pad), s3(k_pad), s3(v_pad), s3(O),
                _fa2_lib.strides2(h * (n + nq_pad), n + nq_pad), float(scale), flags)
        fn = lib.fa2_fwd
        if bias is not None:
            if h_kv != h:
                raise RuntimeError("fa2: the masked forward has no grouped-query form (flash_attention(mask=...) expands k / v for it)")
            bias_t, kind, bstr = _prepare_bias(bias, b, h, n, n_kv, q_pad.dtype, q.device)
            args += (bias_t.data_ptr(), kind, _fa2_lib.strides3(*bstr))
            fn = lib.fa2_fwd_bias
        if scoremod is not None:   # logit soft-capping / ALiBi: fa2_fwd_scoremod (the windowed call's arguments, then softcap, the slopes and their stride)
            with torch.cuda.device(dev):
                rc = lib.fa2_fwd_scoremod(*(args[:8] + (h_kv,) + args[8:]), *window, _raw_stream(dev), *_scoremod_args(scoremod))
        elif dropout is not None:  # attention dropout: fa2_fwd_dropout (the windowed call's arguments, then p and the seed)
            with torch.cuda.device(dev):
                rc = lib.fa2_fwd_dropout(*(args[:8] + (h_kv,) + args[8:]), *window, _raw_stream(dev), float(dropout[0]), int(dropout[1]))
        elif window is not None:   # sliding window: fa2_fwd_window (grouped or not: K / V addressed through the group)
            with torch.cuda.device(dev):
                rc = lib.fa2_fwd_window(*(args[:8] + (h_kv,) + args[8:]), *window, _raw_stream(dev))
        elif h_kv != h:        # grouped-query attention: fa2_fwd_gqa (the MHA call's kernels, K / V addressed through the group)
            args = args[:8] + (h_kv,) + args[8:]
            with torch.cuda.device(dev):
                rc = _launch_fwd_gqa(lib, args, dev, q.device, not causal)
        elif dev != _current_device():
            with torch.cuda.device(dev):
                rc = _launch_fwd(lib, fn, args, dev, q.device, bias is None and not causal)
        else:
            rc = _launch_fwd(lib, fn, args, dev, q.device, bias is None and not causal)
        if rc:
            _fa2_lib.check(rc)

        O_fwd = O                                # a view into the padded O (kernel_fp16.cu:865-875)
        if nq_pad:
            O_fwd = O_fwd.narrow(n_ax, 0, n)
        if d_pad:
            O_fwd = O_fwd[..., :d]
        return [O_fwd, q_pad, k_pad, v_pad, O, L]

    @staticmethod
    def backward(Q, K, V, O, dO, L, act_n, act_nkv, act_d, Br, Bc, causal, scale, permute_NH, bias=None):
        """Returns [dQ, dK, dV] sliced to the actual sizes, like backward_fp16/backward_bf16
        (host.cpp:47-58, kernel_fp16.cu:878-1028).  Q, K, V, O, L are the tensors the forward returned
        (D a multiple of 8); the gfx950 kernels take the actual Nq / Nkv / D and mask in-kernel, so nothing is
        padded here except a dO whose D differs from Q's."""
        if bias is None:
            fe = _frontend()
            if fe is not None and hasattr(fe, "backward"):      # the compiled front end (csrc/frontend.cpp): the same steps in C++
                return fe.backward(Q, K, V, O, dO, L, int(act_n), int(act_nkv), int(act_d), int(Br), int(Bc), bool(causal), float(scale), bool(permute_NH))
        return _FlashAttnWmma.backward_py(Q, K, V, O, dO, L, act_n, act_nkv, act_d, Br, Bc, causal, scale, permute_NH, bias)

    @staticmethod
    def backward_py(Q, K, V, O, dO, L, act_n, act_nkv, act_d, Br, Bc, causal, scale, permute_NH, bias=None, window=None, dropout=None, scoremod=None,
                    dlse=None):
        """backward() in Python (masked calls; every call when the compiled front end is absent).  window: as forward_window's.
        dlse: None, or the gradient of the natural-log LSE, f32 [B, H, Nq] with any strides: the family's *_lse entry point (fa2_bwd_lse without a window,
        fa2_bwd_window_lse with one) instead of the call made without it.
        dropout = (p, seed) of the forward: the mask is regenerated (fa2_bwd_dropout; it is keyed by the query head, so expanding grouped K / V changes nothing)."""
        if dropout is not None and (window is None or bias is not None):
            raise RuntimeError("fa2: the dropout backward is the windowed one (pass window=(-1, -1, 0) for full attention) and takes no bias")
        # scoremod = (softcap, slopes) of the forward (fa2_bwd_scoremod; the slopes belong to the query heads, so expanding grouped K / V changes nothing)
        if scoremod is not None and (window is None or bias is not None or dropout is not None):
            raise RuntimeError("fa2: the score-modifier backward is the windowed one (pass window=(-1, -1, 0) for full attention) and takes neither bias nor dropout")
        if window is not None:
            window = _fa2_lib.parse_window((window[0], window[1]), window[2])
        lib = _fa2_lib.load()
        if not (Q.is_cuda and dO.is_cuda):
            raise RuntimeError("fa2: tensors must be on a ROCm device (no CPU path in this operator)")
        n_ax, h_ax = (1, 2) if permute_NH else (2, 1)
        b, h, dk = Q.size(0), Q.size(h_ax), Q.size(3)
        h_kv = K.size(h_ax)
        _check_groups(h, h_kv)
        if h_kv != h:
            if bias is not None:
                raise RuntimeError("fa2: the masked backward has no grouped-query form (flash_attention(mask=...) expands k / v for it)")
            mha = _FlashAttnWmma.backward_py if window is None and dlse is None else (
                lambda *a: _FlashAttnWmma.backward_py(*a, window=window, dropout=dropout, scoremod=scoremod, dlse=dlse))
            return _grouped_backward(mha, Q, K, V, O, dO, L, act_n, act_nkv, act_d, Br, Bc, causal, scale, permute_NH)
        act_n, act_nkv, act_d = int(act_n), int(act_nkv), int(act_d)
        dtype_code = _fa2_lib.FA2_DTYPE_F16 if Q.dtype == torch.float16 else _fa2_lib.FA2_DTYPE_BF16
        if dO.dtype != Q.dtype:
            dO = dO.to(Q.dtype)                       # host.cpp:47-58 dispatches on dO's dtype; Q's wins here
        if dO.size(3) != dk:                          # kernel_fp16.cu:900-905: dO is padded in D like Q
            dO = torch.nn.functional.pad(dO, (0, dk - dO.size(3)))
        dO = _kernel_ready(dO)
        dQ = torch.empty(Q.shape, dtype=Q.dtype, device=Q.device)   # every element [:act_n] is written by its owner
        dK = torch.empty(K.shape, dtype=K.dtype, device=K.device)
        dV = torch.empty(V.shape, dtype=V.dtype, device=V.device)
        delta = torch.empty((b, h, L.size(2)), dtype=torch.float32, device=Q.device)
        if L.stride() != delta.stride():
            L = L.contiguous()

        def s3(t):
            st = t.stride()
            return _fa2_lib.strides3(st[0], st[h_ax], st[n_ax])

        stream = _raw_stream(Q.device.index)
        args = (dtype_code, Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), L.data_ptr(),
                dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), delta.data_ptr(), b, h, act_n, act_nkv, dk,
                s3(Q), s3(K), s3(V), s3(O), s3(dO), s3(dQ), s3(dK), s3(dV),
                _fa2_lib.strides2(L.stride(0), L.stride(1)), float(scale), 1 if causal else 0)
        fn = lib.fa2_bwd
        if dlse is not None:         # a gradient for the LSE: the superset entry points take every family's arguments, then dlse (log2 units) and its strides
            g = _dlse_log2(dlse)
            if window is not None:
                args += tuple(window) + (stream,) + ((0.0, 0) if dropout is None else (float(dropout[0]), int(dropout[1])))
                args += (0.0, None, 0) if scoremod is None else _scoremod_args(scoremod)
                fn = lib.fa2_bwd_window_lse
            else:
                if bias is not None:
                    bias_t, kind, bstr = _prepare_bias(bias, b, h, act_n, act_nkv, Q.dtype, Q.device)
                    args += (bias_t.data_ptr(), kind, _fa2_lib.strides3(*bstr))
                else:
                    args += (None, _fa2_lib.FA2_BIAS_NONE, None)
                need = 0 if causal else (lib.fa2_bwd_workspace_bytes if bias is None else lib.fa2_bwd_bias_workspace_bytes)(dtype_code, b, h, act_n, act_nkv, dk, 0)
                ws = _workspace(need, Q.device, Q.device.index, stream) if need else None
                args += (ws.data_ptr() if need else None, need, stream)
                fn = lib.fa2_bwd_lse
            args += (g.data_ptr(), _fa2_lib.strides2(g.stride(0), g.stride(1)))
            with torch.cuda.device(Q.device):
                rc = fn(*args)
            if rc:
                _fa2_lib.check(rc)
            if permute_NH:
                return [dQ[:, :act_n, :, :act_d], dK[:, :act_nkv, :, :act_d], dV[:, :act_nkv, :, :act_d]]
            return [dQ[:, :, :act_n, :act_d], dK[:, :, :act_nkv, :act_d], dV[:, :, :act_nkv, :act_d]]
        if bias is not None:         # backward through forward_bias (extension, like the masked forward itself): same bias arguments
            bias_t, kind, bstr = _prepare_bias(bias, b, h, act_n, act_nkv, Q.dtype, Q.device)
            args += (bias_t.data_ptr(), kind, _fa2_lib.strides3(*bstr))
            fn = lib.fa2_bwd_bias
        if window is not None:
            args += tuple(window)
            fn = lib.fa2_bwd_window
        elif not causal:
            # scratch for the split of a partly filled last round of workgroups (fa2_bwd_ws / fa2_bwd_bias_ws, the backward's twins of fa2_fwd_ws)
            need = (lib.fa2_bwd_workspace_bytes if bias is None else lib.fa2_bwd_bias_workspace_bytes)(dtype_code, b, h, act_n, act_nkv, dk, 0)
            if need:
                ws = _workspace(need, Q.device, Q.device.index, stream)
                args += (ws.data_ptr(), need)
                fn = lib.fa2_bwd_ws if bias is None else lib.fa2_bwd_bias_ws
        args += (stream,)
        if dropout is not None:
            args += (float(dropout[0]), int(dropout[1]))
            fn = lib.fa2_bwd_dropout
        if scoremod is not None:
            args += _scoremod_args(scoremod)
            fn = lib.fa2_bwd_scoremod
        if Q.device.index != _current_device():
            with torch.cuda.device(Q.device):
                rc = fn(*args)
        else:
            rc = fn(*args)
        if rc:
            _fa2_lib.check(rc)
        if permute_NH:
            return [dQ[:, :act_n, :, :act_d], dK[:, :act_nkv, :, :act_d], dV[:, :act_nkv, :, :act_d]]
        return [dQ[:, :, :act_n, :act_d], dK[:, :, :act_nkv, :act_d], dV[:, :, :act_nkv, :act_d]]


_WS_POOL = {}            # (device index, raw stream) -> uint8 tensor: the split's scratch, allocated once per stream and reused (grown when a call needs more)
_WS_POOL_MAX = 8         # streams with a pooled workspace (least recently used dropped beyond that)
_WS_KEEP = 4 << 20       # a block up to this size stays whatever the next call needs


def _workspace_unused(dev, stream):
    """A call on `stream` that needs no scratch: a pooled block above _WS_KEEP is released (the allocator caches it; the next call that splits takes it
    back) — the operator's footprint follows the calls being made, not the largest one ever made."""
    ws = _WS_POOL.get((dev, stream))
    if ws is not None and ws.numel() > _WS_KEEP:
        del _WS_POOL[(dev, stream)]


def _workspace(need, device, dev, stream):
    """`need` bytes of scratch for a call on `stream`: ONE tensor per (device, stream), reused by every later call on that stream (kernels of one
    stream run in order, so the merge of call n has read the tiles before the parts of call n + 1 write them) — the operator's memory footprint is
    its outputs plus at most 64 MiB per stream in use, instead of a fresh block per call in flight (the reference records peak
    memory on every run, bench_with_sdpa.py:34).  While a graph is being captured the block comes from the allocator (the capture's private pool
    keeps it alive for the graph's replays); FA2_WS_POOL=0 restores per-call allocation."""
    if not _POOL_ON or torch.cuda.is_current_stream_capturing():
        return torch.empty(need, dtype=torch.uint8, device=device)
    key = (dev, stream)
    ws = _WS_POOL.pop(key, None)
    # grown when a call needs more — and (round 6) let go when a call needs less than half of a block above _WS_KEEP: the pool was a high-water mark,
    # every later call of the process carried the largest block any call had needed (the reference harness's D scan: +60 MB on every row)
    if ws is None or ws.numel() < need or (ws.numel() > _WS_KEEP and ws.numel() > 2 * need):
        ws = None                # (drop the old block first: the allocator can hand the same memory back)
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        while len(_WS_POOL) >= _WS_POOL_MAX:
            _WS_POOL.pop(next(iter(_WS_POOL)))
    _WS_POOL[key] = ws       # (re-inserted: most recently used last)
    return ws


def workspace_pool_bytes():
    """Bytes the per-stream scratch blocks of this process hold right now (tools/scan_bench.py reports it beside the peak)."""
    n = sum(t.numel() for t in _WS_POOL.values())
    fe = _frontend()
    if fe is not None and hasattr(fe, "workspace_pool_bytes"):      # the compiled front end keeps its own blocks
        n += int(fe.workspace_pool_bytes())
    return n


_POOL_ON = os.environ.get("FA2_WS_POOL", "1") != "0"


def _launch_fwd(lib, fn, args, dev, device, may_split):
    """The C-ABI call on torch's current stream.  Non-causal, unbiased launches go through fa2_fwd_ws when the library can use a
    workspace for this shape (KV-split of the last, partly filled round of workgroups: include/fa2_gfx950.h): scratch memory from
    the per-stream pool above."""
    if may_split:
        # (the size is a function of dtype, shape, device and the library's options: asked once per shape — _fa2_lib.options() and
        #  _fa2_lib.set_option() drop the cache; a stale entry would only cost the split, the library re-plans every call itself)
        key = (args[0], args[6], args[7], args[8], args[9], args[10], dev)
        need = _WS_CACHE.get(key)
        if need is None:
            if len(_WS_CACHE) > 4096:
                _WS_CACHE.clear()
            need = _WS_CACHE[key] = lib.fa2_fwd_workspace_bytes(args[0], *args[6:11], 0)
        if need:
            stream = _raw_stream(dev)
            ws = _workspace(need, device, dev, stream)
            return lib.fa2_fwd_ws(*args, ws.data_ptr(), need, stream)
    stream = _raw_stream(dev)
    if _WS_POOL:
        _workspace_unused(dev, stream)
    return fn(*args, stream)


def _launch_fwd_gqa(lib, args, dev, device, may_split):
    """fa2_fwd_gqa on torch's current stream (args: fa2_fwd's with the K / V head count after H), with the KV-split's scratch where the library
    can use it for this shape (fa2_fwd_gqa_workspace_bytes: the MHA call's answer)."""
    stream = _raw_stream(dev)
    need = lib.fa2_fwd_gqa_workspace_bytes(args[0], *args[6:12], 0) if may_split else 0
    if need:
        ws = _workspace(need, device, dev, stream)
        return lib.fa2_fwd_gqa(*args, ws.data_ptr(), need, stream)
    if _WS_POOL:
        _workspace_unused(dev, stream)
    return lib.fa2_fwd_gqa(*args, None, 0, stream)


def _grouped_backward(mha_backward, Q, K, V, O, dO, L, act_n, act_nkv, act_d, Br, Bc, causal, scale, permute_NH):
    """The operator's backward of a grouped-query call: K / V expanded to q's head count, the MHA backward, dK / dV summed over each group (f32
    accumulation, one rounding).  The C-ABI's fa2_bwd_gqa sums the groups in-kernel without the expanded tensors, but its dK / dV pass runs
    B * Hkv KV owners — a grid g times smaller — and lost to this path on every shape measured (profiles/r28_gqa_bench.txt)."""
    h_ax = 2 if permute_NH else 1
    g = Q.size(h_ax) // K.size(h_ax)
    dQ, dKe, dVe = mha_backward(Q, K.repeat_interleave(g, dim=h_ax), V.repeat_interleave(g, dim=h_ax), O, dO, L, act_n, act_nkv, act_d, Br, Bc,
                                causal, scale, permute_NH)
    return [dQ, dKe.unflatten(h_ax, (K.size(h_ax), g)).sum(h_ax + 1), dVe.unflatten(h_ax, (V.size(h_ax), g)).sum(h_ax + 1)]


_I64x2, _I64x3 = ctypes.c_int64 * 2, ctypes.c_int64 * 3          # (the array types of _fa2_lib.strides2 / strides3)


def _s2(t):
    """{head, row} element strides of a packed [total, heads, D] tensor, as the varlen entry points take them."""
    s = t.stride()
    return _I64x2(s[1], s[0])


def _packed_ready(t):
    """A packed [total, heads, D] tensor the kernels can address: D contiguous, strides multiples of 8 elements, 16-byte aligned."""
    s0, s1, s2 = t.stride()
    return t if s2 == 1 and not ((s0 | s1) & 7) and not (t.data_ptr() & 15) else t.contiguous()


def _check_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, dv=False):
    """The argument checks of the packed calls, before any device work -> (H, Hkv, D).  dv: v may be narrower than k (flash_attention_varlen's
    Dv route, which has checked the pair of widths already); everywhere else v has k's shape."""
    if not all(torch.is_tensor(t) for t in (q, k, v)) or q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise ValueError("fa2: q, k, v of a packed (varlen) call must be 3-D: [total_q, H, D] and [total_k, Hkv, D]")
    if not torch.is_tensor(cu_seqlens_q) or not torch.is_tensor(cu_seqlens_k) or cu_seqlens_q.dim() != 1 or cu_seqlens_k.dim() != 1:
        raise ValueError("fa2: cu_seqlens_q / cu_seqlens_k must be 1-D int32 tensors of B + 1 row offsets")
    if cu_seqlens_q.numel() != cu_seqlens_k.numel() or cu_seqlens_q.numel() < 2:
        raise ValueError("fa2: cu_seqlens_q and cu_seqlens_k must have the same length B + 1 >= 2, got %d and %d" % (cu_seqlens_q.numel(), cu_seqlens_k.numel()))
    if cu_seqlens_q.dtype != torch.int32 or cu_seqlens_k.dtype != torch.int32:
        raise ValueError("fa2: cu_seqlens_q / cu_seqlens_k must be int32, got %s and %s" % (cu_seqlens_q.dtype, cu_seqlens_k.dtype))
    if cu_seqlens_q.device != q.device or cu_seqlens_k.device != q.device:
        raise ValueError("fa2: cu_seqlens_q / cu_seqlens_k must be on the device of q")
    if k.shape[2] != q.shape[2] or (v.shape[:2] != k.shape[:2] if dv else v.shape != k.shape):
        raise RuntimeError("fa2: inconsistent q/k/v shapes %s %s %s" % (tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    _check_groups(q.shape[1], k.shape[1])
    if q.shape[2] > _MAX_HEAD_DIM:
        raise RuntimeError("fa2: head dim %d is larger than the largest gfx950 kernel" % q.shape[2])
    if not q.is_cuda or not k.is_cuda or not v.is_cuda:
        raise RuntimeError("fa2: q, k, v must be on a ROCm device (no CPU path in this operator)")
    if k.device != q.device or v.device != q.device:
        raise RuntimeError("fa2: q, k, v must be on the same device")
    if not cu_seqlens_q.is_contiguous() or not cu_seqlens_k.is_contiguous():
        raise ValueError("fa2: cu_seqlens_q / cu_seqlens_k must be contiguous")
    return q.shape[1], k.shape[1], q.shape[2]


def _check_groups(h, h_kv):
    """Grouped-query attention: k and v share a head count that divides q's (Q head i attends K / V head i // (h // h_kv))."""
    if h_kv < 1 or h % h_kv:
        raise RuntimeError("fa2: the head count of k / v (%d) must divide the head count of q (%d)" % (h_kv, h))


_FRONTEND = [False]      # False = not looked for yet, None = absent


def _frontend():
    """The optional compiled front end (rocwmma_fattn/_fa2_frontend.so, built by build.py); FA2_FRONTEND=py disables it."""
    if _FRONTEND[0] is False:
        mod = None
        if os.environ.get("FA2_FRONTEND", "") != "py":
            _fa2_lib.load()                       # the kernel library first: the front end links against it
            try:
                from . import _fa2_frontend as mod  # noqa: F401
            except ImportError:
                mod = None
        _FRONTEND[0] = mod
    return _FRONTEND[0]


_STRIDE_CACHE = {}       # (batch, head, row) element strides -> ctypes int64[3] (the arrays are read-only for the library)
_WS_CACHE = _fa2_lib.WS_CACHE      # (dtype, B, H, Nq, Nkv, D, device) -> fa2_fwd_workspace_bytes
_MAX_HEAD_DIM = 512      # largest kernel head dim, forward and backward (fa2_supported_head_dims)
_MAX_MASKED_BWD_HEAD_DIM = 256     # ... of the masked backward (fa2_bwd_bias)


def _raw_stream(device_index):
    """hipStream_t of torch's current stream on that device, as an integer (the cheap form of
    torch.cuda.current_stream(dev).cuda_stream: this is on the path of every call)."""
    return torch._C._cuda_getCurrentRawStream(device_index)


def _current_device():
    return torch._C._cuda_getDevice()


def _strides_ok(t):
    s0, s1, s2, s3 = t.stride()
    return s3 == 1 and not ((s0 | s1 | s2) & 7) and not (t.data_ptr() & 15)


def _prepare_bias(bias, b, h, n, n_kv, io_dtype, device):
    """Attention bias / mask -> (tensor kept alive by the caller, bias_kind, element strides (batch, head, row)) for fa2_fwd_bias.
    Broadcasting follows torch.nn.functional.scaled_dot_product_attention: a 2-, 3- or 4-D tensor is aligned on the right
    against [B, H, Nq, Nkv] and every dimension is 1 or full size; broadcast dimensions become stride 0 — nothing is expanded
    in memory unless the Nkv dimension itself is broadcast or strided."""
    if not torch.is_tensor(bias) or bias.dim() < 2 or bias.dim() > 4:
        raise RuntimeError("fa2: the attention mask must be a 2-, 3- or 4-D tensor broadcastable to [B, H, Nq, Nkv]")
    if bias.device != device:
        raise RuntimeError("fa2: the attention mask must be on the device of q")
    m = bias
    while m.dim() < 4:
        m = m.unsqueeze(0)
    for size, full in zip(m.shape, (b, h, n, n_kv)):
        if size != 1 and size != full:
            raise RuntimeError("fa2: attention mask of shape %s does not broadcast to %s" % (tuple(bias.shape), (b, h, n, n_kv)))
    if m.dtype == torch.bool:
        kind = _fa2_lib.FA2_BIAS_BOOL
    elif m.dtype == torch.float32:
        kind = _fa2_lib.FA2_BIAS_F32
    else:
        kind = _fa2_lib.FA2_BIAS_IO_DTYPE
        if m.dtype != io_dtype:
            m = m.to(io_dtype)
    if m.size(3) != n_kv:
        m = m.expand(m.size(0), m.size(1), m.size(2), n_kv).contiguous()
    elif m.stride(3) != 1 and n_kv > 1:
        m = m.contiguous()
    if kind == _fa2_lib.FA2_BIAS_BOOL:
        m = m.view(torch.uint8)
    strides = tuple(m.stride(i) if m.size(i) > 1 else 0 for i in range(3))
    return m, kind, strides


def _kernel_ready(t):
    """kernel_fp16.cu:780-787 makes a tensor contiguous iff its last stride is not 1; the gfx950
    kernel additionally wants 16-byte aligned rows (strides multiple of 8 elements)."""
    return t if _strides_ok(t) else t.contiguous()


flash_attn_wmma = _FlashAttnWmma()


class FlashAttentionFunction(torch.autograd.Function):

    @staticmethod
    @torch.no_grad()
    def forward(ctx, q, k, v, mask=None, causal=None, scale=None, BNHD_fmt=False, *args, **kwargs):
        # reference: FlashAttn.py:47-76.  `mask` is accepted and ignored there too (only stored).
        D = q.shape[3]
        N = q.shape[2]
        Nkv = k.shape[2]

        Br = 64
        Bc = 128

        if BNHD_fmt:
            N = q.shape[1]
            Nkv = k.shape[1]

        if scale is None:
            scale = D ** -0.5
        if D > 384:
            Br = 32
            Bc = 128

        # a call that will be differentiated scales the f32 product (FA2_FLAG_EXACT_SCALE: the reference kernel's contract, kernel_fp16.cu:164) whatever
        # option "fold" says: the backward then recomputes P from the very scores L was formed from
        # (q, k OR v: the reference looks at q alone, FlashAttn.py:73, and a call in which only K / V need gradients fails in its backward)
        needs_grad = ctx is not None and (q.requires_grad or k.requires_grad or v.requires_grad)
        flags = (_fa2_lib.FA2_FLAG_CAUSAL if causal else 0) | (_fa2_lib.FA2_FLAG_EXACT_SCALE if needs_grad else 0)
        ret = flash_attn_wmma.forward(q, k, v, Br, Bc, flags if needs_grad else bool(causal), scale, BNHD_fmt)

        o, q_bwd, k_bwd, v_bwd, o_bwd, L = ret

        if needs_grad:       # (ctx is None on the inference fast path below, e.g. under torch.no_grad())
            ctx.args = (causal, scale, mask, N, Nkv, D, BNHD_fmt)
            ctx.save_for_backward(q_bwd, k_bwd, v_bwd, o_bwd, L)
        return o

    @staticmethod
    @torch.no_grad()
    def backward(ctx, do):
        # reference: FlashAttn.py:78-92
        causal, scale, mask, N, Nkv, D, BNHD_fmt = ctx.args
        q, k, v, o, L = ctx.saved_tensors
        Br = 128
        Bc = 128
        dQ, dK, dV = flash_attn_wmma.backward(q, k, v, o, do, L, N, Nkv, D, Br, Bc, causal, scale, BNHD_fmt)
        return dQ, dK, dV, None, None, None, None


# Inference fast path: when nothing can require a gradient the autograd.Function machinery (a Python-side graph node
# per call, ~5 us) is skipped and forward() runs directly; `FlashAttentionFunction.apply(...)` keeps the reference's
# call shape and result either way (reference: FlashAttn.py:45-76).
_autograd_apply = FlashAttentionFunction.apply


def _apply(q, k, v, mask=None, causal=None, scale=None, BNHD_fmt=False, *args, **kwargs):
    h_ax = 2 if BNHD_fmt else 1
    if q.dim() == 4 and k.dim() == 4 and k.shape[h_ax] != q.shape[h_ax]:
        _check_groups(q.shape[h_ax], k.shape[h_ax])      # (grouped-query attention: refused before any device work when the counts do not divide)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        fe = _frontend()
        if fe is not None and q.requires_grad and not args and not kwargs and hasattr(fe, "attention"):
            # the same node in C++ (csrc/frontend.cpp::AttentionNode): its backward runs on the autograd engine's device thread without the GIL
            return fe.attention(q, k, v, bool(causal), float(q.shape[3] ** -0.5 if scale is None else scale), bool(BNHD_fmt))
        return _autograd_apply(q, k, v, mask, causal, scale, BNHD_fmt, *args, **kwargs)
    return FlashAttentionFunction.forward(None, q, k, v, mask, causal, scale, BNHD_fmt)


FlashAttentionFunction.apply = staticmethod(_apply)


class _MaskedAttentionFunction(torch.autograd.Function):
    """autograd node of flash_attention(mask=...): forward = fa2_fwd_bias, backward = fa2_bwd_bias (the mask is a constant: no gradient)."""

    @staticmethod
    @torch.no_grad()
    def forward(ctx, q, k, v, mask, causal, scale, BNHD_fmt):
        D = q.shape[3]
        # what fa2_bwd_bias would refuse is refused HERE, before the forward's work is done (a training step must not fail inside loss.backward())
        if D > _MAX_MASKED_BWD_HEAD_DIM:
            raise RuntimeError("fa2: a masked attention call that needs gradients supports head dims up to %d (got %d): fa2_bwd_bias has no kernel above"
                               % (_MAX_MASKED_BWD_HEAD_DIM, D))
        if torch.is_tensor(mask) and mask.dim() >= 2 and mask.shape[-2] > 1:
            n_ax_ = 1 if BNHD_fmt else 2
            if (q.shape[n_ax_] + 63) * k.shape[n_ax_] * (4 if mask.dtype == torch.float32 else 1 if mask.dtype == torch.bool else 2) >= 2 ** 31 - 1:
                raise RuntimeError("fa2: one (batch, head) slice of the attention mask must span < 2 GiB for the masked backward (fa2_bwd_bias)")
        Br = 32 if D > 384 else 64                      # FlashAttn.py:56-67
        o, q_bwd, k_bwd, v_bwd, o_bwd, L = flash_attn_wmma.forward_bias(q, k, v, mask, Br, 128, bool(causal), scale, BNHD_fmt)     # (the biased kernels never fold)
        n_ax = 1 if BNHD_fmt else 2
        ctx.args = (causal, scale, q.shape[n_ax], k.shape[n_ax], D, BNHD_fmt)
        ctx.save_for_backward(q_bwd, k_bwd, v_bwd, o_bwd, L, mask)
        return o

    @staticmethod
    @torch.no_grad()
    def backward(ctx, do):
        causal, scale, N, Nkv, D, BNHD_fmt = ctx.args
        q, k, v, o, L, mask = ctx.saved_tensors
        dQ, dK, dV = flash_attn_wmma.backward(q, k, v, o, do, L, N, Nkv, D, 128, 128, causal, scale, BNHD_fmt, bias=mask)
        return dQ, dK, dV, None, None, None, None


class _WindowAttentionFunction(torch.autograd.Function):
    """autograd node of flash_attention(window=..., q_offset=...): forward = fa2_fwd_window, backward = fa2_bwd_window; saves the three integers."""

    @staticmethod
    @torch.no_grad()
    def forward(ctx, q, k, v, causal, scale, BNHD_fmt, window):
        D = q.shape[3]
        Br = 32 if D > 384 else 64                      # FlashAttn.py:56-67
        flags = (_fa2_lib.FA2_FLAG_CAUSAL if causal else 0) | _fa2_lib.FA2_FLAG_EXACT_SCALE
        o, q_bwd, k_bwd, v_bwd, o_bwd, L = flash_attn_wmma.forward_window(q, k, v, Br, 128, flags, scale, BNHD_fmt, window)
        n_ax = 1 if BNHD_fmt else 2
        ctx.args = (causal, scale, q.shape[n_ax], k.shape[n_ax], D, BNHD_fmt, window)
        ctx.save_for_backward(q_bwd, k_bwd, v_bwd, o_bwd, L)
        return o

    @staticmethod
    @torch.no_grad()
    def backward(ctx, do):
        causal, scale, N, Nkv, D, BNHD_fmt, window = ctx.args
        q, k, v, o, L = ctx.saved_tensors
        dQ, dK, dV = flash_attn_wmma.backward_window(q, k, v, o, do, L, N, Nkv, D, 128, 128, causal, scale, BNHD_fmt, window)
        return dQ, dK, dV, None, None, None, None


class _VarlenAttentionFunction(torch.autograd.Function):
    """autograd node of flash_attention_varlen: forward = fa2_fwd_varlen (flagged FA2_FLAG_EXACT_SCALE), backward = fa2_bwd_varlen.
    dropout = None or (p, seed): the dropout twins of the two; the node saves the seed and the backward regenerates the mask."""

    @staticmethod
    @torch.no_grad()
    def forward(ctx, q, k, v, cu_q, cu_k, max_q, max_k, flags, scale, window, dropout=None):
        o, q_bwd, k_bwd, v_bwd, o_bwd, L = flash_attn_wmma.forward_varlen(q, k, v, cu_q, cu_k, max_q, max_k, flags | _fa2_lib.FA2_FLAG_EXACT_SCALE, scale, window,
                                                                          dropout)
        ctx.args = (max_q, max_k, q.shape[2], flags, scale, window, dropout)
        ctx.save_for_backward(q_bwd, k_bwd, v_bwd, o_bwd, L, cu_q, cu_k)
        return o

    @staticmethod
    @torch.no_grad()
    def backward(ctx, do):
        max_q, max_k, D, flags, scale, window, dropout = ctx.args
        q, k, v, o, L, cu_q, cu_k = ctx.saved_tensors
        dQ, dK, dV = flash_attn_wmma.backward_varlen(q, k, v, o, do, L, cu_q, cu_k, max_q, max_k, D, flags, scale, window, dropout)
        return dQ, dK, dV, None, None, None, None, None, None, None, None


class _DropoutAttentionFunction(torch.autograd.Function):
    """autograd node of flash_attention(dropout_p > 0): forward = fa2_fwd_dropout, backward = fa2_bwd_dropout; saves the window, p and the seed — the
    backward regenerates the forward's mask."""

    @staticmethod
    @torch.no_grad()
    def forward(ctx, q, k, v, causal, scale, BNHD_fmt, window, dropout):
        D = q.shape[3]
        Br = 32 if D > 384 else 64                      # FlashAttn.py:56-67
        flags = (_fa2_lib.FA2_FLAG_CAUSAL if causal else 0) | _fa2_lib.FA2_FLAG_EXACT_SCALE
        o, q_bwd, k_bwd, v_bwd, o_bwd, L = flash_attn_wmma.forward_py(q, k, v, Br, 128, flags, scale, BNHD_fmt, window=window, dropout=dropout)
        n_ax = 1 if BNHD_fmt else 2
        ctx.args = (causal, scale, q.shape[n_ax], k.shape[n_ax], D, BNHD_fmt, window, dropout)
        ctx.save_for_backward(q_bwd, k_bwd, v_bwd, o_bwd, L)
        return o

    @staticmethod
    @torch.no_grad()
    def backward(ctx, do):
        causal, scale, N, Nkv, D, BNHD_fmt, window, dropout = ctx.args
        q, k, v, o, L = ctx.saved_tensors
        dQ, dK, dV = flash_attn_wmma.backward_py(q, k, v, o, do, L, N, Nkv, D, 128, 128, causal, scale, BNHD_fmt, window=window, dropout=dropout)
        return dQ, dK, dV, None, None, None, None, None


class _ScoreModAttentionFunction(torch.autograd.Function):
    """autograd node of flash_attention(softcap > 0 or alibi_slopes): forward = fa2_fwd_scoremod, backward = fa2_bwd_scoremod; saves the window, softcap and
    the slopes, which are constants of the call (no gradient, as in flash-attn)."""

    @staticmethod
    @torch.no_grad()
    def forward(ctx, q, k, v, slopes, causal, scale, BNHD_fmt, window, softcap):
        D = q.shape[3]
        Br = 32 if D > 384 else 64                      # FlashAttn.py:56-67
        flags = (_fa2_lib.FA2_FLAG_CAUSAL if causal else 0) | _fa2_lib.FA2_FLAG_EXACT_SCALE
        o, q_bwd, k_bwd, v_bwd, o_bwd, L = flash_attn_wmma.forward_py(q, k, v, Br, 128, flags, scale, BNHD_fmt, window=window, scoremod=(softcap, slopes))
        n_ax = 1 if BNHD_fmt else 2
        ctx.args = (causal, scale, q.shape[n_ax], k.shape[n_ax], D, BNHD_fmt, window, softcap, slopes is not None)
        ctx.save_for_backward(q_bwd, k_bwd, v_bwd, o_bwd, L, *(() if slopes is None else (slopes,)))
        return o

    @staticmethod
    @torch.no_grad()
    def backward(ctx, do):
        causal, scale, N, Nkv, D, BNHD_fmt, window, softcap, has_slopes = ctx.args
        q, k, v, o, L = ctx.saved_tensors[:5]
        slopes = ctx.saved_tensors[5] if has_slopes else None
        dQ, dK, dV = flash_attn_wmma.backward_py(q, k, v, o, do, L, N, Nkv, D, 128, 128, causal, scale, BNHD_fmt, window=window, scoremod=(softcap, slopes))
        return dQ, dK, dV, None, None, None, None, None, None


class _VarlenScoreModAttentionFunction(torch.autograd.Function):
    """autograd node of flash_attention_varlen(softcap > 0 or alibi_slopes): forward = fa2_fwd_varlen_scoremod, backward = fa2_bwd_varlen_scoremod."""

    @staticmethod
    @torch.no_grad()
    def forward(ctx, q, k, v, slopes, cu_q, cu_k, max_q, max_k, flags, scale, window, softcap):
        o, q_bwd, k_bwd, v_bwd, o_bwd, L = flash_attn_wmma.forward_varlen(q, k, v, cu_q, cu_k, max_q, max_k, flags | _fa2_lib.FA2_FLAG_EXACT_SCALE, scale, window,
                                                                          scoremod=(softcap, slopes))
        ctx.args = (max_q, max_k, q.shape[2], flags, scale, window, softcap, slopes is not None)
        ctx.save_for_backward(q_bwd, k_bwd, v_bwd, o_bwd, L, cu_q, cu_k, *(() if slopes is None else (slopes,)))
        return o

    @staticmethod
    @torch.no_grad()
    def backward(ctx, do):
        max_q, max_k, D, flags, scale, window, softcap, has_slopes = ctx.args
        q, k, v, o, L, cu_q, cu_k = ctx.saved_tensors[:7]
        slopes = ctx.saved_tensors[7] if has_slopes else None
        dQ, dK, dV = flash_attn_wmma.backward_varlen(q, k, v, o, do, L, cu_q, cu_k, max_q, max_k, D, flags, scale, window, scoremod=(softcap, slopes))
        return dQ, dK, dV, None, None, None, None, None, None, None, None, None


_LN2 = 0.6931471805599453


def _dlse_log2(dlse):
    """The gradient of the natural-log LSE the operator returned -> the C-ABI's dlse: f32, in log2 units (g * ln 2), rows contiguous, strides >= 0."""
    g = dlse.to(torch.float32) * _LN2          # (a fresh tensor: an expanded gradient, e.g. of lse.sum(), becomes a dense one here)
    return g if g.stride(-1) == 1 or g.size(-1) <= 1 else g.contiguous()


def _lse_forward(q, k, v, mask, slopes, causal, scale, BNHD_fmt, window, dropout, softcap):
    """The forward of flash_attention(return_lse=True): the family's forward flagged FA2_FLAG_EXACT_SCALE -> the 6-tensor return and the natural-log LSE
    [B, H, Nq], sliced out of the row-padded L.  window None: the plain / masked call; a triple: the windowed / dropout / score-modifier call."""
    D = q.shape[3]
    Br = 32 if D > 384 else 64                      # FlashAttn.py:56-67
    flags = (_fa2_lib.FA2_FLAG_CAUSAL if causal else 0) | _fa2_lib.FA2_FLAG_EXACT_SCALE
    smod = (softcap, slopes) if (softcap or slopes is not None) else None
    if window is None:
        ret = flash_attn_wmma.forward_py(q, k, v, Br, 128, flags, scale, BNHD_fmt, bias=mask)
    elif dropout is None and smod is None:
        ret = flash_attn_wmma.forward_window(q, k, v, Br, 128, flags, scale, BNHD_fmt, window)
    else:
        ret = flash_attn_wmma.forward_py(q, k, v, Br, 128, flags, scale, BNHD_fmt, window=window, dropout=dropout, scoremod=smod)
    n = q.shape[1 if BNHD_fmt else 2]
    return ret, ret[5][:, :, :n] * _LN2


class _LseAttentionFunction(torch.autograd.Function):
    """autograd node of flash_attention(return_lse=True), every route: outputs (out, lse), backward takes (dO, dLSE) — either may be None — and runs the
    family's *_lse backward (fa2_bwd_lse / fa2_bwd_window_lse).  A missing dLSE passes no dlse: exactly the family's backward of today."""

    @staticmethod
    @torch.no_grad()
    def forward(ctx, q, k, v, mask, slopes, causal, scale, BNHD_fmt, window, dropout, softcap):
        ctx.set_materialize_grads(False)
        if mask is not None and q.shape[3] > _MAX_MASKED_BWD_HEAD_DIM:
            raise RuntimeError("fa2: a masked attention call that needs gradients supports head dims up to %d (got %d): fa2_bwd_bias has no kernel above"
                               % (_MAX_MASKED_BWD_HEAD_DIM, q.shape[3]))
        (o, q_bwd, k_bwd, v_bwd, o_bwd, L), lse = _lse_forward(q, k, v, mask, slopes, causal, scale, BNHD_fmt, window, dropout, softcap)
        n_ax = 1 if BNHD_fmt else 2
        ctx.args = (causal, scale, q.shape[n_ax], k.shape[n_ax], q.shape[3], BNHD_fmt, window, dropout, softcap, mask is not None, slopes is not None)
        ctx.save_for_backward(q_bwd, k_bwd, v_bwd, o_bwd, L, *(t for t in (mask, slopes) if t is not None))
        return o, lse

    @staticmethod
    @torch.no_grad()
    def backward(ctx, do, dlse):
        causal, scale, N, Nkv, D, BNHD_fmt, window, dropout, softcap, has_mask, has_slopes = ctx.args
        q, k, v, o, L = ctx.saved_tensors[:5]
        mask = ctx.saved_tensors[5] if has_mask else None
        slopes = ctx.saved_tensors[5 + has_mask] if has_slopes else None
        if do is None:
            do = torch.zeros_like(q)                # (the kernels read a dO; dLSE alone is the rare case)
        smod = (softcap, slopes) if (softcap or slopes is not None) else None
        dQ, dK, dV = flash_attn_wmma.backward_py(q, k, v, o, do, L, N, Nkv, D, 128, 128, causal, scale, BNHD_fmt, bias=mask, window=window, dropout=dropout,
                                                 scoremod=smod, dlse=dlse)
        return dQ, dK, dV, None, None, None, None, None, None, None, None


class _VarlenLseAttentionFunction(torch.autograd.Function):
    """autograd node of flash_attention_varlen(return_lse=True): outputs (out, lse [H, total_q]), backward = fa2_bwd_varlen_lse."""

    @staticmethod
    @torch.no_grad()
    def forward(ctx, q, k, v, slopes, cu_q, cu_k, max_q, max_k, flags, scale, window, dropout, softcap):
        ctx.set_materialize_grads(False)
        smod = (softcap, slopes) if (softcap or slopes is not None) else None
        o, q_bwd, k_bwd, v_bwd, o_bwd, L = flash_attn_wmma.forward_varlen(q, k, v, cu_q, cu_k, max_q, max_k, flags | _fa2_lib.FA2_FLAG_EXACT_SCALE, scale, window,
                                                                          dropout, smod)
        ctx.args = (max_q, max_k, q.shape[2], flags, scale, window, dropout, softcap, slopes is not None)
        ctx.save_for_backward(q_bwd, k_bwd, v_bwd, o_bwd, L, cu_q, cu_k, *(() if slopes is None else (slopes,)))
        return o, L * _LN2

    @staticmethod
    @torch.no_grad()
    def backward(ctx, do, dlse):
        max_q, max_k, D, flags, scale, window, dropout, softcap, has_slopes = ctx.args
        q, k, v, o, L, cu_q, cu_k = ctx.saved_tensors[:7]
        slopes = ctx.saved_tensors[7] if has_slopes else None
        if do is None:
            do = torch.zeros_like(q)
        smod = (softcap, slopes) if (softcap or slopes is not None) else None
        dQ, dK, dV = flash_attn_wmma.backward_varlen(q, k, v, o, do, L, cu_q, cu_k, max_q, max_k, D, flags, scale, window, dropout, smod, dlse=dlse)
        return dQ, dK, dV, None, None, None, None, None, None, None, None, None, None


def _flash_attention_lse(q, k, v, mask, causal, scale, BNHD_fmt, window, q_offset, dropout_p, dropout_seed, softcap, alibi_slopes):
    """flash_attention(return_lse=True): the argument checks of every route, then ONE node (or, when nothing needs a gradient, the bare forward)."""
    if not (torch.is_tensor(q) and torch.is_tensor(k) and torch.is_tensor(v)) or q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise RuntimeError("fa2: q, k, v must be 4-D ([B,H,N,D] or [B,N,H,D] with BNHD_fmt)")
    if not q.is_cuda or not k.is_cuda or not v.is_cuda:
        raise RuntimeError("fa2: q, k, v must be on a ROCm device (no CPU path in this operator)")
    h_ax, n_ax = (2, 1) if BNHD_fmt else (1, 2)
    dropout = _parse_dropout(dropout_p, dropout_seed)
    smod = _parse_scoremod(softcap, alibi_slopes, q, q.shape[h_ax], q.shape[0])
    if smod is not None and mask is not None:
        raise ValueError("fa2: flash_attention(mask=..., softcap / alibi_slopes) is not supported: the score modifiers run on the unmasked / windowed kernels only")
    if smod is not None and dropout is not None:
        raise ValueError("fa2: flash_attention(softcap / alibi_slopes, dropout_p > 0) is not supported: the score modifiers do not combine with dropout")
    if dropout is not None and mask is not None:
        raise ValueError("fa2: flash_attention(mask=..., dropout_p > 0) is not supported: dropout runs on the unmasked / windowed kernels only")
    _check_groups(q.shape[h_ax], k.shape[h_ax])
    win = None
    if smod is not None or dropout is not None or window is not None or q_offset != 0:
        win = _fa2_lib.parse_window(window if window is not None else (-1, -1), q_offset)
    if mask is not None:
        if win is not None:                      # the band folded into the mask, as flash_attention does without return_lse
            band = _band_mask(q.shape[n_ax], k.shape[n_ax], win, causal, q.device)
            mask = mask & band if mask.dtype == torch.bool else (mask + torch.zeros_like(band, dtype=mask.dtype)).masked_fill(~band, float("-inf"))
            causal, win = False, None
        if k.shape[h_ax] != q.shape[h_ax]:       # the masked kernels have no grouped form: expanded here, autograd sums dK / dV per group
            g = q.shape[h_ax] // k.shape[h_ax]
            k, v = k.repeat_interleave(g, dim=h_ax), v.repeat_interleave(g, dim=h_ax)
    if scale is None:
        scale = q.shape[3] ** -0.5
    cap, slopes = smod if smod is not None else (0.0, None)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        return _LseAttentionFunction.apply(q, k, v, mask, slopes, bool(causal), scale, BNHD_fmt, win, dropout, cap)
    ret, lse = _lse_forward(q, k, v, mask, slopes, bool(causal), scale, BNHD_fmt, win, dropout, cap)
    return ret[0], lse


class _MergeFunction(torch.autograd.Function):
    """autograd node of merge_attention for up to 16 parts: forward = fa2_merge_fwd, backward = fa2_merge_bwd (natural-log LSEs)."""

    @staticmethod
    @torch.no_grad()
    def forward(ctx, BNHD_fmt, n, *parts):
        ctx.set_materialize_grads(False)
        outs, lses = list(parts[:n]), list(parts[n:])
        d = outs[0].shape[-1]
        d_pad = -d % 8
        if d_pad:
            outs = [torch.nn.functional.pad(t, (0, d_pad)) for t in outs]
        ready = _strides_ok if outs[0].dim() == 4 else (lambda t: _packed_ready(t) is t)
        if any(t.stride() != outs[0].stride() or not ready(t) for t in outs):
            outs = [t.contiguous() for t in outs]
        lses = [t.to(torch.float32) for t in lses]
        if any(t.stride() != lses[0].stride() or (t.stride(-1) != 1 and t.size(-1) > 1) for t in lses):
            lses = [t.contiguous() for t in lses]
        out = torch.empty(outs[0].shape, dtype=outs[0].dtype, device=outs[0].device)
        lse = torch.empty(lses[0].shape, dtype=torch.float32, device=outs[0].device)
        geo = _merge_geometry(outs[0], BNHD_fmt)
        dev = out.device.index
        with torch.cuda.device(dev):
            rc = _fa2_lib.load().fa2_merge_fwd(geo[0], n, _ptr_array(outs), _ptr_array(lses), out.data_ptr(), lse.data_ptr(), *geo[1:],
                                               _merge_s3(outs[0], BNHD_fmt), _merge_s2(lses[0]), _merge_s3(out, BNHD_fmt), _merge_s2(lse),
                                               _fa2_lib.FA2_MERGE_NATURAL_LSE, _raw_stream(dev))
        if rc:
            _fa2_lib.check(rc)
        ctx.args = (BNHD_fmt, n, d)
        ctx.save_for_backward(lse, *outs, *lses)
        return (out[..., :d] if d_pad else out), lse

    @staticmethod
    @torch.no_grad()
    def backward(ctx, dout, dlse):
        BNHD_fmt, n, d = ctx.args
        lse, outs, lses = ctx.saved_tensors[0], ctx.saved_tensors[1:1 + n], ctx.saved_tensors[1 + n:]
        if dout is None:
            dout = torch.zeros_like(outs[0])
        else:
            if dout.dtype != outs[0].dtype:
                dout = dout.to(outs[0].dtype)
            if dout.shape[-1] != outs[0].shape[-1]:
                dout = torch.nn.functional.pad(dout, (0, outs[0].shape[-1] - dout.shape[-1]))
            if not (_strides_ok(dout) if dout.dim() == 4 else _packed_ready(dout) is dout):
                dout = dout.contiguous()
        if dlse is not None:
            dlse = dlse.to(torch.float32)
            if dlse.stride(-1) != 1 or min(dlse.stride()) < 0 or dlse.data_ptr() & 3:
                dlse = dlse.contiguous()
        douts = [torch.empty(outs[0].shape, dtype=outs[0].dtype, device=lse.device) for _ in range(n)]
        dlses = [torch.empty(lse.shape, dtype=torch.float32, device=lse.device) for _ in range(n)]
        geo = _merge_geometry(outs[0], BNHD_fmt)
        dev = lse.device.index
        with torch.cuda.device(dev):
            rc = _fa2_lib.load().fa2_merge_bwd(geo[0], n, _ptr_array(outs), _ptr_array(lses), lse.data_ptr(), dout.data_ptr(),
                                               None if dlse is None else dlse.data_ptr(), _ptr_array(douts), _ptr_array(dlses), *geo[1:],
                                               _merge_s3(outs[0], BNHD_fmt), _merge_s2(lses[0]), _merge_s2(lse), _merge_s3(dout, BNHD_fmt),
                                               None if dlse is None else _merge_s2(dlse), _merge_s3(douts[0], BNHD_fmt), _merge_s2(dlses[0]),
                                               _fa2_lib.FA2_MERGE_NATURAL_LSE, _raw_stream(dev))
        if rc:
            _fa2_lib.check(rc)
        if douts[0].shape[-1] != d:
            douts = [t[..., :d] for t in douts]
        return (None, None, *douts, *dlses)


def _ptr_array(tensors):
    """A host array of device pointers, as fa2_merge_* take them (copied into the kernel's argument block by the library)."""
    return (ctypes.c_void_p * len(tensors))(*(t.data_ptr() for t in tensors))


def _merge_geometry(o, BNHD_fmt):
    """(dtype code, B, H, Nq, D) of a part: [B, H, N, D], [B, N, H, D] with BNHD_fmt, or the packed [total, H, D] (B = 1)."""
    code = _fa2_lib.FA2_DTYPE_F16 if o.dtype == torch.float16 else _fa2_lib.FA2_DTYPE_BF16
    if o.dim() == 3:
        return code, 1, o.shape[1], o.shape[0], o.shape[2]
    return (code, o.shape[0], o.shape[2], o.shape[1], o.shape[3]) if BNHD_fmt else (code, o.shape[0], o.shape[1], o.shape[2], o.shape[3])


def _merge_s3(o, BNHD_fmt):
    st = o.stride()
    if o.dim() == 3:
        return _fa2_lib.strides3(0, st[1], st[0])
    return _fa2_lib.strides3(st[0], st[2], st[1]) if BNHD_fmt else _fa2_lib.strides3(st[0], st[1], st[2])


def _merge_s2(lse):
    st = lse.stride()
    return _fa2_lib.strides2(0, st[0]) if lse.dim() == 2 else _fa2_lib.strides2(st[0], st[1])


_MERGE_MAX_PARTS = 16


def merge_attention(outs, lses, BNHD_fmt=False):
    """Merge attention computed over disjoint pieces of the KV axis: `outs` / `lses` are sequences of equal-shaped tensors as
    flash_attention(..., return_lse=True) returns them — out [B, H, Nq, D] ([B, Nq, H, D] with BNHD_fmt), lse [B, H, Nq] f32 natural-log — or the packed
    forms of flash_attention_varlen ([total_q, H, D] and [H, total_q]).  Returns (out, lse) of the attention over the union of the pieces: per row
    w_k = exp(lse_k - lse), out = sum_k w_k out_k (f32, rounded once), lse = logsumexp_k lse_k.  A row no piece saw (every lse_k = -inf) gives zeros and
    -inf; a piece with lse_k = -inf has weight exactly 0.  One HIP kernel each way (C-ABI fa2_merge_fwd / fa2_merge_bwd, no atomics), differentiable in
    every out and every lse, capturable in a graph.  More than 16 parts are folded in groups of 16 (the operation is associative; each fold rounds its
    out once).  Parts whose strides differ are made contiguous first."""
    outs, lses = list(outs), list(lses)
    if not outs or len(outs) != len(lses):
        raise ValueError("fa2: merge_attention takes as many lses as outs, at least one")
    o0, l0 = outs[0], lses[0]
    if not all(torch.is_tensor(t) for t in outs + lses) or o0.dim() not in (3, 4):
        raise ValueError("fa2: merge_attention takes tensors: outs [B, H, Nq, D] or packed [total_q, H, D], lses [B, H, Nq] or [H, total_q]")
    if not all(t.is_cuda for t in outs + lses):
        raise RuntimeError("fa2: the parts must be on a ROCm device (no CPU path in this operator)")
    if o0.dim() == 3:
        lshape = (o0.shape[1], o0.shape[0])
    else:
        lshape = (o0.shape[0], o0.shape[2], o0.shape[1]) if BNHD_fmt else tuple(o0.shape[:3])
    for o, l in zip(outs, lses):
        if o.shape != o0.shape or o.dtype != o0.dtype or o.device != o0.device or tuple(l.shape) != lshape or l.device != o0.device:
            raise ValueError("fa2: merge_attention: every out must be %s %s and every lse %s on %s" % (tuple(o0.shape), o0.dtype, lshape, o0.device))
    if o0.dtype not in (torch.float16, torch.bfloat16) or o0.shape[-1] > _MAX_HEAD_DIM:
        raise RuntimeError("fa2: merge_attention takes fp16 / bf16 outs of head dim <= %d" % _MAX_HEAD_DIM)
    if o0.numel() == 0:
        return torch.zeros_like(o0), torch.full(lshape, float("-inf"), dtype=torch.float32, device=o0.device)
    while len(outs) > _MERGE_MAX_PARTS:
        o, l = _MergeFunction.apply(BNHD_fmt, _MERGE_MAX_PARTS, *outs[:_MERGE_MAX_PARTS], *lses[:_MERGE_MAX_PARTS])
        outs, lses = [o] + outs[_MERGE_MAX_PARTS:], [l] + lses[_MERGE_MAX_PARTS:]
    return _MergeFunction.apply(BNHD_fmt, len(outs), *outs, *lses)


_DECODE_MAX_ROWS = 64       # Nq * (H / Hkv) query rows per K / V head (four MFMA row tiles)
_DECODE_MAX_SPLITS = 16
_DECODE_ROUTE = "flash_attention_varlen(..., causal=True, bottom_right=True) on packed tensors serves such calls"


def _decode_strides_ok(t, mult=8):
    s0, s1, s2, s3 = t.stride()
    return s3 == 1 and not ((s0 | s1 | s2) & (mult - 1)) and s1 > 0 and not (t.data_ptr() & 15)


def _bnhd_ready(t):
    """A [B, N, heads, D] tensor the serving kernels can address (_packed_ready's rule): itself, or a contiguous copy"""
    return t if _decode_strides_ok(t) else t.contiguous()


_FP8_CACHE = getattr(torch, "float8_e4m3fn", None)
_FP8_OTHERS = tuple(d for d in (getattr(torch, n, None) for n in ("float8_e5m2", "float8_e4m3fnuz", "float8_e5m2fnuz")) if d is not None)


def _cache_format(who, q, k_cache, v_cache, k_descale, v_descale):
    """The cache-format checks flash_attention_decode and kvcache_append share (q: the 16-bit tensor whose dtype is the call's I/O dtype).  -> fp8"""
    if k_cache.dtype in _FP8_OTHERS or v_cache.dtype in _FP8_OTHERS:
        raise ValueError("fa2: %s takes FP8 caches as torch.float8_e4m3fn (OCP e4m3) only: e5m2 and the fnuz formats are not "
                         "served, got %s %s" % (who, k_cache.dtype, v_cache.dtype))
    fp8 = _FP8_CACHE is not None and (k_cache.dtype == _FP8_CACHE or v_cache.dtype == _FP8_CACHE)
    if fp8 and k_cache.dtype != v_cache.dtype:
        raise ValueError("fa2: %s takes k_cache and v_cache of one dtype (both float8_e4m3fn, or both q's dtype), got %s %s"
                         % (who, k_cache.dtype, v_cache.dtype))
    if q.dtype not in (torch.float16, torch.bfloat16) or (not fp8 and (k_cache.dtype != q.dtype or v_cache.dtype != q.dtype)):
        raise ValueError("fa2: %s takes fp16 or bf16 q, k_cache, v_cache of one dtype (or float8_e4m3fn caches), got %s %s %s"
                         % (who, q.dtype, k_cache.dtype, v_cache.dtype))
    if not fp8 and (k_descale is not None or v_descale is not None):
        raise ValueError("fa2: k_descale / v_descale belong to float8_e4m3fn caches; this cache is %s" % k_cache.dtype)
    return fp8


def _dtype_code(t):
    return _fa2_lib.FA2_DTYPE_F16 if t.dtype == torch.float16 else _fa2_lib.FA2_DTYPE_BF16


def _device_index(t):
    return t.device.index if t.device.index is not None else _current_device()


def _bnhd(t):
    """{batch | page, head, row} element strides of a [B, N, heads, D] tensor"""
    s = t.stride()
    return _I64x3(s[0], s[2], s[1])


# A KV cache as the five serving entries of the C-ABI take it (host.cpp's CacheDesc, seen from Python): made by _cache_desc alone, which has checked it.
# k / v: the caches (the copies, on flash_attention_prefill's pad path), D: their head dim; the descales share one stride pair.  The entries order the
# cache's arguments differently, so these come in groups and a call puts the groups in its order: fmt (the format code), ptrs (k, v), tables (cache_seqlens,
# block_table), sizes (capacity, page_size, num_pages), strides (ks, vs), bts (the block table's row stride), descales (kd, vd, their stride pair ds).
_Cache = collections.namedtuple("_Cache", "fp8 capacity page_size num_pages Hkv D k v lens block_table k_descale v_descale fmt ptrs tables sizes strides bts descales")


def _cache_desc(fp8, io, B, k_cache, v_cache, cache_seqlens, block_table, k_descale, v_descale, aux=(), num_splits=None, d_pad=0):
    """The one place a cache is checked and described, behind _cache_format (-> fp8): the lengths, the block table, the page size, the descales, the
    devices and the cache strides.  io: the tensor that sets the device (q, or an append's k), B: the batch size (a packed call: its sequences), aux:
    further tensors that must be on that device (cu_seqlens); num_splits: decode's, checked in its place; d_pad: flash_attention_prefill's pad of the
    head dim, which copies the caches — the stride checks see the copies.  -> _Cache"""
    Hkv = k_cache.shape[2]
    if cache_seqlens.dtype != torch.int32 or tuple(cache_seqlens.shape) != (B,) or not cache_seqlens.is_contiguous():
        raise ValueError("fa2: cache_seqlens must be a contiguous int32 tensor of shape [B] = [%d], got %s %s" % (B, cache_seqlens.dtype, tuple(cache_seqlens.shape)))
    if num_splits is not None and (isinstance(num_splits, bool) or not isinstance(num_splits, int) or not 0 <= num_splits <= _DECODE_MAX_SPLITS):
        raise ValueError("fa2: num_splits is 0 (the library chooses) or 1 .. %d, got %r" % (_DECODE_MAX_SPLITS, num_splits))
    if block_table is None:
        if k_cache.shape[0] != B:
            raise ValueError("fa2: a contiguous cache is [B, Nmax, Hkv, D] with B = %d sequences, got %s (a paged cache needs its block_table)"
                             % (B, tuple(k_cache.shape)))
        capacity, page_size, num_pages = k_cache.shape[1], 0, 0
    else:
        if not torch.is_tensor(block_table) or block_table.dim() != 2 or block_table.dtype != torch.int32 or block_table.shape[0] != B or \
                block_table.shape[1] < 1 or block_table.stride(1) != 1:
            raise ValueError("fa2: block_table must be int32 [B, max_pages] with B = %d sequences and contiguous rows, got %s"
                             % (B, "%s %s" % (block_table.dtype, tuple(block_table.shape)) if torch.is_tensor(block_table) else repr(block_table)))
        capacity, page_size, num_pages = block_table.shape[1], k_cache.shape[1], k_cache.shape[0]
        if page_size < 64 or page_size % 64:
            raise ValueError("fa2: the page size of a paged cache (k_cache.shape[1]) must be a multiple of 64, got %d" % page_size)
        if num_pages < 1:
            raise ValueError("fa2: a paged cache needs at least one page")
    if capacity < 1:
        raise ValueError("fa2: the cache has no key slots")
    descales = tuple(d for d in (k_descale, v_descale) if d is not None)
    for d in descales:
        if not torch.is_tensor(d) or d.dtype != torch.float32 or tuple(d.shape) != (B, Hkv):
            raise ValueError("fa2: k_descale / v_descale must be float32 tensors of shape [B, Hkv] = [%d, %d], got %s"
                             % (B, Hkv, "%s %s" % (d.dtype, tuple(d.shape)) if torch.is_tensor(d) else repr(d)))
    aux = tuple(aux) + ((cache_seqlens,) if block_table is None else (cache_seqlens, block_table)) + descales
    if not all(t.is_cuda for t in (io, k_cache, v_cache) + aux):
        raise RuntimeError("fa2: q (an append: k), the caches, cache_seqlens, cu_seqlens, block_table and the descales must be on a ROCm device (no CPU "
                           "path in this operator)")
    device = io.device
    if any(t.device != device for t in (k_cache, v_cache) + aux):
        raise RuntimeError("fa2: q (an append: k), the caches, cache_seqlens, cu_seqlens, block_table and the descales must be on the same device")
    if d_pad:
        k_cache, v_cache = (torch.nn.functional.pad(t, (0, d_pad)) for t in (k_cache, v_cache))
    if fp8:
        if not _decode_strides_ok(k_cache, 16) or not _decode_strides_ok(v_cache, 16):
            raise ValueError("fa2: float8_e4m3fn k_cache / v_cache need a contiguous head dim, strides that are multiples of 16 elements and 16-byte "
                             "aligned storage")
        if len(descales) == 2 and k_descale.stride() != v_descale.stride():       # the C-ABI takes one stride pair: a device copy, nothing read back
            k_descale, v_descale = k_descale.contiguous(), v_descale.contiguous()
    elif not _decode_strides_ok(k_cache) or not _decode_strides_ok(v_cache):
        raise ValueError("fa2: k_cache / v_cache need a contiguous head dim, strides that are multiples of 8 elements and 16-byte aligned storage")
    d0 = k_descale if k_descale is not None else v_descale
    return _Cache(fp8, capacity, page_size, num_pages, Hkv, k_cache.shape[3], k_cache, v_cache, cache_seqlens, block_table, k_descale, v_descale,
                  _fa2_lib.FA2_CACHE_E4M3 if fp8 else _fa2_lib.FA2_CACHE_16BIT, (k_cache.data_ptr(), v_cache.data_ptr()),
                  (cache_seqlens.data_ptr(), None if block_table is None else block_table.data_ptr()), (capacity, page_size, num_pages),
                  (_bnhd(k_cache), _bnhd(v_cache)), 0 if block_table is None else block_table.stride(0),
                  (None if k_descale is None else k_descale.data_ptr(), None if v_descale is None else v_descale.data_ptr(),
                   None if d0 is None else _fa2_lib.strides2(d0.stride(0), d0.stride(1))))


_APPEND_NAMES = (("kvcache_append", "[B, Nnew, Hkv, D]", "[B, Nnew, H, D]"), ("kvcache_append_varlen", "[total, Hkv, D]", "[total, H, D]"))      # [packed]


def _append_check(packed, k_cache, v_cache, k, v, rotary_cos, rotary_sin, q, fp8):
    """The argument checks of the two appends that concern the new tokens, the rotary tables and q (the caches' own: _cache_format / _cache_desc).
    -> rotary_dim (0: no rotary)"""
    who, layout, q_layout = _APPEND_NAMES[packed]
    if not all(torch.is_tensor(t) and t.dim() == 4 - packed for t in (k, v)) or k.shape != v.shape or k.dtype != v.dtype:
        raise ValueError("fa2: %s takes k and v %s of one shape and dtype, got %s %s" % (who, layout, tuple(getattr(k, "shape", ())), tuple(getattr(v, "shape", ()))))
    shape, cshape = k.shape, k_cache.shape
    Hkv, D = shape[-2], shape[-1]
    if cshape != v_cache.shape or cshape[2] != Hkv or cshape[3] != D:
        raise ValueError("fa2: inconsistent k / k_cache / v_cache shapes %s %s %s" % (tuple(shape), tuple(cshape), tuple(v_cache.shape)))
    if Hkv < 1 or (not packed and (shape[0] < 1 or shape[1] < 1)):                  # (a packed token buffer may be empty)
        raise ValueError("fa2: %s needs %s >= 1, got k %s" % (who, "Hkv" if packed else "B, Nnew, Hkv", tuple(k.shape)))
    if D % (16 if fp8 else 8) or D > 512:
        raise ValueError("fa2: %s serves head dims that are multiples of 8 (float8_e4m3fn caches: of 16) up to 512, got %d" % (who, D))
    rotary_dim = _rotary_check(k, D, rotary_cos, rotary_sin)
    _append_q_check(who, q_layout, q, k, rotary_dim)
    return rotary_dim


def _rotary_check(k, D, rotary_cos, rotary_sin):
    """The rotary tables of an append of new tokens k (uniform or packed) with head dim D -> rotary_dim (0: no rotary)"""
    if (rotary_cos is None) != (rotary_sin is None):
        raise ValueError("fa2: rotary_cos and rotary_sin come together")
    rotary_dim = 0
    if rotary_cos is not None:
        if not all(torch.is_tensor(t) and t.dim() == 2 for t in (rotary_cos, rotary_sin)) or rotary_cos.shape != rotary_sin.shape or rotary_cos.shape[0] < 1:
            raise ValueError("fa2: rotary_cos / rotary_sin must be 2-D tensors [seqlen_ro, rotary_dim / 2] of one shape")
        if rotary_cos.dtype != rotary_sin.dtype or rotary_cos.dtype not in (torch.float32, k.dtype):
            raise ValueError("fa2: rotary_cos / rotary_sin must share one dtype, float32 or the dtype of k (%s), got %s %s"
                             % (k.dtype, rotary_cos.dtype, rotary_sin.dtype))
        rotary_dim = 2 * rotary_cos.shape[1]
        if rotary_dim < 16 or rotary_dim % 16 or rotary_dim > D:
            raise ValueError("fa2: rotary_dim (2 * rotary_cos.shape[1]) must be a multiple of 16 between 16 and the head dim %d, got %d" % (D, rotary_dim))
    return rotary_dim


def _append_q_check(who, layout, q, k, rotary_dim):
    """q of an append of new tokens k: the leading (token) dims of k, H heads with Hkv dividing H, k's dtype and head dim; tables required"""
    if q is None:
        return
    if rotary_dim == 0:
        raise ValueError("fa2: %s takes q to rotate it: q without rotary_cos / rotary_sin has nothing to do" % who)
    if not torch.is_tensor(q) or q.dim() != k.dim() or q.dtype != k.dtype or q.shape[:-2] != k.shape[:-2] or q.shape[-1] != k.shape[-1] or q.shape[-2] < 1 or \
            q.shape[-2] % k.shape[-2]:
        raise ValueError("fa2: %s takes q %s in k's dtype with Hkv dividing H, got %s for k %s"
                         % (who, layout, "%s %s" % (q.dtype, tuple(q.shape)) if torch.is_tensor(q) else repr(q), tuple(k.shape)))


def _rotary_tables(rotary_cos, rotary_sin):
    """The tables as the C-ABI takes them: contiguous rows that start on 16-byte boundaries, one row stride -> cos, sin"""
    per16 = 16 // rotary_cos.element_size()
    rotary_cos, rotary_sin = (t if t.stride(1) == 1 and t.stride(0) % per16 == 0 and not (t.data_ptr() & 15) else t.contiguous() for t in (rotary_cos, rotary_sin))
    if rotary_cos.stride(0) != rotary_sin.stride(0):                   # the C-ABI takes one row stride
        rotary_cos, rotary_sin = rotary_cos.contiguous(), rotary_sin.contiguous()
    return rotary_cos, rotary_sin


def kvcache_append(k_cache, v_cache, k, v, cache_seqlens, block_table=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=True, k_descale=None,
                   v_descale=None, q=None):
    """Append new tokens to a KV cache, in place: the write side of flash_attention_decode (the append and rotary parts of flash_attn_with_kvcache).
    k / v [B, Nnew, Hkv, D] fp16 / bf16; the caches, cache_seqlens, block_table and the descales follow flash_attention_decode's rules (contiguous or
    paged, 16-bit or float8_e4m3fn).  cache_seqlens[b] counts the valid keys INCLUDING the new tokens — the length after the append — so new token i
    is written at key position len_b - Nnew + i, the position decode's query row i has.  A token whose position lies outside the cache, or whose page
    id lies outside the pool, is skipped: nothing is written, nothing is clamped onto a live key, and no content of cache_seqlens / block_table can
    move a write outside the caches.
    rotary_cos / rotary_sin [seqlen_ro, rotary_dim / 2], float32 or k's dtype, rotary_dim a multiple of 16 up to D: new token i of k — and row i of q,
    when q [B, Nnew, H, D] is given — is rotated by table row len_b - Nnew + i (clamped into the table).  rotary_interleaved=True pairs the columns
    (2j, 2j + 1) (GPT-J), False pairs (j, j + rotary_dim / 2) (GPT-NeoX); columns at or beyond rotary_dim and all of v pass through bit for bit.
    float8_e4m3fn caches store rne_e4m3(clamp(y / descale[b, hkv], +-448)) of the f32 value y (NaN -> a NaN code, +-Inf -> +-448, None = 1.0).
    Returns the rotated q (a new tensor; q is not touched) when q and the tables are given, else None.  D: a multiple of 8 (e4m3: of 16) up to 512;
    Nnew has no upper bound (a prefill chunk is a legitimate append).  The host reads no device value: the call can be captured in a graph.
    Not served: cache_batch_idx, cache_leftpad, rotary without an append.  C-ABI fa2_kvcache_append."""
    return _append(False, k_cache, v_cache, k, v, None, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved, k_descale, v_descale, q)


def _check_cu(name, cu):
    if not torch.is_tensor(cu) or cu.dim() != 1 or cu.dtype != torch.int32 or cu.numel() < 2 or not cu.is_contiguous():
        raise ValueError("fa2: %s must be a contiguous 1-D int32 tensor of B + 1 >= 2 row offsets, got %s"
                         % (name, "%s %s" % (cu.dtype, tuple(cu.shape)) if torch.is_tensor(cu) else repr(cu)))
    return cu.numel() - 1


def kvcache_append_varlen(k_cache, v_cache, k, v, cu_seqlens, cache_seqlens, block_table=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=True,
                          k_descale=None, v_descale=None, q=None):
    """Packed (ragged) append to a KV cache, in place: kvcache_append for a batch whose sequences bring different numbers of new tokens — the write side
    of flash_attention_prefill, a continuous-batching step that mixes prefill chunks with decode rows.
    k / v [total, Hkv, D] fp16 / bf16, packed; cu_seqlens int32 [B + 1] on the device: sequence s owns the rows [cu[s], cu[s+1]), Nnew_s may be 0.
    The caches, cache_seqlens [B], block_table and the descales [B, Hkv] follow kvcache_append's rules (contiguous or paged, 16-bit or float8_e4m3fn);
    cache_seqlens[s] counts the valid keys INCLUDING the Nnew_s new tokens, so row cu[s] + i is written at key position len_s - Nnew_s + i, the
    position flash_attention_prefill gives query row i.  rotary_* and q [total, H, D] as in kvcache_append: k — and q — rotated by that position.
    cu[B] < total is legitimate (a token buffer of a fixed, captured size that this step fills partly): rows at or beyond cu[B] belong to no sequence,
    write nothing, and their q rows come back unrotated, bit for bit.  cu_seqlens is device data nobody validated, like the lengths and the block
    table: an array that is not ascending loses tokens, it moves no write outside the caches.  A token whose position lies outside the cache or whose
    page id lies outside the pool is skipped, as in kvcache_append.
    Returns the rotated q (a new tensor) when q and the tables are given, else None.  The host reads no device value: the call can be captured in a
    graph.  Not served: cache_batch_idx, cache_leftpad, rotary without an append.  C-ABI fa2_kvcache_append_varlen."""
    return _append(True, k_cache, v_cache, k, v, cu_seqlens, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved, k_descale, v_descale, q)


def _append(packed, k_cache, v_cache, k, v, cu_seqlens, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved, k_descale, v_descale, q):
    """kvcache_append (packed = False) and kvcache_append_varlen (True): the tensors' ranks and the cache format, then check, then launch"""
    who, layout, _ = _APPEND_NAMES[packed]
    if not all(torch.is_tensor(t) for t in (k_cache, v_cache, k, v, cache_seqlens)) or k_cache.dim() != 4 or v_cache.dim() != 4 or k.dim() != 4 - packed or \
            v.dim() != 4 - packed:
        raise ValueError("fa2: %s takes k / v %s and 4-D k_cache / v_cache ([B, Nmax, Hkv, D], or [num_pages, page_size, Hkv, D] with a block_table)"
                         % (who, layout))
    fp8 = _cache_format(who, k, k_cache, v_cache, k_descale, v_descale)
    B = _check_cu("cu_seqlens", cu_seqlens) if packed else k.shape[0]
    return _append_launch(*_append_prepare(packed, fp8, B, k_cache, v_cache, k, v, cu_seqlens, cache_seqlens, block_table, rotary_cos, rotary_sin,
                                           rotary_interleaved, k_descale, v_descale, q))


def _append_prepare(packed, fp8, B, k_cache, v_cache, k, v, cu_seqlens, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved, k_descale,
                    v_descale, q, lead=None, num_splits=None):
    """Every argument check of an append, and what its launch needs: the cache description, rotary_dim, the tensors and tables as the kernel can address
    them (copies where it cannot), q_out.  Nothing is launched here: a fused call (lead: its q, which then sets the device; num_splits: decode's) runs
    this beside its own checks and _append_launch after all of them, so a call that is refused leaves the caches as they were.
    -> _append_launch's arguments, the cache description first"""
    rotary_dim = _append_check(packed, k_cache, v_cache, k, v, rotary_cos, rotary_sin, q, fp8)
    cache = _cache_desc(fp8, k if lead is None else lead, B, k_cache, v_cache, cache_seqlens, block_table, k_descale, v_descale,
                        aux=(cu_seqlens,) if packed else (), num_splits=num_splits)
    extra = tuple(t for t in (k, v, q, rotary_cos, rotary_sin) if t is not None)
    device = k_cache.device
    if not all(t.is_cuda and t.device == device for t in extra):
        raise RuntimeError("fa2: k, v, q and the rotary tables must be on the ROCm device of the caches")
    ready = _packed_ready if packed else _bnhd_ready
    k, v = ready(k), ready(v)
    q_out = None
    if q is not None:
        q = ready(q)
        q_out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    if rotary_dim:
        rotary_cos, rotary_sin = _rotary_tables(rotary_cos, rotary_sin)
    return cache, packed, B, k, v, cu_seqlens, q, q_out, rotary_dim, rotary_cos, rotary_sin, rotary_interleaved


def _append_launch(cache, packed, B, k, v, cu_seqlens, q, q_out, rotary_dim, cos, sin, rotary_interleaved):
    """The one C call of an append _append_prepare has checked -> q_out (the rotated q, or None)"""
    if packed and k.shape[0] == 0:                   # an empty token buffer: nothing to launch
        return q_out
    lib = _fa2_lib.load()
    code = _dtype_code(k)
    if packed:                                       # ([total, heads, D] and cu_seqlens against [B, Nnew, heads, D]: what the two entries differ in)
        entry, st, cu, sizes, nq = lib.fa2_kvcache_append_varlen, _s2, (cu_seqlens.data_ptr(),), (B, k.shape[0], cache.Hkv, cache.D), ()
    else:
        entry, st, cu, sizes, nq = lib.fa2_kvcache_append, _bnhd, (), (B, cache.Hkv, k.shape[1], cache.D), (k.shape[1] if q is not None else 0,)
    q_args = (None, None, 0, *nq, None, None) if q is None else (q.data_ptr(), q_out.data_ptr(), q.shape[-2], *nq, st(q), st(q_out))
    rotary = (None, None, 0, 0, 0, 0)
    if rotary_dim:
        rotary = (cos.data_ptr(), sin.data_ptr(), _fa2_lib.FA2_DTYPE_F32 if cos.dtype == torch.float32 else code, rotary_dim, cos.shape[0], cos.stride(0))
    dev = _device_index(k)
    with torch.cuda.device(dev):
        rc = entry(code, cache.fmt, k.data_ptr(), v.data_ptr(), *cache.ptrs, *cu, *cache.tables, *sizes, *cache.sizes, st(k), st(v), *cache.strides, cache.bts,
                   *q_args, *rotary, 1 if rotary_interleaved else 0, *cache.descales, _raw_stream(dev))
    _fa2_lib.check(rc)
    return q_out


def flash_attention_decode(q, k_cache, v_cache, cache_seqlens, block_table=None, scale=None, return_lse=False, num_splits=0, k_descale=None,
                           v_descale=None, k=None, v=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=True, window=None, softcap=0.0,
                           alibi_slopes=None):
    """KV-cache decode attention (the flash_attn_with_kvcache shape): a few new query tokens per sequence against a preallocated cache.
    q [B, Nq, H, D] fp16 / bf16.  Contiguous cache: k_cache / v_cache [B, Nmax, Hkv, D].  Paged cache: k_cache / v_cache [num_pages, page_size, Hkv, D]
    with block_table int32 [B, max_pages] on q's device, page_size a multiple of 64.  Strided views are fine (D contiguous, strides multiples of 8
    elements); a q that is not is copied, a cache that is not raises — copying the cache is what this call exists to avoid.
    cache_seqlens: int32 [B] on q's device, the valid keys of each sequence INCLUDING the Nq new tokens (the caller has written their K / V).  The host
    never reads it or the block table: no synchronisation, the call can be captured in a graph, and replaying the graph after either tensor changed in
    place gives the result for the new contents.
    Masking is bottom-right causal per sequence: query row i of sequence b sits at position len_b - Nq + i and sees the keys j <= that position (Nq = 1:
    every valid key).  Rows at a negative position return zeros (lse -inf).  Keys at or beyond len_b and unused pages contribute nothing whatever
    they hold; lengths and page ids are clamped into the cache in-kernel, so wrong ones give a wrong answer, never an out-of-bounds read.
    Hkv divides H; D is 64 or 128; Nq * (H / Hkv) <= 64.  Anything else raises ValueError (longer chunks: flash_attention_varlen).
    Returns o [B, Nq, H, D]; with return_lse=True also lse f32 [B, H, Nq] in natural-log units (merge_attention combines such pairs).
    num_splits: 0 = the library's plan, 1 .. 16 = that many parts per (sequence, K / V head).  Inference only: no backward.
    FP8 caches: k_cache and v_cache may both be torch.float8_e4m3fn (OCP e4m3, gfx950's FP8; not e5m2, not fnuz) in the same two layouts, q staying
    fp16 / bf16.  k_descale / v_descale: float32 [B, Hkv] on q's device (any strides), each optional, None = 1.0; K = float(k_cache) * k_descale[b, hkv],
    V = float(v_cache) * v_descale[b, hkv].  They are device data the host never reads, like cache_seqlens: a captured graph replays correctly after
    they changed in place.  An fp8 cache needs a contiguous head dim, 16-byte aligned storage and strides that are multiples of 16 elements.  A descale
    with a 16-bit cache raises ValueError.  C-ABI fa2_fwd_decode_fp8; o and lse as for a 16-bit cache.
    Append and rotary: with k / v [B, Nq, Hkv, D] given (both, k.shape[1] == Nq) the call first runs kvcache_append — the new tokens' K / V written
    at positions len_b - Nq + i (cache_seqlens already counts them), k and q rotated by rotary_cos / rotary_sin when given, quantised for an e4m3
    cache — and then the decode below on the rotated q, on one stream.  rotary_* without k / v raises ValueError.  With none of the five keywords
    the call makes exactly the launches it made before they existed.
    Window, soft-capping, ALiBi: window = None, an int W or (left, right) as in flash_attention; only `left` is used — row i also needs
    j >= pos_i - left — and a legal `right` has no effect, decode being causal.  A part sweeps only the key tiles that hold a key some row sees:
    keys below len_b - Nq - left contribute nothing whatever they hold (like keys at or beyond len_b), and a page that holds only such keys is never
    addressed, nor its block-table entry read — a server may have freed it.  softcap > 0: s = softcap * tanh(x / softcap) on the descaled, scaled
    score x.  alibi_slopes: float32 [H] or [B, H] on q's device, s -= slope[b, h] * (pos_i - j) with h the QUERY head.  The masks come last; o and
    lse are those of s.  The slopes are device data the host never reads: a captured graph follows slopes changed in place — CONTIGUOUS
    slopes: a non-contiguous tensor is copied once per call, as in flash_attention, and a capture would follow the copy.  window and softcap are
    host values, baked into a capture.  The three combine with each other and with everything above (the append runs first and is unaffected); with
    none of them the call goes to the entries below with the launches it made before.  C-ABI fa2_fwd_decode_window.
    C-ABI fa2_fwd_decode: K and V are read once per K / V head group (the group's rows are the M rows of the MFMA), no atomics."""
    if not all(torch.is_tensor(t) for t in (q, k_cache, v_cache, cache_seqlens)) or q.dim() != 4 or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise ValueError("fa2: flash_attention_decode takes q [B, Nq, H, D] and 4-D k_cache / v_cache ([B, Nmax, Hkv, D], or [num_pages, page_size, Hkv, D] "
                         "with a block_table)")
    if torch.is_grad_enabled() and (q.requires_grad or k_cache.requires_grad or v_cache.requires_grad):
        raise ValueError("fa2: flash_attention_decode is inference only (an input requires grad); " + _DECODE_ROUTE)
    fp8 = _cache_format("flash_attention_decode", q, k_cache, v_cache, k_descale, v_descale)
    fused = k is not None or v is not None
    if not fused and (rotary_cos is not None or rotary_sin is not None):
        raise ValueError("fa2: rotary_cos / rotary_sin rotate the appended tokens: flash_attention_decode takes them together with k and v (rotary without "
                         "an append is not served)")
    B, Nq, H, D = q.shape
    Hkv = k_cache.shape[2]
    if v_cache.shape != k_cache.shape or k_cache.shape[3] != D:
        raise ValueError("fa2: inconsistent q / k_cache / v_cache shapes %s %s %s" % (tuple(q.shape), tuple(k_cache.shape), tuple(v_cache.shape)))
    if B < 1 or Nq < 1 or Hkv < 1 or H % Hkv:
        raise ValueError("fa2: the head count of the cache (%d) must divide the head count of q (%d), and B, Nq >= 1; %s" % (Hkv, H, _DECODE_ROUTE))
    if D not in (64, 128):
        raise ValueError("fa2: flash_attention_decode serves head dims 64 and 128, got %d; %s" % (D, _DECODE_ROUTE))
    if Nq * (H // Hkv) > _DECODE_MAX_ROWS:
        raise ValueError("fa2: flash_attention_decode serves Nq * (H / Hkv) <= %d query rows per K / V head, got %d * %d; %s"
                         % (_DECODE_MAX_ROWS, Nq, H // Hkv, _DECODE_ROUTE))
    window_left = _fa2_lib.parse_window(window)[0]
    scoremod = _parse_scoremod(softcap, alibi_slopes, q, H, B)
    if fused:
        if not all(torch.is_tensor(t) and t.dim() == 4 for t in (k, v)) or k.dtype != q.dtype or k.shape[0] != B or k.shape[1] != Nq:
            raise ValueError("fa2: flash_attention_decode takes k and v together, [B, Nq, Hkv, D] = [%d, %d, %d, %d] in q's dtype: the new tokens are the "
                             "query rows' own (k.shape[1] == Nq); got %s %s" % (B, Nq, Hkv, D, tuple(getattr(k, "shape", ())), tuple(getattr(v, "shape", ()))))
        app = _append_prepare(False, fp8, B, k_cache, v_cache, k, v, None, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved, k_descale,
                              v_descale, q if rotary_cos is not None else None, lead=q, num_splits=num_splits)
        cache = app[0]
    else:
        cache = _cache_desc(fp8, q, B, k_cache, v_cache, cache_seqlens, block_table, k_descale, v_descale, num_splits=num_splits)
    if fused:               # every check lies above: the append launch, then today's call on the rotated q, on one stream, so that decode reads what it wrote
        q_rot = _append_launch(*app)
        q = q if q_rot is None else q_rot
    q = _bnhd_ready(q)
    if scale is None:
        scale = D ** -0.5
    lib = _fa2_lib.load()
    code = _dtype_code(q)
    o = torch.empty((B, Nq, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    dev = _device_index(q)
    with torch.cuda.device(dev):
        stream = _raw_stream(dev)
        banded = window_left >= 0 or scoremod is not None
        if banded:
            need = lib.fa2_fwd_decode_window_workspace_bytes(code, B, H, Hkv, Nq, D, cache.capacity, cache.page_size, num_splits, window_left)
        else:
            need = (lib.fa2_fwd_decode_fp8_workspace_bytes if fp8 else lib.fa2_fwd_decode_workspace_bytes)(code, B, H, Hkv, Nq, D, cache.capacity, cache.page_size,
                                                                                                           num_splits)
        ws = _workspace(need, q.device, dev, stream) if need else None
        if ws is None and _WS_POOL:
            _workspace_unused(dev, stream)
        head = (q.data_ptr(), *cache.ptrs, o.data_ptr(), lse.data_ptr(), *cache.tables, B, H, Hkv, Nq, D, *cache.sizes, _bnhd(q), *cache.strides, _bnhd(o),
                _fa2_lib.strides2(lse.stride(0), lse.stride(1)), cache.bts, float(scale))
        tail = (num_splits, None if ws is None else ws.data_ptr(), need, stream)
        if banded:
            rc = lib.fa2_fwd_decode_window(code, cache.fmt, *head, *cache.descales, window_left,
                                           *_scoremod_args(scoremod if scoremod is not None else (0.0, None)), *tail)
        elif fp8:
            rc = lib.fa2_fwd_decode_fp8(code, *head, *cache.descales, *tail)
        else:
            rc = lib.fa2_fwd_decode(code, *head, *tail)
    _fa2_lib.check(rc)
    return (o, lse * _LN2) if return_lse else o


def _mla_kv4(kv_cache):
    """The latent as a cache of ONE head, K and V at once: _cache_desc checks it as it checks every cache (a head stride of one row keeps its rule quiet)"""
    return (kv_cache if kv_cache.dim() == 3 else kv_cache[:, :, 0]).unsqueeze(2)


_MLA_APPEND_NAMES = (("kvcache_append_mla", "[B, Nnew, 512]", "[B, Nnew, 64]", "[B, Nnew, H, 576]"),
                     ("kvcache_append_mla_varlen", "[total, 512]", "[total, 64]", "[total, H, 576]"))      # [packed]


def _mla_rows_ready(t):
    """New-token rows [.., width] the append can address (last dim contiguous, strides multiples of 8 elements with a positive row stride, 16-byte
    aligned storage — the two slices of one [.., 576] projection output are): themselves, or a contiguous copy"""
    st = t.stride()
    ok = st[-1] == 1 and not any(x & 7 for x in st[:-1]) and st[-2] > 0 and all(x >= 0 for x in st) and not (t.data_ptr() & 15)
    return t if ok else t.contiguous()


def _mla_append_prepare(packed, B, kv_cache, kv_c, k_pe, cu_seqlens, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved, q, lead=None):
    """Every argument check of a latent-cache append and what its launch needs (_append_prepare's split: nothing is launched here, so that the fused
    decode call checks everything before it launches anything).  lead: the fused call's q, which then sets the device.
    -> _mla_append_launch's arguments, the cache description first"""
    who, c_layout, pe_layout, q_layout = _MLA_APPEND_NAMES[packed]
    rank = 3 - packed
    if not all(torch.is_tensor(t) for t in (kv_cache, kv_c, k_pe, cache_seqlens)):
        raise ValueError("fa2: %s takes tensors kv_cache, kv_c %s, k_pe %s and cache_seqlens" % (who, c_layout, pe_layout))
    kv_c, k_pe = (t[..., 0, :] if t.dim() == rank + 1 and t.shape[-2] == 1 else t for t in (kv_c, k_pe))        # a head axis of size 1
    if kv_c.dim() != rank or k_pe.dim() != rank or kv_cache.dim() not in (3, 4) or (kv_cache.dim() == 4 and kv_cache.shape[2] != 1):
        raise ValueError("fa2: %s takes kv_c %s, k_pe %s and a latent kv_cache [B, Nmax, 576] ([num_pages, page_size, 576] with a block_table); a head "
                         "axis, where there is one, has size 1" % (who, c_layout, pe_layout))
    if kv_c.shape[-1] != _MLA_DV or k_pe.shape[-1] != _MLA_D - _MLA_DV or kv_cache.shape[-1] != _MLA_D or kv_c.shape[:-1] != k_pe.shape[:-1]:
        raise ValueError("fa2: %s writes rows of %d columns: %d of kv_c, then %d of k_pe, one row of each per token; got kv_c %s k_pe %s kv_cache %s"
                         % (who, _MLA_D, _MLA_DV, _MLA_D - _MLA_DV, tuple(kv_c.shape), tuple(k_pe.shape), tuple(kv_cache.shape)))
    if kv_c.dtype not in (torch.float16, torch.bfloat16) or k_pe.dtype != kv_c.dtype or kv_cache.dtype != kv_c.dtype:
        raise ValueError("fa2: %s takes fp16 or bf16 kv_c, k_pe and kv_cache of one dtype (e4m3 latents are not served), got %s %s %s"
                         % (who, kv_c.dtype, k_pe.dtype, kv_cache.dtype))
    if not packed and (kv_c.shape[0] < 1 or kv_c.shape[1] < 1):                       # (a packed token buffer may be empty)
        raise ValueError("fa2: %s needs B, Nnew >= 1, got kv_c %s" % (who, tuple(kv_c.shape)))
    rotary_dim = _rotary_check(k_pe, _MLA_D - _MLA_DV, rotary_cos, rotary_sin)
    if rotary_dim not in (0, _MLA_D - _MLA_DV):
        raise ValueError("fa2: %s rotates the whole 64-wide k_pe: rotary_cos / rotary_sin must be [seqlen_ro, 32], got rotary_dim %d" % (who, rotary_dim))
    if q is not None:
        if rotary_dim == 0:
            raise ValueError("fa2: %s takes q to rotate it: q without rotary_cos / rotary_sin has nothing to do" % who)
        if not torch.is_tensor(q) or q.dim() != rank + 1 or q.dtype != kv_c.dtype or q.shape[:-2] != kv_c.shape[:-1] or q.shape[-1] != _MLA_D or \
                not 1 <= q.shape[-2] <= _MLA_MAX_HEADS:
            raise ValueError("fa2: %s takes q %s in kv_c's dtype with 1 .. %d heads, got %s for kv_c %s"
                             % (who, q_layout, _MLA_MAX_HEADS, "%s %s" % (q.dtype, tuple(q.shape)) if torch.is_tensor(q) else repr(q), tuple(kv_c.shape)))
    kv4 = _mla_kv4(kv_cache)
    cache = _cache_desc(False, kv_c if lead is None else lead, B, kv4, kv4, cache_seqlens, block_table, None, None, aux=(cu_seqlens,) if packed else ())
    extra = tuple(t for t in (kv_c, k_pe, q, rotary_cos, rotary_sin) if t is not None)
    device = kv_cache.device
    if not all(t.is_cuda and t.device == device for t in extra):
        raise RuntimeError("fa2: kv_c, k_pe, q and the rotary tables must be on the ROCm device of the cache")
    kv_c, k_pe = _mla_rows_ready(kv_c), _mla_rows_ready(k_pe)
    q_out = None
    if q is not None:
        q = (_packed_ready if packed else _bnhd_ready)(q)
        q_out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    if rotary_dim:
        rotary_cos, rotary_sin = _rotary_tables(rotary_cos, rotary_sin)
    return cache, packed, B, kv_c, k_pe, cu_seqlens, q, q_out, rotary_dim, rotary_cos, rotary_sin, rotary_interleaved


def _mla_append_launch(cache, packed, B, kv_c, k_pe, cu_seqlens, q, q_out, rotary_dim, cos, sin, rotary_interleaved):
    """The one C call of a latent-cache append _mla_append_prepare has checked -> q_out (the rotated q, or None)"""
    if packed and kv_c.shape[0] == 0:                # an empty token buffer: nothing to launch
        return q_out
    lib = _fa2_lib.load()
    code = _dtype_code(kv_c)
    if packed:
        entry, cu, sizes, nq = lib.fa2_kvcache_append_mla_varlen, (cu_seqlens.data_ptr(),), (B, kv_c.shape[0]), ()
        rows, st = (lambda t: (ctypes.c_int64 * 1)(t.stride(0))), _s2
    else:
        entry, cu, sizes, nq = lib.fa2_kvcache_append_mla, (), (B, kv_c.shape[1]), (kv_c.shape[1] if q is not None else 0,)
        rows, st = (lambda t: _I64x2(t.stride(0), t.stride(1))), _bnhd
    q_args = (None, None, 0, *nq, None, None) if q is None else (q.data_ptr(), q_out.data_ptr(), q.shape[-2], *nq, st(q), st(q_out))
    rotary = (None, None, 0, 0, 0, 0)
    if rotary_dim:
        rotary = (cos.data_ptr(), sin.data_ptr(), _fa2_lib.FA2_DTYPE_F32 if cos.dtype == torch.float32 else code, rotary_dim, cos.shape[0], cos.stride(0))
    dev = _device_index(kv_c)
    with torch.cuda.device(dev):
        rc = entry(code, kv_c.data_ptr(), k_pe.data_ptr(), cache.ptrs[0], *cu, *cache.tables, *sizes, _MLA_D, _MLA_DV, *cache.sizes, rows(kv_c), rows(k_pe),
                   cache.strides[0], cache.bts, *q_args, *rotary, 1 if rotary_interleaved else 0, _raw_stream(dev))
    _fa2_lib.check(rc)
    return q_out


def kvcache_append_mla(kv_cache, kv_c, k_pe, cache_seqlens, block_table=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=True, q=None):
    """Append new tokens to a latent (MLA) KV cache, in place: the write side of flash_attention_decode_mla.
    kv_c [B, Nnew, 512] (the compressed KV) and k_pe [B, Nnew, 64] (the rotary key), fp16 / bf16, become ONE cache row of 576 columns per token:
    kv_c bit for bit in columns 0 .. 511, k_pe in columns 512 .. 575.  kv_cache, cache_seqlens and block_table follow flash_attention_decode_mla's
    rules (contiguous [B, Nmax, 576] or paged [num_pages, page_size, 576]); a head axis of size 1 is accepted on kv_c, k_pe and the cache.
    cache_seqlens[b] counts the valid keys INCLUDING the new tokens, so new token i is written at key position len_b - Nnew + i, the position the
    decode call's query row i has.  A token whose position lies outside the cache, or whose page id lies outside the pool, is skipped: nothing is
    written, nothing is clamped onto a live key, and no content of cache_seqlens / block_table can move a write outside the cache.
    rotary_cos / rotary_sin [seqlen_ro, 32], float32 or kv_c's dtype (rotary_dim is exactly 64): k_pe of token i — and the trailing 64 columns of
    row i of q [B, Nnew, H, 576], when q is given — are rotated by table row len_b - Nnew + i (clamped into the table), in f32 with one rounding.
    rotary_interleaved=True pairs the columns (512 + 2j, 512 + 2j + 1), False pairs (512 + j, 512 + 32 + j).  Without tables k_pe is copied bit for
    bit (a caller who rotated it already).  Strided views are fine when the last dim is contiguous, the strides are multiples of 8 elements and the
    storage is 16-byte aligned — the two slices of one [.., 576] projection output go in without a copy; another source is copied, another cache
    raises.  Returns the rotated q (a new tensor; q is not touched; its columns 0 .. 511 bit for bit) when q and the tables are given, else None.
    The host reads no device value: the call can be captured in a graph.  Not served: e4m3 latents, cache_batch_idx, cache_leftpad, rotary without
    an append.  C-ABI fa2_kvcache_append_mla."""
    B = kv_c.shape[0] if torch.is_tensor(kv_c) and kv_c.dim() >= 1 else 0
    return _mla_append_launch(*_mla_append_prepare(False, B, kv_cache, kv_c, k_pe, None, cache_seqlens, block_table, rotary_cos, rotary_sin,
                                                   rotary_interleaved, q))


def kvcache_append_mla_varlen(kv_cache, kv_c, k_pe, cu_seqlens, cache_seqlens, block_table=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=True,
                              q=None):
    """Packed (ragged) append to a latent (MLA) KV cache, in place: kvcache_append_mla for a batch whose sequences bring different numbers of new tokens.
    kv_c [total, 512], k_pe [total, 64] and q [total, H, 576], packed; cu_seqlens int32 [B + 1] on the device: sequence s owns the rows
    [cu[s], cu[s + 1]), Nnew_s may be 0; row cu[s] + i is written at key position len_s - Nnew_s + i.  cu[B] < total is legitimate (a token buffer of a
    fixed, captured size that this step fills partly): rows at or beyond cu[B] belong to no sequence, write nothing, and their q rows come back
    unrotated, bit for bit.  cu_seqlens is device data nobody validated, like the lengths and the block table: an array that is not ascending loses
    tokens, it moves no write outside the cache.  Everything else is kvcache_append_mla's.  C-ABI fa2_kvcache_append_mla_varlen."""
    B = _check_cu("cu_seqlens", cu_seqlens)
    return _mla_append_launch(*_mla_append_prepare(True, B, kv_cache, kv_c, k_pe, cu_seqlens, cache_seqlens, block_table, rotary_cos, rotary_sin,
                                                   rotary_interleaved, q))


_MLA_D, _MLA_DV, _MLA_MAX_HEADS, _MLA_MAX_ROWS, _MLA_MAX_SPLITS = 576, 512, 128, 512, 128      # csrc/fa2_decode_mla.hip.h (the split cap: the plan reports it)


def flash_attention_decode_mla(q, kv_cache, cache_seqlens, block_table=None, head_dim_v=512, scale=None, return_lse=False, num_splits=0, kv_c=None, k_pe=None,
                               rotary_cos=None, rotary_sin=None, rotary_interleaved=True):
    """Decode attention on a multi-head-latent (MLA) KV cache — the decode step of DeepSeek-V2 / V3 / R1 and Kimi K2 with the up-projections absorbed
    into the query and the output (the flash_mla_with_kvcache shape).
    q [B, Nq, H, 576] fp16 / bf16: the absorbed query, q_nope . W_UK in columns 0 .. 511 and the rotated q_pe in columns 512 .. 575.  A q the kernel
    cannot address (last dim not contiguous, strides no multiples of 8 elements, storage not 16-byte aligned) is copied, as in flash_attention_decode.
    kv_cache, in q's dtype: one latent row of 576 columns per token, shared by all heads — 512 of compressed KV, then 64 of rotary key; its first 512
    columns are also the value.  Contiguous: [B, Nmax, 576].  Paged: [num_pages, page_size, 576] with block_table int32 [B, max_pages] on q's device,
    page_size a multiple of 64.  A 4-D cache with a head axis of size 1 ([.., .., 1, 576]) is accepted in both forms.  Strided views are fine; a cache
    the kernel cannot address raises — it is never copied.
    cache_seqlens: int32 [B] on q's device, the valid keys of each sequence INCLUDING the Nq new tokens.  The host reads neither it nor the block
    table: the call can be captured in a graph and replayed as they change in place.
    o[b, i, h] = softmax_j(scale * q[b, i, h, :] . kv[b, j, :]) . kv[b, j, :512] under decode's mask, bottom-right causal: row i sits at position
    len_b - Nq + i.  Rows at a negative position return zeros (lse -inf).  Keys at or beyond len_b and unused pages contribute nothing whatever they
    hold, NaN included; lengths and page ids are clamped in-kernel: a wrong one gives a wrong answer, never an out-of-bounds access.
    scale: None = 576 ** -0.5 (FlashMLA's default).  DeepSeek callers pass their own: the softmax scale of the NON-absorbed head dim (192 ** -0.5, times
    the YaRN mscale factor where the model has one).
    head_dim_v must be 512 and q.shape[-1] 576; H is 1 .. 128 and Nq * H <= 512 (TP8's 16 heads up to all 128, with a few speculative tokens).
    Anything else raises ValueError.  Returns o [B, Nq, H, 512]; with return_lse=True also lse f32 [B, H, Nq] in natural-log units (merge_attention
    composes with it).  num_splits: 0 = the library's plan, 1 .. 128 = that many parts per (sequence, block of 64 rows).  Inference only.
    kv_c [B, Nq, 512] and k_pe [B, Nq, 64] (both or neither): the query rows' own new tokens, appended first by kvcache_append_mla's rules —
    cache_seqlens counts them already — with rotary_cos / rotary_sin [seqlen_ro, 32] rotating k_pe and the trailing 64 columns of q by each row's
    position; the attention then reads the rotated q.  Every check of both halves runs before the first launch, so a call that is refused leaves the
    cache as it was; the two launches share q's stream.  rotary_* without kv_c / k_pe raises (rotary without an append is not served).  With none of
    the five the call makes exactly the launches it made before.  Standalone: kvcache_append_mla, kvcache_append_mla_varlen.
    C-ABI fa2_fwd_decode_mla: each cache row is fetched once per workgroup and used as K and as V for up to 64 (token, head) rows; no atomics."""
    who = "flash_attention_decode_mla"
    if not all(torch.is_tensor(t) for t in (q, kv_cache, cache_seqlens)) or q.dim() != 4 or kv_cache.dim() not in (3, 4) or \
            (kv_cache.dim() == 4 and kv_cache.shape[2] != 1):
        raise ValueError("fa2: %s takes q [B, Nq, H, 576] and a latent kv_cache [B, Nmax, 576] ([num_pages, page_size, 576] with a block_table); a 4-D "
                         "cache has a head axis of size 1" % who)
    if torch.is_grad_enabled() and (q.requires_grad or kv_cache.requires_grad):
        raise ValueError("fa2: %s is inference only (an input requires grad)" % who)
    if isinstance(head_dim_v, bool) or head_dim_v != _MLA_DV or q.shape[3] != _MLA_D or kv_cache.shape[-1] != _MLA_D:
        raise ValueError("fa2: %s serves latent rows of %d columns whose first %d are the value (head_dim_v), got q %s kv_cache %s head_dim_v=%r"
                         % (who, _MLA_D, _MLA_DV, tuple(q.shape), tuple(kv_cache.shape), head_dim_v))
    if q.dtype not in (torch.float16, torch.bfloat16) or kv_cache.dtype != q.dtype:
        raise ValueError("fa2: %s takes fp16 or bf16 q and kv_cache of one dtype, got %s %s" % (who, q.dtype, kv_cache.dtype))
    B, Nq, H, D = q.shape
    if B < 1 or Nq < 1 or not 1 <= H <= _MLA_MAX_HEADS or Nq * H > _MLA_MAX_ROWS:
        raise ValueError("fa2: %s serves 1 .. %d heads and Nq * H <= %d query rows (B, Nq >= 1), got q %s" % (who, _MLA_MAX_HEADS, _MLA_MAX_ROWS, tuple(q.shape)))
    if isinstance(num_splits, bool) or not isinstance(num_splits, int) or not 0 <= num_splits <= _MLA_MAX_SPLITS:
        raise ValueError("fa2: num_splits is 0 (the library chooses) or 1 .. %d, got %r" % (_MLA_MAX_SPLITS, num_splits))
    fused = kv_c is not None or k_pe is not None
    if not fused and (rotary_cos is not None or rotary_sin is not None):
        raise ValueError("fa2: rotary_cos / rotary_sin rotate the appended tokens: %s takes them together with kv_c and k_pe (rotary without an append is "
                         "not served)" % who)
    if fused:
        if not all(torch.is_tensor(t) and t.dim() in (3, 4) for t in (kv_c, k_pe)) or tuple(kv_c.shape[:2]) != (B, Nq) or tuple(k_pe.shape[:2]) != (B, Nq):
            raise ValueError("fa2: %s takes kv_c and k_pe together, [B, Nq, 512] and [B, Nq, 64] = [%d, %d, ..] in q's dtype: the new tokens are the query "
                             "rows' own (shape[1] == Nq); got %s %s" % (who, B, Nq, tuple(getattr(kv_c, "shape", ())), tuple(getattr(k_pe, "shape", ()))))
        app = _mla_append_prepare(False, B, kv_cache, kv_c, k_pe, None, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved,
                                  q if rotary_cos is not None else None, lead=q)
        cache = app[0]
        q_rot = _mla_append_launch(*app)      # every check lies above: the append launch, then today's call on the rotated q, on one stream
        q = q if q_rot is None else q_rot
    else:
        cache = _cache_desc(False, q, B, _mla_kv4(kv_cache), _mla_kv4(kv_cache), cache_seqlens, block_table, None, None)
    q = _bnhd_ready(q)
    if scale is None:
        scale = _MLA_D ** -0.5
    lib = _fa2_lib.load()
    code = _dtype_code(q)
    o = torch.empty((B, Nq, H, _MLA_DV), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    dev = _device_index(q)
    with torch.cuda.device(dev):
        stream = _raw_stream(dev)
        need = lib.fa2_fwd_decode_mla_workspace_bytes(code, B, H, Nq, _MLA_D, _MLA_DV, cache.capacity, cache.page_size, num_splits)
        ws = _workspace(need, q.device, dev, stream) if need else None
        if ws is None and _WS_POOL:
            _workspace_unused(dev, stream)
        rc = lib.fa2_fwd_decode_mla(code, q.data_ptr(), cache.ptrs[0], o.data_ptr(), lse.data_ptr(), *cache.tables, B, H, Nq, _MLA_D, _MLA_DV, *cache.sizes,
                                    _bnhd(q), cache.strides[0], _bnhd(o), _fa2_lib.strides2(lse.stride(0), lse.stride(1)), cache.bts, float(scale),
                                    num_splits, None if ws is None else ws.data_ptr(), need, stream)
    _fa2_lib.check(rc)
    return (o, lse * _LN2) if return_lse else o


def flash_attention_prefill(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table=None, max_seqlen_q=None, scale=None, window=None, softcap=0.0,
                            alibi_slopes=None, return_lse=False, k_descale=None, v_descale=None, k=None, v=None, rotary_cos=None, rotary_sin=None,
                            rotary_interleaved=True):
    """Chunked prefill against a KV cache: many query rows per sequence (packed, as flash_attention_varlen's) against the cache kvcache_append writes and
    flash_attention_decode reads — a prompt whose prefix sits in cached pages, a prompt processed in chunks, a continuous-batching step that mixes
    prefill chunks with decode rows (other libraries: flash_attn_varlen_func(..., block_table=), flash_attn_with_kvcache with a long seqlen_q).
    q [total_q, H, D] fp16 / bf16; cu_seqlens_q int32 [B + 1] on q's device: sequence s owns the rows [cu[s], cu[s+1]), Nq_s may be 0, 1 or thousands.
    k_cache / v_cache: flash_attention_decode's two 16-bit layouts — [B, Nmax, Hkv, D], or [num_pages, page_size, Hkv, D] with block_table int32
    [B, max_pages], page_size a multiple of 64 (a pool may exceed 4 GiB).  Strided views are fine; a cache that is not addressable raises.
    cache_seqlens: int32 [B] on q's device, the valid keys of each sequence INCLUDING its Nq_s new tokens (the caller has written their K / V, with
    kvcache_append or otherwise).  The host never reads it or the block table, and no maximum key length is asked for: the call can be captured in
    a graph and replayed after lengths, table and cache contents changed in place.
    max_seqlen_q: a host int >= every Nq_s; it sizes the grid.  None computes it from cu_seqlens_q, which is a device-to-host SYNCHRONISATION (and
    cannot be captured) — pass it in a hot loop.  A sequence longer than the stated maximum is the caller's error: its extra rows are not computed.
    Masking is decode's, bottom-right causal per sequence: row i of sequence s sits at position len_s - Nq_s + i and sees the keys j <= that position;
    window = None, an int W or (left, right): only `left` acts (j >= pos - left).  softcap / alibi_slopes (float32 [H] or [B, H]) as in
    flash_attention_decode, positions as above.  Rows at a negative position (Nq_s > len_s) return zeros and lse = -inf.  Keys at or beyond len_s and
    unused pages contribute nothing whatever they hold; lengths and page ids are clamped into the cache in-kernel (a wrong one gives a wrong answer,
    never an out-of-bounds read); a page that holds no key a workgroup's rows see is never addressed, nor its block-table entry read.
    Returns o [total_q, H, D]; with return_lse=True also lse f32 [H, total_q] in natural-log units (merge_attention combines such pairs).
    Inference only.  Head dims up to 512; one that is no multiple of 8 is zero-padded — q AND both caches, i.e. copies of the caches.
    Append and rotary: with k / v [total_q, Hkv, D] given (both) the call first runs kvcache_append_varlen with cu_seqlens_q as its cu_seqlens — the
    new tokens' K / V written at positions len_s - Nq_s + i, k and q rotated by rotary_cos / rotary_sin when given — and then the call above on the
    rotated q, on one stream: with the lengths incremented in place before it, a whole ragged serving step is one capturable sequence.  The append
    serves head dims that are multiples of 8.  rotary_* without k / v raises ValueError.  Every argument check of this function and of
    kvcache_append_varlen runs before the append launch, so a call they refuse leaves the caches as they were; what only the C entry refuses after that
    (a window or a grid beyond its limits) leaves caches that hold the new tokens.  With none of the five keywords the call makes exactly the launches it
    made before they existed.
    float8_e4m3fn caches and k_descale / v_descale raise ValueError: 16-bit caches only (flash_attention_prefill_fp8 serves e4m3 caches).
    C-ABI fa2_fwd_prefill."""
    who = "flash_attention_prefill"
    _prefill_tensors(who, q, k_cache, v_cache, cu_seqlens_q, cache_seqlens)
    if _cache_format(who, q, k_cache, v_cache, None, None) or k_descale is not None or v_descale is not None:
        raise ValueError("fa2: %s serves 16-bit caches only (fp16 / bf16, q's dtype): float8_e4m3fn caches and k_descale / v_descale are "
                         "flash_attention_decode's" % who)
    return _prefill(who, False, q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, max_seqlen_q, scale, window, softcap, alibi_slopes,
                    return_lse, None, None, k, v, rotary_cos, rotary_sin, rotary_interleaved)


_PREFILL_FP8_MAX_D = 256        # the largest head dim fa2_fwd_prefill_fp8 has a kernel for (the head-dim-512 one would need scratch memory)


def flash_attention_prefill_fp8(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table=None, max_seqlen_q=None, scale=None, window=None, softcap=0.0,
                                alibi_slopes=None, return_lse=False, k_descale=None, v_descale=None, k=None, v=None, rotary_cos=None, rotary_sin=None,
                                rotary_interleaved=True):
    """flash_attention_prefill against a float8_e4m3fn KV cache — the cache kvcache_append_varlen quantises into and flash_attention_decode reads — so a
    server that keeps its cache in e4m3 uses cached prefix pages, chunks a prompt and mixes prefill chunks with decode rows without dequantising a copy.
    Everything is flash_attention_prefill's, with K = float(k_cache) * k_descale[s, hkv] and V = float(v_cache) * v_descale[s, hkv]; what differs:
    k_cache / v_cache must both be torch.float8_e4m3fn (OCP e4m3; e5m2, the fnuz formats and 16-bit caches raise ValueError) with a contiguous head dim,
    16-byte aligned storage and strides that are multiples of 16 elements (flash_attention_decode's rules for e4m3).  q stays fp16 / bf16.
    k_descale / v_descale: float32 [B, Hkv] on q's device, each optional, None = 1.0.  They are device data the host never reads, like cache_seqlens: a
    captured graph replays correctly after they changed in place.  softcap caps the descaled, scaled score; o and lse are those of the descaled K / V.
    D must be a multiple of 16, at most 256: there is no padding path (it would copy the caches), and no kernel above 256.
    Append: with k / v [total_q, Hkv, D] (fp16 / bf16) the call first runs kvcache_append_varlen with the same descales — which quantises the new tokens
    into the cache — and then attends, on one stream; every argument check of both runs before the first launch.
    With descales that are null or powers of two in [1/8, 8] the result equals flash_attention_prefill's on the dequantised 16-bit cache bit for bit.
    C-ABI fa2_fwd_prefill_fp8."""
    who = "flash_attention_prefill_fp8"
    _prefill_tensors(who, q, k_cache, v_cache, cu_seqlens_q, cache_seqlens)
    if not _cache_format(who, q, k_cache, v_cache, k_descale, v_descale):
        raise ValueError("fa2: %s serves float8_e4m3fn caches only, got %s %s: 16-bit caches are flash_attention_prefill's" % (who, k_cache.dtype, v_cache.dtype))
    return _prefill(who, True, q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, max_seqlen_q, scale, window, softcap, alibi_slopes,
                    return_lse, k_descale, v_descale, k, v, rotary_cos, rotary_sin, rotary_interleaved)


def _prefill_tensors(who, q, k_cache, v_cache, cu_seqlens_q, cache_seqlens):
    """The first two checks of the prefill calls: the tensors' ranks, and inference only"""
    if not all(torch.is_tensor(t) for t in (q, k_cache, v_cache, cu_seqlens_q, cache_seqlens)) or q.dim() != 3 or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise ValueError("fa2: %s takes q [total_q, H, D], 4-D k_cache / v_cache ([B, Nmax, Hkv, D], or [num_pages, page_size, Hkv, D] with a "
                         "block_table), cu_seqlens_q and cache_seqlens" % who)
    if torch.is_grad_enabled() and (q.requires_grad or k_cache.requires_grad or v_cache.requires_grad):
        raise ValueError("fa2: %s is inference only (an input requires grad); flash_attention_varlen on packed keys is differentiable" % who)


def _prefill(who, fp8, q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, max_seqlen_q, scale, window, softcap, alibi_slopes, return_lse,
             k_descale, v_descale, k, v, rotary_cos, rotary_sin, rotary_interleaved):
    """flash_attention_prefill (fp8 = False: 16-bit caches, no descales) and flash_attention_prefill_fp8 (fp8 = True) behind their cache-format checks:
    the argument checks both share, the fused append, the launch."""
    fused = k is not None or v is not None
    if not fused and (rotary_cos is not None or rotary_sin is not None):
        raise ValueError("fa2: rotary_cos / rotary_sin rotate the appended tokens: %s takes them together with k and v (rotary without an append is "
                         "not served)" % who)
    total_q, H, D = q.shape
    Hkv = k_cache.shape[2]
    if v_cache.shape != k_cache.shape or k_cache.shape[3] != D:
        raise ValueError("fa2: inconsistent q / k_cache / v_cache shapes %s %s %s" % (tuple(q.shape), tuple(k_cache.shape), tuple(v_cache.shape)))
    _check_groups(H, Hkv)
    if D < 1 or D > _MAX_HEAD_DIM:
        raise ValueError("fa2: %s serves head dims 1 .. %d, got %d" % (who, _MAX_HEAD_DIM, D))
    if fp8 and (D % 16 or D > _PREFILL_FP8_MAX_D):
        raise ValueError("fa2: %s serves head dims that are multiples of 16 up to %d (no padding path: it would copy the caches), got %d"
                         % (who, _PREFILL_FP8_MAX_D, D))
    if fused:
        if not all(torch.is_tensor(t) and t.dim() == 3 and t.dtype == q.dtype and tuple(t.shape) == (total_q, Hkv, D) for t in (k, v)):
            raise ValueError("fa2: %s takes k and v together, [total_q, Hkv, D] = [%d, %d, %d] in q's dtype: the new tokens are the query rows' own "
                             "(k.shape[0] == total_q); got %s %s" % (who, total_q, Hkv, D, tuple(getattr(k, "shape", ())), tuple(getattr(v, "shape", ()))))
        if D % 8:
            raise ValueError("fa2: %s appends k / v at head dims that are multiples of 8 (kvcache_append_varlen's), got %d" % (who, D))
    B = _check_cu("cu_seqlens_q", cu_seqlens_q)
    if max_seqlen_q is not None and (isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int) or max_seqlen_q < 0):
        raise ValueError("fa2: max_seqlen_q is None or a non-negative int, got %r" % (max_seqlen_q,))
    window_left = _fa2_lib.parse_window(window)[0]
    scoremod = _parse_scoremod(softcap, alibi_slopes, q, H, B)
    d_pad = 0 if fp8 else -D % 8   # (0 in a fused call: its check above)
    if fused:
        app = _append_prepare(True, fp8, B, k_cache, v_cache, k, v, cu_seqlens_q, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved,
                              k_descale, v_descale, q if rotary_cos is not None else None, lead=q)
        cache = app[0]
    else:
        cache = _cache_desc(fp8, q, B, k_cache, v_cache, cache_seqlens, block_table, k_descale, v_descale, aux=(cu_seqlens_q,), d_pad=d_pad)
    if d_pad:
        q = torch.nn.functional.pad(q, (0, d_pad))
    if max_seqlen_q is None:
        max_seqlen_q = int((cu_seqlens_q[1:] - cu_seqlens_q[:-1]).max())
    if scale is None:
        scale = D ** -0.5
    if fused:               # every check lies above: the packed append launch, then today's call on the rotated q, on one stream
        if not math.isfinite(float(scale)):
            raise ValueError("fa2: %s needs a finite scale, got %r" % (who, scale))
        q_rot = _append_launch(*app)
        q = q if q_rot is None else q_rot
    q = _packed_ready(q)
    o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    lse = torch.empty((H, total_q), dtype=torch.float32, device=q.device)
    if total_q and max_seqlen_q > 0:
        lib = _fa2_lib.load()
        code = _dtype_code(q)
        dev = _device_index(q)
        head = (q.data_ptr(), *cache.ptrs, o.data_ptr(), lse.data_ptr(), cu_seqlens_q.data_ptr(), *cache.tables, B, H, Hkv, int(max_seqlen_q), cache.D,
                *cache.sizes, _s2(q), *cache.strides, _s2(o), lse.stride(0), cache.bts, float(scale))
        with torch.cuda.device(dev):
            tail = (window_left, *_scoremod_args(scoremod if scoremod is not None else (0.0, None)), _raw_stream(dev))
            if fp8:
                rc = lib.fa2_fwd_prefill_fp8(code, *head, *cache.descales, *tail)
            else:
                rc = lib.fa2_fwd_prefill(code, cache.fmt, *head, *tail)
        _fa2_lib.check(rc)
    elif total_q:                  # (a stated maximum of 0: no row is computed)
        o.zero_()
        lse.fill_(float("-inf"))
    out = o[..., :D] if d_pad else o
    return (out, lse * _LN2) if return_lse else out


SOFTCAP_MESSAGE = "fa2: softcap must be 0 (off) or a finite positive number (a normal float32: >= 1.18e-38)"
_SOFTCAP_MIN = 2.0 ** -126          # the smallest normal float32: below it 1 / softcap overflows (the library answers FA2_ERR_SOFTCAP)
ALIBI_MESSAGE = "fa2: alibi_slopes must be a float32 tensor on q's device, shaped [H] or [B, H] (packed calls: [H] or [num_sequences, H])"


def _parse_scoremod(softcap, alibi_slopes, q, h, nb):
    """The operator's softcap / alibi_slopes arguments -> None (both off) or (softcap, slopes).  h: query heads, nb: batches (packed calls: sequences).
    Raises ValueError before any device work."""
    try:
        cap = float(softcap)
    except (TypeError, ValueError):
        raise ValueError(SOFTCAP_MESSAGE + ", got %r" % (softcap,))
    if isinstance(softcap, bool) or not (cap == 0.0 or _SOFTCAP_MIN <= cap <= 3.0e38):           # (NaN fails the comparisons)
        raise ValueError(SOFTCAP_MESSAGE + ", got %r" % (softcap,))
    if alibi_slopes is not None:
        a = alibi_slopes
        if not torch.is_tensor(a) or a.dtype != torch.float32 or a.device != q.device or tuple(a.shape) not in ((h,), (nb, h)):
            got = "%s %s on %s" % (tuple(a.shape), a.dtype, a.device) if torch.is_tensor(a) else repr(a)
            raise ValueError(ALIBI_MESSAGE + "; H = %d, B = %d, q on %s, got %s" % (h, nb, q.device, got))
    if cap == 0.0 and alibi_slopes is None:
        return None
    if alibi_slopes is not None and not alibi_slopes.is_contiguous():
        alibi_slopes = alibi_slopes.contiguous()       # once, here: this is the tensor the launches read and the autograd node saves for the backward
    return (cap, alibi_slopes)


def _scoremod_args(scoremod):
    """(softcap, slopes) -> the three trailing arguments of the C-ABI's score-modifier entry points."""
    cap, a = scoremod
    if a is None:
        return (float(cap), None, 0)
    if not a.is_contiguous():      # (_parse_scoremod hands over a contiguous tensor; a temporary made here would be freed before the launch)
        raise RuntimeError("fa2: the slope tensor of a score-modifier call must be contiguous")
    return (float(cap), a.data_ptr(), a.stride(0) if a.dim() == 2 else 0)


DROPOUT_MESSAGE = "fa2: dropout_p must be a number in [0, 1)"


def _parse_dropout(dropout_p, dropout_seed):
    """The operator's dropout arguments -> None (dropout_p == 0) or (p, seed).  Raises ValueError before any device work.  dropout_seed=None draws a
    63-bit seed from torch's CPU default generator, so torch.manual_seed reproduces a run."""
    try:
        p = float(dropout_p)
    except (TypeError, ValueError):
        raise ValueError(DROPOUT_MESSAGE + ", got %r" % (dropout_p,))
    if isinstance(dropout_p, bool) or not (0.0 <= p < 1.0):           # (NaN fails the comparison)
        raise ValueError(DROPOUT_MESSAGE + ", got %r" % (dropout_p,))
    if p == 0.0:
        return None
    if dropout_seed is None:
        dropout_seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, device="cpu").item())
    if isinstance(dropout_seed, bool) or not isinstance(dropout_seed, int) or not (0 <= dropout_seed < 2 ** 64):
        raise ValueError("fa2: dropout_seed must be None or an int in [0, 2**64), got %r" % (dropout_seed,))
    return (p, dropout_seed)


def dropout_keep_mask(seed, p, B, H, Nq, Nkv):
    """The keep mask of a dropout call as a CPU bool tensor [B, H, Nq, Nkv] (True = kept), from the library's host function fa2_dropout_keep_mask — the
    same inline functions the kernels call (csrc/fa2_dropout.h).  For a packed call B counts the sequences and Nq / Nkv are positions inside one.
    No GPU needed."""
    lib = _fa2_lib.load()
    out = torch.empty((B, H, Nq, Nkv), dtype=torch.uint8)
    for b in range(B):
        for h in range(H):
            rc = lib.fa2_dropout_keep_mask(int(seed), float(p), int(H), b, h, 0, int(Nq), 0, int(Nkv), out[b, h].data_ptr())
            if rc:
                if rc == -9:
                    raise ValueError(DROPOUT_MESSAGE + ", got %r" % (p,))
                _fa2_lib.check(rc)
    return out.bool()


def flash_attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=None, max_seqlen_k=None, causal=False, scale=None, window=None,
                           bottom_right=False, dropout_p=0.0, dropout_seed=None, softcap=0.0, alibi_slopes=None, return_lse=False):
    """Packed, variable-length attention: B sequences of individual lengths in one buffer (the flash_attn_varlen_func shape).
    q [total_q, H, D], k / v [total_k, Hkv, D] (Hkv divides H: grouped K / V are not expanded); cu_seqlens_q / cu_seqlens_k: int32 [B + 1] on q's
    device, non-decreasing — sequence s owns the rows [cu[s], cu[s+1]); zero-length sequences are fine.  Returns [total_q, H, D].
    max_seqlen_q / max_seqlen_k: host ints >= every sequence's length; they size the grids.  None computes the maximum from the tensor, which is a
    device-to-host SYNCHRONISATION — pass them in a hot loop.  A sequence longer than the stated maximum is the caller's error: its extra rows are
    not computed.
    causal / window: per sequence, as flash_attention's (window None, an int W or (left, right); causal means right = 0).  Row i of a sequence sits at
    key position i (top-left, this library's convention) or, with bottom_right=True, at i + Nkv_s - Nq_s (other libraries' causal convention; a
    sequence with fewer keys than queries then has leading rows that see nothing).  Rows that see no key return zeros.
    Differentiable in q, k, v (C-ABI fa2_fwd_varlen / fa2_bwd_varlen): no atomics, deterministic gradients.
    dropout_p / dropout_seed: attention dropout as flash_attention's; the mask is keyed by the sequence index and the positions inside the sequence.
    softcap / alibi_slopes: as flash_attention's; the slopes are [H] or [num_sequences, H], the positions count inside the sequence (row i at i, or at
    i + Nkv_s - Nq_s with bottom_right=True).  Not together with dropout_p > 0 (ValueError).
    return_lse=True returns (out, lse), lse f32 [H, total_q] in natural-log units, -inf for rows that see no key, differentiable like out (see
    flash_attention); merge_attention combines such pairs.  False takes exactly the path taken without the argument.
    v narrower than k — v [total_k, Hkv, Dv] with Dv != D, the non-absorbed prefill of multi-head-latent attention (D 192, Dv 128) — returns
    [total_q, H, Dv] (C-ABI fa2_fwd_varlen_dv).  Served: D a multiple of 8 in 136 .. 256 with Dv a multiple of 8 in 8 .. 128; forward only (no input may
    require grad under grad mode), no dropout, softcap or alibi_slopes: ValueError otherwise.  scale=None stays D ** -0.5.  v is read in place whatever
    its row pitch (a column slice of the up-projection's output); return_lse and merge_attention work as above."""
    if _varlen_dv(k, v):
        return _flash_attention_varlen_dv(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, scale, window, bottom_right, dropout_p,
                                          softcap, alibi_slopes, return_lse)
    dropout = None if dropout_p.__class__ is float and dropout_p == 0.0 else _parse_dropout(dropout_p, dropout_seed)      # (the default: no work)
    left, right, _ = _fa2_lib.parse_window(window, 0)
    smod = None
    if not (softcap.__class__ is float and softcap == 0.0 and alibi_slopes is None):                                      # (the default: no work)
        if not (torch.is_tensor(q) and q.dim() == 3 and torch.is_tensor(cu_seqlens_q) and cu_seqlens_q.dim() == 1):
            raise RuntimeError("fa2: q must be [total_q, H, D] and cu_seqlens_q a 1-D tensor")
        smod = _parse_scoremod(softcap, alibi_slopes, q, q.shape[1], cu_seqlens_q.numel() - 1)
        if smod is not None and dropout is not None:
            raise ValueError("fa2: flash_attention_varlen(softcap / alibi_slopes, dropout_p > 0) is not supported: the score modifiers do not combine with dropout")
    h, h_kv, D = _check_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k)
    if max_seqlen_q is None:
        max_seqlen_q = int((cu_seqlens_q[1:] - cu_seqlens_q[:-1]).max())
    if max_seqlen_k is None:
        max_seqlen_k = int((cu_seqlens_k[1:] - cu_seqlens_k[:-1]).max())
    if scale is None:
        scale = D ** -0.5
    flags = (_fa2_lib.FA2_FLAG_CAUSAL if causal else 0) | (_fa2_lib.FA2_FLAG_BOTTOM_RIGHT if bottom_right else 0)
    if return_lse:
        cap, slopes = smod if smod is not None else (0.0, None)
        if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
            return _VarlenLseAttentionFunction.apply(q, k, v, slopes, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), flags, scale,
                                                     (left, right), dropout, cap)
        ret = flash_attn_wmma.forward_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), flags | _fa2_lib.FA2_FLAG_EXACT_SCALE,
                                             scale, (left, right), dropout, smod)
        return ret[0], ret[5] * _LN2
    if smod is not None:
        if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
            return _VarlenScoreModAttentionFunction.apply(q, k, v, smod[1], cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), flags, scale,
                                                          (left, right), smod[0])
        return flash_attn_wmma.forward_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), flags | _fa2_lib.FA2_FLAG_EXACT_SCALE,
                                              scale, (left, right), scoremod=smod)[0]
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        if dropout is not None:
            return _VarlenAttentionFunction.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), flags, scale, (left, right), dropout)
        return _VarlenAttentionFunction.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), flags, scale, (left, right))
    if dropout is not None:
        return flash_attn_wmma.forward_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), flags, scale, (left, right), dropout)[0]
    return flash_attn_wmma.forward_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), flags, scale, (left, right))[0]


def _varlen_dv(k, v):
    """Is this packed call one with v narrower (or wider) than k — same tokens, same heads, another head dim?  Anything else is _check_varlen's to judge."""
    return torch.is_tensor(k) and torch.is_tensor(v) and k.dim() == 3 and v.dim() == 3 and v.shape[2] != k.shape[2] and v.shape[:2] == k.shape[:2]


def _flash_attention_varlen_dv(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, scale, window, bottom_right, dropout_p, softcap,
                               alibi_slopes, return_lse):
    """flash_attention_varlen with v narrower than k: the refusals (before any device work), then fa2_fwd_varlen_dv."""
    D, Dv = k.shape[2], v.shape[2]
    if D % 8 or not 136 <= D <= 256 or Dv % 8 or not 8 <= Dv <= 128:
        raise ValueError("fa2: flash_attention_varlen serves v narrower than k for head dims D in 136 .. 256 and Dv in 8 .. 128, multiples of 8 "
                         "(192 / 128: the MLA prefill); got D = %d, Dv = %d" % (D, Dv))
    if not (dropout_p == 0 and softcap == 0 and alibi_slopes is None):
        raise ValueError("fa2: flash_attention_varlen with v narrower than k takes no dropout_p > 0, softcap or alibi_slopes")
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (q, k, v)):
        raise ValueError("fa2: flash_attention_varlen with v narrower than k is forward only (an input requires grad): call it under torch.no_grad()")
    left, right, _ = _fa2_lib.parse_window(window, 0)
    _check_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, dv=True)
    if max_seqlen_q is None:
        max_seqlen_q = int((cu_seqlens_q[1:] - cu_seqlens_q[:-1]).max())
    if max_seqlen_k is None:
        max_seqlen_k = int((cu_seqlens_k[1:] - cu_seqlens_k[:-1]).max())
    if scale is None:
        scale = D ** -0.5
    flags = (_fa2_lib.FA2_FLAG_CAUSAL if causal else 0) | (_fa2_lib.FA2_FLAG_BOTTOM_RIGHT if bottom_right else 0)
    out, L = flash_attn_wmma.forward_varlen_dv(q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), flags, scale, (left, right))
    return (out, L * _LN2) if return_lse else out


def _band_mask(nq, nkv, window, causal, device):
    """The window as a boolean keep-mask [Nq, Nkv] (True = attend): what flash_attention folds into `mask` when both are given."""
    left, right, off = window
    if causal:
        right = 0
    pos = torch.arange(nq, device=device).unsqueeze(1) + off
    j = torch.arange(nkv, device=device).unsqueeze(0)
    keep = torch.ones((nq, nkv), dtype=torch.bool, device=device)
    if left >= 0:
        keep &= j >= pos - left
    if right >= 0:
        keep &= j <= pos + right
    return keep


def flash_attention(q, k, v, mask=None, causal=False, scale=None, BNHD_fmt=False, window=None, q_offset=0, dropout_p=0.0, dropout_seed=None,
                    softcap=0.0, alibi_slopes=None, return_lse=False):
    """Forward attention that HONOURS `mask` — the extension the reference lists as to do (README.md:45; its
    FlashAttentionFunction accepts the argument and ignores it, FlashAttn.py:49, :74, and `FlashAttentionFunction.apply` here
    keeps doing exactly that so that existing call sites see no change).  `mask` follows
    torch.nn.functional.scaled_dot_product_attention(attn_mask=...): broadcastable to [B, H, Nq, Nkv]; bool = True where
    attention is allowed, float = added to the scaled scores.  mask=None is FlashAttentionFunction.apply.  Rows whose every
    position is masked return zeros.  Differentiable in q, k, v (C-ABI fa2_bwd_bias; head dims up to 256); the mask gets no gradient.

    `window` / `q_offset`: sliding-window (local) attention.  window is None, an int W (= (W, W)) or (left, right) with -1 / None = unbounded;
    query row i sits at key position i + q_offset and attends the keys [i + q_offset - left, i + q_offset + right]; `causal` then means right = 0
    (causal=True, window=(W - 1, 0): W keys ending at the query's own; q_offset = Nkv - Nq: new queries against a longer KV cache).  The kernels
    sweep only the tiles of the band (C-ABI fa2_fwd_window / fa2_bwd_window: no [Nq, Nkv] mask in memory, grouped k / v without expansion); rows
    that see no key return zeros.  With a `mask` as well the band is folded into it and the masked path runs.  window=None, q_offset=0: as before.

    `dropout_p` / `dropout_seed`: attention dropout, the dropout_p of scaled_dot_product_attention.  Each probability is dropped after the softmax with
    probability p_eff = round(p * 65536) / 65536 and the kept ones are scaled by 1 / (1 - p_eff); the mask is generated in-kernel (Philox4x32-10 keyed by
    the seed: csrc/fa2_dropout.h has the contract, dropout_keep_mask() returns it on the CPU) and regenerated by the backward, so no [Nq, Nkv] tensor
    exists.  It applies whenever dropout_p > 0, whatever the grad mode (as SDPA); dropout_p == 0 takes exactly the path it takes without the argument.
    dropout_seed=None draws a seed from torch's CPU default generator (torch.manual_seed reproduces a run).  Works with causal, window, q_offset and
    grouped k / v (C-ABI fa2_fwd_dropout / fa2_bwd_dropout, every head dim up to 512).  Limits: the seed is a host value, so a call captured in a
    graph replays the same mask; `mask=` together with dropout_p > 0 is not supported (ValueError).

    `softcap` / `alibi_slopes`: the two keywords of flash_attn_func that change the score itself, applied between Q.K^T and the softmax:
    s = softcap * tanh(scale * q.k / softcap) when softcap > 0 (Gemma-2 / -3, Grok), then s -= slope[b, h] * |i + q_offset - j| when alibi_slopes is
    given (BLOOM, MPT, Baichuan) — a float32 tensor on q's device, [H] or [B, H], one slope per QUERY head, no gradient —, then the causal / window
    masks.  No [Nq, Nkv] tensor exists; works with causal, window, q_offset and grouped k / v, differentiable in q, k, v (C-ABI fa2_fwd_scoremod /
    fa2_bwd_scoremod, every head dim up to 512).  softcap=0.0, alibi_slopes=None: exactly the path taken without the arguments.  Not together with
    `mask=` or dropout_p > 0 (ValueError).

    `return_lse`: True returns (out, lse) — flash_attn_func's return_attn_probs / return_lse.  lse is the row log-sum-exp of the (masked, modified)
    scaled scores, f32 [B, H, Nq] whatever BNHD_fmt is, in NATURAL-log units, -inf for rows that see no key; under dropout it is that of the undropped
    probabilities.  It works on every route above.  When q, k or v needs a gradient, lse is a differentiable output of the same autograd node as out
    (C-ABI fa2_bwd_lse / fa2_bwd_window_lse: d lse_i / d s_ij = P_ij enters the dQ pass's row term), so attention over pieces of the KV axis can be
    merged with merge_attention and differentiated — ring / sequence-parallel attention, chunked prefill, shared-prefix inference, a sink term added by
    the caller.  Such a call ALWAYS scales the f32 scores (FA2_FLAG_EXACT_SCALE), also under no_grad: the LSE is a result the caller combines with the
    LSEs of other calls, so it must be that of the f32-scaled scores, not of a kernel that folds the scale into a rounded Q.  With a gradient for lse
    head dim 128 runs the compiler-scheduled backward passes (fa2_bwd_lse_plan).  False takes exactly the path taken without the argument."""
    if return_lse:
        return _flash_attention_lse(q, k, v, mask, causal, scale, BNHD_fmt, window, q_offset, dropout_p, dropout_seed, softcap, alibi_slopes)
    dropout = None if dropout_p.__class__ is float and dropout_p == 0.0 else _parse_dropout(dropout_p, dropout_seed)      # (the default: no work)
    if not (softcap.__class__ is float and softcap == 0.0 and alibi_slopes is None):                                      # (the default: no work)
        if not (torch.is_tensor(q) and torch.is_tensor(k) and torch.is_tensor(v)) or q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
            raise RuntimeError("fa2: q, k, v must be 4-D ([B,H,N,D] or [B,N,H,D] with BNHD_fmt)")
        smod = _parse_scoremod(softcap, alibi_slopes, q, q.shape[2 if BNHD_fmt else 1], q.shape[0])
        if smod is not None:
            if mask is not None:
                raise ValueError("fa2: flash_attention(mask=..., softcap / alibi_slopes) is not supported: the score modifiers run on the unmasked / windowed kernels only")
            if dropout is not None:
                raise ValueError("fa2: flash_attention(softcap / alibi_slopes, dropout_p > 0) is not supported: the score modifiers do not combine with dropout")
            win = _fa2_lib.parse_window(window if window is not None else (-1, -1), q_offset)
            if not q.is_cuda or not k.is_cuda or not v.is_cuda:
                raise RuntimeError("fa2: q, k, v must be on a ROCm device (no CPU path in this operator)")
            D = q.shape[3]
            if scale is None:
                scale = D ** -0.5
            if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
                return _ScoreModAttentionFunction.apply(q, k, v, smod[1], bool(causal), scale, BNHD_fmt, win, smod[0])
            Br = 32 if D > 384 else 64                      # FlashAttn.py:56-67
            flags = (_fa2_lib.FA2_FLAG_CAUSAL if causal else 0) | _fa2_lib.FA2_FLAG_EXACT_SCALE
            return flash_attn_wmma.forward_py(q, k, v, Br, 128, flags, scale, BNHD_fmt, window=win, scoremod=smod)[0]
    if dropout is not None:
        if mask is not None:
            raise ValueError("fa2: flash_attention(mask=..., dropout_p > 0) is not supported: dropout runs on the unmasked / windowed kernels only")
        win = _fa2_lib.parse_window(window if window is not None else (-1, -1), q_offset)
        if not (torch.is_tensor(q) and torch.is_tensor(k) and torch.is_tensor(v)) or q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
            raise RuntimeError("fa2: q, k, v must be 4-D ([B,H,N,D] or [B,N,H,D] with BNHD_fmt)")
        if not q.is_cuda or not k.is_cuda or not v.is_cuda:
            raise RuntimeError("fa2: q, k, v must be on a ROCm device (no CPU path in this operator)")
        D = q.shape[3]
        if scale is None:
            scale = D ** -0.5
        if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
            return _DropoutAttentionFunction.apply(q, k, v, bool(causal), scale, BNHD_fmt, win, dropout)
        Br = 32 if D > 384 else 64                      # FlashAttn.py:56-67
        flags = (_fa2_lib.FA2_FLAG_CAUSAL if causal else 0) | _fa2_lib.FA2_FLAG_EXACT_SCALE
        return flash_attn_wmma.forward_py(q, k, v, Br, 128, flags, scale, BNHD_fmt, window=win, dropout=dropout)[0]
    if window is not None or q_offset != 0:
        win = _fa2_lib.parse_window(window, q_offset)
        if mask is not None:
            n_ax = 1 if BNHD_fmt else 2
            band = _band_mask(q.shape[n_ax], k.shape[n_ax], win, causal, q.device)
            if mask.dtype == torch.bool:
                mask = mask & band
            else:
                mask = (mask + torch.zeros_like(band, dtype=mask.dtype)).masked_fill(~band, float("-inf"))      # (broadcast to [..., Nq, Nkv] first)
            return flash_attention(q, k, v, mask, False, scale, BNHD_fmt)
        h_ax = 2 if BNHD_fmt else 1
        if q.dim() == 4 and k.dim() == 4 and k.shape[h_ax] != q.shape[h_ax]:
            _check_groups(q.shape[h_ax], k.shape[h_ax])
        D = q.shape[3]
        if scale is None:
            scale = D ** -0.5
        if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
            return _WindowAttentionFunction.apply(q, k, v, bool(causal), scale, BNHD_fmt, win)
        Br = 32 if D > 384 else 64                      # FlashAttn.py:56-67
        return flash_attn_wmma.forward_window(q, k, v, Br, 128, bool(causal), scale, BNHD_fmt, win)[0]
    if mask is None:
        return FlashAttentionFunction.apply(q, k, v, None, causal, scale, BNHD_fmt)
    h_ax = 2 if BNHD_fmt else 1
    if q.dim() == 4 and k.dim() == 4 and v.dim() == 4 and k.shape[h_ax] != q.shape[h_ax]:
        # grouped-query attention under a mask: the masked kernels have no grouped form, so K / V are expanded to q's head count here and autograd
        # sums dK / dV over each group (correct, not a hot path: the expanded K / V cross memory g times)
        _check_groups(q.shape[h_ax], k.shape[h_ax])
        if v.shape[h_ax] != k.shape[h_ax]:
            raise RuntimeError("fa2: inconsistent q/k/v shapes %s %s %s" % (tuple(q.shape), tuple(k.shape), tuple(v.shape)))
        g = q.shape[h_ax] // k.shape[h_ax]
        k, v = k.repeat_interleave(g, dim=h_ax), v.repeat_interleave(g, dim=h_ax)
    D = q.shape[3]
    if scale is None:
        scale = D ** -0.5
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        return _MaskedAttentionFunction.apply(q, k, v, mask, causal, scale, BNHD_fmt)
    Br = 32 if D > 384 else 64                      # FlashAttn.py:56-67
    return flash_attn_wmma.forward_bias(q, k, v, mask, Br, 128, bool(causal), scale, BNHD_fmt)[0]
