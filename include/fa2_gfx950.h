/*
 * fa2_gfx950.h — C-ABI of the MI355X (gfx950 / CDNA4) FlashAttention-2 path (forward + backward).
 *
 * This is the drop-in boundary for the ONE hot path of
 * Repeerc/flash-attention-v2-RDNA3-minimal: the forward attention operator behind
 * rocwmma_fattn/FlashAttn.py.  Citations are relative to the reference tree.
 *
 * What each entry point replaces in the reference:
 *
 *   fa2_fwd_f16   <->  forward_fp16(q,k,v,Br,Bc,causal,scale,permute_NH)
 *                      declared rocwmma_fattn/host.cpp:24-28, defined
 *                      rocwmma_fattn/kernel_fp16.cu:744-876 (launcher) + :306-544 (fwd_kernel)
 *   fa2_fwd_bf16  <->  forward_bf16(...), rocwmma_fattn/host.cpp:24-28,
 *                      rocwmma_fattn/kernel_bf16.cu:802-941 + :329-577
 *   fa2_fwd       <->  the dtype switch `forward(...)`, rocwmma_fattn/host.cpp:30-45
 *
 * Differences from the reference's C++ symbols (deliberate):
 *   - plain pointers / sizes / strides, no torch types, no allocation: the CALLER owns q,k,v,o,lse;
 *   - asynchronous launch on the hipStream_t handed in (reference: null stream, kernel_fp16.cu:844);
 *   - 64-bit element strides (reference: 32-bit `int` offsets, kernel_fp16.cu:324);
 *   - returns an error code (reference: printf only, kernel_fp16.cu:854-863);
 *   - Br/Bc are not parameters: tile sizes are an internal choice of the gfx950 kernel.
 *
 * Layout contract
 *   q   : [B, H, Nq , D]  element (b,h,i,c) at q + b*q_strides[0] + h*q_strides[1] + i*q_strides[2] + c
 *   k,v : [B, H, Nkv, D]  likewise with k_strides / v_strides
 *   o   : [B, H, Nq , D]  likewise with o_strides
 *   lse : f32, element (b,h,i) at lse + b*lse_strides[0] + h*lse_strides[1] + i
 *   Strides are in ELEMENTS; the last (D) dimension is contiguous.  The reference's BNHD
 *   ("permute_NH", kernel_fp16.cu:328-333) layout is the same call with the head and row strides
 *   of the [B,N,H,D] tensor: strides = {N*H*D, D, H*D}.
 *   All base pointers must be 16-byte aligned and every stride a multiple of 8 elements.
 *   D is any multiple of 8 up to the largest kernel head dim (512, forward and backward): the call runs on the
 *   kernel of fa2_padded_head_dim(D) and columns >= D are masked in-kernel — read as zero, never stored — where
 *   the reference zero-pads D on the host (kernel_fp16.cu:763, :767-779).
 *   Span rules ("addressing limits").  The span of one head's matrix of n rows is ((n - 1) * row stride + D) * 2 bytes.  Bounded, with 64
 *   further rows of the same pitch as slack: span + 64 * row stride * 2 <= 2^31 - 1, else FA2_ERR_BAD_SHAPE —
 *     forward : K and V (n = Nkv);            backward : K, V (n = Nkv), Q and dO (n = Nq);
 *     packed  : the same tensors with n = the stated maximum length (a sequence's rows, not the packed tensor's);
 *     bias    : one (b, h) slice, ((Nq - 1) * bias_strides[2] + Nkv + 64 * bias_strides[2]) * element size < 2^31 - 1, in the backward (the
 *               forward accepts any bias slice and chooses the load form by it).
 *   Not bounded: Q, O and LSE of the forward; O, dQ, dK, dV, LSE and delta_ws of the backward; every batch and head stride; the packed tensors
 *   as a whole.  These are addressed with 64-bit pointers.  Where a hand-scheduled kernel would address one of them with 32-bit offsets the call
 *   runs on the compiler-scheduled kernels instead, and the plan query says so:
 *     Q of the forward's 256-row bodies: ((Nq + 64) * row stride + D) * 2 < 2^32 at the body's head dim (64, 128), < 2^31 at a head dim below it;
 *     Q and O of the forward's 128-row kernel (head dims 136 .. 256): ((Nq + 128) * row stride + 256) * 2 < 2^32 — every wave of the last
 *       workgroup forms its rows' offsets, up to 127 rows past Nq;
 *     O of the backward's hand-scheduled dQ pass (fa2_bwd_plan): the K / V rule above, which keeps O's loads in the range of Q's and dO's.
 *   The forward stages a bias by LDS-DMA (fa2_fwd_bias_form) only while one (b, h) slice obeys the backward's bias rule.
 *
 * Numerics contract (reference: kernel_fp16.cu:434-490, :510-543)
 *   S = (Q K^T) * scale * log2(e)   (f32 accumulate on MFMA)
 *   causal: (i, j) masked iff j > i, top-left aligned (kernel_fp16.cu:403-410).  The `causal` argument of every entry point carries the call's
 *   flags: bit 0 (FA2_FLAG_CAUSAL, i.e. the reference's 0 / 1) and bit 1, FA2_FLAG_EXACT_SCALE: this forward call scales the f32 product like the
 *   reference kernel (kernel_fp16.cu:164) whatever option "fold" says — the operator sets it on the forward of calls that will be differentiated, so
 *   that the backward recomputes P from the very scores the saved L was formed from; the backward entry points accept and ignore it.  Any other
 *   bit set is FA2_ERR_BAD_SHAPE (until round 5 every non-zero value meant "causal": a caller that passes another truthy int is told so instead of
 *   silently getting a non-causal forward).  A caller that pairs fa2_fwd* with fa2_bwd* itself — the reference's module-level
 *   flash_attn_wmma.forward / .backward (host.cpp:30-58) — sets FA2_FLAG_EXACT_SCALE on the forward; the Python front end does it for such callers
 *   whenever an input requires a gradient
 *   online softmax in f32 (running max m, running sum l), P rounded to the I/O dtype (RNE) for P·V,
 *   O accumulated in f32 registers, O = O / l rounded once to the I/O dtype,
 *   lse[i] = m + log2(l)  — the LOG2-domain log-sum-exp of the scaled scores, i.e.
 *   natural LSE * log2(e), the reference kernel's convention (kernel_fp16.cu:541-542).
 */
#ifndef FA2_GFX950_H
#define FA2_GFX950_H

#include <stddef.h>
#include <stdint.h>

#define FA2_FLAG_CAUSAL      1
#define FA2_FLAG_EXACT_SCALE 2
#define FA2_FLAG_BOTTOM_RIGHT 4   /* the packed (varlen) entry points only: see fa2_fwd_varlen; every other entry point refuses this bit */

#ifdef __cplusplus
extern "C" {
#endif

/* dtype codes for fa2_fwd */
#define FA2_DTYPE_F16  0
#define FA2_DTYPE_BF16 1

/* return codes: 0 = launched; >0 = hipError_t from the runtime; <0 = argument validation */
#define FA2_OK                 0
#define FA2_ERR_NULL_POINTER  -1
#define FA2_ERR_BAD_SHAPE     -2   /* B,H,Nq,Nkv,D < 1 */
#define FA2_ERR_HEAD_DIM      -3   /* D not a multiple of 8, or larger than the largest kernel head dim */
#define FA2_ERR_ALIGNMENT     -4   /* pointer not 16-B aligned or stride not a multiple of 8 */
#define FA2_ERR_DTYPE         -5
#define FA2_ERR_SCALE         -6   /* scale is NaN/inf */
#define FA2_ERR_GRID          -7   /* B*H*ceil(Nq/256) exceeds the 2^31-1 grid limit */
#define FA2_ERR_BIAS          -8   /* unknown bias_kind or a negative bias stride */
#define FA2_ERR_DROPOUT       -9   /* dropout_p < 0, >= 1 or NaN (the dropout entry points) */
#define FA2_ERR_SOFTCAP       -10  /* softcap < 0, NaN or inf (the score-modifier entry points) */

/* bias_kind codes for fa2_fwd_bias */
#define FA2_BIAS_NONE     0   /* no bias: the call is fa2_fwd */
#define FA2_BIAS_IO_DTYPE 1   /* additive bias in the I/O dtype (fp16 / bf16, as `dtype` says) */
#define FA2_BIAS_F32      2   /* additive bias, f32 */
#define FA2_BIAS_BOOL     3   /* keep-mask, one byte per element: non-zero = attend, zero = masked (score -> -inf) */

/* Forward attention, fp16 I/O.  Replaces forward_fp16 (rocwmma_fattn/host.cpp:24-28). */
int fa2_fwd_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                int B, int H, int Nq, int Nkv, int D,
                const int64_t q_strides[3], const int64_t k_strides[3],
                const int64_t v_strides[3], const int64_t o_strides[3],
                const int64_t lse_strides[2],
                float scale, int causal, void* hip_stream);

/* Forward attention, bf16 I/O.  Replaces forward_bf16 (rocwmma_fattn/host.cpp:24-28). */
int fa2_fwd_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                 int B, int H, int Nq, int Nkv, int D,
                 const int64_t q_strides[3], const int64_t k_strides[3],
                 const int64_t v_strides[3], const int64_t o_strides[3],
                 const int64_t lse_strides[2],
                 float scale, int causal, void* hip_stream);

/* dtype-switched entry.  Replaces forward() (rocwmma_fattn/host.cpp:30-45). */
int fa2_fwd(int dtype,
            const void* q, const void* k, const void* v, void* o, float* lse,
            int B, int H, int Nq, int Nkv, int D,
            const int64_t q_strides[3], const int64_t k_strides[3],
            const int64_t v_strides[3], const int64_t o_strides[3],
            const int64_t lse_strides[2],
            float scale, int causal, void* hip_stream);

/*
 * Forward attention with a caller-owned workspace: the same call as fa2_fwd, plus scratch memory that lets the library balance the
 * last, partly filled round of workgroups.  B*H*ceil(Nq/256) equal workgroups on the chip's CUs take ceil(x / CUs) rounds however
 * empty the last one is (SDXL's 64x64 self-attention, B2 H10 N4096 D64, is 320 workgroups on 256 CUs: two rounds for 1.25 rounds of
 * work; the reference's own N sweep, bench_with_sdpa.py:201-224, saw-tooths for the same reason).  With a workspace, the items of
 * that last round are each swept by several workgroups over disjoint KV ranges and a small kernel merges the partial results
 * (non-causal launches of head dims <= 128; every other call, and any call whose workspace is NULL or too small, is exactly fa2_fwd).
 * Round 6: a grid that covers at most half of the CUs over a long sweep — a batch-1 call, a decode-sized call (one query row x 8 192 keys x 32
 * heads: 45 us with the workspace, 147 without) — has EVERY item split the same way, where that saves at least twice the scheme's fixed cost.
 * The reference has no counterpart (its launcher pads the grid to its 96 CUs instead, kernel_fp16.cu:808-813).
 *   fa2_fwd_workspace_bytes  bytes fa2_fwd_ws can use for this shape on the current device (0: it would not use any).  A function
 *                            of the arguments, the device's CU count and the "split" option only; never more than 64 MiB.
 *   workspace                >= that many bytes, 16-byte aligned, owned by the caller, free for reuse once the work queued on
 *                            `hip_stream` by this call has run (calls on one stream may share it; concurrent streams may not).
 * Results agree with fa2_fwd to f32 rounding of the merge (the parts are normalised in f32 and rounded to the I/O dtype once).
 */
int fa2_fwd_ws(int dtype,
               const void* q, const void* k, const void* v, void* o, float* lse,
               int B, int H, int Nq, int Nkv, int D,
               const int64_t q_strides[3], const int64_t k_strides[3],
               const int64_t v_strides[3], const int64_t o_strides[3],
               const int64_t lse_strides[2],
               float scale, int causal, void* workspace, size_t workspace_bytes, void* hip_stream);
size_t fa2_fwd_workspace_bytes(int dtype, int B, int H, int Nq, int Nkv, int D, int causal);

/*
 * Forward attention with an attention bias / mask: S = (Q K^T) * scale + bias[b, h, i, j] before the softmax (additive kinds), or
 * masked to -inf where the boolean mask is zero — the semantics of torch's scaled_dot_product_attention(attn_mask=...).
 * This is the `mask` argument the reference reserves but never implements: FlashAttentionFunction.forward accepts and
 * ignores it (rocwmma_fattn/FlashAttn.py:49, :74), README.md:45 lists it as to do; SURVEY section 8 row f4.
 *   bias         : element (b,h,i,j) at bias + b*bias_strides[0] + h*bias_strides[1] + i*bias_strides[2] + j, in ELEMENTS of the
 *                  bias type (bias_kind); a stride of 0 broadcasts that dimension; the last (Nkv) dimension is contiguous.
 *                  The pointer must be aligned to the element size; no other alignment is required (Nkv = 77 rows are fine).
 *   causal       : may be combined with the bias (both masks apply).
 *   fully masked rows (every score -inf) produce O = 0 and lse = -inf (torch's math path returns NaN there).
 * Runs the compiler-scheduled HIP kernels (the hand-scheduled bodies have no bias stream): a dense per-row bias whose pointer, strides and Nkv
 * are multiples of 16 bytes, on a grid that fills the chip at head dims <= 128, as 8-wave 256-row workgroups with the bias tile staged by LDS-DMA;
 * everything else as 4-wave 128-row workgroups (a bias broadcast over the rows, bias_strides[2] == 0 — a key-padding mask — costs one load per
 * wave and KV tile there).  Its backward is fa2_bwd_bias (fa2_bwd recomputes unbiased scores).
 */
int fa2_fwd_bias(int dtype,
                 const void* q, const void* k, const void* v, void* o, float* lse,
                 int B, int H, int Nq, int Nkv, int D,
                 const int64_t q_strides[3], const int64_t k_strides[3],
                 const int64_t v_strides[3], const int64_t o_strides[3],
                 const int64_t lse_strides[2],
                 float scale, int causal,
                 const void* bias, int bias_kind, const int64_t bias_strides[3],
                 void* hip_stream);

/*
 * Backward attention: dQ, dK, dV from dO.  Replaces backward_fp16 / backward_bf16 (rocwmma_fattn/host.cpp:24-28,
 * :47-58; rocwmma_fattn/kernel_fp16.cu:878-1028 launcher + :547-740 bwd_kernel; bf16 twin kernel_bf16.cu).
 *   o, lse   : the forward's outputs (lse in log2 units, as fa2_fwd writes it)
 *   dout     : [B,H,Nq,D] upstream gradient, same dtype as q
 *   dq/dk/dv : outputs, caller-owned, every element written (no zero-init needed)
 *   delta_ws : caller-owned f32 workspace addressed like lse (lse_strides), >= Nq floats per (b,h): scratch of the call
 *              (it carries D_i = rowsum(dO_i * O_i), the reference's `Di`, kernel_fp16.cu:605-631 — or its negative,
 *              depending on the kernel family — from the dQ pass to the dK/dV pass)
 * Two launches on `hip_stream` at D <= 128 (dQ — which also fills delta_ws —, then dK and dV in one sweep: one fused pass at D <= 64, wave pairs at D <= 128),
 * three above (dQ, dV, dK); deterministic: every output element has one owner — the
 * reference's dQ is an unsynchronised read-modify-write across KV blocks (kernel_fp16.cu:736).
 * Gradients are those of O = softmax(scale * Q K^T [+ causal mask]) V, i.e. what torch autograd returns.
 * Head dims: multiples of 8 up to 512, like the forward.  D > 128 runs 4-wave, single-LDS-stage kernels, D > 256 as 128-column slabs of
 * the outputs that recompute S and dP per slab (three launches): correct, not tuned.
 */
int fa2_bwd_f16(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                void* dq, void* dk, void* dv, float* delta_ws,
                int B, int H, int Nq, int Nkv, int D,
                const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                const int64_t dk_strides[3], const int64_t dv_strides[3], const int64_t lse_strides[2],
                float scale, int causal, void* hip_stream);

int fa2_bwd_bf16(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                 void* dq, void* dk, void* dv, float* delta_ws,
                 int B, int H, int Nq, int Nkv, int D,
                 const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                 const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                 const int64_t dk_strides[3], const int64_t dv_strides[3], const int64_t lse_strides[2],
                 float scale, int causal, void* hip_stream);

/* dtype-switched entry.  Replaces backward() (rocwmma_fattn/host.cpp:47-58). */
int fa2_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
            void* dq, void* dk, void* dv, float* delta_ws,
            int B, int H, int Nq, int Nkv, int D,
            const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
            const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
            const int64_t dk_strides[3], const int64_t dv_strides[3], const int64_t lse_strides[2],
            float scale, int causal, void* hip_stream);

/*
 * Backward with a caller-owned workspace: fa2_bwd plus scratch memory, the backward's twin of fa2_fwd_ws.  With it the last, partly filled
 * round of 256-row workgroups of the dQ pass (head dims <= 128, compiler-scheduled kernels) and of the fused dK / dV pass (head dims <= 64)
 * is split into parts that sweep disjoint tile ranges and leave f32 partial accumulators in the workspace; a small kernel sums them, applies
 * `scale` and rounds once (the split changes the f32 summation order of those rows, nothing else).  Non-causal calls; everything else, and any
 * call whose workspace is NULL or too small, is exactly fa2_bwd.  fa2_bwd_workspace_bytes: as fa2_fwd_workspace_bytes (<= 64 MiB, 0 for most shapes).
 * Round 6: as in the forward, a pass whose grid covers at most half of the CUs splits every item.
 */
int fa2_bwd_ws(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
               void* dq, void* dk, void* dv, float* delta_ws,
               int B, int H, int Nq, int Nkv, int D,
               const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
               const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
               const int64_t dk_strides[3], const int64_t dv_strides[3], const int64_t lse_strides[2],
               float scale, int causal, void* workspace, size_t workspace_bytes, void* hip_stream);
size_t fa2_bwd_workspace_bytes(int dtype, int B, int H, int Nq, int Nkv, int D, int causal);

/*
 * Backward through fa2_fwd_bias: the gradients of O = softmax(scale * Q K^T + bias [+ causal mask]) V with respect to Q, K, V (the bias /
 * mask itself is a constant of the call: it receives no gradient).  o and lse are the outputs of the fa2_fwd_bias call with the SAME bias
 * arguments; fully masked rows (lse = -inf) contribute nothing.  Arguments as fa2_bwd plus the bias triple of fa2_fwd_bias.
 * The compiler-scheduled passes — dQ, then dK and dV in one sweep at head dims <= 64 (dV, then dK above); a per-row bias whose pointer, strides and Nkv are multiples of 16 bytes is staged
 * tile by tile with LDS-DMA, anything else (Nkv = 77) read with one bounds-checked load per score — a bias broadcast over the Q rows (a
 * [B, 1, 1, Nkv] key-padding mask) with one load per KV row in the dK / dV pass.  One (b, h) slice of the
 * bias must span < 2 GiB (FA2_ERR_BAD_SHAPE).  Head dims up to 256 (FA2_ERR_HEAD_DIM above).  The reference has no counterpart (its `mask` is
 * ignored, FlashAttn.py:49/:74).
 */
int fa2_bwd_bias(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                 void* dq, void* dk, void* dv, float* delta_ws,
                 int B, int H, int Nq, int Nkv, int D,
                 const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                 const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                 const int64_t dk_strides[3], const int64_t dv_strides[3], const int64_t lse_strides[2],
                 float scale, int causal,
                 const void* bias, int bias_kind, const int64_t bias_strides[3],
                 void* hip_stream);

/*
 * fa2_bwd_bias with scratch memory — fa2_bwd_ws for the masked backward: non-causal calls of head dims <= 128 split the workgroups of a partly
 * filled last round of the dQ pass, and (head dims <= 64) of the fused dK / dV pass, where an underfilled KV-owner grid — cross-attention over
 * 77 keys has B * H workgroups in all — splits every workgroup along its Q sweep.  Same contract as fa2_bwd_ws: 16-byte aligned workspace of at
 * least fa2_bwd_bias_workspace_bytes(...) bytes, private to the call until the stream has passed it; NULL / too small / 0 needed: exactly
 * fa2_bwd_bias.  The plan does not depend on the bias' kind or strides.
 */
int fa2_bwd_bias_ws(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                    void* dq, void* dk, void* dv, float* delta_ws,
                    int B, int H, int Nq, int Nkv, int D,
                    const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                    const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                    const int64_t dk_strides[3], const int64_t dv_strides[3], const int64_t lse_strides[2],
                    float scale, int causal,
                    const void* bias, int bias_kind, const int64_t bias_strides[3],
                    void* workspace, size_t workspace_bytes, void* hip_stream);
size_t fa2_bwd_bias_workspace_bytes(int dtype, int B, int H, int Nq, int Nkv, int D, int causal);

/*
 * Grouped-query attention (GQA) and multi-query attention (MQA, Hkv = 1): K and V have Hkv heads that serve the H query heads, the semantics of
 * torch's scaled_dot_product_attention(..., enable_gqa=True).
 * Layout contract
 *   q, o, dout, dq : [B, H,   Nq,  D]  as in fa2_fwd / fa2_bwd
 *   k, v, dk, dv   : [B, Hkv, Nkv, D]  element (b,hk,j,c) at k + b*k_strides[0] + hk*k_strides[1] + j*k_strides[2] + c (likewise v, dk, dv)
 *   lse, delta_ws  : [B, H, Nq] (indexed by the Q head, lse_strides)
 *   Hkv >= 1 must divide H (FA2_ERR_BAD_SHAPE otherwise); g = H / Hkv; Q head h attends K / V head h / g.
 *   dK / dV of K / V head hk are the SUM of the gradients of the Q heads hk*g .. hk*g + g-1 — formed in-kernel: one workgroup owns a K / V head's
 *   rows and sweeps the Q tiles of its g member heads in turn, accumulating in f32 registers and rounding once (no atomics, deterministic).
 * Kernels.  The forward runs the kernels the MHA call of the same shape runs (fa2_fwd_gqa_plan reports the same plan), with K / V addressed through
 * the group; the workspace acts as in fa2_fwd_ws (NULL / too small: the call is fa2_fwd's).  The backward's dQ pass is the MHA call's, hand-scheduled
 * one at head dim 128 included; the dK / dV passes are the compiler-scheduled ones at every head dim (head dim 128: the wave-pair pass, not the
 * hand-scheduled body), and fa2_bwd_gqa's workspace splits their B * Hkv owners over the virtual sweep of g x (Q tiles) as in fa2_bwd_ws.
 * A call with Hkv == H is exactly the corresponding fa2_fwd_ws / fa2_bwd_ws call.  Masked (bias) calls have no grouped form.
 * When to call which.  fa2_fwd_gqa is the fast choice for every grouped forward (0.94 .. 1.00x the MHA call on pre-expanded K / V, which also
 * needs the expansion).  fa2_bwd_gqa is the MEMORY-lean backward: no expanded K / V, no [B, H, Nkv, D] dK / dV buffers.  It is not the fast one on
 * the shapes measured: its dK / dV passes run B * Hkv * ceil(Nkv / rows) workgroups, a grid g times smaller than the MHA
 * call's, and at head dim 128 without the hand-scheduled body — 1.05 .. 1.5x the time of expanding K / V, fa2_bwd_ws and summing dK / dV over
 * each group at g = 4 .. 8, 5.8x for MQA at B1 N4096.  A caller with the memory to spare takes that route; the Python operator does.
 */
int fa2_fwd_gqa(int dtype,
                const void* q, const void* k, const void* v, void* o, float* lse,
                int B, int H, int Hkv, int Nq, int Nkv, int D,
                const int64_t q_strides[3], const int64_t k_strides[3],
                const int64_t v_strides[3], const int64_t o_strides[3],
                const int64_t lse_strides[2],
                float scale, int causal, void* workspace, size_t workspace_bytes, void* hip_stream);
size_t fa2_fwd_gqa_workspace_bytes(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D, int causal);
int fa2_bwd_gqa(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                void* dq, void* dk, void* dv, float* delta_ws,
                int B, int H, int Hkv, int Nq, int Nkv, int D,
                const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                const int64_t dk_strides[3], const int64_t dv_strides[3], const int64_t lse_strides[2],
                float scale, int causal, void* workspace, size_t workspace_bytes, void* hip_stream);
size_t fa2_bwd_gqa_workspace_bytes(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D, int causal);

/*
 * Sliding-window (local) attention with an offset between query and key positions.
 * Three integers per call:
 *   window_left  >= 0, or -1 = unbounded
 *   window_right >= 0, or -1 = unbounded
 *   q_offset     >= 0: the position of query row 0 on the key axis (0: top-left alignment, this library's causal convention; Nkv - Nq: the
 *                bottom-right alignment of other libraries — a chunk of new queries against a longer KV cache, decode with Nq = 1)
 * Query row i attends key j iff
 *   (window_left < 0 or j >= i + q_offset - window_left) and (window_right < 0 or j <= i + q_offset + window_right) and 0 <= j < Nkv.
 * FA2_FLAG_CAUSAL in `flags` (the `causal` argument of the other entry points: FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE) means window_right = 0 under
 * the same q_offset: causal with q_offset = 0 is the causal call of the other entry points, causal with window_left = W - 1 a window of W keys that
 * ends at the query's own position.  window_left = window_right = -1, q_offset = 0 is plain attention.
 * Rows that see no key (possible when Nq + q_offset > Nkv + window_left) return O = 0 and lse = -inf and contribute zero gradients; dK / dV of a
 * key no row sees are zero, and every element of dq / dk / dv is written (no zero-init needed).
 * Negative values other than -1, a negative q_offset, or values whose sums with Nq / Nkv leave 32-bit position arithmetic: FA2_ERR_BAD_SHAPE.
 * Layout as the grouped entry points: q, o [B, H, Nq, D]; k, v [B, Hkv, Nkv, D], Hkv divides H (the forward addresses K / V through the group, no
 * expansion).  The backward is the multi-head one (k, v, dk, dv have H heads): a caller with grouped K / V expands them and sums dK / dV per group.
 * Numerical contract 0 (f32 scale of the product, row sums of the f32 P); lse in log2 units.
 * Kernels.  The workgroup of a block of query rows sweeps only the KV tiles that hold a key one of its rows sees (the dK / dV passes: the Q tiles
 * of the transposed band), masks the tiles the band's edges cut and runs the unmasked steady-state loop in between: compiler-scheduled kernels at
 * every head dim (FA2_KERNEL_HIP_WINDOW; option "rows" picks 128- or 256-row forward workgroups as elsewhere).  No KV-split, no hand-scheduled
 * bodies.  A call whose window masks nothing for its Nq / Nkv — both -1 with q_offset 0, the causal flag alone with q_offset 0, or bounds at least
 * as long as the sequences — IS the fa2_fwd_gqa / fa2_bwd call of the same arguments (same plan, same kernels, bit-identical results).
 * The plan query reports this; its strides may be NULL for contiguous tensors, as in the other plan queries.
 */
int fa2_fwd_window(int dtype,
                   const void* q, const void* k, const void* v, void* o, float* lse,
                   int B, int H, int Hkv, int Nq, int Nkv, int D,
                   const int64_t q_strides[3], const int64_t k_strides[3],
                   const int64_t v_strides[3], const int64_t o_strides[3],
                   const int64_t lse_strides[2],
                   float scale, int flags, int window_left, int window_right, int q_offset, void* hip_stream);
int fa2_bwd_window(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                   void* dq, void* dk, void* dv, float* delta_ws,
                   int B, int H, int Nq, int Nkv, int D,
                   const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                   const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                   const int64_t dk_strides[3], const int64_t dv_strides[3], const int64_t lse_strides[2],
                   float scale, int flags, int window_left, int window_right, int q_offset, void* hip_stream);
/* The tile-range arithmetic the windowed kernels and their launchers use (pure host arithmetic, no GPU needed; csrc/fa2_window.h).
 * fa2_window_tile_range: the KV tiles of `tile` keys that the block of `rows` query rows starting at `row0` has to sweep are
 * [*first_tile, *first_tile + *ntiles); both ends hold a visible (row, key) pair, ntiles = 0 when the block sees no key.
 * fa2_window_row_range: its transpose — the tiles of `tile` query rows that see at least one of the `keys` keys starting at `key0`.
 * `causal` != 0 means window_right = 0.  Returns FA2_OK, FA2_ERR_NULL_POINTER, or FA2_ERR_BAD_SHAPE for bad windows / offsets / lengths / blocks. */
int fa2_window_tile_range(int Nq, int Nkv, int window_left, int window_right, int q_offset, int causal,
                          int row0, int rows, int tile, int* first_tile, int* ntiles);
int fa2_window_row_range(int Nq, int Nkv, int window_left, int window_right, int q_offset, int causal,
                         int key0, int keys, int tile, int* first_tile, int* ntiles);

/*
 * Packed, variable-length attention: B sequences of individual lengths in one buffer, the layout of other libraries' varlen calls.
 * Layout
 *   q, o, dout, dq : [total_q, H, D]; row t of head h at ptr + t*strides[1] + h*strides[0] — element strides {head, row}, D contiguous
 *   k, v, dk, dv   : [total_k, Hkv, D], addressed the same way (the backward is the multi-head one: its k, v, dk, dv have H heads; a caller with
 *                    grouped K / V expands them and sums dK / dV per group, as for fa2_bwd_window).  The forward addresses K / V through the
 *                    group h / (H / Hkv); nothing is expanded.
 *   Alignment as everywhere: 16-byte pointers, strides multiples of 8 elements.
 *   cu_seqlens_q, cu_seqlens_k : int32[B + 1] in DEVICE memory, non-decreasing.  Sequence s owns the rows [cu[s], cu[s+1]): Nq_s queries, Nkv_s keys.
 *                    Zero-length sequences are legal on either side.  Rows at or beyond cu[B] are neither read nor written.
 *   max_seqlen_q, max_seqlen_k : host integers >= every Nq_s / Nkv_s.  They size the grids (B * H * ceil(max_seqlen / rows) workgroups), so the call
 *                    needs no device-to-host synchronisation.  A sequence LONGER than the stated maximum is the caller's error and cannot be detected
 *                    on the host: its query rows (in the dK / dV passes: its key rows) beyond the maximum are not computed, their outputs not written.
 *   lse, delta_ws  : f32 [H, total_q]; element (h, t) at lse + h*lse_stride + t.  lse in log2 units, as everywhere.
 * Masking, per sequence: the windowed contract above with a per-sequence offset off_s.  Row i of sequence s attends key j of the SAME sequence iff
 *   (window_left < 0 or j >= i + off_s - window_left) and (window_right < 0 or j <= i + off_s + window_right) and 0 <= j < Nkv_s.
 * FA2_FLAG_CAUSAL means window_right = 0.  off_s = 0 is this library's top-left convention and the default; FA2_FLAG_BOTTOM_RIGHT makes
 * off_s = Nkv_s - Nq_s (the convention of other libraries' causal varlen calls).  That offset is negative for a sequence with fewer keys than
 * queries: its first Nq_s - Nkv_s - window_right rows then see nothing.
 * A row that sees no key (Nkv_s = 0, or a row outside the band) returns O = 0 and lse = -inf and contributes no gradient; dK / dV of keys nobody sees
 * are zero (Nq_s = 0 included).  Every element of o, lse, dq, dk, dv below cu[B] is written — no zero-init needed — by exactly one owner: no atomics,
 * deterministic results.  FA2_FLAG_EXACT_SCALE is accepted; the kernels are contract 0 (f32 scale, f32 row sums) either way.
 * Validation (the existing codes; the contents of cu_seqlens are not validated, they live on the device): null pointers; B, H, Hkv, D or a maximum
 * below 1; Hkv not dividing H; a bad window; flag bits other than the three named here; head dim; alignment; a stated maximum whose K / V span
 * (max_seqlen * row pitch; in the backward also Q / dO) reaches 2 GiB; grids beyond 2^31 - 1.  Everything but the tensors and cu_seqlens is
 * checked first, so a bad argument is reported as what it is even with null tensors.
 * Kernels (FA2_KERNEL_HIP_VARLEN): the compiler-scheduled windowed kernels with the lengths, base rows and offset read per workgroup from cu_seqlens.
 * A workgroup whose block starts at or beyond its sequence's length returns at once; the K / V (and Q / dO / lse) buffer descriptors of a workgroup end
 * at the last row of its own sequence, so a neighbour's rows are never fetched.  A band that masks nothing runs the unmasked steady-state loop.
 * Head dims: multiples of 8 up to 512.  Option "rows" picks 128- or 256-row forward workgroups as elsewhere, otherwise a heuristic on the grid of
 * the stated maxima; the plan query reports it (rows as launched, heads_main = B*H; its strides may be NULL for contiguous tensors).
 * The result for a sequence is bit-identical to fa2_fwd_window on that sequence alone (q_offset = off_s, same "rows") wherever that call runs
 * FA2_KERNEL_HIP_WINDOW.
 */
int fa2_fwd_varlen(int dtype,
                   const void* q, const void* k, const void* v, void* o, float* lse,
                   int B, int H, int Hkv, int max_seqlen_q, int max_seqlen_k, int D,
                   const int* cu_seqlens_q, const int* cu_seqlens_k,
                   const int64_t q_strides[2], const int64_t k_strides[2],
                   const int64_t v_strides[2], const int64_t o_strides[2],
                   int64_t lse_stride,
                   float scale, int flags, int window_left, int window_right, void* hip_stream);
int fa2_bwd_varlen(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                   void* dq, void* dk, void* dv, float* delta_ws,
                   int B, int H, int max_seqlen_q, int max_seqlen_k, int D,
                   const int* cu_seqlens_q, const int* cu_seqlens_k,
                   const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2],
                   const int64_t o_strides[2], const int64_t do_strides[2], const int64_t dq_strides[2],
                   const int64_t dk_strides[2], const int64_t dv_strides[2], int64_t lse_stride,
                   float scale, int flags, int window_left, int window_right, void* hip_stream);
/*
 * Packed attention with V narrower than K: the non-absorbed prefill of multi-head-latent attention (q and k 192 wide — 128 "nope" plus 64 rotary
 * columns —, v 128 wide).  Forward only, packed layout only.  fa2_fwd_varlen's argument list with Dv after D:
 *   q              : [total_q, H, D]      k : [total_k, Hkv, D]      v : [total_k, Hkv, Dv]      o : [total_q, H, Dv]
 * Served pairs: D a multiple of 8 in 136 .. 256 and Dv a multiple of 8 in 8 .. 128; (192, 128) is the pair the call exists for.
 * v's strides are its own and independent of Dv — typically the slice [..., 128:256] of the up-projection's output: columns of that buffer at or beyond
 * Dv are never fetched, and nothing of o beyond column Dv is written.  Everything else is fa2_fwd_varlen's: device cu_seqlens, zero-length sequences,
 * grouped K / V not expanded, the flags and the window, rows that see no key (O = 0, lse = -inf), one owner per element of o[:, :, :Dv] and lse below
 * cu[B], contract 0, lse in log2 units.  scale is the caller's (D ** -0.5 for the plain softmax scale, not Dv ** -0.5).
 * Validation: fa2_fwd_varlen's order and codes; in addition Dv < 1 is FA2_ERR_BAD_SHAPE (with the other sizes), a pair outside the served set
 * FA2_ERR_HEAD_DIM (where the head dim is checked), and v's span rule counts Dv columns in its last row.
 * Kernel (FA2_KERNEL_HIP_VARLEN_DV, csrc/varlen_dv_hip.cpp): the packed kernel of head dim 256 run as ONE 128-column slab, with ceil(D / 16) Q.K^T
 * k-steps rounded up to 12 (D <= 192) or 16 and ceil(Dv / 32) O column blocks.  With the same "rows" the result equals fa2_fwd_varlen on v zero-padded
 * to D, sliced to Dv, bit for bit: the skipped k-steps and the skipped slab only ever multiplied zeros.  Option "rows" picks 128- or 256-row workgroups.
 */
int fa2_fwd_varlen_dv(int dtype,
                      const void* q, const void* k, const void* v, void* o, float* lse,
                      int B, int H, int Hkv, int max_seqlen_q, int max_seqlen_k, int D, int Dv,
                      const int* cu_seqlens_q, const int* cu_seqlens_k,
                      const int64_t q_strides[2], const int64_t k_strides[2],
                      const int64_t v_strides[2], const int64_t o_strides[2],
                      int64_t lse_stride,
                      float scale, int flags, int window_left, int window_right, void* hip_stream);
/* The per-sequence range arithmetic of the packed kernels: fa2_window_tile_range / fa2_window_row_range for one sequence of Nq_s queries and Nkv_s
 * keys (>= 0), the offset derived from `flags` (FA2_FLAG_BOTTOM_RIGHT: Nkv_s - Nq_s, which may be negative — the windowed queries above keep
 * refusing negative offsets; FA2_FLAG_CAUSAL: window_right = 0).  Pure host arithmetic. */
int fa2_varlen_tile_range(int Nq_s, int Nkv_s, int window_left, int window_right, int flags,
                          int row0, int rows, int tile, int* first_tile, int* ntiles);
int fa2_varlen_row_range(int Nq_s, int Nkv_s, int window_left, int window_right, int flags,
                         int key0, int keys, int tile, int* first_tile, int* ntiles);

/*
 * Attention dropout: the windowed and the packed entry points with a dropout probability and a seed.
 *   fa2_fwd_dropout / fa2_bwd_dropout               fa2_fwd_window's / fa2_bwd_window's argument lists, then float dropout_p, uint64_t seed
 *   fa2_fwd_varlen_dropout / fa2_bwd_varlen_dropout  fa2_fwd_varlen's / fa2_bwd_varlen's argument lists, then the same two
 * Everything those entry points document holds (window_left = window_right = -1, q_offset = 0 is full attention; grouped K / V in the forward, the
 * multi-head backward; layouts; validation), except that these calls always run the dropout kernels (FA2_DROP forms of the compiler-scheduled windowed /
 * packed kernels, every head dim up to 512), whatever the window masks.
 * The mask (csrc/fa2_dropout.h has the contract in full).  Whether the probability at (b, h, i, j) — batch or sequence b, QUERY head h, row i, key j, the
 * latter two counted inside the sequence — is kept is a pure function of (seed, b * H + h, i, j) and the threshold: Philox4x32-10 keyed by the seed,
 * counter { call(j), i, b * H + h, 0 }, sixteen bits per element, dropped when they are < t = round(dropout_p * 65536) (clamped to 65535).  So
 * p_eff = t / 65536 and the kept probabilities are scaled by 1 / (1 - p_eff).  It does not depend on tile sizes, option "rows", head dim, dtype, layout,
 * grouped or expanded K / V, or the pass: the backward regenerates the forward's mask from the same seed.
 * Numerics.  The softmax state is untouched: the row sum and the LSE are those of the undropped probabilities (the LSE of a dropout call is the LSE of the
 * same call without dropout).  O = (sum_j keep P16 V) / l / (1 - p_eff); dV = (keep o P16)^T dO / (1 - p_eff); dP = keep o (dO V^T) / (1 - p_eff),
 * dS = P o (dP - delta), delta = rowsum(dO o O).  Contract 0 (f32 scale of the product); a row that sees no key returns zeros.
 * dropout_p == 0 keeps everything.  dropout_p < 0, >= 1 or NaN: FA2_ERR_DROPOUT, reported before anything else is looked at.
 * The seed is a host value: a call captured in a graph replays the same mask.
 */
int fa2_fwd_dropout(int dtype,
                    const void* q, const void* k, const void* v, void* o, float* lse,
                    int B, int H, int Hkv, int Nq, int Nkv, int D,
                    const int64_t q_strides[3], const int64_t k_strides[3],
                    const int64_t v_strides[3], const int64_t o_strides[3],
                    const int64_t lse_strides[2],
                    float scale, int flags, int window_left, int window_right, int q_offset, void* hip_stream,
                    float dropout_p, uint64_t seed);
int fa2_bwd_dropout(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                    void* dq, void* dk, void* dv, float* delta_ws,
                    int B, int H, int Nq, int Nkv, int D,
                    const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                    const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                    const int64_t dk_strides[3], const int64_t dv_strides[3], const int64_t lse_strides[2],
                    float scale, int flags, int window_left, int window_right, int q_offset, void* hip_stream,
                    float dropout_p, uint64_t seed);
int fa2_fwd_varlen_dropout(int dtype,
                           const void* q, const void* k, const void* v, void* o, float* lse,
                           int B, int H, int Hkv, int max_seqlen_q, int max_seqlen_k, int D,
                           const int* cu_seqlens_q, const int* cu_seqlens_k,
                           const int64_t q_strides[2], const int64_t k_strides[2],
                           const int64_t v_strides[2], const int64_t o_strides[2],
                           int64_t lse_stride,
                           float scale, int flags, int window_left, int window_right, void* hip_stream,
                           float dropout_p, uint64_t seed);
int fa2_bwd_varlen_dropout(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                           void* dq, void* dk, void* dv, float* delta_ws,
                           int B, int H, int max_seqlen_q, int max_seqlen_k, int D,
                           const int* cu_seqlens_q, const int* cu_seqlens_k,
                           const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2],
                           const int64_t o_strides[2], const int64_t do_strides[2], const int64_t dq_strides[2],
                           const int64_t dk_strides[2], const int64_t dv_strides[2], int64_t lse_stride,
                           float scale, int flags, int window_left, int window_right, void* hip_stream,
                           float dropout_p, uint64_t seed);
/* Host-only (no GPU needed).  fa2_dropout_keep_mask: mask[(i - i0) * (j1 - j0) + (j - j0)] = 1 where the element (b, h, i, j) is kept, 0 where it is
 * dropped, for the rectangle [i0, i1) x [j0, j1) of one (b, h) of a call with H query heads.  FA2_ERR_NULL_POINTER, FA2_ERR_BAD_SHAPE (negative or
 * empty ranges, b / h out of range), FA2_ERR_DROPOUT.
 * fa2_dropout_threshold: t of dropout_p (the return value, or FA2_ERR_DROPOUT), and p_eff = t / 65536 (p_eff may be NULL).
 * fa2_philox4x32_10: the generator itself, out = Philox4x32-10(ctr, key). */
int fa2_dropout_keep_mask(uint64_t seed, float dropout_p, int H, int b, int h, int64_t i0, int64_t i1, int64_t j0, int64_t j1, uint8_t* mask);
int fa2_dropout_threshold(float dropout_p, float* p_eff);
int fa2_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/*
 * Score modifiers — logit soft-capping and ALiBi slopes: the windowed and the packed entry points with three further arguments.
 *   fa2_fwd_scoremod / fa2_bwd_scoremod               fa2_fwd_window's / fa2_bwd_window's argument lists, then
 *   fa2_fwd_varlen_scoremod / fa2_bwd_varlen_scoremod  fa2_fwd_varlen's / fa2_bwd_varlen's argument lists, then
 *       float softcap, const float* alibi_slopes, int64_t alibi_batch_stride
 * Everything those entry points document holds (window_left = window_right = -1, q_offset = 0 is full attention; grouped K / V in the forward, the
 * multi-head backward; layouts; validation order).
 * Contract (csrc/fa2_scoremod.h has the arithmetic).  For query row i at key position pos = i + q_offset (packed: i + the sequence's offset — 0, or
 * Nkv_s - Nq_s under FA2_FLAG_BOTTOM_RIGHT) and key j:
 *     x  = (q_i . k_j) * scale                          f32: the MFMA product scaled in f32 (contract 0)
 *     s  = softcap > 0 ? softcap * tanh(x / softcap) : x
 *     s += alibi_slopes ? -slope[b, h] * |pos - j| : 0  h = the QUERY head; b = the batch, or the sequence of a packed call;
 *                                                       slope[b, h] = alibi_slopes[b * alibi_batch_stride + h]
 *     s  = -inf outside the band (window / causal / Nkv): the masks come LAST (tanh(-inf) = -1: capping a masked score would un-mask it)
 * The softmax state, the LSE (log2 units) and P are those of s.  Rows that see no key return zeros and lse = -inf.
 * Backward, with t = tanh(x / softcap): P is recomputed from s and the saved LSE, dS = P o (dP - delta), dX = dS o (1 - t^2) (f32, then rounded to the
 * I/O dtype for the dX.K and dX^T.Q products), dQ = scale dX K, dK = scale dX^T Q; dV is unchanged.  (The wave-pair dK / dV pass of head dims 65 .. 128
 * hands round16(P o (1 - t^2)) from one wave to the other: there dX = round16(round16(P (1 - t^2)) o (dP - delta)).)  The slopes are constants of the
 * call and get no gradient.
 * softcap = 0 means off; softcap < 0, NaN, inf or a positive value below the smallest normal float (1.18e-38: its reciprocal overflows): FA2_ERR_SOFTCAP,
 * reported before anything else is looked at.  Slopes of either sign are served.  alibi_slopes: f32 in device memory, one
 * value per QUERY head, NULL = off; alibi_batch_stride = elements between the vectors of two batches / sequences, 0 = one [H] vector for all; a negative
 * stride is FA2_ERR_BAD_SHAPE and a pointer that is not 4-byte aligned FA2_ERR_ALIGNMENT — these two come next, in this order, before the checks of
 * the windowed / packed call.
 * With softcap == 0 and alibi_slopes == NULL the call IS the windowed / packed call of the same arguments: same kernels, bit-identical results.
 * Otherwise it always runs the score-modifier kernels (FA2_SMOD forms of the compiler-scheduled windowed / packed kernels, every head dim up to 512,
 * contract 0), whatever the window masks.  Not combined with dropout or a bias.
 */
int fa2_fwd_scoremod(int dtype,
                     const void* q, const void* k, const void* v, void* o, float* lse,
                     int B, int H, int Hkv, int Nq, int Nkv, int D,
                     const int64_t q_strides[3], const int64_t k_strides[3],
                     const int64_t v_strides[3], const int64_t o_strides[3],
                     const int64_t lse_strides[2],
                     float scale, int flags, int window_left, int window_right, int q_offset, void* hip_stream,
                     float softcap, const float* alibi_slopes, int64_t alibi_batch_stride);
int fa2_bwd_scoremod(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                     void* dq, void* dk, void* dv, float* delta_ws,
                     int B, int H, int Nq, int Nkv, int D,
                     const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                     const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                     const int64_t dk_strides[3], const int64_t dv_strides[3], const int64_t lse_strides[2],
                     float scale, int flags, int window_left, int window_right, int q_offset, void* hip_stream,
                     float softcap, const float* alibi_slopes, int64_t alibi_batch_stride);
int fa2_fwd_varlen_scoremod(int dtype,
                            const void* q, const void* k, const void* v, void* o, float* lse,
                            int B, int H, int Hkv, int max_seqlen_q, int max_seqlen_k, int D,
                            const int* cu_seqlens_q, const int* cu_seqlens_k,
                            const int64_t q_strides[2], const int64_t k_strides[2],
                            const int64_t v_strides[2], const int64_t o_strides[2],
                            int64_t lse_stride,
                            float scale, int flags, int window_left, int window_right, void* hip_stream,
                            float softcap, const float* alibi_slopes, int64_t alibi_batch_stride);
int fa2_bwd_varlen_scoremod(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                            void* dq, void* dk, void* dv, float* delta_ws,
                            int B, int H, int max_seqlen_q, int max_seqlen_k, int D,
                            const int* cu_seqlens_q, const int* cu_seqlens_k,
                            const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2],
                            const int64_t o_strides[2], const int64_t do_strides[2], const int64_t dq_strides[2],
                            const int64_t dk_strides[2], const int64_t dv_strides[2], int64_t lse_stride,
                            float scale, int flags, int window_left, int window_right, void* hip_stream,
                            float softcap, const float* alibi_slopes, int64_t alibi_batch_stride);
/* Host-only (no GPU needed): the transform itself, through the inline functions the kernels call.  *s = the modified score of the scaled score x
 * for key position pos and key j (slope 0: no ALiBi term), *dfactor = ds / dx = 1 - tanh^2(x / softcap) (1 when softcap == 0).
 * FA2_ERR_SOFTCAP, FA2_ERR_NULL_POINTER. */
int fa2_scoremod_eval(float x, float softcap, float slope, int pos, int j, float* s, float* dfactor);

/* ---- A gradient for the LSE.
 * The forward's `lse` is a result a caller may consume (merging attention over pieces of the KV axis: fa2_merge_fwd below), so the backward accepts a
 * gradient for it.  `dlse`: f32 in device memory, the gradient of the loss with respect to the `lse` the forward wrote — in ITS unit, log2 — addressed
 * dlse[b * dlse_strides[0] + h * dlse_strides[1] + row] (packed: dlse[h * dlse_stride + t]); strides of its own, so a compact gradient needs no padded
 * copy.  With natural-log lse_n = lse * ln 2, d lse_n[i] / d s[i][j] = P[i][j], hence dS = P (dP - delta + dlse_n): the dQ pass replaces the row term
 * delta[i] by delta[i] - log2(e) * dlse[i] (a caller holding the natural-log gradient g passes g * ln 2) before it uses it and before it stores it to
 * delta_ws, which therefore holds the modified value.  This holds under dropout (the LSE is that of the undropped P) and under soft-capping.  A row
 * whose saved lse is -inf (it saw no key) ignores its dlse entirely: even a NaN there yields zero gradients.
 * Each entry point is a superset of a family; with dlse == NULL it IS the existing call of the same arguments (same kernels, same plan, bit-identical
 * results).  With a dlse, head dim 128 runs the compiler-scheduled passes (the hand-scheduled bodies form delta inside generated code):
 * fa2_bwd_lse_plan reports it.
 *   fa2_bwd_lse          fa2_bwd_bias_ws's arguments (bias_kind = FA2_BIAS_NONE: fa2_bwd_ws), then the dlse pair.
 *   fa2_bwd_window_lse   fa2_bwd_window's arguments, then fa2_bwd_dropout's (dropout_p, seed) and fa2_bwd_scoremod's (softcap, alibi_slopes,
 *                        alibi_batch_stride), then the dlse pair.  dropout_p > 0: the call is fa2_bwd_dropout; softcap > 0 or slopes: fa2_bwd_scoremod;
 *                        neither: fa2_bwd_window.  Checked first, in this order: dropout_p (FA2_ERR_DROPOUT), the score-modifier arguments (their
 *                        codes), both at once (FA2_ERR_DROPOUT: the kernels have no such form).
 *   fa2_bwd_varlen_lse   the same for fa2_bwd_varlen; dlse_stride = elements between two heads' rows.
 * The dlse arguments are checked LAST: a pointer that is not 4-byte aligned FA2_ERR_ALIGNMENT, a negative stride FA2_ERR_BAD_SHAPE. */
int fa2_bwd_lse(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                void* dq, void* dk, void* dv, float* delta_ws, int B, int H, int Nq, int Nkv, int D,
                const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],
                const int64_t do_strides[3], const int64_t dq_strides[3], const int64_t dk_strides[3], const int64_t dv_strides[3],
                const int64_t lse_strides[2], float scale, int causal,
                const void* bias, int bias_kind, const int64_t bias_strides[3], void* workspace, size_t workspace_bytes, void* hip_stream,
                const float* dlse, const int64_t dlse_strides[2]);
int fa2_bwd_window_lse(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                       void* dq, void* dk, void* dv, float* delta_ws, int B, int H, int Nq, int Nkv, int D,
                       const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],
                       const int64_t do_strides[3], const int64_t dq_strides[3], const int64_t dk_strides[3], const int64_t dv_strides[3],
                       const int64_t lse_strides[2], float scale, int flags, int window_left, int window_right, int q_offset, void* hip_stream,
                       float dropout_p, uint64_t seed, float softcap, const float* alibi_slopes, int64_t alibi_batch_stride,
                       const float* dlse, const int64_t dlse_strides[2]);
int fa2_bwd_varlen_lse(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                       void* dq, void* dk, void* dv, float* delta_ws, int B, int H, int max_seqlen_q, int max_seqlen_k, int D,
                       const int* cu_seqlens_q, const int* cu_seqlens_k,
                       const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2],
                       const int64_t o_strides[2], const int64_t do_strides[2], const int64_t dq_strides[2],
                       const int64_t dk_strides[2], const int64_t dv_strides[2], int64_t lse_stride,
                       float scale, int flags, int window_left, int window_right, void* hip_stream,
                       float dropout_p, uint64_t seed, float softcap, const float* alibi_slopes, int64_t alibi_batch_stride,
                       const float* dlse, int64_t dlse_stride);

/* ---- Merge of partial attention results.
 * nparts (1 .. 16) calls over disjoint pieces of the KV axis left (O_k, lse_k); per row
 *     m = max_k lse_k,   w_k = 2^(lse_k - m) / sum_k 2^(lse_k - m),   O = sum_k w_k O_k (f32, rounded once),   lse = m + log2 sum_k 2^(lse_k - m)
 * is the result over the union.  A row whose parts are all -inf gives O = 0, lse = -inf; a part of weight exactly 0 is not read (its O_k may hold
 * anything).  o_parts / lse_parts (and do_parts / dlse_parts) are HOST arrays of device pointers, copied into the kernel's argument block: no device
 * copy, and the call can be captured in a graph.  All parts share one stride set: part_strides {batch, head, row} in elements (D contiguous),
 * part_lse_strides {batch, head} (rows contiguous) — the forward's O and padded L buffers can be passed as they are.  The packed layout [total, H, D] /
 * [H, total] is the same call with B = 1, Nq = total and the matching strides.  D: a multiple of 8, up to 512.  flags: FA2_MERGE_NATURAL_LSE = every
 * LSE (in and out, and their gradients) is natural-log; clear = log2, as fa2_fwd writes them.
 * fa2_merge_bwd: dO_k = w_k dO (rounded to the I/O dtype), dlse_k = w_k (dlse + dO.(O_k - O)), with dO.O formed as sum_k w_k (dO.O_k) in f32 (the
 * merged O is not read) and the dot term scaled by ln 2 when the LSEs are log2; `lse` is the merged LSE the forward wrote, dlse (may be NULL = zeros)
 * its gradient with strides dlse_strides; dout has do_strides, the parts' gradients dpart_strides / dpart_lse_strides.  Dead rows and zero-weight
 * parts get zeros.  No atomics: every output element has one owner.
 * Errors: FA2_ERR_DTYPE; nparts outside 1 .. 16, a size < 1, an unknown flag bit or a negative stride FA2_ERR_BAD_SHAPE; FA2_ERR_HEAD_DIM;
 * FA2_ERR_NULL_POINTER; tensors not 16-byte (LSEs: 4-byte) aligned or strides not multiples of 8 elements FA2_ERR_ALIGNMENT; FA2_ERR_GRID. */
enum { FA2_MERGE_NATURAL_LSE = 1 };
int fa2_merge_fwd(int dtype, int nparts, const void* const* o_parts, const float* const* lse_parts, void* o, float* lse,
                  int B, int H, int Nq, int D, const int64_t part_strides[3], const int64_t part_lse_strides[2],
                  const int64_t o_strides[3], const int64_t lse_strides[2], int flags, void* hip_stream);
int fa2_merge_bwd(int dtype, int nparts, const void* const* o_parts, const float* const* lse_parts, const float* lse,
                  const void* dout, const float* dlse, void* const* do_parts, float* const* dlse_parts,
                  int B, int H, int Nq, int D, const int64_t part_strides[3], const int64_t part_lse_strides[2],
                  const int64_t lse_strides[2], const int64_t do_strides[3], const int64_t dlse_strides[2],
                  const int64_t dpart_strides[3], const int64_t dpart_lse_strides[2], int flags, void* hip_stream);

/* ---- KV-cache decode attention: a few new query tokens per sequence against a preallocated cache whose valid length lives on the device.
 * Layout (element strides {batch, head, row}, D contiguous, as everywhere; the call takes the [B, Nq, H, D] / [B, Nmax, Hkv, D] tensors of other
 * libraries' kv-cache calls through their strides)
 *   q, o          : B x H x Nq x D.
 *   k_cache, v_cache, page_size == 0 : B x Hkv x capacity x D — a contiguous cache of `capacity` (Nmax) key slots per sequence.
 *   k_cache, v_cache, page_size  > 0 : num_pages x Hkv x page_size x D (strides[0] = the page stride); key j of sequence b lies in page
 *                   block_table[b * block_table_stride + j / page_size] at slot j % page_size; `capacity` = the block-table entries per sequence.
 *                   page_size is a multiple of 64, so a key tile never straddles a page.
 *   cache_seqlens : int32[B], DEVICE memory: the valid keys of each sequence, INCLUDING the Nq new tokens (their K / V are in the cache already).
 *   block_table   : int32, DEVICE memory (paged calls only).
 *   lse           : f32 B x H x Nq, lse_strides {batch, head}, log2 units as everywhere.
 * The host reads neither cache_seqlens nor block_table: no synchronisation, the call can be captured in a graph, and a replay after they changed in
 * place computes the result for the new contents.  The plan (below) depends on the shape, `capacity` and the CU count only, never on the lengths.
 * Masking: bottom-right causal per sequence.  With len = clamp(cache_seqlens[b], 0, capacity_keys) (capacity_keys = capacity, paged: capacity *
 * page_size), query row i sits at position len - Nq + i and sees the keys j <= that position.  Rows at a negative position (len < Nq) see no key:
 * O = 0, lse = -inf.  Keys at or beyond len and pages beyond the used ones contribute nothing WHATEVER they hold, NaN and Inf in K and in V included.
 * No content of cache_seqlens or block_table can make the kernel read outside the two cache allocations: len is clamped as above (fa2_decode_part_range),
 * every page id into [0, num_pages).  A wrong length gives a wrong answer, not a fault.
 * Shapes: Hkv divides H; D is 64 or 128 (FA2_ERR_HEAD_DIM otherwise); Nq * (H / Hkv) <= 64 query rows per K / V head — longer chunks are
 * fa2_fwd_varlen's; num_splits 0 (the plan chooses) or 1 .. 16 (forced).  A bad row count, page_size, num_splits: FA2_ERR_BAD_SHAPE.
 * Checked in this order: null pointers (block_table only when paged), sizes, head dim, alignment (16-byte tensors, 4-byte lse / cache_seqlens /
 * block_table, strides multiples of 8 with a positive row stride, a non-negative block-table stride), dtype, scale, FA2_ERR_GRID (B or Hkv above
 * 65535), and last the workspace: with a split above 1 it must be non-null (FA2_ERR_NULL_POINTER), 16-byte aligned (FA2_ERR_ALIGNMENT) and hold
 * fa2_fwd_decode_workspace_bytes(...) bytes (FA2_ERR_BAD_SHAPE).  It is private to the call until the stream has passed it.
 * Kernel (FA2_KERNEL_HIP_DECODE, csrc/fa2_decode.hip.h; contract 0: f32 scale of the product, f32 softmax state and row sums, P rounded RNE to the
 * I/O dtype before P.V, f32 accumulator).  One workgroup per (sequence, K / V head, part): the Nq * G rows of the group are the M rows of
 * v_mfma_f32_16x16x32 in `row_tiles` tiles of 16, so K and V are fetched once per group.  With a split of 1 the kernel writes o / lse itself;
 * otherwise the parts leave normalised f32 rows and log2 LSEs of the live rows in the workspace (an empty part: lse = -inf, no O) and a second
 * kernel merges them and rounds once (all parts empty: zeros and -inf).  No atomics.
 * Writing the new tokens' K / V into the cache, rotating q and k and quantising to e4m3 is fa2_kvcache_append (its own section, below): one launch
 * in front of this call, on the same stream.  A sliding window, soft-capping and ALiBi slopes are fa2_fwd_decode_window (below).  Not here: a backward. */
enum { FA2_KERNEL_HIP_DECODE = 7 };     /* (an enumerator, like FA2_KERNEL_HIP_WINDOW) */
typedef struct fa2_decode_plan_t {
    int kernel;        /* FA2_KERNEL_HIP_DECODE */
    int nsplit;        /* parts per (sequence, K / V head); 1: no workspace, no combine kernel */
    int row_tiles;     /* row tiles of 16 query rows per K / V head the kernel runs (1, 2 or 4) */
    int key_tile;      /* keys per tile: the `tile` of fa2_decode_part_range */
} fa2_decode_plan_t;
int fa2_fwd_decode(int dtype, const void* q, const void* k_cache, const void* v_cache, void* o, float* lse,
                   const int* cache_seqlens, const int* block_table,
                   int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_pages,
                   const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],
                   const int64_t lse_strides[2], int64_t block_table_stride,
                   float scale, int num_splits, void* workspace, size_t workspace_bytes, void* hip_stream);
/* The plan of that call (the launch executes the same one) and its workspace: pure host functions of the arguments and the device's CU count.
 * Split rule: 1 when B * Hkv * row_tiles workgroups' worth of row tiles already cover the CUs, else floor(2 * CUs / (B * Hkv * row_tiles)), at most 16
 * and at most one part per 8 key tiles of the capacity.  fa2_fwd_decode_workspace_bytes: B * Hkv * nsplit * Nq * (H / Hkv) * (D + 1) * 4, 0 for a
 * split of 1; 0 as well for arguments the call would refuse. */
int fa2_fwd_decode_plan(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits, fa2_decode_plan_t* plan);
size_t fa2_fwd_decode_workspace_bytes(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits);
/* The key tiles part `part` of `nsplit` sweeps for a sequence of `len` keys — the host side of the one function the kernel calls
 * (csrc/fa2_decode.hip.h: decode_part_range).  len is clamped into [0, capacity_keys]; tiles = ceil(len / tile), per = ceil(tiles / nsplit), the
 * part takes [part * per, min((part + 1) * per, tiles)): [*first_tile, *first_tile + *ntiles), ntiles = 0 for an empty part.
 * FA2_ERR_NULL_POINTER; FA2_ERR_BAD_SHAPE for capacity_keys < 0, Nq < 1, tile < 1, nsplit outside 1 .. 16 or part outside [0, nsplit). */
int fa2_decode_part_range(int64_t len, int64_t capacity_keys, int Nq, int tile, int nsplit, int part, int* first_tile, int* ntiles);

/* ---- ... on FP8 caches: fa2_fwd_decode with k_cache / v_cache in OCP e4m3 (gfx950's FP8: torch.float8_e4m3fn, not MI300's fnuz; no e5m2) and one f32
 * descale per (sequence, K / V head).  `dtype` stays the dtype of q and o (f16 or bf16); the cache strides are in elements, which here are bytes.
 *   k_descale, v_descale : f32 B x Hkv, DEVICE memory, descale_strides {batch, K / V head}; either may be null = 1.0 (both null: descale_strides may be).
 *                          Like cache_seqlens the host never reads them: a captured call replays correctly after they changed in place.
 * Meaning: K = float(k_cache) * k_descale[b, hkv], V = float(v_cache) * v_descale[b, hkv]; everything else — layouts, paging, masking, dead rows, the
 * clamps, num_splits, the workspace, lse — is fa2_fwd_decode's.  Every finite e4m3 value is a f16 and a bf16 value, so the in-register conversion
 * rounds nothing; k_descale is folded into the f32 score scale (scale * log2(e) * k_descale), v_descale multiplies the normalised f32 row before its one
 * rounding (a split call: before the row goes to the workspace), the LSE is that of the descaled scores.  Contract 0 otherwise.
 * e4m3 has NaN codes (0x7f, 0xff) and no Inf: keys at or beyond len still contribute nothing whatever the bytes are.  A NaN descale poisons its own
 * (sequence, K / V head) only.  No content of any device input can move an address.
 * Checked in this order: null pointers (block_table only when paged; descale_strides when a descale is given), sizes (as fa2_fwd_decode; a negative
 * descale stride), head dim, alignment (16-byte q / o / caches, CACHE strides multiples of 16 — one 16-byte load covers 16 columns —, q / o strides
 * multiples of 8, positive row strides, 4-byte lse / cache_seqlens / block_table / descales, a non-negative block-table stride), dtype, scale,
 * FA2_ERR_GRID, and last the workspace (null, alignment, size) as in fa2_fwd_decode.
 * Plan and workspace: the fp8 kernel sweeps the same 32-key tiles under the same split rule, so both functions answer as the 16-bit pair does; they
 * are pure host functions of shape, capacity and CU count.  plan.key_tile is the tile the fp8 kernel uses. */
int fa2_fwd_decode_fp8(int dtype, const void* q, const void* k_cache, const void* v_cache, void* o, float* lse,
                       const int* cache_seqlens, const int* block_table,
                       int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_pages,
                       const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],
                       const int64_t lse_strides[2], int64_t block_table_stride, float scale,
                       const float* k_descale, const float* v_descale, const int64_t descale_strides[2],
                       int num_splits, void* workspace, size_t workspace_bytes, void* hip_stream);
int fa2_fwd_decode_fp8_plan(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits, fa2_decode_plan_t* plan);
size_t fa2_fwd_decode_fp8_workspace_bytes(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits);

/* ---- ... with a sliding window, logit soft-capping and ALiBi slopes: the superset of the two entries above (cache_format: FA2_CACHE_16BIT or
 * FA2_CACHE_E4M3, the constants of fa2_kvcache_append; descales belong to e4m3 caches).  Everything not named here is fa2_fwd_decode's / _fp8's.
 * With len = clamp(cache_seqlens[b], 0, capacity_keys), query row i at pos = len - Nq + i, query head h and key j:
 *     x  = (q_i . K_j) * scale                     f32; e4m3 cache: K_j is the descaled key, i.e. the factor is scale * k_descale[b, hkv]
 *     s  = softcap > 0 ? softcap * tanh(x / softcap) : x
 *     s -= slope[b, h] * (pos - j)                 alibi_slopes f32, DEVICE memory, slope[b, h] = alibi_slopes[b * alibi_stride + h] (alibi_stride 0:
 *                                                  one [H] vector for every sequence); null = no ALiBi.  h is the QUERY head.
 *     keep(j) = 0 <= j <= pos  and  (window_left < 0 or j >= pos - window_left)
 * The masks come last; the softmax, P, O and the LSE are those of s.  The arithmetic is csrc/fa2_scoremod.h's (smod_cap, smod_alibi: the tanh and the
 * float distance of the score-modifier entries).  Decode is causal, so the window has a left edge only.  window_left = -1, softcap = 0 and null
 * slopes is fa2_fwd_decode / fa2_fwd_decode_fp8 bit for bit, and so is a window that reaches across the whole cache for EVERY row
 * (window_left >= capacity_keys - 1: the last row sits at len - 1) without a cap and slopes: such calls run the plain kernels.  The slopes are device data the host never reads (a captured call
 * follows slopes changed in place); window_left and softcap are host values.
 * Keys below the window: lo = window_left < 0 ? 0 : max(0, len - Nq - window_left) is the lowest key any row of the sequence sees.  Keys below lo
 * contribute nothing WHATEVER they hold, NaN and Inf in K and in V included — the guarantee keys at or beyond len have, kept the same way (scores
 * replaced by -inf through a select on the position, V rows replaced by zero bits before they reach LDS).  A key tile that lies wholly below lo is
 * never swept: its block-table entry is never read and its page never addressed, so a server may free the pages that fell out of the window.  The
 * clamps of lengths, page ids and key indices apply to everything that is read; no device value, slopes included, can move an address.
 * Parts: fa2_decode_window_part_range — t0 = lo / tile, t1 = ceil(len / tile), per = ceil((t1 - t0) / nsplit), part s sweeps
 * [t0 + s * per, min(t0 + (s + 1) * per, t1)); with window_left = -1 it is fa2_decode_part_range.  Its argument checks are that function's, plus
 * window_left < -1: FA2_ERR_BAD_SHAPE.
 * Plan: fa2_fwd_decode_plan's rule with "at most one part per 8 key tiles of the capacity" read as "... of the span a sequence can sweep",
 * min(capacity tiles, ceil((window_left + Nq) / 32) + 1) when window_left >= 0 — still a pure host function of shape, capacity, CU count and
 * window_left, never of the lengths.  The workspace formula is unchanged.
 * Checked in fa2_fwd_decode_fp8's order with the new arguments where their kind is: null pointers; sizes (also window_left < -1, alibi_stride < 0);
 * head dim; alignment (also 4-byte alibi_slopes); dtype (also a cache_format that is neither constant, and descales with a 16-bit cache:
 * FA2_ERR_DTYPE, fa2_kvcache_append's answer); scale; softcap (FA2_ERR_SOFTCAP, the rule of fa2_fwd_scoremod); FA2_ERR_GRID; the workspace.
 * Every combination of D, row tiles, dtype and cache format is served; no instantiation uses scratch. */
int fa2_fwd_decode_window(int dtype, int cache_format, const void* q, const void* k_cache, const void* v_cache, void* o, float* lse,
                          const int* cache_seqlens, const int* block_table,
                          int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_pages,
                          const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],
                          const int64_t lse_strides[2], int64_t block_table_stride, float scale,
                          const float* k_descale, const float* v_descale, const int64_t descale_strides[2],
                          int window_left, float softcap, const float* alibi_slopes, int64_t alibi_stride,
                          int num_splits, void* workspace, size_t workspace_bytes, void* hip_stream);
int fa2_fwd_decode_window_plan(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits, int window_left,
                               fa2_decode_plan_t* plan);
size_t fa2_fwd_decode_window_workspace_bytes(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits,
                                             int window_left);
int fa2_decode_window_part_range(int64_t len, int64_t capacity_keys, int Nq, int window_left, int tile, int nsplit, int part, int* first_tile,
                                 int* ntiles);

/* ---- Decode attention on a multi-head-latent (MLA) KV cache: the decode step of DeepSeek-V2 / V3 / R1 style models with the up-projections absorbed
 * into the query and the output.  The cache holds ONE row of D = 576 columns per token, shared by all heads (512 of compressed KV, then 64 of rotary
 * key); its first Dv = 512 columns are also the value.  With len and the positions as in fa2_fwd_decode,
 *   o[b, h, i, :] = softmax_j(scale * q[b, h, i, :] . kv[b, j, :]) . kv[b, j, :512]      over the keys j <= len - Nq + i.
 *   q             : B x H x Nq x 576 (the absorbed query), o : B x H x Nq x 512; element strides {batch, head, row}, last dim contiguous.
 *   kv_cache      : page_size == 0: B x capacity x 576; page_size > 0: num_pages x page_size x 576 under block_table, page_size a multiple of 64.
 *                   kv_strides {batch | page, head, row}: the head stride is not used (there is one latent head) but is checked like the others.
 *   cache_seqlens, block_table, lse, capacity, num_pages, block_table_stride : fa2_fwd_decode's, device data the host never reads (graph replay).
 * Masking, dead rows (O = 0, lse = -inf), keys at or beyond len (nothing, whatever they hold) and the clamps of lengths and page ids are
 * fa2_fwd_decode's.  Addresses are formed in 64 bits: a pool may exceed 4 GiB.
 * Shapes: H 1 .. 128 and Nq * H <= 512 packed rows r = i * H + h; num_splits 0 (the plan chooses) or 1 .. 128 (fa2_decode_mla_plan_t.max_split);
 * page_size as above: FA2_ERR_BAD_SHAPE otherwise.  D != 576 or Dv != 512: FA2_ERR_HEAD_DIM, looked at after those.
 * Checked in fa2_fwd_decode's order: null pointers (block_table only when paged), sizes, head dim, alignment, dtype, scale, FA2_ERR_GRID (B above
 * 65535), and last the workspace (null, alignment, size) when the split is above 1.
 * Kernel (FA2_KERNEL_HIP_DECODE_MLA, csrc/fa2_decode_mla.hip.h; contract 0 as fa2_fwd_decode): one workgroup of four waves per (sequence, block of
 * up to 64 packed rows, part); each 32-key tile of the cache is loaded once per workgroup into LDS and serves both products; each wave owns 16 rows.
 * A split call leaves normalised f32 rows and log2 LSEs of the live rows in the workspace (an empty part: lse = -inf alone) and the combine kernel of
 * fa2_fwd_decode, at head dim 512, merges them.  No atomics.
 * Writing new tokens into the 576-wide cache is fa2_kvcache_append_mla (its own section, below; fa2_kvcache_append stops at head dim 512 and rotates
 * the LEADING columns).  Not here: e4m3 latents, a window, soft-capping, slopes, a backward. */
enum { FA2_KERNEL_HIP_DECODE_MLA = 9 };     /* (an enumerator, like FA2_KERNEL_HIP_WINDOW) */
typedef struct fa2_decode_mla_plan_t {
    int kernel;        /* FA2_KERNEL_HIP_DECODE_MLA */
    int nsplit;        /* parts per (sequence, row block); 1: no workspace, no combine kernel */
    int row_blocks;    /* blocks of up to 64 packed rows: ceil(Nq * H / 64) */
    int key_tile;      /* keys per tile (32) */
    int max_split;     /* the largest num_splits the call takes (128) */
} fa2_decode_mla_plan_t;
int fa2_fwd_decode_mla(int dtype, const void* q, const void* kv_cache, void* o, float* lse,
                       const int* cache_seqlens, const int* block_table,
                       int B, int H, int Nq, int D, int Dv, int capacity, int page_size, int num_pages,
                       const int64_t q_strides[3], const int64_t kv_strides[3], const int64_t o_strides[3],
                       const int64_t lse_strides[2], int64_t block_table_stride,
                       float scale, int num_splits, void* workspace, size_t workspace_bytes, void* hip_stream);
/* The plan of that call and its workspace: pure host functions of the shape, the capacity and the device's CU count, never of the lengths.
 * Split rule: 1 when B * row_blocks workgroups cover the CUs (a workgroup fills a CU), else floor(CUs / (B * row_blocks)), at most 128 and at most one
 * part per 8 key tiles of the capacity (a shorter part moves more workspace than cache).  Workspace: B * nsplit * Nq * H * (512 + 1) * 4 bytes, 0 for
 * a split of 1 and for arguments the call would refuse. */
int fa2_fwd_decode_mla_plan(int dtype, int B, int H, int Nq, int D, int Dv, int capacity, int page_size, int num_splits, fa2_decode_mla_plan_t* plan);
size_t fa2_fwd_decode_mla_workspace_bytes(int dtype, int B, int H, int Nq, int D, int Dv, int capacity, int page_size, int num_splits);
/* The host side of the functions the kernel calls (csrc/fa2_decode_mla.hip.h: mla_part_range, mla_tile).
 * fa2_decode_mla_part_range: fa2_decode_part_range's rule on 32-key tiles with nsplit in 1 .. 128.
 * fa2_decode_mla_tile: where 32-key tile `tile` of a sequence lies — len is clamped into [0, capacity_keys] (capacity_keys = capacity, paged:
 * capacity * page_size); *page_slot = the block-table slot of its page (contiguous: 0), *row_in_page its first row there, *valid_rows how many of its 32
 * rows hold a key of the sequence (0: the tile lies at or beyond the length).  FA2_ERR_NULL_POINTER; FA2_ERR_BAD_SHAPE for capacity < 1, a page size
 * that is no multiple of 64, or a tile outside [0, ceil(capacity_keys / 32)). */
int fa2_decode_mla_part_range(int64_t len, int64_t capacity_keys, int nsplit, int part, int* first_tile, int* ntiles);
int fa2_decode_mla_tile(int64_t len, int capacity, int page_size, int tile, int* page_slot, int* row_in_page, int* valid_rows);

/* ---- KV-cache append: the write side of the decode calls.  One launch writes the K and V rows of Nnew new tokens per sequence into the cache at the
 * key position only the device knows, optionally rotates k (and q) by that position and optionally quantises to e4m3.
 * Layout (element strides {batch, head, row}, D contiguous)
 *   k_new, v_new  : B x Hkv x Nnew x D, the I/O dtype.
 *   k_cache, v_cache, cache_seqlens, block_table, capacity, page_size, num_pages, block_table_stride : as in fa2_fwd_decode; cache_format says what the
 *                   caches hold: FA2_CACHE_16BIT (the I/O dtype) or FA2_CACHE_E4M3 (OCP e4m3 bytes; element strides are bytes, as in fa2_fwd_decode_fp8).
 *   q, q_out      : optional, both or neither: B x H x Nq x D with Nq == Nnew and Hkv dividing H.  q is NOT rotated in place: the rotated rows go to
 *                   q_out, which the decode call then reads.  Refused without rotary tables (FA2_ERR_BAD_SHAPE): there would be nothing to do.
 *   rotary_cos, rotary_sin : optional, both or neither: [seqlen_ro, rotary_dim / 2], rows rotary_row_stride elements apart, f32 (rotary_dtype
 *                   FA2_DTYPE_F32) or the I/O dtype (rotary_dtype == dtype).  rotary_dim is a multiple of 16, 16 <= rotary_dim <= D.
 *   k_descale, v_descale, descale_strides : as in fa2_fwd_decode_fp8; e4m3 caches only (FA2_ERR_DTYPE with a 16-bit cache).
 * Semantics.  len = cache_seqlens[b] counts the valid keys INCLUDING the new tokens: it is the length after the append (a serving step increments the
 * lengths in place, appends, decodes).  New token i sits at key position p = len - Nnew + i, the position query row i of the decode call has.  A token
 * with p < 0 or p >= capacity_keys is SKIPPED, and so is a paged token whose page id lies outside [0, num_pages): nothing is written.  A position is
 * never clamped onto a valid row — a clamped write would destroy a live key.  No content of cache_seqlens or block_table can make the kernel write
 * outside the two cache allocations: a wrong value loses a token, it never faults.  fa2_kvappend_slot is the host side of that one mapping.
 * Rotary: new token i of k and row i of q are rotated by table row clamp(p, 0, seqlen_ro - 1) (a table that is too short gives a wrong answer, not a
 * fault).  rotary_interleaved != 0 pairs the columns (2j, 2j + 1) (GPT-J), 0 pairs (j, j + rotary_dim / 2) (GPT-NeoX); in f32
 * y1 = fma(x1, c, -(x2 s)), y2 = fma(x1, s, x2 c), each rounded once to the destination format.  Columns at or beyond rotary_dim pass through bit for
 * bit.  V is never rotated.  fa2_rotary_eval is the host side of that arithmetic (csrc/fa2_rotary.h).
 * 16-bit cache: V, and K without rotary, land bit for bit; rotated K is rounded once (RNE).  e4m3 cache: code = rne_e4m3(clamp(y / descale[b, hkv],
 * +-448)) with y the f32 value (rotated or not; never rounded to 16 bits first), a correctly rounded f32 division and the clamp in f32 BEFORE the
 * convert.  NaN in gives an e4m3 NaN code, +-Inf saturates to +-448, a null descale is 1.0; a NaN, zero or negative descale spoils its own (sequence,
 * K / V head) only and moves no address.
 * The host reads no device value: the call can be captured in a graph and replays for the lengths, block table and descales of that time.
 * Shapes: D a multiple of 8 (e4m3 caches: of 16) up to 512; Nnew >= 1 without an upper bound (a prefill chunk is a legitimate append); page_size a
 * multiple of 64.  Checked in this order: null pointers (block_table only when paged; q, q_out and their strides together; cos and sin together;
 * descale_strides when a descale is given), sizes (FA2_ERR_BAD_SHAPE: a size < 1, page_size, H % Hkv, Nq != Nnew, q without rotary, seqlen_ro < 1, a
 * negative table or descale stride), head dim and rotary_dim (FA2_ERR_HEAD_DIM), alignment (16-byte tensors and tables, 4-byte cache_seqlens /
 * block_table / descales, strides multiples of 8 — cache strides of an e4m3 cache multiples of 16 — with a positive row stride, a table row stride
 * that keeps rows 16-byte aligned, a non-negative block-table stride), dtype (dtype, cache_format, rotary_dtype, a descale with a 16-bit cache),
 * FA2_ERR_GRID (B * Nnew above 2^31 - 1).
 * Kernel (csrc/fa2_kvappend.hip.h): one workgroup slice per (sequence, token); a lane moves two 16-byte chunks of one row — 16 consecutive columns,
 * or, in the rotated span of a non-interleaved row, a chunk and its partner half a rotary span away, so that no value crosses lanes. */
#define FA2_DTYPE_F32 2          /* the rotary tables of fa2_kvcache_append only */
enum { FA2_CACHE_16BIT = 0, FA2_CACHE_E4M3 = 1 };
int fa2_kvcache_append(int dtype, int cache_format, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                       const int* cache_seqlens, const int* block_table,
                       int B, int Hkv, int Nnew, int D, int capacity, int page_size, int num_pages,
                       const int64_t k_new_strides[3], const int64_t v_new_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                       int64_t block_table_stride,
                       const void* q, void* q_out, int H, int Nq, const int64_t q_strides[3], const int64_t q_out_strides[3],
                       const void* rotary_cos, const void* rotary_sin, int rotary_dtype, int rotary_dim, int seqlen_ro, int64_t rotary_row_stride,
                       int rotary_interleaved,
                       const float* k_descale, const float* v_descale, const int64_t descale_strides[2], void* hip_stream);
/* The key position new token i of Nnew is written at — the host side of the one function the kernel calls (csrc/fa2_decode.hip.h: kvappend_slot):
 * *pos = len - Nnew + i when that lies in [0, capacity_keys), else -1 (skipped).  FA2_ERR_NULL_POINTER; FA2_ERR_BAD_SHAPE for capacity_keys < 0,
 * Nnew < 1 or i outside [0, Nnew). */
int fa2_kvappend_slot(int64_t len, int64_t capacity_keys, int Nnew, int i, int64_t* pos);
/* ---- Packed (ragged) KV-cache append: fa2_kvcache_append for a batch whose sequences bring DIFFERENT numbers of new tokens — the write side of
 * fa2_fwd_prefill, a continuous-batching step that mixes prefill chunks with decode rows.  One launch; what is not said here is fa2_kvcache_append's.
 * Layout (element strides {head, row}, as the packed attention calls take them; D contiguous)
 *   k_new, v_new  : total x Hkv x D, the I/O dtype: the new tokens of all sequences, packed.
 *   cu_seqlens    : int32 [B + 1], DEVICE: sequence s owns the packed rows [cu[s], cu[s + 1]), Nnew_s = cu[s + 1] - cu[s] may be 0.  cu[B] < total is
 *                   legitimate — a token buffer of a fixed (captured) size that this step fills only partly: the rows t >= cu[B], like rows
 *                   t < cu[0], belong to no sequence.
 *   q, q_out      : optional, both or neither: total x H x D, rotated as in fa2_kvcache_append (tables required).
 * Semantics.  Packed row t = cu[s] + i is new token i of sequence s and is treated as fa2_kvcache_append treats token i of Nnew_s: position
 * p = cache_seqlens[s] - Nnew_s + i, skipped when p lies outside [0, capacity_keys) or its page id outside [0, num_pages), rotated by table row
 * clamp(p, 0, seqlen_ro - 1), descaled by descale[s, hkv].  The q row of a token that belongs to a sequence is rotated whether or not its K / V is
 * written; the q row of a token that belongs to no sequence is copied to q_out bit for bit (q_out never holds uninitialised memory), and no K / V is
 * written for it.
 * cu_seqlens is device data nobody validated, like cache_seqlens and block_table.  The kernel finds s by a binary search whose probes stay inside
 * cu[1 .. B] whatever the array holds, then checks 0 <= cu[s] <= t < cu[s + 1]: on an array that is not ascending, holds negative entries or ends
 * above total a token either belongs to no sequence or gets a consistent (s, i, Nnew_s).  No content of cu_seqlens, cache_seqlens or block_table can
 * move a write outside the two caches and q_out, nor a read outside k_new, v_new, q and the tables: a wrong value loses a token, it never faults.  All
 * addressing is in 64 bits.  fa2_kvappend_varlen_token is the host side of the search (csrc/fa2_decode.hip.h: kvappend_varlen_token, one function).
 * The host reads no device value: the call can be captured in a graph and replays for the offsets, lengths, block table and descales of that time.
 * Checked in fa2_kvcache_append's order: null pointers (cu_seqlens too), sizes (FA2_ERR_BAD_SHAPE: B, Hkv, D < 1, total < 0, and the rest of that
 * list but Nq), head dim and rotary_dim, alignment (4-byte cu_seqlens too), dtype, FA2_ERR_GRID (total above 2^31 - 1).  total == 0 passes the checks
 * and returns FA2_OK without a launch. */
int fa2_kvcache_append_varlen(int dtype, int cache_format, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                              const int* cu_seqlens, const int* cache_seqlens, const int* block_table,
                              int B, int64_t total, int Hkv, int D, int capacity, int page_size, int num_pages,
                              const int64_t k_new_strides[2], const int64_t v_new_strides[2], const int64_t k_strides[3], const int64_t v_strides[3],
                              int64_t block_table_stride,
                              const void* q, void* q_out, int H, const int64_t q_strides[2], const int64_t q_out_strides[2],
                              const void* rotary_cos, const void* rotary_sin, int rotary_dtype, int rotary_dim, int seqlen_ro, int64_t rotary_row_stride,
                              int rotary_interleaved,
                              const float* k_descale, const float* v_descale, const int64_t descale_strides[2], void* hip_stream);
/* The sequence that owns packed token t — the host side of the one function the kernel calls; cu_seqlens is HOST memory of B + 1 ints here.
 * *seq in [0, B) with *i = t - cu[*seq] in [0, *nnew) and *nnew = cu[*seq + 1] - cu[*seq]; or *seq = -1 (*i = *nnew = 0): no sequence owns t.  Any
 * array contents give one of the two.  FA2_ERR_NULL_POINTER; FA2_ERR_BAD_SHAPE for B < 1. */
int fa2_kvappend_varlen_token(const int* cu_seqlens, int B, int64_t t, int* seq, int* i, int* nnew);
/* One row of D 16-bit values x rotated into y with the arithmetic the kernel calls (csrc/fa2_rotary.h): cos_row / sin_row hold rotary_dim / 2 floats;
 * columns at or beyond rotary_dim are copied bit for bit.  FA2_ERR_NULL_POINTER, FA2_ERR_BAD_SHAPE (D < 1), FA2_ERR_HEAD_DIM (D, rotary_dim),
 * FA2_ERR_DTYPE, in this order. */
int fa2_rotary_eval(int dtype, const void* x, const float* cos_row, const float* sin_row, int D, int rotary_dim, int interleaved, void* y);

/* ---- Append for a latent (MLA) KV cache: the write side of fa2_fwd_decode_mla.  One launch writes the rows of Nnew new tokens per sequence into the
 * 576-wide cache at the key position only the device knows, rotating the TRAILING 64 columns by that position, and optionally writes the rotated q.
 * Everything not said here is fa2_kvcache_append's contract, word for word: the lengths AFTER the append, p = len - Nnew + i, tokens with p outside
 * [0, capacity_keys) or a page id outside [0, num_pages) SKIPPED and never clamped onto a live row, device data nobody validated moving no write
 * outside kv_cache and q_out and no read outside kv_c, k_pe, q and the tables, 64-bit addressing, no host read of a device value (graph replay).
 * Layout (last dim contiguous)
 *   kv_c          : B x Nnew x 512, the compressed KV; k_pe : B x Nnew x 64, the rotary key; element strides {batch, row} each.  The two may be
 *                   slices of one projection output.
 *   kv_cache, cache_seqlens, block_table, capacity, page_size, num_pages, kv_strides, block_table_stride : as in fa2_fwd_decode_mla (D = 576, Dv = 512).
 *   q, q_out      : optional, both or neither: B x H x Nq x 576 with Nq == Nnew and H 1 .. 128, strides {batch, head, row}.  Needs the tables.
 *   rotary_cos, rotary_sin : optional, both or neither: [seqlen_ro, 32], f32 or the I/O dtype; rotary_dim is exactly 64.
 * The cache row at p receives kv_c[b, i, :] bit for bit in columns 0 .. 511 and k_pe[b, i, :] in columns 512 .. 575: rotated by table row
 * clamp(p, 0, seqlen_ro - 1) with tables (csrc/fa2_rotary.h's arithmetic in f32, one RNE rounding; fa2_rotary_eval on the 64-wide sub-row is its host
 * side), copied bit for bit without (a caller who rotated it already).  rotary_interleaved != 0 pairs the columns (512 + 2j, 512 + 2j + 1), 0 pairs
 * (512 + j, 512 + 32 + j).  q_out row i of every head: columns 0 .. 511 of q bit for bit, columns 512 .. 575 rotated by the table row of token i,
 * whether or not that token's latent row was written.  q itself is not touched.
 * Checked in fa2_kvcache_append's order: null pointers, sizes (FA2_ERR_BAD_SHAPE: B, Nnew, D, Dv < 1, page_size, H outside 1 .. 128, Nq != Nnew, q
 * without tables, seqlen_ro < 1, a negative table stride), head dim (FA2_ERR_HEAD_DIM: D != 576, Dv != 512, rotary_dim != 64), alignment, dtype,
 * FA2_ERR_GRID (B * Nnew above 2^31 - 1).  There is no cache_format and there are no descales: e4m3 latents are not served.
 * Kernel (csrc/fa2_kvappend_mla.hip.h): fa2_kvcache_append's decomposition with R = 1 + H rows of 36 units; a unit is two 16-byte chunks of a row's
 * 72 — fa2_kvappend_mla_chunks is the host side of that one map: (2u, 2u + 1), or with halves != 0 (a rotated GPT-NeoX tail) (64 + c, 68 + c) for
 * unit 32 + c.  FA2_ERR_NULL_POINTER; FA2_ERR_BAD_SHAPE for a unit outside [0, 36). */
int fa2_kvcache_append_mla(int dtype, const void* kv_c, const void* k_pe, void* kv_cache,
                           const int* cache_seqlens, const int* block_table,
                           int B, int Nnew, int D, int Dv, int capacity, int page_size, int num_pages,
                           const int64_t kv_c_strides[2], const int64_t k_pe_strides[2],
                           const int64_t kv_strides[3], int64_t block_table_stride,
                           const void* q, void* q_out, int H, int Nq, const int64_t q_strides[3], const int64_t q_out_strides[3],
                           const void* rotary_cos, const void* rotary_sin, int rotary_dtype, int rotary_dim, int seqlen_ro,
                           int64_t rotary_row_stride, int rotary_interleaved, void* hip_stream);
/* ... its packed (ragged) form, as fa2_kvcache_append_varlen is fa2_kvcache_append's: kv_c total x 512 and k_pe total x 64 with one row stride each
 * (kv_c_strides[1], k_pe_strides[1]), q and q_out total x H x 576 with {head, row}; cu_seqlens int32 [B + 1] on the device, cu[B] < total legitimate.
 * A token no sequence owns writes no latent row and its q row is copied to q_out bit for bit.  total == 0 passes the checks and returns FA2_OK
 * without a launch; FA2_ERR_GRID for total above 2^31 - 1. */
int fa2_kvcache_append_mla_varlen(int dtype, const void* kv_c, const void* k_pe, void* kv_cache,
                                  const int* cu_seqlens, const int* cache_seqlens, const int* block_table,
                                  int B, int64_t total, int D, int Dv, int capacity, int page_size, int num_pages,
                                  const int64_t kv_c_strides[1], const int64_t k_pe_strides[1],
                                  const int64_t kv_strides[3], int64_t block_table_stride,
                                  const void* q, void* q_out, int H, const int64_t q_strides[2], const int64_t q_out_strides[2],
                                  const void* rotary_cos, const void* rotary_sin, int rotary_dtype, int rotary_dim, int seqlen_ro,
                                  int64_t rotary_row_stride, int rotary_interleaved, void* hip_stream);
int fa2_kvappend_mla_chunks(int unit, int halves, int* chunk_a, int* chunk_b);

/* Head dims the forward kernels are instantiated for (ascending).  Writes up to `cap` entries into `dims`, returns
 * the total count.  Any D that is a multiple of 8 runs on the next of these with its tail columns masked; only a D
 * that is not a multiple of 8 has to be zero-padded by the caller (to the next multiple of 8). */
int fa2_supported_head_dims(int* dims, int cap);

/* Head dim of the kernel that serves D (the smallest instantiated one >= D), or -1 if D is larger than the largest. */
int fa2_padded_head_dim(int D);

/* Q rows per workgroup / KV rows per tile of the kernel chosen for head dim D (informational:
 * the counterparts of the reference's Br / Bc, FlashAttn.py:56-67). */
int fa2_tile_rows(int D, int* q_rows_per_block, int* kv_rows_per_tile);

/*
 * Which kernel serves a forward call, and which numerical contract its results follow — exact, per call (the launch code executes the
 * same plan this function reports; csrc/host.cpp: plan_fwd).
 *
 * Contracts.  The reference KERNEL scales the f32 Q.K^T product (`* scale`, kernel_fp16.cu:164; its Q prescale is commented out, :364) and
 * sums the unrounded f32 P; the reference's own ORACLE scales Q first, in the I/O dtype (`scale * q_frags`, pure_torch_ver.py:61).
 *   contract == 0                 the reference kernel's: S = (Q K^T) * scale*log2(e) in f32, row sums of the f32 P.  Every compiler-scheduled
 *                                 kernel, and the hand-scheduled bodies when they do not fold (bf16 by default; scale*log2(e) > 1; option "fold" = 0).
 *   FA2_CONTRACT_PRESCALE_Q       Q * scale*log2(e) is rounded ONCE to the I/O dtype before Q K^T (the reference oracle's contract) and the running
 *                                 reference maximum enters the first Q.K^T k-step as its C operand.  Removes the 64 v_fma per tile of bodies that run
 *                                 at their instruction-issue bound (+9 % at head dim 64, +1.4 ... +2.9 % at 128).  fp16: ~2e-4 of log2 LSE on
 *                                 U[0,1) / N(0,1) inputs, growing with the logits (~1e-2 in O at logits of several hundred); bf16: ~6e-3.
 *   FA2_CONTRACT_LSUM_P16         the row sums add the P values ROUNDED to the I/O dtype — the ones the P.V product consumes, so the weights O applies
 *                                 sum to exactly one; the LSE carries the rounding (fp16: <= 7e-4 of log2 LSE for a one-hot row, ~1e-4 on N(0,1)
 *                                 inputs).  Version 0.8's head-dim-64 body formed them on the matrix pipe; since round 5 the head-dim-128 bodies that
 *                                 fold the scale (option "fold", never a call flagged FA2_FLAG_EXACT_SCALE) built on v_mfma_f32_16x16x32 do: one MFMA
 *                                 with a constant operand per (16 rows, 32 kv) instead of 64 v_add_f32 per tile, -4 % of a launch.
 * Kernels.
 *   FA2_KERNEL_HIP_256 / _128     compiler-scheduled HIP kernel, 8-wave 256-row / 4-wave 128-row workgroups (csrc/fa2_fwd_kernel.hip.h)
 *   FA2_KERNEL_ASM                hand-scheduled 4-wave 256-row body (csrc/gen/fwd_d128_gen.py, fwd_m16_gen.py): head dims 64 and 128, and — on the
 *                                 16x16x32 bodies, padded columns zero-filled by the LDS-DMA — 40 .. 56 and 88 .. 120 (f32-scale kinds from 104);
 *                                 round 6: head dims 136 .. 256 (below 176: non-causal calls) on a 4-wave 128-row body (`rows` = 128; csrc/gen/fwd_m16_d256_gen.py: f32 scale,
 *                                 FA2_CONTRACT_LSUM_P16; calls flagged FA2_FLAG_EXACT_SCALE keep the compiler-scheduled kernels)
 *   FA2_KERNEL_HIP_BIAS           the BIAS forms of the HIP kernel (fa2_fwd_bias); `rows` is reported as 0 = unspecified for it: the load form, and with it
 *                                 128- or 256-row workgroups, depends on the bias strides and alignment, which this query does not take
 * A call is at most two launches: heads [0, heads_main) of the flattened (b * H + h) order run `kernel` under `contract`, the others (head dims
 * <= 64 whose last round of workgroups is nearly empty: a second launch of 128-row workgroups) run `kernel_tail` under `contract_tail`.
 * nsplit > 1: with a workspace of `workspace_bytes` the `split_items` items of the last round run as nsplit KV-split parts each (fa2_fwd_ws), inside `kernel`.
 *   q_strides / k_strides: as in fa2_fwd, or NULL for contiguous [B,H,N,D] tensors (the plan looks at the row pitches of Q and K only);
 *   bias_kind: FA2_BIAS_NONE for fa2_fwd / fa2_fwd_ws;  workspace_bytes: 0 for fa2_fwd.
 * Returns FA2_OK or the validation code the call itself would return.  Depends on the arguments, the options and the device's CU count.
 */
#define FA2_KERNEL_HIP_256  1
#define FA2_KERNEL_HIP_128  2
#define FA2_KERNEL_ASM      3
#define FA2_KERNEL_HIP_BIAS 4
#define FA2_CONTRACT_PRESCALE_Q 1
#define FA2_CONTRACT_LSUM_P16   2
typedef struct fa2_fwd_plan_t {
    int kernel, contract, rows;                 /* main launch: FA2_KERNEL_*, FA2_CONTRACT_* bits, Q rows per workgroup */
    int heads_main;                             /* flattened heads [0, heads_main) belong to it (B*H: the only launch) */
    int kernel_tail, contract_tail, rows_tail;  /* second launch over the remaining heads (0: none) */
    int nsplit, split_items;                    /* KV-split of the last round, or of every item of an underfilled grid (0: none) */
} fa2_fwd_plan_t;
int fa2_fwd_plan(int dtype, int B, int H, int Nq, int Nkv, int D,
                 const int64_t q_strides[3], const int64_t k_strides[3],
                 float scale, int causal, int bias_kind, size_t workspace_bytes, fa2_fwd_plan_t* plan);
/* The plan of fa2_fwd_gqa (k_strides: those of the [B, Hkv, Nkv, D] K, or NULL for a contiguous one): the MHA call's plan for the same shape. */
int fa2_fwd_gqa_plan(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D,
                     const int64_t q_strides[3], const int64_t k_strides[3],
                     float scale, int causal, size_t workspace_bytes, fa2_fwd_plan_t* plan);

/* The plan of fa2_bwd / fa2_bwd_ws / fa2_bwd_gqa (Hkv = H for the first two) and of fa2_bwd_bias: which kernel serves each of the two passes, for
 * these strides.  The launch code executes the same plan.
 *   FA2_BWD_KERNEL_HIP    the compiler-scheduled pass (every head dim, every layout the validation accepts: 64-bit row pointers for O, dQ, dK, dV)
 *   FA2_BWD_KERNEL_ASM    the hand-scheduled pass of head dim exactly 128 (row pitches of the staged matrices multiples of 128 elements; dK / dV pass:
 *                         Nq a multiple of 32, Hkv = H, and only beside the hand-scheduled dQ pass; dQ pass: O's span bounded like Q's — see the
 *                         span rules above)
 *   FA2_BWD_KERNEL_SHORT  (dQ pass) the single-pass kernel of non-causal sweeps of at most two KV tiles
 * Any stride array may be NULL: a contiguous [B, heads, N, D] tensor (dO and O: Q's shape).  dQ / dK / dV are described with Q's / K's / V's strides: no
 * pass looks at them.  bias_kind other than FA2_BIAS_NONE: fa2_bwd_bias (bias_strides as there, or NULL), both passes FA2_BWD_KERNEL_HIP.
 * Returns FA2_OK or the validation code the call itself would return with non-null, aligned tensors.
 * (Enumerators, like FA2_KERNEL_HIP_WINDOW below.) */
enum { FA2_BWD_KERNEL_HIP = 1, FA2_BWD_KERNEL_ASM = 2, FA2_BWD_KERNEL_SHORT = 3 };
typedef struct fa2_bwd_plan_t {
    int dq_kernel, dkv_kernel;                  /* FA2_BWD_KERNEL_* of the dQ (+ delta) pass and of the dK / dV pass */
} fa2_bwd_plan_t;
int fa2_bwd_plan(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D,
                 const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                 const int64_t o_strides[3], const int64_t do_strides[3],
                 float scale, int causal, int bias_kind, const int64_t bias_strides[3], fa2_bwd_plan_t* plan);
/* ... of fa2_bwd_lse: has_dlse = 0 is fa2_bwd_plan's answer; has_dlse = 1: what the launch with a dlse executes (no FA2_BWD_KERNEL_ASM pass). */
int fa2_bwd_lse_plan(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D,
                     const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                     const int64_t o_strides[3], const int64_t do_strides[3],
                     float scale, int causal, int bias_kind, const int64_t bias_strides[3], int has_dlse, fa2_bwd_plan_t* plan);

/* How fa2_fwd_bias fetches a bias of these strides whose pointer is 16-byte aligned (the forward accepts every bias; the form follows its geometry):
 *   FA2_BIAS_FORM_SCALAR    one guarded load per score
 *   FA2_BIAS_FORM_VEC4      one aligned load per four consecutive keys (Nkv and the strides multiples of 4)
 *   FA2_BIAS_FORM_TILE      coalesced tile loads through LDS from 64-bit row pointers (Nkv and the strides whole 16-byte granules, head dims <= 256)
 *   FA2_BIAS_FORM_TILE_DMA  the tile staged by LDS-DMA with 32-bit byte offsets into one (b, h) slice: the TILE geometry on a grid of more than 3/8 of
 *                           the CUs' worth of 256-row workgroups, head dims <= 128, the slice within the backward's bias span rule above
 *   FA2_BIAS_FORM_ROW       a bias broadcast over the Q rows (bias_strides[2] == 0), head dims <= 256
 * Returns the form (>= 0) or a validation code (< 0). */
enum { FA2_BIAS_FORM_SCALAR = 0, FA2_BIAS_FORM_VEC4 = 1, FA2_BIAS_FORM_TILE = 2, FA2_BIAS_FORM_TILE_DMA = 3, FA2_BIAS_FORM_ROW = 4 };
int fa2_fwd_bias_form(int bias_kind, int B, int H, int Nq, int Nkv, int D, const int64_t bias_strides[3]);

/* The plan of the windowed forward above.  kernel = FA2_KERNEL_HIP_WINDOW, contract 0, rows as launched — or, for a window that masks nothing, exactly the grouped plan query's answer.
 * (An enumerator, not a #define: the macro list above is the closed set tests/test_boundary.py pins for the other entry points' plans.) */
enum { FA2_KERNEL_HIP_WINDOW = 5 };
int fa2_fwd_window_plan(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D,
                        const int64_t q_strides[3], const int64_t k_strides[3],
                        float scale, int flags, int window_left, int window_right, int q_offset,
                        size_t workspace_bytes, fa2_fwd_plan_t* plan);

/* The plan of the packed forward (fa2_fwd_varlen above): kernel = FA2_KERNEL_HIP_VARLEN, contract 0, rows as launched, heads_main = B*H. */
enum { FA2_KERNEL_HIP_VARLEN = 6 };     /* (an enumerator, like FA2_KERNEL_HIP_WINDOW) */
int fa2_fwd_varlen_plan(int dtype, int B, int H, int Hkv, int max_seqlen_q, int max_seqlen_k, int D,
                        const int64_t q_strides[2], const int64_t k_strides[2],
                        float scale, int flags, int window_left, int window_right, fa2_fwd_plan_t* plan);

/* The plan of fa2_fwd_varlen_dv above: kernel = FA2_KERNEL_HIP_VARLEN_DV, contract 0, rows as launched, heads_main = B*H.  The strides may be NULL
 * (contiguous tensors); v takes k's, o takes q's.  Sizes, flags, window, dtype, the (D, Dv) pair and the scale are checked as by the call. */
enum { FA2_KERNEL_HIP_VARLEN_DV = 10 };     /* (an enumerator, like FA2_KERNEL_HIP_WINDOW) */
int fa2_fwd_varlen_dv_plan(int dtype, int B, int H, int Hkv, int max_seqlen_q, int max_seqlen_k, int D, int Dv,
                           const int64_t q_strides[2], const int64_t k_strides[2],
                           float scale, int flags, int window_left, int window_right, fa2_fwd_plan_t* plan);

/* ---- Chunked prefill against a KV cache: packed queries (as fa2_fwd_varlen's) against the cache fa2_kvcache_append writes and fa2_fwd_decode reads,
 * contiguous or paged, with every length and the block table read on the device — a prompt whose prefix already sits in cached pages, a prompt
 * processed in chunks, a continuous-batching step that mixes prefill chunks with decode rows.  Inference only: there is no backward.
 *   q, o            : [total_q, H, D] of `dtype`, element strides {head, row} as in fa2_fwd_varlen; lse f32 [H, total_q] (log2 units) with its head stride
 *   cu_seqlens_q    : int32 [B + 1], device memory: sequence s owns the query rows [cu[s], cu[s+1]) — Nq_s may be 0, 1 or thousands.  NOT validated
 *                     (fa2_fwd_varlen's contract: ascending, cu[0] >= 0, cu[B] <= the rows of q / o / lse, Nq_s <= max_seqlen_q).
 *   max_seqlen_q    : host int >= every Nq_s; it sizes the grid B * H * ceil(max_seqlen_q / rows).  A longer sequence's rows beyond it are not computed.
 *   cache_seqlens   : int32 [B], device memory: the valid keys of sequence s INCLUDING its Nq_s new tokens, whose K / V the caller has already written
 *                     (fa2_kvcache_append or otherwise).  Clamped into [0, capacity_keys] by the kernel.
 *   k_cache, v_cache: 16-bit caches of `dtype` in fa2_fwd_decode's two layouts: [B, capacity, Hkv, D] (page_size = 0, capacity = key slots per sequence)
 *                     or a pool [num_pages, page_size, Hkv, D] under an int32 block_table [B, capacity] (page_size a multiple of 64, capacity =
 *                     block-table entries per sequence).  Element strides {batch | page, head, row}.  cache_format must be FA2_CACHE_16BIT: e4m3 caches
 *                     are FA2_ERR_DTYPE here (fa2_fwd_prefill_fp8 below serves them).
 *   window_left     : -1 (none) or >= 0.  softcap, alibi_slopes (f32 [H] or [B, H], device memory), alibi_stride: fa2_fwd_decode_window's.
 * Masking is decode's: bottom-right causal per sequence — row i of sequence s sits at key position len_s - Nq_s + i and attends the keys j with
 * pos - window_left <= j <= pos.  Rows at a negative position (Nq_s > len_s) return zeros and lse = -inf.  The host reads neither cache_seqlens nor
 * block_table, and no maximum key length is asked for: the capacity bounds the sweep and the device length ends it, so a call is captured in a graph once
 * and replayed as lengths, tables and cache contents change in place.
 * Safety (decode's rules): a length is clamped into [0, capacity_keys], a page id into [0, num_pages); keys at or beyond the length contribute nothing
 * whatever the cache holds there (a tile's buffer descriptor ends at the sequence's last valid row: such rows read as zeros, and their scores are masked
 * by position); no content of cache_seqlens or block_table moves a read outside the two cache allocations — a wrong value gives a wrong answer; a page
 * that holds no key visible to any row of a workgroup (below a window, beyond the causal edge of the workgroup's last row) is never addressed and its
 * block-table entry never read.
 * Addressing: every 64-key tile is staged through a descriptor of its own whose base is formed in 64 bits (fa2_prefill_tile below has the arithmetic),
 * so a pool may exceed 4 GiB and fa2_fwd_varlen's "K / V span below 2 GiB" rule does not apply: only one tile, 64 * row stride * 2 bytes, must stay
 * below 2^31 (FA2_ERR_BAD_SHAPE).
 * Checks, in fa2_fwd_decode's class order: null pointers (the block table of a paged call included); sizes (FA2_ERR_BAD_SHAPE: a size < 1, H % Hkv, a
 * page_size that is negative or no multiple of 64, capacity_keys above 2^31 - 65, num_pages < 1 of a paged call, window_left < -1, a negative lse /
 * slope stride, position sums that leave 32 bits, the tile rule above); head dim (FA2_ERR_HEAD_DIM: D a multiple of 8 up to 512); alignment (16-byte
 * tensors, 4-byte lse / cu_seqlens_q / cache_seqlens / block_table / slopes, strides multiples of 8 with a positive row stride, a non-negative
 * block-table stride); dtype and cache_format (FA2_ERR_DTYPE); scale; softcap (FA2_ERR_SOFTCAP); FA2_ERR_GRID.
 * Kernels (FA2_KERNEL_HIP_PREFILL, contract 0): the packed kernels (FA2_KERNEL_HIP_VARLEN) with the key count from cache_seqlens and a per-tile
 * descriptor; everything after the staging is shared, so the results equal fa2_fwd_varlen's (FA2_FLAG_CAUSAL | FA2_FLAG_BOTTOM_RIGHT, the same
 * window; with softcap > 0 or slopes: fa2_fwd_varlen_scoremod's) on the sequence's keys gathered into a packed buffer BIT FOR BIT.  128- or 256-row
 * workgroups by the packed call's rule on (B, H, max_seqlen_q) and option "rows" at head dims up to 128, 128-row workgroups above.  No KV-split. */
enum { FA2_KERNEL_HIP_PREFILL = 8 };    /* (an enumerator, like FA2_KERNEL_HIP_WINDOW) */
int fa2_fwd_prefill(int dtype, int cache_format, const void* q, const void* k_cache, const void* v_cache, void* o, float* lse,
                    const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table,
                    int B, int H, int Hkv, int max_seqlen_q, int D, int capacity, int page_size, int num_pages,
                    const int64_t q_strides[2], const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[2],
                    int64_t lse_stride, int64_t block_table_stride, float scale, int window_left, float softcap,
                    const float* alibi_slopes, int64_t alibi_stride, void* hip_stream);
/* The plan of the call above: kernel = FA2_KERNEL_HIP_PREFILL, contract 0, rows as launched, heads_main = B * H.  Sizes and dtype are checked as above. */
int fa2_fwd_prefill_plan(int dtype, int B, int H, int Hkv, int max_seqlen_q, int D, int capacity, int page_size, fa2_fwd_plan_t* plan);

/* ---- ... on e4m3 caches with per (sequence, K / V head) descales: the cache fa2_kvcache_append_varlen writes with FA2_CACHE_E4M3 and fa2_fwd_decode_fp8
 * reads.  Everything is fa2_fwd_prefill's with K = float(k_cache) * k_descale[s, hkv] and V = float(v_cache) * v_descale[s, hkv]; what differs:
 *   k_cache, v_cache: OCP e4m3 bytes in the same two layouts; their element strides count bytes, as in fa2_fwd_decode_fp8.
 *   k_descale, v_descale: f32 [B, Hkv] in device memory with element strides descale_strides = {sequence, K / V head}; either may be null (= 1.0).  They are
 *                     read on the device, once per workgroup: a captured call is replayed as they change in place.  k_descale multiplies the score
 *                     factor, so soft-capping sees the descaled score and the LSE is that of the descaled scores; v_descale multiplies the normalised
 *                     f32 row before its one rounding.  A NaN descale poisons the rows of its own (sequence, K / V head) and nothing else.
 * Safety: fa2_fwd_prefill's rules.  A tile's descriptor ends at the sequence's last valid row, in bytes: rows at or beyond the length read zero bytes
 * (= +0.0) whatever the cache holds there, the e4m3 NaN codes 0x7f / 0xff included.
 * Addressing: fa2_fwd_prefill's, in bytes: one tile, 64 * row stride bytes, must stay below 2^31 (FA2_ERR_BAD_SHAPE).
 * Checks, in fa2_fwd_prefill's class order, with fa2_fwd_decode_fp8's additions where their kind is: null pointers (+ descale_strides when a descale is
 * given); sizes (+ a negative descale stride; the tile rule in bytes); head dim (FA2_ERR_HEAD_DIM: D a multiple of 16 up to 256 — the kernel of head dim
 * 512 would keep its e4m3 staging registers in scratch memory and is not compiled, so 256 < D <= 512 is refused here while fa2_fwd_prefill takes it);
 * alignment (16-byte caches whose strides are multiples of 16, 4-byte descales); dtype (f16 / bf16); scale; softcap; FA2_ERR_GRID.
 * Kernels (FA2_KERNEL_HIP_PREFILL, contract 0): fa2_fwd_prefill's with the register form of the K / V staging at every head dim — a 16-byte LDS granule
 * is fetched as its 8 e4m3 bytes and converted to `dtype` in registers, exactly, before the LDS write; everything after the LDS image is shared.  With
 * descales that are null or powers of two in [1/8, 8] (every finite e4m3 value times such a factor is a f16 and a bf16 value) the results equal
 * fa2_fwd_prefill's on the 16-bit cache (float(cache) * descale) BIT FOR BIT.  Rows per workgroup: fa2_fwd_prefill's rule.  No KV-split. */
int fa2_fwd_prefill_fp8(int dtype, const void* q, const void* k_cache, const void* v_cache, void* o, float* lse,
                        const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table,
                        int B, int H, int Hkv, int max_seqlen_q, int D, int capacity, int page_size, int num_pages,
                        const int64_t q_strides[2], const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[2],
                        int64_t lse_stride, int64_t block_table_stride, float scale,
                        const float* k_descale, const float* v_descale, const int64_t descale_strides[2],
                        int window_left, float softcap, const float* alibi_slopes, int64_t alibi_stride, void* hip_stream);
/* The plan of the call above: fa2_fwd_prefill_plan's answer on the same shape, with the head-dim rule of the e4m3 call. */
int fa2_fwd_prefill_fp8_plan(int dtype, int B, int H, int Hkv, int max_seqlen_q, int D, int capacity, int page_size, fa2_fwd_plan_t* plan);

/* Where 64-key tile `tile` of a sequence lies — the host side of the one function the kernel calls (csrc/fa2_prefill.h: prefill_tile).  len is clamped into
 * [0, capacity_keys] (capacity_keys = capacity * page_size, or capacity when page_size = 0: the contiguous layout, one page per sequence).
 * *page_slot: the block-table entry of the tile's page (contiguous: 0); *row_in_page: the tile's first row inside that page; *valid_rows: how many of
 * its 64 rows hold a key of the sequence (0 .. 64; 0: the tile lies at or beyond the length).  FA2_ERR_NULL_POINTER; FA2_ERR_BAD_SHAPE for capacity < 1,
 * a page_size that is negative or no multiple of 64, capacity_keys above 2^31 - 65, or a tile outside [0, ceil(capacity_keys / 64)). */
int fa2_prefill_tile(int64_t len, int capacity, int page_size, int tile, int* page_slot, int* row_in_page, int* valid_rows);

/* Coarse form of the above (kept for callers of version 0.8): 1 if launches of this head dim MAY fold the scale into Q (head dims exactly 64
 * and 128, 0 < scale*log2(e) <= 1, option "fold" >= 1: the fp16 launches the hand-scheduled bodies take), 0 if none does, -1: D not supported.
 * fa2_fwd_plan is the exact, per-call answer. */
int fa2_fwd_prescales_q(int D, float scale);

/*
 * Process-wide tuning switches.  They choose between kernels that satisfy the same contract (results agree to rounding,
 * not necessarily bit for bit) and exist for A/B measurements and for the test-suite; the defaults are the measured best.
 * Initial values come from the environment variable named below, read once when the library is loaded.
 *   "rows"  FA2_ROWS   0 (default: heuristic on the grid size) | 128 | 256 — Q rows per forward (and dQ-pass) workgroup
 *   "asm"       FA2_ASM        bit 0: hand-scheduled forward bodies (head dims 64 and 128), bit 1: hand-scheduled backward
 *                              bodies (head dim 128), bits 2 / 3: ... except its dQ pass / its dK-dV pass, bit 4: the head-dim-64
 *                              forward body for non-causal launches too (default: causal only), bit 6: the forward launches the hand-scheduled kernel
 *                              takes — whole items and KV-split parts alike — run the bodies built on v_mfma_f32_16x16x32 (round 5: +3 .. 5 % on a
 *                              power-limited chip, same contracts; bit 6 clear: the 32x32x16 bodies), bits 7 / 8: the same for the dQ / the dK-dV pass
 *                              of the head dim 128 backward (-7 .. 8 % of either pass on fp16), bit 9: the 16x16x32 forward bodies keep their row sums
 *                              on the matrix pipe (FA2_CONTRACT_LSUM_P16; -4 % of a launch).  Their fast loop never moves the reference; since
 *                              round 6 a tile in which a P leaves the 16-bit range (fp16: a score 16 octaves above its row's reference) is formed again
 *                              in place and the wave finishes its sweep on the max-first bodies — <= 1.09x the sum-check bodies (bit 9 clear) on
 *                              N(0, amp^2) logits for every amp, 0.97x on benign data (profiles/r20_growth_cliff.txt; round 5 redid the item: 1.3 ..
 *                              1.7x); bit 10: head dims 136 .. 256 (D = 256: K / V row pitches that are multiples of 512 bytes; below 176: non-causal) on the
 *                              hand-scheduled 128-row kernel — 1.25 .. 1.6x the compiler-scheduled kernels at D >= 176, from 512 keys (causal: 1024) on,
 *                              profiles/r21_d256_ab.txt.
 *                              Default 1987.
 *                              0 = compiler-scheduled HIP kernels everywhere
 *   "persist"   FA2_PERSIST    1 (default) | 0 — persistent workgroups of the hand-scheduled forward kernels
 *   "split"     FA2_SPLIT      1 (default) | 0 — fa2_fwd_ws / fa2_bwd_ws may split the last round of workgroups (0: they are fa2_fwd / fa2_bwd)
   "fold"      FA2_FOLD       1 (default) | 0 | 2 — which launches of the hand-scheduled forward bodies fold scale*log2(e) into Q
                              (FA2_CONTRACT_PRESCALE_Q above): 0 none — every launch scales the f32 product like the reference kernel
                              (kernel_fp16.cu:164); 1 fp16 launches; 2 bf16 launches too.  Never when scale*log2(e) > 1 (the prescaled Q could
                              leave the dtype's range), never for a call flagged FA2_FLAG_EXACT_SCALE.  This one changes the numerical contract,
                              within the bounds stated there (measured against float64 per input class: profiles/r16_fold_evidence.txt — bf16, option
                              value 2, leaves BASELINE.md's acceptance from logits of ~+-20 on, which is why it stays opt-in).
   "kfold"     FA2_KFOLD      0 (default) | 1 — the hand-scheduled dK / dV pass (head dim 128) recomputes P from K * scale*log2(e) rounded once
                              to the I/O dtype, for the dtypes "fold" covers (round 4's default; -1.8 % backward time, but gradients 2-4x
                              the f32-scale pass's error at logits of +-30: off since round 5)
 *   "short"     FA2_SHORT      1 (default) | 0 — non-causal calls without a bias whose KV sweep is at most two tiles (Nkv <= 128: cross-attention on a text
 *                              prompt) at head dims <= 128 run the single-pass kernel (csrc/fa2_fwd_short.hip.h: one memory round trip, exact row
 *                              max, f32 scale, f32 row sums — contract 0; fa2_fwd_plan: FA2_KERNEL_HIP_128, rows 128).  Option "rows" != 0 keeps the
 *                              streaming kernels as well.  SDXL cross-attention 11.1 -> 7.4 us (profiles/r22_short_probe.txt).  fa2_bwd* runs the dQ pass
 *                              of such calls on the kernel's twin (csrc/fa2_bwd_short.hip.h; head dim 128 exactly keeps the hand-scheduled pass)
 *   "bwd_parts" (no variable)  3 (default) | 1 | 2 — profiling only: fa2_bwd runs just its dQ pass (1) or just its dK / dV pass (2);
 *                              the outputs of the skipped pass are not written (the dK / dV pass needs delta_ws from an earlier full call)
 * These (plus FA2_FRONTEND=py and FA2_GFX950_LIB=<path> of the Python package) are all the switches there are.
 * fa2_set_option returns FA2_OK, or FA2_ERR_BAD_SHAPE for an unknown name / value; fa2_get_option the value (>= 0) or that code.
 * fa2_get_option("epoch") counts the fa2_set_option calls so far: a caller that caches fa2_fwd_plan / fa2_*_workspace_bytes answers keys them on it.
 * Changing an option while launches are being issued from other threads is safe (atomics) but the switch-over point is not ordered.
 */
int fa2_set_option(const char* name, int value);
int fa2_get_option(const char* name);

/* Text for a return code of this library (validation codes and hipError_t values). */
const char* fa2_error_string(int code);

/* "fa2_gfx950 <major>.<minor> (<kernel variant>)" */
const char* fa2_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FA2_GFX950_H */
