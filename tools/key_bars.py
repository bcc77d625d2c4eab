"""Per-element bars for dense attention on random inputs: float64 dense attention with the sums of absolute terms the contract rounds, and the bars of O,
dV, dQ and dK made of them.  Pure torch with a device argument; imports neither the library nor anything under tests/.  tools/fuzz_parity.py and
tools/fuzz_mask.py apply the O and dV bars; tests/key_probes.py re-exports everything (its class C) and states the derivation, tests/test_key_probes.py proves
the same-contract oracle inside every bar and float64 mutants outside, and measures KAPPA."""
import torch

LOG2E = 1.4426950408889634
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}            # unit roundoff (half an ulp at 1.0)
FP16_MIN_NORMAL = 2.0 ** -14
# The 16-bit roundings alone reach 2 u sum P|v| on a row that one key dominates: the compiled forward kernels move their reference only when a row's maximum
# grew by more than 8 log2 units (FA2_DEFER_THR), the hand-scheduled ones keep a deferred reference too, so the dominant P is some 2^x, x in [0, 8], rounded with
# up to u relative while l adds the unrounded one (u |v|), and the output rounding adds up to u |O| (u, not u / 2: half an ulp at the bottom of a binade).
# The sweeps show it: the worst element of a run sits at 0.90 .. 0.99 of the bar, in 34 of the 55 cases above 0.8 a row whose largest P is above 0.9
# (profiles/fuzz_runs.md).  What f32 adds on top — exp2's ulp, the scale product, l's sum, the normalisation: four roundings — is F32_SLACK.
F32_SLACK = 4 * 2.0 ** -24
QUANTUM = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}          # half the subnormal spacing: what rounding costs BELOW the smallest normal, absolute
# measured by tests/test_key_probes.py measure_kappa() on the CPU: the same-contract oracle backward, fed its own forward, against float64 on the class-C
# backward inputs of the GPU tests themselves (tests/test_key_probes_gpu.py BACKWARD_CASES: same seed, every head; each finishes in seconds, none was cut
# down).  Largest |g_oracle - g_float64| / bar(kappa = 1), dQ and dK together: fp16 2.039 (dQ of (1, 8, 640, 640, 128) causal: a row of twelve keys whose
# delta cancels), bf16 1.948 (dQ of (1, 2, 4096, 4096, 128) causal); a second draw of the same shapes gave 1.58 / 2.02.  The table is in
# tests/test_key_probes.py's docstring.  KAPPA is twice the largest seen.
KAPPA_MEASURED = {torch.float16: 2.04, torch.bfloat16: 2.02}
KAPPA = {dt: 2.0 * x for dt, x in KAPPA_MEASURED.items()}


def ratio_max(err, bar):
    """max err / bar (0 / 0 counts as 0, a nonzero error on a zero bar as inf)."""
    inf = torch.full_like(err, float("inf"))
    return float(torch.where(bar > 0, err / bar, torch.where(err > 0, inf, torch.zeros_like(err))).max())


def dense64(q, k, v, scale, causal=False, keep=None, do=None, chunk_elems=1 << 25, bias=None, dv_only=False, softcap=0.0, kept=None, rs=1.0, dlse=None):
    """float64 dense attention of [B,H,Nq,D] q and [B,H,Nkv,D] k / v on their device, a few heads at a time, with the sums of absolute terms the class-C bars
    are made of.  causal: top-left; keep: None or a bool mask broadcastable to [B,H,Nq,Nkv]; bias: None or an additive mask, broadcastable likewise; rows
    that see no key give O = 0, lse = -inf.  dv_only: of the gradients, dV and its sums alone (tools/fuzz_parity.py, tools/fuzz_mask.py).
    softcap > 0: s = cap tanh(s / cap) before the masks and the bias (the library's order: cap, slopes, bias), dS times 1 - tanh^2.  kept / rs: a dropout
    keep mask (bool, broadcastable) and 1 / (1 - p_eff): O, dV and dP use P kept rs, the LSE does not.  dlse: the gradient of the natural-log LSE
    [B,H,Nq]: dS += P dlse.
    -> dict: o, lse (log2), o_abs = sum_j P|v|; with do also dq, dk, dv, dv_abs = sum_i P|dO|, a_dq, a_dk (see the module docstring), and a_dq_delta,
    a_dk_delta: the same sums with E_i = sum_c |dO_ic O_ic| in place of |dP| + |delta| (class D's delta-through-rounded-O term)."""
    B, H, Nq, D = q.shape
    Nkv = k.shape[2]
    dev = q.device
    out = dict(o=torch.empty((B, H, Nq, D), dtype=torch.float64, device=dev), lse=torch.empty((B, H, Nq), dtype=torch.float64, device=dev))
    out["o_abs"], out["o_sub"] = torch.empty_like(out["o"]), torch.empty_like(out["o"])
    if do is not None:
        names = (("dq", q), ("a_dq", q), ("a_dq_sub", q), ("a_dq_f32", q), ("a_dq_delta", q), ("dk", k), ("a_dk", k), ("a_dk_sub", k), ("a_dk_f32", k), ("a_dk_delta", k), ("dv", v), ("dv_abs", v), ("dv_sub", v))
        for n, like in names[-3:] if dv_only else names:
            out[n] = torch.empty(like.shape, dtype=torch.float64, device=dev)
    vis = None
    if causal:
        vis = ~torch.ones(Nq, Nkv, dtype=torch.bool, device=dev).triu(1)
    if keep is not None:
        keep = keep.to(dev).expand(B, H, Nq, Nkv)
    if bias is not None:
        bias = bias.to(dev).expand(B, H, Nq, Nkv)
    if kept is not None:
        kept = kept.to(dev).expand(B, H, Nq, Nkv)
    step = max(1, chunk_elems // (Nq * Nkv))
    for b in range(B):
        for h0 in range(0, H, step):
            sl = (b, slice(h0, min(H, h0 + step)))
            qd, kd, vd = q[sl].double(), k[sl].double(), v[sl].double()
            s = torch.matmul(qd, kd.transpose(-1, -2)) * scale
            fac = None
            if softcap > 0:
                t = torch.tanh(s / softcap)
                s, fac = softcap * t, 1.0 - t * t
                del t
            if vis is not None:
                s = s.masked_fill(~vis, float("-inf"))
            if keep is not None:
                s = s.masked_fill(~keep[sl], float("-inf"))
            if bias is not None:
                s = s + bias[sl].double()
            m = s.max(-1, keepdim=True).values
            dead = torch.isinf(m)
            e = torch.exp(s - torch.where(dead, torch.zeros_like(m), m))
            l = e.sum(-1, keepdim=True)
            p = e / torch.where(dead, torch.ones_like(l), l)
            pd = p if kept is None else p * kept[sl].double() * rs           # what multiplies V and dO
            out["o"][sl] = torch.matmul(pd, vd)
            out["o_abs"][sl] = torch.matmul(pd, vd.abs())
            out["o_sub"][sl] = torch.matmul(((e > 0) & (e < FP16_MIN_NORMAL)).double() / torch.where(dead, torch.ones_like(l), l), vd.abs())
            out["lse"][sl] = torch.where(dead, m, (m + torch.log(torch.where(dead, torch.ones_like(l), l))) * LOG2E).squeeze(-1)
            if do is None:
                continue
            gd = do[sl].double()
            pt = pd.transpose(-1, -2)
            out["dv"][sl] = torch.matmul(pt, gd)
            out["dv_abs"][sl] = torch.matmul(pt, gd.abs())
            out["dv_sub"][sl] = torch.matmul(((pt > 0) & (pt < FP16_MIN_NORMAL)).double(), gd.abs())
            if dv_only:
                continue
            dp = torch.matmul(gd, vd.transpose(-1, -2))
            if kept is not None:
                dp = dp * kept[sl].double() * rs
            delta = (gd * out["o"][sl]).sum(-1, keepdim=True)
            e_row = (gd * out["o"][sl]).abs().sum(-1, keepdim=True)
            if dlse is not None:
                delta = delta - dlse[sl].double().unsqueeze(-1)
            if fac is not None:
                p = p * fac                                                 # (P enters the gradients and their sums below only through dS)
            ds = p * (dp - delta) * scale
            out["dq"][sl] = torch.matmul(ds, kd)
            out["dk"][sl] = torch.matmul(ds.transpose(-1, -2), qd)
            w = p * (dp.abs() + delta.abs()) * abs(scale)
            sub = ((p > 0) & ((ds / scale).abs() < FP16_MIN_NORMAL)).double() * abs(scale)
            del ds, dp
            w32 = p * (torch.matmul(gd.abs(), vd.abs().transpose(-1, -2)) + (gd * out["o"][sl]).abs().sum(-1, keepdim=True)) * (abs(scale) * D * 2.0 ** -24)
            out["a_dq_f32"][sl] = torch.matmul(w32, kd.abs())
            out["a_dk_f32"][sl] = torch.matmul(w32.transpose(-1, -2), qd.abs())
            del w32
            wd = p * e_row * abs(scale)
            out["a_dq_delta"][sl] = torch.matmul(wd, kd.abs())
            out["a_dk_delta"][sl] = torch.matmul(wd.transpose(-1, -2), qd.abs())
            del wd
            out["a_dq"][sl] = torch.matmul(w, kd.abs())
            out["a_dk"][sl] = torch.matmul(w.transpose(-1, -2), qd.abs())
            out["a_dq_sub"][sl] = torch.matmul(sub, kd.abs())
            out["a_dk_sub"][sl] = torch.matmul(sub.transpose(-1, -2), qd.abs())
    return out


def o_bar(ref, dtype):
    return 2.0 * ((U[dtype] + F32_SLACK) * ref["o_abs"] + QUANTUM[dtype] * ref["o_sub"]) + QUANTUM[dtype]


def dv_bar(ref, dtype):
    return 2.0 * ((U[dtype] + F32_SLACK) * ref["dv_abs"] + QUANTUM[dtype] * ref["dv_sub"]) + QUANTUM[dtype]


def dq_bar(ref, dtype, kappa=None):
    return (KAPPA[dtype] if kappa is None else kappa) * (U[dtype] * ref["a_dq"] + QUANTUM[dtype] * ref["a_dq_sub"] + ref["a_dq_f32"]) + QUANTUM[dtype]


def dk_bar(ref, dtype, kappa=None):
    return (KAPPA[dtype] if kappa is None else kappa) * (U[dtype] * ref["a_dk"] + QUANTUM[dtype] * ref["a_dk_sub"] + ref["a_dk_f32"]) + QUANTUM[dtype]


# ---------------------------------------------------------------------------------------------------------------- class D (two-key pointer inputs)
# Rows that put half their weight on each of two keys (tests/key_probes.py, class D).  The class-C sums, plus one term that P ~ 1 / Nkv washes out and
# P = 1/2 does not, and a floor:
#   delta through the rounded O.  The backward forms delta_i = sum_c dO_ic O_ic from the O the forward STORED, 16-bit: O is off by up to u |O_ic| per
#       element, delta_i by up to u E_i, E_i = sum_c |dO_ic O_ic|, dS_ij by |scale| P_ij u E_i.  On random inputs the signs of a row's 1 / P keys cancel;
#       here one key carries half of it.  a_dq_delta / a_dk_delta are the class-C sums with E_i in place of |dP| + |delta|; they enter with weight u like
#       the rest.
#   (No term for a P that is rounded to fp16 BEFORE it meets dP - delta.  The contract is the one tools/fuzz_lse.py emulate() runs: the f32 P times
#       dP - delta, dS rounded once; a_*_sub counts q = 2^-25 per subnormal dS for that.  A pass that rounds P first loses q (|dP| + |delta|) per
#       pair whose P is below 2^-14 and the whole pair below 2^-25; a key whose dK element rests on one such pair then misses its bar, and should.
#       The fp16 soft-capped band of the GPU tests has such a key: P = 1.1e-8, true dK 2.2e-7.  The wave-pair dK / dV pass returned 0 for it, and now
#       sends 2^14 P through its slot: tests/test_key_probes_gpu.py test_pair_pass_keeps_a_pair_whose_p_is_below_fp16.)
#   an absolute floor for bf16.  QUANTUM[bf16] = 0 leaves bars of 1e-43 on gradients whose true value is the leak's (1e-41): f32 flushes what is below
#       2^-126, so a dS of that size is lost whole, and up to Nkv <= 2^13 of them times |k| <= 1 (dQ), or Nq <= 2^13 times |q| <= 2^7 (dK), add up
#       to 2^-106.  FLOOR_D[bf16] = 2^-100 (8e-31): sixty-four times that sum, thirty orders below any value a probe rests on.
# KAPPA_D is measured as KAPPA is: the same-contract oracle backward, fed its own forward, against float64 on the class-D inputs of the GPU tests' dense
# cases (tests/test_key_probes_gpu.py BACKWARD_CASES with "B", both map kinds, seed as there), both dtypes, every head; largest
# |g_oracle - g_float64| / bar(kappa = 1) over dQ and dK, doubled.  `python tests/test_key_probes.py kappa_d` prints the table that
# tests/test_key_probes.py's docstring keeps: fp16 0.813 (dK of (1, 2, 129, 127, 128) causal, inner targets), bf16 0.937 (dK of (1, 24, 3072, 3072, 64)).
# With the delta term in the sum the factor is below 1: on these rows the term is as large as A itself, and the oracle attains most of the sum.
FLOOR_D = {torch.float16: QUANTUM[torch.float16], torch.bfloat16: 2.0 ** -100}
KAPPA_D_MEASURED = {torch.float16: 0.82, torch.bfloat16: 0.94}
KAPPA_D = {dt: 2.0 * x for dt, x in KAPPA_D_MEASURED.items()}


def o_bar_d(ref, dtype):
    return o_bar(ref, dtype) + FLOOR_D[dtype]


def dv_bar_d(ref, dtype):
    return dv_bar(ref, dtype) + FLOOR_D[dtype]


def dq_bar_d(ref, dtype, kappa=None):
    return (KAPPA_D[dtype] if kappa is None else kappa) * (U[dtype] * (ref["a_dq"] + ref["a_dq_delta"]) + QUANTUM[dtype] * ref["a_dq_sub"] + ref["a_dq_f32"]) + FLOOR_D[dtype]


def dk_bar_d(ref, dtype, kappa=None):
    return (KAPPA_D[dtype] if kappa is None else kappa) * (U[dtype] * (ref["a_dk"] + ref["a_dk_delta"]) + QUANTUM[dtype] * ref["a_dk_sub"] + ref["a_dk_f32"]) + FLOOR_D[dtype]
