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


def dense64(q, k, v, scale, causal=False, keep=None, do=None, chunk_elems=1 << 25, bias=None, dv_only=False):
    """float64 dense attention of [B,H,Nq,D] q and [B,H,Nkv,D] k / v on their device, a few heads at a time, with the sums of absolute terms the class-C bars
    are made of.  causal: top-left; keep: None or a bool mask broadcastable to [B,H,Nq,Nkv]; bias: None or an additive mask, broadcastable likewise; rows
    that see no key give O = 0, lse = -inf.  dv_only: of the gradients, dV and its sums alone (tools/fuzz_parity.py, tools/fuzz_mask.py).
    -> dict: o, lse (log2), o_abs = sum_j P|v|; with do also dq, dk, dv, dv_abs = sum_i P|dO|, a_dq, a_dk (see the module docstring)."""
    B, H, Nq, D = q.shape
    Nkv = k.shape[2]
    dev = q.device
    out = dict(o=torch.empty((B, H, Nq, D), dtype=torch.float64, device=dev), lse=torch.empty((B, H, Nq), dtype=torch.float64, device=dev))
    out["o_abs"], out["o_sub"] = torch.empty_like(out["o"]), torch.empty_like(out["o"])
    if do is not None:
        names = (("dq", q), ("a_dq", q), ("a_dq_sub", q), ("a_dq_f32", q), ("dk", k), ("a_dk", k), ("a_dk_sub", k), ("a_dk_f32", k), ("dv", v), ("dv_abs", v), ("dv_sub", v))
        for n, like in names[-3:] if dv_only else names:
            out[n] = torch.empty(like.shape, dtype=torch.float64, device=dev)
    vis = None
    if causal:
        vis = ~torch.ones(Nq, Nkv, dtype=torch.bool, device=dev).triu(1)
    if keep is not None:
        keep = keep.to(dev).expand(B, H, Nq, Nkv)
    if bias is not None:
        bias = bias.to(dev).expand(B, H, Nq, Nkv)
    step = max(1, chunk_elems // (Nq * Nkv))
    for b in range(B):
        for h0 in range(0, H, step):
            sl = (b, slice(h0, min(H, h0 + step)))
            qd, kd, vd = q[sl].double(), k[sl].double(), v[sl].double()
            s = torch.matmul(qd, kd.transpose(-1, -2)) * scale
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
            out["o"][sl] = torch.matmul(p, vd)
            out["o_abs"][sl] = torch.matmul(p, vd.abs())
            out["o_sub"][sl] = torch.matmul(((e > 0) & (e < FP16_MIN_NORMAL)).double() / torch.where(dead, torch.ones_like(l), l), vd.abs())
            out["lse"][sl] = torch.where(dead, m, (m + torch.log(torch.where(dead, torch.ones_like(l), l))) * LOG2E).squeeze(-1)
            if do is None:
                continue
            gd = do[sl].double()
            pt = p.transpose(-1, -2)
            out["dv"][sl] = torch.matmul(pt, gd)
            out["dv_abs"][sl] = torch.matmul(pt, gd.abs())
            out["dv_sub"][sl] = torch.matmul(((pt > 0) & (pt < FP16_MIN_NORMAL)).double(), gd.abs())
            if dv_only:
                continue
            dp = torch.matmul(gd, vd.transpose(-1, -2))
            delta = (gd * out["o"][sl]).sum(-1, keepdim=True)
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
