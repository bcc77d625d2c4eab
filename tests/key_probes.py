"""Inputs whose expected attention output resolves ONE key, however long the sweep: builders, expectations and per-element bars.

The suite's bars are one number per tensor (conftest FLOOR / ATOL / GRAD_TOL, tools/fuzz_parity.py's 2 * FLOOR * max|v|).  On a sweep of 4096 keys one
(row, key) pair moves O by P * |v| ~ 1 / 1500 — under those bars — and a whole dropped 64 x 64 tile passes the bf16 one.  The three input classes here
keep their power at any Nkv.  CPU-only code with a `device` argument; imports neither the library nor the oracle (class C's code is tools/key_bars.py's,
re-exported here; tests/test_key_probes.py proves the conditions, the oracle inside every bar and ten float64 mutants outside; tests/test_key_probes_gpu.py runs the kernels; tools/fuzz_parity.py and
tools/fuzz_mask.py apply the class-C O and dV bars).

A. Counting inputs.  K = 0: every scaled score is exactly 0 under every scaling contract (a Q with the scale folded in, too).  Q is N(0,1), V is
   integer-valued in -3 .. 3: exact in fp16 and bf16, every f32 partial sum exact (|sum| <= 3 * Nkv < 2^24).  Row i that may see cnt_i keys has
       lse_i = log2(cnt_i)   (the library's log2 units; -inf and O = 0 where cnt_i = 0)        bar LSE_COUNT_BAR = 2^-20 absolute:
   log2(cnt) - log2(cnt - 1) >= log2(e) / cnt >= 8.8e-5 up to cnt = 16384, so the count of every row is resolved exactly;
       O_i = (sum of the visible v_j) / cnt_i, rounded once                                      bar 1 ulp of the I/O dtype at the expected value:
   numerator and l are exact in f32, only divide-then-round (or multiply by a reciprocal) may differ.  A call that the plan splits along the keys (nsplit > 1)
   merges per-part results normalised in f32: for it alone, + 2^-22 * sum|v| / cnt (~ 5e-7), which matters only where the expected value is (nearly) 0.  With dropout the kept keys come from the
   library's keep mask: O_i = sum_kept v_j / (cnt_i * (1 - p_eff)), bar 2 ulps (the factor 1 / (1 - p_eff) is one more rounded f32 number, applied to P
   before its 16-bit rounding or to O after), the LSE unchanged.

B. Pointer inputs.  K rows are random +-1 vectors, Q_i = c * K_pi(i) with c a power of two and pi a given row -> key map, V is N(0,1).  The target's
   score is scale * c * D, every other key's scale * c * (an integer of N(0, D) size): row i puts all but `leak_i` = 1 - P_target of its weight on
   key pi(i).  The builder measures leak_i from the exact integer Gram matrix in float64 and REFUSES (ValueError) inputs with a leak above
   POINTER_LEAK = 2^-16; pointer_inputs() starts at c = 4 and doubles c while the condition fails (D = 128: c = 4, leak ~ 1e-10; D = 64 needs c = 8:
   a pair of keys 5.6 sigma alike is 4 * 5.6 = 22 below a target of only 32 at c = 4).
       O_i = v_pi(i)        bar: 1 ulp of the I/O dtype at v + 3 * leak_i * max|v|.  The second term is the builder's own measured leak: what the
                            other keys really add and the target loses (2 leak max|v|), and the 16-bit rounding of those tiny P (an fp16 subnormal P
                            moves by up to itself: once more).  ~ 1e-9: it matters only for elements of v so small that their ulp is smaller.
       lse_i = log2(e) * scale * c * D     bar: pointer_lse_bar = tools/fuzz_parity.py's lse_limit (the f32 logit bound, plus one 16-bit rounding of
                            the dominant P where the row sums add the rounded P).  A launch that folds scale * log2(e) into Q sees the folded c.
       dV_j = sum of dO_i over the rows with pi(i) = j        bar: 1 ulp per summand (sum of ulp(dO_i), at least ulp of the sum) + 2 colleak_j max|dO|
                            (colleak_j: the weight key j gets from the rows that do not point at it, and once more for its 16-bit rounding).
       dQ, dK: the true gradients are ~ 0 (P (dP - delta) cancels on the target, P ~ 0 elsewhere); they are held to float64 dense attention with the
                            class-C bars below.  (GRAD_TOL * max|g_true| is no sound bar here: the cancellation dP_t - delta_i happens in f32 between
                            two dot products of ~ 10, and an O that is one ulp off — allowed above — moves delta_i by u * sum|dO v|; both are inside
                            kappa * u * A, which is ~ 1e-3 * max|dO v| here, and a delta of the wrong row is outside it by three orders.)

C. Random inputs (N(0,1)) against float64 dense attention on the device, with per-element bars made of the terms the contract rounds:
       O:   2 u * sum_j P_ij |v_jc|.      u = 2^-11 fp16, 2^-8 bf16 (half an ulp at 1.0: the largest relative error of one rounding, u / 2 on average).
            The numerator adds rounded P while l adds the unrounded ones (absent where the row sum adds the rounded P): up to u per term; the output
            rounding: up to u |O| <= u sum P|v|.  A row that one key dominates attains both (the kernels' reference is deferred, so that P is not exactly
            1: tools/key_bars.py F32_SLACK has the evidence), and f32 adds four roundings of 2^-24 on top: (2 u + 2^-21) sum P|v|.
       dV:  (2 u + 2^-21) * sum_i P_ij |dO_ic|, by the same derivation.
       dQ:  KAPPA u A_dQ,   A_dQ[i,c] = |scale| sum_j P_ij (|dP_ij| + |delta_i|) |k_jc|
       dK:  KAPPA u A_dK,   A_dK[j,c] = |scale| sum_i P_ij (|dP_ij| + |delta_i|) |q_ic|
   fp16 only: below its smallest normal 2^-14 a rounding costs q = 2^-25 absolute, not u relative.  A backward P = exp2(s - lse) of a 4096-key row is
   ~ 2^-12 and every twelfth is subnormal, so is a dV_j or dK_j that only a few late rows of a causal call reach (the oracle's fp16 dK was 2048 = 1 / u
   "bars" off float64 there: flushed).  Each bar therefore carries, for fp16, q * (the same sum over the terms that are subnormal, weight 1 in place of
   u P) + q for the output itself: o_bar / dv_bar / dq_bar / dk_bar below.  bf16 has f32's exponent range and no such term.
   Both dtypes: dP_ij and delta_i are f32 dot products of D terms; where they cancel (a row of pointer inputs whose dO . v_target is 7e-7 by chance: seen)
   u (|dP| + |delta|) vanishes and their own rounding, <= D 2^-24 (sum_c |dO_ic v_jc| + sum_c |dO_ic O_ic|), is what is left: A_f32 carries it with weight
   D 2^-24 in place of u (1.5 % of u at fp16, D = 128).
   KAPPA is measured, not derived: the largest |g_oracle - g_float64| / (u A) of the same-contract oracle backward over the class-C shapes of the GPU
   tests, both dtypes (tests/test_key_probes.py: measure_kappa(), `python tests/test_key_probes.py kappa`), doubled.
"""
import importlib.util
import math
import os

import torch

# class C (float64 dense attention with the sums of absolute terms, the four bars, KAPPA) lives in tools/key_bars.py, beside the two sweeps that apply the
# O and dV bars, and is re-exported here — the way tests/lse_refs.py and tools/fuzz_lse.py share their references: the tools never import from tests/
_spec = importlib.util.spec_from_file_location("_key_bars", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "tools", "key_bars.py"))
kb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kb)
LOG2E, U, FP16_MIN_NORMAL, QUANTUM, KAPPA_MEASURED, KAPPA = kb.LOG2E, kb.U, kb.FP16_MIN_NORMAL, kb.QUANTUM, kb.KAPPA_MEASURED, kb.KAPPA
dense64, o_bar, dv_bar, dq_bar, dk_bar, ratio_max = kb.dense64, kb.o_bar, kb.dv_bar, kb.dq_bar, kb.dk_bar, kb.ratio_max

_MANT = {torch.float16: 10, torch.bfloat16: 7}
_EMIN = {torch.float16: -14, torch.bfloat16: -126}
GRAD_TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}              # tests/conftest.py's (tests/test_key_probes.py asserts they agree)
LSE_COUNT_BAR = 2.0 ** -20
COUNT_F32 = 4 * 2.0 ** -24                                           # four f32 roundings (the merge of a split call): _counting_finish
POINTER_LEAK = 2.0 ** -16
SHIFTS = (0, 1, 63, 64, 65)                                          # ... and Nkv // 2 + 17: shifts_of(Nkv)


def ulp(x, dtype):
    """The spacing of `dtype` at |x| (float64 tensor; the subnormal spacing below the smallest normal)."""
    _, e = torch.frexp(x.detach().abs().double())                     # |x| = m 2^e, m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(e, _EMIN[dtype]), e - 1).clamp(min=_EMIN[dtype])
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - _MANT[dtype])


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(int(seed))


# ---------------------------------------------------------------------------------------------------------------- visible keys
def row_ranges(Nq, Nkv, causal=False, bottom_right=False, window=(-1, -1), q_offset=0, device=None):
    """Closed form: the half-open key interval [lo_i, hi_i) row i may see (int64 [Nq] each).  Row i sits at key position i + q_offset (bottom_right:
    + Nkv - Nq); window = (left, right), -1 unbounded; causal means right = 0 (plain causal: top-left, j <= i)."""
    left, right = window
    if causal:
        right = 0
    pos = torch.arange(Nq, dtype=torch.int64, device=device) + q_offset + ((Nkv - Nq) if bottom_right else 0)
    lo = torch.zeros_like(pos) if left < 0 else (pos - left).clamp(0, Nkv)
    hi = torch.full_like(pos, Nkv) if right < 0 else (pos + right + 1).clamp(0, Nkv)
    return lo, torch.maximum(hi, lo)


def brute_mask(Nq, Nkv, causal=False, bottom_right=False, window=(-1, -1), q_offset=0, device=None):
    """The same band from its definition, pair by pair: bool [Nq, Nkv] (the check of row_ranges)."""
    left, right = window
    keep = torch.zeros(Nq, Nkv, dtype=torch.bool)
    for i in range(Nq):
        p = i + q_offset + ((Nkv - Nq) if bottom_right else 0)
        for j in range(Nkv):
            ok = (left < 0 or j >= p - left) and ((j <= p) if causal else (right < 0 or j <= p + right))
            keep[i, j] = ok
    return keep.to(device) if device is not None else keep


# ---------------------------------------------------------------------------------------------------------------- A: counting inputs
def counting_inputs(B, H, Hkv, Nq, Nkv, D, dtype, seed, device=None):
    """q N(0,1) [B,H,Nq,D], k = 0 and integer v in -3 .. 3 [B,Hkv,Nkv,D]."""
    assert 3 * Nkv < 2 ** 24, "the f32 partial sums must stay exact"
    g = _gen(seed)
    q = torch.randn((B, H, Nq, D), generator=g).to(dtype)
    k = torch.zeros((B, Hkv, Nkv, D), dtype=dtype)
    v = torch.randint(-3, 4, (B, Hkv, Nkv, D), generator=g).to(dtype)
    return tuple(t.to(device) if device is not None else t for t in (q, k, v))


def _expand(t, H):
    """[B, Hkv, ...] -> [B, H, ...] (query head h reads k / v head h // (H / Hkv))."""
    return t if t.shape[1] == H else t.repeat_interleave(H // t.shape[1], dim=1)


def counting_expect(v, lo, hi, H, dtype, split=False):
    """Expected O (float64 of the value rounded once to dtype) [B,H,Nq,D], lse (log2) [B,H,Nq] and the O bar for rows seeing the keys [lo_i, hi_i):
    prefix sums of v, exact.  split: the call is split along the keys (_counting_finish)."""
    vd = _expand(v, H).double()
    zero = vd.new_zeros((vd.shape[0], vd.shape[1], 1, vd.shape[3]))
    cs, cs_abs = (torch.cat([zero, t.cumsum(dim=2)], dim=2) for t in (vd, vd.abs()))
    assert float(cs_abs.max()) < 2 ** 24
    cnt = (hi - lo).double()
    tot, tot_abs = cs[:, :, hi] - cs[:, :, lo], cs_abs[:, :, hi] - cs_abs[:, :, lo]
    return _counting_finish(tot, tot_abs, cnt.view(1, 1, -1).expand(tot.shape[:3]), dtype, split=split)


def counting_expect_mask(v, keep, H, dtype, kept=None, p_eff=0.0):
    """... for rows seeing the keys keep[..., i, :] (bool, broadcastable to [B,H,Nq,Nkv]).  Dropout: `kept` (bool [B,H,Nq,Nkv], the library's keep mask)
    selects the summands, the count stays keep's, the result is divided by 1 - p_eff; the bar is then 2 ulps."""
    vd = _expand(v, H).double()
    B, _, Nkv, _ = vd.shape
    keep = keep.expand(B, H, keep.shape[-2], Nkv)
    w = keep if kept is None else (keep & kept)
    tot, tot_abs = torch.matmul(w.double(), vd), torch.matmul(w.double(), vd.abs())
    assert float(tot_abs.max()) < 2 ** 24
    if kept is not None:
        tot, tot_abs = tot / (1.0 - p_eff), tot_abs / (1.0 - p_eff)
    return _counting_finish(tot, tot_abs, keep.sum(-1).double(), dtype, ulps=1.0 if kept is None else 2.0)


def _counting_finish(tot, tot_abs, cnt, dtype, ulps=1.0, split=False):
    """split (the plan's nsplit > 1): + COUNT_F32 * sum|v| / cnt: a call that is split along the keys merges per-part results that were normalised in f32 (s_p / l_p, the weights
    l_p / l, their products and the sum: four f32 roundings of terms of that size), so an expected 0 comes out as ~ 1e-8, not 0."""
    dead = cnt == 0
    c1 = cnt.clamp(min=1)[..., None]
    o = torch.where(dead[..., None], torch.zeros_like(tot), tot / c1).to(dtype).double()
    lse = torch.where(dead, torch.full_like(cnt, float("-inf")), torch.log2(cnt.clamp(min=1)))
    return o, lse, ulps * ulp(o, dtype) + (COUNT_F32 * tot_abs / c1 if split else 0.0)


def check_counting(o, lse, o_exp, lse_exp, o_bar):
    """-> list of failures (empty: inside the bars).  o, lse: what the code under test returned."""
    fails = []
    o, lse = o.double(), lse.double()
    if not torch.isfinite(o).all():
        return ["O non-finite"]
    dead = torch.isinf(lse_exp)
    if not torch.equal(torch.isinf(lse) & (lse < 0), dead):
        fails.append("rows that see no key: -inf LSE in %d rows, expected in %d" % (int((torch.isinf(lse) & (lse < 0)).sum()), int(dead.sum())))
    lerr = torch.where(dead, torch.zeros_like(lse), (lse - torch.where(dead, torch.zeros_like(lse_exp), lse_exp)).abs())
    if not bool((lerr <= LSE_COUNT_BAR).all()):       # (NaN fails)
        i = int(torch.nan_to_num(lerr, nan=float("inf")).argmax())
        fails.append("LSE: %d rows off the count, worst %.3e at flat row %d (got %.6f, log2(count) = %.6f)" % (
            int((~(lerr <= LSE_COUNT_BAR)).sum()), float(lerr.flatten()[i]), i, float(lse.flatten()[i]), float(lse_exp.flatten()[i])))
    bad = ~((o - o_exp).abs() <= o_bar)
    if bool(bad.any()):
        r = ((o - o_exp).abs() / o_bar).max()
        fails.append("O: %d elements off, worst %.1f bars" % (int(bad.sum()), float(r)))
    return fails


# ---------------------------------------------------------------------------------------------------------------- B: pointer inputs
def shifts_of(Nkv):
    return SHIFTS + (Nkv // 2 + 17,)


def pointer_map(kind, Nq, Nkv, shift=0, seed=0):
    """Row -> key maps (int64 [Nq]).  'shift': (i + s) mod Nkv; 'causal': max(i - s, 0) (the last key for rows past Nkv); 'perm': one seeded random
    permutation of the keys (taken modulo for Nq > Nkv), 'perm_causal': min(perm(i), i).  'edges' / 'edges_causal': of every four rows one points into the
    sweep's FIRST tile, one into its LAST (causal: the diagonal), two `shift` away — every row block, whatever its size, targets both ends of its sweep."""
    i = torch.arange(Nq, dtype=torch.int64)
    if kind == "shift":
        return (i + shift) % Nkv
    if kind == "causal":
        return (i - shift).clamp(0, Nkv - 1)
    if kind == "perm":
        return torch.randperm(Nkv, generator=_gen(seed))[i % Nkv]
    if kind == "perm_causal":
        return torch.minimum(pointer_map("perm", Nq, Nkv, 0, seed), i.clamp(max=Nkv - 1))
    if kind in ("edges", "edges_causal"):
        first = i % min(64, Nkv)
        if kind == "edges":
            last, rest = Nkv - 1 - first, (i + shift) % Nkv
        else:
            first, last, rest = torch.minimum(first, i).clamp(max=Nkv - 1), i.clamp(max=Nkv - 1), (i - shift).clamp(0, Nkv - 1)
        return torch.where(i % 4 == 0, first, torch.where(i % 4 == 1, last, rest))
    raise ValueError(kind)


def pointer_leaks(k, pi, c, scale, visible=None):
    """From the exact integer Gram matrix, in float64: leak [B,Hkv,Nq] = 1 - P_target per row and colleak [B,Hkv,Nkv] = the weight key j gets from rows that
    do NOT point at it.  k [B,Hkv,Nkv,D] of +-1, pi int64 [Nq], visible: None or bool [Nq, Nkv]."""
    B, Hkv, Nkv, D = k.shape
    pi = pi.to(k.device)
    leak = torch.empty((B, Hkv, pi.numel()), dtype=torch.float64, device=k.device)
    colleak = torch.empty((B, Hkv, Nkv), dtype=torch.float64, device=k.device)
    rows = torch.arange(pi.numel(), device=k.device)
    for b in range(B):
        for h in range(Hkv):
            kf = k[b, h].float()
            gram = torch.matmul(kf[pi], kf.t())                          # integers of magnitude <= D: exact in f32
            s = gram.double() * (c * scale) - (c * scale * D)             # score minus the target's: 0 at j = pi(i)
            if visible is not None:
                s = s.masked_fill(~visible, float("-inf"))
                assert bool(visible[rows, pi].all()), "a row's target key is masked"
            e = torch.exp(s)
            e[rows, pi] = 0.0                                             # (keys equal to the target row by chance stay: they are leak)
            tot = e.sum(-1)
            leak[b, h] = tot / (1.0 + tot)
            colleak[b, h] = (e / (1.0 + tot)[:, None]).sum(0)
    return leak, colleak


def pointer_inputs(B, H, Hkv, Nq, Nkv, D, dtype, pi, seed, device=None, scale=None, c=None, visible=None):
    """-> dict(q, k, v, c, leak [B,H,Nq], colleak [B,H,Nkv], pi).  c=None: 4, doubled while some row's leak exceeds POINTER_LEAK; a given c that fails the
    condition raises ValueError.  Grouped k / v (Hkv < H): every query head of a group points the same way."""
    scale = D ** -0.5 if scale is None else scale
    g = _gen(seed)
    k = (torch.randint(0, 2, (B, Hkv, Nkv, D), generator=g) * 2 - 1).to(dtype)
    v = torch.randn((B, Hkv, Nkv, D), generator=g).to(dtype)
    if device is not None:
        k, v = k.to(device), v.to(device)
    vis = visible.to(k.device) if visible is not None else None
    cc = 4.0 if c is None else float(c)
    while True:
        assert math.log2(cc) == int(math.log2(cc)), "c must be a power of two"
        leak, colleak = pointer_leaks(k, pi, cc, scale, vis)
        if float(leak.max()) <= POINTER_LEAK:
            break
        if c is not None or cc >= 64:
            raise ValueError("pointer inputs: 1 - P_target = %.3e > 2^-16 at c = %g (D = %d, Nkv = %d)" % (float(leak.max()), cc, D, Nkv))
        cc *= 2
    q = (_expand(k, H)[:, :, pi.to(k.device)].float() * cc).to(dtype)
    return dict(q=q, k=k, v=v, c=cc, leak=_expand(leak, H), colleak=_expand(colleak, H), pi=pi.to(k.device), scale=scale)


def pointer_expect_o(inp, dtype):
    """Expected O [B,H,Nq,D] (float64) and its bar."""
    H = inp["q"].shape[1]
    v = _expand(inp["v"], H).double()
    o = v[:, :, inp["pi"]]
    return o, ulp(o, dtype) + 3.0 * inp["leak"][..., None] * float(v.abs().max())


def pointer_expect_lse(inp, dtype, folded=False):
    """Expected log2 LSE (a number: the same for every row).  folded: the launch rounds scale * log2(e) * q once to the I/O dtype and scores with 1."""
    D = inp["q"].shape[-1]
    if folded:
        return D * float(torch.tensor(inp["c"] * inp["scale"] * LOG2E, dtype=torch.float64).to(dtype))
    return LOG2E * inp["scale"] * inp["c"] * D


def pointer_lse_bar(inp, dtype, p16):
    """tools/fuzz_parity.py's lse_limit for these inputs (max|q| = c, max|k| = 1); p16: the launch's row sums add the rounded P (FA2_CONTRACT_LSUM_P16)."""
    D = inp["q"].shape[-1]
    return lse_logit_bar(inp["c"], 1.0, D, inp["scale"], dtype, p16)


def lse_logit_bar(qmax, kmax, D, scale, dtype, p16):
    smag = qmax * kmax * D * abs(scale) * LOG2E
    lim = max(1e-3, 4e-6 * smag)
    if (D == 64 or p16) and dtype == torch.bfloat16:
        lim = max(lim, 2.8e-3 + lim, 6e-3)
    elif p16:
        lim = max(lim, 3.6e-4 + lim)
    return lim


def pointer_expect_dv(inp, do, dtype):
    """Expected dV [B,Hkv,Nkv,D] (float64) for the upstream gradient do [B,H,Nq,D], and its bar."""
    B, H, Nq, D = do.shape
    Hkv, Nkv = inp["k"].shape[1], inp["k"].shape[2]
    dod = do.double()
    dv = torch.zeros((B, H, Nkv, D), dtype=torch.float64, device=do.device).index_add_(2, inp["pi"], dod)
    bar = torch.zeros_like(dv).index_add_(2, inp["pi"], ulp(dod, dtype))
    leak = inp["colleak"]
    if Hkv != H:                                                            # a k / v head collects its whole group
        dv, bar, leak = (t.view(B, Hkv, H // Hkv, *t.shape[2:]).sum(2) for t in (dv, bar, leak))
    return dv, torch.maximum(bar, ulp(dv, dtype)) + 2.0 * leak[..., None] * float(dod.abs().max())


def check_elements(name, got, want, bar):
    """-> list of failures for one tensor against a per-element bar."""
    got = got.double()
    if not torch.isfinite(got).all():
        return ["%s non-finite" % name]
    err = (got - want).abs()
    bad = ~(err <= bar)
    if bool(bad.any()):
        ratio = torch.where(bar > 0, err / bar, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        return ["%s: %d elements outside their bar, worst %.2f bars (abs err %.3e)" % (name, int(bad.sum()), float(ratio.max()), float(err[bad].max()))]
    return []


def worst_ratio(got, want, bar):
    return ratio_max((got.double() - want).abs(), bar)


# ---------------------------------------------------------------------------------------------------------------- C: random inputs
def random_inputs(B, H, Hkv, Nq, Nkv, D, dtype, seed, device=None, with_do=False):
    g = _gen(seed)
    shapes = [(B, H, Nq, D), (B, Hkv, Nkv, D), (B, Hkv, Nkv, D)] + ([(B, H, Nq, D)] if with_do else [])
    out = tuple(torch.randn(s, generator=g).to(dtype) for s in shapes)
    return tuple(t.to(device) for t in out) if device is not None else out


def fold_kv_heads(t, Hkv):
    """Per-query-head sums [B,H,Nkv,D] -> per k / v head [B,Hkv,Nkv,D]."""
    B, H = t.shape[:2]
    return t if H == Hkv else t.view(B, Hkv, H // Hkv, *t.shape[2:]).sum(2)


def check_random(ref, dtype, o=None, dq=None, dk=None, dv=None):
    """-> list of failures of whichever results are given against the class-C bars of `ref` = dense64(...)."""
    fails = []
    if o is not None:
        fails += check_elements("O", o, ref["o"], o_bar(ref, dtype))
    if dv is not None:
        fails += check_elements("dV", dv, ref["dv"], dv_bar(ref, dtype))
    if dq is not None:
        fails += check_elements("dQ", dq, ref["dq"], dq_bar(ref, dtype))
    if dk is not None:
        fails += check_elements("dK", dk, ref["dk"], dk_bar(ref, dtype))
    return fails
