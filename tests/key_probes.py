"""Inputs whose expected attention output resolves ONE key, however long the sweep: builders, expectations and per-element bars.

The suite's bars are one number per tensor (conftest FLOOR / ATOL / GRAD_TOL, tools/fuzz_parity.py's 2 * FLOOR * max|v|).  On a sweep of 4096 keys one
(row, key) pair moves O by P * |v| ~ 1 / 1500 — under those bars — and a whole dropped 64 x 64 tile passes the bf16 one.  The four input classes here
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

D. Two-key pointer inputs.  B's keys and values; Q_i = c (K_a(i) + K_b(i)): entries -2c, 0, 2c, exact in fp16 and bf16.  Both targets score
   scale c (D + K_a . K_b), the same integer times c: P_a = P_b = 1/2 up to the leak, O_i = (v_a + v_b) / 2, and the backward does NOT cancel on them:
       dS_a = -dS_b = scale g_i / 4,  g_i = dO_i . (v_a - v_b);   dQ_i = dS_a (k_a - k_b),   dK_a += dS_a q_i,   dV_a += dO_i / 2
   all O(1) at any sweep length.  dO = N(0,1) + sig (v_a - v_b) / 2 keeps g_i away from 0 (g_i ~ sig D).  two_pointer_maps puts a and b ON the edges of the
   row's visible interval [lo_i, hi_i) (kind "edge") or one key inside them (kind "inner"): a transposed band that is one key short or long at either
   end drops or adds exactly such a pair, and the two kinds together tell which side.  Under a keep mask or a dropout mask the targets are the row's
   first and last kept visible keys.  Rows with a = b (a band one key wide, a sequence of one key) probe O and dV only, rows that see no key get
   q = 0 and must come back with dQ = 0.
   The expected values are float64 dense attention under the call's own modifiers (dense64 with keep= / bias= / softcap= / kept= / dlse=), the bars
   class C's with two more terms (tools/key_bars.py: delta through the rounded O, an absolute floor for bf16) and a KAPPA_D measured as KAPPA is.
   The builder REFUSES (ValueError) inputs that are not a probe — conditions, checked in float64 from that reference:
       leak    1 - P_a - P_b <= POINTER_LEAK for every row, under the call's score modifiers (c starts at 4 and doubles, up to 256: D = 64 needs 32);
       power   for every (row, target) pair, leaving the pair out of the backward moves some element of dV by >= POWER_D = 4 of that element's bars,
               and for rows with two targets some element of dQ and some element of dK likewise (bars of the dtype in use; a key that many rows
               point at has a larger bar, which is why this is checked and not assumed).
   Three things the conditions forced.  A row that can see ONE key (a packed sequence of one key under 700 rows) has P = 1 whatever the scores are, and no
   element of that key's dV resolves one of 700 summands: such rows are exempt from the dV condition and reported apart (power["dv_lone"]); O holds them.
   Heads of a group that all point at one key put g summands under one dK / dV bar: where that leaves a pair under POWER_D (bf16, g >= 4) the caller
   asks for spread_group, one pointing head per row.  And a head in which some row's two targets tie with a third key gets new keys (_tied_heads).
   ALiBi (P_a != P_b: the nearer target wins by exp(slope * width)) and soft-capping (the capped target must still beat the capped rest) are given as
   bias= and softcap=; the caller chooses slopes with slope * width of order 1 and a cap above the target's score, and the two conditions decide.
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
FLOOR_D, KAPPA_D_MEASURED, KAPPA_D = kb.FLOOR_D, kb.KAPPA_D_MEASURED, kb.KAPPA_D
o_bar_d, dv_bar_d, dq_bar_d, dk_bar_d = kb.o_bar_d, kb.dv_bar_d, kb.dq_bar_d, kb.dk_bar_d

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


# ---------------------------------------------------------------------------------------------------------------- D: two-key pointer inputs
POWER_D = 4.0
C_MAX_D = 256.0
DRAWS_D = 8


def _uniform_in(lo, width, gen):
    """One seeded uniform draw per row from [lo, lo + width) (width >= 1)."""
    return lo + (torch.rand(lo.shape, generator=gen, dtype=torch.float64) * width.double()).long().clamp(max=width - 1)


def two_pointer_maps(lo, hi, Nkv, seed, kind="edge", keep=None):
    """-> (a, b): int64 target keys of every row, -1 for rows that see no key.  lo, hi: row_ranges' output.  a(i) = lo_i where the band bounds the row from
    the left (lo_i > 0), else a seeded uniform key of [lo_i, hi_i); b(i) = hi_i - 1 where hi_i < Nkv, else uniform, different from a where the row sees two
    keys.  kind "inner": lo_i + 1 and hi_i - 2 instead (kept inside the interval).  keep (bool [..., Nq, Nkv], already the visible & kept keys): the first
    and the last True of every row instead, lo / hi unused; the result has keep's leading shape."""
    if keep is not None:
        any_ = keep.any(-1)
        idx = torch.arange(keep.shape[-1], device=keep.device)
        a = torch.where(keep, idx, torch.full_like(idx, keep.shape[-1])).min(-1).values
        b = torch.where(keep, idx, torch.full_like(idx, -1)).max(-1).values
        if kind == "inner":                                             # the second and the second-to-last kept key, where the row has that many
            k2 = keep.clone()
            k2.scatter_(-1, a.clamp(max=keep.shape[-1] - 1).unsqueeze(-1), False)
            a2 = torch.where(k2, idx, torch.full_like(idx, keep.shape[-1])).min(-1).values
            k2 = keep.clone()
            k2.scatter_(-1, b.clamp(min=0).unsqueeze(-1), False)
            b2 = torch.where(k2, idx, torch.full_like(idx, -1)).max(-1).values
            many = keep.sum(-1) >= 4
            a, b = torch.where(many, a2, a), torch.where(many, b2, b)
        return torch.where(any_, a, torch.full_like(a, -1)), torch.where(any_, b, torch.full_like(b, -1))
    lo, hi = lo.cpu(), hi.cpu()
    g = _gen(seed)
    width = (hi - lo).clamp(min=1)
    inner = 1 if kind == "inner" else 0
    a_edge, b_edge = lo > 0, hi < Nkv
    a = torch.where(a_edge, torch.minimum(lo + inner, hi - 1), _uniform_in(lo, width, g))
    # b: the edge, or a uniform key other than a (a + 1 + r mod width, r uniform in [0, width - 1))
    r = _uniform_in(torch.zeros_like(lo), (width - 1).clamp(min=1), g)
    b = torch.where(b_edge, torch.maximum(hi - 1 - inner, lo), torch.where(width > 1, lo + (a - lo + 1 + r) % width, a))
    r = _uniform_in(torch.zeros_like(lo), (width - 1).clamp(min=1), g)
    a = torch.where(~a_edge & b_edge & (a == b) & (width > 1), lo + (b - lo + 1 + r) % width, a)
    dead = hi <= lo
    return torch.where(dead, torch.full_like(a, -1), a), torch.where(dead, torch.full_like(b, -1), b)


def _gather_rows(t, idx):
    """t [B,H,N,D], idx int64 [B,H,R] (>= 0) -> [B,H,R,D]."""
    return torch.gather(t, 2, idx.unsqueeze(-1).expand(*idx.shape, t.shape[-1]))


def two_pointer_inputs(B, H, Hkv, Nq, Nkv, D, dtype, pa, pb, seed, *args, draws=None, **kw):
    """two_pointer_draw(..., seed + 1000 t) for t = 0, 1, ... < draws (DRAWS_D): the first draw of keys and values that meets the conditions; the last
    draw's ValueError where none does.  (Among 3072 keys of 64 signs some third key matches the two targets on every sign they share, once in a few
    draws: a three-way tie that no c separates.  The conditions are the same for every draw; "draw" in the result says which one was taken.)"""
    for t in range(DRAWS_D if draws is None else draws):
        try:
            out = two_pointer_draw(B, H, Hkv, Nq, Nkv, D, dtype, pa, pb, seed + 1000 * t, *args, **kw)
            out["draw"] = t
            return out
        except ValueError as e:
            err = e
    raise err


def two_pointer_draw(B, H, Hkv, Nq, Nkv, D, dtype, pa, pb, seed, device=None, scale=None, visible=None, bias=None, softcap=0.0, kept=None, rs=1.0,
                     dlse=None, sig=1.0, c=None, per_query_head=False, spread_group=False):
    """-> dict(q, k, v, do, c, scale, pa, pb [B,H,Nq], leak [B,H,Nq], power = dict(dv, dq, dk: the smallest moved-element / bar ratio over the pairs),
    ref = dense64(...) of the inputs under the given modifiers: the expected values and the sums the bars are made of).
    pa, pb: int64 [Nq] or [B,Hkv,Nq], -1 for rows that see no key.  visible: None or bool broadcastable to [B,H,Nq,Nkv] (band and / or keep mask);
    bias: additive, broadcastable likewise (an additive mask, ALiBi as -slope |distance|); softcap; kept / rs: a dropout keep mask and 1 / (1 - p_eff);
    dlse: a gradient of the natural-log LSE [B,H,Nq].  Raises ValueError where the leak or the power condition fails (module docstring).
    per_query_head: the backward under test runs on expanded k / v and returns dK / dV per query head (the power condition then uses those bars, not a
    group's sum).  spread_group: row i points in ONE head of its group, head i mod g, and has q = 0 in the others (same map for all): g heads that
    point at one key put g summands under one dK / dV bar and each pair keeps 1 / g of its power — at bf16 and g = 16, 1.3 bars."""
    scale = D ** -0.5 if scale is None else scale
    g = _gen(seed)
    k = (torch.randint(0, 2, (B, Hkv, Nkv, D), generator=g) * 2 - 1).to(dtype)
    v = torch.randn((B, Hkv, Nkv, D), generator=g).to(dtype)
    noise = torch.randn((B, H, Nq, D), generator=g)
    dev = torch.device("cpu") if device is None else device
    k, v, noise = k.to(dev), v.to(dev), noise.to(dev)
    pa, pb = (_expand(t.to(dev).expand(B, Hkv, Nq) if t.dim() == 3 else t.to(dev).view(1, 1, Nq).expand(B, Hkv, Nq), H) for t in (pa, pb))
    live = pa >= 0
    if not bool(((pb >= 0) == live).all()):
        raise ValueError("two-pointer inputs: a row has one target and not the other")
    if spread_group and H != Hkv:
        g_ = H // Hkv
        mine = (torch.arange(Nq, device=dev)[None, :] % g_) == (torch.arange(H, device=dev)[:, None] % g_)
        pa, pb = (torch.where(mine[None], t, torch.full_like(t, -1)) for t in (pa, pb))
        live = pa >= 0
    ia, ib = pa.clamp(min=0), pb.clamp(min=0)
    for t in range(1, DRAWS_D + 1):                                     # k / v heads with a tie get new keys (the other heads keep theirs)
        tied = _tied_heads(k, ia, ib, live, visible, H)
        if not tied:
            break
        for (b_, h_) in tied:
            k[b_, h_] = (torch.randint(0, 2, (Nkv, D), generator=_gen(seed + 7919 * t + b_ * Hkv + h_)) * 2 - 1).to(dtype).to(dev)
    ke, ve = _expand(k, H), _expand(v, H)
    ka, kb_ = _gather_rows(ke, ia).float(), _gather_rows(ke, ib).float()
    va, vb = _gather_rows(ve, ia).float(), _gather_rows(ve, ib).float()
    do = (noise + (0.5 * sig) * (va - vb) * live.unsqueeze(-1)).to(dtype)
    mods = dict(keep=visible, bias=bias, softcap=softcap)
    cc = 4.0 if c is None else float(c)
    while True:
        assert math.log2(cc) == int(math.log2(cc)), "c must be a power of two"
        q = ((ka + kb_) * cc * live.unsqueeze(-1)).to(dtype)
        fwd = dense64(q, ke, ve, scale, **mods)
        p_a, p_b, _ = _target_p(q, ke, scale, fwd["lse"], ia, ib, bias, softcap, visible)
        leak = torch.where(live, 1.0 - p_a - torch.where(ia == ib, torch.zeros_like(p_b), p_b), torch.zeros_like(p_a))
        if bool(torch.isfinite(leak).all()) and float(leak.max()) <= POINTER_LEAK:
            break
        if c is not None or cc >= C_MAX_D or not float(leak.max()) < 0.2:       # (a fifth and more: a tie, the same at every c)
            raise ValueError("two-pointer inputs: 1 - P_a - P_b = %.3e > 2^-16 at c = %g (D = %d, Nkv = %d)" % (float(leak.max()), cc, D, Nkv))
        cc *= 2
    del fwd
    ref = dense64(q, ke, ve, scale, do=do, kept=kept, rs=rs, dlse=dlse, **mods)
    out = dict(q=q, k=k, v=v, do=do, c=cc, scale=scale, pa=pa, pb=pb, leak=leak, ref=ref, Hkv=Hkv, softcap=softcap, bias=bias, visible=visible, kept=kept, rs=rs, dlse=dlse,
               per_query_head=per_query_head)
    out["power"] = two_pointer_power(out, dtype)
    bad = [n for n, x in out["power"].items() if n != "dv_lone" and not x >= POWER_D]
    if bad:
        raise ValueError("two-pointer inputs: a dropped (row, target) pair moves %s by only %s bars (< %g)" % (bad, [round(out["power"][n], 2) for n in bad], POWER_D))
    return out


def _tied_heads(k, ia, ib, live, visible, H):
    """The k / v heads [(b, h)] in which some row sees a THIRD key that scores exactly what its two targets score: (k_a + k_b) . k_j = D + k_a . k_b, in
    integers (exact in f32).  No c separates such a key (P = 1/3 each): among 3072 keys of 64 signs it happens to one head in some fifteen."""
    B, Hkv, Nkv, D = k.shape
    g = H // Hkv
    out = []
    for b in range(B):
        for h in range(Hkv):
            kf = k[b, h].float()
            tie = False
            for hq in range(h * g, (h + 1) * g):                        # (a group's heads point the same way; their visible keys may differ)
                a, bb = ia[b, hq], ib[b, hq]
                gram = torch.matmul(kf[a] + kf[bb], kf.t())
                hit = gram >= (D + (kf[a] * kf[bb]).sum(-1))[:, None]
                rows = torch.arange(a.numel(), device=k.device)
                hit[rows, a] = False
                hit[rows, bb] = False
                if visible is not None:
                    hit &= visible.to(k.device).expand(B, H, a.numel(), Nkv)[b, hq]
                tie = tie or bool((hit & live[b, hq][:, None]).any())
            if tie:
                out.append((b, h))
    return out


def _target_p(q, ke, scale, lse2, ia, ib, bias, softcap, visible):
    """P of the two targets of every row [B,H,Nq] each and the soft-capping's d s / d x at them, in float64, from the reference's LSE (log2)."""
    res = []
    B, H, Nq, _ = q.shape
    for idx in (ia, ib):
        s = (q.double() * _gather_rows(ke, idx).double()).sum(-1) * scale
        fac = torch.ones_like(s)
        if softcap > 0:
            t = torch.tanh(s / softcap)
            s, fac = softcap * t, 1.0 - t * t
        if bias is not None:
            s = s + torch.gather(bias.to(q.device).expand(B, H, Nq, ke.shape[2]), 3, idx.unsqueeze(-1)).squeeze(-1).double()
        if visible is not None:
            ok = torch.gather(visible.to(q.device).expand(B, H, Nq, ke.shape[2]), 3, idx.unsqueeze(-1)).squeeze(-1)
            s = s.masked_fill(~ok, float("-inf"))
        res.append((torch.exp(s - lse2 / LOG2E), fac))
    return res[0][0], res[1][0], (res[0][1], res[1][1])


def _visible_count(inp, B, H, Nq):
    Nkv = inp["k"].shape[2]
    ok = torch.ones((B, H, Nq, Nkv), dtype=torch.bool, device=inp["q"].device)
    if inp["visible"] is not None:
        ok = ok & inp["visible"].to(ok.device)
    if inp["bias"] is not None:
        ok = ok & ~torch.isneginf(inp["bias"].to(ok.device))
    return ok.sum(-1)


def two_pointer_power(inp, dtype):
    """The power condition's figures: over every (row, target) pair, the smallest of max_c |what leaving the pair out of the backward moves| / bar, for dV
    (all pairs) and for dQ and dK (rows with two targets).  float64, from inp["ref"]."""
    ref, q, do = inp["ref"], inp["q"], inp["do"].double()
    B, H, Nq, D = q.shape
    Hkv = inp["Hkv"]
    ke, ve = _expand(inp["k"], H), _expand(inp["v"], H)
    live = inp["pa"] >= 0
    two = live & (inp["pa"] != inp["pb"])
    # a row that can see ONE key has P = 1 whatever the scores are (a packed sequence of one key under 700 rows: no element of that key's dV can resolve one
    # of 700 summands); leaving its pair out of the forward gives O = 0 for v, 1 / (2 u) bars.  Such rows are reported apart ("dv_lone"), not refused.
    lone = live & (_visible_count(inp, B, H, Nq) == 1)
    ia, ib = inp["pa"].clamp(min=0), inp["pb"].clamp(min=0)
    p_a, p_b, facs = _target_p(q, ke, inp["scale"], ref["lse"], ia, ib, inp["bias"], inp["softcap"], inp["visible"])
    delta = (do * ref["o"]).sum(-1)
    if inp["dlse"] is not None:
        delta = delta - inp["dlse"].double()
    # the bars of dK / dV belong to the k / v heads: a group's query heads add up (fold_kv_heads), and so do their bars
    dvb, dkb = (f(ref, dtype) if inp["per_query_head"] else _expand(fold_kv_heads(f(ref, dtype), Hkv), H) for f in (dv_bar_d, dk_bar_d))
    dqb = dq_bar_d(ref, dtype)
    inf = torch.full((B, H, Nq), float("inf"), dtype=torch.float64, device=q.device)
    worst = dict(dv=inf, dq=inf, dk=inf, dv_lone=inf)
    for idx, p, fac in ((ia, p_a, facs[0]), (ib, p_b, facs[1])):
        pd = p * inp["rs"]                                               # (the targets are kept keys)
        r_dv = ((pd.unsqueeze(-1) * do).abs() / _gather_rows(dvb, idx)).max(-1).values
        ds = p * ((do * _gather_rows(ve, idx).double()).sum(-1) * inp["rs"] - delta) * fac * inp["scale"]
        r_dq = ((ds.unsqueeze(-1) * _gather_rows(ke, idx).double()).abs() / dqb).max(-1).values
        r_dk = ((ds.unsqueeze(-1) * q.double()).abs() / _gather_rows(dkb, idx)).max(-1).values
        worst["dv"] = torch.minimum(worst["dv"], torch.where(live & ~lone, r_dv, inf))
        worst["dv_lone"] = torch.minimum(worst["dv_lone"], torch.where(lone, r_dv, inf))
        worst["dq"] = torch.minimum(worst["dq"], torch.where(two, r_dq, inf))
        worst["dk"] = torch.minimum(worst["dk"], torch.where(two, r_dk, inf))
    return {n: float(x.min()) for n, x in worst.items()}


def check_two_pointer(inp, dtype, o=None, dq=None, dk=None, dv=None):
    """-> (failures, {tensor: worst err / bar}) of whichever results are given against inp["ref"] and the class-D bars.  dk, dv: per k / v head
    [B,Hkv,Nkv,D] (the reference and its bars are summed over each group), or, for inputs built with per_query_head, per query head [B,H,Nkv,D] (a backward
    run on expanded k / v).  Rows that see no key must have dQ = 0 exactly."""
    ref, Hkv, per_query_head = inp["ref"], inp["Hkv"], inp["per_query_head"]
    fold = (lambda t: t) if per_query_head else (lambda t: fold_kv_heads(t, Hkv))
    items = [("O", o, ref["o"], o_bar_d(ref, dtype)), ("dQ", dq, ref["dq"], dq_bar_d(ref, dtype)),
             ("dK", dk, fold(ref["dk"]), fold(dk_bar_d(ref, dtype))), ("dV", dv, fold(ref["dv"]), fold(dv_bar_d(ref, dtype)))]
    fails, worst = [], {}
    for name, got, want, bar in items:
        if got is None:
            continue
        fails += check_elements(name, got, want, bar)
        worst[name] = worst_ratio(got, want, bar) if bool(torch.isfinite(got.double()).all()) else float("nan")
    if dq is not None:
        dead = torch.isinf(ref["lse"])
        if bool(dead.any()) and not bool((dq.double()[dead] == 0).all()):
            fails.append("dQ: rows that see no key are not exactly 0")
    return fails, worst
