"""CPU tests of tests/key_probes.py: the builders' conditions, the same-contract oracle inside every bar, ten float64 mutants of dense attention outside,
and every case of tests/test_key_probes_gpu.py on its route on paper (the plan queries need no GPU).

The ten mutants (mutant(); Nq = Nkv = 4096, D = 128, N(0,1) inputs where the old comparators are concerned; `seam` at 2304 with two heads, `tail` at
Nkv = 4069).  "old" = what the suite had: the conftest rule |O - ref| <= ATOL + RTOL |ref| against the unmutated result, tools/fuzz_parity.py's O bar
2 FLOOR max|v| and its gradient bar 2 GRAD_TOL max(1, max|g|) against float64 (`python tests/test_key_probes.py old` prints the figures):

  mutant                                                   max O err (fp16 / bf16)   conftest rule      fuzz_parity's O bar, fp16 / bf16     rejected here by
                                                                                     (fp16 / bf16)      (rows 9, 10: its gradient bar)
  (1)  pair       one (row, key) pair, last row block      9.1e-5 / 3.7e-4           accepts / accepts  accepts / accepts (9.8e-3, 7.8e-2)  A: LSE, one count
  (2)  diag       j <= i - 1 for rows = 63 mod 64          1.7e-2 / 1.7e-2           rejects / rejects  rejects / ACCEPTS                A: LSE, 64 rows
  (3)  tail       key Nkv - 1 missed by 16 rows            2.2e-3 / 2.3e-3           rejects / ACCEPTS  ACCEPTS / ACCEPTS                A: LSE, 16 rows
  (4)  dup        tile t + 1 = tile t, one row block       2.7e-2 / 2.7e-2           rejects / rejects  rejects / ACCEPTS                A: O; B: O
  (5)  vswap      V rows j, j + 1 exchanged                1.1e-2 / 1.1e-2           rejects / rejects  rejects / ACCEPTS                A (causal): O; B: O
  (6)  norescale  O not rescaled at one seam               9.6e-2 / 9.6e-2           rejects / rejects  rejects / rejects                B: O (4e7 bars)
  (7)  seam       first tile from the previous head        4.6e-2 / 4.6e-2           rejects / rejects  rejects / ACCEPTS                A: O; B: O
  (8)  split      two parts, weights exchanged             1.5e-2 / 1.5e-2           rejects / rejects  rejects / ACCEPTS                A (causal): O; B: O
  (9)  dv_block   dV misses a row block x key tile         dV 3.5e-2 / 3.5e-2        -                  rejects (4.0e-3) / rejects by 10 % (3.2e-2)   B: dV (2047 / 255 bars); C: dV
  (10) dk_diag    dK misses the diagonal tiles (causal)    dK 2.1 / 2.1              -                  rejects / rejects                C: dK (633 / 63 bars)

(max errors over the whole tensor: one row with a large P on the touched key decides them.)  Every bf16 mutant but `norescale` passes
fuzz_parity's O bar; `pair` passes everything the suite had, in both dtypes.  Only the new checks are asserted below.

KAPPA (the dQ / dK bars' factor, tests/key_probes.py): `python tests/test_key_probes.py kappa` runs the oracle's backward on the class-C backward inputs of
the GPU tests and prints |g_oracle - g_float64| / bar(kappa = 1):

  plain     (1, 2, 1100, 1984, 128) fp16         dQ 0.316 dK 0.342        bf16          dQ 0.285 dK 0.421
  plain     (1, 2, 1100, 1984, 128) fp16 causal  dQ 1.177 dK 1.237        bf16 causal   dQ 1.274 dK 1.445
  m16_both  (1, 8, 640, 640, 128)   fp16 causal  dQ 2.039 dK 1.283        bf16          dQ 0.459 dK 0.464
  wave_pair (1, 2, 129, 127, 128)   fp16 causal  dQ 0.963 dK 1.061
  split     (1, 24, 3072, 3072, 64) bf16         dQ 0.295 dK 0.323
  long      (1, 2, 4096, 4096, 128) bf16 causal  dQ 1.948 dK 1.373
  largest: fp16 2.039, bf16 1.948 (an earlier draw of the same shapes: 1.58 / 2.02)  ->  KAPPA_MEASURED 2.04 / 2.02, KAPPA 4.08 / 4.04.
  The oracle's O and dV on the same inputs use at most 0.79 / 0.85 of their bars (the issue's estimate for output rounding alone: 0.47).
"""
import os
import sys

import numpy as np
import pytest
import torch

import conftest
import key_probes as kp
from oracle import fa2_oracle as fo

DTYPES = {0: torch.float16, 1: torch.bfloat16}
CONTRACTS = {"exact": 0, "prescale": fo.PRESCALE_Q, "lsum_p16": fo.LSUM_P16}


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def _from_bits(bits, dt):
    return torch.from_numpy(fo.bits_to_f32(bits, dt)).double()


def _oracle_fwd(q, k, v, dt, causal, contract, scale=None):
    flags = CONTRACTS[contract]
    if dt == 0 and flags & fo.PRESCALE_Q:
        flags |= fo.PRESCALE_FUSED
    o_bits, lse = fo.fwd_c(_bits(q), _bits(k), _bits(v), dt, causal, scale=scale, flags=flags)
    return _from_bits(o_bits, dt), torch.from_numpy(lse).double(), o_bits


def _twin(q, scale, dtype):
    """tools/fuzz_parity.py prescaled_q: what a folded launch sees."""
    return (q.float() * (scale * kp.LOG2E)).to(dtype), 1.0 / kp.LOG2E


def test_constants_agree_with_conftest_and_the_fuzz_tool():
    assert {DTYPES[c]: x for c, x in conftest.GRAD_TOL.items()} == kp.GRAD_TOL
    for dtype, (one, sub) in ((torch.float16, (2.0 ** -10, 2.0 ** -24)), (torch.bfloat16, (2.0 ** -7, 2.0 ** -133))):
        x = torch.tensor([1.0, -1.5, 1.9999, 2.0, 0.75, 0.0, 3e-8 if dtype == torch.float16 else 1e-39], dtype=torch.float64)
        want = [one, one, one, 2 * one, one / 2, sub, sub]
        assert kp.ulp(x, dtype).tolist() == want
        # the definition: the distance to the next representable value
        y = torch.tensor([0.3, 7.7, 1000.0, 1e-3]).to(dtype)
        nxt = (y.view(torch.int16) + 1).view(dtype)
        assert torch.equal(kp.ulp(y.double(), dtype), nxt.double() - y.double())
    # pointer_lse_bar is tools/fuzz_parity.py's lse_limit
    import importlib.util
    spec = importlib.util.spec_from_file_location("_fuzz_parity", os.path.join(conftest.ROOT, "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    from rocwmma_fattn import _fa2_lib

    class Plan:
        contract_tail = 0
    for D in (64, 128, 256):
        for dtype in (torch.float16, torch.bfloat16):
            for p16 in (False, True):
                for c in (4.0, 8.0, 16.0):
                    plan = Plan()
                    plan.contract = _fa2_lib.FA2_CONTRACT_LSUM_P16 if p16 else 0
                    q, k = torch.full((1, 1, 2, D), c), torch.ones((1, 1, 2, D))
                    assert fz.lse_limit(plan, q, k, D, D ** -0.5, dtype) == pytest.approx(kp.lse_logit_bar(c, 1.0, D, D ** -0.5, dtype, p16), rel=1e-6)


# ---------------------------------------------------------------------------------------------------------------- builder conditions
def _gpu_cases():
    sys.path.insert(0, os.path.dirname(os.path.realpath(__file__)))
    import test_key_probes_gpu as g
    return g


def test_every_gpu_case_names_its_route_on_paper():
    """The plan queries run without a GPU: every case of tests/test_key_probes_gpu.py reaches the kernel it is named for (the GPU run asserts it again)."""
    g = _gpu_cases()
    assert (1, 32, 1, 8192, 128, 0, False) in g.SPLIT_SHAPES and len(g.PERSISTENT) == 4
    routes = set()
    for c in g.FORWARD_CASES:
        g.route_of(c)
        routes.add(c["route"])
    assert routes == {"d128_m16", "d128_m32", "persistent", "persistent_long", "split", "d64", "d256", "short_kv", "compiled", "grouped"}
    for b in g.BACKWARD_CASES:
        g.bwd_route_of(b)


def test_row_ranges_match_the_brute_force_mask():
    cases = [dict(), dict(causal=True), dict(causal=True, bottom_right=True), dict(window=(3, 5)), dict(window=(70, 0), q_offset=9),
             dict(causal=True, window=(10, -1), q_offset=40), dict(window=(-1, 2), q_offset=0), dict(window=(5, 5), q_offset=200),
             dict(window=(0, 0), bottom_right=True)]
    for Nq, Nkv in ((1, 1), (5, 70), (70, 5), (67, 67), (130, 64)):
        for kw in cases:
            lo, hi = kp.row_ranges(Nq, Nkv, **kw)
            j = torch.arange(Nkv)[None]
            assert torch.equal((j >= lo[:, None]) & (j < hi[:, None]), kp.brute_mask(Nq, Nkv, **kw)), (Nq, Nkv, kw)
    g = _gpu_cases()
    for kw in g.WINDOW_CASES:                                # the GPU tests' bands, at their own sizes
        Nq, Nkv = kw["Nq"], kw["Nkv"]
        lo, hi = kp.row_ranges(Nq, Nkv, causal=kw["causal"], window=kw["window"], q_offset=kw["q_offset"])
        j = torch.arange(Nkv)[None]
        pos = torch.arange(Nq)[:, None] + kw["q_offset"]
        left, right = kw["window"][0], (0 if kw["causal"] else kw["window"][1])
        keep = torch.ones(Nq, Nkv, dtype=torch.bool)
        if left >= 0:
            keep &= j >= pos - left
        if right >= 0:
            keep &= j <= pos + right
        assert torch.equal((j >= lo[:, None]) & (j < hi[:, None]), keep), kw


def test_counting_sums_are_exact_in_f32_and_counts_resolve():
    g = _gpu_cases()
    nkv_max = max(s[3] for s in g.all_forward_shapes())
    assert nkv_max <= 16384 and 3 * nkv_max < 2 ** 24
    # one key more or less is at least 8.8e-5 of log2, 84 bars
    cnt = torch.arange(1, 16385, dtype=torch.float64)
    assert float((torch.log2(cnt[1:]) - torch.log2(cnt[:-1])).min()) >= 8.8e-5 > 64 * kp.LSE_COUNT_BAR
    q, k, v = kp.counting_inputs(1, 2, 1, 40, nkv_max, 16, torch.bfloat16, 1)
    assert float(k.abs().max()) == 0 and set(v.unique().tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    assert torch.equal(v.float().cumsum(2).double(), v.double().cumsum(2))          # the f32 running sums are the exact ones
    lo, hi = kp.row_ranges(40, nkv_max, causal=True, window=(100, 0), q_offset=5000)
    o, lse, bar = kp.counting_expect(v, lo, hi, 2, torch.bfloat16)
    j = torch.arange(nkv_max)[None]
    keep = (j >= lo[:, None]) & (j < hi[:, None])
    o2, lse2, bar2 = kp.counting_expect_mask(v, keep, 2, torch.bfloat16)
    assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(bar, bar2)


def test_pointer_margin_holds_for_every_gpu_pair_and_the_builder_refuses_a_leaky_one():
    g = _gpu_cases()
    seen = set()
    for (D, Nq, Nkv, causal) in sorted(g.pointer_pairs()):
        for kind, shift in g.maps_of(Nq, Nkv, causal):
            pi = kp.pointer_map(kind, Nq, Nkv, shift, seed=5)
            vis = (~torch.ones(Nq, Nkv, dtype=torch.bool).triu(1)) if causal else None
            inp = kp.pointer_inputs(1, 1, 1, Nq, Nkv, D, torch.bfloat16, pi, seed=D + Nkv, visible=vis)
            assert float(inp["leak"].max()) <= kp.POINTER_LEAK and inp["c"] <= (4.0 if D >= 128 else 8.0 if D >= 64 else 16.0), (D, Nq, Nkv, kind, shift, inp["c"])
            seen.add((D, inp["c"]))
    assert (128, 4.0) in seen
    with pytest.raises(ValueError):                         # head dim 64 at c = 4: some pair of keys is too much alike
        kp.pointer_inputs(1, 1, 1, 4096, 4096, 64, torch.float16, kp.pointer_map("shift", 4096, 4096, 65), seed=1, c=4)
    with pytest.raises(ValueError):
        kp.pointer_inputs(1, 1, 1, 64, 512, 16, torch.float16, kp.pointer_map("shift", 64, 512, 1), seed=1, c=4)


# ---------------------------------------------------------------------------------------------------------------- the oracle inside every bar
ORACLE_SHAPES = [(2, 300, 700, 128), (2, 257, 1024, 64)]        # H, Nq, Nkv, D (cut down: Nkv <= 1024)


@pytest.mark.parametrize("contract", list(CONTRACTS))
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_meets_the_counting_bars(shape, dt, contract):
    H, Nq, Nkv, D = shape
    dtype = DTYPES[dt]
    q, k, v = kp.counting_inputs(1, H, H, Nq, Nkv, D, dtype, seed=3)
    for causal in (False, True):
        o, lse, _ = _oracle_fwd(q, k, v, dt, causal, contract)
        lo, hi = kp.row_ranges(Nq, Nkv, causal=causal)
        o_exp, lse_exp, bar = kp.counting_expect(v, lo, hi, H, dtype)
        assert kp.check_counting(o, lse, o_exp, lse_exp, bar) == []


@pytest.mark.parametrize("contract", list(CONTRACTS))
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_meets_the_pointer_bars(shape, dt, contract):
    H, Nq, Nkv, D = shape
    dtype = DTYPES[dt]
    scale = D ** -0.5
    for causal in (False, True):
        vis = (~torch.ones(Nq, Nkv, dtype=torch.bool).triu(1)) if causal else None
        for kind, shift in (("causal", 1), ("causal", 65), ("perm", 0)) if causal else (("shift", 0), ("shift", 64), ("shift", Nkv // 2 + 17), ("perm", 0)):
            pi = kp.pointer_map(kind, Nq, Nkv, shift, seed=9)
            if causal and kind == "perm":
                pi = torch.minimum(pi, torch.arange(Nq))
            inp = kp.pointer_inputs(1, H, H, Nq, Nkv, D, dtype, pi, seed=11 + shift, visible=vis)
            o, lse, o_bits = _oracle_fwd(inp["q"], inp["k"], inp["v"], dt, causal, contract)
            o_exp, bar = kp.pointer_expect_o(inp, dtype)
            fails = kp.check_elements("O", o, o_exp, bar)
            lse_exp = kp.pointer_expect_lse(inp, dtype, folded=contract == "prescale")
            lbar = kp.pointer_lse_bar(inp, dtype, p16=contract == "lsum_p16")
            if not float((lse - lse_exp).abs().max()) <= lbar:
                fails.append("LSE err %.3e > %.3e" % (float((lse - lse_exp).abs().max()), lbar))
            if contract != "prescale":                      # (a differentiated call never folds the scale)
                do = torch.randn(inp["q"].shape, generator=torch.Generator().manual_seed(5)).to(dtype)
                dq, dk, dv = (_from_bits(b, dt) for b in fo.bwd_c(_bits(inp["q"]), _bits(inp["k"]), _bits(inp["v"]), o_bits, _bits(do),
                                                                  lse.float().numpy(), dt, causal))
                dv_exp, dv_bar = kp.pointer_expect_dv(inp, do, dtype)
                fails += kp.check_elements("dV", dv, dv_exp, dv_bar)
                ref = kp.dense64(inp["q"], inp["k"], inp["v"], scale, causal=causal, do=do)
                fails += kp.check_random(ref, dtype, dq=dq, dk=dk)
            assert fails == [], (causal, kind, shift, fails)


@pytest.mark.parametrize("contract", list(CONTRACTS))
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_meets_the_random_input_bars(shape, dt, contract):
    H, Nq, Nkv, D = shape
    dtype = DTYPES[dt]
    scale = D ** -0.5
    q, k, v, do = kp.random_inputs(1, H, H, Nq, Nkv, D, dtype, seed=21, with_do=True)
    for causal in (False, True):
        o, lse, o_bits = _oracle_fwd(q, k, v, dt, causal, contract)
        if contract == "prescale":
            qs, s_alt = _twin(q, scale, dtype)
            ref = kp.dense64(qs, k, v, s_alt, causal=causal)
            assert kp.check_random(ref, dtype, o=o) == []
            continue
        ref = kp.dense64(q, k, v, scale, causal=causal, do=do)
        dq, dk, dv = (_from_bits(b, dt) for b in fo.bwd_c(_bits(q), _bits(k), _bits(v), o_bits, _bits(do), lse.float().numpy(), dt, causal))
        assert kp.check_random(ref, dtype, o=o, dq=dq, dk=dk, dv=dv) == []
        print("worst / bar: O %.2f dQ %.2f dK %.2f dV %.2f" % (kp.worst_ratio(o, ref["o"], kp.o_bar(ref, dtype)), kp.worst_ratio(dq, ref["dq"], kp.dq_bar(ref, dtype)),
                                                                 kp.worst_ratio(dk, ref["dk"], kp.dk_bar(ref, dtype)), kp.worst_ratio(dv, ref["dv"], kp.dv_bar(ref, dtype))))


# ---------------------------------------------------------------------------------------------------------------- power: float64 mutants
def _attn_rows(q, k, v, scale, vis):
    """float64 attention of some rows: q [R, D], k / v [Nkv, D], vis bool [R, Nkv] or None -> o [R, D], lse (log2) [R], p [R, Nkv]."""
    s = (q @ k.t()) * scale
    if vis is not None:
        s = s.masked_fill(~vis, float("-inf"))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    return (e @ v) / l, ((m + torch.log(l)) * kp.LOG2E).squeeze(-1), e / l          # (numerator first, like a kernel: exact on counting inputs)


MUTANTS = ("pair", "diag", "tail", "dup", "vswap", "norescale", "seam", "split", "dv_block", "dk_diag")
BWD_MUTANTS = ("dv_block", "dk_diag")
RB = 256            # rows of a row block (the forward's workgroup); 64 keys per tile


def mutant(kind, q, k, v, scale, causal, do=None, prev=None):
    """Single-head float64 dense attention with one defect (None: none).  q [Nq, D], k / v [Nkv, D] in float64.  prev: (k, v) of the previous head ('seam').
    -> dict o, lse (, dq, dk, dv)."""
    Nq, Nkv = q.shape[0], k.shape[0]
    vis = (~torch.ones(Nq, Nkv, dtype=torch.bool).triu(1)) if causal else torch.ones(Nq, Nkv, dtype=torch.bool)
    last = slice((Nq - 1) // RB * RB, Nq)                   # the last row block
    mid = slice(Nq // 2 // RB * RB, Nq // 2 // RB * RB + RB)  # a row block in the middle of the sweep
    tmid = Nkv // 2 // 64                                   # a key tile that row block sees under causal too
    if kind == "pair":                                      # (1) one (row, key) pair at a 64-key boundary, last row block
        vis[last.start + 100, tmid * 64] = False
    elif kind == "diag":                                    # (2) j <= i - 1 for rows = 63 mod 64
        assert causal
        r = torch.arange(63, min(Nq, Nkv), 64)
        vis[r, r] = False
    elif kind == "tail":                                    # (3) the last key of a ragged tail missed by one group of 16 rows
        assert Nkv % 64 != 0
        vis[last.start + 32:last.start + 48, Nkv - 1] = False
    o, lse, p = _attn_rows(q, k, v, scale, vis)
    if kind in ("dup", "vswap", "seam"):
        k2, v2 = k.clone(), v.clone()
        rows = mid
        if kind == "dup":                                   # (4) tile t + 1 is a second copy of tile t, K and V, one row block
            t = tmid
            k2[(t + 1) * 64:(t + 2) * 64], v2[(t + 1) * 64:(t + 2) * 64] = k[t * 64:(t + 1) * 64], v[t * 64:(t + 1) * 64]
        elif kind == "vswap":                               # (5) V rows j, j + 1 exchanged within one tile, one row block
            j = tmid * 64 + 20 if not causal else mid.start + 20      # (causal: a pair on the diagonal of the block)
            v2[[j, j + 1]] = v[[j + 1, j]]
        else:                                               # (7) the first key tile comes from the previous head's last tile, one row block
            rows = slice(0, RB)
            n = min(64, Nkv - (Nkv - 1) // 64 * 64)
            k2[:n], v2[:n] = prev[0][(Nkv - 1) // 64 * 64:], prev[1][(Nkv - 1) // 64 * 64:]
        o[rows], lse[rows], _ = _attn_rows(q[rows], k2, v2, scale, vis[rows])
    elif kind == "norescale":                               # (6) O not rescaled when the maximum moves at one tile seam of one row block
        rows, cut = mid, (tmid - 1) * 64
        s = ((q[rows] @ k.t()) * scale).masked_fill(~vis[rows], float("-inf"))
        m_before, m_all = s[:, :cut].max(-1, keepdim=True).values, s.max(-1, keepdim=True).values
        acc = torch.exp(s[:, :cut] - m_before) @ v[:cut] + torch.exp(s[:, cut:] - m_all) @ v[cut:]      # (the first part keeps its old reference)
        o[rows] = acc / torch.exp(s - m_all).sum(-1, keepdim=True)
    elif kind == "split":                                   # (8) two parts merged with the parts' weights exchanged
        half = Nkv // 2
        o1, l1, _ = _attn_rows(q, k[:half], v[:half], scale, vis[:, :half])
        has2 = vis[:, half:].any(-1)
        o2, l2 = torch.zeros_like(o1), torch.full_like(l1, float("-inf"))
        o2[has2], l2[has2], _ = _attn_rows(q[has2], k[half:], v[half:], scale, vis[has2][:, half:])
        w1 = 1.0 / (1.0 + torch.exp2(l2 - l1))
        o = (1.0 - w1)[:, None] * o1 + w1[:, None] * o2     # (w1 belongs to part 1)
    out = dict(o=o, lse=lse)
    if do is not None:
        dp = do @ v.t()
        delta = (do * (p @ v)).sum(-1, keepdim=True)
        ds = p * (dp - delta) * scale
        pv = p.clone()
        if kind == "dv_block":                              # (9) dV misses one row block's contribution to one key tile
            pv[mid, tmid * 64:(tmid + 1) * 64] = 0
        if kind == "dk_diag":                               # (10) dK misses the diagonal tile's contribution under causal
            assert causal
            ds = ds.clone()
            for t in range(min(Nq, Nkv) // 64):
                ds[t * 64:(t + 1) * 64, t * 64:(t + 1) * 64] = 0
            out.update(dq=(p * (dp - delta) * scale) @ k, dk=ds.t() @ q, dv=pv.t() @ do)
        else:
            out.update(dq=ds @ k, dk=ds.t() @ q, dv=pv.t() @ do)
    return out


def _as_output(res, dtype):
    """What a kernel hands back: 16-bit O and gradients, f32 LSE."""
    return {n: (t.float().double() if n == "lse" else t.to(dtype).double()) for n, t in res.items()}


def _new_checks(cls, inp, res, dtype, causal):
    """The new checks of input class `cls` on one head's results -> failures."""
    h = inp["head"]
    if cls == "A":
        return kp.check_counting(res["o"], res["lse"], inp["o_exp"][0, h], inp["lse_exp"][0, h], inp["o_bar"][0, h])
    if cls == "B":
        fails = kp.check_elements("O", res["o"], inp["o_exp"][0, h], inp["o_bar"][0, h])
        if not float((res["lse"] - inp["lse_exp"]).abs().max()) <= inp["lse_bar"]:
            fails.append("LSE")
        if "dv" in res:
            fails += kp.check_elements("dV", res["dv"], inp["dv_exp"][0, h], inp["dv_bar"][0, h])
        return fails
    ref = {n: t[0, h] for n, t in inp["ref"].items()}
    return kp.check_random(ref, dtype, o=res["o"], dq=res.get("dq"), dk=res.get("dk"), dv=res.get("dv"))


def _class_inputs(cls, Nq, Nkv, dtype, causal, bwd, H=1, pmap=None):
    D = 128
    scale = D ** -0.5
    if cls == "A":
        q, k, v = kp.counting_inputs(1, H, H, Nq, Nkv, D, dtype, seed=31)
        lo, hi = kp.row_ranges(Nq, Nkv, causal=causal)
        o_exp, lse_exp, bar = kp.counting_expect(v, lo, hi, H, dtype)
        return dict(q=q, k=k, v=v, o_exp=o_exp, lse_exp=lse_exp, o_bar=bar, scale=scale)
    if cls == "B":
        kind, shift = pmap
        pi = kp.pointer_map(kind, Nq, Nkv, shift, seed=3)
        vis = (~torch.ones(Nq, Nkv, dtype=torch.bool).triu(1)) if causal else None
        inp = kp.pointer_inputs(1, H, H, Nq, Nkv, D, dtype, pi, seed=32, visible=vis)
        inp["o_exp"], inp["o_bar"] = kp.pointer_expect_o(inp, dtype)
        inp["lse_exp"], inp["lse_bar"] = kp.pointer_expect_lse(inp, dtype), kp.pointer_lse_bar(inp, dtype, p16=False)
        if bwd:
            inp["do"] = torch.randn(inp["q"].shape, generator=torch.Generator().manual_seed(33)).to(dtype)
            inp["dv_exp"], inp["dv_bar"] = kp.pointer_expect_dv(inp, inp["do"], dtype)
        return inp
    t = kp.random_inputs(1, H, H, Nq, Nkv, D, dtype, seed=34, with_do=True)
    inp = dict(q=t[0], k=t[1], v=t[2], do=t[3], scale=scale)
    inp["ref"] = kp.dense64(t[0], t[1], t[2], scale, causal=causal, do=t[3] if bwd else None)
    return inp


# which class (and which call) each mutant is shown to: (class, causal, pointer map)
POWER_PLAN = {
    "pair": [("A", False, None)],
    "diag": [("A", True, None)],
    "tail": [("A", False, None)],
    "dup": [("A", False, None), ("B", False, ("shift", 0))],
    "vswap": [("A", True, None), ("B", False, ("shift", 0))],
    "norescale": [("B", False, ("shift", 0)), ("B", True, ("causal", 65))],
    "seam": [("A", False, None), ("B", False, ("shift", 0))],
    "split": [("A", True, None), ("B", False, ("shift", 65))],
    "dv_block": [("B", False, ("shift", 0)), ("C", False, None)],
    "dk_diag": [("C", True, None)],
}


def _sizes(kind):
    if kind == "seam":
        return 2304, 2304, 2          # an item seam: the second head of two
    if kind == "tail":
        return 4096, 4096 - 27, 1     # a ragged tail
    return 4096, 4096, 1


_INPUT_CACHE = {}


def _inputs(cls, kind, dtype, causal, pmap):
    Nq, Nkv, H = _sizes(kind)
    bwd = kind in BWD_MUTANTS
    key = (cls, Nq, Nkv, H, dtype, causal, bwd, pmap)
    if key not in _INPUT_CACHE:
        _INPUT_CACHE.clear() if len(_INPUT_CACHE) > 6 else None
        _INPUT_CACHE[key] = _class_inputs(cls, Nq, Nkv, dtype, causal, bwd, H, pmap)
    return _INPUT_CACHE[key], H


def _run(kind, inp, H, causal, bwd):
    h = H - 1
    q, k, v = (inp[n][0, h].double() for n in "qkv")
    prev = (inp["k"][0, h - 1].double(), inp["v"][0, h - 1].double()) if H > 1 else None
    do = inp["do"][0, h].double() if bwd else None
    inp["head"] = h
    return mutant(kind, q, k, v, inp["scale"], causal, do=do, prev=prev)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("kind", MUTANTS)
def test_power_every_mutant_is_rejected_and_the_plain_result_is_not(kind, dt):
    dtype = DTYPES[dt]
    bwd = kind in BWD_MUTANTS
    rejected = []
    for cls, causal, pmap in POWER_PLAN[kind]:
        inp, H = _inputs(cls, kind, dtype, causal, pmap)
        plain = _new_checks(cls, inp, _as_output(_run(None, inp, H, causal, bwd), dtype), dtype, causal)
        assert plain == [], ("float64 dense attention, rounded once, must be inside every bar", cls, causal, plain)
        fails = _new_checks(cls, inp, _as_output(_run(kind, inp, H, causal, bwd), dtype), dtype, causal)
        if fails:
            rejected.append((cls, causal, fails))
    assert rejected, "mutant %r passed every new check" % kind
    print(kind, [(c, ca, f[0][:60]) for c, ca, f in rejected])


# ---------------------------------------------------------------------------------------------------------------- measurements (python tests/test_key_probes.py ...)
def old_verdicts():
    """Per mutant, on N(0,1) inputs: what the OLD comparators say (the module docstring's table)."""
    rows = []
    for kind in MUTANTS:
        for dt in (0, 1):
            dtype = DTYPES[dt]
            causal = kind in ("diag", "dk_diag")
            bwd = kind in BWD_MUTANTS
            Nq, Nkv, H = _sizes(kind)
            t = kp.random_inputs(1, H, H, Nq, Nkv, 128, dtype, seed=34, with_do=True)
            inp = dict(q=t[0], k=t[1], v=t[2], do=t[3], scale=128 ** -0.5)
            good = _as_output(_run(None, inp, H, causal, bwd), dtype)
            plain64 = _run(None, inp, H, causal, bwd)
            bad = _as_output(_run(kind, inp, H, causal, bwd), dtype)
            d = (bad["o"] - good["o"]).abs()
            conf = bool((d <= conftest.ATOL[dt] + conftest.RTOL[dt] * good["o"].abs()).all())
            vmax = max(1.0, float(inp["v"].float().abs().max()))
            err_o = float((bad["o"] - plain64["o"]).abs().max())
            fz = err_o <= 2 * conftest.FLOOR[dt] * vmax
            line = "%-10s %-4s O err %.2e: conftest %s, fuzz_parity O bar %.2e %s" % (kind, "fp16" if dt == 0 else "bf16", err_o, "accepts" if conf else "rejects",
                                                                                      2 * conftest.FLOOR[dt] * vmax, "accepts" if fz else "rejects")
            if bwd:
                for n in ("dk", "dv"):
                    e = float((bad[n] - plain64[n]).abs().max())
                    lim = 2 * conftest.GRAD_TOL[dt] * max(1.0, float(plain64[n].abs().max()))
                    line += "; %s err %.2e vs %.2e %s" % (n, e, lim, "accepts" if e <= lim else "rejects")
            rows.append(line)
            print(line, flush=True)
    return rows


def measure_kappa():
    """The largest |g_oracle - g_float64| / bar(kappa = 1) of the same-contract oracle backward (fed its own forward) on the class-C inputs of the GPU tests
    themselves: tests/test_key_probes_gpu.py BACKWARD_CASES, same seed, every head."""
    g = _gpu_cases()
    worst = {0: 0.0, 1: 0.0}
    for b in g.BACKWARD_CASES:
        route, B, H, Nq, Nkv, D, dtype, causal, ws, classes, kernels = b
        if "C" not in classes:
            continue
        dt = 0 if dtype == torch.float16 else 1
        q, k, v, do = kp.random_inputs(B, H, H, Nq, Nkv, D, dtype, seed=g.SEED_C_BWD, with_do=True)
        o, lse, o_bits = _oracle_fwd(q, k, v, dt, causal, "exact")
        dq, dk, dv = (_from_bits(x, dt) for x in fo.bwd_c(_bits(q), _bits(k), _bits(v), o_bits, _bits(do), lse.float().numpy(), dt, causal))
        ref = kp.dense64(q, k, v, D ** -0.5, causal=causal, do=do)
        rq, rk = kp.worst_ratio(dq, ref["dq"], kp.dq_bar(ref, dtype, kappa=1.0)), kp.worst_ratio(dk, ref["dk"], kp.dk_bar(ref, dtype, kappa=1.0))
        ro, rv = kp.worst_ratio(o, ref["o"], kp.o_bar(ref, dtype)), kp.worst_ratio(dv, ref["dv"], kp.dv_bar(ref, dtype))
        worst[dt] = max(worst[dt], rq, rk)
        print("%-9s %s %s%s: dQ %.3f dK %.3f   (O %.3f, dV %.3f of their bars)" % (route, (B, H, Nq, Nkv, D), "fp16" if dt == 0 else "bf16", " causal" if causal else "",
                                                                                 rq, rk, ro, rv), flush=True)
    print("largest: fp16 %.3f bf16 %.3f" % (worst[0], worst[1]))


if __name__ == "__main__":
    torch.manual_seed(0)
    {"kappa": measure_kappa, "old": old_verdicts}[sys.argv[1]]()
