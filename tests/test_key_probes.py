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

Class D (two-key pointer inputs, tests/key_probes.py): the tests below prove the maps inside the brute-force mask, the builder's conditions for every
class-D case of tests/test_key_probes_gpu.py (cut down to one batch and one group of heads, the dense cases to two heads: the conditions of the
FULL shapes are established where the GPU test calls the builder, which refuses there as here; the cut-down proofs take about three minutes), the oracle (dense) or the fuzz tools' emulation (families) inside every bar,
and eleven float64 mutants of the BACKWARD outside (family64(): the forward is right, one pass is not).  `python tests/test_key_probes.py old_d` shows each
mutant to what the suite had, on N(0,1) inputs at 2048 keys under the mutant's own kind of call (band (70, 30) unless stated): tools/fuzz_features.py's bar
tol max(1, max|true|) with tol = GRAD_TOL (its other term, 2 err_emu, is smaller), GRAD_TOL max|true|, and class C; worst of dQ / dK / dV, fp16 / bf16:

  mutant                                                      fuzz_features' bar     GRAD_TOL max|g|        class C                 class D, worst bars (fp16 / bf16)
  dq_pair        one pair left out of the dQ pass     band    rejects / ACCEPTS      rejects / ACCEPTS      rejects / ACCEPTS       dQ 281 / 31, dK and dV untouched
                                            full attention    ACCEPTS / ACCEPTS      ACCEPTS / ACCEPTS      ACCEPTS (0.1 bars)
  dkv_pair       ... of the dK / dV pass              band    rejects / rejects      rejects / rejects      rejects / rejects       dK 615 / 68, dV 1004 / 127, dQ untouched
                                            full attention    ACCEPTS / ACCEPTS      ACCEPTS / ACCEPTS      ACCEPTS (0.7 bars)
  rows_short_lo  every key's row range one short, first row   rejects                rejects                rejects                 dK 713 / 79, dV 1024 / 128
  rows_short_hi  ... last row                                 rejects                rejects                rejects                 dK 692 / 77, dV 1024 / 128
  neighbour_key  a packed sequence's keys read one early (full attention; the sequence loses its last key.  The neighbour's key that such a read ADDS is
                 not modelled: a random key added to a row gets P ~ the leak, which no class resolves; the probe sees the key that goes missing)
                                                              rejects                rejects                rejects (bf16 dQ: 1.7)  dQ 288 / 32, dK 583 / 65, dV 1023 / 128
  top_left       bottom-right rows placed top-left            rejects                rejects                rejects                 dQ 652 / 73, dK 681 / 75, dV 1024 / 128
  delta_next_row delta of row i + 1 in the dQ pass            rejects                rejects                rejects                 dQ 337 / 38
  head_missing   one of four heads not in the group sum       rejects                rejects                rejects                 dK 187 / 77, dV 956 / 127
  dropout_transposed  mask [j, i] in the dK / dV pass         rejects                rejects                rejects                 dK 683 / 76, dV 1024 / > 1e8
  alibi_off_by_one    distance |i + off + 1 - j|              rejects / ACCEPTS dQ, dK (rejects dV by 10 %)   rejects / rejects     rejects (bf16: 1.4 .. 2.9)   20 .. 31 / 2.2 .. 4.4
  no_fac         1 - tanh^2 left out                          rejects                rejects                rejects                 dQ 479 / 53, dK 631 / 70

  What the suite could not see is ONE pair: under full attention at 2048 keys both pair mutants pass every old comparator in both dtypes, under a band of 101
  keys the bf16 dQ pair does.  The defects that touch every row or every key (a whole column of pairs, a wrong mask, a missing factor) were within reach of
  the per-tensor bars at these sizes; class D holds them by a further one to two orders, and tells the pass (dq_pair moves dQ alone, dkv_pair dK and dV alone).

KAPPA_D (tools/key_bars.py): `python tests/test_key_probes.py kappa_d`, the oracle's backward on the class-D inputs of the dense GPU cases (both map kinds where
the call has a band edge), |g_oracle - g_float64| / bar(kappa = 1):

  plain     (1, 2, 1100, 1984, 128) fp16         dQ 0.510 dK 0.714                                   bf16          dQ 0.537 dK 0.674
  plain     (1, 2, 1100, 1984, 128) fp16 causal  dQ 0.504 dK 0.769 (inner: 0.444, 0.717)              bf16 causal   dQ 0.546 dK 0.773 (inner: 0.490, 0.731)
  m16_both  (1, 8, 640, 640, 128)   fp16 causal  dQ 0.460 dK 0.746 (inner: 0.524, 0.779)              bf16          dQ 0.522 dK 0.819
  wave_pair (1, 2, 129, 127, 128)   fp16 causal  dQ 0.463 dK 0.572 (inner: 0.390, 0.813)
  split     (1, 24, 3072, 3072, 64) bf16         dQ 0.597 dK 0.937   (c = 32; every other case c = 4)
  largest: fp16 0.813, bf16 0.937  ->  KAPPA_D_MEASURED 0.82 / 0.94, KAPPA_D 1.64 / 1.88.  O and dV use at most 0.50 / 0.79 of their bars.
  The bf16 floor (2^-100) and the added term (delta through the rounded O) are derived in tools/key_bars.py.  There is no term for a P rounded to fp16
  before it meets dP - delta: the fp16 wave-pair dK / dV pass did that and failed the soft-capped band for it (P = 1.1e-8, true dK 2.2e-7, returned 0);
  the pass was changed, tests/test_key_probes_gpu.py test_pair_pass_keeps_a_pair_whose_p_is_below_fp16 keeps the reduced case.
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


# ---------------------------------------------------------------------------------------------------------------- class D: two-key pointer inputs
def _lse_refs():
    import lse_refs
    return lse_refs


def test_dense64_modifiers_agree_with_the_fuzz_tools_truth():
    """dense64's softcap= (with bias= as ALiBi, kept= / rs= as dropout, dlse=) against tools/fuzz_lse.py truth64 (autograd in float64)."""
    lr = _lse_refs()
    g = torch.Generator().manual_seed(41)
    H, Nq, Nkv, D, off = 3, 37, 53, 16, 9
    q, k, v, do = (torch.randn(s_, generator=g, dtype=torch.float64) * a for s_, a in (((H, Nq, D), 3.0), ((H, Nkv, D), 1.0), ((H, Nkv, D), 1.0), ((H, Nq, D), 1.0)))
    u = torch.randn((H, Nq), generator=g, dtype=torch.float64)
    allow = kp.brute_mask(Nq, Nkv, window=(20, 6), q_offset=off)
    allow[5] = False                                                           # a row that sees no key
    slopes = torch.tensor([0.3, 0.05, 0.0], dtype=torch.float64)
    kept = torch.rand((H, Nq, Nkv), generator=g) < 0.75
    gg = _gpu_cases()
    for cap, sl, drop, uu in ((0.0, None, None, None), (2.5, None, None, None), (2.5, slopes, None, u), (0.0, slopes, None, None), (1.5, None, kept, u), (0.0, None, kept, None)):
        want = lr.truth64(q, k, v, do, uu, allow, 0.25, softcap=cap, slopes=sl, off=off, keep=None if drop is None else drop.double(), rs=1.0 if drop is None else 1.25)
        bias = gg.alibi_bias(sl, Nq, Nkv, off) if sl is not None else None
        got = kp.dense64(q[None], k[None], v[None], 0.25, keep=allow, do=do[None], softcap=cap, bias=bias, kept=None if drop is None else drop[None],
                         rs=1.0 if drop is None else 1.25, dlse=None if uu is None else uu[None])
        for n, m in (("o", "O"), ("dq", "dQ"), ("dk", "dK"), ("dv", "dV")):
            assert float((got[n][0] - want[m]).abs().max()) <= 1e-12 * max(1.0, float(want[m].abs().max())), (cap, n)
        live = ~torch.isinf(want["lse"])
        assert torch.equal(torch.isinf(got["lse"][0]), ~live) and float((got["lse"][0][live] - want["lse"][live]).abs().max()) <= 1e-12
        assert float(got["dq"][0, :, 5].abs().max()) == 0.0


D_BANDS = [dict(), dict(causal=True), dict(causal=True, bottom_right=True), dict(window=(70, 30), q_offset=5), dict(window=(10, 10), q_offset=600),
           dict(window=(100, 0), q_offset=200, causal=True), dict(window=(-1, 3)), dict(window=(1000, -1), q_offset=1300, causal=True), dict(window=(40, 0), causal=True, bottom_right=True),
           dict(window=(0, 0)), dict(window=(60, 40), q_offset=200)]


def _definition_mask(Nq, Nkv, causal=False, bottom_right=False, window=(-1, -1), q_offset=0):
    """brute_mask's definition, pair by pair but vectorised (no closed form, no clamp: test_row_ranges_match_the_brute_force_mask's way for the large sizes)."""
    pos = torch.arange(Nq)[:, None] + q_offset + ((Nkv - Nq) if bottom_right else 0)
    j = torch.arange(Nkv)[None]
    left, right = window[0], (0 if causal else window[1])
    keep = torch.ones(Nq, Nkv, dtype=torch.bool)
    if left >= 0:
        keep &= j >= pos - left
    if right >= 0:
        keep &= j <= pos + right
    return keep


def test_two_pointer_maps_stay_inside_the_brute_force_mask():
    """Every band, offset and alignment the GPU tests use (and a band one key wide), at sizes with every kind of row: both kinds of map point at visible keys,
    on the edge (or one inside) wherever the band and not the tensor bounds the row, at two different keys wherever the row sees two, nowhere where it sees none."""
    g = _gpu_cases()
    sizes = [(1, 1), (63, 64), (64, 63), (65, 700), (700, 1), (130, 520), (300, 700), (700, 900), (300, 2000)]
    used = [dict(causal=w["causal"], window=w["window"], q_offset=w["q_offset"]) for w in g.WINDOW_CASES]
    assert all(any(u == {**dict(causal=False, window=(-1, -1), q_offset=0), **b} for b in D_BANDS) for u in used)
    assert all(torch.equal(kp.brute_mask(40, 90, **kw), _definition_mask(40, 90, **kw)) for kw in D_BANDS)
    for Nq, Nkv in sizes:
        for kw in D_BANDS:
            mask = kp.brute_mask(Nq, Nkv, **kw) if Nq * Nkv <= 4096 else _definition_mask(Nq, Nkv, **kw)
            lo, hi = kp.row_ranges(Nq, Nkv, **kw)
            rows = torch.arange(Nq)
            for kind in ("edge", "inner"):
                a, b = kp.two_pointer_maps(lo, hi, Nkv, seed=7, kind=kind)
                live = hi > lo
                assert torch.equal(a >= 0, live) and torch.equal(b >= 0, live), (Nq, Nkv, kw)
                assert bool(mask[rows[live], a[live]].all()) and bool(mask[rows[live], b[live]].all()), (Nq, Nkv, kw, kind)
                assert bool((a != b)[live & (hi - lo > 1)].all())
                inner = 1 if kind == "inner" else 0
                wide = live & (hi - lo > 2)
                assert torch.equal(a[wide & (lo > 0)], (lo + inner)[wide & (lo > 0)]) and torch.equal(b[wide & (hi < Nkv)], (hi - 1 - inner)[wide & (hi < Nkv)])
    keep = torch.rand((2, 3, 40, 70), generator=torch.Generator().manual_seed(3)) < 0.3
    keep[0, 0, 4] = False
    for kind in ("edge", "inner"):
        a, b = kp.two_pointer_maps(None, None, 70, 0, kind=kind, keep=keep)
        live = keep.any(-1)
        assert torch.equal(a >= 0, live) and not bool(live[0, 0, 4])
        assert bool(torch.gather(keep, 3, a.clamp(min=0)[..., None])[live].all()) and bool(torch.gather(keep, 3, b.clamp(min=0)[..., None])[live].all())
        if kind == "edge":
            first = keep.float().argmax(-1)
            assert torch.equal(a[live], first[live]) and bool((b >= a).all())


def _d_case_inputs(dtype):
    """(tag, inputs) of every class-D GPU case, built on the CPU at one batch and one k / v head with its group, the dense cases at two heads.  What is
    proved here is proved for these cut-down inputs; the conditions of the full-shape inputs are established on the GPU run, where the test's own call of
    the builder checks them and raises if one fails."""
    g = _gpu_cases()
    for b in g.BACKWARD_CASES:
        if "B" in b[9] and b[6] == dtype:
            for kind in g.D_KINDS if b[7] else g.D_KINDS[:1]:
                yield "dense %s %s" % (b[0], kind), g.dense_d_inputs(b[:2] + (2,) + b[3:], kind)
    for w in g.window_d_cases():
        if w["dtype"] == dtype and not w["rows"]:
            for kind in g.D_KINDS:
                yield "window %s %s" % (g._wid(w), kind), g.window_d_inputs(w, kind, None, 1, 2, 1, g._dlse_of(1, 2, w["Nq"], 143, None) if w["dlse"] else None)
    for gq in g.GROUPED_D:
        if gq[2] == dtype:
            yield "grouped %s" % (gq[:2],), g.grouped_d_inputs(gq, "edge", None, H=gq[0] // gq[1], Hkv=1)
    for m in g.MASK_D:
        yield "mask %s" % m[0], g.mask_d_inputs((m[0], 1, 2) + m[3:], dtype, None)[0]
    for with_lse in (False, True):
        yield "dropout%s" % (" lse" if with_lse else ""), g.dropout_d_inputs(dtype, with_lse, None)[0]
    for sm in g.SCOREMOD_D:
        yield "scoremod %s" % sm[0], g.scoremod_d_inputs(sm, dtype, None, B=1)[0]
    for pc in g.PACKED_D:
        for i, inp in enumerate(g._packed_d(pc[0], dtype, None, window=pc[1], dlse_seed=161 if pc[2] else None)[1]):
            if inp is not None:
                yield "packed %s seq %d" % (pc[0], i), inp
    for twin in ("dropout", "scoremod"):
        kw = dict(dropout=(g.DROP_P, g.DROP_SEED)) if twin == "dropout" else dict(smod=(1.5 * 4.0 * 128 * 128 ** -0.5, g._slopes(4, 101, None)))
        for i, inp in enumerate(g._packed_d("bottom_right", dtype, None, window=(40, 0), **kw)[1]):
            if inp is not None:
                yield "packed %s seq %d" % (twin, i), inp


def test_two_pointer_builder_refuses_what_is_no_probe():
    lo, hi = kp.row_ranges(300, 700)
    pa, pb = kp.two_pointer_maps(lo, hi, 700, seed=1)
    with pytest.raises(ValueError, match="1 - P_a - P_b"):                    # head dim 64 at c = 4: the rest of the row outweighs the margin
        kp.two_pointer_inputs(1, 1, 1, 300, 700, 64, torch.float16, pa, pb, seed=1, c=4)
    keep = torch.rand((1, 1, 300, 700), generator=torch.Generator().manual_seed(2)) < 0.5
    ka, kb_ = kp.two_pointer_maps(None, None, 700, 0, keep=keep)
    with pytest.raises(ValueError, match="moves"):                            # the first kept key of a random half is key 0 or 1 for most rows: no power
        kp.two_pointer_inputs(1, 1, 1, 300, 700, 128, torch.bfloat16, ka, kb_, seed=1, visible=keep, draws=2)
    with pytest.raises(ValueError, match="moves"):                            # a slope whose product with the band's width is 30: the farther target is gone
        kp.two_pointer_inputs(1, 1, 1, 300, 700, 128, torch.float16, *kp.two_pointer_maps(*kp.row_ranges(300, 700, window=(70, 30), q_offset=200), 700, seed=1), seed=1,
                              visible=kp.brute_mask(300, 700, window=(70, 30), q_offset=200), bias=_gpu_cases().alibi_bias(torch.tensor([0.3]), 300, 700, 200), draws=1)
    with pytest.raises(ValueError):                                           # a cap far below the targets' score: every key saturates
        kp.two_pointer_inputs(1, 1, 1, 300, 700, 128, torch.float16, pa, pb, seed=1, softcap=5.0, draws=1)
    # single-target rows (a band one key wide) are probes of O and dV; rows without a key get q = 0
    lo, hi = kp.row_ranges(90, 60, window=(0, 0), q_offset=0)
    pa, pb = kp.two_pointer_maps(lo, hi, 60, seed=1)
    inp = kp.two_pointer_inputs(1, 2, 1, 90, 60, 128, torch.bfloat16, pa, pb, seed=1, visible=kp.brute_mask(90, 60, window=(0, 0)))
    assert bool((pa == pb).all()) and int((pa < 0).sum()) == 30 and float(inp["q"][:, :, 60:].abs().max()) == 0 and inp["power"]["dq"] == float("inf")
    assert float(inp["ref"]["dq"][:, :, 60:].abs().max()) == 0 and inp["power"]["dv_lone"] >= kp.POWER_D


def _emulate_d(inp, dtype):
    """tools/fuzz_lse.py's same-contract emulation (f32, 16-bit P, dS, O and gradients) of the inputs' call, per batch -> o, dq, dk, dv like the reference
    (dK / dV per query head)."""
    lr = _lse_refs()
    B, H, Nq, D = inp["q"].shape
    Nkv = inp["k"].shape[2]
    ke, ve = kp._expand(inp["k"], H), kp._expand(inp["v"], H)
    outs = []
    for b in range(B):
        allow = torch.ones((H, Nq, Nkv), dtype=torch.bool) if inp["visible"] is None else inp["visible"].expand(B, H, Nq, Nkv)[b]
        bias = None if inp["bias"] is None else inp["bias"].expand(-1, H, Nq, Nkv)[b if inp["bias"].shape[0] > 1 else 0].float()
        kept = inp.get("kept")
        outs.append(lr.emulate(inp["q"][b], ke[b], ve[b], inp["do"][b], None if inp["dlse"] is None else inp["dlse"][b], allow, inp["scale"], dtype, softcap=inp["softcap"],
                               bias=bias, keep=None if kept is None else kept.expand(B, H, Nq, Nkv)[b], rs=inp["rs"]))
    return tuple(torch.stack([o[n] for o in outs]) for n in ("O", "dQ", "dK", "dV"))


@pytest.mark.parametrize("dt", [0, 1])
def test_two_pointer_conditions_hold_and_the_oracle_is_inside_every_bar(dt):
    """One pass over every class-D GPU case (the inputs and their float64 reference are built once): the builder's conditions — leak, power, c, exact q —
    and the same-contract C oracle (dense cases) or the fuzz tools' emulation (the families the oracle lacks) inside every bar."""
    dtype = DTYPES[dt]
    seen_c = set()
    for tag, inp in _d_case_inputs(dtype):
        pw = inp["power"]
        assert float(inp["leak"].max()) <= kp.POINTER_LEAK and all(pw[n] >= kp.POWER_D for n in ("dv", "dq", "dk")), (tag, pw)
        D = inp["q"].shape[-1]
        assert inp["c"] <= (4.0 if D >= 128 else 32.0), (tag, inp["c"])
        seen_c.add((D, inp["c"]))
        assert bool(torch.isin(inp["q"].float(), torch.tensor([-2 * inp["c"], 0.0, 2 * inp["c"]])).all())
        if tag.startswith("dense"):
            causal = inp["visible"] is not None
            o, lse, o_bits = _oracle_fwd(inp["q"], inp["k"], inp["v"], dt, causal, "exact")
            dq, dk, dv = (_from_bits(x, dt) for x in fo.bwd_c(_bits(inp["q"]), _bits(inp["k"]), _bits(inp["v"]), o_bits, _bits(inp["do"]), lse.float().numpy(), dt, causal))
        else:
            o, dq, dk, dv = _emulate_d(inp, dtype)
            if not inp["per_query_head"]:
                dk, dv = kp.fold_kv_heads(dk, inp["Hkv"]), kp.fold_kv_heads(dv, inp["Hkv"])
        fails, worst = kp.check_two_pointer(inp, dtype, o, dq, dk, dv)
        assert fails == [], (tag, fails)
    assert (128, 4.0) in seen_c and any(D == 64 for D, _ in seen_c)


# float64 mutants of one k / v head's group under a band, a mask, dropout and score modifiers: the forward is right, one of the two backward passes is not
D_MUTANTS = ("dq_pair", "dkv_pair", "rows_short_lo", "rows_short_hi", "neighbour_key", "top_left", "delta_next_row", "head_missing", "dropout_transposed", "alibi_off_by_one",
             "no_fac")


def family64(inp, mut=None, alt=None):
    """float64 attention of inp (B = 1, one k / v head) with the dQ pass and the dK / dV pass formed separately -> o, dq, dk, dv ([1,H,...]; dk / dv summed over
    the group unless the inputs are per query head).  alt: what the mutant needs (a wrong mask, a wrong bias, a wrong dropout mask)."""
    q, do = inp["q"][0].double(), inp["do"][0].double()
    H, Nq, D = q.shape
    k, v = inp["k"][0, 0].double(), inp["v"][0, 0].double()
    Nkv = k.shape[0]
    vis = torch.ones((H, Nq, Nkv), dtype=torch.bool) if inp["visible"] is None else inp["visible"].expand(1, H, Nq, Nkv)[0]
    bias = torch.zeros((H, Nq, Nkv), dtype=torch.float64) if inp["bias"] is None else inp["bias"].expand(1, H, Nq, Nkv)[0].double()
    kept = inp.get("kept")
    kd = torch.ones((H, Nq, Nkv), dtype=torch.float64) if kept is None else kept.expand(1, H, Nq, Nkv)[0].double() * inp["rs"]

    def probs(bias_, vis_):
        s = (q @ k.t()) * inp["scale"]
        fac = torch.ones_like(s)
        if inp["softcap"] > 0:
            t = torch.tanh(s / inp["softcap"])
            s, fac = inp["softcap"] * t, 1 - t * t
        return (s + bias_).masked_fill(~vis_, float("-inf")), fac
    s, fac = probs(bias, vis)
    m = s.max(-1, keepdim=True).values
    dead = torch.isinf(m)
    lse = torch.where(dead, m, torch.where(dead, m, m) + torch.log(torch.exp(s - torch.where(dead, torch.zeros_like(m), m)).sum(-1, keepdim=True)))
    p = torch.where(dead, torch.zeros_like(s), torch.exp(s - torch.where(dead, torch.zeros_like(lse), lse)))
    o = (p * kd) @ v
    delta = (do * o).sum(-1, keepdim=True)
    if inp["dlse"] is not None:
        delta = delta - inp["dlse"][0].double().unsqueeze(-1)
    # the backward recomputes P from the LSE under ITS idea of the scores and the mask
    pb, kdb, facb = p, kd, fac
    if mut in ("top_left", "neighbour_key"):
        pb = p * alt.expand(H, Nq, Nkv).double()
    if mut == "alibi_off_by_one":
        s2, _ = probs(alt.expand(1, H, Nq, Nkv)[0].double(), vis)
        pb = torch.where(dead, torch.zeros_like(s), torch.exp(s2 - torch.where(dead, torch.zeros_like(lse), lse)))
    if mut == "no_fac":
        facb = torch.ones_like(fac)
    dp = (do @ v.t())
    ds_q = pb * (dp * kdb - (delta.roll(-1, 1) if mut == "delta_next_row" else delta)) * facb * inp["scale"]
    kd_kv = alt.expand(1, H, Nq, Nkv)[0].double() * inp["rs"] if mut == "dropout_transposed" else kdb
    ds_k = pb * (dp * kd_kv - delta) * facb * inp["scale"]
    p_v = pb * kd_kv
    live = (inp["pa"][0] >= 0) & (inp["pa"][0] != inp["pb"][0])
    if mut in ("dq_pair", "dkv_pair"):                                       # one (row, target) pair: the last two-target row of the first head, its first target
        i = int(live[0].nonzero().flatten()[-1])
        j = int(inp["pa"][0, 0, i])
        if mut == "dq_pair":
            ds_q = ds_q.clone()
            ds_q[0, i, j] = 0
        else:
            ds_k, p_v = ds_k.clone(), p_v.clone()
            ds_k[0, i, j] = 0
            p_v[0, i, j] = 0
    if mut in ("rows_short_lo", "rows_short_hi"):                            # the transposed row range of every key one row short at one end
        idx = torch.arange(Nq)[None, :, None].expand(H, Nq, Nkv)
        edge = torch.where(vis, idx, torch.full_like(idx, Nq if mut == "rows_short_lo" else -1))
        edge = edge.min(1, keepdim=True).values if mut == "rows_short_lo" else edge.max(1, keepdim=True).values
        cut = (idx != edge).double()
        ds_k, p_v = ds_k * cut, p_v * cut
    dq = ds_q @ k
    dk, dv = ds_k.transpose(-1, -2) @ q, p_v.transpose(-1, -2) @ do
    if not inp["per_query_head"]:
        hs = slice(0, H - 1) if mut == "head_missing" else slice(0, H)
        dk, dv = dk[hs].sum(0, keepdim=True), dv[hs].sum(0, keepdim=True)
    return o[None], dq[None], dk[None], dv[None]


def _mutant_case(name, dtype):
    """-> (inputs, alt) of the call a mutant is shown to: the GPU tests' own cases at one batch and one group."""
    g = _gpu_cases()
    if name in ("dq_pair", "dkv_pair", "rows_short_lo", "rows_short_hi", "delta_next_row"):
        w = dict(g.WINDOW_CASES[1], D=128, dtype=dtype)
        lo, hi, vis = g._band_of(w["Nq"], w["Nkv"], window=w["window"], q_offset=w["q_offset"])
        pa, pb = kp.two_pointer_maps(lo, hi, w["Nkv"], seed=g.SEED_D + 2, kind="edge")
        return kp.two_pointer_inputs(1, 1, 1, w["Nq"], w["Nkv"], 128, dtype, pa, pb, seed=g.SEED_D + 3, visible=vis), None
    if name == "head_missing":
        lo, hi, vis = g._band_of(300, 700, window=(70, 30), q_offset=200)
        pa, pb = kp.two_pointer_maps(lo, hi, 700, seed=g.SEED_D + 4, kind="edge")
        return kp.two_pointer_inputs(1, 4, 1, 300, 700, 128, dtype, pa, pb, seed=g.SEED_D + 5, visible=vis, spread_group=dtype == torch.bfloat16), None
    if name == "neighbour_key":        # sequence 2 (63 x 64) of the packed test, full attention: the backward reads its keys one early and loses the last
        inp = g._packed_d("full", dtype, None)[1][2]
        alt = torch.ones((1, 63, 64), dtype=torch.bool)
        alt[:, :, 63] = False
        return inp, alt
    if name == "top_left":             # sequence 4 (65 x 700), bottom-right: the backward places the rows top-left
        return g._packed_d("bottom_right", dtype, None)[1][4], kp.brute_mask(65, 700, causal=True)[None]
    if name == "dropout_transposed":
        from rocwmma_fattn.FlashAttn import dropout_keep_mask
        inp = g.dropout_d_inputs(dtype, False, None)[0]
        inp["kept"] = dropout_keep_mask(g.DROP_SEED, g.DROP_P, 1, 2, 300, 700)
        return inp, dropout_keep_mask(g.DROP_SEED, g.DROP_P, 1, 2, 700, 300).transpose(-1, -2)
    sm = g.SCOREMOD_D[2]
    inp, cap, slopes, _ = g.scoremod_d_inputs(sm, dtype, None, B=1)
    return inp, g.alibi_bias(slopes, 700, 900, sm[2] + 1)


def _one_group(inp):
    """The first k / v head of the inputs with its query heads, as inputs of their own."""
    g_ = inp["q"].shape[1] // inp["Hkv"]
    out = dict(inp)
    for n in ("q", "do", "pa", "pb", "leak"):
        out[n] = inp[n][:1, :g_]
    for n in ("k", "v"):
        out[n] = inp[n][:1, :1]
    for n in ("visible", "bias", "kept", "dlse"):
        t = inp.get(n)
        if t is not None and t.dim() == 4:
            t = t[:1, :g_] if t.shape[1] > 1 else t[:1]
        elif t is not None and t.dim() == 3 and n == "dlse":
            t = t[:1, :g_]
        out[n] = t
    out["ref"] = {n: t[:1, :g_] for n, t in inp["ref"].items()}
    out["Hkv"] = 1
    return out


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("name", D_MUTANTS)
def test_two_pointer_probes_reject_every_backward_mutant(name, dt):
    dtype = DTYPES[dt]
    inp, alt = _mutant_case(name, dtype)
    inp = _one_group(inp)
    if alt is not None and alt.dim() == 4:
        alt = alt[:, :inp["q"].shape[1]]
    rnd = lambda ts: tuple(t.to(dtype).double() for t in ts)  # noqa: E731
    plain, _ = kp.check_two_pointer(inp, dtype, *rnd(family64(inp)))
    assert plain == [], ("float64 attention, rounded once, must be inside every bar", name, plain)
    o, dq, dk, dv = rnd(family64(inp, name, alt))
    fails, worst = kp.check_two_pointer(inp, dtype, o, dq, dk, dv)
    print(name, {n: round(x, 1) for n, x in worst.items()})
    assert fails != [], "mutant %r passed the class-D check" % name
    if name == "dq_pair":
        assert worst["dQ"] > 4 and max(worst["dK"], worst["dV"]) <= 1          # each pass is resolved apart
    if name == "dkv_pair":
        assert min(worst["dK"], worst["dV"]) > 4 and worst["dQ"] <= 1


@pytest.mark.parametrize("family", ["window", "scoremod"])
def test_a_p_rounded_to_fp16_before_ds_is_rejected_on_the_reduced_pair(family):
    """tests/test_key_probes_gpu.py tiny_p_inputs (one pair of P = 1e-8 under key j0): the reference alone puts dK_j0 above POWER_D bars; float64 attention
    rounded once is inside every bar; a dK formed from round16(P (1 - t^2)) — what the fp16 wave-pair pass handed from wave to wave — is outside (dK_j0 = 0);
    the same with round16(2^14 P (1 - t^2)) / 2^14, what the pass hands over now, is inside."""
    g = _gpu_cases()
    dtype = torch.float16
    cap = 1.5 * 4.0 * 128 * 128 ** -0.5 if family == "scoremod" else 0.0
    inp = g.tiny_p_inputs(cap, dtype)
    ref, j0 = inp["ref"], inp["j0"]
    assert float((ref["dk"][0, 0, j0].abs() / kp.dk_bar_d(ref, dtype)[0, 0, j0]).min()) >= kp.POWER_D
    rnd = lambda t: t.to(dtype).double()  # noqa: E731
    assert kp.check_two_pointer(inp, dtype, *(rnd(ref[n]) for n in ("o", "dq", "dk", "dv")))[0] == []
    q, k, v, do = (inp[n][0, 0].double() for n in ("q", "k", "v", "do"))
    s = (q @ k.t()) * inp["scale"]
    fac = torch.ones_like(s)
    if cap:
        t = torch.tanh(s / cap)
        s, fac = cap * t, 1 - t * t
    i, j = torch.arange(s.shape[0])[:, None], torch.arange(s.shape[1])[None]
    p = torch.softmax(s.masked_fill((j < i - 3) | (j > i + 3), float("-inf")), -1)
    core = (do @ v.t()) - (do * (p @ v)).sum(-1, keepdim=True)
    for gain, inside in ((1.0, False), (2.0 ** 14, True)):
        p16 = (p * fac * gain).to(dtype).double() / gain
        dk = rnd(rnd(p16 * core).t() @ q * inp["scale"])[None, None]
        fails, worst = kp.check_two_pointer(inp, dtype, dk=dk)
        print(family, gain, worst)
        assert (fails == []) == inside, (gain, fails)
        if not inside:
            assert bool((dk[0, 0, j0] == 0).all())


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


def measure_kappa_d():
    """measure_kappa() on the class-D inputs of the dense backward cases (dense_d_inputs of tests/test_key_probes_gpu.py: same seeds, both map kinds, every
    head): the largest |g_oracle - g_float64| / bar(kappa = 1) of dQ and dK under the class-D bars, and what O and dV use of theirs."""
    g = _gpu_cases()
    worst = {0: 0.0, 1: 0.0}
    for b in g.BACKWARD_CASES:
        route, B, H, Nq, Nkv, D, dtype, causal, ws, classes, kernels = b
        if "B" not in classes:
            continue
        dt = 0 if dtype == torch.float16 else 1
        for kind in g.D_KINDS:
            inp = g.dense_d_inputs(b, kind)
            ref = inp["ref"]
            o, lse, o_bits = _oracle_fwd(inp["q"], inp["k"], inp["v"], dt, causal, "exact")
            dq, dk, dv = (_from_bits(x, dt) for x in fo.bwd_c(_bits(inp["q"]), _bits(inp["k"]), _bits(inp["v"]), o_bits, _bits(inp["do"]), lse.float().numpy(), dt, causal))
            rq, rk = kp.worst_ratio(dq, ref["dq"], kp.dq_bar_d(ref, dtype, kappa=1.0)), kp.worst_ratio(dk, ref["dk"], kp.dk_bar_d(ref, dtype, kappa=1.0))
            ro, rv = kp.worst_ratio(o, ref["o"], kp.o_bar_d(ref, dtype)), kp.worst_ratio(dv, ref["dv"], kp.dv_bar_d(ref, dtype))
            worst[dt] = max(worst[dt], rq, rk)
            print("%-9s %s %s%s %-5s: dQ %.3f dK %.3f   (O %.3f, dV %.3f of their bars; c = %g, power at KAPPA_D = %s: %s)" % (
                route, (B, H, Nq, Nkv, D), "fp16" if dt == 0 else "bf16", " causal" if causal else "", kind, rq, rk, ro, rv, inp["c"], kp.KAPPA_D[dtype],
                {n: round(x, 1) for n, x in inp["power"].items()}), flush=True)
    print("largest: fp16 %.3f bf16 %.3f" % (worst[0], worst[1]))


def old_verdicts_d():
    """Per class-D mutant, on N(0,1) inputs at 2048 keys under the mutant's own kind of call: what the comparators the suite had say (the docstring's table)."""
    g = _gpu_cases()
    N, D = 2048, 128
    gen = torch.Generator().manual_seed(77)
    for name in D_MUTANTS + ("dq_pair full", "dkv_pair full"):
        for dt in (0, 1):
            dtype = DTYPES[dt]
            H = 4 if name == "head_missing" else 1
            nq = 1024 if name == "top_left" else N
            kw = dict(window=(70, 30), q_offset=5)
            if name == "neighbour_key" or name.endswith(" full"):
                kw = dict()
            if name == "top_left":
                kw = dict(causal=True, bottom_right=True)
            lo, hi, vis = g._band_of(nq, N, **kw)
            pa, pb = kp.two_pointer_maps(lo, hi, N, seed=3)
            q, do = (torch.randn((1, H, nq, D), generator=gen).to(dtype) for _ in range(2))
            k, v = (torch.randn((1, 1, N, D), generator=gen).to(dtype) for _ in range(2))
            inp = dict(q=q, k=k, v=v, do=do, scale=D ** -0.5, visible=vis, bias=None, softcap=0.0, kept=None, rs=1.0, dlse=None, pa=pa.expand(1, H, nq), pb=pb.expand(1, H, nq),
                       per_query_head=False, Hkv=1)
            alt = None
            if name == "neighbour_key":
                alt = torch.ones((1, nq, N), dtype=torch.bool)
                alt[:, :, N - 1] = False
            if name == "top_left":
                alt = kp.brute_mask(nq, N, causal=True)[None]
            if name == "dropout_transposed":
                from rocwmma_fattn.FlashAttn import dropout_keep_mask
                inp.update(kept=dropout_keep_mask(5, 0.25, 1, 1, nq, N), rs=4.0 / 3.0)
                alt = dropout_keep_mask(5, 0.25, 1, 1, N, nq).transpose(-1, -2)
            if name in ("alibi_off_by_one", "no_fac"):
                slopes = torch.tensor([3.0 / 101])
                inp.update(softcap=1.0, bias=g.alibi_bias(slopes, nq, N, 5))
                alt = g.alibi_bias(slopes, nq, N, 6)
            ref = kp.dense64(q, kp._expand(k, H), kp._expand(v, H), inp["scale"], keep=vis, do=do, bias=inp["bias"], softcap=inp["softcap"], kept=inp["kept"], rs=inp["rs"])
            bad = [t.to(dtype).double() for t in family64(inp, name.split()[0], alt)]
            line = "%-18s %s" % (name, "fp16" if dt == 0 else "bf16")
            for i, n in ((1, "dq"), (2, "dk"), (3, "dv")):
                true = kp.fold_kv_heads(ref[n], 1) if n != "dq" else ref[n]
                err = float((bad[i] - true).abs().max())
                tol = conftest.GRAD_TOL[dt]
                bar_c = {"dq": kp.dq_bar, "dk": kp.dk_bar, "dv": kp.dv_bar}[n](ref, dtype)
                bar_c = kp.fold_kv_heads(bar_c, 1) if n != "dq" else bar_c
                line += " | %s err %.1e: fuzz bar %.1e %s, GRAD_TOL max|g| %.1e %s, class C %.1f bars %s" % (
                    n, err, tol * max(1.0, float(true.abs().max())), "acc" if err <= tol * max(1.0, float(true.abs().max())) else "REJ",
                    tol * float(true.abs().max()), "acc" if err <= tol * float(true.abs().max()) else "REJ",
                    kp.ratio_max((bad[i] - true).abs(), bar_c), "acc" if kp.ratio_max((bad[i] - true).abs(), bar_c) <= 1 else "REJ")
            print(line, flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    {"kappa": measure_kappa, "old": old_verdicts, "kappa_d": measure_kappa_d, "old_d": old_verdicts_d}[sys.argv[1]]()
