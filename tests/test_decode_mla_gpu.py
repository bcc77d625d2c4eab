"""GPU tests of decode attention on a latent (MLA) KV cache (flash_attention_decode_mla / fa2_fwd_decode_mla; tests/mla_refs.py has the references,
whose bars are decode_refs.check's).  Every cache row beyond a length, every spare page and every page behind an unused block-table entry holds NaN;
outputs and workspace of the C-ABI calls start as NaN (mla_refs.mla_c)."""
import functools
import random

import pytest
import torch

import decode_calls as dc
import decode_refs as dr
import key_probes as kp
import mla_refs as mr
from conftest import ATOL, LSE_TOL, RTOL
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention_decode_mla, flash_attention_varlen, merge_attention

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 129, 300)
# a lone row; one tile; 15 rows under a head map that is no power of two; one row into a second tile; three tiles; one block; a block edge inside a
# token; two blocks; four blocks
ROWS = ((1, 1), (16, 1), (5, 3), (17, 1), (16, 3), (16, 4), (13, 5), (128, 1), (128, 2))
NMAX = 512            # 16 key tiles: the plan splits a small batch in two, a forced split of 3 leaves parts empty for the short sequences
LN2 = 0.6931471805599453


def _lens(p):
    """four of LENGTHS for row shape p: over the nine shapes every length is drawn three times or more"""
    return [LENGTHS[(4 * p + k) % len(LENGTHS)] for k in range(4)]


@functools.lru_cache(maxsize=None)
def _case(p, dtype):
    """inputs and references of row shape p, computed once and shared (nothing here changes them)"""
    H, Nq = ROWS[p]
    lens = _lens(p)
    q, kv = mr.inputs(len(lens), H, Nq, NMAX, lens, dtype, 300 + p)
    return q, kv, lens, mr.refs(q, kv, lens, dc.code(dtype))


def _dev_case(p, dtype):
    dev = dc.dev()
    q, kv, lens, refs = _case(p, dtype)
    return q.to(dev), kv.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), lens, refs


def test_every_length_is_drawn():
    assert {n for p in range(len(ROWS)) for n in _lens(p)} == set(LENGTHS)
    assert any(n < ROWS[p][1] and n > 0 for p in range(len(ROWS)) for n in _lens(p)), "a sequence shorter than Nq"


@pytest.mark.parametrize("split", [1, 3, 0])
@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("p", range(len(ROWS)))
def test_lengths_and_rows(p, dtype, split):
    q, kv, lens_d, lens, refs = _dev_case(p, dtype)
    if split == 0:
        assert _fa2_lib.decode_mla_plan(dc.code(dtype), len(lens), *ROWS[p], NMAX).nsplit == 2
    o, lse = mr.mla_c(q, kv, lens_d, split)
    dr.check(o, lse, refs, lens, dc.code(dtype), ("mla", ROWS[p], split))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("page", [64, 128])
def test_paged_is_the_contiguous_call_bit_for_bit(page, dtype):
    """Shuffled pages, NaN in every spare page and behind every unused entry, and one page that two sequences share (a common prefix)."""
    dev = dc.dev()
    H, Nq, lens = 13, 5, [300, 129, 65, 0]
    q, kv = mr.inputs(4, H, Nq, NMAX, lens, dtype, 77)
    kv[1, :page] = kv[0, :page]                                                         # sequences 0 and 1 share their first page
    pool, bt = mr.paged(kv, lens, page, torch.Generator().manual_seed(5))
    pool[bt[1, 0]] = float("nan")
    bt[1, 0] = bt[0, 0]
    refs = mr.refs(q, kv, lens, dc.code(dtype))
    qd, kvd, poold, btd, ld = (t.to(dev) for t in (q, kv, pool, bt, torch.tensor(lens, dtype=torch.int32)))
    for split in (1, 3, 0):
        a = mr.mla_c(qd, kvd, ld, split)
        b = mr.mla_c(qd, poold, ld, split, block_table=btd)
        assert dc.same_bits(a, b), (page, split)
        dr.check(b[0], b[1], refs, lens, dc.code(dtype), ("paged", page, split))
    c = mr.mla_c(qd, poold.unsqueeze(2), ld, 3, block_table=btd)                        # the 4-D form with a head axis of size 1
    assert dc.same_bits(c, mr.mla_c(qd, kvd, ld, 3))


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_strided_views_are_their_compact_twins_and_nothing_around_o_is_written(dtype):
    dev = dc.dev()
    q, kv, lens_d, lens, _ = _dev_case(6, dtype)                                        # 65 rows
    B, Nq, H, _ = q.shape
    wide_kv = torch.full((B, NMAX, 640), float("nan"), dtype=dtype, device=dev)
    wide_kv[:, :, 32:608] = kv
    wide_q = torch.full((B, Nq, H + 2, 584), float("nan"), dtype=dtype, device=dev)
    wide_q[:, :, 1:H + 1, 8:] = q
    for split in (1, 3):
        twin = mr.mla_c(q, kv, lens_d, split)
        frame = torch.full((B, Nq, H + 2, 528), 7.0, dtype=dtype, device=dev)           # o: a window of a larger tensor
        o = frame[:, :, 1:H + 1, 8:520]
        lse = torch.full((B, H, Nq + 3), 7.0, device=dev)[:, :, 1:Nq + 1]
        got = mr.mla_c(wide_q[:, :, 1:H + 1, 8:], wide_kv[:, :, 32:608], lens_d, split, o=o, lse=lse)
        assert torch.equal(got[0].view(torch.int16), twin[0].view(torch.int16)) and torch.equal(got[1], twin[1])
        frame[:, :, 1:H + 1, 8:520] = 7.0
        assert bool((frame == 7.0).all()), "bytes around o were written"
        assert bool((lse._base[:, :, 0] == 7.0).all()) and bool((lse._base[:, :, Nq + 1:] == 7.0).all())
    # the operator on the same views (q is addressable as it is; the cache is never copied)
    o1, l1 = flash_attention_decode_mla(wide_q[:, :, 1:H + 1, 8:], wide_kv[:, :, 32:608], lens_d, return_lse=True, num_splits=3)
    assert torch.equal(o1.view(torch.int16), twin[0].view(torch.int16)) and dr.same_lse(l1 / LN2, twin[1])


# ---------------------------------------------------------------------------------------------------------------- key probes
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_counting_probe_resolves_one_key(dtype):
    """q = 0 and integer cache values in -3 .. 3: every score is 0, so the log2 LSE is log2(count) to 2^-20 — one missed or doubled key among 3 000 moves
    it by 4.8e-4 — and O the mean of the visible rows to one ulp (key_probes' counting bars), under a forced split and the plan's."""
    dev = dc.dev()
    B, H, Nq, nmax, lens = 2, 17, 3, 3200, [3001, 2917]
    g = torch.Generator().manual_seed(11)
    kv = torch.randint(-3, 4, (B, nmax, mr.D), generator=g).to(dtype)
    for b, n in enumerate(lens):
        kv[b, n:] = float("nan")
    q = torch.zeros((B, Nq, H, mr.D), dtype=dtype)
    o_exp, lse_exp, bars = [], [], {}
    for split in (5, 0):
        ns = _fa2_lib.decode_mla_plan(dc.code(dtype), B, H, Nq, nmax, 0, split).nsplit
        assert ns > 1
        tot, tot_abs, cnt = (torch.zeros(B, H, Nq, mr.DV, dtype=torch.float64), torch.zeros(B, H, Nq, mr.DV, dtype=torch.float64),
                             torch.zeros(B, H, Nq, dtype=torch.float64))
        for b, n in enumerate(lens):
            cs = kv[b, :n, :mr.DV].double().cumsum(0)
            ca = kv[b, :n, :mr.DV].double().abs().cumsum(0)
            for i in range(Nq):
                c = n - Nq + i + 1
                tot[b, :, i], tot_abs[b, :, i], cnt[b, :, i] = cs[c - 1], ca[c - 1], c
        o_exp, lse_exp, bar = kp._counting_finish(tot, tot_abs, cnt, dtype, split=True)
        o, lse = mr.mla_c(q.to(dev), kv.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), split)
        fails = kp.check_counting(o.cpu().permute(0, 2, 1, 3), lse.cpu(), o_exp, lse_exp, bar)
        assert not fails, (split, ns, fails)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_pointer_probe_returns_the_named_key(dtype):
    """+-1 cache rows and q_r = c K_pi(r): row r puts all but 2^-16 of its weight on key pi(r) (key_probes.pointer_leaks measures it) and returns that key's
    first 512 columns to one ulp.  The targets are the first and the last key of a tile, of a page and of a part, and each row's own last visible key."""
    dev = dc.dev()
    H, Nq, page, n, split, c = 16, 2, 128, 1500, 4, 4.0
    nmax = 1536
    edges = [0, 31, 32, 63, 127, 128, page * 3 - 1, page * 3]
    for part in range(split):
        first, cnt = _fa2_lib.decode_mla_part_range(n, nmax, split, part)
        assert cnt > 0
        edges += [first * 32, min((first + cnt) * 32, n - Nq + 1) - 1]
    g = torch.Generator().manual_seed(13)
    kv = (torch.randint(0, 2, (1, nmax, mr.D), generator=g) * 2 - 1).to(dtype)
    kv[0, n:] = float("nan")
    pos = torch.arange(Nq)[:, None].expand(Nq, H) + (n - Nq)                           # the position of row (i, h)
    pi = torch.tensor([edges[r % len(edges)] for r in range(Nq * H)]).view(Nq, H)
    pi = torch.where(torch.arange(H)[None, :] == H - 1, pos, torch.minimum(pi, pos))    # the last head: the diagonal
    visible = torch.arange(n)[None, :] <= pos.reshape(-1)[:, None]
    leak, _ = kp.pointer_leaks(kv[:, None, :n], pi.reshape(-1), c, mr.SCALE, visible)
    assert float(leak.max()) <= kp.POINTER_LEAK
    q = (kv[0, pi].float() * c).to(dtype).unsqueeze(0)                                  # [1, Nq, H, 576]
    want = kv[0, pi][..., :mr.DV].double().unsqueeze(0)
    bar = kp.ulp(want, dtype) + 3.0 * leak.view(1, Nq, H, 1)
    pool, bt = mr.paged(kv, [n], page, torch.Generator().manual_seed(3))
    for kw in (dict(), dict(block_table=bt.to(dev))):
        o, _ = mr.mla_c(q.to(dev), (pool if kw else kv).to(dev), torch.tensor([n], dtype=torch.int32, device=dev), split, **kw)
        err = (o.cpu().double() - want).abs()
        assert bool((err <= bar).all()), (bool(kw), float((err / bar).max()))


# ---------------------------------------------------------------------------------------------------------------- other routes to the same numbers
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_against_multi_query_attention_at_head_dim_512(dtype):
    """q[..., 512:] = 0: the call is multi-query attention at head dim 512 with K = V = kv[..., :512] — the packed kernels, bottom-right causal, on the
    gathered keys.  Two kernels that share no code: held to the oracle bars against each other."""
    q, kv, lens_d, lens, _ = _dev_case(4, dtype)                                        # H 16, Nq 3
    dev, code = q.device, dc.code(dtype)
    B, Nq, H, _ = q.shape
    q = q.clone()
    q[..., mr.DV:] = 0
    o, lse = flash_attention_decode_mla(q, kv, lens_d, return_lse=True, num_splits=3)
    keys = torch.cat([kv[b, :n, :mr.DV] for b, n in enumerate(lens)]).unsqueeze(1).contiguous()       # [total_k, 1, 512]
    cu_k = torch.tensor([sum(lens[:b]) for b in range(B + 1)], dtype=torch.int32, device=dev)
    cu_q = torch.arange(0, (B + 1) * Nq, Nq, dtype=torch.int32, device=dev)
    o2, lse2 = flash_attention_varlen(q[..., :mr.DV].reshape(B * Nq, H, mr.DV).contiguous(), keys, keys, cu_q, cu_k, Nq, max(lens), causal=True,
                                      scale=mr.SCALE, bottom_right=True, return_lse=True)
    a, b = o.float().reshape(B * Nq, H, mr.DV), o2.float()
    assert bool(torch.isfinite(a).all()) and bool(((a - b).abs() <= ATOL[code] + RTOL[code] * b.abs()).all()), float((a - b).abs().max())
    assert dr.same_lse(lse.permute(1, 0, 2).reshape(H, B * Nq) / LN2, lse2 / LN2)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_two_halves_merge_to_the_whole(dtype):
    dev = dc.dev()
    lens, half = [300, 257, 512, 100], NMAX // 2                                        # across the cut, one key past it, both halves full, the first half alone
    q, kv = mr.inputs(4, 16, 1, NMAX, lens, dtype, 81)
    refs = mr.refs(q, kv, lens, dc.code(dtype))
    q, kv, lens_d = q.to(dev), kv.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev)
    whole = flash_attention_decode_mla(q, kv, lens_d, return_lse=True)
    a = flash_attention_decode_mla(q, kv[:, :half], lens_d.clamp(max=half), return_lse=True)
    b = flash_attention_decode_mla(q, kv[:, half:], (lens_d - half).clamp(min=0), return_lse=True)
    o, lse = merge_attention([a[0], b[0]], [a[1], b[1]], BNHD_fmt=True)
    code = dc.code(dtype)
    dr.check(o, lse / LN2, refs, lens, code, "merged")
    assert bool(((o.float() - whole[0].float()).abs() <= ATOL[code] + RTOL[code] * whole[0].float().abs()).all()) and dr.same_lse(lse / LN2, whole[1] / LN2)


@pytest.mark.parametrize("split", [3, 0])
def test_graph_replay_follows_lengths_and_block_table_changed_in_place(split):
    dev = dc.dev()
    H, Nq, page, dtype = 16, 2, 64, BF16
    lens_a, lens_b = [300, 65, 33], [129, 0, 512]
    q, kv = mr.inputs(3, H, Nq, NMAX, [NMAX] * 3, dtype, 91)
    g = torch.Generator().manual_seed(9)
    pool, bt_a = mr.paged(kv, [NMAX] * 3, page, g, spare=1)
    perm = torch.randperm(pool.shape[0], generator=g)
    pool_b, bt_b = torch.empty_like(pool), perm[bt_a.long()].to(torch.int32)            # the pages shuffled once more
    pool_b[perm] = pool
    qd, poold = q.to(dev), pool_b.to(dev)
    lens_d, bt_d = torch.tensor(lens_a, dtype=torch.int32, device=dev), bt_b.to(dev)
    flash_attention_decode_mla(qd, poold, lens_d, block_table=bt_d, num_splits=split)   # (warm-up: the library is loaded outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = flash_attention_decode_mla(qd, poold, lens_d, block_table=bt_d, return_lse=True, num_splits=split)
    swapped = bt_b.clone()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]
    for lens, table in ((lens_a, bt_b), (lens_b, bt_b), (lens_b, swapped), (lens_a, bt_b)):
        lens_d.copy_(torch.tensor(lens, dtype=torch.int32))
        bt_d.copy_(table)
        graph.replay()
        torch.cuda.synchronize()
        eager = flash_attention_decode_mla(qd, poold, lens_d, block_table=bt_d, return_lse=True, num_splits=split)
        assert torch.equal(o.view(torch.int16), eager[0].view(torch.int16)) and torch.equal(lse, eager[1]), (split, lens)
    refs = mr.refs(q, kv, lens_a, dc.code(dtype))
    dr.check(o, lse / LN2, refs, lens_a, dc.code(dtype), "replayed")


def test_clamps_behave_as_the_clamped_values():
    """A length above the capacity is the capacity, a negative one 0, a page id outside the pool the clamped id: each call equals the call made with the
    clamped values bit for bit.  (tests/test_decode_mla.py walks the same arithmetic on the CPU, under the sanitizers, over caches sized to the byte.)  The
    pool here is a window of a larger NaN-filled allocation with a page of slack on either side."""
    dev = dc.dev()
    H, Nq, page, dtype, pages, per = 16, 2, 64, F16, 6, 4
    q, kv = mr.inputs(3, H, Nq, per * page, [per * page] * 3, dtype, 93)
    backing = torch.full((pages + 2, page, mr.D), float("nan"), dtype=dtype, device=dev)
    pool = backing[1:pages + 1]
    pool.copy_(torch.randn((pages, page, mr.D), generator=torch.Generator().manual_seed(4)).to(dtype))
    qd, kvd = q.to(dev), kv.to(dev)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)      # noqa: E731
    for split in (1, 3):
        # contiguous: lengths
        got = mr.mla_c(qd, kvd, i32([per * page + 1000, -5, 2 ** 31 - 1]), split)
        assert dc.same_bits(got, mr.mla_c(qd, kvd, i32([per * page, 0, per * page]), split))
        # paged: lengths and page ids
        bt_bad = i32([[0, 5, pages, -1], [2 ** 31 - 1, -2 ** 31, 3, 1], [pages + 7, 2, 2, 0]])
        bt_ok = i32([[0, 5, pages - 1, 0], [pages - 1, 0, 3, 1], [pages - 1, 2, 2, 0]])
        got = mr.mla_c(qd, pool, i32([per * page + 1, 200, -1]), split, block_table=bt_bad)
        assert dc.same_bits(got, mr.mla_c(qd, pool, i32([per * page, 200, 0]), split, block_table=bt_ok))
        assert bool(torch.isfinite(got[0]).all())
    assert bool(torch.isnan(backing[0]).all()) and bool(torch.isnan(backing[-1]).all())


def test_randomised_slice():
    """A seeded slice of 40 cases over dtype, H, Nq, lengths, layout and split, held to the same check."""
    dev = dc.dev()
    rnd = random.Random(2025)
    for case in range(40):
        dtype = rnd.choice([F16, BF16])
        H = rnd.choice([1, 3, 8, 16, 17, 32, 64, 100, 128])
        Nq = rnd.randint(1, min(5, 512 // H))
        B = rnd.randint(1, 3)
        page = rnd.choice([0, 64, 128])
        nmax = rnd.choice([128, 256, 384])
        lens = [rnd.choice([0, 1, rnd.randint(1, nmax), nmax, rnd.choice(LENGTHS)]) for _ in range(B)]
        lens = [min(n, nmax) for n in lens]
        split = rnd.choice([0, 1, 2, 3, 7])
        q, kv = mr.inputs(B, H, Nq, nmax, lens, dtype, 1000 + case)
        refs = mr.refs(q, kv, lens, dc.code(dtype))
        kw = {}
        cache = kv
        if page:
            cache, bt = mr.paged(kv, lens, page, torch.Generator().manual_seed(case))
            kw = dict(block_table=bt.to(dev))
        o, lse = mr.mla_c(q.to(dev), cache.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), split, **kw)
        dr.check(o, lse, refs, lens, dc.code(dtype), ("slice", case, H, Nq, lens, page, split))
