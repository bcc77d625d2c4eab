"""Packed attention with V narrower than K on the GPU: fa2_fwd_varlen_dv and flash_attention_varlen(q, k, v [total_k, Hkv, Dv != D]).

The reference is tests/test_varlen_gpu.py's: the repository's oracle per sequence (fa2_oracle.fwd_c, the same contract-0 arithmetic, and dense float64) —
on V zero-padded to D with O sliced to Dv, which is exact in the oracle's arithmetic (the padded columns of O are sums of zeros).  Tolerances are
tests/conftest.py's ATOL / RTOL / LSE_TOL and 2 * FLOOR against float64.  With the same `rows` the call must also equal fa2_fwd_varlen on the padded V bit
for bit: same row maxima, same rescale decisions, and the k-steps and the column slab it skips only ever multiplied zeros.  The single-key inputs and
their bars are tests/key_probes.py's (v cut to Dv columns), the merge bar tests/test_merge_gpu.py's for a two-part merge."""
import ctypes

import pytest
import torch

import key_probes as kp
import lse_refs as R
from conftest import LSE_TOL
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention_varlen, merge_attention
from test_varlen_gpu import BR, CAUSAL, VARIANTS, _check_forward, _code, _cu, _dev, _fwd_varlen, _rand, _s2, _stream

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
LN2 = R.LN2
# (q lengths, k lengths): every length around the 64-key tile and the 128- / 256-row blocks, an empty sequence on either side, fewer keys than queries
LENSETS = {
    "self": ((1, 63, 64, 65, 257, 0, 130), (1, 63, 64, 65, 257, 0, 130)),
    "cross": ((65, 0, 257, 1, 130), (300, 64, 0, 65, 100)),
}


def _fwd_dv(q, k, v, cu_q, cu_k, max_q, max_k, flags, left, right, o=None, lse=None, Dv=None, check=True):
    """fa2_fwd_varlen_dv on packed tensors; outputs pre-filled with NaN (every element of o[:, :, :Dv] and lse below cu[B] must be written)."""
    lib = _fa2_lib.load()
    H, D = q.shape[1], q.shape[2]
    o = torch.full((q.shape[0], H, v.shape[2]), float("nan"), dtype=q.dtype, device=q.device) if o is None else o
    Dv = v.shape[2] if Dv is None else Dv             # (a refusal test states another width than v's)
    lse = torch.full((H, q.shape[0]), float("nan"), dtype=torch.float32, device=q.device) if lse is None else lse
    rc = lib.fa2_fwd_varlen_dv(_code(q.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu_q.numel() - 1, H, k.shape[1], max_q, max_k,
                               D, Dv, cu_q.data_ptr(), cu_k.data_ptr(), _s2(q), _s2(k), _s2(v), _s2(o), lse.stride(0), D ** -0.5, flags, left, right, _stream())
    torch.cuda.synchronize()
    if check:
        _fa2_lib.check(rc)
        return o, lse
    return rc, o, lse


def _pad(t, D):
    return torch.nn.functional.pad(t, (0, D - t.shape[-1]))


def _dv_plan(dt, B, H, Hkv, mq, mk, D, Dv, flags, left, right):
    plan = _fa2_lib.FwdPlan()
    _fa2_lib.check(_fa2_lib.load().fa2_fwd_varlen_dv_plan(_code(dt), B, H, Hkv, mq, mk, D, Dv, None, None, D ** -0.5, flags, left, right, ctypes.byref(plan)))
    return plan


def _parity(D, Dv, H, Hkv, dt, variants):
    """Both length sets, both `rows` options: the oracle and float64 per sequence, NaN-prefilled outputs fully written, and the padded route's bits."""
    dev = _dev()
    for (lname, (lq, lk)), vname in [(a, b) for a in LENSETS.items() for b in variants]:
        flags, left, right = VARIANTS[vname]
        g = torch.Generator(device="cpu").manual_seed(D + Dv + H + len(vname) + 7 * len(lname))
        q, k, v = _rand((sum(lq), H, D), dt, g), _rand((sum(lk), Hkv, D), dt, g), _rand((sum(lk), Hkv, Dv), dt, g)
        vp = _pad(v, D)
        qd, kd, vd, vpd = q.to(dev), k.to(dev), v.to(dev), vp.to(dev)
        cq, ck = _cu(lq, dev), _cu(lk, dev)
        for rows in (128, 256):
            tag = "D%d/%d H%d/%d %s %s rows %d" % (D, Dv, H, Hkv, lname, vname, rows)
            with _fa2_lib.options(rows=rows):
                pl = _dv_plan(dt, len(lq), H, Hkv, max(lq), max(lk), D, Dv, flags, left, right)
                assert pl.kernel == _fa2_lib.FA2_KERNEL_HIP_VARLEN_DV and pl.contract == 0 and pl.rows == rows and pl.heads_main == len(lq) * H, pl.as_dict()
                o, lse = _fwd_dv(qd, kd, vd, cq, ck, max(lq), max(lk), flags, left, right)
                o_pad, lse_pad = _fwd_varlen(qd, kd, vpd, cq, ck, max(lq), max(lk), flags, left, right)
            assert o.shape == (sum(lq), H, Dv)
            # the padded route, same rows: bit for bit
            assert torch.equal(o, o_pad[..., :Dv]) and torch.equal(lse, lse_pad), (tag, "not the padded route's bits",
                                                                                   (o.float() - o_pad[..., :Dv].float()).abs().max().item())
            assert (o_pad[..., Dv:] == 0).all(), (tag, "the padded route's own padding")
            # the oracle on V zero-padded to D, O sliced: the columns at and beyond Dv are sums of zeros on both sides
            _check_forward(_pad(o, D), lse, q, k, vp, lq, lk, flags, left, right, dt, tag)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (2, 2)])
def test_forward_192_128_against_oracle_float64_and_the_padded_route(H, Hkv, dt):
    _parity(192, 128, H, Hkv, dt, ("plain", "causal", "causal_br", "left", "band_br"))


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D,Dv", [(256, 128), (192, 64), (136, 72)])
def test_forward_other_pairs_causal(D, Dv, dt):
    """16 k-steps (D above 192); two O column blocks; a D that ends inside a k-step with a Dv that ends inside a column block."""
    for H, Hkv in ((4, 2), (2, 2)):
        _parity(D, Dv, H, Hkv, dt, ("causal",))


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_v_is_a_slice_of_the_up_projection_and_o_a_slice_of_a_wider_buffer(dt):
    """V = kv_up[..., 128:256] of a [total_k, Hkv, 256] tensor whose other columns are NaN; O a column slice of a buffer poisoned with a bit pattern:
    the results are those of contiguous tensors, and every byte outside o[:, :, :Dv] keeps the poison."""
    dev = _dev()
    H, Hkv, D, Dv = 4, 2, 192, 128
    lq, lk = LENSETS["cross"]
    cq, ck = _cu(lq, dev), _cu(lk, dev)
    g = torch.Generator(device="cpu").manual_seed(31)
    q, k, v = (_rand(s, dt, g).to(dev) for s in ((sum(lq), H, D), (sum(lk), Hkv, D), (sum(lk), Hkv, Dv)))
    kv_up = torch.full((sum(lk), Hkv, 256), float("nan"), dtype=dt, device=dev)
    kv_up[..., 128:256] = v
    v_slice = kv_up[..., 128:256]
    assert v_slice.stride() == (Hkv * 256, 256, 1)
    poison = 0x7B7B if dt == torch.float16 else 0x7F7B        # (finite in fp16; any pattern will do: it is compared as bits)
    for flags, left, right in (VARIANTS["causal_br"], VARIANTS["plain"]):
        for rows in (128, 256):
            with _fa2_lib.options(rows=rows):
                want_o, want_l = _fwd_dv(q, k, v, cq, ck, max(lq), max(lk), flags, left, right)
                rows_extra = 3                                    # rows at and beyond cu[B] are not written either
                buf = torch.full((sum(lq) + rows_extra, H, 192), poison, dtype=torch.int16, device=dev)
                o_view = buf.view(dt)[:sum(lq), :, 32:32 + Dv]
                lse = torch.full((H, sum(lq) + rows_extra), float("nan"), dtype=torch.float32, device=dev)
                _fwd_dv(q, k, v_slice, cq, ck, max(lq), max(lk), flags, left, right, o=o_view, lse=lse)
            assert torch.equal(o_view, want_o) and torch.equal(lse[:, :sum(lq)], want_l), (flags, rows)
            assert torch.isnan(lse[:, sum(lq):]).all()
            keep = torch.ones(buf.shape, dtype=torch.bool, device=dev)
            keep[:sum(lq), :, 32:32 + Dv] = False
            assert (buf[keep] == poison).all(), (flags, rows, "bytes outside o[:, :, :Dv] were written")
    # the operator reads the slice in place and returns the same bits
    with torch.no_grad():
        got = flash_attention_varlen(q, k, v_slice, cq, ck, max(lq), max(lk), causal=True, bottom_right=True)
        want = flash_attention_varlen(q, k, v, cq, ck, causal=True, bottom_right=True)                    # the maxima computed from the tensors
    assert got.shape == (sum(lq), H, Dv) and torch.equal(got, want) and torch.isfinite(got).all()


# ---------------------------------------------------------------------------------------------------------------- single-key resolution
PROBE_LENS = (300, 65)


@pytest.mark.parametrize("align", ["full", "top_left", "bottom_right"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_counting_inputs_count_every_rows_keys(align, dt):
    """K = 0, integer V: the log2 LSE is log2 of the visible key count to 2^-20 and O the exact mean of the visible v, rounded once (1 ulp)."""
    dev = _dev()
    H, Hkv, D, Dv = 4, 2, 192, 128
    lq = lk = PROBE_LENS
    cq = _cu(lq, dev)
    q4, k4, v4 = kp.counting_inputs(1, H, Hkv, sum(lq), sum(lk), D, dt, seed=211, device=dev)
    v4 = v4[..., :Dv].contiguous()
    q, k, v = (t[0].transpose(0, 1).contiguous() for t in (q4, k4, v4))
    flags = {"full": 0, "top_left": CAUSAL, "bottom_right": CAUSAL | BR}[align]
    fails = []
    for rows in (128, 256):
        with _fa2_lib.options(rows=rows):
            o, lse = _fwd_dv(q, k, v, cq, cq, max(lq), max(lk), flags, -1, -1)
        q0 = 0
        for n in lq:
            lo, hi = kp.row_ranges(n, n, causal=align != "full", bottom_right=align == "bottom_right", device=dev)
            exp = kp.counting_expect(v4[:, :, q0:q0 + n], lo, hi, H, dt)
            fails += ["rows %d, %d x %d: %s" % (rows, n, n, f) for f in kp.check_counting(o[q0:q0 + n].transpose(0, 1)[None], lse[None, :, q0:q0 + n], *exp)]
            q0 += n
    assert fails == [], fails


@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_pointer_inputs_return_the_one_key_each_row_points_at(causal, dt):
    """+-1 keys, Q_i = c K_pi(i): row i returns v_pi(i) to one ulp (plus the builder's measured leak), whatever the other 299 keys hold."""
    dev = _dev()
    H, Hkv, D, Dv = 4, 2, 192, 128
    parts = []
    for s, n in enumerate(PROBE_LENS):
        pi = kp.pointer_map("perm_causal" if causal else "perm", n, n, seed=40 + s)
        vis = None
        if causal:
            lo, hi = kp.row_ranges(n, n, causal=True)
            j = torch.arange(n)[None, :]
            vis = (j >= lo[:, None]) & (j < hi[:, None])
        inp = kp.pointer_inputs(1, H, Hkv, n, n, D, dt, pi, seed=50 + s, device=dev, visible=vis)
        inp["v"] = inp["v"][..., :Dv].contiguous()
        parts.append(inp)
    q, k, v = (torch.cat([p[name][0].transpose(0, 1) for p in parts], 0).contiguous() for name in ("q", "k", "v"))
    cq = _cu(PROBE_LENS, dev)
    fails = []
    for rows in (128, 256):
        with _fa2_lib.options(rows=rows):
            o, lse = _fwd_dv(q, k, v, cq, cq, max(PROBE_LENS), max(PROBE_LENS), CAUSAL if causal else 0, -1, -1)
        q0 = 0
        for n, inp in zip(PROBE_LENS, parts):
            want, bar = kp.pointer_expect_o(inp, dt)
            got = o[q0:q0 + n].transpose(0, 1)[None].double()
            bad = ~((got - want).abs() <= bar)
            if bool(bad.any()):
                fails.append("rows %d, %d keys: %d elements off, worst %.1f bars" % (rows, n, int(bad.sum()), float(((got - want).abs() / bar).max())))
            lse_want, lse_bar = kp.pointer_expect_lse(inp, dt), kp.pointer_lse_bar(inp, dt, False)
            lerr = float((lse[:, q0:q0 + n].double() - lse_want).abs().max())
            if not lerr <= lse_bar:
                fails.append("rows %d, %d keys: LSE off by %.3e (bar %.3e)" % (rows, n, lerr, lse_bar))
            q0 += n
    assert fails == [], fails


# ---------------------------------------------------------------------------------------------------------------- the use the call is for
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_chunked_context_merges_to_the_one_bottom_right_causal_call(dt):
    """130 cached + 70 new tokens, and 0 cached + 65 new: pass A (new queries, cached keys, non-causal) merged with pass B (new queries, new keys,
    causal) equals one bottom-right-causal call over the concatenated keys — within test_merge_gpu's bar for a two-part merge (one rounding of the I/O
    dtype at the largest magnitude, twice), the LSE within LSE_TOL in log2 units.  The sequence without cached keys is pass B alone."""
    dev = _dev()
    H, Hkv, D, Dv = 4, 2, 192, 128
    cached, new = (130, 0), (70, 65)
    g = torch.Generator(device="cpu").manual_seed(77)
    q = _rand((sum(new), H, D), dt, g).to(dev)
    k_ctx, v_ctx = _rand((sum(cached), Hkv, D), dt, g).to(dev), _rand((sum(cached), Hkv, Dv), dt, g).to(dev)
    k_new, v_new = _rand((sum(new), Hkv, D), dt, g).to(dev), _rand((sum(new), Hkv, Dv), dt, g).to(dev)
    cu_new, cu_ctx = _cu(new, dev), _cu(cached, dev)
    with torch.no_grad():
        oa, la = flash_attention_varlen(q, k_ctx, v_ctx, cu_new, cu_ctx, max(new), max(cached), return_lse=True)
        ob, lb = flash_attention_varlen(q, k_new, v_new, cu_new, cu_new, max(new), max(new), causal=True, return_lse=True)
        om, lm = merge_attention([oa, ob], [la, lb])
        k_all = torch.cat([k_ctx[:130], k_new[:70], k_new[70:]], 0)
        v_all = torch.cat([v_ctx[:130], v_new[:70], v_new[70:]], 0)
        total = tuple(c + n for c, n in zip(cached, new))
        of, lf = flash_attention_varlen(q, k_all, v_all, cu_new, _cu(total, dev), max(new), max(total), causal=True, bottom_right=True, return_lse=True)
    torch.cuda.synchronize()
    assert oa.shape == ob.shape == om.shape == of.shape == (sum(new), H, Dv) and la.shape == (H, sum(new))
    # no cached keys: pass A's rows are zeros with lse -inf, and the merge is pass B
    assert (oa[70:] == 0).all() and torch.isneginf(la[:, 70:]).all()
    assert torch.equal(om[70:], ob[70:]) and torch.equal(lm[:, 70:], lb[:, 70:])
    assert torch.isfinite(om).all() and torch.isfinite(lm).all()
    bar_o = 2 * R.MERGE_EPS[dt] * max(1.0, of.float().abs().max().item())
    err_o = (om.float() - of.float()).abs().max().item()
    err_l = ((lm.double() - lf.double()) / LN2).abs().max().item()
    print("chunked context %s: O err %.3g (bar %.3g), lse err %.3g log2 units (bar %.3g)" % (str(dt)[6:], err_o, bar_o, err_l, LSE_TOL))
    assert err_o <= bar_o and err_l <= LSE_TOL


def test_call_replays_from_a_graph_after_the_lengths_change_in_place():
    """Captured once with the maxima passed (no synchronisation inside), replayed after cu_seqlens_q / cu_seqlens_k changed in place."""
    dev = _dev()
    dt, H, Hkv, D, Dv = torch.bfloat16, 4, 2, 192, 128
    first, second = ((100, 60, 140), (100, 200, 0)), ((1, 299, 0), (150, 20, 130))
    g = torch.Generator(device="cpu").manual_seed(91)
    q, k, v = (_rand(s, dt, g).to(dev) for s in ((300, H, D), (300, Hkv, D), (300, Hkv, Dv)))
    cq, ck = _cu(first[0], dev), _cu(first[1], dev)
    kw = dict(max_seqlen_q=300, max_seqlen_k=300, causal=True, bottom_right=True, return_lse=True)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            flash_attention_varlen(q, k, v, cq, ck, **kw)                   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            go, gl = flash_attention_varlen(q, k, v, cq, ck, **kw)
        for lens in (first, second):
            cq.copy_(_cu(lens[0], dev))
            ck.copy_(_cu(lens[1], dev))
            go.zero_()
            gl.zero_()
            graph.replay()
            torch.cuda.synchronize()
            eo, el = flash_attention_varlen(q, k, v, cq, ck, **kw)
            torch.cuda.synchronize()
            assert torch.equal(go, eo) and torch.equal(gl, el), lens
            assert torch.isfinite(go).all()


def test_refusals_on_device_tensors_leave_o_untouched():
    dev = _dev()
    dt, H, Hkv, D, Dv = torch.float16, 4, 2, 192, 128
    lq = lk = (70, 0, 130)
    cu = _cu(lq, dev)
    g = torch.Generator(device="cpu").manual_seed(13)
    q, k, v = (_rand(s, dt, g).to(dev) for s in ((200, H, D), (200, Hkv, D), (200, Hkv, Dv)))
    codes = {"shape": -2, "head_dim": -3, "alignment": -4, "scale": -6}
    wide = torch.zeros((200, Hkv, Dv + 8), dtype=dt, device=dev)
    cases = (
        (dict(Dv=100), "head_dim"), (dict(Dv=136), "head_dim"), (dict(Dv=0), "shape"), (dict(flags=8), "shape"), (dict(left=-2), "shape"),
        (dict(v=wide[..., 4:4 + Dv]), "alignment"),                       # a slice that starts 8 bytes into a row
        (dict(v=torch.zeros((200, Hkv, Dv + 4), dtype=dt, device=dev)[..., :Dv]), "alignment"),      # a row pitch that is no multiple of 8 elements
        (dict(q=q[..., :128]), "head_dim"),                               # D = 128 with Dv = 128: no served pair
    )
    for kw, want in cases:
        args = dict(q=q, k=k, v=v, flags=0, left=-1, right=-1, Dv=None)
        args.update(kw)
        if args["q"].shape[2] != D:
            args["k"] = k[..., :args["q"].shape[2]]
        rc, o, lse = _fwd_dv(args["q"], args["k"], args["v"], cu, cu, max(lq), max(lk), args["flags"], args["left"], args["right"], Dv=args["Dv"], check=False)
        assert rc == codes[want], (kw.keys(), rc)
        assert torch.isnan(o).all() and torch.isnan(lse).all(), (kw.keys(), "a refused call wrote its outputs")
    # the operator refuses before any device work
    for kw, vv, words in ((dict(dropout_p=0.1), v, "dropout_p"), (dict(softcap=20.0), v, "softcap"), (dict(alibi_slopes=torch.ones(H, device=dev)), v, "alibi"),
                          (dict(), torch.zeros((200, Hkv, 100), dtype=dt, device=dev), "136 .. 256")):
        with pytest.raises(ValueError, match="fa2: .*" + words):
            flash_attention_varlen(q, k, vv, cu, cu, **kw)
    with pytest.raises(ValueError, match="fa2: .*forward only"):
        flash_attention_varlen(q.clone().requires_grad_(True), k, v, cu, cu)
    with pytest.raises(RuntimeError, match="fa2: inconsistent"):
        flash_attention_varlen(q, k, v[:199], cu, cu)
