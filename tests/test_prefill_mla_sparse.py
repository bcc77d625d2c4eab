"""CPU tests of sparse MLA attention for packed tokens (include/fa2_gfx950.h: fa2_fwd_prefill_mla_sparse, and its e4m3 twin).
Nothing here touches a device."""
import pytest
import torch

import decode_calls as dc
from rocwmma_fattn import FlashAttn, _fa2_lib
from test_decode_mla import ALIGN, DTYPE, F16, GRID, HEAD_DIM, HEADER, NULLP, OK, SCALE, SHAPE

P, S2, S3 = dc.HOST, _fa2_lib.strides2, _fa2_lib.strides3
ENTRIES = ("fa2_fwd_prefill_mla_sparse", "fa2_fwd_prefill_mla_sparse_fp8")


def test_symbols_are_declared_exported_and_bound():
    lib, text = _fa2_lib.load(), open(HEADER).read()
    for name, nargs in ((ENTRIES[0], 26), (ENTRIES[1], 26)):
        assert name + "(" in text and len(_fa2_lib.SYMBOLS[name][1]) == nargs and getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1], name
    assert "flash_attention_prefill_mla" in FlashAttn.__all__


@pytest.mark.parametrize("fp8", [False, True])
def test_c_codes_in_the_documented_order(fp8):
    row = 656 if fp8 else 576
    ok = dict(dtype=F16, q=P, k=P, o=P, lse=P, idx=P, cu=P, lens=P, bt=None, B=2, H=16, total=0, D=576, Dv=512, topk=64, cap=256, page=0, pages=0,
              qs=S2(16 * 576, 576), ks=S3(256 * row, row, row), os=S2(16 * 512, 512), ls=64, is_=64, bts=0, scale=0.04, stream=None)
    rc = lambda **kw: getattr(_fa2_lib.load(), ENTRIES[fp8])(*dict(ok, **kw).values())      # noqa: E731
    bad_ks, nan = S3(256 * row, row, row + 4), float("nan")
    assert rc() == OK and rc(total=2 ** 40) == GRID and rc(total=2 ** 30, H=128) == GRID      # total_q == 0 passes every check; the grid is the last
    for kw in (dict(idx=None), dict(cu=None), dict(q=None), dict(page=64), dict(cu=None, topk=0, D=512, ks=bad_ks, dtype=2)):
        assert rc(**kw) == NULLP, kw
    for kw in (dict(topk=0), dict(total=-1), dict(H=129), dict(B=0), dict(page=32, bt=P), dict(topk=2 ** 31 - 64), dict(topk=0, D=512, ks=bad_ks, dtype=2)):
        assert rc(**kw) == SHAPE, kw
    assert rc(D=512, ls=-1) == HEAD_DIM and rc(Dv=576, idx=P + 2, dtype=2) == HEAD_DIM
    for kw in (dict(ls=-1), dict(is_=-1), dict(page=64, bt=P, pages=0), dict(is_=-1, idx=P + 2, dtype=2)):
        assert rc(**kw) == SHAPE, kw
    assert rc(ks=S3(256 * row, row, 8)) == (SHAPE if fp8 else OK) and rc(ks=bad_ks) == (SHAPE if fp8 else ALIGN)
    for kw in (dict(idx=P + 2), dict(cu=P + 1), dict(q=P + 8), dict(qs=S2(16 * 576, 580)), dict(os=S2(-512, 512)), dict(ks=S3(256 * row + 4, row, row)),
               dict(cu=P + 2, dtype=2, scale=nan)):
        assert rc(**kw) == ALIGN, kw
    assert rc(idx=P + 4, cu=P + 4) == OK and rc(dtype=2, scale=nan, total=2 ** 40) == DTYPE and rc(scale=nan, total=2 ** 40) == SCALE


def test_python_argument_checks():
    f = FlashAttn.flash_attention_prefill_mla
    q, kv, lens = torch.zeros(6, 16, 576, dtype=torch.float16), torch.zeros(2, 128, 576, dtype=torch.float16), torch.full((2,), 5, dtype=torch.int32)
    cu, good = torch.tensor([0, 2, 6], dtype=torch.int32), torch.zeros(6, 8, dtype=torch.int32)
    for bad in (good.long(), good.float(), good[:5], good[None], good[0], good[:, :0], good[:, ::2], good.t().contiguous().t(), good.tolist(), None):
        with pytest.raises(ValueError, match="indices"):
            f(q, kv, cu, lens, bad)
    with pytest.raises(ValueError, match="1 .. 128 heads"):
        f(torch.zeros(6, 129, 576, dtype=torch.float16), kv, cu, lens, good)
    with pytest.raises(ValueError, match="latent rows of 576 columns"):
        f(q, torch.zeros(2, 128, 656, dtype=torch.int8), cu, lens, good)                # 656-byte rows are uint8 / float8_e4m3fn
    with pytest.raises(ValueError, match="rows of 656 bytes"):
        f(q, torch.zeros(2, 128, 576, dtype=torch.uint8), cu, lens, good)
    with pytest.raises(ValueError, match="inference only"):
        f(q.clone().requires_grad_(True), kv, cu, lens, good)
    with pytest.raises(ValueError, match="cu_seqlens_q"):
        f(q, kv, cu.long(), lens, good)
    with pytest.raises(ValueError, match="cache_seqlens"):
        f(q, kv, cu, lens[:1], good)
