"""CPU test of the call layer (tests/decode_calls.py over tools/decode_abi.py): the argument tuple it builds for each of the four entries has the length
the bindings declare and converts under their argtypes.  A tuple that drifted from the C signature would otherwise show up only as a wrong pointer on the GPU."""
import pytest

import decode_calls as dc
from rocwmma_fattn import _fa2_lib

NULLP = -1


@pytest.mark.parametrize("entry", list(dc.ENTRIES))
def test_the_tuple_of_every_entry_matches_its_binding(entry):
    symbol, order, _ = dc.ENTRIES[entry]
    P = dc.HOST
    kw = dict.fromkeys(order, 0)                                        # every size 0, every pointer HOST, every stride set three / two zeros
    kw.update({n: P for n in ("q", "k", "v", "o", "lse", "lens", "bt", "kd", "vd", "sl", "ws", "kn", "vn", "qo", "cos", "sin") if n in order})
    kw.update({n: _fa2_lib.strides3(0, 0, 0) for n in ("qs", "ks", "vs", "os", "kns", "vns", "qos") if n in order})
    kw.update({n: _fa2_lib.strides2(0, 0) for n in ("ls", "ds") if n in order})
    kw.update(scale=0.0, cap_=0.0, stream=None)
    kw = {n: kw[n] for n in order}
    args = dc.c_args(entry, **kw)
    assert len(args) == len(order) == len(_fa2_lib.SYMBOLS[symbol][1])
    assert dc.call(entry, **dict(kw, q=None)) == NULLP                  # (a ctypes.ArgumentError would mean a value in the wrong place)
    # a keyword of another entry is refused unless it holds the value this entry computes with
    if entry == "plain":
        assert dc.c_args(entry, **kw, kd=None, wl=-1, fmt=_fa2_lib.FA2_CACHE_16BIT) == args
        for extra in (dict(kd=P), dict(wl=5), dict(fmt=_fa2_lib.FA2_CACHE_E4M3)):
            with pytest.raises(AssertionError):
                dc.c_args(entry, **kw, **extra)
