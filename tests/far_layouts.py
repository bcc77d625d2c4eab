"""Layouts and the checker of the far-offset tests (tests/test_far_offsets.py on the CPU, tests/test_far_offsets_gpu.py on the GPU).

Every kernel forms an address from a 64-bit base (pointer + b * stride[0] + h * stride[1], packed calls + cu_seqlens[s] * row pitch) and 32-bit per-lane
byte offsets.  The tests place the tensors of a call as strided views into ONE poisoned byte buffer ("arena"), so that batch, head or row strides carry
slices past byte offsets 2^31 and 2^32, run the call, copy the views out, poison them again and require the whole arena to be poison once more.  Pairs
and quads of 0xFF bytes are NaN in fp16, bf16 and f32: a read outside the views poisons its result, a write outside them stays in the arena.

This module is plain geometry and comparisons, independent of the device: the CPU test builds the same layouts on device "meta" to prove that they
cross what they claim, and feeds the checker mutants on small tensors.

Case tables: DENSE_CASES, SPAN_CASES, BIAS_SPAN_CASES, PACKED_CASES, F32_CASES (dense, windowed, dropout, biased, packed calls), SCOREMOD_CASES
(score modifiers: slopes with a far batch stride), LSE_CASES (a dlse slot with strides of its own), MERGE_CASES (parts of one far stride set),
DECODE_CASES (16-bit and e4m3 caches: far batches, far heads, a wide key row pitch, paged pools)."""
import numpy as np
import torch

MIB = 1 << 20
GIB = 1 << 30
ARENA_BYTES = 4 * GIB + 256 * MIB
ARENA_F32_BYTES = 8 * GIB + 256 * MIB        # f32 tensors at an ELEMENT index past 2^31
POISON = 0xFF
# Slices of a far placement sit at c, FAR_STEP + c and 2 * FAR_STEP + c (c: a few KiB per tensor of the case): the second crosses byte offset 2^31 by
# 12 KiB + c, the third 2^32 by 24 KiB + c — neither by a round number
FAR_STEP = (1 << 31) + 3 * 4096
# The documented span rule (include/fa2_gfx950.h): ((n - 1) * pitch + D) * 2 bytes of one head's n rows, plus 64 further rows of that pitch, fit 2^31 - 1
SPAN_LIMIT = (1 << 31) - 1
SPAN_SLACK_ROWS = 64


def span_bytes(n, pitch, D, esize=2):
    """Bytes one head's matrix of n rows spans: from its first element to the end of its last row."""
    return ((n - 1) * pitch + D) * esize


def last_pitch(n, D, limit=SPAN_LIMIT, slack=SPAN_SLACK_ROWS, esize=2):
    """The largest row pitch (elements, a multiple of 8) whose n-row span plus `slack` rows still fits `limit` bytes."""
    return (limit // esize - D) // (n - 1 + slack) // 8 * 8


def _up(x, a):
    return -(-x // a) * a


class Slot:
    """One tensor of a case: dtype, shape, element strides and the byte offset of its first element in the arena.  The last dimension is contiguous."""

    def __init__(self, name, dtype, shape, strides, offset, kind=None):
        self.name, self.dtype, self.shape, self.strides, self.offset = name, dtype, tuple(shape), tuple(strides), int(offset)
        self.kind = kind or ("dense" if len(self.shape) == 4 else "flat")          # "packed": [total, H, D] with strides {row, head, 1}
        self.esize = torch.empty((), dtype=dtype).element_size()
        assert self.strides[-1] == 1 and self.offset % self.esize == 0 and len(self.shape) == len(self.strides)

    def view(self, arena):
        return torch.as_strided(arena.view(self.dtype), self.shape, self.strides, self.offset // self.esize)

    def bytes_view(self, arena):
        """The same bytes as uint8 (to poison them again)."""
        return torch.as_strided(arena, self.shape[:-1] + (self.shape[-1] * self.esize,), tuple(s * self.esize for s in self.strides[:-1]) + (1,), self.offset)

    def row_bytes(self):
        return self.shape[-1] * self.esize

    def row_starts(self):
        """Byte offset of every row (all leading indices), as an int64 array of the leading shape."""
        at = np.full(self.shape[:-1], self.offset, dtype=np.int64)
        for d, (n, s) in enumerate(zip(self.shape[:-1], self.strides[:-1])):
            idx = np.arange(n, dtype=np.int64) * (s * self.esize)
            at = at + idx.reshape([-1 if i == d else 1 for i in range(len(self.shape) - 1)])
        return at

    def slice_range(self, dim, i):
        """(first byte, one past the last byte) of the slice with index i along dimension dim."""
        at = np.take(self.row_starts(), i, axis=dim)
        return int(at.min()), int(at.max()) + self.row_bytes()

    def extent(self):
        at = self.row_starts()
        return int(at.min()), int(at.max()) + self.row_bytes()


def validate(slots, arena_bytes):
    """Every row of every slot lies inside the arena and no two rows (of one slot or of two) share a byte.  -> bytes covered."""
    starts = np.concatenate([s.row_starts().reshape(-1) for s in slots])
    ends = np.concatenate([s.row_starts().reshape(-1) + s.row_bytes() for s in slots])
    assert starts.min() >= 0 and ends.max() <= arena_bytes, (int(starts.min()), int(ends.max()), arena_bytes)
    order = np.argsort(starts, kind="stable")
    assert (starts[order][1:] >= ends[order][:-1]).all(), "two views overlap"
    return int((ends - starts).sum())


def head_step(H, step=FAR_STEP):
    """Head stride in bytes that carries the last of H heads past 2 * step (H = 3: step itself)."""
    return step if H <= 3 else _up(2 * step // (H - 1) + 1, 4096)


def place(specs, far, step=FAR_STEP, start=0, gap=4096):
    """Slots of the tensors `specs` = [(name, dtype, shape, pitch)]: shape [B, H, N, D] with a row pitch in elements, or [B, H, N] (LSE, delta: rows of
    floats).  far = "batch": the batch stride is `step` bytes; "head": the head stride is head_step(H) bytes (B = 1); None: contiguous batches and heads.
    A spec may carry its own `far` as a fifth entry.  Heads inside a far batch, rows inside a head are contiguous; the tensors follow one another
    `gap` bytes and a stagger apart (poison between them) from byte `start` on."""
    slots, cur = {}, start
    for spec in specs:
        name, dtype, shape, pitch = spec[:4]
        how = spec[4] if len(spec) > 4 else far
        es = torch.empty((), dtype=dtype).element_size()
        B, H, N = shape[:3]
        inner = N * pitch if len(shape) == 4 else N                  # elements of one head
        tail = (pitch, 1) if len(shape) == 4 else (1,)
        if how == "batch":
            assert step % es == 0
            strides, used = (step // es, inner) + tail, H * inner * es
        elif how == "head":
            hs = head_step(H, step)
            assert B == 1 and hs % es == 0 and inner * es <= hs
            strides, used = (H * hs // es, hs // es) + tail, inner * es
        else:
            strides, used = (H * inner, inner) + tail, B * H * inner * es
        slots[name] = Slot(name, dtype, shape, strides, cur)
        cur += _up(used, 4096) + gap + 1040                         # (staggered: no slice lands on a round offset)
    return slots


def place_bnhd(specs, step=FAR_STEP, start=0, gap=4096):
    """Far batches of [N, H, D] memory — the heads of a row side by side: shape [B, H, N, D] with strides {step, D, H * D, 1} (include/fa2_gfx950.h: the
    reference's BNHD layout).  specs = [(name, dtype, shape [B, H, N, D])]."""
    slots, cur = {}, start
    for name, dtype, shape in specs:
        es = torch.empty((), dtype=dtype).element_size()
        B, H, N, D = shape
        assert step % es == 0 and N * H * D * es <= step
        slots[name] = Slot(name, dtype, shape, (step // es, D, H * D, 1), cur)
        cur += _up(N * H * D * es, 4096) + gap + 1040
    return slots


def place_rows(specs, pitch_bytes, start=0, gap=64):
    """Slots that share one row pitch and interleave inside it: specs = [(name, dtype, shape [N, H, D] or [1, 1, N, D])]; tensor t's row r starts at
    byte start + r * pitch_bytes + its column offset.  The packed row-far layout and the span cases, whose pitch leaves room for nothing else."""
    slots, col = {}, start
    for name, dtype, shape in specs:
        es = torch.empty((), dtype=dtype).element_size()
        assert pitch_bytes % es == 0
        if len(shape) == 3:                                          # packed [total, H, D]: strides {row, head, 1}
            strides, width = (pitch_bytes // es, shape[2], 1), shape[1] * shape[2] * es
        else:                                                        # [1, 1, N, D]
            strides, width = (shape[2] * pitch_bytes // es, shape[2] * pitch_bytes // es, pitch_bytes // es, 1), shape[3] * es
        slots[name] = Slot(name, dtype, shape, strides, col, "packed" if len(shape) == 3 else "dense")
        col += _up(width, 16) + gap
    assert col - start <= pitch_bytes, "the interleaved columns do not fit one row pitch"
    return slots


def twin_of(slots, keep_pitch=True):
    """The compact twin of a case: same shapes, same row pitches (unless keep_pitch is False: rows contiguous), batch and head strides contiguous,
    in a small buffer of its own.  -> (slots, bytes)."""
    out, cur = {}, 0
    for name, s in slots.items():
        if len(s.shape) == 4:
            B, H, N, D = s.shape
            pitch = s.strides[2] if keep_pitch else D
            strides = (H * N * pitch, N * pitch, pitch, 1)
            used = B * H * N * pitch
        elif s.kind == "packed":                                     # [total, H, D]
            T, H, D = s.shape
            pitch = s.strides[0] if keep_pitch else H * D
            strides, used = (pitch, D, 1), T * pitch
        else:                                                        # [B, H, N] rows of floats, [H, total], or a flat buffer
            strides, used = [1], 1
            for n in reversed(s.shape[1:]):
                strides.insert(0, strides[0] * n)
            strides, used = tuple(strides), int(np.prod(s.shape))
        out[name] = Slot(name, s.dtype, s.shape, strides, cur, s.kind)
        cur += _up(used * s.esize, 4096) + 4096
    return out, cur


# ---------------------------------------------------------------------------------------------------------------- the arena and the checker
def new_arena(nbytes, device):
    assert nbytes % 8 == 0
    a = torch.empty(nbytes, dtype=torch.uint8, device=device)
    a.fill_(POISON)
    return a


def arena_is_poison(arena):
    """One pass over the arena as 64-bit words: all of them all-ones."""
    w = arena.view(torch.int64)
    return bool(w.min() == -1) and bool(w.max() == -1)


def first_stray_byte(arena, chunk=64 * MIB):
    """Byte offset of the first byte that is not poison (the failure path: chunked, so that it needs no second arena), or None."""
    for at in range(0, arena.numel(), chunk):
        bad = (arena[at:at + chunk] != POISON).nonzero()
        if bad.numel():
            return at + int(bad[0])
    return None


def write_inputs(arena, slots, data):
    for name, t in data.items():
        slots[name].view(arena).copy_(t)


def harvest(arena, slots):
    """Copy every view out, poison every view again, and require the arena to be all poison: nothing was written outside the views.
    -> {name: contiguous copy}.  Raises AssertionError naming the first stray byte."""
    out = {name: s.view(arena).clone(memory_format=torch.contiguous_format) for name, s in slots.items()}
    for s in slots.values():
        s.bytes_view(arena).fill_(POISON)
    if not arena_is_poison(arena):
        at = first_stray_byte(arena)
        arena.fill_(POISON)                                          # (the next case starts clean)
        raise AssertionError("a byte outside the views of the case was written: arena offset %d (0x%x)" % (at, at))
    return out


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def compare_exact(far, twin, names):
    """Bitwise comparison of the outputs `names` of the far call and of its twin.  -> list of failures, each naming the first differing index."""
    fails = []
    for n in names:
        a, b = _bits(far[n]), _bits(twin[n])
        if a.shape != b.shape:
            fails.append("%s: shapes %s / %s" % (n, tuple(a.shape), tuple(b.shape)))
        elif not torch.equal(a, b):
            diff = (a != b).nonzero()
            fails.append("%s: %d elements differ from the twin's, first at %s" % (n, diff.shape[0], tuple(int(i) for i in diff[0])))
    return fails


def nan_in_live_rows(out, names, live=None):
    """NaN in an output row that has a visible key.  live: bool mask over the leading dims of each output's rows (None: every row); dict name -> mask
    for outputs of different leading shapes.  -> list of failures."""
    fails = []
    for n in names:
        t = out[n].float()
        bad = torch.isnan(t)
        m = live.get(n) if isinstance(live, dict) else live
        if m is not None:
            while m.dim() < bad.dim():
                m = m.unsqueeze(-1)
            bad = bad & m.to(bad.device)
        if bad.any():
            fails.append("%s: NaN in a live row, first at %s" % (n, tuple(int(i) for i in bad.nonzero()[0])))
    return fails


# ---------------------------------------------------------------------------------------------------------------- the cases
# One table for both test modules: the CPU module proves on device "meta" that every layout crosses what it claims, the GPU module runs the calls.
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
BIAS_DTYPES = {"io": None, "f32": torch.float32, "bool": torch.bool}        # io: the call's dtype
ASM_DEFAULT = 1987                                                            # option "asm" as the library starts (fa2_launch.h)


def _case(id, fam="dense", dt="f16", B=None, H=None, Hkv=None, Nq=320, Nkv=None, D=64, causal=False, far="batch", bwd=False, opts=None, expect=None,
          ws=None, window=None, p=0.0, bias=None, layout="far", expect_bwd=None, form=None, softcap=0.0, slopes=False, dlse=None):
    if B is None:
        B = 3 if far == "batch" else 1
    if H is None:
        H = 2 if far == "batch" else 3
    return dict(id="%s-%s" % (id, far or layout), fam=fam, dt=dt, B=B, H=H, Hkv=Hkv or H, Nq=Nq, Nkv=Nkv or Nq, D=D, causal=causal, far=far, bwd=bwd,
                opts=opts or {}, expect=expect, ws=ws, window=window, p=p, seed=0x5EED0000 + D, bias=bias, layout=layout, expect_bwd=expect_bwd, form=form, softcap=softcap, slopes=slopes, dlse=dlse)


def _both(*a, **kw):
    return [_case(*a, far="batch", **kw), _case(*a, far="head", **kw)]


W100 = (100, -1, 64)          # left = 100, right from the causal flag, q_offset = 64

DENSE_CASES = (
    # ---- forward.  Compiler-scheduled, a head dim below its kernel's
    _both("fwd_hip_d96_bf16", dt="bf16", D=96, expect="hip") + _both("fwd_hip_d96_bf16_causal", dt="bf16", D=96, causal=True, expect="hip") +
    # hand-scheduled 256-row bodies (option rows = 256 takes the underfilled-grid rule away, as the other GPU tests do): fp16 on the 16x16x32 bodies, bf16, D = 64
    _both("fwd_asm_d128_f16", D=128, Nq=576, opts=dict(rows=256), expect="asm") + _both("fwd_asm_d128_bf16", dt="bf16", D=128, Nq=576, opts=dict(rows=256), expect="asm") +
    _both("fwd_asm_d64_f16", D=64, Nq=576, opts=dict(rows=256), expect="asm") +
    # the hand-scheduled 128-row kernel (option asm bit 5: sweeps this short too), at its own head dim and trimmed
    _both("fwd_d256", D=256, Nq=384, opts=dict(asm=ASM_DEFAULT | 32), expect="asm128") + _both("fwd_d160", dt="bf16", D=160, Nq=384, opts=dict(asm=ASM_DEFAULT | 32), expect="asm128") +
    _both("fwd_d512", D=512, Nq=192, expect="hip") +
    # the single-pass kernel of short KV sweeps
    _both("fwd_short", D=64, Nq=320, Nkv=77, expect="hip") +
    # every item of a grid of three split over the KV sweep; the workspace near and past 4 GiB
    [_case("fwd_split", B=3, H=1, D=128, Nq=64, Nkv=8192, far="batch", ws="near", expect="split"),
     _case("fwd_split_ws_far", B=1, H=3, D=128, Nq=64, Nkv=8192, far="head", ws="far", expect="split")] +
    # grouped K / V heads, far too
    [_case("fwd_gqa", B=1, H=6, Hkv=3, D=64, Nq=320, far="head", expect="hip"), _case("fwd_gqa", B=3, H=4, Hkv=2, D=128, Nq=320, dt="bf16", far="batch", expect="hip")] +
    # ---- backward (each case runs its forward first: O and LSE are that call's)
    # (expect_bwd: the kernels of the dQ and of the dK / dV pass, as fa2_bwd_plan names them)
    _both("bwd_hip_d64", D=64, Nq=320, bwd=True, expect_bwd=("hip", "hip")) + _both("bwd_hip_d64_causal", dt="bf16", D=64, Nq=300, causal=True, bwd=True, expect_bwd=("hip", "hip")) +
    _both("bwd_asm_d128", D=128, Nq=320, bwd=True, expect_bwd=("asm", "asm")) +
    _both("bwd_asm_d128_causal", dt="bf16", D=128, Nq=320, causal=True, bwd=True, expect_bwd=("asm", "asm")) +
    [_case("bwd_gqa", B=1, H=6, Hkv=3, D=64, Nq=320, far="head", bwd=True, expect_bwd=("hip", "hip")),
     _case("bwd_gqa", B=3, H=4, Hkv=2, D=128, Nq=320, far="batch", bwd=True, expect_bwd=("asm", "hip"))] +
    _both("bwd_short", D=64, Nq=320, Nkv=77, bwd=True, expect_bwd=("short", "hip")) + _both("bwd_d512", D=512, Nq=192, bwd=True, expect_bwd=("hip", "hip")) +
    [_case("bwd_split", B=3, H=1, D=64, Nq=256, Nkv=2048, far="batch", bwd=True, ws="near", expect="bwd_split"),
     _case("bwd_split_ws_far", B=1, H=3, D=64, Nq=256, Nkv=2048, far="head", bwd=True, ws="far", expect="bwd_split")] +
    # ---- bias and masks, forward and fa2_bwd_bias: the bias's batch stride is far
    [_case("bias_%s" % kind, fam="bias", B=3, H=2, D=64, Nq=256, bwd=True, bias=(kind, (3, 1, 256, 256)), expect="bias", form="tile") for kind in ("io", "f32", "bool")] +
    [_case("bias_rowbcast", fam="bias", B=3, H=2, D=64, Nq=256, bwd=True, bias=("bool", (3, 1, 1, 256)), expect="bias", form="row"),
     _case("bias_dma_grid", fam="bias", B=3, H=33, D=64, Nq=256, bwd=True, bias=("io", (3, 1, 256, 256)), expect="bias", form="tile_dma")] +
    # ---- sliding window with a query offset, and dropout: grouped forwards (K / V heads far), multi-head backwards
    [_case("window_gqa_d%d" % D, fam="window", B=1, H=6, Hkv=3, D=D, Nq=320, causal=True, far="head", window=W100, expect="window") for D in (64, 128)] +
    [c for D in (64, 128) for c in _both("window_d%d" % D, fam="window", D=D, Nq=320, causal=True, window=W100, bwd=True, expect="window")] +
    [_case("dropout_gqa_d%d" % D, fam="dropout", B=1, H=6, Hkv=3, D=D, Nq=320, causal=True, far="head", window=W100, p=0.25) for D in (64, 128)] +
    [c for D in (64, 128) for c in _both("dropout_d%d" % D, fam="dropout", D=D, Nq=320, causal=True, window=W100, p=0.25, bwd=True)]
)


def dense_specs(case):
    """[(name, dtype, shape, pitch[, far])] of a dense case's tensors, in the order they are placed."""
    dt, B, H, Hkv, Nq, Nkv, D = DTYPES[case["dt"]], case["B"], case["H"], case["Hkv"], case["Nq"], case["Nkv"], case["D"]
    specs = [("q", dt, (B, H, Nq, D), D), ("k", dt, (B, Hkv, Nkv, D), D), ("v", dt, (B, Hkv, Nkv, D), D), ("o", dt, (B, H, Nq, D), D),
             ("lse", torch.float32, (B, H, Nq), None)]
    if case["bwd"]:
        specs += [("do", dt, (B, H, Nq, D), D), ("dq", dt, (B, H, Nq, D), D), ("dk", dt, (B, Hkv, Nkv, D), D), ("dv", dt, (B, Hkv, Nkv, D), D),
                  ("delta", torch.float32, (B, H, Nq), None)]
    if case["bias"]:
        kind, shape = case["bias"]
        specs.append(("bias", BIAS_DTYPES[kind] or dt, shape, shape[3], "batch"))
    if case.get("dlse"):                                             # the gradient of the LSE: strides of its own — far like the rest, or compact
        specs.append(("dlse", torch.float32, (B, H, Nq), None) + ((None,) if case["dlse"] == "compact" else ()))
    return specs


WS_FAR_OFFSET = 2 * FAR_STEP + 128 * MIB        # a workspace past 4 GiB
SLOPES_OFFSET = 48 * MIB + 5 * 4096 + 16        # ALiBi slopes: behind the first slices too
WS_NEAR_OFFSET = 192 * MIB                      # ... and one behind the first slices (validate() proves that nothing else is there)


def dense_slots(case, ws_bytes=0, step=FAR_STEP):
    """-> (far slots, twin slots, bytes of the twin's buffer).  The workspace of a split call is a flat slot of the far layout (scratch: poisoned
    again like every view); the twin gets one of its own."""
    slots = place(dense_specs(case), case["far"], step=step, gap=32768)
    if case.get("slopes"):                                           # ALiBi slopes: [B, H] with a far batch stride, or one shared [H] vector (B = 1: stride 0)
        B, H = case["B"], case["H"]
        slots["slopes"] = Slot("slopes", torch.float32, (B, H), (step // 4 if B > 1 else H, 1), SLOPES_OFFSET)
    twin, tbytes = twin_of(slots)
    if ws_bytes:
        at = WS_FAR_OFFSET if case["ws"] == "far" else WS_NEAR_OFFSET
        slots["ws"] = Slot("ws", torch.uint8, (ws_bytes,), (1,), at)
        twin["ws"] = Slot("ws", torch.uint8, (ws_bytes,), (1,), tbytes)
        tbytes += _up(ws_bytes, 4096) + 4096
    return slots, twin, tbytes


# ---- packed, row-far: [total, H, D] views with a row pitch of 2^19 elements (1 MiB); the sequences' first rows cross 2^31 and 2^32
PACKED_TOTAL = 4352
PACKED_PITCH_BYTES = MIB
PACKED_LENS = [1500, 700, 0, 1100, 300, 500, 1, 200]       # bases 0 1500 2200 2200 3300 3600 4100 4101: two sequences start past 4 GiB; 51 rows lie behind cu[B]
# The K / V lengths differ (fewer and more keys than queries): a sequence's Q and K bases are different far rows, and bottom-right causal — row i
# sees the keys up to i + nk - nq — is not top-left causal.  Bases 0 1300 2200 2200 3250 3600 4100 4103; 99 rows lie behind cu_k[B]
PACKED_LENS_K = [1300, 900, 0, 1050, 350, 500, 3, 150]
PACKED_CASES = [
    dict(id="varlen_gqa_topleft", H=4, Hkv=2, D=64, dt="f16", causal=True, bottom_right=False, p=0.0, bwd=False),
    dict(id="varlen_bottomright", H=2, Hkv=2, D=64, dt="bf16", causal=True, bottom_right=True, p=0.0, bwd=True),
    dict(id="varlen_topleft", H=2, Hkv=2, D=128, dt="f16", causal=True, bottom_right=False, p=0.0, bwd=True),
    dict(id="varlen_dropout_gqa", H=4, Hkv=2, D=64, dt="f16", causal=True, bottom_right=True, p=0.25, bwd=False),
    dict(id="varlen_dropout", H=2, Hkv=2, D=64, dt="f16", causal=False, bottom_right=False, p=0.25, bwd=True),
    # score modifiers (fa2_fwd_varlen_scoremod / fa2_bwd_varlen_scoremod): slopes [num_sequences, H], the last sequences' vectors past byte 2^31
    dict(id="varlen_smod_gqa_topleft", H=4, Hkv=2, D=64, dt="f16", causal=True, bottom_right=False, p=0.0, bwd=False, softcap=30.0, slopes=True),
    dict(id="varlen_smod_bottomright", H=2, Hkv=2, D=64, dt="bf16", causal=True, bottom_right=True, p=0.0, bwd=True, softcap=30.0, slopes=True),
    # a gradient for the LSE (fa2_bwd_varlen_lse): dlse [H, total] far like the LSE; bottom-right rows without a visible key carry a NaN in it
    dict(id="varlen_lse", H=2, Hkv=2, D=64, dt="f16", causal=True, bottom_right=True, p=0.0, bwd=True, dlse=True),
]
for _c in PACKED_CASES:
    _c["seed"] = 0x5EED1000 + _c["D"]
PACKED_LSE_OFFSET = (1 << 32) + 3 * 4096 + 512 * 1024      # LSE and delta [H, total] far too, in the gap between two rows' columns
PACKED_SLOPES_OFFSET = 576 * 1024                          # ALiBi slopes [num_sequences, H]: in the gaps as well, ...
PACKED_SLOPES_STEP = 384 * MIB + 3 * 4096                  # ... the sequences' vectors this many bytes apart: the last two lie past 2^31


def packed_slots(case):
    dt, H, Hkv, D, T = DTYPES[case["dt"]], case["H"], case["Hkv"], case["D"], PACKED_TOTAL
    specs = [("q", dt, (T, H, D)), ("k", dt, (T, Hkv, D)), ("v", dt, (T, Hkv, D)), ("o", dt, (T, H, D))]
    flat = ["lse"]
    if case["bwd"]:
        specs += [("do", dt, (T, H, D)), ("dq", dt, (T, H, D)), ("dk", dt, (T, Hkv, D)), ("dv", dt, (T, Hkv, D))]
        flat.append("delta")
    if case.get("dlse"):
        flat.append("dlse")
    slots = place_rows(specs, PACKED_PITCH_BYTES)
    at = PACKED_LSE_OFFSET
    for name in flat:
        slots[name] = Slot(name, torch.float32, (H, T), (T, 1), at)
        at += _up(H * T * 4, 4096) + 4096
    if case.get("slopes"):
        slots["slopes"] = Slot("slopes", torch.float32, (len(PACKED_LENS), H), (PACKED_SLOPES_STEP // 4, 1), PACKED_SLOPES_OFFSET)
    twin, tbytes = twin_of(slots, keep_pitch=False)
    return slots, twin, tbytes


# ---- spans: one head (B = H = 1) whose rows are so far apart that the SPAN reaches a limit.  The tensors with the wide pitch and their twins — same
# pitch, the base moved — interleave inside the pitch; everything else is compact in the gap behind the first row's columns.
SPAN_PITCH_3G = 10 * MIB            # bytes: 320 rows span 3.1 GiB — inside [2 GiB, 4 GiB), and 384 rows stay below 4 GiB (the hand-scheduled forward's rule)
SPAN_PITCH_4G = 15 * MIB            # bytes: 288 rows span 4.2 GiB
SPAN_START = FAR_STEP + 600 * MIB    # the limit cases' base: past 2^31, and the 1.6 GiB span behind it crosses 2^32
SPAN_CASES = [
    # K / V on the last accepted pitch of the documented rule; the base moved past 2^31, so that the span also crosses 2^32
    dict(id="span_kv_at_limit", D=64, Nq=320, Nkv=192, dt="f16", wide=("k", "v"), pitch="limit", start=SPAN_START, bwd=False, expect="hip"),
    # backward: Q and dO too
    dict(id="span_bwd_at_limit", D=64, Nq=192, Nkv=192, dt="bf16", wide=("q", "k", "v", "do"), pitch="limit", start=SPAN_START, bwd=True, expect_bwd=("hip", "hip")),
    # forward: Q and O with a per-head span in [2 GiB, 4 GiB): the hand-scheduled body still takes it (32-bit offsets, unsigned) ...
    dict(id="span_qo_3g_asm", D=128, Nq=320, Nkv=576, dt="f16", wide=("q", "o"), pitch=SPAN_PITCH_3G, start=0, bwd=False, opts=dict(rows=256), expect="asm"),
    # ... and beyond 4 GiB: the planner must leave the hand-scheduled bodies (256-row, and the 128-row kernel of D = 256)
    dict(id="span_qo_4g_d128", D=128, Nq=288, Nkv=576, dt="f16", wide=("q", "o"), pitch=SPAN_PITCH_4G, start=0, bwd=False, opts=dict(rows=256), expect="hip"),
    dict(id="span_qo_4g_d256", D=256, Nq=288, Nkv=576, dt="bf16", wide=("q", "o"), pitch=SPAN_PITCH_4G, start=0, bwd=False, opts=dict(asm=ASM_DEFAULT | 32), expect="hip"),
    # backward: O, dQ, dK, dV beyond 4 GiB.  O is the one the hand-scheduled dQ pass would address with 32-bit offsets: the planner leaves it (host.cpp: launch_bwd)
    dict(id="span_bwd_outputs_4g", D=128, Nq=288, Nkv=288, dt="f16", wide=("o", "dq", "dk", "dv"), pitch=SPAN_PITCH_4G, start=0, bwd=True, expect_bwd=("hip", "hip")),
    dict(id="span_bwd_o_4g_d64", D=64, Nq=288, Nkv=288, dt="bf16", wide=("o", "dq", "dk", "dv"), pitch=SPAN_PITCH_4G, start=0, bwd=True, expect_bwd=("hip", "hip")),
    # ... on either side of that bound: O on the last pitch of the 2 GiB rule keeps both hand-scheduled passes, an O span in [2 GiB, 4 GiB) leaves them
    dict(id="span_bwd_o_at_limit", D=128, Nq=320, Nkv=320, dt="f16", wide=("o",), pitch="limit", start=FAR_STEP + 500 * MIB, bwd=True, expect_bwd=("asm", "asm")),
    dict(id="span_bwd_o_3g", D=128, Nq=320, Nkv=320, dt="bf16", wide=("o",), pitch=SPAN_PITCH_3G, start=0, bwd=True, expect_bwd=("hip", "hip")),
    # forward, a head dim below the body's (96 on the 128 body): Q on the last pitch of the hand-scheduled bodies' 2 GiB rule — 64 rows past Nq; the
    # marker of a granule the row does not have is byte offset 2^31
    dict(id="span_q_trimmed_at_limit", D=96, Nq=320, Nkv=576, dt="f16", wide=("q",), pitch="limit_trim", start=FAR_STEP + 500 * MIB, bwd=False,
         opts=dict(rows=256), expect="asm"),
    # forward, the 128-row kernel: Q and O on the last pitch of its 4 GiB rule — 128 rows past Nq — with a ragged Nq (264 = 2 * 128 + 8, 257: the last
    # workgroup's waves 1 .. 3 lie wholly past Nq and still form their rows' offsets, up to row Nq + 126), at the kernel's head dim and a trimmed one
    dict(id="span_qo_d256_at_limit", D=256, Nq=264, Nkv=576, dt="bf16", wide=("q", "o"), pitch="limit128", start=0, bwd=False,
         opts=dict(asm=ASM_DEFAULT | 32), expect="asm128"),
    dict(id="span_qo_d160_at_limit", D=160, Nq=257, Nkv=576, dt="f16", wide=("q", "o"), pitch="limit128", start=0, bwd=False,
         opts=dict(asm=ASM_DEFAULT | 32), expect="asm128"),
]
for _c in SPAN_CASES:
    _c.update(fam="dense", B=1, H=1, Hkv=1, causal=False, window=None, p=0.0, seed=0x5EED2000, bias=None, ws=None, far=None, layout="span")
    _c.setdefault("opts", {})
    _c.setdefault("expect", None)
    _c.setdefault("expect_bwd", None)


ASM128_SLACK_ROWS = 128           # the 128-row forward kernel: ((Nq + 128) * pitch + 256) * 2 < 2^32, Q and O
ASM256_SLACK_ROWS = 64            # the 256-row forward bodies: ((Nq + 64) * pitch + D) * 2 < 2^32, or 2^31 at a head dim below the body's


def span_pitch_bytes(case):
    if case["pitch"] == "limit128":
        return 2 * (((1 << 31) - 1 - 256) // (case["Nq"] + ASM128_SLACK_ROWS) // 8 * 8)
    if case["pitch"] == "limit_trim":
        return 2 * (((1 << 30) - 1 - case["D"]) // (case["Nq"] + ASM256_SLACK_ROWS) // 8 * 8)
    if case["pitch"] != "limit":
        return case["pitch"]
    n = max(case["Nq"] if w in ("q", "do") else case["Nkv"] for w in case["wide"])
    return 2 * last_pitch(n, case["D"])


def span_slots(case):
    """-> (far slots, twin slots): both in the arena."""
    dt, Nq, Nkv, D = DTYPES[case["dt"]], case["Nq"], case["Nkv"], case["D"]
    rows = dict(q=Nq, o=Nq, do=Nq, dq=Nq, k=Nkv, v=Nkv, dk=Nkv, dv=Nkv)
    names = ["q", "k", "v", "o"] + (["do", "dq", "dk", "dv"] if case["bwd"] else [])
    pitch = span_pitch_bytes(case)
    wide = place_rows([(n + t, dt, (1, 1, rows[n], D)) for t in ("", "_t") for n in case["wide"]], pitch, start=case["start"])
    specs = [(n + t, dt, (1, 1, rows[n], D), D) for t in ("", "_t") for n in names if n not in case["wide"]]
    specs += [(n + t, torch.float32, (1, 1, Nq), None) for t in ("", "_t") for n in (["lse", "delta"] if case["bwd"] else ["lse"])]
    rest = place(specs, None, start=case["start"] + 65536, gap=4096)
    assert max(s.extent()[1] for s in rest.values()) <= case["start"] + pitch
    both = dict(wide, **rest)
    return ({n: s for n, s in both.items() if not n.endswith("_t")},
            {n[:-2]: Slot(n[:-2], s.dtype, s.shape, s.strides, s.offset, s.kind) for n, s in both.items() if n.endswith("_t")})


# ---- one bias slice on the last accepted pitch of the backward's 2 GiB slice rule (include/fa2_gfx950.h):
# ((Nq - 1) * pitch + Nkv + 64 * pitch) * element size < 2^31 - 1
def last_bias_pitch(Nq, Nkv, esize, gran=None):
    gran = gran or 16 // esize                    # whole 16-byte granules: the tile forms of the kernels
    return ((SPAN_LIMIT - 1) // esize - Nkv) // (Nq - 1 + SPAN_SLACK_ROWS) // gran * gran


BIAS_SPAN_CASE = dict(id="bias_slice_at_limit", fam="bias", dt="f16", B=1, H=1, Hkv=1, Nq=256, Nkv=256, D=64, causal=False, far=None, bwd=True, opts={},
                      expect="bias", ws=None, window=None, p=0.0, seed=0x5EED3000, bias=("f32", (1, 1, 256, 256)), layout="bias_span", expect_bwd=("hip", "hip"),
                      pitch_step=0, form="tile")
# The forward's own use of that rule: a grid past 3/8 of the CUs (3 * 33 = 99 workgroups of 256 rows against 96 on 256 CUs) stages the bias tile by
# LDS-DMA, with 32-bit byte offsets into the slice — one [256, 256] slice shared by every batch and head (strides 0), on the last pitch of the rule.  On
# the next pitch the forward is still served: it takes the tile loads from 64-bit row pointers (the backward refuses that pitch: forward only).
BIAS_DMA_SPAN_CASES = [
    dict(BIAS_SPAN_CASE, id="bias_dma_slice_at_limit", B=3, H=33, Hkv=33, bias=("io", (1, 1, 256, 256)), seed=0x5EED3001, form="tile_dma"),
    dict(BIAS_SPAN_CASE, id="bias_dma_slice_next_pitch", B=3, H=33, Hkv=33, bias=("io", (1, 1, 256, 256)), seed=0x5EED3002, form="tile", pitch_step=1,
         bwd=False, expect_bwd=None),
]
BIAS_SPAN_CASES = [BIAS_SPAN_CASE] + BIAS_DMA_SPAN_CASES


def bias_span_slots(case):
    """The bias and its twin (same pitch, base moved) interleave from SPAN_START on; the call's other tensors are compact, far run and twin apart: in
    the gap behind the first row's columns where they fit, else in front of SPAN_START.  pitch_step: whole granules past the last accepted pitch."""
    kind, shape = case["bias"]
    bdt = BIAS_DTYPES[kind] or DTYPES[case["dt"]]
    es = torch.empty((), dtype=bdt).element_size()
    pitch = (last_bias_pitch(case["Nq"], case["Nkv"], es) + case["pitch_step"] * (16 // es)) * es
    wide = place_rows([("bias", bdt, shape), ("bias_t", bdt, shape)], pitch, start=SPAN_START)
    specs = [(n + t,) + tuple(s[1:]) for t in ("", "_t") for s in dense_specs(case) for n in [s[0]] if n != "bias"]
    rest = place([s[:4] for s in specs], None, start=SPAN_START + 65536, gap=4096)
    if max(s.extent()[1] for s in rest.values()) > SPAN_START + pitch:
        rest = place([s[:4] for s in specs], None, start=8192, gap=4096)
        assert max(s.extent()[1] for s in rest.values()) <= SPAN_START
    both = dict(wide, **rest)
    return ({n: s for n, s in both.items() if not n.endswith("_t")},
            {n[:-2]: Slot(n[:-2], s.dtype, s.shape, s.strides, s.offset, s.kind) for n, s in both.items() if n.endswith("_t")})


# ---- f32 tensors at an element index past 2^31 (their own arena of 8 GiB + 256 MiB): LSE, delta and an f32 bias with a far batch stride
F32_STEP = (1 << 32) + 3 * 4096                  # bytes: batch 1 sits at float index 2^30 + 3072, batch 2 at 2^31 + 6144
F32_CASES = [
    _case("f32_lse_delta", D=128, Nq=320, bwd=True, far="batch", expect_bwd=("asm", "asm")),
    _case("f32_bias", fam="bias", B=3, H=2, D=64, Nq=256, bwd=True, bias=("f32", (3, 1, 256, 256)), far="batch", expect="bias", form="tile"),
    # dlse and the ALiBi slopes at a float index past 2^31 (the slopes' batch stride is the step too); dead rows carry a NaN in dlse
    _case("f32_dlse_slopes", fam="scoremod", D=64, Nq=320, Nkv=256, causal=True, window=W100, softcap=30.0, slopes=True, bwd=True, far="batch", dlse="far"),
]

# ---- score modifiers (fa2_fwd_scoremod / fa2_bwd_scoremod): soft-capping at 30 and ALiBi slopes on the causal window W100.  Batch-far cases: slopes
# [B, H] whose batch stride is FAR_STEP bytes (b * alibi_batch_stride + h); head-far cases: one shared [H] vector, stride 0.
SCOREMOD_CASES = (
    [c for D in (64, 128) for c in _both("smod_d%d" % D, fam="scoremod", D=D, Nq=320, causal=True, window=W100, softcap=30.0, slopes=True, bwd=True)] +
    [_case("smod_gqa", fam="scoremod", B=1, H=6, Hkv=3, D=64, Nq=320, causal=True, far="head", window=W100, softcap=30.0, slopes=True)]
)
# ---- a gradient for the LSE (fa2_bwd_lse, fa2_bwd_window_lse): a dlse slot with strides of its own, far like lse, or compact beside far tensors.
# The windowed cases have 256 keys for 320 rows at q_offset 64: rows 292 .. 319 see no key, carry a NaN in dlse and must get zero gradients.
LSE_CASES = (
    [_case("lse_d64", D=64, Nq=320, bwd=True, far="batch", dlse="far", expect_bwd=("hip", "hip")),
     _case("lse_d64", D=64, Nq=320, bwd=True, far="head", dlse="compact", expect_bwd=("hip", "hip"))] +
    # head dim 128 with a dlse leaves the hand-scheduled passes (fa2_bwd_lse_plan)
    _both("lse_d128", dt="bf16", D=128, Nq=320, causal=True, bwd=True, dlse="far", expect_bwd=("hip", "hip")) +
    [_case("lse_bias", fam="bias", B=3, H=2, D=64, Nq=256, bwd=True, bias=("f32", (3, 1, 256, 256)), far="batch", dlse="far", expect="bias", form="tile"),
     # fa2_bwd_window_lse on each of its routes: the windowed, the dropout and the score-modifier backward
     _case("lse_window", fam="window", D=64, Nq=320, Nkv=256, causal=True, window=W100, bwd=True, far="batch", dlse="far", expect="window"),
     _case("lse_dropout", fam="dropout", dt="bf16", D=128, Nq=320, Nkv=256, causal=True, window=W100, p=0.25, bwd=True, far="head", dlse="far"),
     _case("lse_smod", fam="scoremod", D=128, Nq=320, Nkv=256, causal=True, window=W100, softcap=30.0, slopes=True, bwd=True, far="batch", dlse="compact")]
)


# ---- KV-cache decode (fa2_fwd_decode, fa2_fwd_decode_fp8): the header states no span limit, so every product of the kernel must be 64-bit — page id
# times page stride, batch times batch stride, key row times row pitch, the block table's and the descales' batch strides.  Tensors are the
# operator's: q / o [B, Nq, H, D], caches [B, Nmax, Hkv, D] or [num_pages, page, Hkv, D], lse [B, H, Nq].  fmt "16": caches of the I/O dtype;
# "fp8": e4m3 bytes in the SAME byte layout, so that an element index is a byte offset and passes 2^31 and 2^32 where the bytes do.
# Cache rows at or beyond a length, unused pages and the workspace stay poison: 0xFFFF is NaN in fp16 and bf16, 0xFF an e4m3 NaN, 0xFFFFFFFF a f32 NaN.
E4M3 = torch.float8_e4m3fn
DECODE_NMAX = 1024
DECODE_WIDE_NMAX = 1008
DECODE_WIDE_PITCH = 4 * MIB + 77 * 4096           # bytes of a key row: 1000 valid keys span 4.2 GiB, the 1008 rows of the capacity fit the arena
DECODE_PAGE_STRIDE = 64 * MIB + 5 * 4096          # bytes from page to page
DECODE_POOL_BASE = 8 * MIB                        # page 0 (the compact tensors of the case lie in front of it)
DECODE_NUM_PAGES = 68                             # pages 0 .. 31 end below 2^31, 32 .. 63 lie between 2^31 and 2^32, 64 .. 67 past 2^32


def _dcase(id, layout, dt, D, H, Hkv, Nq, lens, rt, page=0, bt=None, descale="kv"):
    """descale: which of k_descale / v_descale the FP8 call is given ("kv", "k", "v")."""
    return dict(id=id, layout=layout, dt=dt, D=D, H=H, Hkv=Hkv, Nq=Nq, lens=tuple(lens), B=len(lens), rt=rt, page=page, bt=bt, descale=descale,
                nmax=DECODE_WIDE_NMAX if layout == "wide" else DECODE_NMAX, seed=0x5EED5000 + 131 * D + 17 * H + Nq + page)


DECODE_CASES = [
    # batches FAR_STEP bytes apart: q, o, lse, both caches, the descales.  Rows per K / V head 1, 20 and 64: the kernels of 1, 2 and 4 row tiles
    _dcase("decode_batch_rt1", "batch", "f16", 128, 8, 8, 1, (129, 65, 1000), 1),
    _dcase("decode_batch_rt2", "batch", "bf16", 64, 10, 2, 4, (2, 1000, 65), 2, descale="v"),
    _dcase("decode_batch_rt4", "batch", "bf16", 128, 16, 1, 4, (1000, 0, 129), 4),
    # three K / V heads FAR_STEP bytes apart, the query heads of q, o and lse far too (six of them: the last lies past 2^32)
    _dcase("decode_head_rt1", "head", "bf16", 128, 3, 3, 1, (129,), 1),
    _dcase("decode_head_rt2", "head", "f16", 64, 6, 3, 10, (1000,), 2, descale="k"),
    # one sequence whose key rows are 4.3 MiB apart, K and V interleaved inside the pitch
    _dcase("decode_wide_row", "wide", "f16", 128, 16, 1, 4, (1000,), 4),
    # paged: pages 64 MiB + 20 KiB apart, every sequence with keys takes pages of all three regions; the block table's rows far / compact
    _dcase("decode_paged64", "paged", "f16", 128, 10, 2, 4, (1000, 0, 129), 2, page=64, bt="far"),
    _dcase("decode_paged128", "paged", "bf16", 64, 16, 1, 4, (300, 1000, 0), 4, page=128, bt="compact", descale="k"),
]
DECODE_FORMATS = ("16", "fp8")
DECODE_F32_CASE = DECODE_CASES[6]                 # runs in the f32 arena too, batch stride F32_STEP: b * stride of lse, descales and block table past element 2^31


def _bslot(name, dtype, shape, byte_strides, offset):
    """A slot from BYTE strides of the leading dimensions (the last one is contiguous)."""
    es = torch.empty((), dtype=dtype).element_size()
    assert all(s % es == 0 for s in byte_strides)
    return Slot(name, dtype, shape, tuple(s // es for s in byte_strides) + (1,), offset)


def decode_page_regions(case, fmt):
    """Page ids whose K and V blocks end below byte 2^31, lie between 2^31 and 2^32, start past 2^32."""
    block = 2 * (_up(case["page"] * case["Hkv"] * case["D"] * (1 if fmt == "fp8" else 2), 4096) + 4096)
    at = [DECODE_POOL_BASE + p * DECODE_PAGE_STRIDE for p in range(DECODE_NUM_PAGES)]
    low = [p for p, a in enumerate(at) if a + block <= 1 << 31]
    mid = [p for p, a in enumerate(at) if a > 1 << 31 and a + block <= 1 << 32]
    high = [p for p, a in enumerate(at) if a > 1 << 32]
    assert len(low) + len(mid) + len(high) == DECODE_NUM_PAGES
    return low, mid, high


def decode_block_tables(case, fmt):
    """-> (far block table [B, max_pages], twin block table, far poison page, twin page count): every sequence with keys takes one page of each region
    and the rest from below 2^32, in an order shuffled with the case's seed; entries beyond a sequence's pages name a page nobody wrote (a valid id,
    past 2^32).  The twin numbers its own small pool, in another shuffled order."""
    rng = np.random.RandomState(case["seed"] & 0xFFFF)
    page, per = case["page"], DECODE_NMAX // case["page"]
    low, mid, high = (list(rng.permutation(r)) for r in decode_page_regions(case, fmt))
    used = [-(-n // page) for n in case["lens"]]
    poison = int(high.pop())
    total_t = sum(used) + 1
    order_t = list(rng.permutation(total_t))
    bt, bt_t = np.full((case["B"], per), poison, dtype=np.int32), np.full((case["B"], per), int(order_t.pop()), dtype=np.int32)
    for b, n in enumerate(used):
        if n == 0:
            continue
        assert n >= 3, "a sequence with keys needs a page of each region"
        mine = [high.pop(), mid.pop(), low.pop()]
        rest = low + mid
        take = list(rng.permutation(len(rest))[:n - 3])
        mine += [rest[i] for i in take]
        low, mid = [p for p in low if p not in mine], [p for p in mid if p not in mine]
        bt[b, :n] = rng.permutation(mine)
        bt_t[b, :n] = [order_t.pop() for _ in range(n)]
    return bt, bt_t, poison, total_t


def decode_slots(case, fmt, ws_bytes=0, ws="near", step=FAR_STEP):
    """-> (far slots, twin slots, bytes of the twin's buffer).  Slots: q k v o lse lens, bt (paged), kd / vd (fp8, as the case's `descale` says), ws
    (a split call).  The twin: the same shapes, compact, in a buffer of its own; a paged twin is a small pool of its own numbering.
    step: the batch stride in bytes of the batch-far tensors (F32_STEP in the f32 arena: lse, the descales and the block table at ELEMENT indices past 2^31)."""
    io, fp8 = DTYPES[case["dt"]], fmt == "fp8"
    cdt, ces = (E4M3, 1) if fp8 else (io, 2)
    B, H, Hkv, Nq, D, N, lay = case["B"], case["H"], case["Hkv"], case["Nq"], case["D"], case["nmax"], case["layout"]
    i32, f32 = torch.int32, torch.float32
    names = ["q", "k", "v", "o", "lse", "lens"] + (["bt"] if lay == "paged" else []) + (["kd", "vd"] if fp8 else [])
    if fp8:
        names = [n for n in names if n not in {"kv": (), "k": ("vd",), "v": ("kd",)}[case["descale"]]]
    # compact shapes and byte strides (the twin's, and the inner dimensions of the far layouts)
    cshape = (DECODE_NUM_PAGES, case["page"], Hkv, D) if lay == "paged" else (B, N, Hkv, D)
    shapes = dict(q=(B, Nq, H, D), o=(B, Nq, H, D), k=cshape, v=cshape, lse=(B, H, Nq), lens=(B,), kd=(B, Hkv), vd=(B, Hkv), bt=(B, DECODE_NMAX // max(case["page"], 1)))
    dts = dict(q=io, o=io, k=cdt, v=cdt, lse=f32, lens=i32, kd=f32, vd=f32, bt=i32)

    def compact(shape, es):
        st = [es]
        for n in reversed(shape[1:]):
            st.insert(0, st[0] * n)
        return st[:-1]

    slots, cur = {}, 0 if lay != "wide" else 65536
    hs_q = head_step(H)
    for n in names:
        shape, dt = shapes[n], dts[n]
        es = torch.empty((), dtype=dt).element_size()
        st = compact(shape, es)
        if n in ("k", "v") and lay in ("wide", "paged"):
            continue
        if lay in ("batch", "paged") and n != "lens" and not (n == "bt" and case["bt"] == "compact"):
            st[0] = step
            used = int(np.prod(shape[1:])) * es
        elif lay == "head" and n in ("q", "o"):
            st, used = [H * hs_q, D * es, hs_q], Nq * D * es                      # [B, Nq, H, D]: each head a block of Nq rows
        elif lay == "head" and n in ("k", "v"):
            st, used = [Hkv * FAR_STEP, D * es, head_step(Hkv)], N * D * es
        elif lay == "head" and n == "lse":
            st, used = [H * hs_q, hs_q], Nq * es
        else:
            used = int(np.prod(shape)) * es
        slots[n] = _bslot(n, dt, shape, st, cur)
        cur += _up(used, 4096) + 32768 + 1040
    if lay == "wide":                                                             # K and V interleave inside the row pitch
        P, width = DECODE_WIDE_PITCH, _up(Hkv * D * ces, 16) + 64
        for i, n in enumerate(("k", "v")):
            slots[n] = _bslot(n, cdt, cshape, [N * P, P, D * ces], i * width)
        assert cur <= P and 2 * width <= 65536
    if lay == "paged":                                                            # ... and inside the page stride
        assert cur <= DECODE_POOL_BASE
        block = _up(case["page"] * Hkv * D * ces, 4096) + 4096
        for i, n in enumerate(("k", "v")):
            slots[n] = _bslot(n, cdt, cshape, [DECODE_PAGE_STRIDE, Hkv * D * ces, D * ces], DECODE_POOL_BASE + i * block)
    twin, tcur = {}, 0
    for n in names:
        shape = shapes[n]
        if lay == "paged" and n in ("k", "v"):
            shape = (decode_block_tables(case, fmt)[3],) + shape[1:]
        es = torch.empty((), dtype=dts[n]).element_size()
        twin[n] = _bslot(n, dts[n], shape, compact(shape, es), tcur)
        tcur += _up(int(np.prod(shape)) * es, 4096) + 4096
    if ws_bytes:
        slots["ws"] = Slot("ws", torch.uint8, (ws_bytes,), (1,), WS_FAR_OFFSET if ws == "far" else WS_NEAR_OFFSET)
        twin["ws"] = Slot("ws", torch.uint8, (ws_bytes,), (1,), tcur)
        tcur += _up(ws_bytes, 4096) + 4096
    return slots, twin, tcur


def decode_inputs(case, fmt):
    """CPU data of a case (one generator, the case's seed): q, the LOGICAL caches k / v [B, Nmax, Hkv, D] (e4m3 for fmt "fp8": clamp(randn / d, +-448)
    with power-of-two descales d per (sequence, K / V head), 1 where the case leaves the descale out), kd / vd (None: left out)."""
    g = torch.Generator(device="cpu").manual_seed(case["seed"])
    io, B, H, Hkv, Nq, D, N = DTYPES[case["dt"]], case["B"], case["H"], case["Hkv"], case["Nq"], case["D"], case["nmax"]
    data = {"q": torch.randn((B, Nq, H, D), generator=g).to(io), "lens": torch.tensor(case["lens"], dtype=torch.int32)}
    xk, xv = (torch.randn((B, N, Hkv, D), generator=g) for _ in range(2))
    if fmt != "fp8":
        data.update(k=xk.to(io), v=xv.to(io), kd=None, vd=None)
        return data
    kd, vd = (2.0 ** -torch.randint(5, 8, (B, Hkv), generator=g).float() for _ in range(2))
    kd, vd = (kd if "k" in case["descale"] else None), (vd if "v" in case["descale"] else None)
    one = torch.ones(B, 1, Hkv, 1)
    data.update(k=(xk / (one if kd is None else kd[:, None, :, None])).clamp(-448.0, 448.0).to(E4M3),
                v=(xv / (one if vd is None else vd[:, None, :, None])).clamp(-448.0, 448.0).to(E4M3), kd=kd, vd=vd)
    return data


def _poison_like(slot):
    return torch.full(slot.shape[:-1] + (slot.shape[-1] * slot.esize,), POISON, dtype=torch.uint8)


def decode_images(case, fmt, slots, data, block_table=None):
    """What each INPUT slot must hold before and after the call, as uint8 tensors of the slot's shape (last dimension in bytes): the valid rows of the
    caches — scattered into their pages for a paged case — and poison everywhere else in them."""
    img = {}
    for n, s in slots.items():
        if n in ("o", "lse", "ws"):
            continue
        im = _poison_like(s)
        if n in ("k", "v"):
            raw = data[n].contiguous().view(torch.uint8)
            for b, ln in enumerate(case["lens"]):
                if case["layout"] != "paged":
                    im[b, :ln] = raw[b, :ln]
                    continue
                page = case["page"]
                for j in range(-(-ln // page)):
                    rows = min(page, ln - j * page)
                    im[int(block_table[b, j]), :rows] = raw[b, j * page:j * page + rows]
        elif n == "bt":
            im = torch.from_numpy(np.ascontiguousarray(block_table)).view(torch.uint8)
        else:
            im = data[n].contiguous().view(torch.uint8)
        assert tuple(im.shape) == tuple(_poison_like(s).shape), (n, im.shape)
        img[n] = im
    return img


def image_failures(got, images, who=""):
    """The harvested input slots against the images they were written from, byte for byte.  -> list of failures."""
    return ["%s input %s was written, or a row beyond a length is no longer poison" % (who, n) for n, im in images.items()
            if not torch.equal(got[n].cpu().contiguous().view(torch.uint8).reshape(im.shape), im)]


# ---- merge of partial results (fa2_merge_fwd, fa2_merge_bwd): three parts that share one far stride set, as the C-ABI demands; o, lse, dout, dlse and
# the parts' gradients are far as well.  Part 1 has rows of weight exactly 0 (lse -inf) whose O stays poison: the contract says they are never read.
# A far stride leaves no room for a base past 4 GiB inside the arena, so the batch- and head-far parts start as far apart as their slices allow
# and one compact case puts part 0 at the arena's start, part 1 past 2^31 and part 2 past 2^32.
MERGE_PARTS = 3
MERGE_CASES = [
    dict(id="merge_batch", layout="batch", dt="f16", B=3, H=2, Nq=203, D=128, natural=False),
    dict(id="merge_head_d40", layout="head", dt="bf16", B=1, H=3, Nq=203, D=40, natural=True),          # D / 8 = 5: the backward's idle group lanes
    dict(id="merge_packed", layout="packed", dt="f16", B=1, H=2, Nq=PACKED_TOTAL, D=64, natural=False),  # B = 1, Nq = total, rows 1 MiB apart
    dict(id="merge_bases", layout="bases", dt="bf16", B=2, H=2, Nq=203, D=128, natural=False),
]
for _i, _c in enumerate(MERGE_CASES):
    _c["seed"] = 0x5EED6000 + _i
MERGE_O_NAMES = ["o%d" % k for k in range(MERGE_PARTS)] + ["o", "dout"] + ["do%d" % k for k in range(MERGE_PARTS)]
MERGE_L_NAMES = ["l%d" % k for k in range(MERGE_PARTS)] + ["lse", "dlse"] + ["dl%d" % k for k in range(MERGE_PARTS)]
MERGE_INPUTS = ["o%d" % k for k in range(MERGE_PARTS)] + ["l%d" % k for k in range(MERGE_PARTS)] + ["dout", "dlse"]
MERGE_PART_GAP = 20 * MIB           # batch- and head-far: bytes between the parts' bases


def merge_slots(case):
    """-> (far slots, twin slots, bytes of the twin's buffer).  Dense slots are [B, H, Nq, D] / [B, H, Nq]; packed ones [total, H, D] / [H, total]."""
    dt, B, H, Nq, D, lay = DTYPES[case["dt"]], case["B"], case["H"], case["Nq"], case["D"], case["layout"]
    if lay == "packed":
        slots = place_rows([(n, dt, (Nq, H, D)) for n in MERGE_O_NAMES], PACKED_PITCH_BYTES)
        at = PACKED_LSE_OFFSET
        for n in MERGE_L_NAMES:
            slots[n] = Slot(n, torch.float32, (H, Nq), (Nq, 1), at)
            at += _up(H * Nq * 4, 4096) + 4096
        twin, tbytes = twin_of(slots, keep_pitch=False)
        return slots, twin, tbytes
    slots = {}
    groups = [["o%d" % k, "l%d" % k, "do%d" % k, "dl%d" % k] for k in range(MERGE_PARTS)]      # a part and its gradients start MERGE_PART_GAP after the last
    groups.append(["o", "lse", "dout", "dlse"])
    for gi, names in enumerate(groups):
        specs = [(n, dt, (B, H, Nq, D), D) if n in MERGE_O_NAMES else (n, torch.float32, (B, H, Nq), None) for n in names]
        if lay == "bases":                                           # compact tensors: group 0 at the start, 1 past 2^31, 2 past 2^32, the rest between
            start = (0, FAR_STEP + 5 * 4096, 2 * FAR_STEP + 7 * 4096, FAR_STEP // 2)[gi]
            slots.update(place(specs, None, start=start, gap=4096))
        else:
            slots.update(place(specs, lay, start=gi * MERGE_PART_GAP, gap=32768))
    slots = {n: slots[n] for n in MERGE_O_NAMES + MERGE_L_NAMES}
    twin, tbytes = twin_of(slots)
    return slots, twin, tbytes


def merge_inputs(case):
    """CPU data of a merge case as [B, H, Nq, D] / [B, H, Nq]: the parts' O and LSE (the case's unit; spread over ~40 log2 units), dout, dlse.  Row 0
    is -inf in every part (nobody saw a key), part 1 has further -inf rows; `unwritten`: the rows of o1 that stay poison."""
    g = torch.Generator(device="cpu").manual_seed(case["seed"])
    dt, B, H, Nq, D = DTYPES[case["dt"]], case["B"], case["H"], case["Nq"], case["D"]
    data = {}
    for k in range(MERGE_PARTS):
        o, l = torch.randn((B, H, Nq, D), generator=g).to(dt), torch.randn((B, H, Nq), generator=g) * 6.0
        if k == 1:
            l[torch.rand((B, H, Nq), generator=g) < 0.3] = float("-inf")
        l[:, :, 0] = float("-inf")
        data["o%d" % k], data["l%d" % k] = o, l
    data["dout"], data["dlse"] = torch.randn((B, H, Nq, D), generator=g).to(dt), torch.randn((B, H, Nq), generator=g)
    data["unwritten"] = torch.isneginf(data["l1"])
    return data


def merge_as_slot(case, t):
    """A [B, H, Nq, D] / [B, H, Nq] tensor in the slot's own shape (packed: [total, H, D] / [H, total]), and back (the same call: B = 1)."""
    if case["layout"] != "packed":
        return t
    if t.dim() in (4, 3) and t.shape[0] == 1 and t.shape[1] == case["H"]:
        return t[0].transpose(0, 1) if t.dim() == 4 else t[0]
    return t.transpose(0, 1).unsqueeze(0) if t.dim() == 3 else t.unsqueeze(0)


def merge_images(case, slots, data):
    """What each input slot holds before and after the calls (uint8, the slot's shape, last dimension in bytes); the unwritten rows of o1 are poison."""
    img = {}
    for n in MERGE_INPUTS:
        t = merge_as_slot(case, data[n]).contiguous()
        im = t.view(torch.uint8).clone()
        if n == "o1":
            im[merge_as_slot(case, data["unwritten"].unsqueeze(-1).expand(-1, -1, -1, 1))[..., 0]] = POISON
        assert tuple(im.shape) == tuple(_poison_like(slots[n]).shape), (n, im.shape)
        img[n] = im
    return img

