"""One tiny call per launch route of libfa2_gfx950.so (developer tool): every host-side launcher is reached at least once.

    python tools/launch_routes.py LIB [--out FILE] [--seed S] [--only PREFIX]

LIB is the library to load (a build of another revision for an A/B).  Inputs are seeded, so two libraries that launch the same kernels with the same
arguments produce the same bytes: every output of every route (O, LSE, dQ, dK, dV) is written to FILE as one sha256 line, and two FILEs are compared with
diff.  Under `rocprofv3 --kernel-trace -- python tools/launch_routes.py LIB` the trace lists each route's kernels, grids, workgroup and LDS sizes.
Routes (B1 H2, Nq 130, Nkv 200 unless stated; fp16 and bf16): the plain forward and backward with option asm = 0 at rows 128 / 256 over every head dim that
has kernels or a trim of its own; the default options at D 64 / 128 (hand-scheduled bodies) with each 16 x 16 bit of `asm` cleared once and `kfold` set
once; the short-KV kernels; the split passes at the shapes of tests/test_split_gpu.py; the three bias forms; the six kernel families; the *_lse backwards.
"""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("lib")
ap.add_argument("--out", default=None)
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--only", default="")
args = ap.parse_args()
os.environ["FA2_GFX950_LIB"] = os.path.abspath(args.lib)      # read when rocwmma_fattn._fa2_lib is imported
os.environ["FA2_FRONTEND"] = "py"                              # the compiled front end links against the in-tree library: every call through ctypes

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))
from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import flash_attention, flash_attention_varlen, flash_attn_wmma  # noqa: E402

DEV = torch.device("cuda", 0)
DTYPES = (torch.float16, torch.bfloat16)
LINES = []


def rand(shape, dtype, gen, grad=False):
    t = torch.randn(shape, generator=gen).to(dtype).to(DEV)
    return t.requires_grad_(True) if grad else t


def record(name, **tensors):
    torch.cuda.synchronize()
    for key, t in tensors.items():
        raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
        LINES.append("%s %s %s %s" % (name, key, tuple(t.shape), hashlib.sha256(raw).hexdigest()))
    print(name, flush=True)


def route(name, fn):
    """Run one route; a call the library refuses (an `fa2` error: a route this revision does not have) is recorded as such, anything else ends the run."""
    if not name.startswith(args.only):
        return
    try:
        fn(name)
    except (RuntimeError, ValueError) as e:
        if not str(e).startswith("fa2"):
            raise
        torch.cuda.synchronize()
        LINES.append("%s REFUSED %s" % (name, str(e)[:120]))
        print(name, "refused:", str(e)[:120], flush=True)


def dense(name, dtype, D, Nq=130, Nkv=200, B=1, H=2, Hkv=None, bnhd=False, lse=False, with_bwd=True, **kw):
    """flash_attention forward (+ backward) on seeded inputs; kw goes to flash_attention."""
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    Hkv = Hkv or H
    shp = (lambda h, n: (B, n, h, D)) if bnhd else (lambda h, n: (B, h, n, D))
    q, k, v = rand(shp(H, Nq), dtype, g, with_bwd), rand(shp(Hkv, Nkv), dtype, g, with_bwd), rand(shp(Hkv, Nkv), dtype, g, with_bwd)
    do = rand(shp(H, Nq), dtype, g)
    if "mask" in kw and callable(kw["mask"]):
        kw["mask"] = kw["mask"](B, H, Nq, Nkv, dtype, g)
    if "alibi_slopes" in kw:
        kw["alibi_slopes"] = torch.linspace(0.05, 0.4, H, dtype=torch.float32, device=DEV)
    out = {}
    if lse:
        o, l = flash_attention(q, k, v, BNHD_fmt=bnhd, return_lse=True, **kw)
        dl = torch.randn(l.shape, generator=g).to(DEV)
        out.update(O=o, LSE=l)
        grads = torch.autograd.grad([o, l], [q, k, v], [do, dl])
    else:
        o = flash_attention(q, k, v, BNHD_fmt=bnhd, **kw)
        out.update(O=o)
        grads = torch.autograd.grad([o], [q, k, v], [do]) if with_bwd else ()
    if grads:
        out.update(dQ=grads[0], dK=grads[1], dV=grads[2])
    record(name, **out)


def plain_lse(name, dtype, D, causal, Nkv=200):
    """O and the LSE of the plain forward, as the backward gets them."""
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    q, k, v = rand((1, 2, 130, D), dtype, g), rand((1, 2, Nkv, D), dtype, g), rand((1, 2, Nkv, D), dtype, g)
    ret = flash_attn_wmma.forward(q, k, v, 32 if D > 384 else 64, 128, causal, D ** -0.5, False)
    record(name, O=ret[0], LSE=ret[5])


def packed(name, dtype, D, lse=False, **kw):
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    lq, lk, H = (130, 70), (200, 90), 2
    cu_q = torch.tensor([0, lq[0], sum(lq)], dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([0, lk[0], sum(lk)], dtype=torch.int32, device=DEV)
    q, k, v = rand((sum(lq), H, D), dtype, g, True), rand((sum(lk), H, D), dtype, g, True), rand((sum(lk), H, D), dtype, g, True)
    do = rand((sum(lq), H, D), dtype, g)
    if "alibi_slopes" in kw:
        kw["alibi_slopes"] = torch.linspace(0.05, 0.4, H, dtype=torch.float32, device=DEV)
    out = {}
    if lse:
        o, l = flash_attention_varlen(q, k, v, cu_q, cu_k, max(lq), max(lk), return_lse=True, **kw)
        dl = torch.randn(l.shape, generator=g).to(DEV)
        out.update(O=o, LSE=l)
        grads = torch.autograd.grad([o, l], [q, k, v], [do, dl])
    else:
        o = flash_attention_varlen(q, k, v, cu_q, cu_k, max(lq), max(lk), **kw)
        out.update(O=o)
        grads = torch.autograd.grad([o], [q, k, v], [do])
    out.update(dQ=grads[0], dK=grads[1], dV=grads[2])
    record(name, **out)


def mask_dense(B, H, Nq, Nkv, dtype, g):          # [B, H, Nq, Nkv] additive, I/O dtype: the tile form where Nkv is a multiple of 16 bytes
    return torch.randn((B, H, Nq, Nkv), generator=g).to(dtype).to(DEV)


def mask_pad(B, H, Nq, Nkv, dtype, g):            # [B, 1, 1, Nkv] key-padding: the per-row form
    keep = torch.ones((B, 1, 1, Nkv), dtype=torch.bool)
    keep[..., Nkv - 13:] = False
    return keep.to(DEV)


def mask_pad_long(B, H, Nq, Nkv, dtype, g):
    keep = torch.ones((B, 1, 1, Nkv), dtype=torch.bool)
    keep[..., Nkv - Nkv // 5:] = False
    return keep.to(DEV)


def mask_f32h(B, H, Nq, Nkv, dtype, g):
    return torch.randn((1, H, Nq, Nkv), generator=g).to(DEV)


def tag(dtype):
    return "f16" if dtype == torch.float16 else "bf16"


# ---- plain forward and backward, compiler-scheduled kernels only
for dtype in DTYPES:
    for rows in (128, 256):
        for causal in (False, True):
            for D in (32, 48, 64, 80, 96, 128, 160, 192, 224, 256, 320, 384, 448, 512):
                with _fa2_lib.options(asm=0, rows=rows):
                    nm = "plain/%s/rows%d/causal%d/D%d" % (tag(dtype), rows, causal, D)
                    route(nm, lambda n: dense(n, dtype, D, causal=causal))
                    route(nm + "/lse_of_fwd", lambda n: plain_lse(n, dtype, D, causal))
    with _fa2_lib.options(asm=0):
        route("plain/%s/grouped/D64" % tag(dtype), lambda n: dense(n, dtype, 64, Hkv=1))
        route("plain/%s/grouped/D128" % tag(dtype), lambda n: dense(n, dtype, 128, Hkv=1, causal=True))

# ---- default options: the hand-scheduled bodies; each 16 x 16 bit of `asm` cleared once, `kfold` set once
ASM_DEFAULT = _fa2_lib.load().fa2_get_option(b"asm")
for dtype in DTYPES:
    for D in (64, 128):
        for causal in (False, True):
            nm = "default/%s/causal%d/D%d" % (tag(dtype), causal, D)
            route(nm, lambda n: dense(n, dtype, D, causal=causal))
            route(nm + "/inference", lambda n: dense(n, dtype, D, causal=causal, with_bwd=False))
            route(nm + "/lse_of_fwd", lambda n: plain_lse(n, dtype, D, causal))
    for bit in (64, 128, 256, 512):
        with _fa2_lib.options(asm=ASM_DEFAULT & ~bit):
            route("default/%s/asm_without_%d/D128" % (tag(dtype), bit), lambda n: dense(n, dtype, 128))
            route("default/%s/asm_without_%d/D128/inference" % (tag(dtype), bit), lambda n: dense(n, dtype, 128, with_bwd=False))
    with _fa2_lib.options(kfold=1):
        route("default/%s/kfold/D128" % tag(dtype), lambda n: dense(n, dtype, 128))

# ---- short KV sweeps
for dtype in DTYPES:
    for D in (64, 128):
        for Nkv in (20, 40, 77, 128):
            nm = "short/%s/D%d/Nkv%d" % (tag(dtype), D, Nkv)
            route(nm, lambda n: dense(n, dtype, D, Nkv=Nkv))
            route(nm + "/lse_of_fwd", lambda n: plain_lse(n, dtype, D, False, Nkv=Nkv))

# ---- split passes: the shapes of tests/test_split_gpu.py (SPLIT_SHAPES, BWD_SPLIT_SHAPES, the short-KV backward, MASKED_SPLIT_CASES)
for i, (B, H, Nq, Nkv, D, dt, bnhd) in enumerate([
        (2, 10, 4096, 4096, 64, 0, False), (1, 24, 3072, 3072, 64, 0, False), (1, 24, 4096, 4096, 64, 1, False), (1, 24, 4096, 4096, 128, 0, False),
        (1, 24, 4096, 4096, 128, 1, True), (2, 10, 4000, 3990, 64, 0, False), (2, 10, 4096, 4096, 40, 0, False), (3, 9, 3072, 2048, 96, 0, False),
        (3, 9, 3072, 2048, 80, 0, False), (1, 40, 2048, 8192, 64, 0, True), (1, 32, 1, 8192, 128, 0, False), (4, 8, 1, 16384, 64, 1, False),
        (1, 32, 16, 8200, 128, 1, True), (1, 8, 4096, 4096, 40, 0, False), (1, 4, 2048, 2048, 128, 0, False)]):
    route("split/fwd/%02d" % i, lambda n: dense(n, DTYPES[dt], D, Nq, Nkv, B, H, bnhd=bnhd, with_bwd=False))
for i, (B, H, Nq, Nkv, D, dt, bnhd) in enumerate([
        (2, 10, 4096, 4096, 64, 0, False), (1, 24, 3072, 3072, 64, 1, False), (3, 8, 4096, 4096, 40, 0, False), (2, 20, 2048, 2048, 80, 0, False),
        (2, 10, 4000, 3990, 64, 0, False), (1, 40, 2048, 4096, 64, 0, True), (2, 10, 4096, 77, 64, 0, False), (2, 8, 4096, 77, 40, 1, False),
        (1, 6, 2048, 300, 64, 0, False)]):
    route("split/bwd/%02d" % i, lambda n: dense(n, DTYPES[dt], D, Nq, Nkv, B, H, bnhd=bnhd))
for i, (B, H, Nq, Nkv, D, dt, kind) in enumerate([
        (2, 10, 4096, 77, 64, 0, mask_pad_long), (2, 8, 4096, 77, 40, 1, mask_pad_long), (2, 10, 2048, 77, 64, 0, mask_dense), (2, 10, 2048, 80, 64, 0, mask_dense),
        (1, 6, 2048, 304, 64, 1, mask_f32h), (2, 10, 4096, 4096, 64, 0, mask_pad_long), (1, 24, 3072, 3072, 64, 0, mask_pad_long),
        (1, 24, 4096, 4096, 128, 0, mask_pad_long)]):
    route("split/masked/%02d" % i, lambda n: dense(n, DTYPES[dt], D, Nq, Nkv, B, H, mask=kind))

# ---- bias: aligned dense (tiles), unaligned dense (Nkv 197: one load per score), key padding (one load per KV row)
for dtype in DTYPES:
    for D in (64, 128, 256):
        for causal in (False, True):
            nm = "bias/%s/causal%d/D%d" % (tag(dtype), causal, D)
            route(nm + "/tile", lambda n: dense(n, dtype, D, mask=mask_dense, causal=causal))
            route(nm + "/score", lambda n: dense(n, dtype, D, Nkv=197, mask=mask_dense, causal=causal))
            route(nm + "/row", lambda n: dense(n, dtype, D, mask=mask_pad, causal=causal))

# ---- the six families: forward at rows 128 and 256, backward; D 64, 128, 256, 512
FAMILIES = (("window", dense, dict(window=(40, 10))), ("dropout", dense, dict(dropout_p=0.25, dropout_seed=77, causal=True)),
            ("scoremod", dense, dict(softcap=20.0, alibi_slopes=True, window=(64, 0))),
            ("varlen", packed, dict(causal=True)), ("varlen_dropout", packed, dict(dropout_p=0.25, dropout_seed=77)),
            ("varlen_scoremod", packed, dict(softcap=20.0, alibi_slopes=True, window=(64, 32))))
for dtype in DTYPES:
    for fam, fn, kw in FAMILIES:
        for D in (64, 128, 256, 512):
            for rows in (128, 256):
                with _fa2_lib.options(rows=rows):
                    route("family/%s/%s/rows%d/D%d" % (fam, tag(dtype), rows, D), lambda n: fn(n, dtype, D, **dict(kw)))

# ---- the *_lse backward calls (a gradient for the LSE): dense, windowed, packed
for dtype in DTYPES:
    for D in (64, 128):
        route("lse/dense/%s/D%d" % (tag(dtype), D), lambda n: dense(n, dtype, D, lse=True, causal=True))
        route("lse/window/%s/D%d" % (tag(dtype), D), lambda n: dense(n, dtype, D, lse=True, window=(40, 10)))
        route("lse/varlen/%s/D%d" % (tag(dtype), D), lambda n: packed(n, dtype, D, lse=True, causal=True))

text = "\n".join(LINES) + "\n"
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
print("%d routes, %d outputs, digest of all: %s" % (len(set(l.split()[0] for l in LINES)), len(LINES), hashlib.sha256(text.encode()).hexdigest()))
