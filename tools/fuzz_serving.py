"""Serving traces of the packed step and of the latent cache against float64 (developer tool; the long runs are recorded in profiles/fuzz_runs.md).

tools/fuzz_decode.py's `trace` mode runs the uniform kvcache_append + flash_attention_decode pair the way a server does.  This tool does the same for
the two families that came after it (--mode, draw_case's `force`):
    step   continuous batching on a regular paged cache: every step adds the per-slot token counts to cache_seqlens in place and calls the fused
           flash_attention_prefill / flash_attention_prefill_fp8 (k=, v=, rotary_*=) on a fixed token buffer of T rows that the step fills partly.  A
           slot brings 0 tokens (idle), 1 (a decode row), a small chunk, a chunk that crosses the 64-key tile or a page edge, once per trace more than
           128 rows and in some traces more than 256.  Slots finish and restart with a prompt that is prefilled in 2 or 3 chunks over consecutive steps
           on the recycled, uncleared pages; under a window the pages below its lower edge are freed and handed on.  16-bit and e4m3 caches with
           general descales, window, softcap, slopes, rotary in both pairings, the `rows` option.
    mla    the latent cache: prompts go in through kvcache_append_mla_varlen (several slots packed into one call, slots with zero tokens among them, a
           buffer longer than cu[B]), then every step increments the lengths in place and calls the fused flash_attention_decode_mla(kv_c=, k_pe=,
           rotary_*=) on recycled pages; one slot is parked (length 0, no increment) beside the live ones for its first steps.
The state is tools/fuzz_decode.py's Trace: a CPU image of the whole pool that the append references alone write (kvappend_refs.append_rows per
sequence; mla_append_refs.expect), a last-in-first-out free list, page 0 all NaN behind every unused block-table entry.  After every step O (the owned
rows) and the LSE are held to float64 over the keys gathered from the image (prefill_calls.reference / check_float64; mla_refs.refs under
decode_refs.check); at three drawn steps and at the last the owned pages and page 0 of the device pool are compared with the image bit for bit; at the
end the device's lengths with the host's.  A trace is also replayed from one captured step, bit for bit against the eager trace — every step trace
(the replay's static o is where the rows at and beyond cu[B] have a known fill: they are held to it on every step), every n-th mla trace.

The draw (draw_case, pure Python) is separate from the run (run_case), so that tests/test_fuzz_serving.py can prove coverage, the checker's power
against float64 mutants of the contract and the references' agreement on the CPU.  No case feeds a length outside [0, capacity_keys] or a page id
outside the pool to the GPU.

    python tools/fuzz_serving.py --mode step --cases 300 --seed 1 [--graph-every 10] [--out FILE]
"""
import argparse
import contextlib
import json
import math
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import fuzz_decode as fd  # noqa: E402 - Trace (whose pool holds _nan_like's page 0), _raw, rotary_tables, pattern
import decode_abi as dc  # noqa: E402
import decode_refs as dr  # noqa: E402
import decode_window_refs as wr  # noqa: E402
import key_bars  # noqa: E402
import kvappend_refs as kr  # noqa: E402
import mla_append_refs as ar  # noqa: E402
import mla_refs as mr  # noqa: E402
import prefill_calls as pc  # noqa: E402
from rocwmma_fattn import _fa2_lib  # noqa: E402

_raw, rotary_tables, pattern = fd._raw, fd.rotary_tables, fd.pattern
MODES = ("step", "mla")
DT = fd.DT
TILE = 64                            # the prefill kernels' key tile
MLA_TILE = 32                        # the latent decode's
MAX_KEYS = 640                       # a slot stops taking chunks here: key lengths stay under about 700
MLA_HEADS = [1, 5, 16, 17, 32]


# ---------------------------------------------------------------------------------------------------------------- the draw: step traces
def _split(rng, n, parts):
    """n tokens in `parts` chunks of nearly equal size, a few tokens moved between neighbours"""
    base = [n // parts + (1 if j < n % parts else 0) for j in range(parts)]
    for j in range(parts - 1):
        m = rng.randint(-3, 3)
        if base[j] + m >= 1 and base[j + 1] - m >= 1:
            base[j], base[j + 1] = base[j] + m, base[j + 1] - m
    return base


def _draw_plan(rng, B, page, steps, T, wl, big):
    """-> (plan [steps][B]: the tokens every slot brings, restarts [(step, slot, chunks)]).  A prompt waits in its slot's queue and goes in chunk by
    chunk over consecutive steps; a slot without one draws what it brings from the kinds of the module docstring."""
    queue = [_split(rng, rng.randint(40, 160), rng.choice([1, 2])) for _ in range(B)]
    queue[0] = [rng.randint(257, T - 30)] if big else [rng.randint(129, 200), rng.randint(5, 40)]
    restarts = []
    for n, slot in enumerate(rng.sample(range(1, B), rng.randint(1, 2))):
        if n == 0 and wl >= 0:                       # three chunks; the third arrives when the window's lower edge has left the prompt's first page
            total, parts = wl + 2 * page + rng.randint(5, 40), 3
        else:
            total, parts = rng.randint(page // 2, page + 80), rng.choice([2, 3])
        total += total % page == 0
        restarts.append((rng.randint(8, steps - 8), slot, _split(rng, total, parts)))
    restarts.sort()
    lens, plan = [0] * B, []
    for s in range(steps):
        for (st, slot, chunks) in restarts:
            if st == s:
                lens[slot], queue[slot] = 0, list(chunks)
        budget, nq = T - 1, [0] * B                  # cu[B] < T: the step fills the token buffer partly
        for b in sorted(range(B), key=lambda b: not queue[b]):
            if queue[b]:
                if queue[b][0] <= budget:
                    nq[b] = queue[b].pop(0)
            elif lens[b] > 0:
                kind = rng.choice(["idle", "decode", "decode", "decode", "decode", "small", "small", "tile", "page"])
                n = {"idle": 0, "decode": 1, "small": rng.randint(2, 9), "tile": TILE - lens[b] % TILE + rng.randint(1, 8),
                     "page": page - lens[b] % page + rng.randint(1, 8)}[kind]
                if lens[b] + n > MAX_KEYS:
                    n = min(n, 1)
                nq[b] = n if n <= budget else min(1, budget)
            budget -= nq[b]
            lens[b] += nq[b]
        plan.append(nq)
    return plan, restarts


def step_walk(d):
    """[(restarted slots, tokens per slot, lengths before the step's increment, after it)] of a step trace"""
    lens, out = [0] * d["B"], []
    for s in range(d["steps"]):
        rs = [slot for (st, slot, _) in d["restarts"] if st == s]
        for b in rs:
            lens[b] = 0
        before = list(lens)
        lens = [n + q for n, q in zip(lens, d["plan"][s])]
        out.append((rs, d["plan"][s], before, list(lens)))
    return out


def step_pages(d):
    """The page traffic of a step trace, mirrored in pure Python from fd.Trace's discipline (release, then per slot: free below the window, hand out;
    a last-in-first-out free list; tests/test_fuzz_serving.py holds it to StepTrace's own maps): per step a list of (taker, logical page, the slot
    whose WINDOW freed the page last or None) for every hand-out, and every slot's {logical page: the mirror's page id} after it."""
    page, wl, B = d["page"], d["window_left"], d["B"]
    free, freed_by, owned, out = list(range(10 ** 4, 0, -1)), {}, [dict() for _ in range(B)], []
    for rs, nq, before, after in step_walk(d):
        takes = []
        for b in rs:
            for j in sorted(owned[b]):
                freed_by.pop(owned[b][j], None)
                free.append(owned[b][j])
            owned[b] = {}
        for b in range(B):
            lo = wr.window_lo(after[b], nq[b], wl)
            for j in [j for j in owned[b] if (j + 1) * page <= lo]:
                pid = owned[b].pop(j)
                freed_by[pid] = b
                free.append(pid)
            for j in range(-(-after[b] // page)):
                if j not in owned[b] and (j + 1) * page > lo:
                    owned[b][j] = free.pop()
                    takes.append((b, j, freed_by.pop(owned[b][j], None)))
        out.append((takes, [dict(o) for o in owned]))
    return out


def step_facts(d):
    """what a step trace reaches, by name -> bool (coverage's conditions, and what the draw insists on)"""
    page, wl, walk = d["page"], d["window_left"], step_walk(d)
    f = dict.fromkeys(("idle beside chunk", "decode beside chunk", "chunk across a page edge", "chunk across a tile edge", "chunk over 128", "chunk over 256",
                       "a page freed by a window taken by another slot", "prompt chunk past its first page's window"), False)
    pending = [[] for _ in range(d["B"])]            # the chunks of a restarted slot's prompt that have not gone in yet; [..., 0]: how many have
    for s, ((rs, nq, before, after), (takes, _)) in enumerate(zip(walk, step_pages(d))):
        for (st, slot, ch) in d["restarts"]:
            if st == s:
                pending[slot] = list(ch) + [0]
        chunk = any(n >= 2 for n in nq)
        f["idle beside chunk"] |= chunk and 0 in nq
        f["decode beside chunk"] |= chunk and 1 in nq
        f["chunk over 128"] |= max(nq) > 128
        f["chunk over 256"] |= max(nq) > 256
        f["a page freed by a window taken by another slot"] |= any(by is not None and by != b for b, _, by in takes)
        for b, n in enumerate(nq):
            if n >= 2:
                f["chunk across a page edge"] |= before[b] % page != 0 and before[b] // page + 1 == (after[b] - 1) // page
                f["chunk across a tile edge"] |= before[b] // TILE != (after[b] - 1) // TILE
            if len(pending[b]) > 1 and n == pending[b][0]:           # (a slot with a prompt in its queue brings its next chunk or nothing)
                later = pending[b][-1] >= 1
                pending[b] = pending[b][1:-1] + [pending[b][-1] + 1]
                f["prompt chunk past its first page's window"] |= later and wl >= 0 and wr.window_lo(after[b], n, wl) >= page
    return f


def _draw_step(i, rng):
    while True:
        B, page, steps, T = rng.randint(3, 5), rng.choice([64, 128]), rng.randint(25, 40), rng.randint(300, 400)
        wl = rng.choice([-1, 40, 70])
        plan, restarts = _draw_plan(rng, B, page, steps, T, wl, big=i % 3 == 0)
        D = rng.choice([64, 128])
        d = dict(mode="step", i=i, seed=rng.getrandbits(48), dtype=rng.choice(["f16", "bf16"]), D=D, Hkv=rng.choice([1, 2, 4]), G=rng.choice([1, 2, 4, 8]), B=B,
                 page=page, steps=steps, T=T, window_left=wl, softcap=rng.choice([0.0, 0.0, 30.0]), slopes=rng.choice([None, "H", "BH"]), fp8=rng.random() < 0.5,
                 rot=rng.choice([32, D]), inter=rng.random() < 0.5, rows=rng.choice([128, 256] if i % 3 == 0 else [0, 128, 256]), plan=plan, restarts=restarts,
                 check_steps=sorted(rng.sample(range(steps), 3)), graph=False)
        d["capacity"] = -(-max(max(after) for _, _, _, after in step_walk(d)) // page) + 1
        f = step_facts(d)
        if f["chunk over 128"] and f["chunk across a page edge"] and f["chunk across a tile edge"] and f["idle beside chunk"] and \
                (wl < 0 or (f["a page freed by a window taken by another slot"] and f["prompt chunk past its first page's window"])):
            return d


# ---------------------------------------------------------------------------------------------------------------- the draw: mla traces
def mla_walk(d):
    """[(lengths before the step's increment, after it, the increments)] of an mla trace: a restarted slot begins at its prompt's length; the parked
    slot stays at 0 and takes no increment during its first `park` steps"""
    lens, out = list(d["prompts"]), []
    for s in range(d["steps"]):
        for (st, slot, n) in d["events"]:
            if st == s:
                lens[slot] = n
        inc = [0 if (b == d["park_slot"] and s < d["park"]) else d["Nq"] for b in range(d["B"])]
        before = list(lens)
        lens = [n + a for n, a in zip(lens, inc)]
        out.append((before, list(lens), inc))
    return out


def mla_empty_part(d):
    """under a forced split, a live slot so short that a part sweeps no 32-key tile"""
    ns = d["num_splits"]
    tiles = [-(-n // MLA_TILE) for _, after, _ in mla_walk(d) for n in after if n]
    return ns >= 2 and any((ns - 1) * -(-t // ns) >= t for t in tiles)


def _draw_mla(i, rng):
    while True:
        B, page, steps, nq = rng.randint(3, 5), rng.choice([64, 128]), rng.randint(30, 50), rng.randint(1, 3)
        prompts = [rng.choice([1, 2]) * page - rng.randint(1, 30) for _ in range(B)]
        park_slot = rng.randrange(B)
        prompts[park_slot] = 0                       # the zero-token slot of the first packed prompt call
        events = []
        for slot in rng.sample(range(B), rng.randint(1, 2)):
            n = rng.choice([rng.randint(1, 40), rng.randint(1, page + 20)])
            events.append((rng.randint(8, steps - 8), slot, n + (n % page == 0)))
        d = dict(mode="mla", i=i, seed=rng.getrandbits(48), dtype=rng.choice(["f16", "bf16"]), H=rng.choice(MLA_HEADS), Nq=nq, B=B, page=page, steps=steps,
                 num_splits=rng.choice([0, 1, 3]), table=rng.choice(["f32", "io"]), inter=rng.random() < 0.5, prompts=prompts, park_slot=park_slot,
                 park=rng.randint(2, 5), events=sorted(events), pad=rng.randint(1, 7), check_steps=sorted(rng.sample(range(steps), 3)), graph=False)
        d["capacity"] = -(-max(max(after) for _, after, _ in mla_walk(d)) // page) + 1
        if all(st >= d["park"] or slot != park_slot for (st, slot, _) in events):
            return d


def draw_case(i, rng, force=None):
    """Trace i of a sweep as a dict that describes it completely; force: "step" | "mla" (None: step).  Pure Python."""
    return (_draw_mla if force == "mla" else _draw_step)(i, rng)


def draw_sweep(seed, counts):
    """The traces of a sweep: counts = [(force, n), ...] drawn in that order from one generator."""
    rng = random.Random(seed)
    out = []
    for force, n in counts:
        for _ in range(n):
            out.append(draw_case(len(out), rng, force))
    return out


# the slices of tests/test_fuzz_serving_gpu.py; tests/test_fuzz_serving.py proves on the CPU what these seeds reach
STEP_SEED, STEP_COUNTS = 3, [("step", 6)]
MLA_SEED, MLA_COUNTS = 3, [("mla", 4)]


def coverage(descs):
    """What a list of drawn traces reaches, as counts by name (the slices of tests/test_fuzz_serving_gpu.py must have every one of them >= 1)."""
    c = {}

    def hit(name, cond=True):
        c[name] = c.get(name, 0) + int(bool(cond))
    for d in descs:
        if d["mode"] == "step":
            f, wl = step_facts(d), d["window_left"]
            hit("an idle slot beside a chunk in one launch", f["idle beside chunk"])
            hit("a decode row beside a chunk", f["decode beside chunk"])
            hit("a chunk whose first row sits mid-page and whose last row sits in the next page", f["chunk across a page edge"])
            hit("a chunk across the 64-key tile", f["chunk across a tile edge"])
            hit("a chunk over 128 rows", f["chunk over 128"])
            hit("a chunk over 256 rows", f["chunk over 256"])
            for r in (128, 256):                     # both workgroup shapes, pinned, meet a block edge inside a sequence
                hit("a chunk over 256 rows under rows %d" % r, f["chunk over 256"] and d["rows"] == r)
            hit("a prompt prefilled in three chunks", any(len(ch) == 3 for _, _, ch in d["restarts"]))
            hit("a prompt prefilled in two chunks", any(len(ch) == 2 for _, _, ch in d["restarts"]))
            hit("a restart on recycled pages that does not end on a page edge", any(sum(ch) % d["page"] for _, _, ch in d["restarts"]))
            hit("a window edge crossing into a freed page", f["a page freed by a window taken by another slot"])
            hit("a prompt chunk admitted while the window excludes its first page", f["prompt chunk past its first page's window"])
            hit("an e4m3 trace with a window", d["fp8"] and wl >= 0)
            hit("a 16-bit trace with a window", not d["fp8"] and wl >= 0)
            hit("an e4m3 trace without a window", d["fp8"] and wl < 0)
            for r in (128, 256):
                hit("a step trace under rows %d" % r, d["rows"] == r)
            hit("a step trace under the plan's rows", d["rows"] == 0)
            hit("a step trace with a cap", d["softcap"] > 0)
            hit("a step trace with slopes [B, H]", d["slopes"] == "BH")
        else:
            hit("an mla trace whose forced split leaves a part empty for a short slot", mla_empty_part(d))
            hit("an mla packed prompt call with a zero-token slot", 0 in d["prompts"] and len(d["events"]) > 0 and d["B"] > 1)
            hit("an mla trace with a parked slot beside live ones", d["park"] > 0)
            hit("an mla restart that does not end on a page edge", any(n % d["page"] for _, _, n in d["events"]))
            hit("an mla trace with Nq > 1", d["Nq"] > 1)
            hit("an mla trace with a head count that is no multiple of 16", d["H"] % 16)
            hit("an mla trace with 16-bit tables", d["table"] == "io")
            hit("an mla trace under the plan's own split", d["num_splits"] == 0)
    return c


# ---------------------------------------------------------------------------------------------------------------- shrink
def cut_steps(d, n):
    """the first n steps of a trace (the pool's size, and with it the random stream of the steps kept, unchanged)"""
    c = dict(d, steps=n, check_steps=[s for s in d["check_steps"] if s < n])
    if d["mode"] == "step":
        c.update(plan=d["plan"][:n], restarts=[r for r in d["restarts"] if r[0] < n])
    else:
        c.update(events=[e for e in d["events"] if e[0] < n])
    return c


def drop_slot(d, b):
    """the trace without slot b"""
    move = lambda x: x - (x > b)          # noqa: E731
    if d["mode"] == "step":
        return dict(d, B=d["B"] - 1, plan=[nq[:b] + nq[b + 1:] for nq in d["plan"]], restarts=[(s, move(x), ch) for (s, x, ch) in d["restarts"] if x != b])
    parked = d["park_slot"] == b
    return dict(d, B=d["B"] - 1, prompts=d["prompts"][:b] + d["prompts"][b + 1:], events=[(s, move(x), n) for (s, x, n) in d["events"] if x != b],
                park_slot=-1 if parked else move(d["park_slot"]), park=0 if parked else d["park"])


def shrink(desc, still_fails):
    """Greedy reduction of a failing trace: the shortest prefix of its steps that still fails (by bisection: a prefix repeats the longer trace's steps
    exactly), then slots dropped one at a time, then window, cap, slopes and fp8 turned off one at a time; a change is kept only while
    still_fails(candidate) holds.  -> the smallest description found."""
    d = dict(desc)
    lo, hi = 1, d["steps"]
    while lo < hi:
        mid = (lo + hi) // 2
        if still_fails(cut_steps(d, mid)):
            hi = mid
        else:
            lo = mid + 1
    d = cut_steps(d, hi)
    for b in range(d["B"] - 1, -1, -1):
        if d["B"] > 1:
            c = drop_slot(d, b)
            if still_fails(c):
                d = c
    for key, off in (("window_left", -1), ("softcap", 0.0), ("slopes", None), ("fp8", False), ("rows", 0)):
        if key in d and d[key] != off:
            c = dict(d, **{key: off})
            if still_fails(c):
                d = c
    return d


# ---------------------------------------------------------------------------------------------------------------- step traces: state and references
class StepTrace(fd.Trace):
    """fd.Trace with a token count per slot and step: the pool image, the free list, the hand-outs and the frees below the window are the base's."""

    def __init__(self, desc, dev=None):
        super().__init__(dict(desc, prompts=[], Nq=0), dev)
        self.nq, self.T, self.s = [0] * desc["B"], desc["T"], -1

    def _hand_out(self, b, whole=False):
        self.d["Nq"] = self.nq[b]
        super()._hand_out(b, whole)

    def _free_below_window(self, b):
        self.d["Nq"] = self.nq[b]
        super()._free_below_window(b)

    def begin_step(self, s):
        """the host's work in front of step s: finished slots restart empty, the lengths grow by the step's counts (the CPU's copy), pages are freed and
        handed out -> cu (a list), the new tokens q, k, v [T, heads, D]"""
        d = self.d
        for (st, slot, _) in d["restarts"]:
            if st == s:
                self.release(slot)
                self.lens[slot] = 0
                if self.dev is not None:
                    self.dlens[slot] = 0
        self.s, self.nq = s, list(d["plan"][s])
        for b in range(d["B"]):
            self.lens[b] += self.nq[b]
            self._free_below_window(b)
            self._hand_out(b)
        cu = [0]
        for n in self.nq:
            cu.append(cu[-1] + n)
        return (cu,) + tuple((2 * fd._randn((self.T, h, d["D"]), self.g)).to(self.dt) for h in (self.H, d["Hkv"], d["Hkv"]))

    def rows_of(self, b, cu, k, v, q=None, lens=None):
        """kvappend_refs.append_rows on sequence b's packed rows -> (K rows, V rows, rotated q) [Nq_b, heads, D]"""
        r = slice(cu[b], cu[b + 1])
        kd, vd = (None if t is None else t[b:b + 1] for t in (self.kd, self.vd))
        rk, rv, qr = kr.append_rows(k[r][None], v[r][None], [self.lens[b] if lens is None else lens], q=None if q is None else q[r][None], cos=self.cos,
                                    sin=self.sin, inter=self.d["inter"], fp8=self.d["fp8"], kd=kd, vd=vd)
        return rk[0], rv[0], None if qr is None else qr[0]

    def apply_step(self, cu, q, k, v, position_i=False):
        """the append reference on the CPU image -> the rotated q [T, H, D] (rows at and beyond cu[B]: q's own bits).  position_i: the image mutant
        that rotates K by the token's index in its chunk."""
        q_rot = q.clone()
        for b, n in enumerate(self.nq):
            if n:
                rk, rv, qr = self.rows_of(b, cu, k, v, q)
                if position_i:
                    rk = self.rows_of(b, cu, k, v, lens=n)[0]
                self._write(b, rk, rv, n)
                q_rot[cu[b]:cu[b + 1]] = qr
        return q_rot

    def keys(self, b, n=None, slot=None):
        """sequence b's keys [0, n) from the image, dequantised exactly under ITS descales (slot: read another slot's pages) -> k, v f32 [n, Hkv, D]"""
        k, v = self.gather(b if slot is None else slot, self.lens[b] if n is None else n)
        kd, vd = (1.0 if t is None else t[b].float()[None, :, None] for t in (self.kd, self.vd))
        return k.float() * kd, v.float() * vd

    def reference(self, cu, q_rot):
        """prefill_calls.reference over the keys gathered from the image -> (o [total, H, D], log2 lse [H, total], the O bar)"""
        ks, vs = zip(*[self.keys(b) for b in range(self.d["B"])])
        return pc.reference(q_rot[:cu[-1]], torch.tensor(cu, dtype=torch.int32), ks, vs, self.scale, self.d["window_left"], self.d["softcap"], self.slopes)

    def mismatches(self, pools):
        """elements of the pages some slot owns, and of the all-NaN page 0, that differ between `pools` (CPU) and the image"""
        pids = [0] + sorted(p for o in self.owned for p in o.values())
        return sum(int((_raw(dp)[pids] != _raw(cp)[pids]).sum()) for dp, cp in zip(pools, self.pool))


def fill_rows(shape, dt):
    """what the rows of o at and beyond cu[B] hold before a launch: a finite pattern no result equals"""
    n = 1
    for x in shape:
        n *= x
    return (pattern(2 * n, 3).view(torch.int16).reshape(shape) & 0x3FFF).view(dt)


def check_step(tag, o, lse2, ref, total, fill=None):
    """-> failures of one step: the owned rows of o [T, H, D] and the log2 lse [H, T] against prefill_calls.check_float64; with `fill` [T, H, D], the
    rows at and beyond cu[B] bit for bit what they held before the launch"""
    ro, rl, bar = ref
    o, lse2 = o.detach().cpu(), lse2.detach().cpu()
    fails = pc.check_float64(tag, o[:total], lse2[:, :total], (ro[:total], rl[:, :total], bar[:total])) if total else []
    if fill is not None and not torch.equal(o[total:].double(), fill[total:].double()):
        fails.append("%s: rows of o at or beyond cu[B] were written" % tag)
    return fails


def step_figures(o, lse2, ref, total):
    ro, rl, bar = ref
    if not total:
        return 0.0, 0.0
    o, lse2 = o.detach().cpu().double()[:total], lse2.detach().cpu().double()[:, :total]
    ratio = key_bars.ratio_max((o - ro[:total]).abs(), bar[:total]) if bool(torch.isfinite(o).all()) else float("inf")
    live = ~torch.isinf(rl[:, :total])
    e = float((lse2 - rl[:, :total])[live].abs().max()) if bool(live.any()) else 0.0
    return ratio, e if math.isfinite(e) else float("inf")


def _prefill(tr, q, k, v, cu, lens):
    from rocwmma_fattn import FlashAttn
    d = tr.d
    kw = dict(k_descale=tr.dkd, v_descale=tr.dvd) if d["fp8"] else {}
    fn = FlashAttn.flash_attention_prefill_fp8 if d["fp8"] else FlashAttn.flash_attention_prefill
    return fn(q, tr.dpool[0], tr.dpool[1], cu, lens, tr.dbt, max_seqlen_q=tr.T, k=k, v=v, rotary_cos=tr.dcos, rotary_sin=tr.dsin, rotary_interleaved=d["inter"],
              window=None if d["window_left"] < 0 else (d["window_left"], 0), softcap=d["softcap"], alibi_slopes=tr.dslopes, return_lse=True, **kw)


def _rows_option(desc):
    return _fa2_lib.options(rows=desc["rows"]) if desc.get("rows") else contextlib.nullcontext()


def _run_step(desc, graph=False, keep=None):
    """The eager trace (graph=False) or its replay from one captured step.  keep: a list that receives every step's owned (o, lse) on the CPU."""
    from rocwmma_fattn import FlashAttn
    dev = torch.device("cuda", torch.cuda.current_device())
    tr = StepTrace(desc, dev)
    B, T, D = desc["B"], desc["T"], desc["D"]
    fails, ratio, lerr, wrong, filled = [], 0.0, 0.0, 0, 0
    fill = fill_rows((T, tr.H, D), tr.dt)
    with _rows_option(desc):
        dcu, dinc = torch.zeros(B + 1, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        if graph:                                    # one step — the in-place increment and the fused call — captured on a side stream, single-stream
            qi, ki, vi = (torch.zeros((T, h, D), dtype=tr.dt, device=dev) for h in (tr.H, desc["Hkv"], desc["Hkv"]))
            scratch = (tr.dpool, tr.dlens)
            tr.dpool, tr.dlens = [t.clone() for t in tr.dpool], tr.dlens.clone()
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):            # warm-up outside the capture, on a pool and lengths of its own
                tr.dlens.add_(dinc)
                _prefill(tr, qi, ki, vi, dcu, tr.dlens)
            torch.cuda.current_stream().wait_stream(side)
            tr.dpool, tr.dlens = scratch
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(cg, stream=side):
                    tr.dlens.add_(dinc)
                    go, gl = _prefill(tr, qi, ki, vi, dcu, tr.dlens)
            torch.cuda.current_stream().wait_stream(side)
        for s in range(desc["steps"]):
            cu, q, k, v = tr.begin_step(s)
            total = cu[-1]
            dcu.copy_(torch.tensor(cu, dtype=torch.int32))
            dinc.copy_(torch.tensor(tr.nq, dtype=torch.int32))
            known = None
            if graph:
                qi.copy_(q.to(dev))
                ki.copy_(k.to(dev))
                vi.copy_(v.to(dev))
                go.copy_(fill.to(dev))
                gl.zero_()
                cg.replay()
                o, lse, known = go, gl, fill
            else:                                    # (the operator allocates o itself: what its unowned rows held before is the replay's to know)
                tr.dlens.add_(dinc)
                o, lse = _prefill(tr, q.to(dev), k.to(dev), v.to(dev), dcu, tr.dlens)
            torch.cuda.synchronize()
            filled += known is not None
            ref = tr.reference(cu, tr.apply_step(cu, q, k, v))
            lse2 = lse / FlashAttn._LN2
            fails += check_step("trace %d step %d" % (desc["i"], s), o, lse2, ref, total, known)
            r, e = step_figures(o, lse2, ref, total)
            ratio, lerr = max(ratio, r), max(lerr, e)
            if keep is not None:
                keep.append((o[:total].cpu().clone(), lse[:, :total].cpu().clone()))
            if s in desc["check_steps"] or s == desc["steps"] - 1:
                bad = tr.mismatches([t.cpu() for t in tr.dpool])
                wrong += bad
                if bad:
                    fails.append("step %d: %d elements of the owned pages and page 0 differ from the image" % (s, bad))
            if len(fails) > 8:
                break
    if tr.dlens.cpu().tolist() != tr.lens:
        fails.append("the device's lengths %s, the host's %s" % (tr.dlens.cpu().tolist(), tr.lens))
    return dict(desc, fails=fails, o_ratio=ratio, lse_err=lerr, wrong=wrong, steps_run=s + 1, recycled=len(tr.recycled), fill_checked=filled)


# ---------------------------------------------------------------------------------------------------------------- mla traces: state and references
class MlaTrace(fd.Trace):
    """fd.Trace on a latent pool: one head of 576 columns, K and V at once (the base's K pool; its V pool is dropped), written by
    mla_append_refs.expect alone."""

    def __init__(self, desc, dev=None):
        super().__init__(dict(desc, prompts=[], Hkv=1, G=desc["H"], D=mr.D, fp8=False, rot=ar.ROT, slopes=None, window_left=-1, softcap=0.0), dev)
        self.pool, self.prompts = self.pool[:1], list(desc["prompts"])
        self.scale = mr.SCALE
        if desc["table"] == "io":
            self.cos, self.sin = self.cos.to(self.dt), self.sin.to(self.dt)
        if dev is not None:
            self.dpool = self.dpool[:1]
            self.dcos, self.dsin = self.cos.to(dev), self.sin.to(dev)
            self.dlat = self.dpool[0][:, :, 0]
        self.inc = [0] * desc["B"]

    def latent(self):
        return self.pool[0][:, :, 0]

    def _expect(self, kv_c, k_pe, owners, q):
        img, q_out = ar.expect(self.latent(), kv_c, k_pe, owners, self.lens, block_table=self.bt, q=q, cos=self.cos, sin=self.sin, inter=self.d["inter"])
        _raw(self.pool[0])[:, :, 0] = _raw(img)
        return q_out

    def admit(self, slots):
        """slots [(b, n)] end and take prompts of n tokens, all in ONE packed call over the B slots (the others bring zero tokens) on a buffer `pad`
        rows longer than cu[B] -> failures (the device's q_out against the reference's, bit for bit)"""
        from rocwmma_fattn import FlashAttn
        d, new = self.d, dict(slots)
        for b, n in slots:
            self.release(b)
            self.lens[b] = n
            self._hand_out(b, whole=True)
        counts = [new.get(b, 0) for b in range(d["B"])]
        owners = [(b, i, n) for b, n in enumerate(counts) for i in range(n)] + [None] * d["pad"]
        kv_c, k_pe, q = (fd._randn((len(owners),) + tail, self.g).to(self.dt) for tail in ((mr.DV,), (ar.ROT,), (d["H"], mr.D)))
        want = self._expect(kv_c, k_pe, owners, q)
        if self.dev is None:
            return []
        for b, n in slots:
            self.dlens[b] = n
        cu = torch.tensor([0] + list(torch.tensor(counts).cumsum(0).tolist()), dtype=torch.int32, device=self.dev)
        got = FlashAttn.kvcache_append_mla_varlen(self.dlat, kv_c.to(self.dev), k_pe.to(self.dev), cu, self.dlens, block_table=self.dbt, rotary_cos=self.dcos,
                                                  rotary_sin=self.dsin, rotary_interleaved=d["inter"], q=q.to(self.dev))
        torch.cuda.synchronize()
        bad = int((_raw(got.cpu()) != _raw(want)).sum())
        return ["prompt call of slots %s: %d elements of q_out differ" % ([b for b, _ in slots], bad)] if bad else []

    def begin_step(self, s):
        """the host's work in front of step s -> failures of the prompt call (if any), the new tokens q [B, Nq, H, 576], kv_c, k_pe"""
        d = self.d
        slots = [(slot, n) for (st, slot, n) in d["events"] if st == s]
        if s == 0:
            slots = list(enumerate(self.prompts))
        fails = self.admit(slots) if slots else []
        self.inc = [0 if (b == d["park_slot"] and s < d["park"]) else d["Nq"] for b in range(d["B"])]
        for b in range(d["B"]):
            self.lens[b] += self.inc[b]
            self._hand_out(b)
        B, nq = d["B"], d["Nq"]
        return (fails,) + tuple(fd._randn((B, nq) + tail, self.g).to(self.dt) for tail in ((d["H"], mr.D), (mr.DV,), (ar.ROT,)))

    def apply_step(self, q, kv_c, k_pe):
        """mla_append_refs.expect on the image -> the rotated q [B, Nq, H, 576]"""
        B, nq = self.d["B"], self.d["Nq"]
        q_out = self._expect(kv_c.reshape(B * nq, -1), k_pe.reshape(B * nq, -1), ar.uniform_owners(B, nq), q.reshape(B * nq, self.d["H"], mr.D))
        return q_out.reshape(q.shape)

    def rows(self, lens=None):
        """the latent rows [B, max len, 576] of every slot from the image (lens: as if the slots had these lengths)"""
        lens = self.lens if lens is None else lens
        kv = torch.zeros((self.d["B"], max(max(lens), 1), mr.D), dtype=self.dt)
        for b, n in enumerate(lens):
            if n:
                kv[b, :n] = self.gather(b, n)[0][:, 0]
        return kv

    def refs(self, q_rot):
        return mr.refs(q_rot, self.rows(), self.lens, dc.code(self.dt))

    def mismatches(self, pools):
        pids = [0] + sorted(p for o in self.owned for p in o.values())
        return int((_raw(pools[0])[pids] != _raw(self.pool[0])[pids]).sum())


def mla_checked(o, lse2, refs, lens, code, tag):
    """tests/decode_refs.py: check (the oracle's bars and float64's), as a list of failures"""
    try:
        dr.check(o, lse2, refs, lens, code, tag)
    except AssertionError as e:
        return ["%s" % (e.args[0],) if e.args else "check failed"]
    return []


def mla_oracle_outputs(refs, B, nq, H):
    """(o [B, Nq, H, 512], log2 lse [B, H, Nq]) of the oracle: what tests/test_fuzz_serving.py feeds the checker in a kernel's place"""
    o, lse = torch.zeros((B, nq, H, mr.DV)), torch.full((B, H, nq), float("-inf"))
    for b, r in enumerate(refs):
        if r is not None:
            live = torch.from_numpy(~r[4])
            o[b][live] = torch.from_numpy(r[0][0]).float().transpose(0, 1)[live]
            lse[b][:, live] = torch.from_numpy(r[1][0]).float()[:, live]
    return o, lse


def mla_figures(o, lse2, refs, code):
    import numpy as np
    from conftest import FLOOR
    ratio = lerr = 0.0
    go, gl = o.detach().float().cpu(), lse2.detach().float().cpu()
    for b, r in enumerate(refs):
        if r is None:
            continue
        e = float(np.abs(go[b].transpose(0, 1).numpy() - r[2][0]).max()) / (2 * FLOOR[code])
        ratio = max(ratio, e if math.isfinite(e) else float("inf"))
        live = ~r[4]
        if live.any():
            e = float(np.abs(gl[b].numpy()[:, live] - r[3][0][:, live]).max())
            lerr = max(lerr, e if math.isfinite(e) else float("inf"))
    return ratio, lerr


def _decode_mla(tr, q, kv_c, k_pe, lens):
    from rocwmma_fattn import FlashAttn
    return FlashAttn.flash_attention_decode_mla(q, tr.dlat, lens, block_table=tr.dbt, return_lse=True, num_splits=tr.d["num_splits"], kv_c=kv_c, k_pe=k_pe,
                                                rotary_cos=tr.dcos, rotary_sin=tr.dsin, rotary_interleaved=tr.d["inter"])


def _run_mla(desc, graph=False, keep=None):
    """The eager trace (graph=False) or its replay from one captured step.  keep: a list that receives every step's (o, lse) on the CPU."""
    from rocwmma_fattn import FlashAttn
    dev = torch.device("cuda", torch.cuda.current_device())
    tr = MlaTrace(desc, dev)
    B, nq, H = desc["B"], desc["Nq"], desc["H"]
    code = dc.code(tr.dt)
    fails, ratio, lerr, wrong = [], 0.0, 0.0, 0
    dinc = torch.zeros(B, dtype=torch.int32, device=dev)
    if graph:
        qi, ci, pi = (torch.zeros((B, nq) + tail, dtype=tr.dt, device=dev) for tail in ((H, mr.D), (mr.DV,), (ar.ROT,)))
        scratch = (tr.dpool, tr.dlat, tr.dlens)
        tr.dpool, tr.dlens = [t.clone() for t in tr.dpool], tr.dlens.clone()
        tr.dlat = tr.dpool[0][:, :, 0]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                # warm-up outside the capture, on a pool and lengths of its own
            tr.dlens.add_(dinc)
            _decode_mla(tr, qi, ci, pi, tr.dlens)
        torch.cuda.current_stream().wait_stream(side)
        tr.dpool, tr.dlat, tr.dlens = scratch
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(cg, stream=side):
                tr.dlens.add_(dinc)
                go, gl = _decode_mla(tr, qi, ci, pi, tr.dlens)
        torch.cuda.current_stream().wait_stream(side)
    for s in range(desc["steps"]):
        pf, q, kv_c, k_pe = tr.begin_step(s)
        fails += pf
        dinc.copy_(torch.tensor(tr.inc, dtype=torch.int32))
        if graph:
            qi.copy_(q.to(dev))
            ci.copy_(kv_c.to(dev))
            pi.copy_(k_pe.to(dev))
            go.zero_()
            gl.zero_()
            cg.replay()
            o, lse = go, gl
        else:
            tr.dlens.add_(dinc)
            o, lse = _decode_mla(tr, q.to(dev), kv_c.to(dev), k_pe.to(dev), tr.dlens)
        torch.cuda.synchronize()
        refs = tr.refs(tr.apply_step(q, kv_c, k_pe))
        lse2 = lse / FlashAttn._LN2
        fails += mla_checked(o, lse2, refs, tr.lens, code, "mla trace %d step %d" % (desc["i"], s))
        r, e = mla_figures(o, lse2, refs, code)
        ratio, lerr = max(ratio, r), max(lerr, e)
        if keep is not None:
            keep.append((o.cpu().clone(), lse.cpu().clone()))
        if s in desc["check_steps"] or s == desc["steps"] - 1:
            bad = tr.mismatches([t.cpu() for t in tr.dpool])
            wrong += bad
            if bad:
                fails.append("step %d: %d elements of the owned pages and page 0 differ from the image" % (s, bad))
        if len(fails) > 8:
            break
    if tr.dlens.cpu().tolist() != tr.lens:
        fails.append("the device's lengths %s, the host's %s" % (tr.dlens.cpu().tolist(), tr.lens))
    return dict(desc, fails=fails, o_ratio=ratio, lse_err=lerr, wrong=wrong, steps_run=s + 1, recycled=len(tr.recycled))


# ---------------------------------------------------------------------------------------------------------------- run
def run_with_graph(desc):
    """the eager trace, then the same trace replayed from a captured step: every step's O and LSE bit for bit"""
    run = _run_mla if desc["mode"] == "mla" else _run_step
    eager, replay = [], []
    out = run(desc, keep=eager)
    g = run(desc, graph=True, keep=replay)
    fails = out["fails"] + ["graph: " + f for f in g["fails"]]
    if len(eager) != len(replay) or not all(dc.same_bits(a, b) for a, b in zip(eager, replay)):
        fails.append("the graph replay differs from the eager trace")
    out = dict(out, fails=fails, graph=True, o_ratio=max(out["o_ratio"], g["o_ratio"]), lse_err=max(out["lse_err"], g["lse_err"]))
    if "fill_checked" in g:
        out["fill_checked"] = out["fill_checked"] + g["fill_checked"]
    return out


def run_case(desc):
    """Run a drawn trace on the current device and check it: desc plus `fails`, `o_ratio` (the worst O error over its bar), `lse_err`, `steps_run`,
    `recycled`.  A step trace always runs twice, eager and replayed from one captured step: the operator allocates its own o, so only the replay's
    static o has a known fill, and the rows at and beyond cu[B] are held to it on every step of every trace (`fill_checked` counts them; fewer than
    the trace's steps is a failure).  An mla trace is replayed when desc["graph"] says so."""
    if desc["mode"] == "step":
        out = run_with_graph(desc)
        if out["fill_checked"] != out["steps_run"]:
            out["fails"].append("the rows of o at and beyond cu[B] were checked on %d of %d steps" % (out["fill_checked"], out["steps_run"]))
        return out
    return run_with_graph(desc) if desc["graph"] else _run_mla(desc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--mode", default="step", choices=MODES)
    ap.add_argument("--graph-every", type=int, default=10, help="every n-th mla trace is also replayed from a captured graph (0 = never); every step trace is")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bad, worst, steps, filled = [], dict(o_ratio=0.0, lse_err=0.0), 0, 0
    for desc in draw_sweep(args.seed, [(args.mode, args.cases)]):
        if desc["mode"] == "mla" and args.graph_every > 0 and desc["i"] % args.graph_every == 0:
            desc = dict(desc, graph=True)
        try:
            d = run_case(desc)
        except Exception as e:                      # a refused shape or a launch error is a finding too
            d = dict(desc, fails=["exception: %r" % (e,)])
        for key in worst:
            worst[key] = max(worst[key], d.get(key, 0.0))
        steps, filled = steps + d.get("steps_run", 0), filled + d.get("fill_checked", 0)
        if d["fails"]:
            bad.append(d)
            print("FAIL", json.dumps(d), flush=True)
        if desc["i"] % 25 == 24:
            print("%d traces, %d failures" % (desc["i"] + 1, len(bad)), file=sys.stderr, flush=True)
    summary = dict(tool="fuzz_serving", mode=args.mode, cases=args.cases, seed=args.seed, failures=len(bad), worst_o_err_over_bar=worst["o_ratio"],
                   worst_lse_err=worst["lse_err"], steps=steps, unowned_rows_checked_on_steps=filled, device=torch.cuda.get_device_name(0), failing=bad)
    line = json.dumps(summary)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
