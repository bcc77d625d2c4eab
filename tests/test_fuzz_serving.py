"""CPU tests of tools/fuzz_serving.py, the serving traces of the packed step (chunked prefill with the fused packed append) and of the latent cache
(packed prompt appends, then fused MLA decode steps): that the draw is pure and legal, that the slices tests/test_fuzz_serving_gpu.py runs reach every
named condition, that the references alone pass the checker at every step, that the checker flags float64 mutants of the contract which lie at least
5 bars from the truth (tests/test_fuzz_decode.py's MARGIN) wherever they do, that image mutants of the append are caught by the bit-for-bit image
compare, that the drawn windows, caps and slopes are not idle, that the packed image builder equals the existing references and the library's host-side
rotary arithmetic, and that shrink keeps what fails.  "The kernel's output" here is the same-contract emulation — float64 rounded to the I/O dtype
for `step`, the oracle's output for `mla`; nothing touches a device."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import decode_window_refs as wr
import key_bars
import kvappend_refs as kr
import mla_append_refs as ar
import mla_refs as mr
from conftest import FLOOR, LSE_TOL
from test_fuzz_decode import MARGIN, _rotary_eval

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def fs():
    spec = importlib.util.spec_from_file_location("_fuzz_serving", os.path.join(ROOT, "tools", "fuzz_serving.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------------------- draw, coverage
def test_draw_is_pure_reproducible_and_legal(fs):
    for seed, counts in ((fs.STEP_SEED, fs.STEP_COUNTS), (fs.MLA_SEED, fs.MLA_COUNTS), (11, [("step", 25)]), (12, [("mla", 25)])):
        a, b = fs.draw_sweep(seed, counts), fs.draw_sweep(seed, counts)
        assert a == b and len(a) == sum(n for _, n in counts)
        for d in a:
            ck = d["page"] * d["capacity"]
            assert d["mode"] == counts[0][0] and d["page"] in (64, 128) and 3 <= d["B"] <= 5 and len(d["check_steps"]) == 3
            if d["mode"] == "step":
                assert 25 <= d["steps"] <= 40 and 300 <= d["T"] <= 400 and len(d["plan"]) == d["steps"] and d["rows"] in (0, 128, 256)
                for rs, nq, before, after in fs.step_walk(d):
                    assert len(nq) == d["B"] and min(nq) >= 0 and sum(nq) < d["T"], "cu[B] < T: the buffer is filled partly"
                    assert all(0 <= n <= ck for n in after) and max(after) < 720
                assert max(max(nq) for nq in d["plan"]) > 128 and all(len(ch) in (2, 3) and sum(ch) % d["page"] for _, _, ch in d["restarts"])
                used = max(sum(-(-n // d["page"]) for n in after) for _, _, _, after in fs.step_walk(d))
                assert used <= d["B"] * d["capacity"], "page counts within the pool"
            else:
                assert 30 <= d["steps"] <= 50 and d["H"] in fs.MLA_HEADS and 1 <= d["Nq"] <= 3 and d["num_splits"] in (0, 1, 3)
                for before, after, inc in fs.mla_walk(d):
                    assert all(0 <= n <= ck for n in after) and max(after) < 720 and set(inc) <= {0, d["Nq"]}
                assert 0 in d["prompts"] and d["pad"] >= 1


def test_slices_reach_every_named_condition(fs):
    cov = {}
    for seed, counts in ((fs.STEP_SEED, fs.STEP_COUNTS), (fs.MLA_SEED, fs.MLA_COUNTS)):
        cov.update(fs.coverage(fs.draw_sweep(seed, counts)))
    for name in sorted(cov):
        print("%4d  %s" % (cov[name], name))
    for name in ("an idle slot beside a chunk in one launch", "a decode row beside a chunk",
                 "a chunk whose first row sits mid-page and whose last row sits in the next page", "a chunk over 128 rows", "a chunk over 256 rows",
                 "a chunk over 256 rows under rows 128", "a chunk over 256 rows under rows 256",
                 "a prompt prefilled in three chunks", "a restart on recycled pages that does not end on a page edge", "a window edge crossing into a freed page",
                 "an e4m3 trace with a window", "a 16-bit trace with a window", "a step trace under rows 128", "a step trace under rows 256",
                 "an mla trace whose forced split leaves a part empty for a short slot", "an mla packed prompt call with a zero-token slot"):
        assert name in cov, name
    assert len(cov) >= 25 and not [n for n, c in cov.items() if c < 1]


def test_page_mirror_of_the_draw_is_the_traces_own_free_list(fs):
    """step_pages, from which coverage reads who takes a page a window freed, against StepTrace's own maps at every step: the same logical pages
    owned, and one bijection between the mirror's page ids and the pool's over the whole trace"""
    windows = 0
    for d in fs.draw_sweep(fs.STEP_SEED, fs.STEP_COUNTS) + fs.draw_sweep(11, [("step", 6)]):
        tr, ids = fs.StepTrace(d), {}
        for s, (takes, owned) in enumerate(fs.step_pages(d)):
            tr.begin_step(s)
            assert [sorted(o) for o in owned] == [sorted(o) for o in tr.owned], (d["i"], s)
            for b in range(d["B"]):
                for j, mid in owned[b].items():
                    assert ids.setdefault(mid, tr.owned[b][j]) == tr.owned[b][j], (d["i"], s, b, j)
            windows += sum(by is not None and by != b for b, _, by in takes)
        assert len(set(ids.values())) == len(ids)
    assert windows >= 3


# ---------------------------------------------------------------------------------------------------------------- step traces: float64 mutants
def _heads(t, G):
    """[n, Hkv, D] -> [H, n, D]"""
    return t.transpose(0, 1).repeat_interleave(G, dim=0)


def _seq64(tr, b, cu, q_rot, k=None, v=None, keep=None, pos=None, slopes="own"):
    """float64 of sequence b's rows under a changed contract -> O [H, Nq, D], log2 lse [H, Nq]"""
    d = tr.d
    if k is None:
        k, v = tr.keys(b)
    sl = tr.slopes if slopes == "own" else slopes
    sl = None if sl is None else (sl if sl.dim() == 1 else sl[b])
    q = q_rot[cu[b]:cu[b + 1]].transpose(0, 1).float()
    return wr.truth64(q, _heads(k, d["G"]), _heads(v, d["G"]), tr.scale, d["window_left"], d["softcap"], sl, keep=keep, pos=pos)


def _band(pos, n, wl, upper=None):
    """keep [Nq, n]: j <= upper (the row's position by default) and, under a window, j >= pos - wl"""
    j = torch.arange(n)[None, :]
    keep = j <= (pos if upper is None else upper)[:, None]
    return keep & (j >= pos[:, None] - wl) if wl >= 0 else keep


def _m_top_left(tr, b, cu, q_rot):
    n, nq = tr.lens[b], tr.nq[b]
    if n <= nq:
        return None
    return _seq64(tr, b, cu, q_rot, keep=_band(torch.arange(nq), n, tr.d["window_left"]), pos=torch.arange(nq))


def _m_own_keys_invisible(tr, b, cu, q_rot):
    n, nq = tr.lens[b], tr.nq[b]
    pos = n - nq + torch.arange(nq)
    return _seq64(tr, b, cu, q_rot, keep=_band(pos, n, tr.d["window_left"], upper=torch.full((nq,), n - nq - 1)))


def _m_whole_chunk_visible(tr, b, cu, q_rot):
    n, nq = tr.lens[b], tr.nq[b]
    if nq < 2:
        return None
    pos = n - nq + torch.arange(nq)
    return _seq64(tr, b, cu, q_rot, keep=_band(pos, n, tr.d["window_left"], upper=torch.full((nq,), n - 1)))


def _m_one_window_edge(tr, b, cu, q_rot):
    n, nq, wl = tr.lens[b], tr.nq[b], tr.d["window_left"]
    if wl < 0 or nq < 2 or n - 1 - wl <= 0:
        return None
    pos = n - nq + torch.arange(nq)
    return _seq64(tr, b, cu, q_rot, keep=_band(pos, n, -1) & (torch.arange(n)[None, :] >= n - 1 - wl))


def _m_stale_keys(tr, b, cu, q_rot):
    n, nq, page = tr.lens[b], tr.nq[b], tr.d["page"]
    if b not in tr.recycled or n % page == 0:
        return None
    end = -(-n // page) * page
    k, v = tr.keys(b, n=end)
    assert torch.isfinite(k).all() and torch.isfinite(v).all(), "stale keys are finite: the quiet failure"
    pos = n - nq + torch.arange(nq)
    keep = torch.cat([_band(pos, n, tr.d["window_left"]), torch.ones((nq, end - n), dtype=torch.bool)], dim=1)
    return _seq64(tr, b, cu, q_rot, k=k, v=v, keep=keep, pos=pos)


def _m_neighbours_cache(tr, b, cu, q_rot):
    if b == 0:
        return None
    k, v = tr.keys(b, slot=b - 1)
    return _seq64(tr, b, cu, q_rot, k=k, v=v)


def _m_batch_0(tr, b, cu, q_rot):
    d = tr.d
    if b == 0 or not (d["fp8"] or d["slopes"] == "BH"):
        return None
    k, v = tr.gather(b, tr.lens[b])
    if d["fp8"]:
        k, v = k.float() * tr.kd[0].float()[None, :, None], v.float() * tr.vd[0].float()[None, :, None]
    else:
        k, v = k.float(), v.float()
    return _seq64(tr, b, cu, q_rot, k=k, v=v, slopes=None if tr.slopes is None else (tr.slopes if tr.slopes.dim() == 1 else tr.slopes[0]))


def _m_page_first_key(tr, b, cu, q_rot):
    n, page = tr.lens[b], tr.d["page"]
    if n <= page:
        return None
    k, v = (t.clone() for t in tr.keys(b))
    for p in range(1, -(-n // page)):
        k[p * page], v[p * page] = k[(p - 1) * page].clone(), v[(p - 1) * page].clone()
    return _seq64(tr, b, cu, q_rot, k=k, v=v)


STEP_MUTANTS = {"chunk rows placed top-left (pos = i)": _m_top_left, "the chunk's own new keys invisible": _m_own_keys_invisible,
                "the whole chunk visible to every row": _m_whole_chunk_visible, "one lower window edge for the chunk, from its last row": _m_one_window_edge,
                "the previous owner's stale keys take part": _m_stale_keys, "sequence s attends with slot s-1's cache": _m_neighbours_cache,
                "batch 0's descales or slopes for every sequence": _m_batch_0, "the first key of a page read from the page before": _m_page_first_key}
IDLE = "an idle slot's rows written"


def _distance(mut, ref, r0, r1):
    """how far a mutant (O [H, Nq, D], lse [H, Nq]) lies from the truth of the rows [r0, r1), in bars: the larger of O and LSE; dead rows differ: inf"""
    ro, rl, bar = ref
    dist = key_bars.ratio_max((mut[0].transpose(0, 1) - ro[r0:r1]).abs(), bar[r0:r1])
    dead_t, dead_m = torch.isinf(rl[:, r0:r1]), torch.isinf(mut[1])
    if not torch.equal(dead_t, dead_m):
        return INF
    if bool((~dead_t).any()):
        dist = max(dist, float((mut[1] - rl[:, r0:r1])[~dead_t].abs().max()) / LSE_TOL)
    return dist


@pytest.fixture(scope="module")
def step_census(fs):
    """One CPU walk of the GPU slice: per mutant [steps it applies to, steps where it lies >= MARGIN bars from the truth, of those the flagged ones];
    per trace whether its drawn window / cap / slopes move some step by >= MARGIN bars; the emulation's failures (none)."""
    tally = {m: [0, 0, 0] for m in list(STEP_MUTANTS) + [IDLE]}
    emu_fails, live, steps = [], {}, 0
    for d in fs.draw_sweep(fs.STEP_SEED, fs.STEP_COUNTS):
        tr = fs.StepTrace(d)
        fill = fs.fill_rows((d["T"], tr.H, d["D"]), tr.dt)
        banded = d["window_left"] >= 0 or d["softcap"] > 0 or d["slopes"] is not None
        if banded:
            live[d["i"]] = 0.0
        for s in range(d["steps"]):
            cu, q, k, v = tr.begin_step(s)
            total = cu[-1]
            q_rot = tr.apply_step(cu, q, k, v)
            ref = tr.reference(cu, q_rot)
            o, lse = fill.clone(), torch.full((tr.H, d["T"]), float("nan"))
            o[:total], lse[:, :total] = ref[0].to(tr.dt), ref[1].float()
            tag = "trace %d step %d" % (d["i"], s)
            emu_fails += fs.check_step(tag, o, lse, ref, total, fill)
            steps += 1
            if 0 in tr.nq:                                           # an idle slot whose (no) rows a wrong kernel writes: the first row nobody owns
                tally[IDLE][0] += 1
                tally[IDLE][1] += 1
                o2 = o.clone()
                o2[total] = 0
                tally[IDLE][2] += bool(fs.check_step(tag, o2, lse, ref, total, fill))
            for name, fn in STEP_MUTANTS.items():
                best = None
                for b in range(d["B"]):
                    if tr.nq[b] and tr.lens[b]:
                        mut = fn(tr, b, cu, q_rot)
                        if mut is not None:
                            dist = _distance(mut, ref, cu[b], cu[b + 1])
                            if best is None or dist > best[0]:
                                best = (dist, b, mut)
                if best is None:
                    continue
                tally[name][0] += 1
                if best[0] >= MARGIN:
                    tally[name][1] += 1
                    o2, l2 = ref[0].clone(), ref[1].clone()
                    b = best[1]
                    o2[cu[b]:cu[b + 1]], l2[:, cu[b]:cu[b + 1]] = best[2][0].transpose(0, 1), best[2][1]
                    tally[name][2] += bool(fs.check_step(tag, o2, l2, ref, total))
            if banded and total:
                ks, vs = zip(*[tr.keys(b) for b in range(d["B"])])
                plain = fs.pc.reference(q_rot[:total], torch.tensor(cu, dtype=torch.int32), ks, vs, tr.scale)
                live[d["i"]] = max(live[d["i"]], key_bars.ratio_max((plain[0] - ref[0]).abs(), ref[2]))
    return dict(tally=tally, emu_fails=emu_fails, live=live, steps=steps)


def test_step_reference_alone_passes_at_every_step(step_census):
    assert step_census["steps"] >= 150 and not step_census["emu_fails"], step_census["emu_fails"][:3]


def test_checker_flags_float64_mutants_of_the_step_contract(step_census):
    tally = step_census["tally"]
    for name, (applies, far, flagged) in tally.items():
        print("%-58s applies to %3d of %d steps, >= %g bars from the truth on %3d, flagged on %3d" % (name, applies, step_census["steps"], MARGIN, far, flagged))
    assert all(far >= 1 and flagged == far for _, far, flagged in tally.values()), tally


def test_drawn_features_are_not_idle(step_census):
    live = step_census["live"]
    print("step: %d traces draw a window, a cap or slopes; %d differ from the plain call by >= %g bars at some step" % (len(live), sum(v >= MARGIN for v in live.values()), MARGIN))
    assert len(live) >= 3 and sum(v >= MARGIN for v in live.values()) >= 0.8 * len(live), live


def test_step_image_mutant_rotary_position_taken_as_the_chunk_index(fs):
    """K rotated by the token's index in its chunk: the image compare of the last step (which the GPU run makes) sees it in every trace"""
    for d in fs.draw_sweep(fs.STEP_SEED, fs.STEP_COUNTS):
        tr, mut = fs.StepTrace(d), fs.StepTrace(d)
        for s in range(d["steps"]):
            a, b = tr.begin_step(s), mut.begin_step(s)
            assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
            tr.apply_step(*a)
            mut.apply_step(*b, position_i=True)
        assert tr.mismatches(tr.pool) == 0 and tr.mismatches(mut.pool) > 0, d["i"]


# ---------------------------------------------------------------------------------------------------------------- mla traces
MLA_MUTANTS = ("k512", "v64", "rowmap", "dropkey", "diag", "stale")


def _mla_distance(o, lse, refs, code):
    """the largest distance of (o [B, Nq, H, 512], lse [B, H, Nq]) from float64 over the live slots, in decode_refs.check's bars"""
    dist = 0.0
    for b, r in enumerate(refs):
        if r is None:
            continue
        dist = max(dist, float(np.abs(o[b].transpose(0, 1).numpy() - r[2][0]).max()) / (2 * FLOOR[code]))
        gl, tl = lse[b].numpy(), r[3][0]
        if not np.array_equal(np.isinf(gl), np.isinf(tl)):
            return INF
        fin = ~np.isinf(tl)
        if fin.any():
            dist = max(dist, float(np.abs(gl[fin] - tl[fin]).max()) / LSE_TOL)
    return dist


@pytest.fixture(scope="module")
def mla_census(fs):
    tally = {m: [0, 0, 0] for m in MLA_MUTANTS}
    emu_fails, steps = [], 0
    for d in fs.draw_sweep(fs.MLA_SEED, fs.MLA_COUNTS):
        tr = fs.MlaTrace(d)
        code = fs.dc.code(tr.dt)
        for s in range(d["steps"]):
            _, q, kv_c, k_pe = tr.begin_step(s)
            q_rot = tr.apply_step(q, kv_c, k_pe)
            refs = tr.refs(q_rot)                                    # (asserts on the way that the oracle alone meets the float64 bars)
            o, lse = fs.mla_oracle_outputs(refs, d["B"], d["Nq"], d["H"])
            tag = "mla trace %d step %d" % (d["i"], s)
            emu_fails += fs.mla_checked(o, lse, refs, tr.lens, code, tag)
            steps += 1
            for m in MLA_MUTANTS:
                lens = list(tr.lens)
                if m == "stale":
                    lens = [-(-n // d["page"]) * d["page"] if (b in tr.recycled and n) else n for b, n in enumerate(tr.lens)]
                if (m == "stale" and lens == tr.lens) or (m in ("rowmap", "diag") and d["Nq"] < 2) or (m == "rowmap" and d["H"] < 2):
                    continue
                kv = tr.rows(lens)
                assert torch.isfinite(kv.float()).all()
                mo, ml = mr.mla_f64(q_rot, kv, lens, mutant=None if m == "stale" else m)
                tally[m][0] += 1
                if _mla_distance(mo, ml, refs, code) >= MARGIN:
                    tally[m][1] += 1
                    tally[m][2] += bool(fs.mla_checked(mo, ml, refs, tr.lens, code, tag))
    return dict(tally=tally, emu_fails=emu_fails, steps=steps)


def test_mla_oracle_alone_passes_at_every_step(mla_census):
    assert mla_census["steps"] >= 120 and not mla_census["emu_fails"], mla_census["emu_fails"][:3]


def test_checker_flags_float64_mutants_of_the_mla_contract(mla_census):
    tally = mla_census["tally"]
    for name, (applies, far, flagged) in tally.items():
        print("%-8s applies to %3d of %d steps, >= %g bars from the truth on %3d, flagged on %3d" % (name, applies, mla_census["steps"], MARGIN, far, flagged))
    assert all(far >= 1 and flagged == far for _, far, flagged in tally.values()), tally


def _mla_image_mutant(fs, kind):
    class Mutant(fs.MlaTrace):
        def _expect(self, kv_c, k_pe, owners, q):
            q_out = super()._expect(kv_c, k_pe, owners, q)
            page, raw = self.d["page"], fs._raw(self.pool[0])
            for t, o in enumerate(owners):
                if o is None:
                    continue
                b, i, n = o
                pos = self.lens[b] - n + i
                if kind == "clamp" and pos < 0:                          # a token that must be skipped, written at the clamped position
                    raw[int(self.bt[b, 0]), 0, 0, :mr.DV] = fs._raw(kv_c[t])
                elif kind != "clamp" and pos >= 0:
                    tail = k_pe[t] if kind == "unrotated" else ar.rotated_tail(k_pe[t:t + 1], torch.tensor([i]), self.cos, self.sin, self.d["inter"])[0]
                    raw[self.owned[b][pos // page], pos % page, 0, mr.DV:] = fs._raw(tail)
            return q_out
    return Mutant


@pytest.mark.parametrize("kind", ["position_i", "clamp", "unrotated"])
def test_mla_image_mutants_are_caught_by_the_image_compare(fs, kind):
    """the rotary position taken as the token's index in its call; a token at a negative position (the parked slot's) written at the clamped position —
    row 0 of the all-NaN page 0; k_pe stored unrotated: the compare of the last step (which the GPU run makes) sees each in every trace"""
    for d in fs.draw_sweep(fs.MLA_SEED, fs.MLA_COUNTS):
        tr, mut = fs.MlaTrace(d), _mla_image_mutant(fs, kind)(d)
        for s in range(d["steps"]):
            a, b = tr.begin_step(s), mut.begin_step(s)
            assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
            tr.apply_step(*a[1:])
            mut.apply_step(*b[1:])
        assert tr.mismatches(tr.pool) == 0 and tr.mismatches(mut.pool) > 0, (kind, d["i"])


# ---------------------------------------------------------------------------------------------------------------- the builders against the references
def test_step_image_equals_the_append_reference_on_the_uniform_twin(fs):
    """equal counts in every slot: the packed builder's rows and rotated q are kvappend_refs.append_rows' on the [B, Nnew] twin, and (16-bit caches)
    fa2_rotary_eval's, bit for bit"""
    rows = 0
    for d in fs.draw_sweep(fs.STEP_SEED, fs.STEP_COUNTS):
        B = d["B"]
        d = dict(d, steps=2, plan=[[7] * B, [5] * B], restarts=[], check_steps=[0], capacity=2)
        tr = fs.StepTrace(d)
        for s in range(2):
            cu, q, k, v = tr.begin_step(s)
            n = d["plan"][s][0]
            q_rot = tr.apply_step(cu, q, k, v)
            twin = [t[:B * n].reshape(B, n, t.shape[1], t.shape[2]) for t in (q, k, v)]
            rk, rv, rq = kr.append_rows(twin[1], twin[2], tr.lens, q=twin[0], cos=tr.cos, sin=tr.sin, inter=d["inter"], fp8=d["fp8"], kd=tr.kd, vd=tr.vd)
            assert torch.equal(fs._raw(q_rot[:B * n]), fs._raw(rq.reshape(B * n, tr.H, d["D"]))) and torch.equal(fs._raw(q_rot[B * n:]), fs._raw(q[B * n:]))
            for b in range(B):
                gk, gv = tr.gather(b, tr.lens[b])
                assert torch.equal(fs._raw(gk[-n:]), fs._raw(rk[b])) and torch.equal(fs._raw(gv[-n:]), fs._raw(rv[b])), (d["i"], s, b)
                if not d["fp8"]:
                    for i in (0, n - 1):
                        pos = tr.lens[b] - n + i
                        want = _rotary_eval(k[cu[b] + i, 0], tr.cos[pos], tr.sin[pos], d["rot"], d["inter"], tr.dt)
                        assert torch.equal(gk[-n + i, 0].view(torch.int16), want), (d["i"], s, b, i)
                        rows += 1
    assert rows >= 12


def test_mla_image_equals_the_append_reference_and_the_host_arithmetic(fs):
    """the image after the first packed prompt call and a decode step: mla_append_refs.expect fed the same owners on a pool of its own, and the stored
    tails fa2_rotary_eval's, bit for bit"""
    rows = 0
    for d in fs.draw_sweep(fs.MLA_SEED, fs.MLA_COUNTS):
        tr, twin = fs.MlaTrace(d), fs.MlaTrace(d)
        before = twin.latent().clone()
        _, q, kv_c, k_pe = tr.begin_step(0)
        # the twin's stream: the prompt call's tokens, drawn as admit draws them
        for b, n in enumerate(d["prompts"]):
            twin.release(b)
            twin.lens[b] = n
            twin._hand_out(b, whole=True)
        assert torch.equal(twin.bt, tr.bt)
        owners = [(b, i, n) for b, n in enumerate(d["prompts"]) for i in range(n)] + [None] * d["pad"]
        pc_, pp_, pq_ = (fs.fd._randn((len(owners),) + tail, twin.g).to(twin.dt) for tail in ((mr.DV,), (ar.ROT,), (d["H"], mr.D)))
        img, _ = ar.expect(before, pc_, pp_, owners, d["prompts"], block_table=twin.bt, q=pq_, cos=tr.cos, sin=tr.sin, inter=d["inter"])
        lens1 = [n + a for n, a in zip(d["prompts"], fs.mla_walk(d)[0][2])]
        assert lens1 == tr.lens
        assert torch.equal(fs._raw(tr.latent()), fs._raw(img)), (d["i"], "the whole pool after the prompt call")
        tr.apply_step(q, kv_c, k_pe)
        for b in range(d["B"]):
            for i in range(d["Nq"]):
                pos = tr.lens[b] - d["Nq"] + i
                if pos < 0:
                    continue
                got = tr.latent()[tr.owned[b][pos // d["page"]], pos % d["page"]]
                assert torch.equal(got[:mr.DV].view(torch.int16), kv_c[b, i].view(torch.int16))
                want = _rotary_eval(k_pe[b, i], tr.cos[pos].float(), tr.sin[pos].float(), ar.ROT, d["inter"], tr.dt)
                assert torch.equal(got[mr.DV:].contiguous().view(torch.int16), want), (d["i"], b, i)
                rows += 1
    assert rows >= 8


# ---------------------------------------------------------------------------------------------------------------- shrink
def test_shrink_keeps_what_fails_and_drops_the_rest(fs):
    """shrink on pretended failures (`a slot brings more than 128 rows in one step`; `a slot is restarted`): what is left still fails, is a legal draw, is
    smaller, and still builds"""
    for d in fs.draw_sweep(fs.STEP_SEED, fs.STEP_COUNTS)[:3]:
        fails = lambda c: any(max(nq) > 128 for nq in c["plan"])          # noqa: E731
        s = fs.shrink(d, fails)
        assert fails(s) and s["B"] == 1 and s["steps"] <= d["steps"] and max(s["plan"][-1]) > 128 and not any(max(nq) > 128 for nq in s["plan"][:-1])
        assert s["window_left"] == -1 and s["softcap"] == 0.0 and s["slopes"] is None and s["fp8"] is False and s["capacity"] == d["capacity"]
        assert all(sum(nq) < s["T"] and len(nq) == 1 for nq in s["plan"]) and all(slot < s["B"] for _, slot, _ in s["restarts"])
        tr = fs.StepTrace(s)
        for n in range(s["steps"]):
            cu, q, k, v = tr.begin_step(n)
            ref = tr.reference(cu, tr.apply_step(cu, q, k, v))
        assert ref[0].shape[0] == cu[-1] > 128
    for d in fs.draw_sweep(fs.MLA_SEED, fs.MLA_COUNTS)[:2]:
        fails = lambda c: len(c["events"]) > 0                            # noqa: E731
        s = fs.shrink(d, fails)
        assert fails(s) and s["B"] == 1 and s["steps"] == d["events"][0][0] + 1 and len(s["prompts"]) == 1 and s["events"][0][1] == 0
        tr = fs.MlaTrace(s)
        for n in range(s["steps"]):
            _, q, kv_c, k_pe = tr.begin_step(n)
            refs = tr.refs(tr.apply_step(q, kv_c, k_pe))
        assert len(refs) == 1 and tr.lens[0] == s["events"][0][2] + (s["Nq"] if s["park_slot"] != 0 or s["steps"] > s["park"] else 0)
