"""What tools/decode_bench.py, tools/decode_window_bench.py and tools/kvappend_bench.py share: the interleaved timing protocol, a graph replay, the
comparison of two routes' outputs and the paged pool."""
import statistics

import torch


def interleaved(fns, rounds, iters):
    """{name: (median, min, max) ms per call} of the callables in `fns`, timed round-robin (one event pair per (round, callable))."""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / iters)
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


def graphed(fn):
    """fn captured once (after a warm-up on a side stream) -> the replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            keep = fn()
    torch.cuda.current_stream().wait_stream(side)
    graph.keep = keep
    return graph.replay


def close(tool, a, b, dt, what):
    """a against b under the I/O dtype's bar (fp16 1e-3 + 2e-3 |b|, bf16 8e-3 + 1.6e-2 |b|), a finite: else the tool stops"""
    atol, rtol = (1e-3, 2e-3) if dt == torch.float16 else (8e-3, 1.6e-2)
    a, b = a.float(), b.float()
    if ((a - b).abs() > atol + rtol * b.abs()).any() or not torch.isfinite(a).all():
        raise SystemExit("%s: %s disagree (max |diff| %.3g)" % (tool, what, float((a - b).abs().max())))


def paged_pool(kc, vc, page, g, lens=None, spare=4):
    """The [B, Nmax, Hkv, D] caches scattered into pages in shuffled physical order: every page of every sequence, or with `lens` the pages its keys
    reach, and `spare` pages more, which stay zero; table entries without a page name one of those.  -> pool K, pool V, block table [B, Nmax / page]"""
    B, per = kc.shape[0], kc.shape[1] // page
    used = [per] * B if lens is None else [-(-n // page) for n in lens]
    total = sum(used) + spare
    order = torch.randperm(total, generator=g)
    src = torch.tensor([b * per + j for b in range(B) for j in range(used[b])])
    bt = torch.full((B * per,), int(order[-1]), dtype=torch.int32)
    bt[src] = order[:len(src)].to(torch.int32)
    pools = []
    for c in (kc, vc):
        pool = torch.zeros((total, page) + tuple(c.shape[2:]), device=c.device, dtype=c.dtype)
        pages = c[:, :per * page].reshape(B * per, page, *c.shape[2:])
        pool[order[:len(src)].to(c.device)] = pages if lens is None else pages[src.to(c.device)]
        pools.append(pool)
    return pools[0], pools[1], bt.reshape(B, per).to(kc.device)
