"""Pin the host side of the C-ABI: what every plan / workspace query answers and which error code every bad call gets.

    python tests/golden/make_abi_golden.py          # writes tests/golden/abi_golden.npz

Run once, on a machine WITHOUT a GPU, against the library whose behaviour is to be kept (tests/test_abi_golden.py replays the file against the
library of the tree it runs in and asserts equality).  The fixture is data only:
  * `meta`: JSON — the axes of every plan / size grid (the rows are their cross product, in the order `expand` walks it) and the names of the
    entry points and defects of the error table;
  * `plan_rows`: the distinct (return code, nine fields of fa2_fwd_plan_t) answers; `plans/<grid>`: one index into it per row of the grid;
  * `sizes/<grid>`: five byte counts per row (fa2_fwd_ / fa2_fwd_gqa_ / fa2_bwd_ / fa2_bwd_gqa_ / fa2_bwd_bias_workspace_bytes);
  * `errors`: (entry, defect, second defect or -1, code) — every single defect and every pair of defects of one valid call per launching entry point.
Without a GPU the library plans for 256 CUs, the MI355X's count, so the same rows hold on the GPU machines.  No row of the error table may reach a
launch — the pointers are stand-ins — so every row carries a defect and the generator insists that every recorded code is an FA2_ERR_*.
"""
import ctypes
import itertools
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.realpath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd")
FIXTURE = os.path.join(HERE, "abi_golden.npz")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MIB64 = 64 << 20
CAUSAL, EXACT, BOTTOM_RIGHT = 1, 2, 4

# ---------------------------------------------------------------------------------------------------------------- plan and size grids
DS = [8, 40, 64, 72, 88, 104, 128, 136, 160, 176, 256, 264, 512]
NQS = [1, 77, 128, 1024, 4096]
NKVS = [77, 128, 512, 896, 1280, 1792, 4096, 8192]
BHS = [[1, 1], [1, 8], [2, 10], [1, 24], [2, 16], [4, 16], [10, 16]]            # B * H = 1, 8, 20, 24, 32, 64, 160
SCALES = ["rsqrt", "one", "neg_rsqrt", "zero"]                                   # D^-0.5, 1.0, -D^-0.5, 0
STRIDES = ["null", "bnhd", "k_pitch"]                                            # NULL, [B, N, H, D] tensors, a K row pitch of D + 8 elements
WINDOWS = [[-1, -1, 0], [-1, 0, 0], [65, 0, 70], [5000, 5000, 0], [64, 64, 0], [-1, 3, 0]]    # plain, causal, bands (one too wide to mask at short N)
# the slice the option settings and the crossed axes repeat: every head dim, lengths on both sides of every threshold, grids below / at / above one round
SLICE = {"dtype": [0, 1], "D": DS, "Nq": [77, 1024, 4096], "Nkv": [77, 512, 1280, 4096], "BH": [[1, 8], [1, 24], [10, 16]], "flags": [0, CAUSAL]}
BASE = {"dtype": [0, 1], "D": DS, "Nq": NQS, "Nkv": NKVS, "BH": BHS, "flags": [0, CAUSAL]}
OPTION_SETS = [{"rows": 128}, {"rows": 256}, {"asm": 0}, {"fold": 0}, {"fold": 2}, {"split": 0}, {"short": 0}]

# axis order of a grid = the order of AXES; axes a grid does not name take the first value of DEFAULTS
AXES = ["entry", "options", "dtype", "D", "Nq", "Nkv", "BH", "hkv", "flags", "scale", "ws", "strides", "window", "bias_kind"]
DEFAULTS = {"entry": "fa2_fwd_plan", "options": {}, "hkv": "h", "scale": "rsqrt", "ws": MIB64, "strides": "null", "window": [-1, -1, 0], "bias_kind": 0}


def plan_grids():
    g = {}
    g["fwd_base"] = dict(BASE)
    g["fwd_exact"] = dict(BASE, flags=[EXACT, EXACT | CAUSAL])
    g["fwd_no_ws"] = dict(BASE, ws=[0])
    g["fwd_axes"] = dict(SLICE, flags=[0, CAUSAL, EXACT], scale=SCALES, ws=[0, MIB64], strides=STRIDES)
    g["fwd_options"] = dict(SLICE, options=OPTION_SETS, flags=[0, CAUSAL, EXACT], ws=[0, MIB64])
    g["fwd_bias"] = dict(SLICE, bias_kind=[1, 2, 3, 7])
    g["fwd_edges"] = {"dtype": [0, 1, 2], "D": [0, 12, 64, 520], "Nq": [0, 128], "Nkv": [0, 128], "BH": [[0, 1], [1, 0], [1, 8]], "flags": [0, 4, 8]}
    g["gqa"] = dict(SLICE, entry=["fa2_fwd_gqa_plan"], hkv=["one", "half", "h"], ws=[0, MIB64], strides=STRIDES)
    g["gqa_edges"] = {"entry": ["fa2_fwd_gqa_plan"], "dtype": [0], "D": [64], "Nq": [128], "Nkv": [128], "BH": [[1, 8]], "hkv": ["zero", "three", "twice"],
                      "flags": [0]}
    g["window"] = dict(SLICE, entry=["fa2_fwd_window_plan"], hkv=["half", "h"], flags=[0, CAUSAL, EXACT], window=WINDOWS)
    g["window_strides"] = dict(SLICE, entry=["fa2_fwd_window_plan"], hkv=["half"], window=WINDOWS[1:4], strides=STRIDES[1:])
    g["window_options"] = dict(SLICE, entry=["fa2_fwd_window_plan"], options=[{"rows": 128}, {"rows": 256}], window=WINDOWS)
    g["window_edges"] = {"entry": ["fa2_fwd_window_plan"], "dtype": [0], "D": [64], "Nq": [128], "Nkv": [128], "BH": [[1, 8]], "flags": [0, 4, 8],
                         "window": [[-2, 0, 0], [0, -2, 0], [0, 0, -1], [0, 0, 0]]}
    g["varlen"] = dict(SLICE, entry=["fa2_fwd_varlen_plan"], hkv=["half", "h"], flags=[0, EXACT, BOTTOM_RIGHT | CAUSAL],
                       window=[[-1, -1, 0], [65, 0, 0]], strides=STRIDES)
    g["varlen_options"] = dict(SLICE, entry=["fa2_fwd_varlen_plan"], options=[{"rows": 128}, {"rows": 256}])
    g["varlen_edges"] = {"entry": ["fa2_fwd_varlen_plan"], "dtype": [0, 2], "D": [12, 64], "Nq": [0, 128], "Nkv": [128], "BH": [[1, 8]], "hkv": ["three", "h"],
                         "flags": [0, 8], "window": [[-2, 0, 0], [0, 0, 0]]}
    return g


def size_grids():
    g = {}
    g["base"] = dict(BASE, hkv=["one", "half", "h"])
    g["options"] = dict(SLICE, options=OPTION_SETS, hkv=["half", "h"])
    g["edges"] = {"dtype": [0, 2], "D": [0, 12, 64, 520], "Nq": [0, 128], "Nkv": [0, 128], "BH": [[0, 1], [1, 0], [1, 8]], "hkv": ["zero", "three", "h"],
                  "flags": [0, 1, 2, 8]}
    return g


def expand(grid):
    """The rows of a grid: dicts axis -> value, the last axis of AXES running fastest."""
    names = [a for a in AXES if a in grid]
    for combo in itertools.product(*(grid[a] for a in names)):
        row = dict(DEFAULTS)
        row.update(zip(names, combo))
        yield row


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _scale(kind, D):
    d = max(D, 1)
    return {"rsqrt": _f32(d ** -0.5), "one": 1.0, "neg_rsqrt": -_f32(d ** -0.5), "zero": 0.0}[kind]


def _hkv(kind, H):
    return {"h": H, "one": 1, "half": max(H // 2, 1), "zero": 0, "three": 3, "twice": 2 * H}[kind]


def _strides(kind, H, Hkv, Nq, Nkv, D, packed):
    i64 = ctypes.c_int64
    if kind == "null":
        return None, None
    pitch = D + 8 if kind == "k_pitch" else D
    if packed:                  # {head, row} of [total, heads, D]
        return (i64 * 2)(D, H * D), (i64 * 2)(pitch, Hkv * pitch)
    if kind == "bnhd":
        return (i64 * 3)(Nq * H * D, D, H * D), (i64 * 3)(Nkv * Hkv * D, D, Hkv * D)
    return (i64 * 3)(H * Nq * D, Nq * D, D), (i64 * 3)(Hkv * Nkv * pitch, Nkv * pitch, pitch)


class _Options:
    """fa2_set_option for the rows of one option set, restored afterwards."""

    def __init__(self, lib):
        self.lib, self.cur, self.saved = lib, None, {}

    def set(self, opts):
        key = json.dumps(opts, sort_keys=True)
        if key == self.cur:
            return
        self.restore()
        for k, v in opts.items():
            self.saved[k] = self.lib.fa2_get_option(k.encode())
            assert self.saved[k] >= 0 and self.lib.fa2_set_option(k.encode(), int(v)) == 0
        self.cur = key

    def restore(self):
        for k, v in self.saved.items():
            assert self.lib.fa2_set_option(k.encode(), v) == 0
        self.saved, self.cur = {}, None


def run_plan_grid(lib, grid):
    """-> int32 [rows, 10]: return code and the nine fields of fa2_fwd_plan_t (poisoned with -7 before each call, so an untouched plan shows)."""
    from rocwmma_fattn._fa2_lib import FwdPlan
    fields = [n for n, _ in FwdPlan._fields_]
    out, opts, plan = [], _Options(lib), FwdPlan()
    try:
        for r in expand(grid):
            opts.set(r["options"])
            (B, H), D = r["BH"], r["D"]
            entry, packed = r["entry"], r["entry"] == "fa2_fwd_varlen_plan"
            Hkv = H if entry == "fa2_fwd_plan" else _hkv(r["hkv"], H)
            qs, ks = _strides(r["strides"], H, Hkv, r["Nq"], r["Nkv"], D, packed)
            for n in fields:
                setattr(plan, n, -7)
            head = (r["dtype"], B, H) + (() if entry == "fa2_fwd_plan" else (Hkv,)) + (r["Nq"], r["Nkv"], D, qs, ks, _scale(r["scale"], D), r["flags"])
            wl, wr, off = r["window"]
            if entry == "fa2_fwd_plan":
                rc = lib.fa2_fwd_plan(*head, r["bias_kind"], r["ws"], ctypes.byref(plan))
            elif entry == "fa2_fwd_gqa_plan":
                rc = lib.fa2_fwd_gqa_plan(*head, r["ws"], ctypes.byref(plan))
            elif entry == "fa2_fwd_window_plan":
                rc = lib.fa2_fwd_window_plan(*head, wl, wr, off, r["ws"], ctypes.byref(plan))
            else:
                rc = lib.fa2_fwd_varlen_plan(*head, wl, wr, ctypes.byref(plan))
            out.append([rc] + [getattr(plan, n) for n in fields])
    finally:
        opts.restore()
    return np.asarray(out, dtype=np.int32)


def run_size_grid(lib, grid):
    """-> int64 [rows, 5]: fa2_fwd_, fa2_fwd_gqa_, fa2_bwd_, fa2_bwd_gqa_ and fa2_bwd_bias_workspace_bytes."""
    out, opts = [], _Options(lib)
    try:
        for r in expand(grid):
            opts.set(r["options"])
            (B, H), Hkv = r["BH"], _hkv(r["hkv"], r["BH"][1])
            a = (r["dtype"], B, H, r["Nq"], r["Nkv"], r["D"], r["flags"])
            g = a[:3] + (Hkv,) + a[3:]
            out.append([lib.fa2_fwd_workspace_bytes(*a), lib.fa2_fwd_gqa_workspace_bytes(*g), lib.fa2_bwd_workspace_bytes(*a),
                        lib.fa2_bwd_gqa_workspace_bytes(*g), lib.fa2_bwd_bias_workspace_bytes(*a)])
    finally:
        opts.restore()
    return np.asarray(out, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------- error codes and their precedence
FWD_T = ["q", "k", "v", "o", "lse"]
BWD_T = ["q", "k", "v", "o", "dout", "lse", "dq", "dk", "dv", "delta_ws"]
FWD_S = ["q_strides", "k_strides", "v_strides", "o_strides"]
BWD_S = FWD_S + ["do_strides", "dq_strides", "dk_strides", "dv_strides"]
DIMS = ["B", "H", "Nq", "Nkv", "D"]
DIMS_G = ["B", "H", "Hkv", "Nq", "Nkv", "D"]
CU = ["cu_seqlens_q", "cu_seqlens_k"]
TAIL = ["scale", "flags"]
WIN = ["window_left", "window_right", "q_offset"]
WS = ["workspace", "workspace_bytes"]
BIAS = ["bias", "bias_kind", "bias_strides"]
DROP = ["dropout_p", "seed"]

# the parameter names of every entry point that takes tensors, in the header's order (Nq / Nkv: max_seqlen_q / max_seqlen_k of the packed calls)
ENTRIES = {
    "fa2_fwd": ["dtype"] + FWD_T + DIMS + FWD_S + ["lse_strides"] + TAIL + ["stream"],
    "fa2_fwd_f16": FWD_T + DIMS + FWD_S + ["lse_strides"] + TAIL + ["stream"],
    "fa2_fwd_bf16": FWD_T + DIMS + FWD_S + ["lse_strides"] + TAIL + ["stream"],
    "fa2_fwd_ws": ["dtype"] + FWD_T + DIMS + FWD_S + ["lse_strides"] + TAIL + WS + ["stream"],
    "fa2_fwd_bias": ["dtype"] + FWD_T + DIMS + FWD_S + ["lse_strides"] + TAIL + BIAS + ["stream"],
    "fa2_fwd_gqa": ["dtype"] + FWD_T + DIMS_G + FWD_S + ["lse_strides"] + TAIL + WS + ["stream"],
    "fa2_fwd_window": ["dtype"] + FWD_T + DIMS_G + FWD_S + ["lse_strides"] + TAIL + WIN + ["stream"],
    "fa2_fwd_dropout": ["dtype"] + FWD_T + DIMS_G + FWD_S + ["lse_strides"] + TAIL + WIN + ["stream"] + DROP,
    "fa2_fwd_varlen": ["dtype"] + FWD_T + DIMS_G + CU + FWD_S + ["lse_stride"] + TAIL + WIN[:2] + ["stream"],
    "fa2_fwd_varlen_dropout": ["dtype"] + FWD_T + DIMS_G + CU + FWD_S + ["lse_stride"] + TAIL + WIN[:2] + ["stream"] + DROP,
    "fa2_bwd": ["dtype"] + BWD_T + DIMS + BWD_S + ["lse_strides"] + TAIL + ["stream"],
    "fa2_bwd_f16": BWD_T + DIMS + BWD_S + ["lse_strides"] + TAIL + ["stream"],
    "fa2_bwd_bf16": BWD_T + DIMS + BWD_S + ["lse_strides"] + TAIL + ["stream"],
    "fa2_bwd_ws": ["dtype"] + BWD_T + DIMS + BWD_S + ["lse_strides"] + TAIL + WS + ["stream"],
    "fa2_bwd_bias": ["dtype"] + BWD_T + DIMS + BWD_S + ["lse_strides"] + TAIL + BIAS + ["stream"],
    "fa2_bwd_bias_ws": ["dtype"] + BWD_T + DIMS + BWD_S + ["lse_strides"] + TAIL + BIAS + WS + ["stream"],
    "fa2_bwd_gqa": ["dtype"] + BWD_T + DIMS_G + BWD_S + ["lse_strides"] + TAIL + WS + ["stream"],
    "fa2_bwd_window": ["dtype"] + BWD_T + DIMS + BWD_S + ["lse_strides"] + TAIL + WIN + ["stream"],
    "fa2_bwd_dropout": ["dtype"] + BWD_T + DIMS + BWD_S + ["lse_strides"] + TAIL + WIN + ["stream"] + DROP,
    "fa2_bwd_varlen": ["dtype"] + BWD_T + DIMS + CU + BWD_S + ["lse_stride"] + TAIL + WIN[:2] + ["stream"],
    "fa2_bwd_varlen_dropout": ["dtype"] + BWD_T + DIMS + CU + BWD_S + ["lse_stride"] + TAIL + WIN[:2] + ["stream"] + DROP,
}
TENSORS = BWD_T + ["bias"] + CU + ["workspace"]
NAN, INF = float("nan"), float("inf")


def valid_call(entry):
    """One call of `entry` that every check accepts: B2 H4 (Hkv2) Nq130 Nkv200 D64, contiguous tensors at stand-in addresses (never dereferenced: the
    rows of the table all fail a check before the launch)."""
    names = ENTRIES[entry]
    packed, grouped = "cu_seqlens_q" in names, "Hkv" in names
    B, H, Nq, Nkv, D = 2, 4, 130, 200, 64
    Hkv = 2 if grouped else H
    v = {"dtype": 1, "B": B, "H": H, "Hkv": Hkv, "Nq": Nq, "Nkv": Nkv, "D": D, "scale": 0.125, "stream": None, "workspace_bytes": 1 << 20,
         "window_left": 65, "window_right": 0, "q_offset": 70, "dropout_p": 0.25, "seed": 1234, "lse_stride": Nq * B, "lse_strides": [H * Nq, Nq],
         "flags": (BOTTOM_RIGHT | CAUSAL) if packed else CAUSAL, "bias_kind": 2, "bias_strides": [H * Nq * Nkv, Nq * Nkv, Nkv]}
    for i, t in enumerate(TENSORS):
        v[t] = 0x100000 * (i + 1)
    for s in BWD_S:
        heads, rows = (Hkv, Nkv) if s[:2] in ("k_", "v_", "dk", "dv") else (H, Nq)
        v[s] = [D, heads * D] if packed else [heads * rows * D, rows * D, D]
    return {n: v[n] for n in names}


def _set(key, value):
    return key, lambda v: value


def _stride(key, index_from_end, value):
    def f(v):
        v = list(v)
        v[len(v) - index_from_end] = value
        return v
    return key, f


def defects(entry):
    """[(name, key, change)] — every way this table breaks the valid call of `entry`; a pair of defects on the same key is not formed."""
    names = ENTRIES[entry]
    packed, bwd = "cu_seqlens_q" in names, "dq" in names
    d = []
    for n in names:
        if n in TENSORS and n != "workspace":         # (a null workspace is a valid call)
            d.append(("null:" + n,) + _set(n, None))
        if n.endswith("_strides"):
            d.append(("null:" + n,) + _set(n, None))
    d.append(("misaligned:q", "q", lambda v: v + 8))
    last = "dv" if bwd else "v"
    d.append(("misaligned:" + last, last, lambda v: v + 8))
    d.append(("stride:k_row_0",) + _stride("k_strides", 1, 0))
    d.append(("stride:q_head_4",) + _stride("q_strides", 1 if packed else 2, 4))
    d.append(("stride:o_row_12",) + _stride("o_strides", 1, 12))
    d.append(("span:v_row_2^27",) + _stride("v_strides", 1, 1 << 27))                # 199 rows of 2^28 bytes: >= 2 GiB
    if "dtype" in names:
        d.append(("dtype=2",) + _set("dtype", 2))
    for n, bad in (("B", [0]), ("H", [0]), ("Hkv", [0, 3, 8]), ("Nq", [0]), ("Nkv", [0]), ("D", [0, 12, 520])):
        if n in names:
            d += [("%s=%d" % (n, b),) + _set(n, b) for b in bad]
    d.append(("grid:B=2^30",) + _set("B", 1 << 30))                                    # B * H * ceil(Nq / 256) = 2^32
    d.append(("scale=nan",) + _set("scale", NAN))
    d.append(("scale=inf",) + _set("scale", INF))
    d.append(("flags|8", "flags", lambda v: v | 8))
    if not packed:
        d.append(("flags|BOTTOM_RIGHT", "flags", lambda v: v | BOTTOM_RIGHT))
    for n in WIN:
        if n in names:
            d.append(("%s=-2" % n,) + _set(n, -2))
    if "dropout_p" in names:
        d += [("dropout_p=%r" % p,) + _set("dropout_p", p) for p in (1.0, -0.5, NAN)]
    if "bias" in names:
        d.append(("bias_kind=7",) + _set("bias_kind", 7))
        d.append(("bias_stride<0",) + _stride("bias_strides", 2, -8))
        d.append(("misaligned:bias", "bias", lambda v: v + 2))
        if bwd:             # (the backward addresses a (b, h) slice of the bias with 32-bit offsets; the forward has no such limit)
            d.append(("span:bias_row_2^29",) + _stride("bias_strides", 1, 1 << 29))
    return d


def call_entry(lib, entry, values):
    args = []
    for n in ENTRIES[entry]:
        x = values[n]
        if n.endswith("_strides") and x is not None:
            x = (ctypes.c_int64 * len(x))(*x)
        args.append(x)
    return getattr(lib, entry)(*args)


def error_rows(lib):
    """-> (entry names, defect names, int32 [rows, 4]: entry, defect, second defect or -1, code)."""
    entries, dnames, rows = sorted(ENTRIES), [], []
    for ei, entry in enumerate(entries):
        ds = defects(entry)
        for name, _, _ in ds:
            if name not in dnames:
                dnames.append(name)
        combos = [(a,) for a in ds] + [c for c in itertools.combinations(ds, 2) if c[0][1] != c[1][1]]
        for combo in combos:
            v = valid_call(entry)
            for _, key, change in combo:
                v[key] = change(v[key])
            ids = [dnames.index(c[0]) for c in combo] + [-1]
            rows.append([ei, ids[0], ids[1], call_entry(lib, entry, v)])
    return entries, dnames, np.asarray(rows, dtype=np.int32)


def replay_error_row(lib, entries, dnames, row):
    """The code the library under test gives for one recorded row."""
    entry = entries[row[0]]
    by_name = {d[0]: d for d in defects(entry)}
    v = valid_call(entry)
    for di in row[1:3]:
        if di >= 0:
            _, key, change = by_name[dnames[di]]
            v[key] = change(v[key])
    return call_entry(lib, entry, v)


def main():
    import torch
    if torch.cuda.is_available():
        sys.exit("make_abi_golden.py pins the host layer's answers for the default 256 CUs: run it on a machine without a GPU")
    from rocwmma_fattn import _fa2_lib
    lib = _fa2_lib.load()
    out = {}
    pg, sg = plan_grids(), size_grids()
    plans = {name: run_plan_grid(lib, g) for name, g in pg.items()}
    table, inverse = np.unique(np.concatenate(list(plans.values())), axis=0, return_inverse=True)
    assert len(table) < 65536
    out["plan_rows"] = table.astype(np.int32)
    at = 0
    for name, rows in plans.items():
        out["plans/" + name] = inverse.reshape(-1)[at:at + len(rows)].astype(np.uint16)
        at += len(rows)
    for name, g in sg.items():
        out["sizes/" + name] = run_size_grid(lib, g)
    entries, dnames, rows = error_rows(lib)
    assert (rows[:, 3] < 0).all(), "a row of the error table got past the checks: %r" % rows[rows[:, 3] >= 0][:5].tolist()
    # a valid call must reach the launch (hipErrorNoDevice = 100 here): the defects, not the stand-ins, are what the rows above report
    for entry in entries:
        assert call_entry(lib, entry, valid_call(entry)) == 100, entry
    out["errors"] = rows
    out["meta"] = np.array(json.dumps({"plan_grids": pg, "size_grids": sg, "entries": entries, "defects": dnames}))
    np.savez_compressed(FIXTURE, **out)
    print("%s: %d bytes, %d plan rows (%d distinct), %d size rows, %d error rows" % (
        FIXTURE, os.path.getsize(FIXTURE), sum(len(p) for p in plans.values()), len(table), sum(len(out["sizes/" + n]) for n in sg), len(rows)))


if __name__ == "__main__":
    main()
