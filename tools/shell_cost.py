"""What the compiled shell of the hand-scheduled forward kernels costs (developer tool, no GPU).

  python tools/shell_cost.py [--json] [--keep FILE.s]

Compiles csrc/fwd_asm.cpp to gfx950 assembly with build.py's HIPCC_FLAGS and reports, for every instantiation of
fa2::fwd_asm_kernel (csrc/fa2_fwd_d128.hip.h):

  private   the private segment size of the kernel descriptor (.amdhsa_private_segment_fixed_size): scratch bytes per lane
  entry     instructions between the header of the persistent loop and the #ASMSTART of the generated body
  exit      instructions of the loop behind the body's #ASMEND (with the latch, wherever the layout put it)

The counts are static: every block of the loop, the paths a trip does not take (ragged tiles, the redo) included.  A guard
against the shell growing, not a cycle count.
"""
import argparse
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
PKG = os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd")

KERNEL_RE = re.compile(r"^(_ZN3fa214fwd_asm_kernelILi(\d+)E((?:Lb[01]E)+)E\S*):\s*(;.*)?$")
BLOCK_RE = re.compile(r"^\.L(BB\w+):\s*(;.*)?$")
NOTE_RE = re.compile(r"^\s+;.*(Loop|Depth)")
INSN_RE = re.compile(r"^\s+[a-z][a-z0-9_]*(\s|$)")


def _build_module():
    spec = importlib.util.spec_from_file_location("_fa2_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def compile_asm(out_path):
    """csrc/fwd_asm.cpp -> device assembly, with the flags of the product build (the generated bodies are made first)."""
    b = _build_module()
    b.generate()
    flags = [f for f in b.HIPCC_FLAGS if f != "--offload-compress"]
    cmd = [b._hipcc()] + flags + ["-I", b.INCLUDE, "-I", b.CSRC, "--cuda-device-only", "-S", os.path.join(b.CSRC, "fwd_asm.cpp"), "-o", out_path]
    res = subprocess.run(cmd, cwd=b.CSRC, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed (%d):\n%s" % (res.returncode, res.stderr[-4000:]))
    return out_path


def instantiation(tmpl_hd, tmpl_bools):
    """(HD, BF16, CAUSAL, FOLD, M16, LM) of a mangled instantiation."""
    bits = [int(x) for x in re.findall(r"Lb([01])E", tmpl_bools)]
    bits += [0] * (5 - len(bits))
    return (int(tmpl_hd),) + tuple(bits[:5])


def analyse(lines):
    """{mangled name: {"inst": (...), "private": int, "entry": int, "exit": int}} for every fwd_asm_kernel in the assembly."""
    out = {}
    i, n = 0, len(lines)
    while i < n:
        m = KERNEL_RE.match(lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        j = i + 1
        while j < n and not lines[j].startswith(".Lfunc_end"):
            j += 1
        out[name] = dict(inst=instantiation(m.group(2), m.group(3)), private=None, **shell_counts(lines[i + 1:j]))
        i = j
    # the kernel descriptors: .amdhsa_kernel NAME ... .amdhsa_private_segment_fixed_size N ... .end_amdhsa_kernel
    cur = None
    for l in lines:
        s = l.split()
        if len(s) == 2 and s[0] == ".amdhsa_kernel":
            cur = s[1] if s[1] in out else None
        elif cur and len(s) == 2 and s[0] == ".amdhsa_private_segment_fixed_size":
            out[cur]["private"] = int(s[1])
        elif s and s[0] == ".end_amdhsa_kernel":
            cur = None
    return out


def shell_counts(body):
    """The compiler annotates every basic block with the loop it belongs to ("=>This Inner Loop Header: Depth=1", "in Loop: Header=BB39_4 Depth=1",
    "Parent Loop BB39_4 Depth=1"): the persistent loop is the depth-1 loop around the generated body.  Its blocks in front of the body, from the
    header on, are the entry; its blocks behind the body, and those the layout put in front of the header (the rotated latch), are the exit."""
    # the generated body is the longest #ASMSTART ... #ASMEND stretch of the function (the others are the empty statements of the shell)
    spans, start = [], None
    for k, l in enumerate(body):
        if "#ASMSTART" in l:
            start = k
        elif "#ASMEND" in l and start is not None:
            spans.append((start, k))
            start = None
    if not spans:
        return dict(entry=None, exit=None)
    a0, a1 = max(spans, key=lambda s: s[1] - s[0])
    # blocks: (first line, label, loop annotation)
    blocks = []
    for k, l in enumerate(body):
        lm = BLOCK_RE.match(l)
        if lm:
            note, j = lm.group(2) or "", k + 1
            while j < len(body) and NOTE_RE.match(body[j]):
                note += " " + body[j].strip()
                j += 1
            blocks.append((k, lm.group(1), note))
    at_body = [b for b in blocks if b[0] < a0]
    if not at_body:
        return dict(entry=None, exit=None)
    _, label, note = at_body[-1]
    m = re.search(r"(?:Parent Loop|Header=)\s*(BB\w+) Depth=1\b", note)
    if m:
        header = m.group(1)
    elif "Loop Header: Depth=1" in note:
        header = label
    else:                 # no loop around the body
        return dict(entry=None, exit=None)
    in_loop = lambda lab, nt: lab == header or re.search(r"\b%s\b" % re.escape(header), nt) is not None      # noqa: E731
    entry = exit_ = 0
    member, seen_header = False, False
    bi = 0
    for k, l in enumerate(body):
        if bi < len(blocks) and blocks[bi][0] == k:
            member = in_loop(blocks[bi][1], blocks[bi][2])
            seen_header = seen_header or blocks[bi][1] == header
            bi += 1
        if not member or a0 <= k <= a1 or not INSN_RE.match(l):
            continue
        if seen_header and k < a0:
            entry += 1
        else:
            exit_ += 1
    return dict(entry=entry, exit=exit_)


def measure(keep=None):
    with tempfile.TemporaryDirectory(prefix="fa2_shell_") as d:
        path = keep or os.path.join(d, "fwd_asm.s")
        compile_asm(path)
        with open(path) as f:
            return analyse(f.read().splitlines())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--keep", help="write the assembly here and keep it")
    a = ap.parse_args()
    res = measure(a.keep)
    if a.json:
        print(json.dumps({k: v for k, v in sorted(res.items())}))
        sys.exit(0)
    print("%-4s %-5s %-6s %-4s %-3s %-3s %8s %6s %6s" % ("HD", "bf16", "causal", "fold", "m16", "lm", "private", "entry", "exit"))
    for name, r in sorted(res.items(), key=lambda kv: kv[1]["inst"]):
        print("%-4d %-5d %-6d %-4d %-3d %-3d %8s %6s %6s" % (r["inst"] + (r["private"], r["entry"], r["exit"])))
