"""The asm generators (csrc/gen/*.py) keep no process-global state: what a generator emits depends on its own arguments only — not on which
other generator modules have been imported (they used to rebind isa.Label.text), not on generators built before it in the same process (a
scheduler-weight option used to rewrite sched.WEIGHT for everyone after it).  pytest imports all of them into one process, and so does
tools/kbench.py's build, so the product bodies must not care."""
import importlib
import os
import sys

GEN_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "flash-attention-v2-rdna3-minimal_amd", "csrc", "gen")
sys.path.insert(0, GEN_DIR)

# (module, class, constructor arguments): one default program of every generator class, and the variants with a register map of their own
PROGRAMS = [
    ("bwd_d128_gen", "GenDQ", {}),
    ("bwd_d128_gen", "GenDKV", {}),
    ("bwd_dq_m16_gen", "GenDQ16", {}),
    ("bwd_dkv_m16_gen", "GenDKV16", {}),
    ("fwd_m16_d256_gen", "Gen256", {}),
    ("fwd_m16_gen", "Gen16", {}),
    ("fwd_m16_gen", "Gen16", {"opt": ("ct", "lm")}),
    ("fwd_d128_gen", "Gen", {}),
    ("fwd_d128_gen", "Gen", {"hd": 64, "opt": ("ct",)}),
]


def _build(mod, cls, kw):
    import gen_driver
    c = getattr(importlib.import_module(mod), cls)
    prog = c(False, **kw).build()
    return prog.text_lines(), gen_driver.render_inline(prog, c.STEM)


def test_generators_do_not_depend_on_import_or_build_order():
    import sched
    weights = dict(sched.WEIGHT)
    # the backward generators first: they do not import the forward ones, so at a first import of this process the forward modules are not loaded yet
    first = [_build(*p) for p in PROGRAMS]
    assert all(m in sys.modules for (m, _, _) in PROGRAMS)
    # ... now every generator module is imported; non-default schedules in between must not leak into the default programs either
    _build("fwd_d128_gen", "Gen", {"e": (10.0, 60.0), "dma": (12.0, 26.0), "opt": ("maxfirst",)})
    _build("bwd_d128_gen", "GenDQ", {"valu": (1.0, 40.0)})
    second = [_build(*p) for p in reversed(PROGRAMS)][::-1]
    for (name, a, b) in zip(PROGRAMS, first, second):
        assert a[0] == b[0], ("text_lines() differ", name)
        assert a[1] == b[1], ("inline rendering differs", name)
    assert sched.WEIGHT == weights
    for (mod, cls, _), (text, inline) in zip(PROGRAMS, first):
        stem = getattr(sys.modules[mod], cls).STEM
        labels = [t for t in text if t.endswith(":")]
        # plain text_lines(): bare label names; the statement-unique form is the renderer's argument
        assert labels and not any(t.startswith(".L") or "%=" in t for t in labels), (mod, cls, labels[:3])
        assert '"%s\\n"' % (".L%s_%s_%%=:" % (stem, labels[0][:-1])) in inline.split("\n"), (mod, cls)
