"""MI355X (gfx950) drop-in for the reference package `rocwmma_fattn` (forward attention path)."""

_LAZY = ("kvcache_append_varlen", "kvcache_append_mla", "kvcache_append_mla_varlen")


def __getattr__(name):
    """`rocwmma_fattn.kvcache_append_varlen` and the latent-cache appends: FlashAttn (and torch with it) is imported when a name is first asked for."""
    if name in _LAZY:
        from . import FlashAttn
        return getattr(FlashAttn, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
