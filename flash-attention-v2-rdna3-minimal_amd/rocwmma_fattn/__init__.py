"""MI355X (gfx950) drop-in for the reference package `rocwmma_fattn` (forward attention path)."""


def __getattr__(name):
    """`rocwmma_fattn.kvcache_append_varlen`: FlashAttn (and torch with it) is imported when the name is first asked for."""
    if name == "kvcache_append_varlen":
        from .FlashAttn import kvcache_append_varlen
        return kvcache_append_varlen
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
