"""MI355X (gfx950) drop-in for the reference package `rocwmma_fattn` (forward attention path)."""

_LAZY = ("kvcache_append_varlen", "kvcache_append_mla", "kvcache_append_mla_varlen", "mla_cache_to_fp8", "mla_cache_from_fp8", "mla_indexer_logits", "topk_indices",
         "mla_indexer_topk", "mla_indexer_q_to_fp8", "mla_index_cache_to_fp8", "mla_index_cache_from_fp8", "kvcache_append_mla_index", "mla_indexer_logits_varlen",
         "topk_indices_varlen", "mla_indexer_topk_varlen", "flash_attention_prefill_mla")


def __getattr__(name):
    """`rocwmma_fattn.kvcache_append_varlen` and the latent-cache appends: FlashAttn (and torch with it) is imported when a name is first asked for."""
    if name in _LAZY:
        from . import FlashAttn
        return getattr(FlashAttn, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
