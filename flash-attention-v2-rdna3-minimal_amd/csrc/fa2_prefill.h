// fa2_prefill.h — chunked prefill against a KV cache (fa2_fwd_prefill; include/fa2_gfx950.h has the contract): what the FA2_PAGED form of the forward kernel
// (fa2_fwd_kernel.hip.h; prefill_hip.cpp, prefill_scoremod_hip.cpp) shares with the host — the further kernel argument and the arithmetic that maps a
// 64-key tile of a sequence to a place in the cache, which the C-ABI exports as fa2_prefill_tile so that it can be tested on the CPU against brute force.
//
// The cache is a pool of pages under a block table, or — the contiguous layout — one page per sequence: page id = the sequence, page stride = the batch
// stride, keys per page = the capacity rounded up to whole tiles (so no tile index below the capacity ever leaves page slot 0).  A pool's page holds a
// multiple of 64 keys, a tile is 64 keys: no tile straddles a page, and a tile's rows are consecutive in memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FA2_PREFILL_HD __host__ __device__
#else
#define FA2_PREFILL_HD
#endif

namespace fa2 {

constexpr int kPrefillTile = 64;         // = kKvTile of the forward kernel

// What a prefill call adds to the parameter block of its kernels: one further kernel argument (FwdParams keeps its layout).  The page stride travels
// in FwdParams::ks[0] / vs[0] (the packed kernels' batch stride, which such a call does not use otherwise), cu_seqlens_q where the packed calls keep it.
struct PagedKv {
    const int* lens = nullptr;           // cache_seqlens [B], device memory: the valid keys of a sequence including its new tokens
    const int* bt = nullptr;             // block table [B, max_pages], device memory; nullptr: the contiguous layout
    int64_t bts = 0;                     // elements between two block-table rows
    int page_keys = 0;                   // keys per page (contiguous: the capacity rounded up to whole tiles)
    int num_pages = 0;                   // pages in the pool: every page id is clamped into [0, num_pages)
    int capacity_keys = 0;               // key slots of one sequence: every length is clamped into [0, capacity_keys]
};

// What a prefill call on an e4m3 cache adds to that (fa2_fwd_prefill_fp8; the FA2_KV8 kernels alone take it, as one more kernel argument behind PagedKv,
// so the 16-bit kernels keep their kernarg segment): the per (sequence, K / V head) descales, device data like the lengths.
struct KvDescale {
    const float* k = nullptr;            // k_descale [B, Hkv] f32, device memory; nullptr: 1.0
    const float* v = nullptr;            // v_descale, likewise
    int64_t s[2] = {0, 0};               // their element strides {sequence, K / V head}
};

// keys per page as the kernels count them
FA2_PREFILL_HD inline int prefill_page_keys(int page_size, int64_t capacity_keys) {
    return page_size > 0 ? page_size : (int)((capacity_keys + kPrefillTile - 1) / kPrefillTile * kPrefillTile);
}
FA2_PREFILL_HD inline int prefill_clamp_len(int64_t len, int64_t capacity_keys) { return (int)(len < 0 ? 0 : len > capacity_keys ? capacity_keys : len); }
FA2_PREFILL_HD inline int prefill_clamp_page(int pid, int num_pages) { return pid < 0 ? 0 : pid >= num_pages ? num_pages - 1 : pid; }

// Tile t of a sequence of `len` keys (clamped already): the block-table slot of its page, its first row inside that page, and how many of its 64 rows
// hold a key of the sequence (0: the tile lies at or beyond the length).
struct PrefillTile { int slot, row, rows; };
FA2_PREFILL_HD inline int prefill_tile_rows(int key0, int len) {
    const int left = len - key0;
    return left <= 0 ? 0 : left < kPrefillTile ? left : kPrefillTile;
}
FA2_PREFILL_HD inline PrefillTile prefill_tile(int t, int len, int page_keys) {
    const int key0 = t * kPrefillTile;
    PrefillTile r;
    r.slot = key0 / page_keys;
    r.row = key0 - r.slot * page_keys;
    r.rows = prefill_tile_rows(key0, len);
    return r;
}
// ... and the tile after it, without a division (the kernel's running counters)
FA2_PREFILL_HD inline void prefill_tile_next(PrefillTile& r, int key0_next, int len, int page_keys) {
    r.row += kPrefillTile;
    if (r.row >= page_keys) { r.row = 0; ++r.slot; }
    r.rows = prefill_tile_rows(key0_next, len);
}

}  // namespace fa2
