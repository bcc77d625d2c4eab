// fa2_window.h — the range arithmetic of sliding-window (local) attention, shared by the kernels, the launchers and the C-ABI queries
// fa2_window_tile_range / fa2_window_row_range (include/fa2_gfx950.h), so that it can be tested on the CPU against brute force.
//
// Positions.  Query row i sits at key position i + off (off = q_offset >= 0 on the windowed entry points); it attends key j iff
//     (left  < 0 or j >= i + off - left) and (right < 0 or j <= i + off + right) and 0 <= j < Nkv
// (-1 = unbounded).  The causal flag of a windowed call means right = 0 (window_normalize_right): the kernels only ever see (left, right, off).
// Both bounds of a row grow by one per row, so the live rows of a block (rows that see a key at all) are contiguous, and so is the union of
// their key intervals: a block's visible keys are [lo of its first live row, hi of its last live row].  The same holds for the transpose.
// The host validates Nq + |off| + max(left, right) and Nkv + |off| + max(left, right) against 32-bit overflow (window_args_ok): plain int arithmetic here.
//
// Negative offsets (packed attention, fa2_fwd_varlen: off = Nkv_s - Nq_s of a sequence with fewer keys than queries, bottom-right aligned).  The span
// arithmetic below holds for them unchanged; what changes is that the live rows of a block are no longer a prefix of it: rows with i + off + right < 0
// are dead at the TOP (their whole interval lies left of key 0).  They are still contiguous, and the first live row's interval starts at key 0, so
// [max(0, lo of the block's first row), hi of its last live row] is still tight.  The windowed entry points keep refusing off < 0 (window_args_ok's
// default); lengths of 0 (an empty sequence on either side) give empty spans.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FA2_WIN_HD __host__ __device__
#else
#define FA2_WIN_HD
#endif

namespace fa2 {

struct Window {
    int left = -1, right = -1, off = 0;      // -1 = unbounded
};

// `causal` on a windowed call: nothing to the right of the query's own position
FA2_WIN_HD inline int window_normalize_right(int right, int causal) { return causal ? 0 : right; }

// -1 (unbounded) or >= 0, off >= 0 (negative_off: any sign — the packed entry points), and every position sum used below stays inside int
FA2_WIN_HD inline bool window_args_ok(int Nq, int Nkv, int left, int right, int off, bool negative_off = false) {
    if (left < -1 || right < -1 || (off < 0 && !negative_off)) return false;
    const long long m = (left > right ? left : right) > 0 ? (left > right ? left : right) : 0;
    const long long n = Nq > Nkv ? Nq : Nkv;
    const long long a = off < 0 ? -(long long)off : (long long)off;
    return n + a + m + 1024 <= 0x7fffffffLL;
}

// does the window mask nothing at all for these lengths?  (then the call is a plain one)
FA2_WIN_HD inline bool window_is_full(int Nq, int Nkv, int left, int right, int off) {
    const bool l = left < 0 || (long long)(Nq - 1) + off - left <= 0;          // the last row still sees key 0
    const bool r = right < 0 || (long long)off + right >= Nkv - 1;             // the first row already sees the last key
    return l && r;
}

// Keys visible to the query rows [row0, row0 + rows) ∩ [0, Nq): the inclusive interval [*klo, *khi]; false = no row of the block sees a key.
FA2_WIN_HD inline bool window_key_span(int Nq, int Nkv, int left, int right, int off, int row0, int rows, int* klo, int* khi) {
    int r1 = (row0 + rows < Nq ? row0 + rows : Nq) - 1;                          // last row of the block
    if (row0 < 0) row0 = 0;
    if (left >= 0 && r1 > Nkv - 1 + left - off) r1 = Nkv - 1 + left - off;       // rows past this one start beyond the last key: dead
    if (r1 < row0) return false;
    const int lo = left < 0 ? 0 : row0 + off - left;
    *klo = lo > 0 ? lo : 0;
    const int hi = right < 0 ? Nkv - 1 : r1 + off + right;
    *khi = hi < Nkv - 1 ? hi : Nkv - 1;
    return *klo <= *khi;
}

// Query rows that see at least one of the keys [key0, key0 + keys) ∩ [0, Nkv): the transposed band (key j is seen by the rows
// j - off - right ... j - off + left).
FA2_WIN_HD inline bool window_row_span(int Nq, int Nkv, int left, int right, int off, int key0, int keys, int* rlo, int* rhi) {
    int j1 = (key0 + keys < Nkv ? key0 + keys : Nkv) - 1;
    int j0 = key0 > 0 ? key0 : 0;
    if (left >= 0 && j0 < off - left) j0 = off - left;                           // keys before this one end above row 0: unseen
    if (right >= 0 && j1 > Nq - 1 + off + right) j1 = Nq - 1 + off + right;      // keys past this one start below the last row: unseen
    if (j1 < j0) return false;
    const int lo = right < 0 ? 0 : j0 - off - right;
    *rlo = lo > 0 ? lo : 0;
    const int hi = left < 0 ? Nq - 1 : j1 - off + left;
    *rhi = hi < Nq - 1 ? hi : Nq - 1;
    return *rlo <= *rhi;
}

// The KV tiles (of `tile` keys) a block of query rows has to sweep: [*first, *first + *n); n = 0 when the block sees nothing (first = 0 then).
// Tight: the first and the last tile each hold a visible (row, key) pair.
FA2_WIN_HD inline void window_tile_range(int Nq, int Nkv, int left, int right, int off, int row0, int rows, int tile, int* first, int* n) {
    int lo, hi;
    if (!window_key_span(Nq, Nkv, left, right, off, row0, rows, &lo, &hi)) { *first = 0; *n = 0; return; }
    *first = lo / tile;
    *n = hi / tile - *first + 1;
}

// The Q tiles (of `tile` rows) a block of keys has to sweep in the dK / dV passes.
FA2_WIN_HD inline void window_row_range(int Nq, int Nkv, int left, int right, int off, int key0, int keys, int tile, int* first, int* n) {
    int lo, hi;
    if (!window_row_span(Nq, Nkv, left, right, off, key0, keys, &lo, &hi)) { *first = 0; *n = 0; return; }
    *first = lo / tile;
    *n = hi / tile - *first + 1;
}

}  // namespace fa2
