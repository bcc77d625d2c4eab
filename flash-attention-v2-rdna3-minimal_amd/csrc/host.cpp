// host.cpp — C-ABI shim of the gfx950 FlashAttention-2 path (compiled with hipcc -x hip): argument validation, launch
// heuristics and dispatch.  The kernels live in the other translation units of the library (fa2_launch.h).
//
// Layout of the file: the planner (which kernels serve a launch: plan_range, plan_split, plan_fwd) and the launch steps (launch_fwd, launch_bwd);
// the call descriptions FwdCall / BwdCall, which every extern "C" entry point fills by field name; validation (a description -> FwdParams /
// BwdParams + the kernel head dim, or an error code); fwd_run / bwd_run (validate, then answer the plan / size query or launch); the helpers the
// entry points of one family share (dense_window, packed_call, run_query / workspace_query); the entry points.
//
// Counterpart of the reference's host layer:
//   rocwmma_fattn/host.cpp:30-45        dtype switch forward()        -> fa2_fwd
//   rocwmma_fattn/kernel_fp16.cu:744-876 forward_fp16 host launcher   -> fa2_fwd_f16
//   rocwmma_fattn/kernel_bf16.cu:802-941 forward_bf16 host launcher   -> fa2_fwd_bf16
//   rocwmma_fattn/host.cpp:47-58         dtype switch backward()       -> fa2_bwd
//   rocwmma_fattn/kernel_fp16.cu:878-1028 backward_fp16 host launcher  -> fa2_bwd_f16 (bf16 twin -> fa2_bwd_bf16)
// Unlike the reference this layer owns no tensors and allocates nothing: padding, output allocation
// and the 6-tensor return contract live in the Python operator (rocwmma_fattn/FlashAttn.py), the
// launch is asynchronous on the caller's stream, and failures are returned, not printf'ed
// (reference: kernel_fp16.cu:854-863).
#include "fa2_launch.h"
#include "fa2_dropout.h"
#include "fa2_decode_mla.hip.h"      // the latent-cache decode: its constants, the arithmetic the plan shares with the kernel, its launcher
#include "fa2_kvappend_mla.hip.h"    // ... and its append: the parameter block, the unit -> chunks map, its launcher

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "fa2_gfx950.h"

namespace fa2 {

// The tuning switches start from the environment (read once, when the library is loaded) and can be changed at run time
// through fa2_set_option — tests flip them in-process instead of spawning a child process per variant.
Options& options() {
    static Options o;
    static const bool init = [] {
        if (const char* e = std::getenv("FA2_ROWS")) o.rows = std::atoi(e);
        if (const char* e = std::getenv("FA2_ASM")) o.asm_mask = std::atoi(e);
        if (const char* e = std::getenv("FA2_PERSIST")) o.persist = std::atoi(e);
        if (const char* e = std::getenv("FA2_SPLIT")) o.split = std::atoi(e) != 0;
        if (const char* e = std::getenv("FA2_FOLD")) { const int v = std::atoi(e); if (v >= 0 && v <= 2) o.fold = v; }
        if (const char* e = std::getenv("FA2_KFOLD")) o.kfold = std::atoi(e) != 0;
        if (const char* e = std::getenv("FA2_SHORT")) o.short_kv = std::atoi(e) != 0;
        return true;
    }();
    (void)init;
    return o;
}

int device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev >= 0 && dev < 64) {
        const int c = cache[dev].load(std::memory_order_relaxed);
        if (c > 0) return c;
    }
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    if (dev >= 0 && dev < 64) cache[dev].store(cus, std::memory_order_relaxed);
    return cus;
}

}  // namespace fa2

namespace {

constexpr int kHeadDims[] = {64, 128, 256, 512};
constexpr int kMaxBwdHeadDim = 512;   // like the forward (above 256: slab kernels, bwd_hip.cpp)
constexpr int kNumHeadDims = sizeof(kHeadDims) / sizeof(kHeadDims[0]);
constexpr int kFwdRows = 256;         // Q rows per forward workgroup of the default shapes

int forced_rows() { return fa2::options().rows.load(std::memory_order_relaxed); }
int asm_mask() { return fa2::options().asm_mask.load(std::memory_order_relaxed); }
int m16_mode() { return fa2::fwd_m16_mode(asm_mask()); }      // which 16x16x32 forward bodies option "asm" allows (fa2_launch.h)
bool asm_fwd() { return asm_mask() & 1; }

// A grid of 256-row workgroups that covers well under half of the CUs leaves the chip idle: 128-row workgroups double the
// number of busy CUs at the price of staging every K/V tile for half as many rows.  Measured (tools/rows_probe.py, MI355X, 256 CUs):
// 64 workgroups -> 128 of 128 rows: B1 H16 N1024 D128 25.1 -> 20.5 us, B1 H8 N2048 D128 44.1 -> 35.3, B2 H8 N1024 D80 24.0 -> 19.9;
// at 160 workgroups (SDXL 32x32 self-attention) and above the big shape wins (19.9 vs 23.9 us), 64-row workgroups never do.
// Between one and one and a half rounds of 256-row workgroups at head dims <= 64 (non-causal), 128-row workgroups all the way — two per CU since
// they fit the 256-register budget — beat both the plain grid and the tail split (SDXL 64x64 self-attention B2 H10 N4096 D64, 320 workgroups:
// 130.8 plain / 121.2 tail split / 117.4 us; B1 H24 N3072 D64, 288: 97.0 / 90.9 / 84.5 us); at exactly one round (B2 H8 N4096: 66 vs 73 us)
// and below (160 workgroups: 20.0 vs 22.6 us) the 8-wave shape stays ahead.  The thresholds scale with the device's CU count.
bool short_second_round(const fa2::FwdParams& p, bool causal) {
    if (causal || p.D > 64) return false;
    const int64_t w = (int64_t)p.nbh * ((p.Nq + 255) / 256), cus = fa2::device_cus();
    return w > cus && w <= cus + cus / 2;
}

int pick_rows(const fa2::FwdParams& p, bool causal = true) {
    const int f = forced_rows();
    if (f == 128 || f == 256) return f;
    if (p.rows_hint == 128 || p.rows_hint == 256) return p.rows_hint;
    if (short_second_round(p, causal)) return 128;
    return (int64_t)p.nbh * ((p.Nq + 255) / 256) <= fa2::device_cus() * 3 / 8 ? 128 : 256;
}

// Tail split (non-causal): B*H*ceil(Nq/256) equal workgroups on the CUs take ceil(x/CUs) rounds however empty the last one
// is — SDXL's 64x64 self-attention (B2 H10 N4096) is 320 workgroups, two rounds for 1.25 rounds of work.  When the last
// round would be at most half full, the heads that make it up run in a second launch as 128-row workgroups (twice as
// many, ~0.85x as long each: they stream the same K/V for half the rows).  Measured at D = 64 (tools/rows_probe.py): B2 H10
// N4096 130.8 -> 123.9 us, B1 H24 N3072 97.0 -> 92.5 us; one SDXL UNet step's attention 3.11 -> 3.02 ms.  Returns the number of
// heads of the main launch (= nbh: no split).
int tail_split_heads(const fa2::FwdParams& p, bool causal) {
    if (causal || forced_rows() != 0) return p.nbh;
    if (short_second_round(p, causal)) return p.nbh;            // 128-row workgroups for the whole grid instead (pick_rows)
    // a second launch costs ~5 us: only sweeps of at least 16 KV tiles (a workgroup then runs >= ~15 us) can win it back.  SDXL's
    // cross-attention (B2 H10 N4096 x Nkv 77, two tiles) measured 13.8 us split into two launches against 10.1 us for torch SDPA.
    if (p.Nkv < 16 * fa2::kKvTile) return p.nbh;
    const int64_t cus = fa2::device_cus(), nq = (p.Nq + 255) / 256, w = (int64_t)p.nbh * nq;
    if (w <= cus || nq > cus) return p.nbh;
    const int64_t main_heads = (w / cus) * cus / nq;           // whole heads that fit the full rounds
    const int64_t tail_w = (p.nbh - main_heads) * nq;           // 256-row workgroups of the remaining heads
    if (main_heads <= 0 || tail_w <= 0 || tail_w > cus / 2) return p.nbh;
    return (int)main_heads;
}

// Head dim exactly 128 with a positive scale runs the hand-scheduled 4-wave kernel (fa2_fwd_d128.hip.h) unless option "asm"
// bit 0 is cleared (A/B measurements, tools/kbench.py).  The asm block addresses a head's Q rows with 32-bit byte offsets.
// ... and derives a wave's further LDS-DMA source offsets from its first by flipping granule bits of the byte offset (the K image's swizzle follows
// the row), which is only the same as re-swizzling when a row's byte offset has those bits clear: K's row pitch must be a multiple of one tile
// row (2 * HD bytes).  Contiguous BHND and BNHD tensors are; a column slice of a wider matrix is not and runs on the HIP kernels (found by the
// randomised sweep, tools/fuzz_parity.py, once it drew grids wide enough for these kernels: profiles/r06_fuzz_parity_seed5.json).
bool asm_pitch_ok(int64_t row_stride_elems, int HD) { return row_stride_elems % HD == 0; }
// (round 5) Q is staged by LDS-DMA like K: its row pitch has to be a multiple of one tile row too, and the byte offsets of the (up to 63) rows a
// workgroup's last wave reads past Nq — zero-filled by the descriptor — must not wrap
// (any_pitch: launches of a head dim below the body's take the general form of the LDS-DMA offsets — csrc/gen/fwd_m16_gen.py: trim_offsets)
// (any_pitch launches mark a granule the row does not have with byte offset 0x80000000 — "beyond every descriptor": true only while the Q span
//  itself stays below 2 GiB, as K's and V's do)
bool asm_q_span_ok(const fa2::FwdParams& p, bool any_pitch = false) {
    return ((int64_t)(p.Nq + 64) * p.qs[2] + p.D) * 2 < ((int64_t)1 << (any_pitch ? 31 : 32)) && (any_pitch || p.qs[2] % (p.D > 0 ? p.D : 1) == 0);
}
// ... and pays a fixed head and tail per item (the Q tile through LDS, the first K / V tiles before any MFMA, the drain of the software pipeline):
// over a short KV sweep (cross-attention, low-resolution self-attention) the compiler-scheduled kernels — two waves per SIMD hiding each
// other's prologue — are faster.  tools/asm_kv_ab.py, one box, fp16, B4 H16 N4096, HIP time / hand-scheduled time at Nkv = 77, 256, 512,
// 768, 1024, 2048:  D = 64  0.88 0.90 0.96 0.995 1.015 1.06;  D = 128  1.006 0.86 0.955 1.00 1.03 1.08 (bf16 1.12 0.925 0.99 1.02 1.04 1.07;
// bf16 keeps its two-tile sweeps on the hand-scheduled body, fp16 measured 0.94 .. 1.006 there).  The crossover is the same at B2 and at Nq = 1024.
// Causal self-attention sweeps half the sequence on average: B8 H16, N = 512 768 1024 1536 2048: D = 64 0.90 0.90 0.97 0.88 1.10, D = 128 0.92 0.90
// 0.96 0.89 1.07 (bf16 alike) — the hand-scheduled body from N = 1792 (profiles/r06_asm_kv_ab.txt).  Option "asm" bit 5 and option "rows" = 256 ignore this rule (A/B measurements, tests).
bool asm_folds(bool bf16, const fa2::FwdParams& p);
bool asm_kv_len_ok(int HD, bool bf16, const fa2::FwdParams& p, bool causal) {
    if ((asm_mask() & 32) || forced_rows() == 256) return true;     // (option rows = 256 pins the
    if (causal) return p.Nkv >= 1792;                                                                              //  hand-scheduled kernels: tests)
    // Round 5, re-measured with the 16x16x32 bodies (tools/asm_kv_ab.py, profiles/r18_asm_kv_ab.txt; HIP time / hand-scheduled time at Nkv = 256, 512,
    // 768, 1024, 1536): D = 128 fp16 0.90 1.01 1.07 1.11 1.16, bf16 0.91 1.01 1.05 1.07 1.09 -> from 512 on; D = 64 fp16 (folded) 0.82 0.92 0.99 1.03
    // 1.10 -> from 896 on as before; D = 64 bf16 (f32 scale) 0.81 0.88 0.92 0.97 1.02 -> from 1280 on.
    if (p.Nkv >= (HD == 128 ? 512 : (asm_folds(bf16, p) ? 896 : 1280))) return true;
    return HD == 128 && bf16 && p.Nkv <= 2 * fa2::kKvTile;
}

// Does a launch of the hand-scheduled body fold scale * log2(e) into Q (rounded once to the I/O dtype: FA2_CONTRACT_PRESCALE_Q), or does it scale
// the f32 product like the reference kernel (kernel_fp16.cu:164) and every compiler-scheduled kernel here?  Option "fold": 0 never, 1 (default)
// fp16 launches, 2 bf16 launches too.  Only while c = scale * log2(e) <= 1: the prescaled Q must stay inside the I/O dtype's range whatever the
// caller's Q holds (|q| * c <= |q|); a larger scale runs the f32-scale body of the same schedule (scale > 0.69 could overflow fp16).
bool asm_folds(bool bf16, const fa2::FwdParams& p) {
    const int f = fa2::options().fold.load(std::memory_order_relaxed);
    return (bf16 ? f >= 2 : f >= 1) && p.c <= 1.0f && !p.exact_scale;
}

// What one launch over the heads [p.bh0, p.bh0 + p.nbh) runs: the ONE place that decides it (launch_range executes the plan, fa2_fwd_plan reports it).
struct RangePlan { int kernel, contract; int rows; bool fold; bool short_kv = false; };

// Non-causal sweeps of at most two KV tiles without a bias (cross-attention on a text prompt: Nkv = 77) at head dims <= 128: the single-pass kernel
// (fa2_fwd_short.hip.h; option "short").  Option "rows" pins the streaming kernels (tests, A/B).
bool short_kv_ok(int HD, const fa2::FwdParams& p, bool causal) {
    return !causal && HD <= 128 && p.Nkv <= 2 * fa2::kKvTile && p.bias_kind == FA2_BIAS_NONE && forced_rows() == 0 &&
           fa2::options().short_kv.load(std::memory_order_relaxed) != 0;
}

// A head dim below the body's that the 16x16x32 bodies take (see plan_range)
bool asm_trimmed(int HD, bool bf16, const fa2::FwdParams& p, bool fold) {
#ifndef FA2_TRIM_MIN64       // (developer A/B: tools/kbench.py build NAME:-DFA2_TRIM_MIN64=32,-DFA2_TRIM_MIN128=80,only=host)
#define FA2_TRIM_MIN64 40
#endif
#ifndef FA2_TRIM_MIN128
#define FA2_TRIM_MIN128 88      // (B2 H16 N4096 fp16, same file: D = 72 +4 %, 80 +2 %, 88 +7 %, 96 +6 %; D = 24 / 32 on the 64 body: -1 %)
#endif
    return p.D < HD && p.D >= (HD == 64 ? FA2_TRIM_MIN64 : fold ? FA2_TRIM_MIN128 : 104) && fa2::fwd_asm_m16_kind(HD, bf16, p, fold, m16_mode()) != fa2::kM16None;
}

// Head dim exactly 256 (round 6): the hand-scheduled 128-row kernel (fa2_fwd_d256.hip.h; option "asm" bit 10).  It scales the f32 product and adds the
// rounded P into the row sums on the matrix pipe (FA2_CONTRACT_LSUM_P16), so calls flagged FA2_FLAG_EXACT_SCALE keep the compiler-scheduled kernels;
// its LDS-DMA pieces are derived from piece 0 by flipping offset bits: K / V row pitches must be multiples of one 512-byte tile row; Q and O are
// addressed with 32-bit offsets from the head base; short KV sweeps stay on the 8-wave kernels (two waves per SIMD hide each other's prologue).
bool asm_d256_ok(bool bf16, const fa2::FwdParams& p, bool causal) {
    (void)bf16;
    const int mask = asm_mask();
#ifndef FA2_D256_TRIM_MIN      // (developer A/B: tools/kbench.py build NAME:-DFA2_D256_TRIM_MIN=144,only=host)
#define FA2_D256_TRIM_MIN 136
#endif
    if (!(mask & 1) || !(mask & 1024) || p.D > 256 || p.D < FA2_D256_TRIM_MIN || p.negate_q || p.exact_scale || p.bias_kind != 0) return false;
    // Head dims below 256 run ceil(D / 32) k-steps of the body (fwd_asm.cpp).  tools/d256_ab.py, one box (profiles/r21_d256_ab.txt), against the trimmed
    // compiler-scheduled kernels: D 176 .. 248 1.25 .. 1.51x, causal or not; D 136 .. 160 (the 8-wave kernel runs those in ONE pass over all columns)
    // non-causal 1.03 .. 1.05x, causal 0.86x at N = 4096: those keep the 8-wave kernel when causal.
    if (p.D < 176 && causal) return false;
    // D == 256: the pieces of a wave's LDS-DMA share are derived from piece 0 by flipping offset bits — row pitches that are multiples of one 512-byte
    // tile row; below, the general form of the offsets: any pitch
    if (p.D == 256 && (p.ks[2] % 256 || p.vs[2] % 256)) return false;
    // Q and O rows are addressed with 32-bit byte offsets from the head base, and every wave of the last workgroup forms them, also one wholly past Nq
    // (its loads and stores fall outside the descriptor): rows up to Nq - 1 + 96 + 31, plus 504 bytes inside the row — 128 rows of slack, so that no
    // offset wraps back into the descriptor's range
    if (((int64_t)(p.Nq + 128) * p.qs[2] + 256) * 2 >= ((int64_t)1 << 32) || ((int64_t)(p.Nq + 128) * p.os[2] + 256) * 2 >= ((int64_t)1 << 32)) return false;
    if (forced_rows() == 256) return false;              // (option rows = 256 pins the 256-row kernels: tests, A/B)
    return (mask & 32) || p.Nkv >= (causal ? 1024 : 512);
}

// Launches the hand-scheduled persistent kernels of head dims 128 and 64 can take, the workgroup shape aside (plan_range adds the rows checks): the
// one eligibility predicate — plan_range asks it for the launch at hand, plan_split / plan_fwd for the non-causal rounds beside the parts of a split.
bool asm_eligible(int HD, bool bf16, const fa2::FwdParams& p, bool causal) {
    // Head dim exactly 128 with a positive scale: the hand-scheduled 4-wave kernel (256-row workgroups).  Head dim 64 has its generated
    // body too (same generator, half the MFMAs per tile for the same softmax work, row sums on the matrix pipe), but a lone wave per SIMD
    // issues that VALU-bound mix no faster than the two waves of the compiler-scheduled 8-wave kernel: same box (tools/fwd_ab.py) B2 H16
    // N4096 933 vs 947 TF, B1 H24 N8192 1032 vs 1022, causal bf16 917 vs 869 — so it takes the causal launches (+5.5 %) only; option
    // "asm" bit 4 sends every D = 64 launch to it (A/B measurements).
    // (round 3) the body that folds the scale into Q beats the 8-wave kernel non-causal too (+9 %), so every launch that folds takes it.
    const bool fold = asm_folds(bf16, p);
    // (round 5: and every launch the f32-scale 16x16x32 body with the row sums on the matrix pipe takes: calls that are not flagged FA2_FLAG_EXACT_SCALE)
    const bool d64_asm = HD == 64 && (causal || fold || (asm_mask() & 16) || fa2::fwd_asm_m16_kind(HD, bf16, p, fold, m16_mode()) == fa2::kM16F32Lm);
    // Head dims BELOW the body's (round 5; the 16x16x32 bodies only): the padded columns of the Q / K / V images are zero-filled by the LDS-DMA itself (a
    // granule the row does not have gets a source offset beyond the descriptor) and the piece offsets take their general form, so any row pitch goes.
    // The body runs at D / HD of its rate: it takes the head dims where that still beats the trimmed compiler-scheduled kernels
    // (tools/trim_asm_ab.py, profiles/r18_trim_asm_ab.txt, one box): fp16 D = 40 (SD 1.5's 64 x 64 self-attention, B2 H8 N4096) 72.0 -> 64.0 us, D = 48
    // causal +5.8 %, D = 96 +6.5 %, D = 104 .. 120 +19 .. 20 %, D = 112 causal +13 %; bf16 (f32 scale) D = 112 +14 %, D = 96 causal -8.7 %: the folded
    // bodies from 40 / 88 on, the f32-scale ones from 104 on.
    const bool trimmed = asm_trimmed(HD, bf16, p, fold);
    return (HD == 128 || d64_asm) && (p.D == HD || trimmed) && !p.negate_q && asm_fwd() && asm_q_span_ok(p, trimmed) &&
           (trimmed || asm_pitch_ok(p.ks[2], HD)) && asm_kv_len_ok(HD, bf16, p, causal);
}

// the hand-scheduled body's plan: which contract a launch that folds / does not fold the scale runs under
RangePlan asm_range(int HD, bool bf16, const fa2::FwdParams& p, bool fold) {
    // (the folded bodies built on v_mfma_f32_16x16x32 add the rounded P into the row sums — on the matrix pipe; csrc/gen/fwd_m16_gen.py, opt=lm)
    const bool lsum16 = fa2::fwd_asm_lsum16(HD, bf16, p, fold, m16_mode());
    return {FA2_KERNEL_ASM, (fold ? FA2_CONTRACT_PRESCALE_Q : 0) | (lsum16 ? FA2_CONTRACT_LSUM_P16 : 0), 256, fold};
}

RangePlan plan_range(int HD, bool bf16, const fa2::FwdParams& p, bool causal) {
    if (HD == 256 && asm_d256_ok(bf16, p, causal)) return {FA2_KERNEL_ASM, FA2_CONTRACT_LSUM_P16, 128, false};
    if (short_kv_ok(HD, p, causal)) return {FA2_KERNEL_HIP_128, 0, 128, false, true};
    const int rows = pick_rows(p, causal);
    if (asm_eligible(HD, bf16, p, causal) && rows == 256 && pick_rows(p) == 256) return asm_range(HD, bf16, p, asm_folds(bf16, p));
    return {rows == 256 ? FA2_KERNEL_HIP_256 : FA2_KERNEL_HIP_128, 0, rows, false};
}

int launch_range(int HD, bool bf16, const fa2::FwdParams& p, bool causal, hipStream_t stream) {
    const RangePlan r = plan_range(HD, bf16, p, causal);
    // option "asm" bit 6 (default): head dim 128 launches of whole items take the bodies built on v_mfma_f32_16x16x32 (round 5; fwd_asm.cpp)
    if (r.kernel == FA2_KERNEL_ASM && HD == 256) return fa2::launch_fwd_asm_d256(bf16, p, causal, stream);
    if (r.kernel == FA2_KERNEL_ASM)
        return fa2::launch_fwd_asm(HD, bf16, p, causal, r.fold, stream, m16_mode());
    if (r.short_kv) return fa2::launch_fwd_short(bf16, HD, p, stream);
    return fa2::launch_fwd_hip(bf16, HD, p, causal, r.rows, false, stream);
}

// KV-split tail (fa2_fwd_ws).  B*H*ceil(Nq/256) equal workgroups on the CUs take ceil(x / CUs) rounds however empty the last one is: SDXL's
// 64x64 self-attention (B2 H10 N4096 D64) is 320 workgroups — two rounds for 1.25 rounds of work —, the reference harness's own sweep
// (B1 H24 D64, bench_with_sdpa.py:201-224) saw-tooths between 670 and 930 TF with N for the same reason.  With a workspace from the caller the r
// items of the last round are swept by S workgroups each over disjoint KV ranges (r * S parts fill the CUs again) and a small kernel merges the
// partial results (fa2_fwd_kernel.hip.h).  S minimises rounds(r * S) / S plus the fixed cost of the scheme, in units of one whole item:
//   an item sweeps nt KV tiles at ~0.9 us * HD / 64 each (measured: D = 64 N4096 60 us, D = 128 112 us per 256-row item);
//   the merge kernel, its launch and a part's own prologue / epilogue cost ~10 us (+ ~4 us for the extra launch of the D = 128 path);
//   the f32 partial tiles cross memory twice.  The workspace never exceeds 64 MiB (fa2::plan_tail_split, fa2_launch.h).
fa2::SplitPlan plan_split(const fa2::FwdParams& p, int HD, bool bf16, bool causal) {
    fa2::SplitPlan none;
    if (causal || p.bias_kind != FA2_BIAS_NONE || HD > 128 || !fa2::options().split.load(std::memory_order_relaxed)) return none;
    if (short_kv_ok(HD, p, causal)) return none;
    const int f = forced_rows();
    if (f == 128 || p.rows_hint == 128) return none;
    const int64_t items = (int64_t)p.nbh * ((p.Nq + kFwdRows - 1) / kFwdRows);
    const int nt = (p.Nkv + fa2::kKvTile - 1) / fa2::kKvTile;
    // whole rounds on the hand-scheduled persistent kernel (head dim 128; head dim 64 in fp16): the parts need a launch of their own
    // (non-causal launches the hand-scheduled persistent kernels take: head dim 128, and head dim 64 when the launch folds the scale — asm_eligible)
    const bool asm_rounds = asm_eligible(HD, bf16, p, false);
    // (round 6) ... and EVERY item of a grid that covers at most half of the CUs over a long sweep — a decode-sized call: B1 H32 Nq1 Nkv8192 is 32
    // workgroups streaming 134 MB of K / V, 147 us for 30 us of bytes (plan_tail_split, underfilled; the parts run on the 8-wave kernel: plan_fwd)
    return fa2::plan_tail_split(items, nt, 0.9 * HD / 64.0, asm_rounds ? 14.0 : 10.0, fa2::split_ws_bytes(1, 1, HD), fa2::device_cus(), true);
}

// The whole forward call: at most two launches (+ the merge of a split).  plan_fwd decides, launch_fwd executes, fa2_fwd_plan reports.
struct FwdPlan {
    fa2::SplitPlan split;        // nsplit > 1: the last round's items run as KV-split parts (needs the caller's workspace)
    bool split_asm = false;      // ... inside the hand-scheduled persistent kernel (else the 8-wave HIP kernel)
    int main_heads = 0;          // heads [0, main_heads) run `main`, the others `tail` (HD <= 64 tail split; main_heads == nbh: one launch)
    RangePlan main{0, 0, 0, false}, tail{0, 0, 0, false};
};

FwdPlan plan_fwd(int HD, bool bf16, const fa2::FwdParams& p0, bool causal, bool have_ws, size_t ws_bytes) {
    FwdPlan f;
    f.main_heads = p0.nbh;
    if (have_ws) {
        const fa2::SplitPlan pl = plan_split(p0, HD, bf16, causal);
        if (pl.nsplit > 1 && (int64_t)ws_bytes >= fa2::split_ws_bytes(pl.split_items, pl.nsplit, HD)) {
            fa2::FwdParams p = p0;
            p.rows_hint = 256;
            f.split = pl;
            f.split_asm = asm_eligible(HD, bf16, p, false) && pick_rows(p, causal) == 256 &&
                          // (a grid of parts only — plan_split, underfilled: the persistent kernel where a part sweeps at least 24 tiles, else the 8-wave
                          //  kernel, whose prologue is shorter.  Same box, hand-scheduled / 8-wave parts: B1 H8 N4096 D128, 2 parts of 32 tiles, 67.6 / 78.5 us,
                          //  D40 44.5 / 48.3, bf16 D64 48.7 / 53.3; B1 H4 N2048 D128, 4 x 8 tiles, 29.2 / 27.5; B1 H32 Nq1 Nkv8192, 8 x 16, 48.4 / 44.9)
                          (pl.full_items > 0 || ((p.Nkv + fa2::kKvTile - 1) / fa2::kKvTile) / pl.nsplit >= 24);
            f.main = f.split_asm ? asm_range(HD, bf16, p, asm_folds(bf16, p)) : RangePlan{FA2_KERNEL_HIP_256, 0, 256, false};
            return f;
        }
    }
    if (HD <= 64) {     // (measured at D = 128, B1 H24 N4096: 188 -> 194 us — the 128-row shape is too slow there)
        const int main_heads = tail_split_heads(p0, causal);
        if (main_heads < p0.nbh) {
            fa2::FwdParams p = p0;
            p.nbh = main_heads;
            f.main_heads = main_heads;
            f.main = plan_range(HD, bf16, p, causal);
            p.bh0 = p0.bh0 + main_heads;
            p.nbh = p0.nbh - main_heads;
            p.rows_hint = 128;
            f.tail = plan_range(HD, bf16, p, causal);
            return f;
        }
    }
    f.main = plan_range(HD, bf16, p0, causal);
    return f;
}

int launch_fwd(int HD, bool bf16, const fa2::FwdParams& p0, bool causal, hipStream_t stream, void* ws, size_t ws_bytes) {
    const bool have_ws = ws && (reinterpret_cast<uintptr_t>(ws) & 15u) == 0;
    const FwdPlan f = plan_fwd(HD, bf16, p0, causal, have_ws, ws_bytes);
    if (f.split.nsplit > 1) {
        fa2::FwdParams p = p0;
        p.rows_hint = 256;
        p.full_items = f.split.full_items; p.split_items = f.split.split_items; p.nsplit = f.split.nsplit;
        p.ws = (float*)ws;
        int rc;
        if (f.split_asm) {
            // the hand-scheduled persistent kernel: every workgroup works through its whole items, then its parts (the item seam hides a
            // part's load phase like any other item's; the block stores a part's f32 tile itself)
            p.item_cap = f.split.full_items + f.split.split_items * f.split.nsplit;
            rc = fa2::launch_fwd_asm(HD, bf16, p, false, f.main.fold, stream, m16_mode());
        } else {
            rc = fa2::launch_fwd_hip(bf16, HD, p, false, 256, false, stream);
        }
        if (rc) return rc;
        return fa2::launch_fwd_combine(bf16, HD, p, stream);
    }
    if (f.main_heads < p0.nbh) {
        fa2::FwdParams p = p0;
        p.nbh = f.main_heads;
        if (int rc = launch_range(HD, bf16, p, causal, stream)) return rc;
        p.bh0 = p0.bh0 + f.main_heads;
        p.nbh = p0.nbh - f.main_heads;
        p.rows_hint = 128;
        return launch_range(HD, bf16, p, causal, stream);
    }
    return launch_range(HD, bf16, p0, causal, stream);
}

// addressable bytes of n rows of a head's matrix, and whether they — plus one tile of rows past the end: masked lanes add fa2::kOobOffset to such an
// offset, which relies on every in-range offset staying below 2 GiB — fit 31 bits
int64_t span_bytes(int n, const int64_t* s, int D) { return ((int64_t)(n - 1) * s[2] + D) * 2; }
bool span_ok(int n, const int64_t* s, int D) { return span_bytes(n, s, D) + 64 * s[2] * 2 <= 0x7fffffffLL; }

// Head dim exactly 128 runs the hand-scheduled backward kernels (fa2_bwd_d128.hip.h) unless option "asm" bit 1 is cleared; bits 2 / 3 of
// the option take only the dQ pass / only the dK-dV pass off them (A/B measurements of one pass at a time).
struct BwdPlan { int asm_parts; bool neg_delta, kfold, short_dq; };      // the ONE place that decides it: launch_bwd executes the plan, fa2_bwd_plan reports it
BwdPlan plan_bwd(int HD, bool bf16, const fa2::BwdParams& p, bool causal) {
    const int m = asm_mask();
    int asm_parts = 0;
    if (HD == 128 && p.D == 128 && (m & 2)) asm_parts = 3 & ~((m >> 2) & 3) & fa2::kBwdAsmParts;
    // a call with a gradient for the LSE (fa2_bwd_lse): the generated dQ bodies form delta themselves and know no dlse, and the hand-scheduled dK / dV pass
    // only goes with the hand-scheduled dQ pass — both passes are the compiler-scheduled ones (teaching the generators is the follow-up: DESIGN)
    if (p.dlse) asm_parts = 0;
    // row pitches the generated bodies' LDS-DMA offset arithmetic holds for (asm_pitch_ok): the dQ pass stages K and V, the dK / dV pass Q and dO
    if (!asm_pitch_ok(p.ks[2], 128) || !asm_pitch_ok(p.vs[2], 128)) asm_parts &= ~1;
    if (!asm_pitch_ok(p.qs[2], 128) || !asm_pitch_ok(p.dos[2], 128)) asm_parts &= ~2;
    // the hand-scheduled dQ pass reads O's rows (delta = rowsum(dO * O)) at 32-bit byte offsets from the head's base, like Q's and dO's.  Validation bounds
    // those two spans; O is the caller's tensor and may have a wider pitch: an O whose head spans 2 GiB or more runs the compiler-scheduled dQ pass, which
    // forms O's row pointers in 64 bits (fa2_bwd_kernel.hip.h) — the call is served, not refused.  (The product would wrap at 4 GiB; the bound is Q's and
    // dO's 2 GiB: O's loads are the instruction form of theirs and stay in the same range.)
    if (!span_ok(p.Nq, p.os, p.D)) asm_parts &= ~1;
    if (p.Nq % 32 != 0) asm_parts &= ~2;              // the hand-scheduled dK/dV pass sweeps whole 32-row Q tiles
    // grouped-query attention: the hand-scheduled dK/dV body owns one Q head's sweep; the compiler-scheduled wave-pair pass sums the group in-kernel
    // (the hand-scheduled dQ pass then writes +delta, which that pass reads)
    if (p.kv_group > 1) asm_parts &= ~2;
    // the sign delta crosses the workspace with: the hand-scheduled dK/dV pass takes -delta (C operand of its dP product); a dQ pass
    // that is not the hand-scheduled one writes +delta, so the two only go together
    if ((asm_parts & 2) && !(asm_parts & 1)) asm_parts = 0;
    const bool neg_delta = (asm_parts & 2) != 0;
    // Option "fold" reaches the backward too: the hand-scheduled dK / dV pass then recomputes P from K * scale*log2(e) rounded once to the I/O dtype
    // (the forward's folded contract on the other operand of Q.K^T) with L as the C operand of the product — 32 v_fma fewer per body on the wave role
    // every body waits for.  Same guard as the forward: |scale * log2(e)| <= 1 keeps the prescaled K inside the dtype's range.
    const int fopt = fa2::options().fold.load(std::memory_order_relaxed);
    // Round 5: off unless option "kfold" asks for it.  The forward of a differentiated call scales the f32 product (FA2_FLAG_EXACT_SCALE) and so do both
    // backward passes: P is recomputed from the very scores L was formed from.  With the fold, gradients at logits of +-30 and more were 2-4x the
    // suite's tolerance (tests/test_backward_gpu.py::test_hand_scheduled_backward_on_large_logits_under_both_fold_settings).
    const bool kfold = fa2::options().kfold.load(std::memory_order_relaxed) && (bf16 ? fopt >= 2 : fopt >= 1) && std::fabs(p.c) <= 1.0f;
    // (head dim 128 exactly keeps the hand-scheduled dQ pass where that one is available: B8 H16 N4096 x 77, whole backward, 236 us against 246)
    const bool short_dq = !causal && (HD <= 64 || (HD == 128 && !(asm_parts & 1))) && p.Nkv <= 2 * fa2::kKvTile && p.bias_kind == FA2_BIAS_NONE &&
                          forced_rows() == 0 && fa2::options().short_kv.load(std::memory_order_relaxed) != 0;
    return {asm_parts, neg_delta, kfold, short_dq};
}

int launch_bwd(int HD, bool bf16, const fa2::BwdParams& p, bool causal, hipStream_t stream) {
    const int m = asm_mask();
    const int want = fa2::options().bwd_parts.load(std::memory_order_relaxed);      // 3 unless a profiling run asked for one pass only
    const BwdPlan pl = plan_bwd(HD, bf16, p, causal);
    const int asm_parts = pl.asm_parts;
    const bool neg_delta = pl.neg_delta, kfold = pl.kfold, short_dq = pl.short_dq;
    for (int part = 1; part <= 2; part <<= 1) {       // the dQ pass first: it fills the delta workspace the dK / dV pass reads
        if (!(want & part)) continue;
        int rc;
        // (round 6) the dQ pass of a non-causal sweep of at most two KV tiles — cross-attention — is the short-sweep kernel's (fa2_bwd_short.hip.h;
        //  option "short"; option "rows" pins the streaming passes); it leaves delta in the sign the dK / dV pass that follows takes
        if (part == 1 && short_dq) rc = fa2::launch_bwd_short_dq(bf16, HD, p, neg_delta, stream);
        else if (asm_parts & part) rc = fa2::launch_bwd_d128(bf16, p, causal, part, neg_delta, kfold, stream, (m & 128) != 0, (m & 256) != 0);     // option "asm" bits 7 / 8: the 16x16x32 dQ / dK-dV pass
        else rc = fa2::launch_bwd_hip(bf16, HD, p, causal, part, stream);
        if (rc) return rc;
    }
    return 0;
}

// A windowed call as the kernels see it: the causal flag folded into the window (right = 0), and the calls whose window masks nothing for their
// lengths told apart — those ARE plain calls (kind 0) or today's top-left causal call (kind 1) and run exactly what fa2_fwd_gqa / fa2_bwd run.
struct WindowCall { int kind; fa2::Window w; };     // kind: 0 plain, 1 plain causal, 2 windowed, -1 bad arguments
WindowCall reduce_window(int Nq, int Nkv, int left, int right, int off, bool causal) {
    WindowCall c;
    c.kind = -1;
    if (Nq < 1 || Nkv < 1 || !fa2::window_args_ok(Nq, Nkv, left, right, off)) return c;
    c.w.left = left; c.w.right = fa2::window_normalize_right(right, causal); c.w.off = off;
    if (fa2::window_is_full(Nq, Nkv, c.w.left, c.w.right, off)) c.kind = 0;
    else if (c.w.right == 0 && off == 0 && fa2::window_is_full(Nq, Nkv, c.w.left, -1, 0)) c.kind = 1;
    else c.kind = 2;
    return c;
}

bool dropout_p_ok(float p) { return p >= 0.f && p < 1.f; }       // (NaN fails both comparisons)
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool strides_ok(const int64_t* s) { return s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0 && s[2] > 0; }

// ---- One call, described: every extern "C" entry point fills one of these by field name and hands it to fwd_run / bwd_run.
enum class Ask { Launch, Plan, Size };      // what the caller wants: the kernels launched, fa2_fwd_*_plan's report, or a fa2_*_workspace_bytes answer
struct BiasArg { const void* ptr = nullptr; int kind = FA2_BIAS_NONE; const int64_t* strides = nullptr; };
struct Call {                                // what a forward and a backward call have in common
    int dtype = 0, B = 0, H = 0, Hkv = 0, Nq = 0, Nkv = 0, D = 0;      // packed: B = the number of sequences, Nq / Nkv = the stated maximum lengths
    float scale = 0.f;
    int flags = 0;                           // FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE: the causal mask the kernels apply themselves (a window carries its own)
    BiasArg bias;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    void* stream = nullptr;
    bool windowed = false;                   // `window` masks something (reduce_window kind 2): the WIN kernels, contract 0
    fa2::Window window = {};                 // the causal flag folded in (right = 0); packed: the offset field carries the bottom-right flag
    bool packed = false;                     // [total, heads, D] tensors (batch strides 0) and the cu_seqlens arrays, which live in device memory
    const int *cu_q = nullptr, *cu_k = nullptr;
    bool dropout = false;                    // always with a window, which may mask nothing: the seed and the threshold of fa2_dropout.h
    uint64_t seed = 0;
    uint32_t drop_t = 0;
    bool scoremod = false;                   // softcap > 0 or ALiBi slopes (fa2_scoremod.h): always with a window, which may mask nothing; never with dropout
    float softcap = 0.f;
    const float* slopes = nullptr;           // device memory, f32 [.., H]
    int64_t slope_stride = 0;                // elements between two batches' / sequences' slope vectors
    Ask ask = Ask::Launch;
    size_t* ws_need = nullptr;               // Ask::Size
};
struct FwdCall : Call {
    const void *q = nullptr, *k = nullptr, *v = nullptr;
    void* o = nullptr;
    float* lse = nullptr;
    const int64_t *qs = nullptr, *ks = nullptr, *vs = nullptr, *os = nullptr, *ls = nullptr;      // {batch, head, row}; ls: {batch, head}
    fa2_fwd_plan_t* plan = nullptr;          // Ask::Plan
    int Dv = 0;                              // fa2_fwd_varlen_dv: the head dim of v and o, narrower than D (packed calls only); 0 = as D
};
struct BwdCall : Call {
    const void *q = nullptr, *k = nullptr, *v = nullptr, *o = nullptr, *dout = nullptr;
    const float* lse = nullptr;
    void *dq = nullptr, *dk = nullptr, *dv = nullptr;
    float* delta_ws = nullptr;
    fa2_bwd_plan_t* plan = nullptr;          // Ask::Plan
    const float* dlse = nullptr;             // optional: the gradient of the LSE (the *_lse entry points; a plan query: any non-null value = "has one")
    const int64_t* dlses = nullptr;          // ... and its strides {batch, head} (packed: {0, head}); checked last
    const int64_t *qs = nullptr, *ks = nullptr, *vs = nullptr, *os = nullptr, *dos = nullptr, *dqs = nullptr, *dks = nullptr, *dvs = nullptr, *ls = nullptr;
};

// ---- validation: a call description -> FwdParams / BwdParams and the kernel head dim, or an error code.  The order of the checks is part of the
// C-ABI's behaviour (tests/test_abi_golden.py pins which code a call with two defects gets).
int bias_esize(int kind) { return kind == FA2_BIAS_F32 ? 4 : kind == FA2_BIAS_IO_DTYPE ? 2 : 1; }

// (a launch needs the bias and its strides; a plan / size query describes neither: its strides read as 0)
int check_bias(const Call& c) {
    const BiasArg& b = c.bias;
    if (b.kind == FA2_BIAS_NONE) return FA2_OK;
    if (b.kind != FA2_BIAS_IO_DTYPE && b.kind != FA2_BIAS_F32 && b.kind != FA2_BIAS_BOOL) return FA2_ERR_BIAS;
    if (c.ask == Ask::Launch && (!b.ptr || !b.strides)) return FA2_ERR_NULL_POINTER;
    if (b.strides && (b.strides[0] < 0 || b.strides[1] < 0 || b.strides[2] < 0)) return FA2_ERR_BIAS;
    if (reinterpret_cast<uintptr_t>(b.ptr) % (uintptr_t)bias_esize(b.kind)) return FA2_ERR_ALIGNMENT;
    return FA2_OK;
}

// How the forward fetches the bias (FwdParams::bias_vec; fa2_fwd_bias_form reports it): 0 one guarded load per score, 1 ... 4 below.
int bias_load_form(int bias_kind, uintptr_t at, const int64_t* bs, int B, int H, int Nq, int Nkv, int HD) {
    // 1: groups of four consecutive kv can be fetched with one aligned load
    const uintptr_t esize = bias_esize(bias_kind);
    int form = Nkv % 4 == 0 && at % (4 * esize) == 0 && bs[0] % 4 == 0 && bs[1] % 4 == 0 && bs[2] % 4 == 0;
    // 2: a per-row bias whose geometry allows whole 16-byte granules: coalesced tile loads through LDS (a row-broadcast bias —
    // bs[2] == 0, e.g. a key-padding mask — is one cache line for the whole wave already)
    const int64_t gran = 16 / (int64_t)esize;
    if (form && HD <= 256 && Nkv % gran == 0 && at % 16 == 0 && bs[0] % gran == 0 && bs[1] % gran == 0 && bs[2] % gran == 0 && bs[2] != 0)
        form = 2;
    // 3: the same geometry on a grid of more than 3/8 of the CUs' worth of 256-row workgroups, head dims <= 128, one (b, h) slice of the bias within
    // 32-bit byte offsets: the 8-wave shape with the tile staged by LDS-DMA (no bias registers).  Measured (tools/mask_bench.py): dense fp16 bias
    // shared by the heads, B2 H10 N4096 D64, 445 us as 4-wave workgroups; torch SDPA 339.
    if (form == 2 && HD <= 128 && forced_rows() != 128 && (int64_t)B * H * ((Nq + 255) / 256) > fa2::device_cus() * 3 / 8 &&
        ((int64_t)(Nq - 1) * bs[2] + Nkv + 64 * bs[2]) * (int64_t)esize < 0x7fffffffLL)
        form = 3;
    // 4: a bias broadcast over the Q rows (row stride 0 — the [B, 1, 1, Nkv] key-padding mask of padded token batches and of SD cross-attention),
    // any alignment: a wave fetches the tile's 64 values once and spreads them through its LDS image (head dims <= 256: the image exists)
    if (bs[2] == 0 && HD <= 256) form = 4;
    return form;
}

// dtype, sizes, head grouping, head dim, scale — in this order, forward and backward alike.  *HD: the kernel head dim; columns [D, HD) are masked in-kernel.
static_assert(kHeadDims[kNumHeadDims - 1] == kMaxBwdHeadDim, "the backward serves every head dim of the forward");
int check_shape(const Call& c, int* HD) {
    if (c.dtype != FA2_DTYPE_F16 && c.dtype != FA2_DTYPE_BF16) return FA2_ERR_DTYPE;
    if (c.B < 1 || c.H < 1 || c.Nq < 1 || c.Nkv < 1 || c.D < 1) return FA2_ERR_BAD_SHAPE;
    if (c.Hkv < 1 || c.Hkv > c.H || c.H % c.Hkv != 0 || (c.Hkv != c.H && c.bias.kind != FA2_BIAS_NONE)) return FA2_ERR_BAD_SHAPE;
    *HD = fa2_padded_head_dim(c.D);
    if (*HD < 0 || (c.D & 7)) return FA2_ERR_HEAD_DIM;
    if (!std::isfinite(c.scale)) return FA2_ERR_SCALE;
    return FA2_OK;
}

// The tensors of a call: a null pointer (stride arrays included), then alignment.  Dense launches make the first check before everything but the flags
// and the second beside the stride checks; packed launches make both last, so that a bad argument is reported as what it is; plan and size
// queries have no tensors.
bool any_null(std::initializer_list<const void*> ptrs) { return std::any_of(ptrs.begin(), ptrs.end(), [](const void* p) { return !p; }); }
bool all_aligned16(std::initializer_list<const void*> ptrs) { return std::all_of(ptrs.begin(), ptrs.end(), aligned16); }
bool tensors_null(const FwdCall& c) { return any_null({c.q, c.k, c.v, c.o, c.lse, c.qs, c.ks, c.vs, c.os, c.ls}); }
bool tensors_null(const BwdCall& c) {
    return any_null({c.q, c.k, c.v, c.o, c.dout, c.lse, c.dq, c.dk, c.dv, c.delta_ws, c.qs, c.ks, c.vs, c.os, c.dos, c.dqs, c.dks, c.dvs, c.ls});
}
bool tensors_aligned(const FwdCall& c) { return all_aligned16({c.q, c.k, c.v, c.o}); }
bool tensors_aligned(const BwdCall& c) { return all_aligned16({c.q, c.k, c.v, c.o, c.dout, c.dq, c.dk, c.dv}); }
template <typename C>
int check_packed_tensors(const C& c) {
    if (!c.cu_q || !c.cu_k || tensors_null(c)) return FA2_ERR_NULL_POINTER;
    return tensors_aligned(c) ? FA2_OK : FA2_ERR_ALIGNMENT;
}

// what the windowed / packed / dropout kernels read from fields of the parameter block that such a call does not use otherwise
template <typename P>
void set_family(P& p, const Call& c) {
    fa2::set_window(p, c.window);
    if (c.packed) fa2::set_varlen(p, c.cu_q, c.cu_k);
    if (c.dropout) fa2::set_dropout(p, c.seed, c.drop_t);
}

// fa2_fwd_varlen_dv serves D in 136 .. 256 with Dv in 8 .. 128, multiples of 8: one column slab of the kernel of head dim 256 (varlen_dv_hip.cpp)
bool dv_pair_ok(int D, int Dv) { return D % 8 == 0 && D >= 136 && D <= 256 && Dv % 8 == 0 && Dv >= 8 && Dv <= 128; }
// ... in 256-row workgroups, one per CU (96 KiB of LDS), unless that grid covers at most half of the CUs: 128-row workgroups then double the busy CUs.
// Measured (tools/mla_prefill_bench.py, profiles/r51_mla_prefill_bench.txt, bf16 192 / 128): 128 workgroups of 256 rows (H16, 2 048 new tokens on 8 192
// context keys, both passes and the merge) 349.7 -> 291.6 us; everywhere above, 128-row workgroups are 1.34 .. 1.61x SLOWER (B4 H16 x 4 096: 453 -> 606 us),
// so the family's 3/8 rule (pick_rows) gives way to this one.  Option "rows" overrides it.
int dv_rows(const fa2::FwdParams& p) {
    const int f = forced_rows();
    if (f == 128 || f == 256) return f;
    return (int64_t)p.nbh * ((p.Nq + 255) / 256) <= fa2::device_cus() / 2 ? 128 : 256;
}

int fwd_validate(const FwdCall& c, fa2::FwdParams& p, int& HD) {
    // Until round 5 any non-zero value of the flag word meant "causal"; a caller that still passes another truthy int would silently get a non-causal
    // forward: refuse it
    if (c.flags & ~(FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE)) return FA2_ERR_BAD_SHAPE;
    const bool tensors = c.ask == Ask::Launch && !c.packed;
    if (tensors && tensors_null(c)) return FA2_ERR_NULL_POINTER;
    if (int rc = check_bias(c)) return rc;
    int shape_rc = check_shape(c, &HD);
    // (fa2_fwd_varlen_dv: the served (D, Dv) pairs are a head-dim matter, so they are looked at where the head dim is: ahead of the scale)
    if (c.Dv && (shape_rc == FA2_OK || shape_rc == FA2_ERR_SCALE) && !dv_pair_ok(c.D, c.Dv)) shape_rc = FA2_ERR_HEAD_DIM;
    if (shape_rc) return shape_rc;
    const int Dv = c.Dv ? c.Dv : c.D;        // columns of V
    if ((tensors && !tensors_aligned(c)) || !strides_ok(c.qs) || !strides_ok(c.ks) || !strides_ok(c.vs) || !strides_ok(c.os)) return FA2_ERR_ALIGNMENT;
    if (!span_ok(c.Nkv, c.ks, c.D) || !span_ok(c.Nkv, c.vs, Dv)) return FA2_ERR_BAD_SHAPE;

    const int B = c.B, H = c.H, Nq = c.Nq, Nkv = c.Nkv, bias_kind = c.bias.kind;
    p.q = c.q; p.k = c.k; p.v = c.v; p.o = c.o; p.lse = c.lse;
    p.B = B; p.H = H; p.Nq = Nq; p.Nkv = Nkv; p.D = c.D;
    for (int i = 0; i < 3; ++i) {
        p.qs[i] = c.qs[i]; p.ks[i] = c.ks[i]; p.vs[i] = c.vs[i]; p.os[i] = c.os[i];
    }
    p.ls[0] = c.ls[0]; p.ls[1] = c.ls[1];
    p.c = std::fabs(c.scale) * 1.4426950408889634f;  // fold log2(e): reference kernel_fp16.cu:827
    // scale == 0 is the uniform softmax (O = mean of V, as the reference's arithmetic gives).  With c == 0 the first
    // tile's (max - (-inf)) * c would be NaN; a factor too small to move any f32 score off zero gives the same result.
    if (p.c < 1e-30f) p.c = 1e-30f;
    p.negate_q = c.scale < 0.f;
    p.nqblk = (Nq + kFwdRows - 1) / kFwdRows;
    p.bh0 = 0;
    p.nbh = B * H;
    p.rows_hint = 0;
    p.exact_scale = (c.flags & FA2_FLAG_EXACT_SCALE) ? 1 : 0;      // this call scales the f32 product whatever option "fold" says
    p.persist = 1;
    p.full_items = p.split_items = p.nsplit = p.blk0 = p.item_cap = 0;
    p.ws = nullptr;
    p.k_bytes = (uint32_t)span_bytes(Nkv, c.ks, c.D);
    p.v_bytes = (uint32_t)span_bytes(Nkv, c.vs, Dv);
    p.kv_group = H / c.Hkv;
    p.bias = c.bias.ptr;
    p.bias_kind = bias_kind;
    for (int i = 0; i < 3; ++i) p.bs[i] = bias_kind != FA2_BIAS_NONE && c.bias.strides ? c.bias.strides[i] : 0;
    p.bias_vec = bias_kind != FA2_BIAS_NONE ? bias_load_form(bias_kind, reinterpret_cast<uintptr_t>(p.bias), p.bs, B, H, Nq, Nkv, HD) : 0;
    if ((int64_t)B * H * p.nqblk > 0x7fffffffLL) return FA2_ERR_GRID;
    // (the windowed and the BIAS kernels may run as 128-row workgroups)
    if ((c.windowed || bias_kind != FA2_BIAS_NONE) && (int64_t)B * H * ((Nq + 127) / 128) > 0x7fffffffLL) return FA2_ERR_GRID;
    if (c.windowed) set_family(p, c);
    return FA2_OK;
}

// ---- the windowed, packed and dropout kernel families share one launcher signature per direction: [packed][dropout]
using FwdFamilyLaunch = int (*)(bool bf16, int HD, const fa2::FwdParams& p, int rows, hipStream_t stream);
using BwdFamilyLaunch = int (*)(bool bf16, int HD, const fa2::BwdParams& p, hipStream_t stream);
constexpr FwdFamilyLaunch kFwdFamily[2][2] = {{fa2::launch_fwd_window, fa2::launch_fwd_dropout}, {fa2::launch_fwd_varlen, fa2::launch_fwd_varlen_dropout}};
constexpr BwdFamilyLaunch kBwdFamily[2][2] = {{fa2::launch_bwd_window, fa2::launch_bwd_dropout}, {fa2::launch_bwd_varlen, fa2::launch_bwd_varlen_dropout}};

// ... and the score-modifier forms of the windowed / packed kernels, which take the ScoreMod block as well: [packed]
using FwdSmodLaunch = int (*)(bool bf16, int HD, const fa2::FwdParams& p, int rows, hipStream_t stream, const fa2::ScoreMod& sm);
using BwdSmodLaunch = int (*)(bool bf16, int HD, const fa2::BwdParams& p, hipStream_t stream, const fa2::ScoreMod& sm);
constexpr FwdSmodLaunch kFwdSmod[2] = {fa2::launch_fwd_scoremod, fa2::launch_fwd_varlen_scoremod};
constexpr BwdSmodLaunch kBwdSmod[2] = {fa2::launch_bwd_scoremod, fa2::launch_bwd_varlen_scoremod};
fa2::ScoreMod scoremod_of(const Call& c) { return fa2::make_scoremod(c.softcap, c.scale, c.slopes, c.slope_stride); }

// fa2_fwd_workspace_bytes.  The size query has no scale argument, and the split plan depends on the scale at head dim 64 (a launch that folds the
// scale — c <= 1 — runs the parts inside the hand-scheduled kernel: other fixed costs, possibly another S): the answer is the larger of the two plans,
// so a workspace of this size serves the call whatever its scale (the callers' caches are keyed without the scale).
// Likewise FA2_FLAG_EXACT_SCALE (the forward of a call that will be differentiated never folds: another kernel, other fixed costs, possibly
// another S): both settings are planned, whatever the query's flag says — the callers' caches are keyed without it too.
size_t fwd_workspace_need(const fa2::FwdParams& p, int HD, bool bf16, bool causal) {
    size_t need = 0;
    for (const float c_try : {0.5f, 2.0f})
        for (const int exact_try : {0, 1}) {
            fa2::FwdParams pt = p;
            pt.c = c_try;
            pt.exact_scale = exact_try;
            const fa2::SplitPlan pl = plan_split(pt, HD, bf16, causal);
            if (pl.nsplit > 1) need = std::max(need, (size_t)fa2::split_ws_bytes(pl.split_items, pl.nsplit, HD));
        }
    return need;
}

// fa2_fwd_*_plan: what a launch of this call would run, with a (16-byte aligned) workspace of c.ws_bytes bytes
void fwd_report(const FwdCall& c, const fa2::FwdParams& p, int HD, int family_rows, fa2_fwd_plan_t* out) {
    std::memset(out, 0, sizeof(*out));
    out->heads_main = c.B * c.H;
    if (c.windowed) {
        out->kernel = c.Dv ? FA2_KERNEL_HIP_VARLEN_DV : c.packed ? FA2_KERNEL_HIP_VARLEN : FA2_KERNEL_HIP_WINDOW;
        out->rows = family_rows;
    } else if (c.bias.kind != FA2_BIAS_NONE) {
        out->kernel = FA2_KERNEL_HIP_BIAS;
        out->rows = 0;       // unspecified: the load form (and with it 128- or 256-row workgroups) depends on the bias strides and alignment, which the query does not take
    } else {
        const FwdPlan f = plan_fwd(HD, c.dtype == FA2_DTYPE_BF16, p, (c.flags & FA2_FLAG_CAUSAL) != 0, c.ws_bytes > 0, c.ws_bytes);
        out->kernel = f.main.kernel; out->contract = f.main.contract; out->rows = f.main.rows;
        out->heads_main = f.main_heads;
        out->kernel_tail = f.tail.kernel; out->contract_tail = f.tail.contract; out->rows_tail = f.tail.rows;
        out->nsplit = f.split.nsplit > 1 ? f.split.nsplit : 0;
        out->split_items = f.split.nsplit > 1 ? f.split.split_items : 0;
    }
}

// The forward call: validate, then answer the query or launch.
int fwd_run(const FwdCall& c) {
    fa2::FwdParams p;
    int HD = 0;
    if (int rc = fwd_validate(c, p, HD)) return rc;
    const bool bf16 = c.dtype == FA2_DTYPE_BF16, causal = (c.flags & FA2_FLAG_CAUSAL) != 0;
    // rows per workgroup of the windowed / packed kernels (packed: the grid of the stated maximum lengths)
    const int family_rows = !c.windowed ? 0 : c.Dv ? dv_rows(p) : HD > 256 ? 128 : pick_rows(p);
    if (c.ask == Ask::Size) { *c.ws_need = fwd_workspace_need(p, HD, bf16, causal); return FA2_OK; }
    if (c.ask == Ask::Plan) { fwd_report(c, p, HD, family_rows, c.plan); return FA2_OK; }
    if (c.packed)
        if (int rc = check_packed_tensors(c)) return rc;
    hipStream_t stream = (hipStream_t)c.stream;
    if (c.Dv) return fa2::launch_fwd_varlen_dv(bf16, p, c.Dv, family_rows, stream);      // (a packed call without dropout or score modifiers: its entry point sets nothing else)
    if (c.scoremod) return kFwdSmod[c.packed](bf16, HD, p, family_rows, stream, scoremod_of(c));
    if (c.windowed) return kFwdFamily[c.packed][c.dropout](bf16, HD, p, family_rows, stream);
    if (c.bias.kind != FA2_BIAS_NONE) return fa2::launch_fwd_hip(bf16, HD, p, causal, 128, true, stream);
    return launch_fwd(HD, bf16, p, causal, stream, c.ws, c.ws_bytes);
}

int bwd_validate(const BwdCall& c, fa2::BwdParams& p, int& HD) {
    if (c.flags & ~(FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE)) return FA2_ERR_BAD_SHAPE;      // (as in fwd_validate: no value but the documented flag bits;
    if (int rc = check_bias(c)) return rc;                                                    //  bit 1 is what the backward does anyway unless option "kfold" is set)
    const bool tensors = c.ask == Ask::Launch && !c.packed;
    if (tensors && tensors_null(c)) return FA2_ERR_NULL_POINTER;
    if (int rc = check_shape(c, &HD)) return rc;
    if (tensors && !tensors_aligned(c)) return FA2_ERR_ALIGNMENT;
    for (const int64_t* s : {c.qs, c.ks, c.vs, c.os, c.dos, c.dqs, c.dks, c.dvs})
        if (!strides_ok(s)) return FA2_ERR_ALIGNMENT;
    const int B = c.B, H = c.H, Nq = c.Nq, Nkv = c.Nkv, D = c.D, bias_kind = c.bias.kind;
    if (!span_ok(Nq, c.qs, D) || !span_ok(Nq, c.dos, D) || !span_ok(Nkv, c.ks, D) || !span_ok(Nkv, c.vs, D)) return FA2_ERR_BAD_SHAPE;
    const int64_t blocks = (int64_t)B * H * (((Nq > Nkv ? Nq : Nkv) + fa2::kQBlock - 1) / fa2::kQBlock);
    if (blocks > 0x7fffffffLL || (int64_t)B * H * Nq / 16 > 0x7fffffffLL) return FA2_ERR_GRID;

    p.q = c.q; p.k = c.k; p.v = c.v; p.o = c.o; p.dout = c.dout; p.lse = c.lse; p.delta = c.delta_ws; p.dq = c.dq; p.dk = c.dk; p.dv = c.dv;
    p.B = B; p.H = H; p.Nq = Nq; p.Nkv = Nkv; p.D = D;
    for (int i = 0; i < 3; ++i) {
        p.qs[i] = c.qs[i]; p.ks[i] = c.ks[i]; p.vs[i] = c.vs[i]; p.os[i] = c.os[i];
        p.dos[i] = c.dos[i]; p.dqs[i] = c.dqs[i]; p.dks[i] = c.dks[i]; p.dvs[i] = c.dvs[i];
    }
    p.ls[0] = c.ls[0]; p.ls[1] = c.ls[1];
    p.scale = c.scale;
    p.c = c.scale * 1.4426950408889634f;
    p.nblk = 0;
    p.q_bytes = (uint32_t)span_bytes(Nq, c.qs, D); p.k_bytes = (uint32_t)span_bytes(Nkv, c.ks, D); p.v_bytes = (uint32_t)span_bytes(Nkv, c.vs, D);
    p.do_bytes = (uint32_t)span_bytes(Nq, c.dos, D); p.l_bytes = (uint32_t)Nq * 4u;
    p.bias = c.bias.ptr;
    p.bias_kind = bias_kind;
    for (int i = 0; i < 3; ++i) p.bs[i] = bias_kind != FA2_BIAS_NONE && c.bias.strides ? c.bias.strides[i] : 0;
    // bias tiles by LDS-DMA (fa2_bwd_kernel.hip.h: bwd_bias_tile_*): a per-row bias whose pointer, strides and Nkv are multiples of 16 bytes, one
    // (b, h) slice within 32-bit byte offsets; otherwise one guarded load per score
    p.bias_tile = 0;
    p.bias_img = 4096;
    if (bias_kind != FA2_BIAS_NONE) {
        const int64_t esize = bias_esize(bias_kind), gran = 16 / esize;
        // the backward addresses one (b, h) slice of the bias with 32-bit byte offsets (bounds-checked buffer loads), like K and V
        if (((int64_t)(Nq - 1) * p.bs[2] + Nkv + 64 * p.bs[2]) * esize >= 0x7fffffffLL) return FA2_ERR_BAD_SHAPE;
        if (bias_kind == FA2_BIAS_F32) p.bias_img = 8192;
        if (Nkv % gran == 0 && reinterpret_cast<uintptr_t>(p.bias) % 16 == 0 && p.bs[0] % gran == 0 && p.bs[1] % gran == 0 && p.bs[2] % gran == 0 &&
            p.bs[2] != 0)
            p.bias_tile = 1;
    }
    p.full_items = p.split_items = p.nsplit = 0;
    p.ws = (float*)c.ws;
    p.ws_bytes = c.ws_bytes;
    p.kv_group = H / c.Hkv;
    if (c.windowed) set_family(p, c);
    p.dlse = c.dlse;
    return FA2_OK;
}

// The dlse arguments of the *_lse entry points, checked after everything else: alignment of the pointer, then the strides.
int check_dlse(const BwdCall& c, fa2::BwdParams& p) {
    if (!c.dlse) return FA2_OK;
    if (reinterpret_cast<uintptr_t>(c.dlse) & 3u) return FA2_ERR_ALIGNMENT;
    if (c.ask == Ask::Launch && !c.dlses) return FA2_ERR_NULL_POINTER;
    if (c.dlses) {
        if (c.dlses[0] < 0 || c.dlses[1] < 0) return FA2_ERR_BAD_SHAPE;
        p.dls[0] = c.dlses[0]; p.dls[1] = c.dlses[1];
    }
    return FA2_OK;
}

// The backward call: validate, then answer the size query (fa2_bwd_*_workspace_bytes) or launch.
int bwd_run(const BwdCall& c) {
    fa2::BwdParams p;
    int HD = 0;
    if (int rc = bwd_validate(c, p, HD)) return rc;
    const bool bf16 = c.dtype == FA2_DTYPE_BF16, causal = (c.flags & FA2_FLAG_CAUSAL) != 0;
    if (c.ask == Ask::Size) {
        fa2::SplitPlan dq, dkv;
        *c.ws_need = (size_t)fa2::plan_bwd_split(HD, p, causal, &dq, &dkv);
        return FA2_OK;
    }
    if (c.ask != Ask::Launch)
        if (int rc = check_dlse(c, p)) return rc;
    if (c.ask == Ask::Plan) {        // fa2_bwd_plan: the dense unmasked call's passes (the masked backward runs the BIAS forms of the compiler-scheduled passes)
        BwdPlan pl = {0, false, false, false};
        if (c.bias.kind == FA2_BIAS_NONE) pl = plan_bwd(HD, bf16, p, causal);
        c.plan->dq_kernel = pl.short_dq ? FA2_BWD_KERNEL_SHORT : (pl.asm_parts & 1) ? FA2_BWD_KERNEL_ASM : FA2_BWD_KERNEL_HIP;
        c.plan->dkv_kernel = (pl.asm_parts & 2) ? FA2_BWD_KERNEL_ASM : FA2_BWD_KERNEL_HIP;
        return FA2_OK;
    }
    if (c.packed)
        if (int rc = check_packed_tensors(c)) return rc;
    if (int rc = check_dlse(c, p)) return rc;
    hipStream_t stream = (hipStream_t)c.stream;
    if (c.scoremod) return kBwdSmod[c.packed](bf16, HD, p, stream, scoremod_of(c));
    if (c.windowed) return kBwdFamily[c.packed][c.dropout](bf16, HD, p, stream);
    if (c.bias.kind != FA2_BIAS_NONE) return fa2::launch_bwd_bias_hip(bf16, HD, p, causal, stream);
    return launch_bwd(HD, bf16, p, causal, stream);
}

// ---- what the entry points of one family share
// The dense windowed and dropout entry points: the flag check, the window reduced for these lengths, and the flags and window the kernels then take —
// a window that masks nothing IS a plain call (kind 0) or today's top-left causal call (kind 1) and runs exactly what fa2_fwd_gqa / fa2_bwd run, unless
// the call drops: the DROP forms of the windowed kernels are the only ones with the mask, and they scale the f32 product.
int dense_window(Call& c, int flags, int left, int right, int q_offset) {
    if (flags & ~(FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE)) return FA2_ERR_BAD_SHAPE;
    const WindowCall w = reduce_window(c.Nq, c.Nkv, left, right, q_offset, (flags & FA2_FLAG_CAUSAL) != 0);
    if (w.kind < 0) return FA2_ERR_BAD_SHAPE;
    c.window = w.w;
    c.windowed = c.dropout || c.scoremod || w.kind == 2;        // (the score-modifier calls likewise: the SMOD forms are the only kernels with the transform)
    c.flags = c.dropout || c.scoremod ? FA2_FLAG_EXACT_SCALE : (flags & FA2_FLAG_EXACT_SCALE) | (w.kind == 1 ? FA2_FLAG_CAUSAL : 0);
    return FA2_OK;
}

void set_dropout_args(Call& c, float dropout_p, uint64_t seed) {       // (after dropout_p_ok)
    c.dropout = true;
    c.seed = seed;
    c.drop_t = fa2::dropout_threshold(dropout_p, nullptr);
}

// The score-modifier entry points' own three arguments, checked ahead of everything else, in this order: softcap (negative, NaN, inf), the stride of
// the slopes (negative), the slope pointer's alignment.  softcap == 0 and no slopes: nothing is set and the call IS the windowed / packed call.
int set_scoremod_args(Call& c, float softcap, const float* slopes, int64_t stride) {
    if (!fa2::softcap_ok(softcap)) return FA2_ERR_SOFTCAP;
    if (stride < 0) return FA2_ERR_BAD_SHAPE;
    if (reinterpret_cast<uintptr_t>(slopes) & 3u) return FA2_ERR_ALIGNMENT;
    c.scoremod = softcap > 0.f || slopes != nullptr;
    c.softcap = softcap; c.slopes = slopes; c.slope_stride = stride;
    return FA2_OK;
}

// The packed entry points (c.B .. c.D by name already): what the host can check of such a call — the contents of cu_seqlens live on the device —, the window
// as the kernels take it (the causal flag folded in, the offset field carrying the bottom-right flag), and the [total, heads, D] strides {head, row} as the
// kernels' {batch, head, row} with a batch stride of 0: the sequence's first row is added in-kernel.  `two`: q, k, v, o (, do, dq, dk, dv).
struct PackedStrides { int64_t s[8][3], ls[2]; };
int packed_call(Call& c, PackedStrides& ps, std::initializer_list<const int64_t*> two, int64_t lse_stride, int flags, int left, int right) {
    if (c.B < 1 || c.H < 1 || c.Hkv < 1 || c.Nq < 1 || c.Nkv < 1 || c.D < 1 || c.Hkv > c.H || c.H % c.Hkv != 0) return FA2_ERR_BAD_SHAPE;
    if (flags & ~(FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE | FA2_FLAG_BOTTOM_RIGHT)) return FA2_ERR_BAD_SHAPE;
    const bool br = (flags & FA2_FLAG_BOTTOM_RIGHT) != 0;
    const int n = c.Nq > c.Nkv ? c.Nq : c.Nkv;          // a sequence's offset Nkv_s - Nq_s lies in [-max_q, max_k]
    if (!fa2::window_args_ok(c.Nq, c.Nkv, left, right, br ? -n : 0, true)) return FA2_ERR_BAD_SHAPE;
    for (const int64_t* t : two)
        if (!t) return FA2_ERR_NULL_POINTER;
    c.window.left = left;
    c.window.right = fa2::window_normalize_right(right, (flags & FA2_FLAG_CAUSAL) != 0);
    c.window.off = br ? 1 : 0;
    c.windowed = c.packed = true;
    c.flags = c.dropout || c.scoremod ? FA2_FLAG_EXACT_SCALE : flags & FA2_FLAG_EXACT_SCALE;
    int i = 0;
    for (const int64_t* t : two) { ps.s[i][0] = 0; ps.s[i][1] = t[0]; ps.s[i][2] = t[1]; ++i; }
    ps.ls[0] = 0; ps.ls[1] = lse_stride;
    return FA2_OK;
}

// Plan and size queries describe no tensors.  Forward: contiguous [B, H, N, D] ones unless the query passes strides (the plan looks at the row pitches of Q
// and K: a contiguous tensor's are what the size query must assume — ADVICE r3: stand-in pitches of 8 elements made the query plan for the
// compiler-scheduled kernels and the launch for the hand-scheduled ones).  V takes K's strides, O takes Q's.
int run_query(FwdCall& c) {
    if (c.B < 1 || c.H < 1 || c.Hkv < 1 || c.Nq < 1 || c.Nkv < 1 || c.D < 1) return FA2_ERR_BAD_SHAPE;
    const int64_t d = c.D;
    const int64_t q[3] = {(int64_t)c.H * c.Nq * d, (int64_t)c.Nq * d, d}, k[3] = {(int64_t)c.Hkv * c.Nkv * d, (int64_t)c.Nkv * d, d};
    const int64_t ls[2] = {(int64_t)c.H * c.Nq, c.Nq};
    if (!c.qs) c.qs = q;
    if (!c.ks) c.ks = k;
    c.vs = c.ks; c.os = c.qs;
    if (!c.ls) c.ls = ls;
    return fwd_run(c);
}
// Backward: the plan depends on the shape, the options and the device's CU count only — any valid strides will do.
int run_query(BwdCall& c) {
    static const int64_t one[3] = {8, 8, 8}, ls[2] = {0, 0};
    c.qs = c.ks = c.vs = c.os = c.dos = c.dqs = c.dks = c.dvs = one;
    c.ls = ls;
    return bwd_run(c);
}
// fa2_*_workspace_bytes: the validation and planning half of the call; 0 for a call that would be refused
template <typename C>
size_t workspace_query(C& c) {
    size_t need = 0;
    c.ask = Ask::Size;
    c.ws_need = &need;
    return run_query(c) == FA2_OK ? need : 0;
}

}  // namespace

extern "C" {

int fa2_supported_head_dims(int* dims, int cap) {
    for (int i = 0; i < kNumHeadDims && i < cap; ++i)
        if (dims) dims[i] = kHeadDims[i];
    return kNumHeadDims;
}

int fa2_padded_head_dim(int D) {
    if (D < 1) return -1;
    for (int i = 0; i < kNumHeadDims; ++i)
        if (D <= kHeadDims[i]) return kHeadDims[i];
    return -1;
}

int fa2_tile_rows(int D, int* q_rows_per_block, int* kv_rows_per_tile) {
    if (fa2_padded_head_dim(D) != D) return FA2_ERR_HEAD_DIM;
    if (q_rows_per_block) *q_rows_per_block = D > 256 ? 128 : kFwdRows;
    if (kv_rows_per_tile) *kv_rows_per_tile = fa2::kKvTile;
    return FA2_OK;
}

int fa2_fwd_prescales_q(int D, float scale) {
    if (fa2_padded_head_dim(D) < 0) return -1;
    // the fp16 launches that take the hand-scheduled bodies MAY fold (plan_range; fa2_fwd_plan says what one call does)
    return (D == 64 || D == 128) && scale > 0.f && scale * 1.4426950408889634f <= 1.0f && fa2::options().fold.load(std::memory_order_relaxed) >= 1 ? 1 : 0;
}

int fa2_set_option(const char* name, int value) {
    if (!name) return FA2_ERR_NULL_POINTER;
    fa2::Options& o = fa2::options();
    if (!std::strcmp(name, "rows")) { if (value != 0 && value != 128 && value != 256) return FA2_ERR_BAD_SHAPE; o.rows = value; }
    else if (!std::strcmp(name, "asm")) o.asm_mask = value;
    else if (!std::strcmp(name, "persist")) o.persist = value != 0;
    else if (!std::strcmp(name, "split")) o.split = value != 0;
    else if (!std::strcmp(name, "fold")) { if (value < 0 || value > 2) return FA2_ERR_BAD_SHAPE; o.fold = value; }
    else if (!std::strcmp(name, "bwd_parts")) { if (value < 1 || value > 3) return FA2_ERR_BAD_SHAPE; o.bwd_parts = value; }
    else if (!std::strcmp(name, "kfold")) o.kfold = value != 0;
    else if (!std::strcmp(name, "short")) o.short_kv = value != 0;
    else return FA2_ERR_BAD_SHAPE;
    o.epoch.fetch_add(1, std::memory_order_relaxed);
    return FA2_OK;
}

int fa2_get_option(const char* name) {
    if (!name) return FA2_ERR_NULL_POINTER;
    fa2::Options& o = fa2::options();
    if (!std::strcmp(name, "rows")) return o.rows.load();
    if (!std::strcmp(name, "asm")) return o.asm_mask.load();
    if (!std::strcmp(name, "persist")) return o.persist.load();
    if (!std::strcmp(name, "split")) return o.split.load();
    if (!std::strcmp(name, "fold")) return o.fold.load();
    if (!std::strcmp(name, "epoch")) return o.epoch.load() & 0x3fffffff;
    if (!std::strcmp(name, "bwd_parts")) return o.bwd_parts.load();
    if (!std::strcmp(name, "kfold")) return o.kfold.load();
    if (!std::strcmp(name, "short")) return o.short_kv.load();
    return FA2_ERR_BAD_SHAPE;
}

const char* fa2_error_string(int code) {
    switch (code) {
        case FA2_OK: return "ok";
        case FA2_ERR_NULL_POINTER: return "fa2: null pointer argument";
        case FA2_ERR_BAD_SHAPE: return "fa2: B, H, Nq, Nkv, D must be >= 1; one head's K / V (backward: also Q / dO; backward bias: one slice) must span < 2 GiB with 64 rows of slack; window_left / window_right are -1 or >= 0, q_offset >= 0";
        case FA2_ERR_HEAD_DIM: return "fa2: head dim not supported (pad D to fa2_padded_head_dim(D))";
        case FA2_ERR_ALIGNMENT: return "fa2: pointers must be 16-byte aligned, strides multiples of 8 elements, last dim contiguous";
        case FA2_ERR_DTYPE: return "fa2: dtype must be FA2_DTYPE_F16 or FA2_DTYPE_BF16";
        case FA2_ERR_SCALE: return "fa2: scale must be finite";
        case FA2_ERR_GRID: return "fa2: B*H*ceil(Nq/256) exceeds the grid limit";
        case FA2_ERR_BIAS: return "fa2: bias_kind must be FA2_BIAS_{NONE,IO_DTYPE,F32,BOOL} and bias strides >= 0";
        case FA2_ERR_DROPOUT: return "fa2: dropout_p must be in [0, 1)";
        case FA2_ERR_SOFTCAP: return "fa2: softcap must be 0 (off) or a finite positive number (a normal float: >= 1.18e-38)";
        default: break;
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "fa2: unknown error code";
}

const char* fa2_version(void) { return "fa2_gfx950 0.9 (D=128 forward (sum-check fast bodies) + backward and D=64 forward: hand-scheduled 4-wave asm bodies, head dims 136 to 256 forward too; short KV sweeps and the other head dims up to 512: HIP kernels; lds-dma; KV-split tail rounds; attention bias / mask, forward + backward; KV-cache decode and append)"; }

// The parameters every dense forward / backward entry point takes, after `dtype` and up to the flag word (HKV: FA2_HKV where the entry point has an Hkv;
// include/fa2_gfx950.h spells every list out), the same as arguments, and a call description filled from them by field name (the MHA entry points' Hkv is H).
#define FA2_HKV int Hkv,
#define FA2_FWD_ARGS(HKV)                                                                                                            \
    const void *q, const void *k, const void *v, void *o, float *lse, int B, int H, HKV int Nq, int Nkv, int D, const int64_t q_strides[3], \
        const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3], const int64_t lse_strides[2], float scale, int flags
#define FA2_FWD_PASS q, k, v, o, lse, B, H, Nq, Nkv, D, q_strides, k_strides, v_strides, o_strides, lse_strides, scale, flags
#define FA2_FWD_CALL(c)                                                                                                 \
    FwdCall c;                                                                                                          \
    c.dtype = dtype; c.q = q; c.k = k; c.v = v; c.o = o; c.lse = lse; c.B = B; c.H = c.Hkv = H; c.Nq = Nq; c.Nkv = Nkv; c.D = D; \
    c.qs = q_strides; c.ks = k_strides; c.vs = v_strides; c.os = o_strides; c.ls = lse_strides; c.scale = scale; c.flags = flags; c.stream = hip_stream
#define FA2_BWD_ARGS(HKV)                                                                                               \
    const void *q, const void *k, const void *v, const void *o, const void *dout, const float *lse, void *dq, void *dk, \
        void *dv, float *delta_ws, int B, int H, HKV int Nq, int Nkv, int D, const int64_t q_strides[3],                \
        const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],                             \
        const int64_t do_strides[3], const int64_t dq_strides[3], const int64_t dk_strides[3],                          \
        const int64_t dv_strides[3], const int64_t lse_strides[2], float scale, int flags
#define FA2_BWD_PASS                                                                                                    \
    q, k, v, o, dout, lse, dq, dk, dv, delta_ws, B, H, Nq, Nkv, D, q_strides, k_strides, v_strides, o_strides,          \
        do_strides, dq_strides, dk_strides, dv_strides, lse_strides, scale, flags
#define FA2_BWD_CALL(c)                                                                                                 \
    BwdCall c;                                                                                                          \
    c.dtype = dtype; c.q = q; c.k = k; c.v = v; c.o = o; c.dout = dout; c.lse = lse; c.dq = dq; c.dk = dk; c.dv = dv; c.delta_ws = delta_ws; \
    c.B = B; c.H = c.Hkv = H; c.Nq = Nq; c.Nkv = Nkv; c.D = D; c.qs = q_strides; c.ks = k_strides; c.vs = v_strides; c.os = o_strides;         \
    c.dos = do_strides; c.dqs = dq_strides; c.dks = dk_strides; c.dvs = dv_strides; c.ls = lse_strides;                \
    c.scale = scale; c.flags = flags; c.stream = hip_stream
// ... and every query: the shape (fa2_fwd_plan and the MHA size queries: Hkv = H)
#define FA2_QUERY_CALL(Type, c, Hkv_) \
    Type c;                           \
    c.dtype = dtype; c.B = B; c.H = H; c.Hkv = Hkv_; c.Nq = Nq; c.Nkv = Nkv; c.D = D; c.flags = flags

int fa2_fwd(int dtype, FA2_FWD_ARGS(), void* hip_stream) {
    FA2_FWD_CALL(c);
    return fwd_run(c);
}

int fa2_fwd_ws(int dtype, FA2_FWD_ARGS(), void* workspace, size_t workspace_bytes, void* hip_stream) {
    FA2_FWD_CALL(c);
    c.ws = workspace; c.ws_bytes = workspace_bytes;
    return fwd_run(c);
}

size_t fa2_fwd_workspace_bytes(int dtype, int B, int H, int Nq, int Nkv, int D, int flags) {
    FA2_QUERY_CALL(FwdCall, c, H);
    c.scale = (float)(1.0 / std::sqrt((double)D));
    return workspace_query(c);
}

int fa2_fwd_plan(int dtype, int B, int H, int Nq, int Nkv, int D, const int64_t q_strides[3], const int64_t k_strides[3],
                 float scale, int flags, int bias_kind, size_t workspace_bytes, fa2_fwd_plan_t* plan) {
    if (!plan) return FA2_ERR_NULL_POINTER;
    FA2_QUERY_CALL(FwdCall, c, H);
    c.qs = q_strides; c.ks = k_strides; c.scale = scale; c.bias.kind = bias_kind; c.ws_bytes = workspace_bytes;
    c.ask = Ask::Plan; c.plan = plan;
    return run_query(c);
}

int fa2_fwd_bias(int dtype, FA2_FWD_ARGS(), const void* bias, int bias_kind, const int64_t bias_strides[3], void* hip_stream) {
    FA2_FWD_CALL(c);
    c.bias.ptr = bias; c.bias.kind = bias_kind; c.bias.strides = bias_strides;
    return fwd_run(c);
}

int fa2_bwd(int dtype, FA2_BWD_ARGS(), void* hip_stream) {
    FA2_BWD_CALL(c);
    return bwd_run(c);
}

int fa2_bwd_ws(int dtype, FA2_BWD_ARGS(), void* workspace, size_t workspace_bytes, void* hip_stream) {
    FA2_BWD_CALL(c);
    c.ws = workspace; c.ws_bytes = workspace_bytes;
    return bwd_run(c);
}

size_t fa2_bwd_workspace_bytes(int dtype, int B, int H, int Nq, int Nkv, int D, int flags) {
    FA2_QUERY_CALL(BwdCall, c, H);
    c.scale = 1.0f;
    return workspace_query(c);
}

int fa2_bwd_bias_ws(int dtype, FA2_BWD_ARGS(), const void* bias, int bias_kind, const int64_t bias_strides[3], void* workspace, size_t workspace_bytes,
                    void* hip_stream) {
    FA2_BWD_CALL(c);
    c.bias.ptr = bias; c.bias.kind = bias_kind; c.bias.strides = bias_strides;
    c.ws = workspace; c.ws_bytes = workspace_bytes;
    return bwd_run(c);
}

size_t fa2_bwd_bias_workspace_bytes(int dtype, int B, int H, int Nq, int Nkv, int D, int flags) {
    FA2_QUERY_CALL(BwdCall, c, H);
    c.scale = 1.0f;
    c.bias.kind = FA2_BIAS_BOOL;       // (the plan does not depend on the bias' kind or strides: any valid kind will do)
    return workspace_query(c);
}

int fa2_bwd_bias(int dtype, FA2_BWD_ARGS(), const void* bias, int bias_kind, const int64_t bias_strides[3], void* hip_stream) {
    FA2_BWD_CALL(c);
    c.bias.ptr = bias; c.bias.kind = bias_kind; c.bias.strides = bias_strides;
    return bwd_run(c);
}

// ---- grouped-query / multi-query attention: K and V (and dK, dV) have Hkv heads, Q head h reads K / V head h / (H / Hkv)
int fa2_fwd_gqa(int dtype, FA2_FWD_ARGS(FA2_HKV), void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (Hkv < 1) return FA2_ERR_BAD_SHAPE;
    FA2_FWD_CALL(c);
    c.Hkv = Hkv; c.ws = workspace; c.ws_bytes = workspace_bytes;
    return fwd_run(c);
}

size_t fa2_fwd_gqa_workspace_bytes(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D, int flags) {
    // the forward's plan does not depend on the K / V head count (the grouped call runs the MHA call's kernels): fa2_fwd_workspace_bytes, validated
    if (B < 1 || H < 1 || Hkv < 1 || Hkv > H || H % Hkv != 0) return 0;
    return fa2_fwd_workspace_bytes(dtype, B, H, Nq, Nkv, D, flags);
}

int fa2_fwd_gqa_plan(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D, const int64_t q_strides[3], const int64_t k_strides[3],
                     float scale, int flags, size_t workspace_bytes, fa2_fwd_plan_t* plan) {
    if (!plan) return FA2_ERR_NULL_POINTER;
    FA2_QUERY_CALL(FwdCall, c, Hkv);
    c.qs = q_strides; c.ks = k_strides; c.scale = scale; c.ws_bytes = workspace_bytes;
    c.ask = Ask::Plan; c.plan = plan;
    return run_query(c);
}

int fa2_bwd_gqa(int dtype, FA2_BWD_ARGS(FA2_HKV), void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (Hkv < 1) return FA2_ERR_BAD_SHAPE;
    FA2_BWD_CALL(c);
    c.Hkv = Hkv; c.ws = workspace; c.ws_bytes = workspace_bytes;
    return bwd_run(c);
}

int fa2_bwd_plan(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D, const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                 const int64_t o_strides[3], const int64_t do_strides[3], float scale, int flags, int bias_kind, const int64_t bias_strides[3],
                 fa2_bwd_plan_t* plan) {
    if (!plan) return FA2_ERR_NULL_POINTER;
    if (B < 1 || H < 1 || Hkv < 1 || Nq < 1 || Nkv < 1 || D < 1) return FA2_ERR_BAD_SHAPE;
    // a stride array the query does not pass describes a contiguous [B, heads, N, D] tensor; dQ / dK / dV (64-bit stores in every pass) take Q's / K's / V's
    const int64_t d = D, q[3] = {(int64_t)H * Nq * d, (int64_t)Nq * d, d}, k[3] = {(int64_t)Hkv * Nkv * d, (int64_t)Nkv * d, d};
    static const int64_t ls[2] = {0, 0};
    FA2_QUERY_CALL(BwdCall, c, Hkv);
    c.scale = scale; c.bias.kind = bias_kind; c.bias.strides = bias_strides;
    c.qs = c.dqs = q_strides ? q_strides : q; c.ks = c.dks = k_strides ? k_strides : k; c.vs = c.dvs = v_strides ? v_strides : k;
    c.os = o_strides ? o_strides : q; c.dos = do_strides ? do_strides : q; c.ls = ls;
    c.ask = Ask::Plan; c.plan = plan;
    return bwd_run(c);
}

int fa2_fwd_bias_form(int bias_kind, int B, int H, int Nq, int Nkv, int D, const int64_t bias_strides[3]) {
    if (!bias_strides) return FA2_ERR_NULL_POINTER;
    if (bias_kind != FA2_BIAS_IO_DTYPE && bias_kind != FA2_BIAS_F32 && bias_kind != FA2_BIAS_BOOL) return FA2_ERR_BIAS;
    if (bias_strides[0] < 0 || bias_strides[1] < 0 || bias_strides[2] < 0) return FA2_ERR_BIAS;
    if (B < 1 || H < 1 || Nq < 1 || Nkv < 1 || D < 1) return FA2_ERR_BAD_SHAPE;
    const int HD = fa2_padded_head_dim(D);
    if (HD < 0 || (D & 7)) return FA2_ERR_HEAD_DIM;
    return bias_load_form(bias_kind, 0, bias_strides, B, H, Nq, Nkv, HD);
}

size_t fa2_bwd_gqa_workspace_bytes(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D, int flags) {
    FA2_QUERY_CALL(BwdCall, c, Hkv);
    c.scale = 1.0f;
    return workspace_query(c);
}

// ---- sliding-window attention: include/fa2_gfx950.h has the contract, fa2_window.h the arithmetic, window_hip.cpp the kernels
int fa2_fwd_window(int dtype, FA2_FWD_ARGS(FA2_HKV), int window_left, int window_right, int q_offset, void* hip_stream) {
    if (Hkv < 1) return FA2_ERR_BAD_SHAPE;
    FA2_FWD_CALL(c);
    c.Hkv = Hkv;
    if (int rc = dense_window(c, flags, window_left, window_right, q_offset)) return rc;
    return fwd_run(c);
}

int fa2_fwd_window_plan(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D, const int64_t q_strides[3], const int64_t k_strides[3],
                        float scale, int flags, int window_left, int window_right, int q_offset, size_t workspace_bytes, fa2_fwd_plan_t* plan) {
    if (!plan) return FA2_ERR_NULL_POINTER;
    FA2_QUERY_CALL(FwdCall, c, Hkv);
    c.qs = q_strides; c.ks = k_strides; c.scale = scale; c.ws_bytes = workspace_bytes;
    c.ask = Ask::Plan; c.plan = plan;
    if (int rc = dense_window(c, flags, window_left, window_right, q_offset)) return rc;
    return run_query(c);
}

int fa2_bwd_window(int dtype, FA2_BWD_ARGS(), int window_left, int window_right, int q_offset, void* hip_stream) {
    FA2_BWD_CALL(c);
    if (int rc = dense_window(c, flags, window_left, window_right, q_offset)) return rc;
    return bwd_run(c);
}

int fa2_window_tile_range(int Nq, int Nkv, int window_left, int window_right, int q_offset, int causal, int row0, int rows, int tile,
                          int* first_tile, int* ntiles) {
    if (!first_tile || !ntiles) return FA2_ERR_NULL_POINTER;
    if (Nq < 1 || Nkv < 1 || row0 < 0 || rows < 1 || tile < 1 || rows > (1 << 24) || row0 > 0x7fffffff - (1 << 24) ||
        !fa2::window_args_ok(Nq, Nkv, window_left, window_right, q_offset))
        return FA2_ERR_BAD_SHAPE;
    fa2::window_tile_range(Nq, Nkv, window_left, fa2::window_normalize_right(window_right, causal), q_offset, row0, rows, tile, first_tile, ntiles);
    return FA2_OK;
}

int fa2_window_row_range(int Nq, int Nkv, int window_left, int window_right, int q_offset, int causal, int key0, int keys, int tile,
                         int* first_tile, int* ntiles) {
    if (!first_tile || !ntiles) return FA2_ERR_NULL_POINTER;
    if (Nq < 1 || Nkv < 1 || key0 < 0 || keys < 1 || tile < 1 || keys > (1 << 24) || key0 > 0x7fffffff - (1 << 24) ||
        !fa2::window_args_ok(Nq, Nkv, window_left, window_right, q_offset))
        return FA2_ERR_BAD_SHAPE;
    fa2::window_row_range(Nq, Nkv, window_left, fa2::window_normalize_right(window_right, causal), q_offset, key0, keys, tile, first_tile, ntiles);
    return FA2_OK;
}

// ---- packed, variable-length attention: include/fa2_gfx950.h has the contract, varlen_hip.cpp the kernels
// The parameters the packed entry points take under these names (the strides go through packed_call)
#define FA2_PACKED_FILL(c, Hkv_)                                                                                        \
    c.dtype = dtype; c.B = B; c.H = H; c.Hkv = Hkv_; c.Nq = max_seqlen_q; c.Nkv = max_seqlen_k; c.D = D; c.scale = scale
#define FA2_PACKED_FWD_FILL(c, ps)                                                                                      \
    c.q = q; c.k = k; c.v = v; c.o = o; c.lse = lse; c.cu_q = cu_seqlens_q; c.cu_k = cu_seqlens_k;                     \
    c.qs = ps.s[0]; c.ks = ps.s[1]; c.vs = ps.s[2]; c.os = ps.s[3]; c.ls = ps.ls; c.stream = hip_stream
#define FA2_PACKED_BWD_FILL(c, ps)                                                                                      \
    c.q = q; c.k = k; c.v = v; c.o = o; c.dout = dout; c.lse = lse; c.dq = dq; c.dk = dk; c.dv = dv; c.delta_ws = delta_ws; \
    c.cu_q = cu_seqlens_q; c.cu_k = cu_seqlens_k; c.qs = ps.s[0]; c.ks = ps.s[1]; c.vs = ps.s[2]; c.os = ps.s[3];      \
    c.dos = ps.s[4]; c.dqs = ps.s[5]; c.dks = ps.s[6]; c.dvs = ps.s[7]; c.ls = ps.ls; c.stream = hip_stream

int fa2_fwd_varlen(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Hkv,
                   int max_seqlen_q, int max_seqlen_k, int D, const int* cu_seqlens_q, const int* cu_seqlens_k,
                   const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2], const int64_t o_strides[2],
                   int64_t lse_stride, float scale, int flags, int window_left, int window_right, void* hip_stream) {
    FwdCall c;
    PackedStrides ps;
    FA2_PACKED_FILL(c, Hkv);
    if (int rc = packed_call(c, ps, {q_strides, k_strides, v_strides, o_strides}, lse_stride, flags, window_left, window_right)) return rc;
    FA2_PACKED_FWD_FILL(c, ps);
    return fwd_run(c);
}

int fa2_fwd_varlen_plan(int dtype, int B, int H, int Hkv, int max_seqlen_q, int max_seqlen_k, int D, const int64_t q_strides[2], const int64_t k_strides[2],
                        float scale, int flags, int window_left, int window_right, fa2_fwd_plan_t* plan) {
    if (!plan) return FA2_ERR_NULL_POINTER;
    const int64_t cq[2] = {D, (int64_t)H * D}, ck[2] = {D, (int64_t)Hkv * D};          // a contiguous [total, heads, D]
    const int64_t *qs = q_strides ? q_strides : cq, *ks = k_strides ? k_strides : ck;
    FwdCall c;
    PackedStrides ps;
    FA2_PACKED_FILL(c, Hkv);
    if (int rc = packed_call(c, ps, {qs, ks, ks, qs}, 0, flags, window_left, window_right)) return rc;
    c.qs = ps.s[0]; c.ks = ps.s[1]; c.vs = ps.s[2]; c.os = ps.s[3]; c.ls = ps.ls;
    c.ask = Ask::Plan; c.plan = plan;
    return fwd_run(c);
}

// ... with V and O of head dim Dv < D (the non-absorbed MLA prefill, 192 / 128; varlen_dv_hip.cpp).  Dv < 1 is a bad size like the others; the pair is
// checked with the head dim (fwd_validate); V's span rule and descriptor use Dv.
int fa2_fwd_varlen_dv(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Hkv,
                      int max_seqlen_q, int max_seqlen_k, int D, int Dv, const int* cu_seqlens_q, const int* cu_seqlens_k,
                      const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2], const int64_t o_strides[2],
                      int64_t lse_stride, float scale, int flags, int window_left, int window_right, void* hip_stream) {
    FwdCall c;
    PackedStrides ps;
    FA2_PACKED_FILL(c, Hkv);
    if (Dv < 1) return FA2_ERR_BAD_SHAPE;
    if (int rc = packed_call(c, ps, {q_strides, k_strides, v_strides, o_strides}, lse_stride, flags, window_left, window_right)) return rc;
    FA2_PACKED_FWD_FILL(c, ps);
    c.Dv = Dv;
    return fwd_run(c);
}

int fa2_fwd_varlen_dv_plan(int dtype, int B, int H, int Hkv, int max_seqlen_q, int max_seqlen_k, int D, int Dv, const int64_t q_strides[2],
                           const int64_t k_strides[2], float scale, int flags, int window_left, int window_right, fa2_fwd_plan_t* plan) {
    if (!plan) return FA2_ERR_NULL_POINTER;
    const int64_t cq[2] = {D, (int64_t)H * D}, ck[2] = {D, (int64_t)Hkv * D};          // a contiguous [total, heads, D]; V and O take K's and Q's
    const int64_t *qs = q_strides ? q_strides : cq, *ks = k_strides ? k_strides : ck;
    FwdCall c;
    PackedStrides ps;
    FA2_PACKED_FILL(c, Hkv);
    if (Dv < 1) return FA2_ERR_BAD_SHAPE;
    if (int rc = packed_call(c, ps, {qs, ks, ks, qs}, 0, flags, window_left, window_right)) return rc;
    c.qs = ps.s[0]; c.ks = ps.s[1]; c.vs = ps.s[2]; c.os = ps.s[3]; c.ls = ps.ls;
    c.Dv = Dv;
    c.ask = Ask::Plan; c.plan = plan;
    return fwd_run(c);
}

int fa2_bwd_varlen(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                   void* dq, void* dk, void* dv, float* delta_ws, int B, int H, int max_seqlen_q, int max_seqlen_k, int D,
                   const int* cu_seqlens_q, const int* cu_seqlens_k,
                   const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2], const int64_t o_strides[2],
                   const int64_t do_strides[2], const int64_t dq_strides[2], const int64_t dk_strides[2], const int64_t dv_strides[2],
                   int64_t lse_stride, float scale, int flags, int window_left, int window_right, void* hip_stream) {
    BwdCall c;
    PackedStrides ps;
    FA2_PACKED_FILL(c, H);
    if (int rc = packed_call(c, ps, {q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides, dk_strides, dv_strides}, lse_stride, flags,
                             window_left, window_right))
        return rc;
    FA2_PACKED_BWD_FILL(c, ps);
    return bwd_run(c);
}

static int varlen_range(bool transpose, int Nq_s, int Nkv_s, int left, int right, int flags, int row0, int rows, int tile, int* first_tile, int* ntiles) {
    if (!first_tile || !ntiles) return FA2_ERR_NULL_POINTER;
    if (flags & ~(FA2_FLAG_CAUSAL | FA2_FLAG_EXACT_SCALE | FA2_FLAG_BOTTOM_RIGHT)) return FA2_ERR_BAD_SHAPE;
    if (Nq_s < 0 || Nkv_s < 0 || row0 < 0 || rows < 1 || tile < 1 || rows > (1 << 24) || row0 > 0x7fffffff - (1 << 24)) return FA2_ERR_BAD_SHAPE;
    const int off = (flags & FA2_FLAG_BOTTOM_RIGHT) ? Nkv_s - Nq_s : 0;             // (|off| <= max(Nq_s, Nkv_s): no overflow)
    if (!fa2::window_args_ok(Nq_s, Nkv_s, left, right, off, true)) return FA2_ERR_BAD_SHAPE;
    right = fa2::window_normalize_right(right, (flags & FA2_FLAG_CAUSAL) != 0);
    if (transpose) fa2::window_row_range(Nq_s, Nkv_s, left, right, off, row0, rows, tile, first_tile, ntiles);
    else fa2::window_tile_range(Nq_s, Nkv_s, left, right, off, row0, rows, tile, first_tile, ntiles);
    return FA2_OK;
}

int fa2_varlen_tile_range(int Nq_s, int Nkv_s, int window_left, int window_right, int flags, int row0, int rows, int tile, int* first_tile, int* ntiles) {
    return varlen_range(false, Nq_s, Nkv_s, window_left, window_right, flags, row0, rows, tile, first_tile, ntiles);
}

int fa2_varlen_row_range(int Nq_s, int Nkv_s, int window_left, int window_right, int flags, int key0, int keys, int tile, int* first_tile, int* ntiles) {
    return varlen_range(true, Nq_s, Nkv_s, window_left, window_right, flags, key0, keys, tile, first_tile, ntiles);
}

// ---- attention dropout: include/fa2_gfx950.h has the contract, fa2_dropout.h the mask, dropout_hip.cpp / varlen_dropout_hip.cpp the kernels.
// These calls always take the windowed (packed) kernel family, also when the window masks nothing: its DROP forms are the only kernels with the mask.
int fa2_fwd_dropout(int dtype, FA2_FWD_ARGS(FA2_HKV), int window_left, int window_right, int q_offset, void* hip_stream, float dropout_p, uint64_t seed) {
    if (!dropout_p_ok(dropout_p)) return FA2_ERR_DROPOUT;
    if (Hkv < 1) return FA2_ERR_BAD_SHAPE;
    FA2_FWD_CALL(c);
    c.Hkv = Hkv;
    set_dropout_args(c, dropout_p, seed);
    if (int rc = dense_window(c, flags, window_left, window_right, q_offset)) return rc;
    return fwd_run(c);
}

int fa2_bwd_dropout(int dtype, FA2_BWD_ARGS(), int window_left, int window_right, int q_offset, void* hip_stream, float dropout_p, uint64_t seed) {
    if (!dropout_p_ok(dropout_p)) return FA2_ERR_DROPOUT;
    FA2_BWD_CALL(c);
    set_dropout_args(c, dropout_p, seed);
    if (int rc = dense_window(c, flags, window_left, window_right, q_offset)) return rc;
    return bwd_run(c);
}

int fa2_fwd_varlen_dropout(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Hkv,
                           int max_seqlen_q, int max_seqlen_k, int D, const int* cu_seqlens_q, const int* cu_seqlens_k,
                           const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2], const int64_t o_strides[2],
                           int64_t lse_stride, float scale, int flags, int window_left, int window_right, void* hip_stream, float dropout_p, uint64_t seed) {
    if (!dropout_p_ok(dropout_p)) return FA2_ERR_DROPOUT;
    FwdCall c;
    PackedStrides ps;
    set_dropout_args(c, dropout_p, seed);
    FA2_PACKED_FILL(c, Hkv);
    if (int rc = packed_call(c, ps, {q_strides, k_strides, v_strides, o_strides}, lse_stride, flags, window_left, window_right)) return rc;
    FA2_PACKED_FWD_FILL(c, ps);
    return fwd_run(c);
}

int fa2_bwd_varlen_dropout(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                           void* dq, void* dk, void* dv, float* delta_ws, int B, int H, int max_seqlen_q, int max_seqlen_k, int D,
                           const int* cu_seqlens_q, const int* cu_seqlens_k,
                           const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2], const int64_t o_strides[2],
                           const int64_t do_strides[2], const int64_t dq_strides[2], const int64_t dk_strides[2], const int64_t dv_strides[2],
                           int64_t lse_stride, float scale, int flags, int window_left, int window_right, void* hip_stream, float dropout_p, uint64_t seed) {
    if (!dropout_p_ok(dropout_p)) return FA2_ERR_DROPOUT;
    BwdCall c;
    PackedStrides ps;
    set_dropout_args(c, dropout_p, seed);
    FA2_PACKED_FILL(c, H);
    if (int rc = packed_call(c, ps, {q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides, dk_strides, dv_strides}, lse_stride, flags,
                             window_left, window_right))
        return rc;
    FA2_PACKED_BWD_FILL(c, ps);
    return bwd_run(c);
}

// ---- score modifiers (logit soft-capping, ALiBi slopes): include/fa2_gfx950.h has the contract, fa2_scoremod.h the arithmetic, scoremod_hip.cpp /
// varlen_scoremod_hip.cpp the kernels.  With softcap > 0 or slopes these calls always take the SMOD forms of the windowed (packed) kernels, whatever the
// window masks; with neither they are fa2_fwd_window / fa2_bwd_window / fa2_fwd_varlen / fa2_bwd_varlen.
int fa2_fwd_scoremod(int dtype, FA2_FWD_ARGS(FA2_HKV), int window_left, int window_right, int q_offset, void* hip_stream, float softcap,
                     const float* alibi_slopes, int64_t alibi_batch_stride) {
    FA2_FWD_CALL(c);
    if (int rc = set_scoremod_args(c, softcap, alibi_slopes, alibi_batch_stride)) return rc;
    if (Hkv < 1) return FA2_ERR_BAD_SHAPE;
    c.Hkv = Hkv;
    if (int rc = dense_window(c, flags, window_left, window_right, q_offset)) return rc;
    return fwd_run(c);
}

int fa2_bwd_scoremod(int dtype, FA2_BWD_ARGS(), int window_left, int window_right, int q_offset, void* hip_stream, float softcap,
                     const float* alibi_slopes, int64_t alibi_batch_stride) {
    FA2_BWD_CALL(c);
    if (int rc = set_scoremod_args(c, softcap, alibi_slopes, alibi_batch_stride)) return rc;
    if (int rc = dense_window(c, flags, window_left, window_right, q_offset)) return rc;
    return bwd_run(c);
}

int fa2_fwd_varlen_scoremod(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Hkv,
                            int max_seqlen_q, int max_seqlen_k, int D, const int* cu_seqlens_q, const int* cu_seqlens_k,
                            const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2], const int64_t o_strides[2],
                            int64_t lse_stride, float scale, int flags, int window_left, int window_right, void* hip_stream, float softcap,
                            const float* alibi_slopes, int64_t alibi_batch_stride) {
    FwdCall c;
    PackedStrides ps;
    if (int rc = set_scoremod_args(c, softcap, alibi_slopes, alibi_batch_stride)) return rc;
    FA2_PACKED_FILL(c, Hkv);
    if (int rc = packed_call(c, ps, {q_strides, k_strides, v_strides, o_strides}, lse_stride, flags, window_left, window_right)) return rc;
    FA2_PACKED_FWD_FILL(c, ps);
    return fwd_run(c);
}

int fa2_bwd_varlen_scoremod(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                            void* dq, void* dk, void* dv, float* delta_ws, int B, int H, int max_seqlen_q, int max_seqlen_k, int D,
                            const int* cu_seqlens_q, const int* cu_seqlens_k,
                            const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2], const int64_t o_strides[2],
                            const int64_t do_strides[2], const int64_t dq_strides[2], const int64_t dk_strides[2], const int64_t dv_strides[2],
                            int64_t lse_stride, float scale, int flags, int window_left, int window_right, void* hip_stream, float softcap,
                            const float* alibi_slopes, int64_t alibi_batch_stride) {
    BwdCall c;
    PackedStrides ps;
    if (int rc = set_scoremod_args(c, softcap, alibi_slopes, alibi_batch_stride)) return rc;
    FA2_PACKED_FILL(c, H);
    if (int rc = packed_call(c, ps, {q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides, dk_strides, dv_strides}, lse_stride, flags,
                             window_left, window_right))
        return rc;
    FA2_PACKED_BWD_FILL(c, ps);
    return bwd_run(c);
}

int fa2_scoremod_eval(float x, float softcap, float slope, int pos, int j, float* s, float* dfactor) {
    if (!fa2::softcap_ok(softcap)) return FA2_ERR_SOFTCAP;
    if (!s || !dfactor) return FA2_ERR_NULL_POINTER;
    const int64_t d = (int64_t)pos - (int64_t)j;
    const fa2::ScoreMod m = fa2::make_scoremod(softcap, 1.0f, nullptr, 0);
    *s = fa2::smod_score(x, m.softcap, m.inv_softcap, slope, (float)(d < 0 ? -d : d), dfactor);
    return FA2_OK;
}

int fa2_dropout_threshold(float dropout_p, float* p_eff) {
    if (!dropout_p_ok(dropout_p)) return FA2_ERR_DROPOUT;
    return (int)fa2::dropout_threshold(dropout_p, p_eff);
}

int fa2_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    if (!ctr || !key || !out) return FA2_ERR_NULL_POINTER;
    uint32_t o[4];
    fa2::philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], o);
    for (int i = 0; i < 4; ++i) out[i] = o[i];
    return FA2_OK;
}

int fa2_dropout_keep_mask(uint64_t seed, float dropout_p, int H, int b, int h, int64_t i0, int64_t i1, int64_t j0, int64_t j1, uint8_t* mask) {
    if (!dropout_p_ok(dropout_p)) return FA2_ERR_DROPOUT;
    if (!mask) return FA2_ERR_NULL_POINTER;
    if (H < 1 || b < 0 || h < 0 || h >= H || i0 < 0 || j0 < 0 || i1 <= i0 || j1 <= j0 || i1 > 0x7fffffffLL || j1 > 0x7fffffffLL ||
        (int64_t)b * H + h > 0xffffffffLL)
        return FA2_ERR_BAD_SHAPE;
    const uint32_t t = fa2::dropout_threshold(dropout_p, nullptr), bh = (uint32_t)((int64_t)b * H + h);
    for (int64_t i = i0; i < i1; ++i)
        for (int64_t j = j0; j < j1; ++j) mask[(i - i0) * (j1 - j0) + (j - j0)] = fa2::dropout_keep(seed, t, bh, (uint32_t)i, (uint32_t)j) ? 1 : 0;
    return FA2_OK;
}

// ---- a gradient for the LSE: include/fa2_gfx950.h has the contract.  Each entry point is a superset of a family — one more optional field of the call
// description —, and with dlse == NULL it IS the existing call of the same arguments.
int fa2_bwd_lse(int dtype, FA2_BWD_ARGS(), const void* bias, int bias_kind, const int64_t bias_strides[3], void* workspace, size_t workspace_bytes,
                void* hip_stream, const float* dlse, const int64_t dlse_strides[2]) {
    FA2_BWD_CALL(c);
    c.bias.ptr = bias; c.bias.kind = bias_kind; c.bias.strides = bias_strides;
    c.ws = workspace; c.ws_bytes = workspace_bytes;
    c.dlse = dlse; c.dlses = dlse_strides;
    return bwd_run(c);
}

int fa2_bwd_lse_plan(int dtype, int B, int H, int Hkv, int Nq, int Nkv, int D, const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                     const int64_t o_strides[3], const int64_t do_strides[3], float scale, int flags, int bias_kind, const int64_t bias_strides[3],
                     int has_dlse, fa2_bwd_plan_t* plan) {
    if (!plan) return FA2_ERR_NULL_POINTER;
    if (B < 1 || H < 1 || Hkv < 1 || Nq < 1 || Nkv < 1 || D < 1) return FA2_ERR_BAD_SHAPE;
    const int64_t d = D, q[3] = {(int64_t)H * Nq * d, (int64_t)Nq * d, d}, k[3] = {(int64_t)Hkv * Nkv * d, (int64_t)Nkv * d, d};
    static const int64_t ls[2] = {0, 0};
    static const float some_dlse = 0.f;          // (a plan query reads no tensor: any non-null value says "this call has a dlse")
    FA2_QUERY_CALL(BwdCall, c, Hkv);
    c.scale = scale; c.bias.kind = bias_kind; c.bias.strides = bias_strides;
    c.qs = c.dqs = q_strides ? q_strides : q; c.ks = c.dks = k_strides ? k_strides : k; c.vs = c.dvs = v_strides ? v_strides : k;
    c.os = o_strides ? o_strides : q; c.dos = do_strides ? do_strides : q; c.ls = ls;
    c.dlse = has_dlse ? &some_dlse : nullptr;
    c.ask = Ask::Plan; c.plan = plan;
    return bwd_run(c);
}

// dropout_p > 0: fa2_bwd_dropout; softcap > 0 or slopes: fa2_bwd_scoremod; neither: fa2_bwd_window.  Never both (the kernels have no such form).
static int window_lse_family(Call& c, float dropout_p, uint64_t seed, float softcap, const float* alibi_slopes, int64_t alibi_batch_stride) {
    if (!dropout_p_ok(dropout_p)) return FA2_ERR_DROPOUT;
    if (int rc = set_scoremod_args(c, softcap, alibi_slopes, alibi_batch_stride)) return rc;
    if (dropout_p > 0.f && c.scoremod) return FA2_ERR_DROPOUT;
    if (dropout_p > 0.f) set_dropout_args(c, dropout_p, seed);
    return FA2_OK;
}

int fa2_bwd_window_lse(int dtype, FA2_BWD_ARGS(), int window_left, int window_right, int q_offset, void* hip_stream, float dropout_p, uint64_t seed,
                       float softcap, const float* alibi_slopes, int64_t alibi_batch_stride, const float* dlse, const int64_t dlse_strides[2]) {
    FA2_BWD_CALL(c);
    if (int rc = window_lse_family(c, dropout_p, seed, softcap, alibi_slopes, alibi_batch_stride)) return rc;
    if (int rc = dense_window(c, flags, window_left, window_right, q_offset)) return rc;
    c.dlse = dlse; c.dlses = dlse_strides;
    return bwd_run(c);
}

int fa2_bwd_varlen_lse(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                       void* dq, void* dk, void* dv, float* delta_ws, int B, int H, int max_seqlen_q, int max_seqlen_k, int D,
                       const int* cu_seqlens_q, const int* cu_seqlens_k,
                       const int64_t q_strides[2], const int64_t k_strides[2], const int64_t v_strides[2], const int64_t o_strides[2],
                       const int64_t do_strides[2], const int64_t dq_strides[2], const int64_t dk_strides[2], const int64_t dv_strides[2],
                       int64_t lse_stride, float scale, int flags, int window_left, int window_right, void* hip_stream, float dropout_p, uint64_t seed,
                       float softcap, const float* alibi_slopes, int64_t alibi_batch_stride, const float* dlse, int64_t dlse_stride) {
    BwdCall c;
    PackedStrides ps;
    if (int rc = window_lse_family(c, dropout_p, seed, softcap, alibi_slopes, alibi_batch_stride)) return rc;
    FA2_PACKED_FILL(c, H);
    if (int rc = packed_call(c, ps, {q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides, dk_strides, dv_strides}, lse_stride, flags,
                             window_left, window_right))
        return rc;
    FA2_PACKED_BWD_FILL(c, ps);
    const int64_t dls[2] = {0, dlse_stride};
    c.dlse = dlse; c.dlses = dls;
    return bwd_run(c);
}

// ---- merge of partial attention results: include/fa2_gfx950.h has the contract, merge_hip.cpp the kernels
static bool strides3_ok(const int64_t* s) { return s[0] >= 0 && s[1] >= 0 && strides_ok(s); }
static int merge_common(fa2::MergeParams& p, int dtype, int nparts, const void* const* o_parts, const float* const* lse_parts, int B, int H, int Nq, int D,
                        const int64_t part_strides[3], const int64_t part_lse_strides[2], int flags) {
    if (dtype != FA2_DTYPE_F16 && dtype != FA2_DTYPE_BF16) return FA2_ERR_DTYPE;
    if (nparts < 1 || nparts > fa2::kMergeMaxParts || B < 1 || H < 1 || Nq < 1 || D < 1 || (flags & ~FA2_MERGE_NATURAL_LSE)) return FA2_ERR_BAD_SHAPE;
    if ((D & 7) || D > kMaxBwdHeadDim) return FA2_ERR_HEAD_DIM;
    if (!o_parts || !lse_parts || !part_strides || !part_lse_strides) return FA2_ERR_NULL_POINTER;
    for (int k = 0; k < nparts; ++k) {
        if (!o_parts[k] || !lse_parts[k]) return FA2_ERR_NULL_POINTER;
        if (!aligned16(o_parts[k]) || (reinterpret_cast<uintptr_t>(lse_parts[k]) & 3u)) return FA2_ERR_ALIGNMENT;
    }
    if (!strides3_ok(part_strides)) return FA2_ERR_ALIGNMENT;
    if (part_lse_strides[0] < 0 || part_lse_strides[1] < 0) return FA2_ERR_BAD_SHAPE;
    std::memset(&p, 0, sizeof(p));
    for (int k = 0; k < nparts; ++k) { p.o_parts[k] = o_parts[k]; p.lse_parts[k] = lse_parts[k]; }
    p.nparts = nparts; p.B = B; p.H = H; p.Nq = Nq; p.D = D; p.natural = (flags & FA2_MERGE_NATURAL_LSE) != 0;
    for (int i = 0; i < 3; ++i) p.ps[i] = part_strides[i];
    p.pls[0] = part_lse_strides[0]; p.pls[1] = part_lse_strides[1];
    return FA2_OK;
}

int fa2_merge_fwd(int dtype, int nparts, const void* const* o_parts, const float* const* lse_parts, void* o, float* lse, int B, int H, int Nq, int D,
                  const int64_t part_strides[3], const int64_t part_lse_strides[2], const int64_t o_strides[3], const int64_t lse_strides[2], int flags,
                  void* hip_stream) {
    fa2::MergeParams p;
    if (int rc = merge_common(p, dtype, nparts, o_parts, lse_parts, B, H, Nq, D, part_strides, part_lse_strides, flags)) return rc;
    if (!o || !lse || !o_strides || !lse_strides) return FA2_ERR_NULL_POINTER;
    if (!aligned16(o) || (reinterpret_cast<uintptr_t>(lse) & 3u) || !strides3_ok(o_strides)) return FA2_ERR_ALIGNMENT;
    if (lse_strides[0] < 0 || lse_strides[1] < 0) return FA2_ERR_BAD_SHAPE;
    p.o = o; p.lse = lse;
    for (int i = 0; i < 3; ++i) p.os[i] = o_strides[i];
    p.ls[0] = lse_strides[0]; p.ls[1] = lse_strides[1];
    return fa2::launch_merge_fwd(dtype == FA2_DTYPE_BF16, p, (hipStream_t)hip_stream);
}

int fa2_merge_bwd(int dtype, int nparts, const void* const* o_parts, const float* const* lse_parts, const float* lse, const void* dout, const float* dlse,
                  void* const* do_parts, float* const* dlse_parts, int B, int H, int Nq, int D, const int64_t part_strides[3],
                  const int64_t part_lse_strides[2], const int64_t lse_strides[2], const int64_t do_strides[3], const int64_t dlse_strides[2],
                  const int64_t dpart_strides[3], const int64_t dpart_lse_strides[2], int flags, void* hip_stream) {
    fa2::MergeParams p;
    if (int rc = merge_common(p, dtype, nparts, o_parts, lse_parts, B, H, Nq, D, part_strides, part_lse_strides, flags)) return rc;
    if (!lse || !dout || !do_parts || !dlse_parts || !lse_strides || !do_strides || !dpart_strides || !dpart_lse_strides || (dlse && !dlse_strides))
        return FA2_ERR_NULL_POINTER;
    for (int k = 0; k < nparts; ++k) {
        if (!do_parts[k] || !dlse_parts[k]) return FA2_ERR_NULL_POINTER;
        if (!aligned16(do_parts[k]) || (reinterpret_cast<uintptr_t>(dlse_parts[k]) & 3u)) return FA2_ERR_ALIGNMENT;
    }
    if (!aligned16(dout) || ((reinterpret_cast<uintptr_t>(lse) | reinterpret_cast<uintptr_t>(dlse)) & 3u) || !strides3_ok(do_strides) ||
        !strides3_ok(dpart_strides))
        return FA2_ERR_ALIGNMENT;
    if (lse_strides[0] < 0 || lse_strides[1] < 0 || dpart_lse_strides[0] < 0 || dpart_lse_strides[1] < 0 || (dlse && (dlse_strides[0] < 0 || dlse_strides[1] < 0)))
        return FA2_ERR_BAD_SHAPE;
    for (int k = 0; k < nparts; ++k) { p.do_parts[k] = do_parts[k]; p.dlse_parts[k] = dlse_parts[k]; }
    p.lse = const_cast<float*>(lse); p.dout = dout; p.dlse = dlse;
    for (int i = 0; i < 3; ++i) { p.dos[i] = do_strides[i]; p.dps[i] = dpart_strides[i]; }
    p.ls[0] = lse_strides[0]; p.ls[1] = lse_strides[1];
    p.dpls[0] = dpart_lse_strides[0]; p.dpls[1] = dpart_lse_strides[1];
    if (dlse) { p.dls[0] = dlse_strides[0]; p.dls[1] = dlse_strides[1]; }
    return fa2::launch_merge_bwd(dtype == FA2_DTYPE_BF16, p, (hipStream_t)hip_stream);
}

// ---- KV-cache decode attention: include/fa2_gfx950.h has the contract, csrc/fa2_decode.hip.h the kernel, decode_hip.cpp its launches
// A KV cache as the decode and the append calls are handed it, and its checks, each inside one error class (the callers keep the classes' order).
struct CacheDesc {
    const void *k = nullptr, *v = nullptr;                  // [B, capacity, Hkv, D], or a pool [num_pages, page_size, Hkv, D] under a block table
    const int* block_table = nullptr;
    int capacity = 0, page_size = 0, num_pages = 0;         // capacity: key slots (page_size == 0) or block-table entries per sequence
    const int64_t *ks = nullptr, *vs = nullptr;             // {batch | page, head, row} in elements, which are bytes in an e4m3 cache
    int64_t bts = 0;
    int format = FA2_CACHE_16BIT;
    const float *kd = nullptr, *vd = nullptr;               // per (sequence, K / V head) descales: e4m3 caches alone
    const int64_t* ds = nullptr;
    bool fp8() const { return format == FA2_CACHE_E4M3; }
    bool descaled() const { return kd || vd; }
    int64_t capacity_keys() const { return page_size ? (int64_t)capacity * page_size : capacity; }
};
// null pointers: a paged call needs its block table, a descale its stride pair
static bool cache_null(const CacheDesc& c) { return any_null({c.k, c.v, c.ks, c.vs}) || (c.page_size > 0 && !c.block_table) || (c.descaled() && !c.ds); }
// sizes: pages of a multiple of 64 keys, and key positions are ints
static bool cache_paging_ok(const CacheDesc& c) {
    return c.capacity >= 1 && c.page_size >= 0 && c.page_size % 64 == 0 && (c.page_size == 0 || (int64_t)c.capacity * c.page_size <= 0x7fffffffLL - 64);
}
// sizes again, apart from the above: the decode call looks at these two after the head dim, the append before it
static bool cache_extent_ok(const CacheDesc& c) { return !(c.page_size > 0 && c.num_pages < 1) && !(c.descaled() && (c.ds[0] < 0 || c.ds[1] < 0)); }
// alignment: a 16-byte load covers 8 columns of a 16-bit cache and 16 of an e4m3 one
static bool cache_aligned(const CacheDesc& c) {
    const auto strides_ok = [&c](const int64_t* st) { return strides3_ok(st) && (!c.fp8() || ((st[0] | st[1] | st[2]) & 15) == 0); };
    return all_aligned16({c.k, c.v}) && strides_ok(c.ks) && strides_ok(c.vs) && c.bts >= 0 &&
           !((reinterpret_cast<uintptr_t>(c.block_table) | reinterpret_cast<uintptr_t>(c.kd) | reinterpret_cast<uintptr_t>(c.vd)) & 3u);
}
// dtype: one of the two formats, descales with e4m3 alone (fa2_fwd_decode and fa2_fwd_decode_fp8 state a format that passes)
static bool cache_format_ok(const CacheDesc& c) { return (c.format == FA2_CACHE_16BIT || c.fp8()) && (!c.descaled() || c.fp8()); }

// One decode call, described: the three entries fill it by field name; a plan or size query fills the sizes alone.
struct DecodeCall : CacheDesc {
    int dtype = 0, B = 0, H = 0, Hkv = 0, Nq = 0, D = 0;
    const void* q = nullptr;
    void* o = nullptr;
    float* lse = nullptr;
    const int* lens = nullptr;
    const int64_t *qs = nullptr, *os = nullptr, *ls = nullptr;      // {batch, head, row}; ls: {batch, head}
    float scale = 0.f;
    int window_left = -1;                                           // what fa2_fwd_decode_window adds: the older entries leave these four as they are
    float softcap = 0.f;
    const float* slopes = nullptr;
    int64_t slope_stride = 0;
    int num_splits = 0;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    void* stream = nullptr;
};

// The sizes of a decode call, in the documented order (shape, then head dim); *row_tiles: the row tiles the kernel runs (1, 2 or 4).
static int decode_check_shape(const DecodeCall& c, int* row_tiles) {
    if (c.B < 1 || c.H < 1 || c.Hkv < 1 || c.Nq < 1 || c.D < 1 || c.Hkv > c.H || c.H % c.Hkv != 0) return FA2_ERR_BAD_SHAPE;
    const int64_t rows = (int64_t)c.Nq * (c.H / c.Hkv);
    if (rows > fa2::kDecodeMaxRows || !cache_paging_ok(c) || c.num_splits < 0 || c.num_splits > fa2::kDecodeMaxSplit) return FA2_ERR_BAD_SHAPE;
    if (c.D != 64 && c.D != 128) return FA2_ERR_HEAD_DIM;
    const int rt = (int)((rows + 15) / 16);
    *row_tiles = rt == 3 ? 4 : rt;
    return FA2_OK;
}

// The split: a pure function of the shape, the capacity and the CU count (the lengths live on the device).  One workgroup per (sequence, K / V head,
// part) streams its share of K and V once; B * Hkv * row_tiles >= CUs: the chip is covered, no split.  Otherwise two workgroups per CU's worth of
// parts (a workgroup is 4 waves and 36 KiB of LDS: two fit), at most 16, and no part shorter than 8 key tiles of the capacity (two per wave).
static int decode_split(int B, int Hkv, int row_tiles, int capacity_tiles, int num_splits) {
    if (num_splits > 0) return num_splits;
    const int64_t work = (int64_t)B * Hkv * row_tiles, cus = fa2::device_cus();
    if (work >= cus) return 1;
    int64_t S = 2 * cus / work;
    if (S > fa2::kDecodeMaxSplit) S = fa2::kDecodeMaxSplit;
    if (S > capacity_tiles / 8) S = capacity_tiles / 8;
    return S < 1 ? 1 : (int)S;
}

// window_left >= 0 (fa2_fwd_decode_window): "8 key tiles of the capacity" becomes "... of the span a sequence can sweep" — a window of window_left keys
// under Nq rows touches at most ceil((window_left + Nq) / 32) + 1 tiles wherever it starts, so a short window in a long cache is not cut into parts
// of a tile or two.  A window that reaches across the whole cache changes nothing.
static int decode_plan(const DecodeCall& c, int window_left, fa2_decode_plan_t* plan) {
    if (window_left < -1) return FA2_ERR_BAD_SHAPE;
    int row_tiles = 0;
    if (int rc = decode_check_shape(c, &row_tiles)) return rc;
    if (c.dtype != FA2_DTYPE_F16 && c.dtype != FA2_DTYPE_BF16) return FA2_ERR_DTYPE;
    int64_t span_tiles = (c.capacity_keys() + fa2::kDecodeTile - 1) / fa2::kDecodeTile;
    if (window_left >= 0) {
        const int64_t w = ((int64_t)window_left + c.Nq + fa2::kDecodeTile - 1) / fa2::kDecodeTile + 1;
        if (w < span_tiles) span_tiles = w;
    }
    plan->kernel = FA2_KERNEL_HIP_DECODE;
    plan->row_tiles = row_tiles;
    plan->key_tile = fa2::kDecodeTile;
    plan->nsplit = decode_split(c.B, c.Hkv, row_tiles, (int)span_tiles, c.num_splits);
    return FA2_OK;
}

// The f32 parts a split call leaves between its two launches.
static size_t decode_ws_need(const DecodeCall& c, const fa2_decode_plan_t& plan) {
    return (size_t)fa2::decode_ws_bytes((int64_t)c.B * c.Hkv, plan.nsplit, c.Nq * (c.H / c.Hkv), c.D);
}

// The sizes every decode query and entry takes, filled by field name.
#define FA2_DECODE_SIZES(c) \
    DecodeCall c;           \
    c.dtype = dtype; c.B = B; c.H = H; c.Hkv = Hkv; c.Nq = Nq; c.D = D; c.capacity = capacity; c.page_size = page_size; c.num_splits = num_splits

int fa2_fwd_decode_window_plan(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits, int window_left,
                               fa2_decode_plan_t* plan) {
    if (!plan) return FA2_ERR_NULL_POINTER;
    std::memset(plan, 0, sizeof(*plan));
    FA2_DECODE_SIZES(c);
    return decode_plan(c, window_left, plan);
}

size_t fa2_fwd_decode_window_workspace_bytes(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits, int window_left) {
    fa2_decode_plan_t plan;
    FA2_DECODE_SIZES(c);
    return decode_plan(c, window_left, &plan) ? 0 : decode_ws_need(c, plan);
}

int fa2_fwd_decode_plan(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits, fa2_decode_plan_t* plan) {
    return fa2_fwd_decode_window_plan(dtype, B, H, Hkv, Nq, D, capacity, page_size, num_splits, -1, plan);
}

size_t fa2_fwd_decode_workspace_bytes(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits) {
    return fa2_fwd_decode_window_workspace_bytes(dtype, B, H, Hkv, Nq, D, capacity, page_size, num_splits, -1);
}

int fa2_decode_part_range(int64_t len, int64_t capacity_keys, int Nq, int tile, int nsplit, int part, int* first_tile, int* ntiles) {
    if (!first_tile || !ntiles) return FA2_ERR_NULL_POINTER;
    if (capacity_keys < 0 || capacity_keys > 0x7fffffffLL || Nq < 1 || tile < 1 || nsplit < 1 || nsplit > fa2::kDecodeMaxSplit || part < 0 || part >= nsplit)
        return FA2_ERR_BAD_SHAPE;
    fa2::decode_part_range(len, capacity_keys, Nq, tile, nsplit, part, first_tile, ntiles);
    return FA2_OK;
}

int fa2_decode_window_part_range(int64_t len, int64_t capacity_keys, int Nq, int window_left, int tile, int nsplit, int part, int* first_tile, int* ntiles) {
    if (!first_tile || !ntiles) return FA2_ERR_NULL_POINTER;
    if (capacity_keys < 0 || capacity_keys > 0x7fffffffLL || Nq < 1 || tile < 1 || nsplit < 1 || nsplit > fa2::kDecodeMaxSplit || part < 0 || part >= nsplit ||
        window_left < -1)
        return FA2_ERR_BAD_SHAPE;
    fa2::decode_window_part_range(len, capacity_keys, Nq, window_left, tile, nsplit, part, first_tile, ntiles);
    return FA2_OK;
}

// One body for fa2_fwd_decode, fa2_fwd_decode_fp8 and fa2_fwd_decode_window (fp8: e4m3 caches, whose element strides are bytes; the descales and their
// strides belong to e4m3 caches alone).  The checks run in the documented order; the window entry's arguments are checked where their kind is.
// A call whose window reaches across the whole cache, without a cap and without slopes, runs the plain kernels: the same bits as the older entries.
static int decode_run(const DecodeCall& c) {
    if (any_null({c.q, c.o, c.lse, c.lens, c.qs, c.os, c.ls}) || cache_null(c)) return FA2_ERR_NULL_POINTER;
    if (c.window_left < -1 || c.slope_stride < 0) return FA2_ERR_BAD_SHAPE;
    int row_tiles = 0;
    if (int rc = decode_check_shape(c, &row_tiles)) return rc;
    if (!cache_extent_ok(c) || c.ls[0] < 0 || c.ls[1] < 0) return FA2_ERR_BAD_SHAPE;
    if (!all_aligned16({c.q, c.o}) || !cache_aligned(c) ||
        ((reinterpret_cast<uintptr_t>(c.lse) | reinterpret_cast<uintptr_t>(c.lens) | reinterpret_cast<uintptr_t>(c.slopes)) & 3u) || !strides3_ok(c.qs) ||
        !strides3_ok(c.os))
        return FA2_ERR_ALIGNMENT;
    // window_left >= capacity_keys - 1: EVERY row (the last one sits at len - 1 <= capacity_keys - 1) sees every key at or below it
    const int window_left = (int64_t)c.window_left + 1 >= c.capacity_keys() ? -1 : c.window_left;
    fa2_decode_plan_t plan;
    if (int rc = decode_plan(c, window_left, &plan)) return rc;       // (the dtype: after the alignment)
    if (!cache_format_ok(c)) return FA2_ERR_DTYPE;
    if (!std::isfinite(c.scale)) return FA2_ERR_SCALE;
    if (!fa2::softcap_ok(c.softcap)) return FA2_ERR_SOFTCAP;
    if (c.B > 65535 || c.Hkv > 65535) return FA2_ERR_GRID;
    fa2::DecodeParams p;
    std::memset(&p, 0, sizeof(p));
    p.q = c.q; p.k = c.k; p.v = c.v; p.o = c.o; p.lse = c.lse; p.lens = c.lens; p.bt = c.page_size > 0 ? c.block_table : nullptr;
    p.B = c.B; p.H = c.H; p.Hkv = c.Hkv; p.Nq = c.Nq; p.G = c.H / c.Hkv; p.rows = c.Nq * p.G;
    p.page_size = c.page_size; p.num_pages = c.num_pages; p.nsplit = plan.nsplit;
    p.capacity_keys = c.capacity_keys();
    for (int i = 0; i < 3; ++i) { p.qs[i] = c.qs[i]; p.ks[i] = c.ks[i]; p.vs[i] = c.vs[i]; p.os[i] = c.os[i]; }
    p.ls[0] = c.ls[0]; p.ls[1] = c.ls[1];
    p.bts = c.bts;
    p.c = c.scale * 1.4426950408889634f;
    const bool banded = window_left >= 0 || c.softcap > 0.f || c.slopes;
    p.window_left = window_left;
    p.softcap = c.softcap; p.inv_softcap = c.softcap > 0.f ? 1.0f / c.softcap : 0.f;
    p.scale = c.scale;
    p.slopes = c.slopes; p.slope_stride = c.slopes ? c.slope_stride : 0;
    p.kd = c.kd; p.vd = c.vd;
    if (c.descaled()) { p.ds[0] = c.ds[0]; p.ds[1] = c.ds[1]; }
    if (plan.nsplit > 1) {
        if (!c.ws) return FA2_ERR_NULL_POINTER;
        if (!aligned16(c.ws)) return FA2_ERR_ALIGNMENT;
        if (c.ws_bytes < decode_ws_need(c, plan)) return FA2_ERR_BAD_SHAPE;
        p.ws = static_cast<float*>(c.ws);
    }
    const bool bf16 = c.dtype == FA2_DTYPE_BF16;
    hipStream_t const stream = (hipStream_t)c.stream;
    if (banded)
        return c.fp8() ? fa2::launch_decode_band_fp8(bf16, c.D, p, plan.row_tiles, stream) : fa2::launch_decode_band(bf16, c.D, p, plan.row_tiles, stream);
    return c.fp8() ? fa2::launch_decode_fp8(bf16, c.D, p, plan.row_tiles, stream) : fa2::launch_decode(bf16, c.D, p, plan.row_tiles, stream);
}

// ... and the arguments the three entries share, by field name (include/fa2_gfx950.h spells every list out)
#define FA2_DECODE_CALL(c)                                                                                                          \
    FA2_DECODE_SIZES(c);                                                                                                            \
    c.q = q; c.k = k_cache; c.v = v_cache; c.o = o; c.lse = lse; c.lens = cache_seqlens; c.block_table = block_table; c.num_pages = num_pages; \
    c.qs = q_strides; c.ks = k_strides; c.vs = v_strides; c.os = o_strides; c.ls = lse_strides; c.bts = block_table_stride; c.scale = scale;   \
    c.ws = workspace; c.ws_bytes = workspace_bytes; c.stream = hip_stream
#define FA2_DECODE_DESCALES(c) c.kd = k_descale; c.vd = v_descale; c.ds = descale_strides

int fa2_fwd_decode(int dtype, const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const int* cache_seqlens, const int* block_table,
                   int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_pages, const int64_t q_strides[3], const int64_t k_strides[3],
                   const int64_t v_strides[3], const int64_t o_strides[3], const int64_t lse_strides[2], int64_t block_table_stride, float scale,
                   int num_splits, void* workspace, size_t workspace_bytes, void* hip_stream) {
    FA2_DECODE_CALL(c);
    return decode_run(c);
}

// ---- ... on e4m3 caches with per (sequence, K / V head) descales.  The fp8 kernel sweeps the same 32-key tiles under the same split rule, so the plan
// and the workspace are the 16-bit call's (the parts are f32 rows either way).
int fa2_fwd_decode_fp8(int dtype, const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const int* cache_seqlens,
                       const int* block_table, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_pages, const int64_t q_strides[3],
                       const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3], const int64_t lse_strides[2],
                       int64_t block_table_stride, float scale, const float* k_descale, const float* v_descale, const int64_t descale_strides[2],
                       int num_splits, void* workspace, size_t workspace_bytes, void* hip_stream) {
    FA2_DECODE_CALL(c);
    FA2_DECODE_DESCALES(c);
    c.format = FA2_CACHE_E4M3;
    return decode_run(c);
}

// ---- ... with a sliding window, logit soft-capping and ALiBi slopes, on either cache format: the superset entry
int fa2_fwd_decode_window(int dtype, int cache_format, const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const int* cache_seqlens,
                          const int* block_table, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_pages, const int64_t q_strides[3],
                          const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3], const int64_t lse_strides[2],
                          int64_t block_table_stride, float scale, const float* k_descale, const float* v_descale, const int64_t descale_strides[2],
                          int window_left, float softcap, const float* alibi_slopes, int64_t alibi_stride, int num_splits, void* workspace,
                          size_t workspace_bytes, void* hip_stream) {
    FA2_DECODE_CALL(c);
    FA2_DECODE_DESCALES(c);
    c.format = cache_format;
    c.window_left = window_left; c.softcap = softcap; c.slopes = alibi_slopes; c.slope_stride = alibi_stride;
    return decode_run(c);
}

int fa2_fwd_decode_fp8_plan(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits, fa2_decode_plan_t* plan) {
    return fa2_fwd_decode_plan(dtype, B, H, Hkv, Nq, D, capacity, page_size, num_splits, plan);
}

size_t fa2_fwd_decode_fp8_workspace_bytes(int dtype, int B, int H, int Hkv, int Nq, int D, int capacity, int page_size, int num_splits) {
    return fa2_fwd_decode_workspace_bytes(dtype, B, H, Hkv, Nq, D, capacity, page_size, num_splits);
}

// ---- decode attention on a latent (MLA) KV cache: include/fa2_gfx950.h has the contract, csrc/fa2_decode_mla.hip.h the kernel and the arithmetic the
// plan shares with it, decode_mla_hip.cpp the launches.  The cache is a CacheDesc whose k and v are the one latent tensor (Hkv = 1).
struct DecodeMlaCall : CacheDesc {
    int dtype = 0, B = 0, H = 0, Nq = 0, D = 0, Dv = 0;
    const void* q = nullptr;
    void* o = nullptr;
    float* lse = nullptr;
    const int* lens = nullptr;
    const int64_t *qs = nullptr, *os = nullptr, *ls = nullptr;      // {batch, head, row}; ls: {batch, head}
    float scale = 0.f;
    int num_splits = 0;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    void* stream = nullptr;
};

// The sizes of the call, in the documented order (shape, then head dim)
static int decode_mla_check_shape(const DecodeMlaCall& c) {
    if (c.B < 1 || c.H < 1 || c.Nq < 1 || c.D < 1 || c.Dv < 1 || c.H > fa2::kMlaMaxHeads) return FA2_ERR_BAD_SHAPE;
    if ((int64_t)c.Nq * c.H > fa2::kMlaMaxRows || !cache_paging_ok(c) || c.num_splits < 0 || c.num_splits > fa2::kMlaMaxSplit) return FA2_ERR_BAD_SHAPE;
    if (c.D != fa2::kMlaD || c.Dv != fa2::kMlaDv) return FA2_ERR_HEAD_DIM;
    return FA2_OK;
}

// The split: decode_split's reasoning for a workgroup that fills a CU on its own (one per CU: 73 KiB of LDS, more than 256 registers per lane).
// B * row blocks >= CUs: the chip is covered, no split.  Otherwise one workgroup per CU's worth of parts, at most kMlaMaxSplit, and no part shorter
// than kMlaMinPartTiles key tiles of the capacity (csrc/fa2_decode_mla.hip.h has the arithmetic behind both constants).
static int decode_mla_split(int B, int row_blocks, int64_t capacity_tiles, int num_splits) {
    if (num_splits > 0) return num_splits;
    const int64_t work = (int64_t)B * row_blocks, cus = fa2::device_cus();
    if (work >= cus) return 1;
    int64_t S = cus / work;
    if (S > fa2::kMlaMaxSplit) S = fa2::kMlaMaxSplit;
    if (S > capacity_tiles / fa2::kMlaMinPartTiles) S = capacity_tiles / fa2::kMlaMinPartTiles;
    return S < 1 ? 1 : (int)S;
}

static int decode_mla_plan(const DecodeMlaCall& c, fa2_decode_mla_plan_t* plan) {
    if (int rc = decode_mla_check_shape(c)) return rc;
    if (c.dtype != FA2_DTYPE_F16 && c.dtype != FA2_DTYPE_BF16) return FA2_ERR_DTYPE;
    plan->kernel = FA2_KERNEL_HIP_DECODE_MLA;
    plan->row_blocks = fa2::mla_row_blocks(c.Nq * c.H);
    plan->key_tile = fa2::kMlaTile;
    plan->max_split = fa2::kMlaMaxSplit;
    plan->nsplit = decode_mla_split(c.B, plan->row_blocks, (c.capacity_keys() + fa2::kMlaTile - 1) / fa2::kMlaTile, c.num_splits);
    return FA2_OK;
}

// The f32 parts a split call leaves between its two launches: decode's layout with one K / V head
static size_t decode_mla_ws_need(const DecodeMlaCall& c, const fa2_decode_mla_plan_t& plan) {
    return (size_t)fa2::decode_ws_bytes(c.B, plan.nsplit, c.Nq * c.H, fa2::kMlaDv);
}

#define FA2_DECODE_MLA_SIZES(c) \
    DecodeMlaCall c;            \
    c.dtype = dtype; c.B = B; c.H = H; c.Nq = Nq; c.D = D; c.Dv = Dv; c.capacity = capacity; c.page_size = page_size; c.num_splits = num_splits

int fa2_fwd_decode_mla_plan(int dtype, int B, int H, int Nq, int D, int Dv, int capacity, int page_size, int num_splits, fa2_decode_mla_plan_t* plan) {
    if (!plan) return FA2_ERR_NULL_POINTER;
    std::memset(plan, 0, sizeof(*plan));
    FA2_DECODE_MLA_SIZES(c);
    return decode_mla_plan(c, plan);
}

size_t fa2_fwd_decode_mla_workspace_bytes(int dtype, int B, int H, int Nq, int D, int Dv, int capacity, int page_size, int num_splits) {
    fa2_decode_mla_plan_t plan;
    FA2_DECODE_MLA_SIZES(c);
    return decode_mla_plan(c, &plan) ? 0 : decode_mla_ws_need(c, plan);
}

int fa2_decode_mla_part_range(int64_t len, int64_t capacity_keys, int nsplit, int part, int* first_tile, int* ntiles) {
    if (!first_tile || !ntiles) return FA2_ERR_NULL_POINTER;
    if (capacity_keys < 0 || capacity_keys > 0x7fffffffLL - 64 || nsplit < 1 || nsplit > fa2::kMlaMaxSplit || part < 0 || part >= nsplit) return FA2_ERR_BAD_SHAPE;
    fa2::mla_part_range(len, capacity_keys, nsplit, part, first_tile, ntiles);
    return FA2_OK;
}

int fa2_decode_mla_tile(int64_t len, int capacity, int page_size, int tile, int* page_slot, int* row_in_page, int* valid_rows) {
    if (!page_slot || !row_in_page || !valid_rows) return FA2_ERR_NULL_POINTER;
    CacheDesc c;
    c.capacity = capacity; c.page_size = page_size;
    if (!cache_paging_ok(c) || c.capacity_keys() > 0x7fffffffLL - 64) return FA2_ERR_BAD_SHAPE;
    const int64_t cap = c.capacity_keys();
    if (tile < 0 || tile >= (cap + fa2::kMlaTile - 1) / fa2::kMlaTile) return FA2_ERR_BAD_SHAPE;
    const fa2::MlaTile t = fa2::mla_tile(tile, fa2::decode_clamp_len(len, cap), fa2::mla_page_keys(page_size, cap));
    *page_slot = t.slot; *row_in_page = t.row; *valid_rows = t.rows;
    return FA2_OK;
}

static int decode_mla_run(const DecodeMlaCall& c) {
    if (any_null({c.q, c.o, c.lse, c.lens, c.qs, c.os, c.ls}) || cache_null(c)) return FA2_ERR_NULL_POINTER;
    if (int rc = decode_mla_check_shape(c)) return rc;
    if (!cache_extent_ok(c) || c.ls[0] < 0 || c.ls[1] < 0) return FA2_ERR_BAD_SHAPE;
    if (!all_aligned16({c.q, c.o}) || !cache_aligned(c) || ((reinterpret_cast<uintptr_t>(c.lse) | reinterpret_cast<uintptr_t>(c.lens)) & 3u) ||
        !strides3_ok(c.qs) || !strides3_ok(c.os))
        return FA2_ERR_ALIGNMENT;
    fa2_decode_mla_plan_t plan;
    if (int rc = decode_mla_plan(c, &plan)) return rc;                // (the dtype: after the alignment)
    if (!std::isfinite(c.scale)) return FA2_ERR_SCALE;
    if (c.B > 65535) return FA2_ERR_GRID;
    fa2::DecodeParams p;
    std::memset(&p, 0, sizeof(p));
    p.q = c.q; p.k = c.k; p.v = c.k; p.o = c.o; p.lse = c.lse; p.lens = c.lens; p.bt = c.page_size > 0 ? c.block_table : nullptr;
    p.B = c.B; p.H = c.H; p.Hkv = 1; p.Nq = c.Nq; p.G = c.H; p.rows = c.Nq * c.H;
    p.page_size = c.page_size; p.num_pages = c.num_pages; p.nsplit = plan.nsplit;
    p.capacity_keys = c.capacity_keys();
    for (int i = 0; i < 3; ++i) { p.qs[i] = c.qs[i]; p.ks[i] = c.ks[i]; p.vs[i] = c.ks[i]; p.os[i] = c.os[i]; }
    p.ls[0] = c.ls[0]; p.ls[1] = c.ls[1];
    p.bts = c.bts;
    p.c = c.scale * 1.4426950408889634f;
    p.window_left = -1;
    p.scale = c.scale;
    if (plan.nsplit > 1) {
        if (!c.ws) return FA2_ERR_NULL_POINTER;
        if (!aligned16(c.ws)) return FA2_ERR_ALIGNMENT;
        if (c.ws_bytes < decode_mla_ws_need(c, plan)) return FA2_ERR_BAD_SHAPE;
        p.ws = static_cast<float*>(c.ws);
    }
    return fa2::launch_decode_mla(c.dtype == FA2_DTYPE_BF16, p, (hipStream_t)c.stream);
}

int fa2_fwd_decode_mla(int dtype, const void* q, const void* kv_cache, void* o, float* lse, const int* cache_seqlens, const int* block_table, int B, int H,
                       int Nq, int D, int Dv, int capacity, int page_size, int num_pages, const int64_t q_strides[3], const int64_t kv_strides[3],
                       const int64_t o_strides[3], const int64_t lse_strides[2], int64_t block_table_stride, float scale, int num_splits, void* workspace,
                       size_t workspace_bytes, void* hip_stream) {
    FA2_DECODE_MLA_SIZES(c);
    c.q = q; c.k = kv_cache; c.v = kv_cache; c.o = o; c.lse = lse; c.lens = cache_seqlens; c.block_table = block_table; c.num_pages = num_pages;
    c.qs = q_strides; c.ks = kv_strides; c.vs = kv_strides; c.os = o_strides; c.ls = lse_strides; c.bts = block_table_stride; c.scale = scale;
    c.ws = workspace; c.ws_bytes = workspace_bytes; c.stream = hip_stream;
    return decode_mla_run(c);
}

// ---- KV-cache append with rotary embedding and e4m3 quantisation: include/fa2_gfx950.h has the contract, csrc/fa2_kvappend.hip.h the kernel,
// kvappend_hip.cpp its launch.  The checks run in the documented order.
int fa2_kvappend_slot(int64_t len, int64_t capacity_keys, int Nnew, int i, int64_t* pos) {
    if (!pos) return FA2_ERR_NULL_POINTER;
    if (capacity_keys < 0 || Nnew < 1 || i < 0 || i >= Nnew) return FA2_ERR_BAD_SHAPE;
    *pos = fa2::kvappend_slot(len, capacity_keys, Nnew, i);
    return FA2_OK;
}

static int rotary_dim_check(int D, int rotary_dim) { return (rotary_dim < 16 || rotary_dim % 16 != 0 || rotary_dim > D) ? FA2_ERR_HEAD_DIM : FA2_OK; }

int fa2_rotary_eval(int dtype, const void* x, const float* cos_row, const float* sin_row, int D, int rotary_dim, int interleaved, void* y) {
    if (!x || !cos_row || !sin_row || !y) return FA2_ERR_NULL_POINTER;
    if (D < 1) return FA2_ERR_BAD_SHAPE;
    if ((D & 7) || D > kMaxBwdHeadDim) return FA2_ERR_HEAD_DIM;
    if (int rc = rotary_dim_check(D, rotary_dim)) return rc;
    if (dtype != FA2_DTYPE_F16 && dtype != FA2_DTYPE_BF16) return FA2_ERR_DTYPE;
    const bool bf16 = dtype == FA2_DTYPE_BF16;
    const uint16_t* in = static_cast<const uint16_t*>(x);
    uint16_t* out = static_cast<uint16_t*>(y);
    for (int j = rotary_dim; j < D; ++j) out[j] = in[j];                       // bit for bit
    for (int j = 0; j < rotary_dim / 2; ++j) {
        const int c1 = fa2::rotary_col1(j, rotary_dim, interleaved != 0), c2 = fa2::rotary_col2(j, rotary_dim, interleaved != 0);
        float y1, y2;
        fa2::rotary_pair(fa2::rot_io_to_f32(in[c1], bf16), fa2::rot_io_to_f32(in[c2], bf16), cos_row[j], sin_row[j], &y1, &y2);
        out[c1] = fa2::rot_f32_to_io(y1, bf16);
        out[c2] = fa2::rot_f32_to_io(y2, bf16);
    }
    return FA2_OK;
}

// One append call, described: the uniform and the packed entry fill it by field name.  The new tokens' strides are {batch, head, row}; the packed call
// has no batch stride (0) and names its rows by packed token.
struct AppendCall : CacheDesc {
    int dtype = 0, B = 0, Hkv = 0, H = 0, D = 0;
    int Nnew = 0;                                           // the uniform call's; the packed call's sequences take theirs from cu
    const int* cu = nullptr;                                // the packed call's cu_seqlens [B + 1], device
    bool packed = false;
    int64_t groups = 0;                                     // (sequence, token) groups = grid x: B * Nnew, or the packed call's total
    const void *k_new = nullptr, *v_new = nullptr, *q = nullptr;
    void* q_out = nullptr;
    const int* lens = nullptr;
    const int64_t *kns = nullptr, *vns = nullptr, *qs = nullptr, *qos = nullptr;
    const void *cos = nullptr, *sin = nullptr;
    int rotary_dtype = 0, rotary_dim = 0, seqlen_ro = 0, interleaved = 0;
    int64_t ros = 0;
    void* stream = nullptr;
};

static int append_run(const AppendCall& c, bool q_sizes_ok) {
    const bool has_q = c.q || c.q_out, rotary = c.cos || c.sin, fp8 = c.fp8();
    if (any_null({c.k_new, c.v_new, c.lens, c.kns, c.vns}) || (c.packed && !c.cu) || cache_null(c) || (has_q && any_null({c.q, c.q_out, c.qs, c.qos})) ||
        (rotary && (!c.cos || !c.sin)))
        return FA2_ERR_NULL_POINTER;
    if (c.B < 1 || c.Hkv < 1 || (c.packed ? c.groups < 0 : c.Nnew < 1) || c.D < 1 || !cache_paging_ok(c) || !cache_extent_ok(c)) return FA2_ERR_BAD_SHAPE;
    if (has_q && (!rotary || c.H < 1 || c.H % c.Hkv != 0 || !q_sizes_ok)) return FA2_ERR_BAD_SHAPE;          // q rows exist to be rotated
    if (rotary && (c.seqlen_ro < 1 || c.ros < 0)) return FA2_ERR_BAD_SHAPE;
    if ((c.D & (fp8 ? 15 : 7)) || c.D > kMaxBwdHeadDim) return FA2_ERR_HEAD_DIM;
    if (rotary)
        if (int rc = rotary_dim_check(c.D, c.rotary_dim)) return rc;
    const bool tab32 = c.rotary_dtype == FA2_DTYPE_F32;
    if (!all_aligned16({c.k_new, c.v_new, c.q, c.q_out, c.cos, c.sin}) || !cache_aligned(c) ||
        ((reinterpret_cast<uintptr_t>(c.lens) | reinterpret_cast<uintptr_t>(c.cu)) & 3u) || !strides3_ok(c.kns) || !strides3_ok(c.vns) ||
        (has_q && (!strides3_ok(c.qs) || !strides3_ok(c.qos))) || (rotary && c.ros % (tab32 ? 4 : 8) != 0))      // a table row starts on a 16-byte boundary
        return FA2_ERR_ALIGNMENT;
    if ((c.dtype != FA2_DTYPE_F16 && c.dtype != FA2_DTYPE_BF16) || !cache_format_ok(c) || (rotary && !tab32 && c.rotary_dtype != c.dtype)) return FA2_ERR_DTYPE;
    fa2::KvAppendVarlenParams p;
    std::memset(&p, 0, sizeof(p));
    p.k_new = c.k_new; p.v_new = c.v_new; p.k_cache = const_cast<void*>(c.k); p.v_cache = const_cast<void*>(c.v); p.q = c.q; p.q_out = c.q_out;
    p.cos = c.cos; p.sin = c.sin; p.lens = c.lens; p.bt = c.page_size > 0 ? c.block_table : nullptr; p.kd = c.kd; p.vd = c.vd;
    p.B = c.B; p.Hkv = c.Hkv; p.H = has_q ? c.H : 0; p.Nnew = c.Nnew; p.D = c.D;
    p.rot = rotary ? c.rotary_dim : 0; p.interleaved = c.interleaved != 0; p.tab16 = !tab32;
    p.page_size = c.page_size; p.num_pages = c.num_pages;
    p.R = 2 * c.Hkv + p.H; p.UR = (c.D + 15) / 16;
    p.capacity_keys = c.capacity_keys();
    p.seqlen_ro = rotary ? c.seqlen_ro : 1;
    for (int i = 0; i < 3; ++i) {
        p.kns[i] = c.kns[i]; p.vns[i] = c.vns[i]; p.ks[i] = c.ks[i]; p.vs[i] = c.vs[i];
        if (has_q) { p.qs[i] = c.qs[i]; p.qos[i] = c.qos[i]; }
    }
    p.bts = c.bts; p.ros = c.ros;
    if (c.descaled()) { p.ds[0] = c.ds[0]; p.ds[1] = c.ds[1]; }
    p.cu = c.cu;
    if (c.groups > 0x7fffffffLL || ((int64_t)p.R * p.UR + fa2::kAppendThreads - 1) / fa2::kAppendThreads > 65535) return FA2_ERR_GRID;
    const bool bf16 = c.dtype == FA2_DTYPE_BF16;
    hipStream_t const stream = (hipStream_t)c.stream;
    if (c.packed) {
        if (c.groups == 0) return FA2_OK;                    // an empty token buffer: nothing to launch
        return fp8 ? fa2::launch_kvappend_varlen_fp8(bf16, p, c.groups, stream) : fa2::launch_kvappend_varlen(bf16, p, c.groups, stream);
    }
    return fp8 ? fa2::launch_kvappend_fp8(bf16, p, stream) : fa2::launch_kvappend(bf16, p, stream);
}

int fa2_kvcache_append(int dtype, int cache_format, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_seqlens,
                       const int* block_table, int B, int Hkv, int Nnew, int D, int capacity, int page_size, int num_pages, const int64_t k_new_strides[3],
                       const int64_t v_new_strides[3], const int64_t k_strides[3], const int64_t v_strides[3], int64_t block_table_stride, const void* q,
                       void* q_out, int H, int Nq, const int64_t q_strides[3], const int64_t q_out_strides[3], const void* rotary_cos,
                       const void* rotary_sin, int rotary_dtype, int rotary_dim, int seqlen_ro, int64_t rotary_row_stride, int rotary_interleaved,
                       const float* k_descale, const float* v_descale, const int64_t descale_strides[2], void* hip_stream) {
    AppendCall c;
    c.k = k_cache; c.v = v_cache; c.block_table = block_table; c.capacity = capacity; c.page_size = page_size; c.num_pages = num_pages;
    c.ks = k_strides; c.vs = v_strides; c.bts = block_table_stride; c.format = cache_format; c.kd = k_descale; c.vd = v_descale; c.ds = descale_strides;
    c.dtype = dtype; c.B = B; c.Hkv = Hkv; c.H = H; c.D = D; c.Nnew = Nnew; c.groups = (int64_t)B * Nnew;
    c.k_new = k_new; c.v_new = v_new; c.q = q; c.q_out = q_out; c.lens = cache_seqlens;
    c.kns = k_new_strides; c.vns = v_new_strides; c.qs = q_strides; c.qos = q_out_strides;
    c.cos = rotary_cos; c.sin = rotary_sin; c.rotary_dtype = rotary_dtype; c.rotary_dim = rotary_dim; c.seqlen_ro = seqlen_ro; c.ros = rotary_row_stride;
    c.interleaved = rotary_interleaved; c.stream = hip_stream;
    return append_run(c, Nq == Nnew);
}

// ... its packed (ragged) form: the new tokens are [total, heads, D], strides {head, row} as the packed attention calls take them
int fa2_kvappend_varlen_token(const int* cu_seqlens, int B, int64_t t, int* seq, int* i, int* nnew) {
    if (!cu_seqlens || !seq || !i || !nnew) return FA2_ERR_NULL_POINTER;
    if (B < 1) return FA2_ERR_BAD_SHAPE;
    if (!fa2::kvappend_varlen_token(cu_seqlens, B, t, seq, i, nnew)) { *seq = -1; *i = 0; *nnew = 0; }
    return FA2_OK;
}

int fa2_kvcache_append_varlen(int dtype, int cache_format, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cu_seqlens,
                              const int* cache_seqlens, const int* block_table, int B, int64_t total, int Hkv, int D, int capacity, int page_size,
                              int num_pages, const int64_t k_new_strides[2], const int64_t v_new_strides[2], const int64_t k_strides[3],
                              const int64_t v_strides[3], int64_t block_table_stride, const void* q, void* q_out, int H, const int64_t q_strides[2],
                              const int64_t q_out_strides[2], const void* rotary_cos, const void* rotary_sin, int rotary_dtype, int rotary_dim, int seqlen_ro,
                              int64_t rotary_row_stride, int rotary_interleaved, const float* k_descale, const float* v_descale,
                              const int64_t descale_strides[2], void* hip_stream) {
    AppendCall c;
    c.k = k_cache; c.v = v_cache; c.block_table = block_table; c.capacity = capacity; c.page_size = page_size; c.num_pages = num_pages;
    c.ks = k_strides; c.vs = v_strides; c.bts = block_table_stride; c.format = cache_format; c.kd = k_descale; c.vd = v_descale; c.ds = descale_strides;
    c.dtype = dtype; c.B = B; c.Hkv = Hkv; c.H = H; c.D = D; c.packed = true; c.cu = cu_seqlens; c.groups = total;
    c.k_new = k_new; c.v_new = v_new; c.q = q; c.q_out = q_out; c.lens = cache_seqlens;
    int64_t st[4][3] = {};
    const int64_t* in[4] = {k_new_strides, v_new_strides, q_strides, q_out_strides};
    const int64_t** out[4] = {&c.kns, &c.vns, &c.qs, &c.qos};
    for (int j = 0; j < 4; ++j)
        if (in[j]) { st[j][1] = in[j][0]; st[j][2] = in[j][1]; *out[j] = st[j]; }
    c.cos = rotary_cos; c.sin = rotary_sin; c.rotary_dtype = rotary_dtype; c.rotary_dim = rotary_dim; c.seqlen_ro = seqlen_ro; c.ros = rotary_row_stride;
    c.interleaved = rotary_interleaved; c.stream = hip_stream;
    return append_run(c, true);
}

// ---- the append for a latent (MLA) cache: include/fa2_gfx950.h has the contract, csrc/fa2_kvappend_mla.hip.h the kernels, kvappend_mla_hip.cpp their
// launch.  The call is an AppendCall whose "K" source is kv_c and whose "V" source is k_pe (Hkv = 1, no head stride), both caches the one latent tensor,
// in the 16-bit format; the checks run in append_run's order and classes.
int fa2_kvappend_mla_chunks(int unit, int halves, int* chunk_a, int* chunk_b) {
    if (!chunk_a || !chunk_b) return FA2_ERR_NULL_POINTER;
    if (unit < 0 || unit >= fa2::kMlaUnits) return FA2_ERR_BAD_SHAPE;
    fa2::mla_append_chunks(unit, halves != 0, chunk_a, chunk_b);
    return FA2_OK;
}

static int append_mla_run(const AppendCall& c, int Dv, bool q_sizes_ok) {
    const bool has_q = c.q || c.q_out, rotary = c.cos || c.sin;
    if (any_null({c.k_new, c.v_new, c.lens, c.kns, c.vns}) || (c.packed && !c.cu) || cache_null(c) || (has_q && any_null({c.q, c.q_out, c.qs, c.qos})) ||
        (rotary && (!c.cos || !c.sin)))
        return FA2_ERR_NULL_POINTER;
    if (c.B < 1 || (c.packed ? c.groups < 0 : c.Nnew < 1) || c.D < 1 || Dv < 1 || !cache_paging_ok(c) || !cache_extent_ok(c)) return FA2_ERR_BAD_SHAPE;
    if (has_q && (!rotary || c.H < 1 || c.H > fa2::kMlaMaxHeads || !q_sizes_ok)) return FA2_ERR_BAD_SHAPE;      // q rows exist to be rotated
    if (rotary && (c.seqlen_ro < 1 || c.ros < 0)) return FA2_ERR_BAD_SHAPE;
    if (c.D != fa2::kMlaD || Dv != fa2::kMlaDv || (rotary && c.rotary_dim != fa2::kMlaRot)) return FA2_ERR_HEAD_DIM;
    const bool tab32 = c.rotary_dtype == FA2_DTYPE_F32;
    if (!all_aligned16({c.k_new, c.v_new, c.q, c.q_out, c.cos, c.sin}) || !cache_aligned(c) ||
        ((reinterpret_cast<uintptr_t>(c.lens) | reinterpret_cast<uintptr_t>(c.cu)) & 3u) || !strides3_ok(c.kns) || !strides3_ok(c.vns) ||
        (has_q && (!strides3_ok(c.qs) || !strides3_ok(c.qos))) || (rotary && c.ros % (tab32 ? 4 : 8) != 0))
        return FA2_ERR_ALIGNMENT;
    if ((c.dtype != FA2_DTYPE_F16 && c.dtype != FA2_DTYPE_BF16) || (rotary && !tab32 && c.rotary_dtype != c.dtype)) return FA2_ERR_DTYPE;
    if (c.groups > 0x7fffffffLL) return FA2_ERR_GRID;               // (blockIdx.y: at most 129 rows of 36 units)
    if (c.packed && c.groups == 0) return FA2_OK;                   // an empty token buffer: nothing to launch
    fa2::KvAppendMlaParams p;
    std::memset(&p, 0, sizeof(p));
    p.kv_c = c.k_new; p.k_pe = c.v_new; p.kv_cache = const_cast<void*>(c.k); p.q = c.q; p.q_out = c.q_out;
    p.cos = c.cos; p.sin = c.sin; p.lens = c.lens; p.bt = c.page_size > 0 ? c.block_table : nullptr; p.cu = c.cu;
    p.B = c.B; p.H = has_q ? c.H : 0; p.Nnew = c.Nnew;
    p.interleaved = c.interleaved != 0; p.tab16 = !tab32;
    p.page_size = c.page_size; p.num_pages = c.num_pages;
    p.R = 1 + p.H;
    p.capacity_keys = c.capacity_keys();
    p.seqlen_ro = rotary ? c.seqlen_ro : 1;
    p.cs[0] = c.kns[0]; p.cs[1] = c.kns[2]; p.ps[0] = c.vns[0]; p.ps[1] = c.vns[2];
    for (int i = 0; i < 3; ++i) {
        p.ks[i] = c.ks[i];
        if (has_q) { p.qs[i] = c.qs[i]; p.qos[i] = c.qos[i]; }
    }
    p.bts = c.bts; p.ros = c.ros;
    return fa2::launch_kvappend_mla(c.dtype == FA2_DTYPE_BF16, p, c.groups, c.packed, (hipStream_t)c.stream);
}

// what the two entries fill alike: the cache (K and V the one latent tensor), the tables, the lengths
#define FA2_APPEND_MLA_COMMON(c)                                                                                                              \
    AppendCall c;                                                                                                                             \
    c.k = kv_cache; c.v = kv_cache; c.block_table = block_table; c.capacity = capacity; c.page_size = page_size; c.num_pages = num_pages;     \
    c.ks = kv_strides; c.vs = kv_strides; c.bts = block_table_stride; c.dtype = dtype; c.B = B; c.Hkv = 1; c.H = H; c.D = D;                  \
    c.k_new = kv_c; c.v_new = k_pe; c.q = q; c.q_out = q_out; c.lens = cache_seqlens;                                                         \
    c.cos = rotary_cos; c.sin = rotary_sin; c.rotary_dtype = rotary_dtype; c.rotary_dim = rotary_dim; c.seqlen_ro = seqlen_ro;                \
    c.ros = rotary_row_stride; c.interleaved = rotary_interleaved; c.stream = hip_stream

int fa2_kvcache_append_mla(int dtype, const void* kv_c, const void* k_pe, void* kv_cache, const int* cache_seqlens, const int* block_table, int B, int Nnew,
                           int D, int Dv, int capacity, int page_size, int num_pages, const int64_t kv_c_strides[2], const int64_t k_pe_strides[2],
                           const int64_t kv_strides[3], int64_t block_table_stride, const void* q, void* q_out, int H, int Nq, const int64_t q_strides[3],
                           const int64_t q_out_strides[3], const void* rotary_cos, const void* rotary_sin, int rotary_dtype, int rotary_dim, int seqlen_ro,
                           int64_t rotary_row_stride, int rotary_interleaved, void* hip_stream) {
    FA2_APPEND_MLA_COMMON(c);
    c.Nnew = Nnew; c.groups = (int64_t)B * Nnew; c.qs = q_strides; c.qos = q_out_strides;
    int64_t st[2][3] = {};                                   // {batch, row} -> {batch, head (none), row}
    if (kv_c_strides) { st[0][0] = kv_c_strides[0]; st[0][2] = kv_c_strides[1]; c.kns = st[0]; }
    if (k_pe_strides) { st[1][0] = k_pe_strides[0]; st[1][2] = k_pe_strides[1]; c.vns = st[1]; }
    return append_mla_run(c, Dv, Nq == Nnew);
}

// ... its packed (ragged) form: kv_c / k_pe are [total, 512] / [total, 64] with a row stride each, q and q_out [total, H, 576] with {head, row}
int fa2_kvcache_append_mla_varlen(int dtype, const void* kv_c, const void* k_pe, void* kv_cache, const int* cu_seqlens, const int* cache_seqlens,
                                  const int* block_table, int B, int64_t total, int D, int Dv, int capacity, int page_size, int num_pages,
                                  const int64_t kv_c_strides[1], const int64_t k_pe_strides[1], const int64_t kv_strides[3], int64_t block_table_stride,
                                  const void* q, void* q_out, int H, const int64_t q_strides[2], const int64_t q_out_strides[2], const void* rotary_cos,
                                  const void* rotary_sin, int rotary_dtype, int rotary_dim, int seqlen_ro, int64_t rotary_row_stride, int rotary_interleaved,
                                  void* hip_stream) {
    FA2_APPEND_MLA_COMMON(c);
    c.packed = true; c.cu = cu_seqlens; c.groups = total;
    int64_t st[4][3] = {};
    if (kv_c_strides) { st[0][2] = kv_c_strides[0]; c.kns = st[0]; }
    if (k_pe_strides) { st[1][2] = k_pe_strides[0]; c.vns = st[1]; }
    if (q_strides) { st[2][1] = q_strides[0]; st[2][2] = q_strides[1]; c.qs = st[2]; }
    if (q_out_strides) { st[3][1] = q_out_strides[0]; st[3][2] = q_out_strides[1]; c.qos = st[3]; }
    return append_mla_run(c, Dv, true);
}

// ---- chunked prefill against a KV cache: include/fa2_gfx950.h has the contract, csrc/fa2_prefill.h the tile arithmetic, prefill_hip.cpp /
// prefill_scoremod_hip.cpp the kernels (the FA2_PAGED forms of the packed forward).  One call, described: the entry fills it by field name, the plan
// query the sizes alone.  The checks run in decode's class order.  fa2_fwd_prefill_fp8 (prefill_fp8_hip.cpp, prefill_fp8_scoremod_hip.cpp: the KV8 forms) is
// the same call with the cache format its entry serves: an e4m3 cache's strides count bytes, its head dims are multiples of 16 up to the largest compiled
// one, and its descales are checked where decode's are (CacheDesc).
struct PrefillCall : CacheDesc {
    int serves = FA2_CACHE_16BIT;                    // the cache format of the entry: any other stated format is FA2_ERR_DTYPE
    bool kv8() const { return serves == FA2_CACHE_E4M3; }
    int dtype = 0, B = 0, H = 0, Hkv = 0, max_q = 0, D = 0;
    const void* q = nullptr;
    void* o = nullptr;
    float* lse = nullptr;
    const int *cu_q = nullptr, *lens = nullptr;
    const int64_t *qs = nullptr, *os = nullptr;      // {head, row}
    int64_t lse_stride = 0;
    float scale = 0.f;
    int window_left = -1;
    float softcap = 0.f;
    const float* slopes = nullptr;
    int64_t slope_stride = 0;
    void* stream = nullptr;
};

// The sizes of a prefill call (shape, then head dim); *HD: the kernel head dim.
static int prefill_check_shape(const PrefillCall& c, int* HD) {
    if (c.B < 1 || c.H < 1 || c.Hkv < 1 || c.max_q < 1 || c.D < 1 || c.Hkv > c.H || c.H % c.Hkv != 0 || !cache_paging_ok(c)) return FA2_ERR_BAD_SHAPE;
    if (c.capacity_keys() > 0x7fffffffLL - 64 || c.window_left < -1) return FA2_ERR_BAD_SHAPE;
    // a sequence's offset len_s - Nq_s lies in [-max_seqlen_q, capacity_keys]
    const int cap = (int)c.capacity_keys(), n = c.max_q > cap ? c.max_q : cap;
    if (!fa2::window_args_ok(c.max_q, cap, c.window_left, 0, -n, true)) return FA2_ERR_BAD_SHAPE;
    *HD = fa2_padded_head_dim(c.D);
    if (*HD < 0 || (c.D & (c.kv8() ? 15 : 7)) || (c.kv8() && *HD > fa2::kPrefillFp8MaxHD)) return FA2_ERR_HEAD_DIM;
    return FA2_OK;
}

// rows per workgroup: the packed call's heuristic on (B, H, max_seqlen_q) and option "rows"; 128 above head dim 128 (fa2_family_unit.h)
static int prefill_rows(const PrefillCall& c, int HD) {
    fa2::FwdParams p{};
    p.nbh = c.B * c.H; p.Nq = c.max_q; p.D = c.D;
    return HD > 128 ? 128 : pick_rows(p);
}

static int prefill_plan(int serves, int dtype, int B, int H, int Hkv, int max_seqlen_q, int D, int capacity, int page_size, fa2_fwd_plan_t* plan) {
    if (!plan) return FA2_ERR_NULL_POINTER;
    std::memset(plan, 0, sizeof(*plan));
    PrefillCall c;
    c.serves = serves;
    c.dtype = dtype; c.B = B; c.H = H; c.Hkv = Hkv; c.max_q = max_seqlen_q; c.D = D; c.capacity = capacity; c.page_size = page_size;
    int HD = 0;
    if (int rc = prefill_check_shape(c, &HD)) return rc;
    if (dtype != FA2_DTYPE_F16 && dtype != FA2_DTYPE_BF16) return FA2_ERR_DTYPE;
    if ((int64_t)B * H * ((max_seqlen_q + 127) / 128) > 0x7fffffffLL) return FA2_ERR_GRID;
    plan->kernel = FA2_KERNEL_HIP_PREFILL;
    plan->contract = 0;
    plan->rows = prefill_rows(c, HD);
    plan->heads_main = B * H;
    return FA2_OK;
}

int fa2_fwd_prefill_plan(int dtype, int B, int H, int Hkv, int max_seqlen_q, int D, int capacity, int page_size, fa2_fwd_plan_t* plan) {
    return prefill_plan(FA2_CACHE_16BIT, dtype, B, H, Hkv, max_seqlen_q, D, capacity, page_size, plan);
}

int fa2_fwd_prefill_fp8_plan(int dtype, int B, int H, int Hkv, int max_seqlen_q, int D, int capacity, int page_size, fa2_fwd_plan_t* plan) {
    return prefill_plan(FA2_CACHE_E4M3, dtype, B, H, Hkv, max_seqlen_q, D, capacity, page_size, plan);
}

int fa2_prefill_tile(int64_t len, int capacity, int page_size, int tile, int* page_slot, int* row_in_page, int* valid_rows) {
    if (!page_slot || !row_in_page || !valid_rows) return FA2_ERR_NULL_POINTER;
    CacheDesc c;
    c.capacity = capacity; c.page_size = page_size;
    if (!cache_paging_ok(c) || c.capacity_keys() > 0x7fffffffLL - 64) return FA2_ERR_BAD_SHAPE;
    const int64_t cap = c.capacity_keys();
    if (tile < 0 || tile >= (cap + fa2::kPrefillTile - 1) / fa2::kPrefillTile) return FA2_ERR_BAD_SHAPE;
    const fa2::PrefillTile t = fa2::prefill_tile(tile, fa2::prefill_clamp_len(len, cap), fa2::prefill_page_keys(page_size, cap));
    *page_slot = t.slot; *row_in_page = t.row; *valid_rows = t.rows;
    return FA2_OK;
}

static int prefill_run(const PrefillCall& c) {
    if (any_null({c.q, c.o, c.lse, c.cu_q, c.lens, c.qs, c.os}) || cache_null(c)) return FA2_ERR_NULL_POINTER;
    int HD = 0;
    // one tile's rows must stay below the byte offset that stands for "out of range" (kOobOffset), whatever else the pool spans
    const int64_t es = c.kv8() ? 1 : 2;              // bytes per cache element
    const auto tile_ok = [es](const int64_t* s) { return s[2] <= 0 || (int64_t)fa2::kKvTile * s[2] * es < (int64_t)fa2::kOobOffset; };
    if (c.lse_stride < 0 || c.slope_stride < 0 || !cache_extent_ok(c) || !tile_ok(c.ks) || !tile_ok(c.vs)) return FA2_ERR_BAD_SHAPE;
    if (int rc = prefill_check_shape(c, &HD)) return rc;
    const auto strides2_ok = [](const int64_t* s) { return s[0] % 8 == 0 && s[1] % 8 == 0 && s[1] > 0; };
    if (!all_aligned16({c.q, c.o}) || !cache_aligned(c) ||
        ((reinterpret_cast<uintptr_t>(c.lse) | reinterpret_cast<uintptr_t>(c.cu_q) | reinterpret_cast<uintptr_t>(c.lens) |
          reinterpret_cast<uintptr_t>(c.slopes)) & 3u) || !strides2_ok(c.qs) || !strides2_ok(c.os))
        return FA2_ERR_ALIGNMENT;
    if ((c.dtype != FA2_DTYPE_F16 && c.dtype != FA2_DTYPE_BF16) || c.format != c.serves || !cache_format_ok(c)) return FA2_ERR_DTYPE;
    if (!std::isfinite(c.scale)) return FA2_ERR_SCALE;
    if (!fa2::softcap_ok(c.softcap)) return FA2_ERR_SOFTCAP;
    if ((int64_t)c.B * c.H * ((c.max_q + 127) / 128) > 0x7fffffffLL) return FA2_ERR_GRID;

    fa2::FwdParams p{};
    const bool paged = c.page_size > 0;
    const int64_t cap = c.capacity_keys();
    p.q = c.q; p.k = c.k; p.v = c.v; p.o = c.o; p.lse = c.lse;
    p.B = c.B; p.H = c.H; p.Nq = c.max_q; p.Nkv = (int)cap; p.D = c.D;
    p.qs[0] = 0; p.qs[1] = c.qs[0]; p.qs[2] = c.qs[1];
    p.os[0] = 0; p.os[1] = c.os[0]; p.os[2] = c.os[1];
    for (int i = 0; i < 3; ++i) { p.ks[i] = c.ks[i]; p.vs[i] = c.vs[i]; }      // [0]: the page (contiguous: batch) stride, read by the PAGED kernels as such
    p.ls[0] = 0; p.ls[1] = c.lse_stride;
    p.c = std::fabs(c.scale) * 1.4426950408889634f;
    if (p.c < 1e-30f) p.c = 1e-30f;                  // (scale == 0: fwd_validate has the reason)
    p.negate_q = c.scale < 0.f;
    p.nqblk = (c.max_q + kFwdRows - 1) / kFwdRows;
    p.nbh = c.B * c.H;
    p.exact_scale = 1;
    p.persist = 1;
    p.kv_group = c.H / c.Hkv;
    fa2::Window w;
    w.left = c.window_left; w.right = 0; w.off = 1;   // decode's mask: causal, bottom-right (the kernels take the offset per sequence)
    fa2::set_window(p, w);
    fa2::set_varlen(p, c.cu_q, (const int*)nullptr);
    fa2::PagedKv pg;
    pg.lens = c.lens;
    pg.bt = paged ? c.block_table : nullptr;
    pg.bts = paged ? c.bts : 0;
    pg.page_keys = fa2::prefill_page_keys(c.page_size, cap);
    pg.num_pages = paged ? c.num_pages : c.B;         // contiguous: page id = the sequence
    pg.capacity_keys = (int)cap;
    const int rows = prefill_rows(c, HD);
    const bool bf16 = c.dtype == FA2_DTYPE_BF16;
    hipStream_t const stream = (hipStream_t)c.stream;
    if (c.kv8()) {
        fa2::KvDescale kvd;
        kvd.k = c.kd; kvd.v = c.vd;
        if (c.descaled()) { kvd.s[0] = c.ds[0]; kvd.s[1] = c.ds[1]; }
        if (c.softcap > 0.f || c.slopes)
            return fa2::launch_fwd_prefill_fp8_scoremod(bf16, HD, p, rows, stream, pg, kvd,
                                                        fa2::make_scoremod(c.softcap, c.scale, c.slopes, c.slopes ? c.slope_stride : 0));
        return fa2::launch_fwd_prefill_fp8(bf16, HD, p, rows, stream, pg, kvd);
    }
    if (c.softcap > 0.f || c.slopes)
        return fa2::launch_fwd_prefill_scoremod(bf16, HD, p, rows, stream, pg, fa2::make_scoremod(c.softcap, c.scale, c.slopes, c.slopes ? c.slope_stride : 0));
    return fa2::launch_fwd_prefill(bf16, HD, p, rows, stream, pg);
}

int fa2_fwd_prefill(int dtype, int cache_format, const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const int* cu_seqlens_q,
                    const int* cache_seqlens, const int* block_table, int B, int H, int Hkv, int max_seqlen_q, int D, int capacity, int page_size,
                    int num_pages, const int64_t q_strides[2], const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[2],
                    int64_t lse_stride, int64_t block_table_stride, float scale, int window_left, float softcap, const float* alibi_slopes,
                    int64_t alibi_stride, void* hip_stream) {
    PrefillCall c;
    c.dtype = dtype; c.format = cache_format; c.B = B; c.H = H; c.Hkv = Hkv; c.max_q = max_seqlen_q; c.D = D;
    c.capacity = capacity; c.page_size = page_size; c.num_pages = num_pages;
    c.q = q; c.k = k_cache; c.v = v_cache; c.o = o; c.lse = lse; c.cu_q = cu_seqlens_q; c.lens = cache_seqlens; c.block_table = block_table;
    c.qs = q_strides; c.ks = k_strides; c.vs = v_strides; c.os = o_strides; c.lse_stride = lse_stride; c.bts = block_table_stride;
    c.scale = scale; c.window_left = window_left; c.softcap = softcap; c.slopes = alibi_slopes; c.slope_stride = alibi_stride; c.stream = hip_stream;
    return prefill_run(c);
}

int fa2_fwd_prefill_fp8(int dtype, const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const int* cu_seqlens_q,
                        const int* cache_seqlens, const int* block_table, int B, int H, int Hkv, int max_seqlen_q, int D, int capacity, int page_size,
                        int num_pages, const int64_t q_strides[2], const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[2],
                        int64_t lse_stride, int64_t block_table_stride, float scale, const float* k_descale, const float* v_descale,
                        const int64_t descale_strides[2], int window_left, float softcap, const float* alibi_slopes, int64_t alibi_stride,
                        void* hip_stream) {
    PrefillCall c;
    c.serves = c.format = FA2_CACHE_E4M3;
    c.dtype = dtype; c.B = B; c.H = H; c.Hkv = Hkv; c.max_q = max_seqlen_q; c.D = D;
    c.capacity = capacity; c.page_size = page_size; c.num_pages = num_pages;
    c.q = q; c.k = k_cache; c.v = v_cache; c.o = o; c.lse = lse; c.cu_q = cu_seqlens_q; c.lens = cache_seqlens; c.block_table = block_table;
    c.qs = q_strides; c.ks = k_strides; c.vs = v_strides; c.os = o_strides; c.lse_stride = lse_stride; c.bts = block_table_stride;
    c.kd = k_descale; c.vd = v_descale; c.ds = descale_strides;
    c.scale = scale; c.window_left = window_left; c.softcap = softcap; c.slopes = alibi_slopes; c.slope_stride = alibi_stride; c.stream = hip_stream;
    return prefill_run(c);
}

int fa2_fwd_f16(FA2_FWD_ARGS(), void* hip_stream) { return fa2_fwd(FA2_DTYPE_F16, FA2_FWD_PASS, hip_stream); }
int fa2_fwd_bf16(FA2_FWD_ARGS(), void* hip_stream) { return fa2_fwd(FA2_DTYPE_BF16, FA2_FWD_PASS, hip_stream); }
int fa2_bwd_f16(FA2_BWD_ARGS(), void* hip_stream) { return fa2_bwd(FA2_DTYPE_F16, FA2_BWD_PASS, hip_stream); }
int fa2_bwd_bf16(FA2_BWD_ARGS(), void* hip_stream) { return fa2_bwd(FA2_DTYPE_BF16, FA2_BWD_PASS, hip_stream); }

}  // extern "C"
