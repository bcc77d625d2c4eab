// kvappend_mla_fp8_sanitize.cpp — the addressing of the quantising latent-cache append (csrc/fa2_kvappend_mla_fp8.hip.h: mla_fp8_append_row, the one
// function both kernels call for a token's source rows and its 656-byte cache row, and mla_fp8_append_tail for the rotary units; the q units through
// the 16-bit kernel's mla_append_unit, as the kernels take them) as a stand-alone host program for AddressSanitizer and UBSan:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I flash-attention-v2-rdna3-minimal_amd/csrc -I include \
//         tools/kvappend_mla_fp8_sanitize.cpp -o /tmp/kvappend_mla_fp8_sanitize && /tmp/kvappend_mla_fp8_sanitize
//
// 4 000 calls, uniform and packed, contiguous and paged, with and without q and tables, on heap blocks sized to the BYTE: kv_c, k_pe, q, q_out, the byte
// cache (rows * 656 bytes: a row outside it is a report), the tables, the lengths, the block table and cu_seqlens — hostile as in
// tools/kvappend_mla_sanitize.cpp.  The walk is the kernel's: every group, every lane of the launch grid.  Lanes 0 .. 63 of slice 0 read their 16-byte
// chunk of kv_c and write their 8 code bytes, lane 0 the 16 scale bytes, lanes 32 .. 35 move their two chunks of k_pe (and read the 8 table entries of
// either table they would); lanes >= 36 are the q units.  Checked besides what the sanitizers see: a cache row is written in all 656 bytes or in none
// (as often in each) and is the row kvappend_slot and the block table name; every chunk of q_out is written exactly once.
// Prints "ok: <calls> calls, <lanes> lanes"; exit status 1 and the case on a wrong walk.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "fa2_kvappend_mla_fp8.hip.h"

using fa2::KvAppendMlaParams;

template <class T>
static T* block(size_t n) { return n ? new T[n]() : new T[1](); }

int main() {
    std::mt19937_64 g(20254);
    const int ROW = fa2::kMlaFp8RowBytes;
    long calls = 0, lanes = 0;
    for (int trial = 0; trial < 4000; ++trial) {
        const bool packed = trial & 1, paged = trial & 2, has_tab = (trial & 12) != 0, has_q = has_tab && (trial & 4), tab16 = trial & 16;
        const int B = 1 + (int)(g() % 4), H = has_q ? 1 + (int)(g() % (trial % 7 == 0 ? 128 : 9)) : 0;
        const int page_size = paged ? 64 * (1 + (int)(g() % 2)) : 0;
        const int capacity = paged ? 1 + (int)(g() % 4) : 1 + (int)(g() % 200);
        const int num_pages = paged ? 1 + (int)(g() % 6) : 0;
        const int64_t capacity_keys = paged ? (int64_t)capacity * page_size : capacity;
        const int64_t cache_rows = paged ? (int64_t)num_pages * page_size : (int64_t)B * capacity;
        const int seqlen_ro = 1 + (int)(g() % 40);
        const int Nnew = 1 + (int)(g() % (trial % 5 == 0 && H <= 9 ? 140 : 6));
        std::vector<int> cu(B + 1, 0);
        int64_t total = (int64_t)B * Nnew;
        if (packed) {
            for (int s = 0; s < B; ++s) cu[s + 1] = cu[s] + (int)(g() % 5) * (int)(g() % 3);
            total = cu[B] + (int)(g() % 3);
            if (trial % 8 == 5) for (int& x : cu) x = (g() % 3) ? (int)(g() % 30) - 5 : (int)(uint32_t)g();
            if (total == 0) total = 1;
        }
        uint16_t* kv_c = block<uint16_t>((size_t)total * fa2::kMlaDv);
        uint16_t* k_pe = block<uint16_t>((size_t)total * fa2::kMlaRot);
        char* cache = block<char>((size_t)cache_rows * ROW);
        uint16_t* q = has_q ? block<uint16_t>((size_t)total * H * fa2::kMlaD) : nullptr;
        uint16_t* q_out = has_q ? block<uint16_t>((size_t)total * H * fa2::kMlaD) : nullptr;
        const size_t esz = tab16 ? 2 : 4, tab_bytes = (size_t)seqlen_ro * 32 * esz;
        unsigned char* cosb = has_tab ? block<unsigned char>(tab_bytes) : nullptr;
        unsigned char* sinb = has_tab ? block<unsigned char>(tab_bytes) : nullptr;
        int* lens = block<int>(B);
        int* bt = block<int>(paged ? (size_t)B * capacity : 1);
        int* cud = block<int>(B + 1);
        for (int s = 0; s <= B; ++s) cud[s] = cu[s];
        for (int s = 0; s < B; ++s) {
            switch ((trial / 2 + s) % 4) {
                case 0: lens[s] = (int)(uint32_t)g(); break;
                case 1: lens[s] = (int)(g() % 300) - 5; break;
                case 2: lens[s] = (int)(capacity_keys + (int64_t)(g() % 300) - 150); break;
                default: lens[s] = (g() & 1) ? INT_MAX : INT_MIN; break;
            }
        }
        if (paged) for (int j = 0; j < B * capacity; ++j) bt[j] = (g() % 3) ? (int)(g() % (uint64_t)(num_pages + 1)) - (int)(g() % 2) : (int)(uint32_t)g();

        KvAppendMlaParams p;
        std::memset(&p, 0, sizeof(p));
        p.kv_c = kv_c; p.k_pe = k_pe; p.kv_cache = cache; p.q = q; p.q_out = q_out; p.cos = cosb; p.sin = sinb; p.lens = lens; p.bt = paged ? bt : nullptr;
        p.cu = cud; p.B = B; p.H = H; p.Nnew = Nnew; p.interleaved = (trial >> 5) & 1; p.tab16 = tab16;
        p.page_size = page_size; p.num_pages = num_pages; p.R = 1 + H; p.capacity_keys = capacity_keys; p.seqlen_ro = seqlen_ro;
        p.cs[0] = packed ? 0 : (int64_t)Nnew * fa2::kMlaDv; p.cs[1] = fa2::kMlaDv;
        p.ps[0] = packed ? 0 : (int64_t)Nnew * fa2::kMlaRot; p.ps[1] = fa2::kMlaRot;
        p.ks[0] = (int64_t)(paged ? page_size : capacity) * ROW; p.ks[1] = ROW; p.ks[2] = ROW;      // bytes
        if (packed) { p.qs[0] = 0; p.qs[1] = fa2::kMlaD; p.qs[2] = (int64_t)H * fa2::kMlaD; }
        else { p.qs[0] = (int64_t)Nnew * H * fa2::kMlaD; p.qs[1] = fa2::kMlaD; p.qs[2] = (int64_t)H * fa2::kMlaD; }
        for (int k = 0; k < 3; ++k) p.qos[k] = p.qs[k];
        p.bts = capacity; p.ros = 32;

        std::vector<uint16_t> cache_w((size_t)cache_rows * ROW, 0), q_w(has_q ? (size_t)total * H * fa2::kMlaChunks : 0, 0);
        const int group_units = p.R * fa2::kMlaUnits, threads = fa2::append_threads(group_units);
        const int slices = (group_units + threads - 1) / threads;
        for (int64_t t = 0; t < total; ++t) {
            int b, i, nnew;
            int64_t sb, sr;
            bool owned = true;
            if (packed) {
                int s = 0, ii = 0, nn = 1;
                owned = fa2::kvappend_varlen_token(cud, B, t, &s, &ii, &nn);
                b = owned ? s : 0; i = owned ? ii : 0; nnew = owned ? nn : 1; sb = 0; sr = t;
            } else {
                b = (int)(t / Nnew); i = (int)(t - (int64_t)b * Nnew); nnew = Nnew; sb = b; sr = i;
            }
            fa2::MlaFp8AppendRow w;
            const bool row = fa2::mla_fp8_append_row(p, b, i, nnew, sb, sr, owned, &w);
            if (row) {
                const int64_t slot = fa2::kvappend_slot(lens[b], capacity_keys, nnew, i), at = w.dst - cache;
                int64_t want = -1;
                if (slot >= 0) want = paged ? (int64_t)bt[(int64_t)b * capacity + slot / page_size] * page_size + slot % page_size : (int64_t)b * capacity + slot;
                if (!owned || slot < 0 || at % ROW != 0 || at / ROW != want) {
                    std::printf("wrong cache row: trial %d token %lld byte %lld want row %lld\n", trial, (long long)t, (long long)at, (long long)want);
                    return 1;
                }
            }
            for (int lane = 0; lane < slices * threads; ++lane) {
                if (lane < 64 && row) {                                                 // the first wave of slice 0
                    ++lanes;
                    unsigned char sink[32];
                    std::memcpy(sink, w.c + 8 * lane, 16);
                    std::memset(w.dst + 8 * lane, 1, 8);
                    for (int k = 0; k < 8; ++k) ++cache_w[(w.dst - cache) + 8 * lane + k];
                    if (lane == 0) {
                        std::memset(w.dst + fa2::kMlaFp8ScaleOff, 2, 16);
                        for (int k = 0; k < 16; ++k) ++cache_w[(w.dst - cache) + fa2::kMlaFp8ScaleOff + k];
                    }
                    if (lane >= fa2::kMlaTailUnit && lane < fa2::kMlaUnits) {
                        int col_a, col_b, byte_a, byte_b, j0;
                        fa2::mla_fp8_append_tail(lane, w.rotate && !p.interleaved, &col_a, &col_b, &byte_a, &byte_b, &j0);
                        std::memcpy(w.dst + byte_a, w.pe + col_a, 16);
                        std::memcpy(w.dst + byte_b, w.pe + col_b, 16);
                        for (int k = 0; k < 16; ++k) { ++cache_w[(w.dst - cache) + byte_a + k]; ++cache_w[(w.dst - cache) + byte_b + k]; }
                        if (w.rotate) {
                            std::memcpy(sink, cosb + ((size_t)w.tr + j0) * esz, 8 * esz);
                            std::memcpy(sink, sinb + ((size_t)w.tr + j0) * esz, 8 * esz);
                        }
                    }
                }
                if (lane < fa2::kMlaUnits) continue;                                    // the q units: the 16-bit kernel's, never its latent row
                fa2::MlaAppendUnit u;
                if (!fa2::mla_append_unit(p, lane, b, i, nnew, sb, sr, owned, &u)) continue;
                ++lanes;
                std::memcpy(u.dst + 8 * u.ca, u.src + (8 * u.ca - u.sc), 16);
                std::memcpy(u.dst + 8 * u.cb, u.src + (8 * u.cb - u.sc), 16);
                if (u.rotate) {
                    unsigned char sink[32];
                    std::memcpy(sink, cosb + ((size_t)u.tr + u.j0) * esz, 8 * esz);
                    std::memcpy(sink, sinb + ((size_t)u.tr + u.j0) * esz, 8 * esz);
                }
                uint16_t* marks = q_w.data() + (u.dst - q_out) / fa2::kMlaD * fa2::kMlaChunks;
                ++marks[u.ca];
                ++marks[u.cb];
            }
        }
        for (int64_t r = 0; r < cache_rows; ++r)
            for (int c = 1; c < ROW; ++c)
                if (cache_w[(size_t)r * ROW + c] != cache_w[(size_t)r * ROW]) {
                    std::printf("cache row %lld written in part: trial %d byte %d\n", (long long)r, trial, c);
                    return 1;
                }
        for (uint16_t m : q_w)
            if (m != 1) { std::printf("a q_out chunk written %d times: trial %d\n", (int)m, trial); return 1; }
        ++calls;
        delete[] kv_c; delete[] k_pe; delete[] cache; delete[] q; delete[] q_out; delete[] cosb; delete[] sinb; delete[] lens; delete[] bt; delete[] cud;
    }
    std::printf("ok: %ld calls, %ld lanes\n", calls, lanes);
    return 0;
}
