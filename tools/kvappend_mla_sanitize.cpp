// kvappend_mla_sanitize.cpp — the addressing of the latent-cache append (csrc/fa2_kvappend_mla.hip.h: mla_append_unit, the one function both kernels
// call for a unit's source, destination and chunks, over mla_append_chunks, mla_append_cache_row, kvappend_slot, kvappend_varlen_token and
// rotary_table_row) as a stand-alone host program for AddressSanitizer and UBSan:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I flash-attention-v2-rdna3-minimal_amd/csrc -I include \
//         tools/kvappend_mla_sanitize.cpp -o /tmp/kvappend_mla_sanitize && /tmp/kvappend_mla_sanitize
//
// 4 000 calls, uniform and packed, contiguous and paged, with and without q and tables, on heap blocks sized to the BYTE: kv_c, k_pe, q, q_out, the
// cache (rows * 576 values: a row index outside it is a report), the tables (seqlen_ro rows of 32), the lengths, the block table and cu_seqlens.  The
// lengths are of four kinds (any int32, around 0, around the capacity, the extremes), the block table holds any int32, cu_seqlens is well formed, cut
// short (cu[B] < total) or random.  The walk is the kernel's: every group, every unit of the launch grid (the padding lanes of the last slice too),
// through mla_append_unit; each unit that moves something copies its two 16-byte chunks with memcpy and, where it rotates, reads the 8 table entries it
// would.  Checked besides what the sanitizers see: every chunk of q_out is written exactly once; a cache row is written in all 72 chunks or in
// none (as often in each: a block table nobody validated may give one page to two sequences) and is the row kvappend_slot and the table name.
// Prints "ok: <calls> calls, <units> units"; exit status 1 and the case on a wrong walk.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "fa2_kvappend_mla.hip.h"

using fa2::KvAppendMlaParams;

template <class T>
static T* block(size_t n) { return n ? new T[n]() : new T[1](); }      // (a zero-length new[] is legal but useless as a base)

int main() {
    std::mt19937_64 g(20253);
    long calls = 0, units = 0;
    for (int trial = 0; trial < 4000; ++trial) {
        const bool packed = trial & 1, paged = trial & 2, has_tab = (trial & 12) != 0, has_q = has_tab && (trial & 4), tab16 = trial & 16;
        const int B = 1 + (int)(g() % 4), H = has_q ? 1 + (int)(g() % (trial % 7 == 0 ? 128 : 9)) : 0;
        const int page_size = paged ? 64 * (1 + (int)(g() % 2)) : 0;
        const int capacity = paged ? 1 + (int)(g() % 4) : 1 + (int)(g() % 200);
        const int num_pages = paged ? 1 + (int)(g() % 6) : 0;
        const int64_t capacity_keys = paged ? (int64_t)capacity * page_size : capacity;
        const int64_t cache_rows = paged ? (int64_t)num_pages * page_size : (int64_t)B * capacity;
        const int seqlen_ro = 1 + (int)(g() % 40);

        // the tokens: the uniform call's B * Nnew, or the packed call's total under some cu_seqlens
        const int Nnew = 1 + (int)(g() % (trial % 5 == 0 && H <= 9 ? 140 : 6));
        std::vector<int> cu(B + 1, 0);
        int64_t total = (int64_t)B * Nnew;
        if (packed) {
            for (int s = 0; s < B; ++s) cu[s + 1] = cu[s] + (int)(g() % 5) * (int)(g() % 3);
            total = cu[B] + (int)(g() % 3);                                           // cu[B] < total is legitimate
            if (trial % 8 == 5) for (int& x : cu) x = (g() % 3) ? (int)(g() % 30) - 5 : (int)(uint32_t)g();       // nobody validated it
            if (total == 0) total = 1;
        }

        uint16_t* kv_c = block<uint16_t>((size_t)total * fa2::kMlaDv);
        uint16_t* k_pe = block<uint16_t>((size_t)total * fa2::kMlaRot);
        uint16_t* cache = block<uint16_t>((size_t)cache_rows * fa2::kMlaD);
        uint16_t* q = has_q ? block<uint16_t>((size_t)total * H * fa2::kMlaD) : nullptr;
        uint16_t* q_out = has_q ? block<uint16_t>((size_t)total * H * fa2::kMlaD) : nullptr;
        const size_t tab_bytes = (size_t)seqlen_ro * 32 * (tab16 ? 2 : 4);
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
        p.ks[0] = (int64_t)(paged ? page_size : capacity) * fa2::kMlaD; p.ks[1] = fa2::kMlaD; p.ks[2] = fa2::kMlaD;
        if (packed) { p.qs[0] = 0; p.qs[1] = fa2::kMlaD; p.qs[2] = (int64_t)H * fa2::kMlaD; }
        else { p.qs[0] = (int64_t)Nnew * H * fa2::kMlaD; p.qs[1] = fa2::kMlaD; p.qs[2] = (int64_t)H * fa2::kMlaD; }
        for (int k = 0; k < 3; ++k) p.qos[k] = p.qs[k];
        p.bts = capacity; p.ros = 32;

        std::vector<uint16_t> cache_w((size_t)cache_rows * fa2::kMlaChunks, 0), q_w(has_q ? (size_t)total * H * fa2::kMlaChunks : 0, 0);
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
            for (int unit = 0; unit < slices * threads; ++unit) {
                fa2::MlaAppendUnit w;
                if (!fa2::mla_append_unit(p, unit, b, i, nnew, sb, sr, owned, &w)) continue;
                ++units;
                std::memcpy(w.dst + 8 * w.ca, w.src + (8 * w.ca - w.sc), 16);
                std::memcpy(w.dst + 8 * w.cb, w.src + (8 * w.cb - w.sc), 16);
                if (w.rotate) {                                                     // the 8 entries append_table reads of either table
                    unsigned char sink[32];
                    const size_t esz = tab16 ? 2 : 4;
                    std::memcpy(sink, cosb + ((size_t)w.tr + w.j0) * esz, 8 * esz);
                    std::memcpy(sink, sinb + ((size_t)w.tr + w.j0) * esz, 8 * esz);
                }
                const bool isq = unit >= fa2::kMlaUnits;
                uint16_t* marks = isq ? q_w.data() + (w.dst - q_out) / fa2::kMlaD * fa2::kMlaChunks : cache_w.data() + (w.dst - cache) / fa2::kMlaD * fa2::kMlaChunks;
                ++marks[w.ca];
                ++marks[w.cb];
                if ((isq ? w.dst - q_out : w.dst - cache) % fa2::kMlaD != 0 || w.ca == w.cb || w.ca < 0 || w.cb >= fa2::kMlaChunks) {
                    std::printf("a row off its grid or a bad chunk pair: trial %d token %lld unit %d\n", trial, (long long)t, unit);
                    return 1;
                }
                if (!isq) {
                    const int64_t slot = fa2::kvappend_slot(lens[b], capacity_keys, nnew, i);
                    const int64_t row = (w.dst - cache) / fa2::kMlaD;
                    int64_t want = -1;
                    if (slot >= 0) want = paged ? (int64_t)bt[(int64_t)b * capacity + slot / page_size] * page_size + slot % page_size : (int64_t)b * capacity + slot;
                    if (slot < 0 || row != want) {
                        std::printf("wrong cache row: trial %d token %lld unit %d row %lld want %lld\n", trial, (long long)t, unit, (long long)row, (long long)want);
                        return 1;
                    }
                }
            }
        }
        for (int64_t r = 0; r < cache_rows; ++r) {
            for (int c = 1; c < fa2::kMlaChunks; ++c)
                if (cache_w[(size_t)r * fa2::kMlaChunks + c] != cache_w[(size_t)r * fa2::kMlaChunks]) {
                    std::printf("cache row %lld written in part: trial %d\n", (long long)r, trial);
                    return 1;
                }
        }
        for (uint16_t m : q_w)
            if (m != 1) { std::printf("a q_out chunk written %d times: trial %d\n", (int)m, trial); return 1; }
        ++calls;
        delete[] kv_c; delete[] k_pe; delete[] cache; delete[] q; delete[] q_out; delete[] cosb; delete[] sinb; delete[] lens; delete[] bt; delete[] cud;
    }
    std::printf("ok: %ld calls, %ld units\n", calls, units);
    return 0;
}
