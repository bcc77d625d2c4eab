// decode_mla_tile_sanitize.cpp — the addressing arithmetic of the latent-cache decode (csrc/fa2_decode_mla.hip.h: mla_part_range, mla_tile, the clamps
// — the functions the kernel, the host plan and fa2_decode_mla_part_range / fa2_decode_mla_tile call) as a stand-alone host program for AddressSanitizer
// and UBSan:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I flash-attention-v2-rdna3-minimal_amd/csrc -I include \
//         tools/decode_mla_tile_sanitize.cpp -o /tmp/decode_mla_tile_sanitize && /tmp/decode_mla_tile_sanitize
//
// 20 000 caches — contiguous ones of `capacity` rows, pools of num_pages * page_size rows under a block table of `capacity` entries — as heap blocks
// of EXACTLY one byte per row, so a row index outside the cache is a report, with lengths of four kinds (any int32, around 0, around the capacity, the
// extremes) and block tables that hold any int32.  The walk is the kernel's: every part of every split, every tile of the part, every staged row of the
// tile through the row clamp.  Every row read must lie in the page the CLAMPED table entry names, and the live rows of all parts of a split together
// must be the keys [0, clamp(len)) once each.  Prints "ok: <walks> walks, <rows> rows"; exit status 1 and the case on a wrong walk; the sanitizers abort
// on their own findings.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "fa2_decode_mla.hip.h"

int main() {
    std::mt19937_64 g(20252);
    long walks = 0, rows = 0;
    for (int trial = 0; trial < 20000; ++trial) {
        const bool paged = trial & 1;
        const int page_size = paged ? 64 * (1 + (int)(g() % 3)) : 0;
        const int capacity = paged ? 1 + (int)(g() % 6) : 1 + (int)(g() % 700);
        const int num_pages = paged ? 1 + (int)(g() % 9) : 0;
        const int64_t capacity_keys = paged ? (int64_t)capacity * page_size : capacity;
        const int64_t cache_rows = paged ? (int64_t)num_pages * page_size : capacity;
        std::vector<unsigned char>* cache = new std::vector<unsigned char>((size_t)cache_rows, 1);
        std::vector<int>* bt = new std::vector<int>(paged ? capacity : 1);
        for (int& x : *bt) x = (g() % 3) ? (int)(g() % (uint64_t)(num_pages + 1)) : (int)(uint32_t)g();
        int64_t len;
        switch (trial / 2 % 4) {
            case 0: len = (int)(uint32_t)g(); break;
            case 1: len = (int64_t)(g() % 70) - 5; break;
            case 2: len = capacity_keys + (int64_t)(g() % 70) - 35; break;
            default: len = (g() & 1) ? ((g() & 1) ? INT64_MAX : INT_MAX) : ((g() & 1) ? INT64_MIN : INT_MIN); break;
        }
        const int l = fa2::decode_clamp_len(len, capacity_keys);
        const int page_keys = fa2::mla_page_keys(page_size, capacity_keys);
        const int splits[] = {1, 2, 3, 1 + (int)(g() % fa2::kMlaMaxSplit), fa2::kMlaMaxSplit};
        for (int nsplit : splits) {
            std::vector<int> seen((size_t)l, 0);
            for (int part = 0; part < nsplit; ++part) {
                int first = -7, nt = -7;
                fa2::mla_part_range(len, capacity_keys, nsplit, part, &first, &nt);
                ++walks;
                for (int t = first; t < first + nt; ++t) {
                    const fa2::MlaTile mt = fa2::mla_tile(t, l, page_keys);
                    if (mt.rows < 1 || mt.rows > fa2::kMlaTile || mt.slot < 0 || mt.slot >= (paged ? capacity : 1) || mt.row < 0 || mt.row + mt.rows > page_keys) {
                        std::printf("bad tile: len %lld cap %d page %d nsplit %d part %d tile %d -> %d %d %d\n", (long long)len, capacity, page_size, nsplit, part, t,
                                    mt.slot, mt.row, mt.rows);
                        return 1;
                    }
                    const int64_t base = paged ? (int64_t)fa2::prefill_clamp_page((*bt)[mt.slot], num_pages) * page_size : 0;
                    const int last = mt.rows - 1;
                    for (int kk = 0; kk < fa2::kMlaTile; ++kk) {          // the kernel stages all 32 rows of a tile, each through the clamp
                        rows += cache->data()[base + mt.row + (kk < last ? kk : last)];
                        if (kk <= last) ++seen[(size_t)t * fa2::kMlaTile + kk];
                    }
                }
            }
            for (int j = 0; j < l; ++j)
                if (seen[j] != 1) {
                    std::printf("key %d of %d seen %d times: len %lld cap %d page %d nsplit %d\n", j, l, seen[j], (long long)len, capacity, page_size, nsplit);
                    return 1;
                }
        }
        delete bt;
        delete cache;
    }
    std::printf("ok: %ld walks, %ld rows\n", walks, rows);
    return 0;
}
