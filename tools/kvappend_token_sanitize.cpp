// kvappend_token_sanitize.cpp — the token -> sequence function of the packed KV-cache append (csrc/fa2_decode.hip.h: kvappend_varlen_token, the one
// function the kernel and fa2_kvappend_varlen_token call) as a stand-alone host program for AddressSanitizer and UBSan:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I flash-attention-v2-rdna3-minimal_amd/csrc -I include \
//         tools/kvappend_token_sanitize.cpp -o /tmp/kvappend_token_sanitize && /tmp/kvappend_token_sanitize
//
// 20 000 arrays of B + 1 ints (B = 1 .. 40) in heap blocks of exactly that size — so a probe outside cu[0 .. B] is a report — of four kinds: any int32,
// small values around zero, ascending with entries spoilt, the extremes; each with t at and around every entry, at the limits of int and int64 ranges
// and over [-3, 130).  Every answer must be "no sequence" or a consistent (s, i, nnew).  Prints "ok: <calls> calls, <named> named"; exit status 1 and
// the case on an inconsistent answer; the sanitizers abort on their own findings.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "fa2_decode.hip.h"

int main() {
    std::mt19937_64 g(20251);
    long named = 0, calls = 0;
    for (int trial = 0; trial < 20000; ++trial) {
        const int B = 1 + (int)(g() % 40);
        std::vector<int>* cu = new std::vector<int>(B + 1);
        const int kind = trial % 4;
        for (int j = 0; j <= B; ++j) {
            int x;
            if (kind == 0) x = (int)(uint32_t)g();
            else if (kind == 1) x = (int)(g() % 80) - 20;
            else if (kind == 2) x = j * 3 + ((g() % 7) == 0 ? (int)(g() % 600) - 300 : 0);
            else x = (g() % 3) ? INT_MAX - (int)(g() % 3) : INT_MIN + (int)(g() % 3);
            (*cu)[j] = x;
        }
        std::vector<int64_t> ts = {-1, 0, 1, INT_MAX, (int64_t)INT_MAX + 1, INT_MIN, (int64_t)1 << 40, -((int64_t)1 << 40)};
        for (int j = 0; j <= B; ++j) {
            ts.push_back((int64_t)(*cu)[j] - 1);
            ts.push_back((*cu)[j]);
            ts.push_back((int64_t)(*cu)[j] + 1);
        }
        for (int64_t t = -3; t < 130; ++t) ts.push_back(t);
        for (int64_t t : ts) {
            int s = -7, i = -7, n = -7;
            ++calls;
            if (!fa2::kvappend_varlen_token(cu->data(), B, t, &s, &i, &n)) continue;
            ++named;
            const std::vector<int>& c = *cu;
            if (!(s >= 0 && s < B && c[s] >= 0 && c[s] <= t && t < c[s + 1] && i == t - c[s] && n == c[s + 1] - c[s] && i >= 0 && i < n)) {
                std::printf("inconsistent: B %d t %lld -> %d %d %d\n", B, (long long)t, s, i, n);
                return 1;
            }
        }
        delete cu;
    }
    std::printf("ok: %ld calls, %ld named\n", calls, named);
    return 0;
}
