// The chain agreement's result slab (gibbssampling_amd/csrc/gs_statplan.h, agreement_slab)
// checked by a plain host program, built under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_agreement_plan_host.py: the parts' alignment and disjointness, the zeroed prefix
// (the per-chain sums, and the pool's count where the slab decides the pool), which parts a
// call with a summary's flags or a caller's mask leaves out, and the bytes charged.  The slab
// is then used as the device code uses it: every part written in full into a heap block of
// the slab's size, which the sanitizer bounds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "gs_statplan.h"

using namespace gs_plan;

static long failures = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            if (++failures <= 20) std::printf("line %d: %s\n", __LINE__, #x); \
        }                                                               \
    } while (0)

static void check(int64_t R, int64_t n, bool own_flags, bool own_count) {
    const Slab<kAgreementParts> s = agreement_slab(R, n, own_flags, own_count);
    // the kernels' shapes, in the order of the entry points' arguments
    CHECK(s.part[kAgrAgree].bytes() == n * 4);
    CHECK(s.part[kAgrSpread].bytes() == n * 8);
    CHECK(s.part[kAgrSpreadChain].bytes() == n * 4);
    CHECK(s.part[kAgrChainAgree].bytes() == R * 4);
    CHECK(s.part[kAgrChainDist].bytes() == R * 8);
    // the flags are the slab's unless a summary of the same call decided them; the count is
    // the slab's only when the rule decides the flags here (a mask is counted on the host)
    CHECK(s.part[kAgrFlags].bytes() == (own_flags ? R * 4 : 0));
    CHECK(s.part[kAgrNPooled].bytes() == (own_flags && own_count ? 4 : 0));
    // zero at launch: what collects atomic adds; the rest is written in full
    CHECK(s.part[kAgrChainAgree].zero && s.part[kAgrChainDist].zero && s.part[kAgrNPooled].zero);
    CHECK(!s.part[kAgrAgree].zero && !s.part[kAgrSpread].zero && !s.part[kAgrSpreadChain].zero &&
          !s.part[kAgrFlags].zero);
    CHECK(s.zeroed == R * 12 + s.part[kAgrNPooled].bytes());
    int64_t bytes = 0;
    for (int i = 0; i < kAgreementParts; ++i) {
        const Part &p = s.part[i];
        bytes += p.bytes();
        if (!p.wanted) continue;
        CHECK(p.elem == 4 || p.elem == 8);
        CHECK(p.off % p.elem == 0);
        CHECK(p.off >= 0 && p.off + p.bytes() <= s.total);
        if (p.zero)
            CHECK(p.off + p.bytes() <= s.zeroed);
        else
            CHECK(p.off >= s.zeroed);
        for (int j = 0; j < i; ++j) {
            const Part &q = s.part[j];
            if (q.wanted && p.bytes() > 0 && q.bytes() > 0)
                CHECK(p.off + p.bytes() <= q.off || q.off + q.bytes() <= p.off);
        }
    }
    CHECK(s.total - bytes < 8 * kAgreementParts);  // padding only
    // what a call is charged covers the slab whoever owns the flags
    CHECK(agreement_bytes(R, n) == n * 16 + R * 12 + R * 4 + 8);
    CHECK(s.total <= agreement_bytes(R, n) + 8);
    // every part written in full, each with its own byte, inside a block of the slab's size:
    // no write leaves the block and none lands on another part
    std::vector<unsigned char> mem((size_t)(s.total > 0 ? s.total : 1), 0xee);
    if (s.zeroed > 0) std::memset(mem.data(), 0, (size_t)s.zeroed);
    for (int i = 0; i < kAgreementParts; ++i) {
        const Part &p = s.part[i];
        if (!p.wanted || p.bytes() == 0) continue;
        for (int64_t b = 0; b < p.bytes(); ++b) CHECK(mem[(size_t)(p.off + b)] == (p.zero ? 0 : 0xee));
        std::memset(mem.data() + p.off, i + 1, (size_t)p.bytes());
    }
    for (int i = 0; i < kAgreementParts; ++i) {
        const Part &p = s.part[i];
        for (int64_t b = 0; p.wanted && b < p.bytes(); ++b) CHECK(mem[(size_t)(p.off + b)] == i + 1);
    }
}

int main() {
    for (const int64_t R : {1, 2, 3, 5, 64, 513})
        for (const int64_t n : {1, 2, 5, 16, 33})
            for (const bool own_flags : {false, true})
                for (const bool own_count : {false, true}) check(R, n, own_flags, own_count);
    if (failures) {
        std::printf("%ld checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
