// pcm16_launch_test.cpp -- sources set as 16-bit PCM: "the rows themselves, or a converted copy?" (rodio_amd/csrc/rh_rlm_pcm16.h) without a GPU.
// The decision over the cross product of its inputs against the conditions of include/rodio_hip.h (rh_rlm_set_sources_pcm16) written out a second
// time, as a list of reasons to convert.  TEST INFRASTRUCTURE: plain g++, no HIP, no library.
//
//     pcm16_launch_test
#include <cstdio>
#include <initializer_list>

#include "rh_rlm_pcm16.h"

using namespace rh::rlm;

static int g_failures = 0;
#define EXPECT(cond, ...)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++g_failures <= 20) {                      \
                std::fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
                std::fprintf(stderr, __VA_ARGS__);         \
                std::fprintf(stderr, "\n");                \
            }                                              \
        }                                                  \
    } while (0)

// The header comment of rh_rlm_set_sources_pcm16, clause by clause: is the run native?
static bool want_native(Route r, int ring, uint32_t ch, uint64_t frames, uint64_t addr, bool filters, bool subset) {
    if (filters || subset) return false;                  // "a handle ... without rh_rlm_set_filters", "the whole one-shot runs"
    const uint64_t bytes = frames * ch * 2;
    if (r == kChunk) return addr % 16 == 0 && bytes % 16 == 0;  // "every row on a 16-byte boundary and a whole number of 16-byte vectors"
    if (r == kMixed) return ring == 0 && addr % 8 == 0;         // "summed by k_mix_rows (not k_mix_ring): every row on an 8-byte boundary, any length"
    return false;                                         // "every other run"
}

int main() {
    long n = 0, native[kRoutes] = {0}, converted[kRoutes] = {0}, reasons[kPcmReasons] = {0};
    const uint64_t frames[] = {0, 1, 2, 3, 4, 5, 7, 8, 12, 1537, 4099, 30000, 30001, 600000, 600002, 600004, (1ull << 29) - 8, (1ull << 29) - 1};
    const uint64_t bases[] = {0x7f0000000000ull, 0x1000ull, 0xfffffffffff0ull};
    for (int r = 0; r < kRoutes; ++r)
        for (int ring : {0, 2, 3})
            for (uint32_t ch : {1u, 2u})
                for (uint64_t f : frames)
                    for (uint64_t base : bases)
                        for (uint64_t off = 0; off < 32; off += 2)  // (an int16 row starts on a 2-byte boundary)
                            for (int bits = 0; bits < 4; ++bits) {
                                const bool filters = bits & 1, subset = bits & 2;
                                // the OR over the rows: one row on the boundary and one `off` bytes behind it
                                const uint64_t addr_bits = base | (base + off);
                                const Pcm16No d = pcm16_native({(Route)r, ring, ch, f, addr_bits, filters, subset});
                                const bool want = want_native((Route)r, ring, ch, f, off, filters, subset);
                                EXPECT((d == kPcmNative) == want, "route %d ring %d ch %u frames %llu off %llu filters %d subset %d: %d", r, ring, ch, (unsigned long long)f,
                                       (unsigned long long)off, (int)filters, (int)subset, (int)d);
                                // a reason names a condition that does not hold
                                if (d == kPcmFilters) EXPECT(filters, "filters");
                                if (d == kPcmSubset) EXPECT(subset, "subset");
                                if (d == kPcmRoute) EXPECT(r != kChunk && r != kMixed, "route %d", r);
                                if (d == kPcmRing) EXPECT(r == kMixed && ring != 0, "ring %d", ring);
                                if (d == kPcmRows) EXPECT(r == kChunk && (f * ch) % 8 != 0, "rows %llu x %u", (unsigned long long)f, ch);
                                if (d == kPcmAlign) EXPECT(off % (r == kChunk ? 16 : 8) != 0, "off %llu", (unsigned long long)off);
                                (d == kPcmNative ? native : converted)[r] += 1;
                                reasons[d] += 1;
                                ++n;
                            }
    long routes_native = 0, routes_both = 0, reasons_reached = 0;
    for (int r = 0; r < kRoutes; ++r) {
        routes_native += native[r] > 0;
        routes_both += native[r] > 0 && converted[r] > 0;
        if (r != kChunk && r != kMixed) EXPECT(native[r] == 0, "route %d has no native kernel", r);
    }
    for (int d = 1; d < kPcmReasons; ++d) reasons_reached += reasons[d] > 0;
    // the boundaries are the kernels' own: LDS-DMA of 16 bytes a lane, loads of 8 bytes a lane
    EXPECT(kPcmChunkAlign == 16 && kPcmRowsAlign == 8, "alignments");
    std::printf("failures %d decisions %ld routes_native %ld routes_both %ld reasons_reached %ld reasons %d\n", g_failures, n, routes_native, routes_both, reasons_reached, (int)kPcmReasons - 1);
    return g_failures ? 1 : 0;
}
