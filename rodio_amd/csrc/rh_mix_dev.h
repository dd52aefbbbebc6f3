// rh_mix_dev.h -- the device idioms the block mixers' kernels share (rh_widemix, rh_widebatch, rh_spatialmix, rh_playermix, rh_loopmix,
// rh_queuemix, rh_clipmix .hip), once.  Small always-inline helpers: every kernel keeps its own loop and its own body.  Which call sites
// use them, and which stayed written out because a helper changed their code for the worse, is profiles/refactor_block_mixers.txt; the
// four-slot position walk (p = r0 + j F; il = p / T; w = p - il T, and the pick of a source's slot) is written out in every kernel for
// that reason.
#pragma once
#include <cstdint>

namespace rh {
namespace mixdev {

// A table that travels by value lies in the kernel-argument segment and is read through the scalar cache, descriptor after descriptor: the
// first wave of a CU would miss on every line of it in turn (measured: 0.39 us per source, 12.5 us for a table of 32 -- whatever the
// block's length).  One word of each of `kLines` 64-byte lines from `w` on is asked for HERE, all requests in flight at once: one round
// trip, and the walk behind it hits.  `also`: one more word to ask for (a table's header in front of the lines).
template <uint32_t kLines>
__device__ __forceinline__ void touch_lines(const uint32_t *w, uint32_t also = 0) {
    uint32_t t[kLines], touch = also;
#pragma unroll
    for (uint32_t q = 0; q < kLines; ++q) t[q] = w[q * 16u];
#pragma unroll
    for (uint32_t q = 0; q < kLines; ++q) touch |= t[q];
    asm volatile("" ::"s"(touch));
}
// ... every line of a table.
template <class Table>
__device__ __forceinline__ void touch_table(const Table &tbl) {
    touch_lines<(sizeof(Table) + 63) / 64>(reinterpret_cast<const uint32_t *>(&tbl));
}

// channels.rs:59-70: output channel c of a source of ch channels reads input channel c (c < ch), channel 1 of a mono source its only one;
// every other one is 0.0.
__device__ __forceinline__ bool has_channel(uint32_t c, uint32_t ch) { return c < ch || (c == 1u && ch == 1u); }
__device__ __forceinline__ uint32_t in_channel(uint32_t c, uint32_t ch) { return c < ch ? c : 0u; }

// Amplify (amplify.rs:64) in front of the converter, then the lerp in math.rs:25's order with the IEEE division; lerp false: the first tap
// verbatim (a chain's last frame, sample_rate.rs:193-200; F == T, sample_rate.rs:133-136).
__device__ __forceinline__ float amp_lerp(float a, float b, float gain, bool lerp, float w, float Tf) {
    const float x = a * gain;
    float v = x;
    if (lerp) {
        const float y = b * gain;
        v = x + (y - x) * w / Tf;
    }
    return v;
}

}  // namespace mixdev
}  // namespace rh
