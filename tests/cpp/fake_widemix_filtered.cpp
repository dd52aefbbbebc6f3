// fake_widemix_filtered.cpp -- TEST INFRASTRUCTURE ONLY.  The CPU stand-in (see fake_device.cpp) for rh_wide_mix_block_filtered and
// rh_wide_mix_filtered_scratch_bytes of rh_widemix.hip: the entry's three stages restated in plain C++ in the reference's order -- every
// filtered source converted into a row of the mixer's layout (amplify.rs:64, sample_rate.rs:131-201, channels.rs:57-85), the BltFilter
// over the row with its carried state (blt.rs:559; fake_device.cpp's rh_biquad, which runs the reference's order in both modes), and the
// ordered sum with the rows in their sources' places (fake_device.cpp's rh_wide_mix_block).  Linked with fake_device.cpp into every
// *_fake driver of tests/cpp (the header-only mirror names the entry) and into nothing else; it lets GpuMixer's planning of filtered
// wide generations run in the `-m "not gpu"` suite.
//
// Build: rodio_amd/build.py (_fakes: on the link line of every *_fake driver)
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

#include "rodio_hip.h"

extern "C" {

rh_status rh_wide_mix_filtered_scratch_bytes(uint32_t channels, uint64_t out_frames, uint32_t n_filtered, uint64_t *bytes) {
    if (!bytes || !channels || out_frames > 0x7fffffffull) return RH_ERR_INVALID;
    const uint64_t pitch = (out_frames * channels + 3) & ~3ull;
    *bytes = (uint64_t)n_filtered * (2 * pitch + 4ull * channels) * sizeof(float);
    return RH_OK;
}

rh_status rh_wide_mix_block_filtered(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs, uint32_t n, const int32_t *kinds, const float *coeffs5,
                                     float *const *states, int32_t mode, void *scratch, uint64_t scratch_bytes, rh_stream stream) {
    if (out_frames == 0) return RH_OK;
    if (!dst || !channels || !to_rate || (n && (!srcs || !kinds)) || (mode != 0 && mode != 1)) return RH_ERR_INVALID;
    uint32_t filtered = 0;
    for (uint32_t s = 0; s < n; ++s) {
        if (kinds[s] < -1 || kinds[s] > 1 || (kinds[s] >= 0 && !coeffs5)) return RH_ERR_INVALID;
        const rh_wide_src &x = srcs[s];
        if (!x.frames) continue;
        if (!x.data || !x.channels || !x.from_rate || x.frames > out_frames) return RH_ERR_INVALID;
        const uint32_t g = std::gcd(x.from_rate, to_rate);
        if ((uint64_t)(x.from_rate / g) * (to_rate / g) > 0xffffffffull) return RH_ERR_UNSUPPORTED;
        if (x.phase >= to_rate / g) return RH_ERR_INVALID;
        filtered += kinds[s] >= 0;
    }
    if (filtered) {  // (the rows are kept in host vectors here: the caller's buffer is only checked)
        uint64_t need = 0;
        rh_wide_mix_filtered_scratch_bytes(channels, out_frames, filtered, &need);
        if (!scratch || ((uintptr_t)scratch & 15u)) return RH_ERR_INVALID;
        if (scratch_bytes < need) return RH_ERR_CAPACITY;
    }
    std::vector<rh_wide_src> mixed(srcs, srcs + n);
    std::vector<std::vector<float>> rows(n);
    for (uint32_t s = 0; s < n; ++s) {
        const rh_wide_src &x = srcs[s];
        if (kinds[s] < 0 || !x.frames) continue;
        const uint32_t g = std::gcd(x.from_rate, to_rate), F = x.from_rate / g, T = to_rate / g;
        std::vector<float> conv(x.frames * channels);
        for (uint64_t j = 0; j < x.frames; ++j)
            for (uint32_t c = 0; c < channels; ++c) {
                const uint64_t p = (uint64_t)x.phase + j * F, i = p / T;
                const uint32_t num = (uint32_t)(p - i * T);
                float v = 0.0f;
                if (c < x.channels || (c == 1 && x.channels == 1)) {
                    const uint32_t k = c < x.channels ? c : 0;
                    const float a = x.data[i * x.channels + k] * x.gain;
                    v = a;
                    if (F != T && i < x.last) {
                        const float b = x.data[(i + 1) * x.channels + k] * x.gain;
                        v = a + (b - a) * (float)num / (float)T;
                    }
                }
                conv[j * channels + c] = v;
            }
        rows[s].resize(conv.size());
        const rh_status st = rh_biquad(rows[s].data(), conv.data(), x.frames, channels, 1, coeffs5 + 5 * (size_t)s, states ? states[s] : nullptr, 0, stream);
        if (st != RH_OK) return st;
        rh_wide_src &y = mixed[s];
        y.data = rows[s].data();
        y.channels = channels;
        y.from_rate = to_rate;
        y.phase = 0;
        y.last = x.last == 0xffffffffu ? 0xffffffffu : (uint32_t)(x.frames - 1);
        y.gain = 1.0f;
    }
    return rh_wide_mix_block(dst, channels, to_rate, out_frames, mixed.data(), n, stream);
}
}
