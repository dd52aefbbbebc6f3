// fake_live.cpp -- TEST INFRASTRUCTURE ONLY.  The CPU stand-in (see fake_device.cpp) for the entry points of parameters that change
// while a source plays: rh_periodic_update_samples, rh_amplify_steps, rh_channel_volume_steps.  Linked with fake_device.cpp into
// tests/cpp/live_test_fake and into nothing else; it lets the schedule of the periodic_access() closures (tests/test_live_params_cpu.py)
// run without a device.  It also counts the calls of the two stepped entries (fake_live_launches): a SpatialPlayer block is one.
//
// Build: g++ -std=c++17 -O2 -ffp-contract=off -I include tests/cpp/live_test.cpp tests/cpp/fake_device.cpp tests/cpp/fake_live.cpp -o tests/cpp/live_test_fake
#include <cstdint>

#include "rodio_hip.h"

namespace {
uint64_t g_launches = 0;
uint64_t steps_needed(uint64_t first, uint64_t period, uint64_t n) { return n ? (first + n - 1) / period - first / period + 1 : 0; }
}  // namespace

extern "C" {

uint64_t fake_live_launches(void) { return g_launches; }

uint64_t rh_periodic_update_samples(uint64_t period_ns, uint32_t sample_rate, uint32_t channels) {  // periodic.rs:14-22
    const float secs = (float)(period_ns / 1000000000ull) + (float)(uint32_t)(period_ns % 1000000000ull) / 1000000000.0f;
    const float u = secs * (float)sample_rate * (float)channels;
    if (!(u >= 1.0f)) return 1;
    if (u >= 18446744073709551616.0f) return UINT64_MAX;
    return (uint64_t)u;
}

rh_status rh_amplify_steps(float *dst, const float *src, size_t n, uint64_t first, uint64_t period, const float *factors, uint32_t n_factors, rh_stream) {
    if (period == 0) return RH_ERR_INVALID;
    if (n == 0) return RH_OK;
    if (!dst || !src || !factors || steps_needed(first, period, n) > n_factors) return RH_ERR_INVALID;
    ++g_launches;
    for (size_t i = 0; i < n; ++i) dst[i] = src[i] * factors[(first + i) / period - first / period];  // amplify.rs:64
    return RH_OK;
}

rh_status rh_channel_volume_steps(float *dst, const float *src, size_t frames, uint32_t in_ch, uint32_t out_ch, uint64_t first, uint64_t gain_period, const float *gains,
                                  uint32_t n_gains, uint64_t factor_first, uint64_t factor_period, const float *factors, uint32_t n_factors, rh_stream) {
    if (in_ch == 0 || out_ch == 0 || out_ch > 16 || gain_period == 0 || (factors && factor_period == 0)) return RH_ERR_INVALID;
    if (frames == 0) return RH_OK;
    const uint64_t total = (uint64_t)frames * out_ch;
    if (!dst || !src || !gains || steps_needed(first, gain_period, total) > n_gains) return RH_ERR_INVALID;
    if (factors && steps_needed(factor_first, factor_period, total) > n_factors) return RH_ERR_INVALID;
    ++g_launches;
    for (size_t f = 0; f < frames; ++f) {  // channel_volume.rs:71-88, then amplify.rs:64
        float m = 0.0f;
        for (uint32_t c = 0; c < in_ch; ++c) m = m + src[f * in_ch + c];
        m = m / (float)in_ch;
        for (uint32_t k = 0; k < out_ch; ++k) {
            const uint64_t j = f * out_ch + k;
            float y = m * gains[((first + j) / gain_period - first / gain_period) * out_ch + k];
            if (factors) y = y * factors[(factor_first + j) / factor_period - factor_first / factor_period];
            dst[j] = y;
        }
    }
    return RH_OK;
}

}  // extern "C"
