// fake_live_filter.cpp -- TEST INFRASTRUCTURE ONLY.  The CPU stand-in (see fake_device.cpp) for rh_biquad_steps: a BltFilter whose
// coefficients change by steps while its memory stays, in the reference's operation order (blt.rs:559, left to right, unfused) for BOTH
// modes -- what the device computes bit for bit in mode 0 and within the filter contract in mode 1.  Linked with fake_device.cpp +
// fake_live.cpp into tests/cpp/live_filter_test_fake and into nothing else; it lets the host logic of live_low_pass / live_high_pass
// (tests/test_live_filter_cpu.py) run without a device.  It counts its calls (fake_live_filter_launches): a block is one.
//
// Build: g++ -std=c++17 -O2 -ffp-contract=off -I include tests/cpp/live_filter_test.cpp tests/cpp/fake_device.cpp tests/cpp/fake_widemix_filtered.cpp
//        tests/cpp/fake_live.cpp tests/cpp/fake_live_filter.cpp -o tests/cpp/live_filter_test_fake
#include <cstdint>
#include <vector>

#include "rodio_hip.h"

namespace {
uint64_t g_launches = 0;
uint64_t steps_needed(uint64_t first, uint64_t period, uint64_t n) { return n ? (first + n - 1) / period - first / period + 1 : 0; }
}  // namespace

extern "C" {

uint64_t fake_live_filter_launches(void) { return g_launches; }

rh_status rh_biquad_steps(float *dst, const float *src, uint64_t frames, uint32_t channels, uint32_t n_streams, uint64_t first, uint64_t period, const float *coeffs, uint32_t n_steps,
                          uint64_t table_stride, float *state, int32_t mode, rh_stream) {
    if (period == 0 || channels == 0 || (mode != 0 && mode != 1)) return RH_ERR_INVALID;
    if (frames == 0 || n_streams == 0) return RH_OK;
    const uint64_t row = frames * channels;
    if (!dst || !src || !coeffs || steps_needed(first, period, row) > n_steps) return RH_ERR_INVALID;
    if (table_stride != 0 && table_stride < 5ull * n_steps) return RH_ERR_INVALID;
    ++g_launches;
    for (uint32_t s = 0; s < n_streams; ++s) {
        std::vector<float> zero(4 * (size_t)channels, 0.0f);
        float *st = state ? state + (size_t)s * 4 * channels : zero.data();
        const float *x = src + s * row, *tab = coeffs + s * table_stride;
        float *y = dst + s * row;
        for (uint64_t i = 0; i < row; ++i) {
            const float *k = tab + 5 * ((first + i) / period - first / period);
            float *c = st + 4 * (i % channels);  // {x1, x2, y1, y2}
            const float xn = x[i];
            const float r = k[0] * xn + k[1] * c[0] + k[2] * c[1] - k[3] * c[2] - k[4] * c[3];  // blt.rs:559
            c[3] = c[2], c[1] = c[0], c[2] = r, c[0] = xn;
            y[i] = r;
        }
    }
    return RH_OK;
}

}  // extern "C"
