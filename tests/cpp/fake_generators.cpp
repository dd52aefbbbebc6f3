// fake_generators.cpp -- TEST INFRASTRUCTURE ONLY.  The CPU stand-in (see fake_device.cpp) for the generator entry points of
// rh_generators.hip, over the same rodio_amd/csrc/rh_generators.h.  Linked with fake_device.cpp into tests/cpp/generators_mirror_test_fake
// and into nothing else: it lets the C++ mirror's generators (size_hint, total_duration, try_seek, the device path of GpuSource and
// GpuMixer and their upload counters) run in the `-m "not gpu"` suite.  Sine uses the host's sinf.
//
// Build: g++ -std=c++17 -O2 -ffp-contract=off -I include -I rodio_amd/csrc tests/cpp/generators_mirror_test.cpp tests/cpp/fake_device.cpp
//        tests/cpp/fake_generators.cpp -o tests/cpp/generators_mirror_test_fake
#include <cmath>
#include <cstdint>

#include "rh_generators.h"
#include "rodio_hip.h"

namespace {
uint64_t g_generated = 0;
}

extern "C" {

uint64_t fake_generated_samples(void) { return g_generated; }

rh_status rh_signal_generator_init(float state[2], uint32_t sample_rate, float frequency) {
    if (!state || sample_rate == 0 || !(frequency > 0.0f)) return RH_ERR_INVALID;
    state[0] = 1.0f / ((float)sample_rate / frequency);
    state[1] = 0.0f;
    return RH_OK;
}
rh_status rh_signal_generator_seek(float *phase, uint32_t sample_rate, float frequency, uint64_t pos_ns) {
    if (!phase || sample_rate == 0 || !(frequency > 0.0f)) return RH_ERR_INVALID;
    const float period = (float)sample_rate / frequency;
    const float secs = (float)(pos_ns / 1000000000ull) + (float)(uint32_t)(pos_ns % 1000000000ull) / 1000000000.0f;
    const float r = std::fmod(secs * (float)sample_rate / period, 1.0f);
    *phase = r < 0.0f ? r + 1.0f : r;
    return RH_OK;
}
float rh_signal_phase_advance(float phase, float phase_step, uint64_t n) { return rhgen::advance(phase, phase_step, n); }
rh_status rh_signal_generate(float *dst, uint64_t ld, uint64_t n, float *st, const int32_t *fns, uint32_t n_gens, rh_stream) {
    if (n == 0 || n_gens == 0) return RH_OK;
    if (!dst || !st || !fns || ld < n) return RH_ERR_INVALID;
    for (uint32_t g = 0; g < n_gens; ++g) {
        float p = st[2 * g + 1];
        for (uint64_t i = 0; i < n; ++i) {
            dst[g * ld + i] = rhgen::value(fns[g], p);
            p = rhgen::step(p, st[2 * g]);
        }
        st[2 * g + 1] = p;
    }
    g_generated += n * n_gens;
    return RH_OK;
}
rh_status rh_chirp_total_samples(uint32_t sample_rate, uint64_t duration_ns, uint64_t *total) {
    if (!total || sample_rate == 0) return RH_ERR_INVALID;
    const double v = ((double)(duration_ns / 1000000000ull) + (double)(uint32_t)(duration_ns % 1000000000ull) / 1e9) * (double)sample_rate;
    *total = !(v > 0.0) ? 0 : v >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)v;
    return RH_OK;
}
rh_status rh_chirp_total_duration(uint32_t sample_rate, uint64_t total, uint64_t *secs, uint32_t *nanos) {
    if (!secs || !nanos || sample_rate == 0) return RH_ERR_INVALID;
    rhgen::duration_from_secs_f64((double)total / (double)sample_rate, secs, nanos);
    return RH_OK;
}
rh_status rh_chirp(float *dst, uint64_t first, uint64_t n, uint64_t total, uint32_t rate, float f0, float f1, uint64_t *out_n, rh_stream) {
    if (!out_n || rate == 0) return RH_ERR_INVALID;
    const uint64_t m = first >= total ? 0 : (total - first < n ? total - first : n);
    *out_n = m;
    for (uint64_t k = 0; k < m; ++k) {
        const uint64_t i = first + k;
        const float ratio = (float)((double)i / (double)total);
        const float freq = f0 * (1.0f - ratio) + f1 * ratio;
        dst[k] = std::sin((float)((double)i / (double)rate) * 6.2831855f * freq);
    }
    g_generated += m;
    return RH_OK;
}
}
