// fake_noise.cpp -- TEST INFRASTRUCTURE ONLY.  The CPU stand-in (see fake_device.cpp) for rh_noise_init / rh_noise_generate of
// rh_noise.hip, over the same rodio_amd/csrc/rh_noise.h.  Linked with fake_device.cpp into tests/cpp/noise_mirror_test_fake and into
// nothing else: it lets the C++ mirror's noise sources (trait answers, try_seek, the device path of GpuSource and GpuMixer and their
// upload counters) run in the `-m "not gpu"` suite.  The integrators run the serial recurrence here; the Gaussian uses the host's logf / cosf.
//
// Build: g++ -std=c++17 -O2 -ffp-contract=off -I include -I rodio_amd/csrc tests/cpp/noise_mirror_test.cpp tests/cpp/fake_device.cpp
//        tests/cpp/fake_noise.cpp -o tests/cpp/noise_mirror_test_fake
#include <cstdint>
#include <cstring>

#include "rh_noise.h"
#include "rodio_hip.h"

namespace {
uint64_t g_noise_generated = 0;
using namespace rhnoise;
}  // namespace

extern "C" {

uint64_t fake_noise_generated_samples(void) { return g_noise_generated; }

rh_status rh_noise_init(uint32_t state[8], int32_t kind, uint32_t sample_rate, uint64_t seed, uint32_t density) {
    if (!state || kind < WHITE_UNIFORM || kind > VELVET || sample_rate == 0 || (kind == VELVET && density == 0)) return RH_ERR_INVALID;
    std::memset(state, 0, 8 * sizeof(uint32_t));
    state[W_SEED_LO] = (uint32_t)seed, state[W_SEED_HI] = (uint32_t)(seed >> 32);
    state[W_KIND] = (uint32_t)kind;
    if (kind == VELVET) {
        const uint64_t grid = velvet_grid(sample_rate, density);
        state[W_PARAM] = (uint32_t)grid, state[W_SCALE] = (uint32_t)(grid >> 32);
    } else if (kind == RED || kind == BROWNIAN) {
        const float leak = integrator_leak(sample_rate), scale = integrator_scale(leak, kind == RED ? uniform_std_dev() : 0.6f);
        std::memcpy(&state[W_PARAM], &leak, 4);
        std::memcpy(&state[W_SCALE], &scale, 4);
    }
    return RH_OK;
}

rh_status rh_noise_generate(float *dst, uint64_t ld, uint64_t n, uint32_t *states, uint32_t n_streams, rh_stream) {
    if (n == 0 || n_streams == 0) return RH_OK;
    if (!dst || !states || ld < n || n_streams > 65535u) return RH_ERR_INVALID;
    for (uint32_t g = 0; g < n_streams; ++g) {
        uint32_t *st = states + 8 * (size_t)g;
        const uint64_t seed = (uint64_t)st[W_SEED_LO] | ((uint64_t)st[W_SEED_HI] << 32), k0 = (uint64_t)st[W_K_LO] | ((uint64_t)st[W_K_HI] << 32);
        const int32_t kind = (int32_t)st[W_KIND];
        float leak, scale, acc;
        std::memcpy(&leak, &st[W_PARAM], 4), std::memcpy(&scale, &st[W_SCALE], 4), std::memcpy(&acc, &st[W_ACC], 4);
        const uint64_t grid = (uint64_t)st[W_PARAM] | ((uint64_t)st[W_SCALE] << 32);
        float *row = dst + (size_t)g * ld;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t k = k0 + i, h = hash(seed, k);
            float v;
            switch (kind) {
                case WHITE_UNIFORM: v = u1(h); break;
                case WHITE_TRIANGULAR: v = triangular(h); break;
                case WHITE_GAUSSIAN: v = gaussian(h); break;
                case PINK: v = pink(seed, k); break;
                case BLUE: v = blue(seed, k); break;
                case VIOLET: v = violet(seed, k); break;
                case VELVET: v = velvet(seed, k, grid); break;
                case RED:
                case BROWNIAN:
                    acc = acc * leak + integrator_white(kind, seed, k);
                    v = acc * scale;
                    break;
                default: v = __builtin_nanf("");
            }
            row[i] = v;
        }
        const uint64_t k = k0 + n;
        st[W_K_LO] = (uint32_t)k, st[W_K_HI] = (uint32_t)(k >> 32);
        if (kind == RED || kind == BROWNIAN) std::memcpy(&st[W_ACC], &acc, 4);
    }
    g_noise_generated += n * n_streams;
    return RH_OK;
}
}
