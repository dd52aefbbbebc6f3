// rh_noise.h -- the library's one meaning of "noise": a counter-based generator whose draw k is a pure function of (seed, k).
// rh_dither (rh_formats.hip) and the noise sources (rh_noise.hip; src/source/noise.rs) both use it, so the dither's TPDF / RPDF /
// GPDF / HighPass noise is bit for bit WhiteTriangular / WhiteUniform / WhiteGaussian / Blue of the same seed (dither.rs:73-99).
//
//   h(seed, k) = mix(seed ^ mix(k + 1)), mix = the splitmix64 finaliser
//   u1(h) = (int(h >> 40) - 2^23) / 2^23,  u2(h) = (int((h >> 16) & 0xffffff) - 2^23) / 2^23      (24 bits each -> [-1, 1))
//   W(k) = u1(h(seed, k))                                                                          (the white uniform stream)
//
// Every expression is f32 in the stated order, built without contraction (-ffp-contract=off).  __host__ __device__: the kernels, the
// CPU stand-in (tests/cpp/fake_noise.cpp) and the host mirror's restatement (include/rodio_hip.hpp) agree on every bit except the
// Gaussian's, whose logf / cosf are the device's on the device and the host's on the host.
#ifndef RH_NOISE_H
#define RH_NOISE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RH_NOISE_HD __host__ __device__
#else
#define RH_NOISE_HD
#endif

namespace rhnoise {

// kinds (RH_NOISE_* of rodio_hip.h) and the eight state words of a stream
enum { WHITE_UNIFORM = 0, WHITE_TRIANGULAR = 1, WHITE_GAUSSIAN = 2, PINK = 3, BLUE = 4, VIOLET = 5, BROWNIAN = 6, RED = 7, VELVET = 8 };
enum { W_SEED_LO = 0, W_SEED_HI = 1, W_K_LO = 2, W_K_HI = 3, W_KIND = 4, W_PARAM = 5, W_SCALE = 6, W_ACC = 7, STATE_WORDS = 8 };
constexpr int kPinkGenerators = 16;  // PINK_NOISE_GENERATORS (noise.rs:427)

RH_NOISE_HD inline uint64_t mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}
RH_NOISE_HD inline uint64_t hash(uint64_t seed, uint64_t k) { return mix(seed ^ mix(k + 1)); }
RH_NOISE_HD inline float u1(uint64_t h) { return (float)((int32_t)(h >> 40) - 8388608) * 1.1920928955078125e-07f; }
RH_NOISE_HD inline float u2(uint64_t h) { return (float)((int32_t)((h >> 16) & 0xffffffu) - 8388608) * 1.1920928955078125e-07f; }
RH_NOISE_HD inline float triangular(uint64_t h) { return (u1(h) + u2(h)) * 0.5f; }
// Box-Muller on the two 24-bit fields, sigma 0.6 (noise.rs:383-412's distribution)
RH_NOISE_HD inline float gaussian(uint64_t h) {
    const float a = (float)((uint32_t)(h >> 40) + 1u) * 5.9604644775390625e-08f;       // (0, 1]
    const float b = (float)((uint32_t)(h >> 16) & 0xffffffu) * 5.9604644775390625e-08f;  // [0, 1)
    return sqrtf(-2.0f * logf(a)) * cosf(6.2831853071795864769f * b) * 0.6f;
}
RH_NOISE_HD inline float white(uint64_t seed, uint64_t k) { return u1(hash(seed, k)); }

// Blue (noise.rs:570-583): W(k) - W(k-1), W(-1) = 0.  Violet (:638-651): B(k) - B(k-1), B(-1) = 0.
RH_NOISE_HD inline float blue(uint64_t seed, uint64_t k) { return white(seed, k) - (k ? white(seed, k - 1) : 0.0f); }
RH_NOISE_HD inline float violet(uint64_t seed, uint64_t k) { return blue(seed, k) - (k ? blue(seed, k - 1) : 0.0f); }

RH_NOISE_HD inline uint32_t popc64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(x);
#else
    return (uint32_t)__builtin_popcountll(x);
#endif
}
// Pink (noise.rs:472-512, Voss-McCartney over 16 generators).  Generator i draws from W at every sample m that is a nonzero multiple of
// 2^i (its counter starts at 0 and reaches 2^i first at sample 2^i: generator 0 first updates at sample 1), the generators of one sample in
// the order i = 0, 1, ..  The draws made before sample m are D(m) = sum_{j<16} floor((m-1) / 2^j) for m >= 1; with
// sum_{j>=0} floor(x / 2^j) = 2x - popcount(x) that is 2x - popc(x) - (2y - popc(y)), x = m - 1, y = x >> 16 (u64 arithmetic, mod 2^64).
RH_NOISE_HD inline uint64_t pink_draws_before(uint64_t m) {
    const uint64_t x = m - 1, y = x >> 16;
    return (2 * x - popc64(x)) - (2 * y - popc64(y));
}
// Generator i's value at sample k: 0 before its first update, else the draw it made at m = k & ~(2^i - 1).
RH_NOISE_HD inline float pink_value(uint64_t seed, uint64_t k, int i) {
    const uint64_t m = k & ~((1ull << i) - 1);
    return m == 0 ? 0.0f : white(seed, pink_draws_before(m) + (uint64_t)i);
}
RH_NOISE_HD inline float pink(uint64_t seed, uint64_t k) {
    float sum = 0.0f;
    for (int i = 0; i < kPinkGenerators; ++i) sum += pink_value(seed, k, i);
    return sum / 16.0f;
}

// Velvet (noise.rs:282-330): grid = ceil(rate as f32 / density as f32) samples a cell (f32 arithmetic, :283); cell c = k / grid holds one
// impulse, at (u32(h >> 32) * grid) >> 32 (64-bit product) with h = h(seed, c), +1 if bit 31 of h is set, else -1; every other sample +0.0.
RH_NOISE_HD inline uint64_t velvet_grid(uint32_t rate, uint32_t density) { return (uint64_t)ceilf((float)rate / (float)density); }
RH_NOISE_HD inline uint64_t velvet_pos(uint64_t hc, uint64_t grid) { return ((hc >> 32) * grid) >> 32; }
RH_NOISE_HD inline float velvet_sign(uint64_t hc) { return (hc & 0x80000000ull) ? 1.0f : -1.0f; }
RH_NOISE_HD inline float velvet(uint64_t seed, uint64_t k, uint64_t grid) {
    const uint64_t c = k / grid, hc = hash(seed, c);
    return k - c * grid == velvet_pos(hc, grid) ? velvet_sign(hc) : 0.0f;
}

// Red / Brownian (IntegratedNoise, noise.rs:680-712): acc = acc * leak + w; out = acc * scale, with
// leak = 1 - (2 PI 5) / rate and scale = 1 / sqrt((sigma sigma) / (1 - leak leak)), f32 left to right; sigma = sqrt(1/3) (Red: WhiteUniform's
// std_dev, :157) or 0.6 (Brownian: WhiteGaussian's, :371).
constexpr float kPi = 3.14159265358979323846f;
RH_NOISE_HD inline float integrator_leak(uint32_t rate) { return 1.0f - (2.0f * kPi * 5.0f) / (float)rate; }
RH_NOISE_HD inline float integrator_scale(float leak, float sigma) {
    const float variance = (sigma * sigma) / (1.0f - leak * leak);
    return 1.0f / sqrtf(variance);
}
RH_NOISE_HD inline float uniform_std_dev() { return sqrtf(1.0f / 3.0f); }

// The white sample an integrator adds at k: WhiteUniform for Red, WhiteGaussian for Brownian
RH_NOISE_HD inline float integrator_white(int kind, uint64_t seed, uint64_t k) {
    const uint64_t h = hash(seed, k);
    return kind == BROWNIAN ? gaussian(h) : u1(h);
}

}  // namespace rhnoise

#endif
