// rh_live.hip -- parameters that change while a source plays (rodio's Player / SpatialPlayer chains):
//   Amplify::set_factor / set_log_factor under PeriodicAccess       (src/source/amplify.rs:27-35,64; periodic.rs:63-77)
//   ChannelVolume::set_volume / Spatial::set_positions, + a factor  (src/source/channel_volume.rs:71-88; spatial.rs:48-69)
// The value of a parameter is a TABLE of steps in device memory: sample `first + i` of the stream takes entry
// (first + i) / period - first / period.  The index is a 32-bit quotient relative to the block, by a multiplier the host
// computes once per launch (no 64-bit division per sample).  The arithmetic per sample is the reference's: x * factor;
// ((0 + s0) + s1 + ..) / C_in * gain[k], then * factor -- the same bits as rh_amplify / rh_channel_volume with that step's values.
#include <cstdint>

#include "rh_common.h"

namespace {

constexpr int kBlock = 256;
// A launch covers at most this many samples (output samples for the channel volume): every in-block index, plus the phase of the
// first sample inside its period, then fits in 32 bits.
constexpr uint64_t kMaxLaunchSamples = 1ull << 30;

// x / d for x < 2^32, 1 <= d <= 2^31 (the round-up method, Granlund-Montgomery): m = floor(2^32 (2^l - d) / d) + 1, l = ceil(log2 d);
// q = (hi(x m) + ((x - hi(x m)) >> min(l, 1))) >> max(l - 1, 0).  Exact for every x (tests/test_gpu_live.py checks the boundaries).
struct StepDiv {
    uint32_t phase;  // (first % period), reduced as below
    uint32_t m, s1, s2;
    __device__ __forceinline__ uint32_t step(uint32_t i) const {
        const uint32_t x = phase + i;
        const uint32_t t = __umulhi(x, m);
        return (t + ((x - t) >> s1)) >> s2;
    }
};

// The table index of sample i (< n <= 2^30) of a block whose first sample is the stream's sample `first`, for `period` >= 1.
StepDiv step_div(uint64_t first, uint64_t period, uint64_t n) {
    uint64_t d = period, phase = first % period;
    if (d > (1ull << 31)) {
        // at most one boundary inside the block, at i = period - phase: the same quotient with d = 2^31 and the phase moved so that the
        // boundary stays where it is (i < 2^30 keeps phase + i below 2^32)
        const uint64_t t = d - phase;
        d = 1ull << 31;
        phase = t >= n ? 0 : d - t;
    }
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    const uint64_t m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
    return StepDiv{(uint32_t)phase, (uint32_t)m, l < 1 ? l : 1u, l > 1 ? l - 1 : 0u};
}

// Entries of a table that covers samples [first, first + n) at `period`.
uint64_t steps_needed(uint64_t first, uint64_t period, uint64_t n) { return n ? (first + n - 1) / period - first / period + 1 : 0; }

// ----------------------------------------------------------- stepped Amplify ----
// rh::map4's shape (four consecutive samples a lane, one 16-byte load and store, rows that start anywhere, in place).
// WIDE (period >= 4): the four samples of a lane cross at most one boundary -- two table loads a lane (the second one only where the
// lane crosses), not four.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_amplify_steps(float *__restrict__ dst, const float *__restrict__ src, size_t n, StepDiv sd, const float *__restrict__ factors, int vec) {
    if (!WIDE) {
        rh::map4<kBlock>(dst, src, n, vec, [=](size_t i, float x) { return x * factors[sd.step((uint32_t)i)]; });
        return;
    }
    const size_t nvec = (n + 3) / 4, stride = (size_t)gridDim.x * kBlock;
    for (size_t v = (size_t)blockIdx.x * kBlock + threadIdx.x; v < nvec; v += stride) {
        const size_t i = 4 * v;
        if (i + 4 <= n) {
            const float4 x = (vec & 1) ? rh::ld_nt(reinterpret_cast<const float4 *>(src) + v) : rh::ld4_at(src, (int64_t)i, n);
            const uint32_t q0 = sd.step((uint32_t)i), q3 = sd.step((uint32_t)i + 3u);
            const float fa = factors[q0], fb = q3 != q0 ? factors[q3] : fa;
            const float4 y = make_float4(x.x * fa, x.y * (sd.step((uint32_t)i + 1u) == q0 ? fa : fb), x.z * (sd.step((uint32_t)i + 2u) == q0 ? fa : fb), x.w * fb);
            if (vec & 2) {
                rh::st_nt(reinterpret_cast<float4 *>(dst) + v, y);
            } else {
                dst[i] = y.x, dst[i + 1] = y.y, dst[i + 2] = y.z, dst[i + 3] = y.w;
            }
        } else {
            for (int j = 0; j < 4; ++j)
                if (i + j < n) dst[i + j] = src[i + j] * factors[sd.step((uint32_t)(i + j))];
        }
    }
}

// ---------------------------------------------- stepped ChannelVolume (+ factor) ----
// out[j] = (mean(frame j / out_ch) * gains[step_g(j)][j % out_ch]) * factors[step_f(j)]; factors == nullptr: no factor.
struct Tables {
    const float *gains;    // [steps][out_ch]
    const float *factors;  // [steps] or nullptr
    StepDiv g, f;
    __device__ __forceinline__ float apply(float m, uint32_t j, uint32_t k, uint32_t out_ch) const {
        const float y = m * gains[(size_t)g.step(j) * out_ch + k];
        return factors ? y * factors[f.step(j)] : y;
    }
};
// Stereo in / stereo out (the SpatialPlayer tail): two frames a lane, one 16-byte load, one 16-byte store (k_channel_volume_2x2's shape).
__global__ __launch_bounds__(kBlock) void k_channel_volume_steps_2x2(float *__restrict__ dst, const float *__restrict__ src, size_t frames, Tables t, int vec_ok) {
    const size_t nvec = (frames + 1) / 2, stride = (size_t)gridDim.x * kBlock;
    for (size_t v = (size_t)blockIdx.x * kBlock + threadIdx.x; v < nvec; v += stride) {
        const uint32_t j = 4u * (uint32_t)v;
        auto one = [&](float l, float r, uint32_t jj, float &ol, float &orr) {
            float m = (0.0f + l) + r;
            m = m / 2.0f;
            ol = t.apply(m, jj, 0, 2), orr = t.apply(m, jj + 1, 1, 2);
        };
        if (vec_ok && 2 * v + 2 <= frames) {
            const float4 x = rh::ld_nt(reinterpret_cast<const float4 *>(src) + v);
            float4 y;
            one(x.x, x.y, j, y.x, y.y);
            one(x.z, x.w, j + 2, y.z, y.w);
            rh::st_nt(reinterpret_cast<float4 *>(dst) + v, y);
        } else {
            for (size_t f = 2 * v; f < 2 * v + 2 && f < frames; ++f) one(src[2 * f], src[2 * f + 1], 2u * (uint32_t)f, dst[2 * f], dst[2 * f + 1]);
        }
    }
}
// Any layout: k_channel_volume_tile's shape -- the tile's input comes in as aligned 16-byte vectors into LDS, a lane per frame takes the
// mean, a lane per four output samples applies the steps and stores 16 bytes.
__global__ __launch_bounds__(kBlock) void k_channel_volume_steps_tile(float *__restrict__ dst, const float *__restrict__ src, size_t frames, uint32_t in_ch, uint32_t out_ch, Tables t,
                                                                      uint32_t tile_frames, uint32_t in_floats, int vec_ok) {
    extern __shared__ uint4 cvs_tile[];
    float *lds = reinterpret_cast<float *>(cvs_tile);
    float *means = lds + in_floats;
    const size_t f0 = (size_t)blockIdx.x * tile_frames;  // (a multiple of 4 frames)
    const uint32_t nf = (uint32_t)(frames - f0 < tile_frames ? frames - f0 : tile_frames);
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(src + f0 * in_ch), a0 = p0 & ~(uintptr_t)15;
    const uint32_t shift = (uint32_t)(p0 - a0) / 4u, nvec = (shift + nf * in_ch + 3u) / 4u;
    for (uint32_t v = threadIdx.x; v < nvec; v += kBlock) cvs_tile[v] = rh::ld_nt(reinterpret_cast<const uint4 *>(a0) + v);
    __syncthreads();
    for (uint32_t f = threadIdx.x; f < nf; f += kBlock) {
        const float *x = lds + shift + f * in_ch;
        float m = 0.0f;
        for (uint32_t c = 0; c < in_ch; ++c) m = m + x[c];
        means[f] = m / (float)in_ch;
    }
    __syncthreads();
    const uint32_t total = nf * out_ch, nv = (total + 3u) / 4u, j0 = (uint32_t)(f0 * out_ch);
    float *out = dst + f0 * out_ch;
    for (uint32_t v = threadIdx.x; v < nv; v += kBlock) {
        const uint32_t o0 = 4u * v;
        uint32_t f = o0 / out_ch, k = o0 - f * out_ch;
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = o0 + j < total ? t.apply(means[f], j0 + o0 + j, k, out_ch) : 0.0f;
            if (++k == out_ch) k = 0, ++f;
        }
        if (vec_ok && o0 + 4u <= total) {
            rh::st_nt(reinterpret_cast<float4 *>(out + o0), make_float4(e[0], e[1], e[2], e[3]));
        } else {
            for (int j = 0; j < 4; ++j)
                if (o0 + j < total) out[o0 + j] = e[j];
        }
    }
}
// Frames of hundreds of channels (a tile would not fit): a lane per frame.
__global__ __launch_bounds__(kBlock) void k_channel_volume_steps(float *__restrict__ dst, const float *__restrict__ src, size_t frames, uint32_t in_ch, uint32_t out_ch, Tables t) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t f = (size_t)blockIdx.x * kBlock + threadIdx.x; f < frames; f += stride) {
        float m = 0.0f;
        for (uint32_t c = 0; c < in_ch; ++c) m = m + src[f * in_ch + c];
        m = m / (float)in_ch;
        for (uint32_t k = 0; k < out_ch; ++k) dst[f * out_ch + k] = t.apply(m, (uint32_t)(f * out_ch + k), k, out_ch);
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

uint64_t rh_periodic_update_samples(uint64_t period_ns, uint32_t sample_rate, uint32_t channels) {
    // periodic.rs:14-22: (period.as_secs_f32() * rate as f32 * channels as f32) as usize, at least 1.  Duration::as_secs_f32 is
    // secs as f32 + subsec_nanos as f32 / 1e9 (f32); `as usize` saturates.
    const float secs = (float)(period_ns / 1000000000ull) + (float)(uint32_t)(period_ns % 1000000000ull) / 1000000000.0f;
    const float u = secs * (float)sample_rate * (float)channels;
    if (!(u >= 1.0f)) return 1;
    if (u >= 18446744073709551616.0f) return UINT64_MAX;
    return (uint64_t)u;
}

rh_status rh_amplify_steps(float *dst, const float *src, size_t n, uint64_t first, uint64_t period, const float *factors_dev, uint32_t n_factors, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (period == 0) return RH_ERR_INVALID;
    if (n == 0) return RH_OK;
    if (!dst || !src || !factors_dev || steps_needed(first, period, n) > n_factors) return RH_ERR_INVALID;
    for (uint64_t i0 = 0; i0 < n; i0 += kMaxLaunchSamples) {
        const uint64_t m = n - i0 < kMaxLaunchSamples ? n - i0 : kMaxLaunchSamples;
        const uint64_t at = first + i0;
        const StepDiv sd = step_div(at, period, m);
        if (period >= 4)
            hipLaunchKernelGGL(k_amplify_steps<true>, dim3(rh::grid_tiles((m + 3) / 4)), dim3(kBlock), 0, rh::as_stream(stream), dst + i0, src + i0, (size_t)m, sd,
                               factors_dev + (at / period - first / period), rh::rows_vec_bits(dst + i0, src + i0));
        else
            hipLaunchKernelGGL(k_amplify_steps<false>, dim3(rh::grid_tiles((m + 3) / 4)), dim3(kBlock), 0, rh::as_stream(stream), dst + i0, src + i0, (size_t)m, sd,
                               factors_dev + (at / period - first / period), rh::rows_vec_bits(dst + i0, src + i0));
        RH_CHECK_LAUNCH();
    }
    return RH_OK;
}

rh_status rh_channel_volume_steps(float *dst, const float *src, size_t frames, uint32_t in_ch, uint32_t out_ch, uint64_t first, uint64_t gain_period, const float *gains_dev,
                                  uint32_t n_gains, uint64_t factor_first, uint64_t factor_period, const float *factors_dev, uint32_t n_factors, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (in_ch == 0 || out_ch == 0 || out_ch > 16 || gain_period == 0 || (factors_dev && factor_period == 0)) return RH_ERR_INVALID;
    if (frames == 0) return RH_OK;
    const uint64_t total = (uint64_t)frames * out_ch;
    if (!dst || !src || !gains_dev || steps_needed(first, gain_period, total) > n_gains) return RH_ERR_INVALID;
    if (factors_dev && steps_needed(factor_first, factor_period, total) > n_factors) return RH_ERR_INVALID;
    // launches of whole frames, a multiple of 4 (the tile's first output sample starts a 16-byte vector), <= 2^30 output samples
    const uint64_t chunk = (kMaxLaunchSamples / out_ch) & ~3ull;
    for (uint64_t f0 = 0; f0 < frames; f0 += chunk) {
        const uint64_t nf = frames - f0 < chunk ? frames - f0 : chunk, j = f0 * out_ch, m = nf * out_ch;
        Tables t{gains_dev + (size_t)((first + j) / gain_period - first / gain_period) * out_ch, nullptr, step_div(first + j, gain_period, m), StepDiv{0, 1, 0, 0}};
        if (factors_dev) {
            t.factors = factors_dev + ((factor_first + j) / factor_period - factor_first / factor_period);
            t.f = step_div(factor_first + j, factor_period, m);
        }
        float *d = dst + j;
        const float *s = src + f0 * in_ch;
        if (in_ch == 2 && out_ch == 2) {
            hipLaunchKernelGGL(k_channel_volume_steps_2x2, dim3(rh::grid_tiles((nf + 1) / 2)), dim3(kBlock), 0, rh::as_stream(stream), d, s, (size_t)nf, t, (int)(aligned16(d) && aligned16(s)));
        } else {
            const uint64_t tf = (10240ull / (4ull * (in_ch + out_ch))) & ~3ull;  // ~10 KiB in + out a tile, as rh_channel_volume
            if (tf >= 8) {
                const uint32_t in_floats = (uint32_t)((tf * in_ch + 4 + 3) & ~3ull);
                const size_t lds = ((size_t)in_floats + tf) * 4;
                hipLaunchKernelGGL(k_channel_volume_steps_tile, dim3((unsigned)((nf + tf - 1) / tf)), dim3(kBlock), lds, rh::as_stream(stream), d, s, (size_t)nf, in_ch, out_ch, t,
                                   (uint32_t)tf, in_floats, (int)aligned16(d));
            } else {
                hipLaunchKernelGGL(k_channel_volume_steps, dim3(rh::grid_for(nf)), dim3(kBlock), 0, rh::as_stream(stream), d, s, (size_t)nf, in_ch, out_ch, t);
            }
        }
        RH_CHECK_LAUNCH();
    }
    return RH_OK;
}
