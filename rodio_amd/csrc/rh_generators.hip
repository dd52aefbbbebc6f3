// rh_generators.hip -- sources that start on the device: rodio's synthetic generators.
//   SignalGenerator::new(rate, freq, Function) and SineWave / SquareWave / TriangleWave / SawtoothWave::new(freq)
//                                                  (src/source/signal_generator.rs:86-154; sine.rs, square.rs, triangle.rs, sawtooth.rs)
//   chirp(rate, f0, f1, duration)                  (src/source/chirp.rs:11-97)
// Built with -ffp-contract=off (rodio_amd/build.py): no expression below is fused.  Sine uses the accurate sinf, not __sinf.
//
// A generator's phase is a serial f32 recurrence (rh_generators.h).  rh_signal_generate is two launches on one stream:
//   k_gen_walk  one lane per generator walks the recurrence (rhgen::advance) over the block and leaves the phase at the start of
//               every chunk of kChunk samples IN THE OUTPUT ROW, in the chunk's first slot; then writes the end phase back to the state;
//   k_gen_fill  one lane per chunk reads its start phase from that slot, runs the literal recurrence over kChunk samples, evaluates
//               the function into LDS and the wavefront stores the chunks coalesced.
// No scratch memory and no host round trip: block after block, the state array carries the stream on.
#include <cmath>
#include <cstdint>

#include "rh_common.h"
#include "rh_generators.h"

namespace {

constexpr uint32_t kChunk = 64;  // samples a lane of k_gen_fill produces from one checkpoint
constexpr uint32_t kFillLanes = 64;
constexpr float kTau = 6.2831855f;  // std::f32::consts::TAU (chirp; the generators' is in rh_generators.h)

__global__ __launch_bounds__(64) void k_gen_walk(float *__restrict__ dst, uint64_t ld, uint64_t n, float *__restrict__ st, uint32_t n_gens) {
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= n_gens) return;
    const float s = st[2 * g];
    rhgen::Walk w(st[2 * g + 1], s);
    float *row = dst + (size_t)g * ld;
    for (uint64_t c = 0; c < n; c += kChunk) {
        row[c] = w.p;
        w.advance(n - c < kChunk ? n - c : kChunk);
    }
    st[2 * g + 1] = w.p;
}

// grid (chunks / kFillLanes, generators); one wavefront a block
__global__ __launch_bounds__(kFillLanes) void k_gen_fill(float *__restrict__ dst, uint64_t ld, uint64_t n, const float *__restrict__ st, const int32_t *__restrict__ fns) {
    __shared__ float lds[kFillLanes * (kChunk + 1)];  // row per lane, padded: the column reads below hit 64 distinct banks
    const uint32_t g = blockIdx.y, t = threadIdx.x;
    float *row = dst + (size_t)g * ld;
    const uint64_t s0 = (uint64_t)blockIdx.x * kFillLanes * kChunk;  // first sample of the block
    const uint64_t c0 = s0 + (uint64_t)t * kChunk;                   // first sample of this lane's chunk
    const float s = st[2 * g];
    const int32_t fn = fns[g];
    if (c0 < n) {
        float p = row[c0];  // k_gen_walk's checkpoint
        const uint32_t m = n - c0 < kChunk ? (uint32_t)(n - c0) : kChunk;
        for (uint32_t j = 0; j < m; ++j) {
            lds[t * (kChunk + 1) + j] = rhgen::value(fn, p);  // (sine: the device's accurate sinf)
            p = rhgen::step(p, s);
        }
    }
    __syncthreads();  // every lane has read its checkpoint before any lane stores over the block's slots
    const uint64_t left = n - s0;
    const uint32_t total = left < (uint64_t)kFillLanes * kChunk ? (uint32_t)left : kFillLanes * kChunk;
    for (uint32_t i = t; i < total; i += kFillLanes) row[s0 + i] = lds[(i / kChunk) * (kChunk + 1) + i % kChunk];
}

// i = first + k for k < n (chirp.rs:53-63): ratio and time in f64 (IEEE division), the rest in f32, left to right.
__global__ __launch_bounds__(256) void k_chirp(float *__restrict__ dst, uint64_t first, uint64_t n, double total, double rate, float f0, float f1) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < n; k += stride) {
        const uint64_t i = first + k;
        const float ratio = (float)((double)i / total);
        const float freq = f0 * (1.0f - ratio) + f1 * ratio;
        const float t = (float)((double)i / rate) * kTau * freq;
        dst[k] = sinf(t);
    }
}

float rem_euclid1(float x) {  // Rust's f32::rem_euclid(x, 1.0)
    const float r = std::fmod(x, 1.0f);
    return r < 0.0f ? r + 1.0f : r;
}

}  // namespace

rh_status rh_signal_generator_init(float state[2], uint32_t sample_rate, float frequency) {
    // signal_generator.rs:99-113: assert!(frequency > 0.0) (NaN fails it too); period = rate as f32 / freq; phase_step = 1 / period
    if (!state || sample_rate == 0 || !(frequency > 0.0f)) return RH_ERR_INVALID;
    const float period = (float)sample_rate / frequency;
    state[0] = 1.0f / period;
    state[1] = 0.0f;
    return RH_OK;
}

rh_status rh_signal_generator_seek(float *phase, uint32_t sample_rate, float frequency, uint64_t pos_ns) {
    // signal_generator.rs:148-153: (as_secs_f32(d) * rate as f32 / period).rem_euclid(1.0), left to right
    if (!phase || sample_rate == 0 || !(frequency > 0.0f)) return RH_ERR_INVALID;
    const float period = (float)sample_rate / frequency;
    const float secs = (float)(pos_ns / 1000000000ull) + (float)(uint32_t)(pos_ns % 1000000000ull) / 1000000000.0f;
    *phase = rem_euclid1(secs * (float)sample_rate / period);
    return RH_OK;
}

float rh_signal_phase_advance(float phase, float phase_step, uint64_t n) { return rhgen::advance(phase, phase_step, n); }

rh_status rh_signal_generate(float *dst, uint64_t ld, uint64_t n, float *states_dev, const int32_t *functions_dev, uint32_t n_gens, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (n == 0 || n_gens == 0) return RH_OK;
    if (!dst || !states_dev || !functions_dev || ld < n || n_gens > 65535u) return RH_ERR_INVALID;
    const uint64_t chunks = (n + kChunk - 1) / kChunk, blocks = (chunks + kFillLanes - 1) / kFillLanes;
    if (blocks > 0x7fffffffull) return RH_ERR_INVALID;
    hipStream_t hs = rh::as_stream(stream);
    hipLaunchKernelGGL(k_gen_walk, dim3((n_gens + 63u) / 64u), dim3(64), 0, hs, dst, ld, n, states_dev, n_gens);
    RH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gen_fill, dim3((unsigned)blocks, n_gens), dim3(kFillLanes), 0, hs, dst, ld, n, states_dev, functions_dev);
    RH_CHECK_LAUNCH();
    return RH_OK;
}

rh_status rh_chirp_total_samples(uint32_t sample_rate, uint64_t duration_ns, uint64_t *total) {
    // chirp.rs:36-44: (duration.as_secs_f64() * rate as f64) as u64 (a saturating cast)
    if (!total || sample_rate == 0) return RH_ERR_INVALID;
    const double secs = (double)(duration_ns / 1000000000ull) + (double)(uint32_t)(duration_ns % 1000000000ull) / 1e9;
    const double v = secs * (double)sample_rate;
    *total = !(v > 0.0) ? 0 : v >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)v;
    return RH_OK;
}

rh_status rh_chirp_total_duration(uint32_t sample_rate, uint64_t total, uint64_t *secs, uint32_t *nanos) {
    // chirp.rs:83-86: Duration::from_secs_f64(total as f64 / rate as f64)
    if (!secs || !nanos || sample_rate == 0) return RH_ERR_INVALID;
    const double v = (double)total / (double)sample_rate;
    if (!(v >= 0.0) || v >= 18446744073709551616.0) return RH_ERR_INVALID;  // (from_secs_f64 panics)
    rhgen::duration_from_secs_f64(v, secs, nanos);
    return RH_OK;
}

rh_status rh_chirp(float *dst, uint64_t first, uint64_t n, uint64_t total, uint32_t sample_rate, float start_frequency, float end_frequency,
                   uint64_t *out_n, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (!out_n || sample_rate == 0) return RH_ERR_INVALID;
    // the iterator ends at `total` (chirp.rs:53-56): the block holds what is left of it
    const uint64_t m = first >= total ? 0 : (total - first < n ? total - first : n);
    *out_n = m;
    if (m == 0) return RH_OK;
    if (!dst) return RH_ERR_INVALID;
    hipLaunchKernelGGL(k_chirp, dim3(rh::grid_for(m)), dim3(256), 0, rh::as_stream(stream), dst, first, m, (double)total, (double)sample_rate, start_frequency, end_frequency);
    RH_CHECK_LAUNCH();
    return RH_OK;
}
