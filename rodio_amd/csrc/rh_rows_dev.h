// rh_rows_dev.h -- the per-sample arithmetic of the row adapters that more than one kernel spells: TakeDuration's fade-out filter
// (rh_take_duration), LinearGainRamp (rh_linear_gain_ramp), the converter's lerp and the channel rule (rh_uniform_segments).  The
// stand-alone kernels and the fused crossfade (rh_mix2.hip) call the same functions, so their bits cannot drift apart.  Every
// translation unit that includes this is built with -ffp-contract=off: the expressions below are the reference's operations in the
// reference's order.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace rhrows {

// TakeDuration's fade-out filter (take.rs:33-41): sample * remaining.as_millis() as f32 / total.as_millis() as f32 -- a multiply, then
// an IEEE divide; a duration under 1 ms gives x * 0 / 0.  total_ms = (float)(requested_ns / 1000000).
__device__ __forceinline__ float take_fade(float x, uint64_t remaining_ns, float total_ms) { return x * (float)(remaining_ns / 1000000ull) / total_ms; }

// LinearGainRamp (linear_ramp.rs:79-110): `elapsed` is a pure function of the frame index while the ramp runs (frame * (1e9 / rate) ns).
struct Ramp {
    uint64_t step_ns;     // 1e9 / rate (0 above 1 GHz: the ramp never advances)
    uint64_t done_frame;  // elapsed >= total from this frame on
    float total_s, start_gain, end_gain, after;
};
__host__ __device__ inline float secs_f32(uint64_t ns) { return (float)(ns / 1000000000ull) + (float)(uint32_t)(ns % 1000000000ull) / 1000000000.0f; }
inline Ramp make_ramp(uint32_t sample_rate, uint64_t duration_ns, float start_gain, float end_gain, bool clamp_end) {
    Ramp r;
    r.step_ns = 1000000000ull / sample_rate;  // linear_ramp.rs:98-100
    r.total_s = secs_f32(duration_ns);
    r.done_frame = r.step_ns ? (duration_ns + r.step_ns - 1) / r.step_ns : 0;
    r.start_gain = start_gain, r.end_gain = end_gain, r.after = clamp_end ? end_gain : 1.0f;
    return r;
}
__device__ __forceinline__ float ramp_factor(const Ramp &r, uint64_t frame) {
    // elapsed >= total  <=>  frame >= ceil(total / step) (done_frame; never when the step is 0)
    if (r.step_ns != 0 && frame >= r.done_frame) return r.after;
    const float p = secs_f32(frame * r.step_ns) / r.total_s;
    return r.start_gain * (1.0f - p) + r.end_gain * p;
}

// math.rs:23-26: first + (second - first) * numerator / denominator, in that order
__device__ __forceinline__ float lerp(float first, float second, float num, float den) { return first + (second - first) * num / den; }

// #m with floor(m*F/T) <= n-2 (both taps of the lerp exist)
__host__ __device__ inline uint64_t lerp_ready(uint64_t n, uint64_t F, uint64_t T) {
    if (n == 0) return 0;
    return (uint64_t)((((unsigned __int128)(n - 1) * T) + F - 1) / F);
}

}  // namespace rhrows
