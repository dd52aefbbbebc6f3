// rh_playermix.hip -- a block of a mixer of PLAYERS in one launch:
//     out[m][c] = ((0.0 + v_0[m][c]) + v_1[m][c]) + ...                                                 mixer.rs:185-198, insertion order
//     v_s       = ChannelCountConverter(SampleRateConverter(Amplify_steps(LinearGainRamp(Amplify_gain(x_s)))))
// Player::append wraps every sound in speed -> .. -> amplify -> .. under a periodic_access that resets the volume (player.rs:121-166), the
// sound it is handed is very often source.fade_in(d) or a linear_gain_ramp, and the mixer converts the result to its own rate and layout
// and adds it (mixer.rs:58-66).  Until now that was rh_linear_gain_ramp and rh_amplify_steps per source into a row and rh_wide_mix_block
// over the rows: 2 N + ceil(N / 32) launches, every row written twice and read three times.  Both adapters are pure functions of a
// sample's position -- the ramp's factor of its FRAME (rhrows::ramp_factor, the function rh_linear_gain_ramp and the fused crossfade
// share), the stepped factor of its SAMPLE index (rh_live.hip's rule: sample k = f * src_channels + c takes entry
// (first + k) / period - first / period) -- so, as in rh_widemix.hip and rh_spatialmix.hip, a lane per output sample works out
//     i = floor((phase + j F) / T), num = (phase + j F) mod T
//     i <  last :  a + (b - a) * num / T       (math.rs:25; a, b: samples (i, k) and (i + 1, k) behind the three multiplies)
//     i >= last :  a, verbatim (sample_rate.rs:193-200);   F == T: a (sample_rate.rs:133-136)
// with k by channels.rs:59-70, walks the sources in insertion order and adds: the reference's rounding sequence, bit for bit.  Per tap, each
// a rounded f32 multiply of its own (-ffp-contract=off): x * gain, * ramp factor (where there is a ramp), * step factor (where there is a table).
// The host decisions are rh_player_mix_plan.h's; the source table travels by value as a kernel argument (32 sources a launch; more
// continue from the stored partial sum).
#include "rh_common.h"
#include "rh_mix_dev.h"
#include "rh_player_mix_plan.h"
#include "rh_rows_dev.h"

namespace {

namespace md = rh::mixdev;
namespace pm = rh::playermix;

constexpr int kBlock = 256;
constexpr int kGroup = (int)pm::kGroup;

using rh::mixplan::StepDiv;  // rh_live.hip's step index: sample k of the source's stream, counted from data -> entry of a step table
using rh::mixplan::step_div;
using rh::mixplan::kStepNone;

struct PmDesc {
    const float *data;     // the frame that holds the first tap of the block's first output frame
    const float *factors;  // the entry of that frame's first sample; nullptr: no stepped Amplify
    uint32_t ch;           // channels of the source
    uint32_t frames;       // output frames the source reaches (0: a slot that pads the table to whole groups)
    uint32_t last;         // ended sources: index (relative to data) of the LAST frame; live ones: 0xffffffff
    uint32_t rate;         // index into PmTable::r
    float gain;            // the innermost Amplify
    float Tf;              // T of its rate as a float; 0: the converter passes through (F == T)
    uint32_t ramp;         // pm::RampMode: 0 no multiply, 1 the constant `cf`, 2 rhrows::ramp_factor(r, first_frame + i) per tap
    float cf;
    StepDiv f;             // sample k of the source's stream, counted from data -> entry of factors
    uint64_t first_frame;  // frames of the ramp's stream in front of data
    rhrows::Ramp r;
};
struct PmTable {
    pm::Rate r[pm::kRates];
    PmDesc d[pm::kChunk];
};
static_assert(sizeof(PmTable) + 64 <= 4096, "the table and the other arguments share one 4 KiB kernel-argument segment");

// One lane per output SAMPLE, as k_wide_mix and k_spatial_mix: coalesced loads and stores for any layout.  The sources are walked in groups
// of kGroup whose taps and table entries are asked for before the first of them is used; a lane's additions stay in insertion order.  A
// source that does not reach the sample -- it has ended, or the channel is one it does not have -- reads its own first frame and entry and
// adds +0.0, which leaves a sum that started at +0.0 as it is; a tap that is not taken (verbatim frame, F == T) reads the first one again.
// Which ramp a source has is the same for every lane: a source without a running ramp pays no 64-bit arithmetic.
template <bool CONT>
__global__ __launch_bounds__(kBlock) void k_player_mix(float *__restrict__ dst, uint32_t to_ch, uint32_t out_frames, const PmTable tbl, uint32_t n_sources) {
    const uint64_t total = (uint64_t)out_frames * to_ch;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    md::touch_table(tbl);  // (the first wave of a CU would miss on the table's lines one after the other)
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += stride) {
        const uint32_t j = (uint32_t)(o / to_ch);
        const uint32_t c = (uint32_t)(o - (uint64_t)j * to_ch);
        uint32_t il[pm::kRates];
        float w[pm::kRates];  // num as a float (math.rs:25 multiplies by it, then divides by T)
#pragma unroll
        for (uint32_t q = 0; q < pm::kRates; ++q) {
            const uint32_t p = tbl.r[q].r0 + j * tbl.r[q].F;  // (host: fits 32 bits)
            il[q] = p / tbl.r[q].T;
            w[q] = (float)(p - il[q] * tbl.r[q].T);
        }
        float acc = CONT ? dst[o] : 0.0f;
        for (uint32_t s0 = 0; s0 < n_sources; s0 += kGroup) {  // (host: n_sources is a whole number of groups)
            float a[kGroup], b[kGroup], fa[kGroup], fb[kGroup], ra[kGroup], rb[kGroup], wv[kGroup];
            bool on[kGroup], lerp[kGroup];
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const PmDesc &d = tbl.d[s0 + u];
                const uint32_t q = d.rate;
                const uint32_t i = q == 0 ? il[0] : (q == 1 ? il[1] : (q == 2 ? il[2] : il[3]));
                wv[u] = q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
                const uint32_t k = md::in_channel(c, d.ch);
                on[u] = j < d.frames && md::has_channel(c, d.ch);
                lerp[u] = on[u] && d.Tf != 0.0f && i < d.last;
                const uint32_t ia = on[u] ? i : 0u, ib = lerp[u] ? ia + 1u : ia;
                a[u] = d.data[(uint64_t)ia * d.ch + k];
                b[u] = d.data[(uint64_t)ib * d.ch + k];
                const float *fp = d.factors ? d.factors : d.data;  // (no table: something readable, not used)
                fa[u] = fp[d.factors ? d.f.step(ia * d.ch + k) : 0u];  // (host: the sample index stays below 2^30)
                fb[u] = fp[d.factors ? d.f.step(ib * d.ch + k) : 0u];
                ra[u] = rb[u] = d.cf;
                if (d.ramp == pm::kRampLive) {  // the same for every lane
                    ra[u] = rhrows::ramp_factor(d.r, d.first_frame + ia);
                    rb[u] = rhrows::ramp_factor(d.r, d.first_frame + ib);
                }
            }
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const PmDesc &d = tbl.d[s0 + u];
                float x = a[u] * d.gain;                         // Amplify (amplify.rs:64), as k_wide_mix
                if (d.ramp != pm::kRampNone) x = x * ra[u];      // LinearGainRamp (linear_ramp.rs:79-110): the factor of the tap's frame
                if (d.factors) x = x * fa[u];                    // Amplify under periodic_access: the factor of the tap's sample
                float v = x;
                if (lerp[u]) {
                    float y = b[u] * d.gain;
                    if (d.ramp != pm::kRampNone) y = y * rb[u];
                    if (d.factors) y = y * fb[u];
                    v = x + (y - x) * wv[u] / d.Tf;
                }
                acc += on[u] ? v : 0.0f;
            }
        }
        dst[o] = acc;
    }
}

// ---- what a scene of Players usually is: STEREO sources of one rate into a STEREO mix, every source of the launch reaching every frame with
// both taps.  k_spatial_mix_mono2's shape: a lane takes an output FRAME -- its two 8-byte taps and ONE ramp factor per tap serve both channels,
// the tap offset and the weight are the lane's own, the store is 8 bytes --, a workgroup takes 64 frames and its four WAVES share the launch's
// sources: wave w works out the terms of sources 8 w .. 8 w + 7, their sixteen taps and their table entries in flight together, then the waves
// add in turn, each continuing the sum of the one before through LDS: the additions keep the insertion order.  The four samples a lane takes
// from a source -- (i, 0), (i, 1), (i + 1, 0), (i + 1, 1): consecutive in its stream -- almost always lie in one step: the steps of the first
// and the last are worked out, and only a lane that sees the two differ works out the two in between.  The same operations in the same order
// as k_player_mix.
struct PmFastSrc {
    const float2 *data;
    const float *factors;
    StepDiv f;
    float gain;
    uint32_t ramp;
    float cf;
    uint32_t pad;
    uint64_t first_frame;
    rhrows::Ramp r;
};
struct PmFastTable {
    uint32_t F, T, r0;
    float Tf;
    PmFastSrc d[pm::kChunk];
};
static_assert(sizeof(PmFastTable) + 64 <= 4096, "the table and the other arguments share one 4 KiB kernel-argument segment");
constexpr int kFastGroup = 8;                   // sources a wave takes
constexpr uint32_t kFastWaves = kBlock / 64;    // ... of the four of a workgroup
constexpr uint32_t kFastFrames = 64;            // frames a workgroup takes at a time
static_assert(kFastGroup * kFastWaves == pm::kChunk, "the waves of a workgroup share a launch's sources");
static_assert((kFastGroup * sizeof(PmFastSrc)) % 64 == 0, "a wave's descriptors are whole lines");
template <bool CONT, bool LERP>
__global__ __launch_bounds__(kBlock) void k_player_mix_stereo(float2 *__restrict__ dst, uint32_t out_frames, const PmFastTable tbl, uint32_t n_sources) {
    __shared__ float2 part[kFastFrames];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (a scalar: the wave's descriptors come through the scalar cache)
    const uint32_t s0 = wave * kFastGroup;
    const bool mine = s0 < n_sources;  // (wave-uniform: a wave without sources only keeps the barriers)
    if (mine) {
        // (a word of every line of the wave's descriptors, and the header, all requests in flight at once)
        md::touch_lines<(kFastGroup * sizeof(PmFastSrc)) / 64>(reinterpret_cast<const uint32_t *>(&tbl.d[s0]), tbl.F);
    }
    for (uint32_t base = blockIdx.x * kFastFrames; base < out_frames; base += gridDim.x * kFastFrames) {  // (host: out_frames < 2^31; the same trips for every lane)
        const bool act = base + lane < out_frames;
        const uint32_t j = act ? base + lane : out_frames - 1u;  // (a lane behind the block's end works on its last frame and stores nothing)
        float v0[kFastGroup], v1[kFastGroup];
        if (mine) {
            const uint32_t p = tbl.r0 + j * tbl.F;
            const uint32_t il = LERP ? p / tbl.T : j;
            const float w = LERP ? (float)(p - il * tbl.T) : 0.0f;
            const uint32_t k0 = 2u * il, k3 = LERP ? k0 + 3u : k0 + 1u;  // the first and the last sample of the source's stream this frame takes
            float2 a[kFastGroup], b[kFastGroup];
            float f0[kFastGroup], f3[kFastGroup], ra[kFastGroup], rb[kFastGroup];
            uint32_t h0[kFastGroup], h3[kFastGroup];
#pragma unroll
            for (int u = 0; u < kFastGroup; ++u) {  // (the slots behind the launch's last source repeat its first one: read, not added)
                const PmFastSrc &d = tbl.d[s0 + u];
                a[u] = d.data[il];
                b[u] = LERP ? d.data[il + 1u] : make_float2(0.0f, 0.0f);
                h0[u] = d.factors ? d.f.step(k0) : 0u, h3[u] = d.factors ? d.f.step(k3) : 0u;
                const float *fp = d.factors ? d.factors : reinterpret_cast<const float *>(d.data);
                f0[u] = fp[h0[u]];
                f3[u] = fp[h3[u]];
                ra[u] = rb[u] = d.cf;
                if (d.ramp == pm::kRampLive) {  // the same for every lane
                    ra[u] = rhrows::ramp_factor(d.r, d.first_frame + il);
                    if (LERP) rb[u] = rhrows::ramp_factor(d.r, d.first_frame + il + 1u);
                }
            }
#pragma unroll
            for (int u = 0; u < kFastGroup; ++u) {
                const PmFastSrc &d = tbl.d[s0 + u];
                // the step factors of (i, 0), (i, 1) and, with a second tap, (i + 1, 0), (i + 1, 1)
                float fa0 = f0[u], fa1 = LERP ? f0[u] : f3[u], fb0 = f0[u], fb1 = f3[u];
                if (LERP && h3[u] != h0[u]) {
                    fa1 = d.factors[d.f.step(k0 + 1u)];
                    fb0 = d.factors[d.f.step(k0 + 2u)];
                }
                float x0 = a[u].x * d.gain, x1 = a[u].y * d.gain;
                if (d.ramp != pm::kRampNone) x0 = x0 * ra[u], x1 = x1 * ra[u];
                if (d.factors) x0 = x0 * fa0, x1 = x1 * fa1;
                v0[u] = x0, v1[u] = x1;
                if (LERP) {
                    float y0 = b[u].x * d.gain, y1 = b[u].y * d.gain;
                    if (d.ramp != pm::kRampNone) y0 = y0 * rb[u], y1 = y1 * rb[u];
                    if (d.factors) y0 = y0 * fb0, y1 = y1 * fb1;
                    v0[u] = x0 + (y0 - x0) * w / tbl.Tf;
                    v1[u] = x1 + (y1 - x1) * w / tbl.Tf;
                }
            }
        }
        // the ordered sum: wave 0 starts it (from the stored partial sum behind an earlier launch), every wave continues the one before
#pragma unroll
        for (uint32_t turn = 0; turn < kFastWaves; ++turn) {
            if (wave == turn) {
                float2 acc = make_float2(0.0f, 0.0f);
                if (turn == 0) {
                    if (CONT) acc = dst[j];
                } else {
                    acc = part[lane];
                }
                if (mine) {
#pragma unroll
                    for (int u = 0; u < kFastGroup; ++u) {
                        const bool is = s0 + u < n_sources;
                        acc.x += is ? v0[u] : 0.0f;  // (+ 0.0 leaves a sum that started at + 0.0 as it is)
                        acc.y += is ? v1[u] : 0.0f;
                    }
                }
                if (turn + 1 < kFastWaves) part[lane] = acc;
                else if (act) dst[j] = acc;
            }
            __syncthreads();
        }
    }
}

}  // namespace

rh_status rh_player_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs_host, uint32_t n_sources, const uint64_t *ramps_host,
                              const float *ramp_gains_host, const float *const *factors_dev_host, const uint64_t *factor_steps_host, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (out_frames == 0) return RH_OK;
    // Everything is checked before the first launch: a call that fails has written nothing.
    const rh_status ok = pm::check(dst, channels, to_rate, out_frames, srcs_host, n_sources, ramps_host, ramp_gains_host, factors_dev_host, factor_steps_host);
    if (ok != RH_OK) return ok;
    hipStream_t st = rh::as_stream(stream);
    const uint32_t nf = (uint32_t)out_frames;
    // what the three adapters of source s are for this block (worked out where it is needed, not kept: the call allocates nothing)
    struct Adapters {
        uint32_t ramp;
        float cf;
        uint64_t first_frame;
        rhrows::Ramp r;
        const float *factors;
        StepDiv f;
    };
    auto adapters_of = [&](uint32_t s) {
        const rh_wide_src &x = srcs_host[s];
        Adapters a{pm::kRampNone, 1.0f, 0, rhrows::Ramp{0, 0, 0.0f, 0.0f, 0.0f, 1.0f}, nullptr, kStepNone};
        if (ramps_host && ramps_host[4 * (size_t)s] != 0) {
            const uint64_t *w = ramps_host + 4 * (size_t)s;
            a.r = rhrows::make_ramp((uint32_t)w[3], w[1], ramp_gains_host[2 * (size_t)s], ramp_gains_host[2 * (size_t)s + 1], w[0] == 2);
            a.first_frame = w[2];
            a.ramp = pm::ramp_mode(w[0], a.r.step_ns, a.r.done_frame, a.first_frame);
            a.cf = a.r.after;  // (a constant ramp: what rhrows::ramp_factor returns from done_frame on)
        }
        if (factors_dev_host && factors_dev_host[s]) {
            pm::Reach reach;
            pm::check_src(x, channels, to_rate, out_frames, &reach);
            const uint64_t first = factor_steps_host[3 * (size_t)s], period = factor_steps_host[3 * (size_t)s + 1];
            a.factors = factors_dev_host[s];
            a.f = step_div(first % period, period, reach.samples);
        }
        return a;
    };
    pm::walk(channels, to_rate, out_frames, srcs_host, n_sources, (reinterpret_cast<uintptr_t>(dst) & 7u) == 0, [&](const pm::Launch &L) {
        if (L.kernel == pm::kStereo) {
            PmFastTable u;
            u.F = L.r[0].F, u.T = L.r[0].T, u.r0 = L.r[0].r0, u.Tf = L.r[0].Tf;
            for (uint32_t q = 0; q < pm::kChunk; ++q) {
                const uint32_t s = L.src[q < L.n ? q : 0];
                const Adapters a = adapters_of(s);
                u.d[q] = PmFastSrc{reinterpret_cast<const float2 *>(srcs_host[s].data), a.factors, a.f, srcs_host[s].gain, a.ramp, a.cf, 0u, a.first_frame, a.r};
            }
            const bool lerp = u.F != u.T;
            const dim3 grid(rh::grid_for((size_t)nf, kFastFrames, 256u * 16u));
            float2 *d = reinterpret_cast<float2 *>(dst);
            if (L.cont && lerp) hipLaunchKernelGGL((k_player_mix_stereo<true, true>), grid, dim3(kBlock), 0, st, d, nf, u, L.n);
            else if (L.cont) hipLaunchKernelGGL((k_player_mix_stereo<true, false>), grid, dim3(kBlock), 0, st, d, nf, u, L.n);
            else if (lerp) hipLaunchKernelGGL((k_player_mix_stereo<false, true>), grid, dim3(kBlock), 0, st, d, nf, u, L.n);
            else hipLaunchKernelGGL((k_player_mix_stereo<false, false>), grid, dim3(kBlock), 0, st, d, nf, u, L.n);
            return;
        }
        PmTable tbl;
        for (uint32_t q = 0; q < pm::kRates; ++q) tbl.r[q] = L.r[q];
        uint32_t k = 0;
        for (; k < L.n; ++k) {
            const uint32_t s = L.src[k];
            const rh_wide_src &x = srcs_host[s];
            const Adapters a = adapters_of(s);
            const pm::Rate &r = L.r[L.rate[k]];
            tbl.d[k] = PmDesc{x.data, a.factors, x.channels, (uint32_t)x.frames, x.last, L.rate[k], x.gain, r.F == r.T ? 0.0f : r.Tf, a.ramp, a.cf, a.f, a.first_frame, a.r};
        }
        // whole groups: slots that reach no frame (and point at something readable: the first source's first tap, or dst where there is no source)
        const float *readable = L.n ? tbl.d[0].data : dst;
        while (k % pm::kGroup) tbl.d[k++] = PmDesc{readable, nullptr, 1u, 0u, 0u, 0u, 0.0f, 0.0f, pm::kRampNone, 1.0f, kStepNone, 0, rhrows::Ramp{0, 0, 0.0f, 0.0f, 0.0f, 1.0f}};
        const uint64_t total = (uint64_t)nf * channels;
        const dim3 grid(rh::grid_for((size_t)total, kBlock, 256u * 16u));
        if (L.cont) hipLaunchKernelGGL(k_player_mix<true>, grid, dim3(kBlock), 0, st, dst, channels, nf, tbl, k);
        else hipLaunchKernelGGL(k_player_mix<false>, grid, dim3(kBlock), 0, st, dst, channels, nf, tbl, k);
    });
    RH_CHECK_LAUNCH();
    return RH_OK;
}
