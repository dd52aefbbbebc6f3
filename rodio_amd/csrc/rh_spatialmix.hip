// rh_spatialmix.hip -- a block of a mixer of spatial emitters in one launch:
//     out[m][c] = ((0.0 + v_0[m][c]) + v_1[m][c]) + ...                                        mixer.rs:185-198, insertion order
//     v_s       = SampleRateConverter(Amplify(ChannelVolume(x_s)))                             spatial_player.rs:60-77, player.rs:121-166, mixer.rs:58-66
// rodio's SpatialPlayer wraps a sound in Spatial -- a ChannelVolume over its mono mean with one gain per ear (spatial.rs:48-69,
// channel_volume.rs:71-88) --, retunes the gains every few milliseconds under periodic_access and puts an Amplify behind it; the mixer
// converts the result to its own rate and adds it.  Until now an emitter was a launch of its own per block (rh_channel_volume_steps: 4 bytes
// a frame of a mono source in, 8 out) whose stereo row rh_wide_mix_block then read back.  Here, as in rh_widemix.hip, the converter is a
// pure function of the output frame,
//     i = floor((phase + j F) / T), num = (phase + j F) mod T
//     i <  last :  a + (b - a) * num / T       (math.rs:25, in that order; a, b: samples (i, c) and (i + 1, c) of the emitter's output)
//     i >= last :  a, verbatim (sample_rate.rs:193-200);   F == T: a (sample_rate.rs:133-136)
// and a sample (f, c) of the emitter's output a pure function of source frame f: the mean ((0 + s0) + s1 + ..) / in_ch, times the gain
// of ITS step, column c, times the factor of ITS step (rh_live.hip's step rule: sample k = f * channels + c of the adapter's output takes
// entry (first + k) / period - first / period; a change may fall between the channels of a frame, and the two taps of one lerp may lie
// in different steps).  A lane walks the sources in insertion order and adds: the reference's rounding sequence, bit for bit.
// 4 in_ch N bytes in per source (the second tap of a frame is the first tap of the next: L1 / L2), 4 C M out.
// The source table travels by value as a kernel argument (32 sources a launch; more continue from the stored partial sum).
#include "rh_common.h"
#include "rh_mix_plan.h"

namespace {

namespace mp = rh::mixplan;
using mp::StepDiv;  // rh_live.hip's step index: sample k of the emitter's output, counted from a launch's first one -> entry of a step table
using mp::step_div;

constexpr int kBlock = 256;
constexpr uint32_t kSpChunk = mp::kChunk;  // sources a launch (the table: 2.6 KiB of the 4 KiB kernel-argument segment)
constexpr int kSpGroup = (int)mp::kGroup;  // ... walked in groups of this many, whose loads leave together
constexpr uint32_t kSpRates = mp::kRates;  // ... of at most this many different (rate, phase) pairs, as k_wide_mix
// A launch reaches at most this many samples of an emitter's output: every in-launch index, plus the phase of the first one inside
// its period, then fits in 32 bits (rh_live.hip's bound).
constexpr uint64_t kMaxLaunchSamples = 1ull << 30;
using SpRate = mp::Rate;  // r0: (phase + j0 F) mod T

struct SpDesc {
    const float *data;     // the frame that holds the first tap of the launch's first output frame
    const float *gains;    // the entry of that frame's first sample, [steps][channels]
    const float *factors;  // likewise, [steps]; nullptr: no Amplify
    uint32_t ch;           // channels of the source
    uint32_t frames;       // output frames of this launch the source reaches (0: a slot that pads the table to whole groups)
    uint32_t last;         // ended sources: index (relative to data) of the LAST frame; live ones: 0xffffffff
    uint32_t rate;         // index into SpTable::r
    float Tf;              // T of its rate as a float; 0: the converter passes through (F == T)
    uint32_t pad;
    StepDiv g, f;          // sample k of the emitter's output, counted from data -> entry of gains / factors
};
struct SpTable {
    SpRate r[kSpRates];
    SpDesc d[kSpChunk];
};
static_assert(sizeof(SpTable) + 64 <= 4096, "the table and the other arguments share one 4 KiB kernel-argument segment");

// One lane per output SAMPLE, as k_wide_mix: coalesced loads and stores for any channel count.  The sources are walked in groups of
// kSpGroup: the taps' first two channels (what a mono or stereo emitter has) and the table entries of the whole group are asked for
// before the first of them is used; further channels of a wider source follow in a loop.  A lane's additions stay in insertion order.
// A source that does not reach the frame reads its own first frame and first entries and adds +0.0, which leaves a sum that started
// at +0.0 as it is; a tap that is not taken (verbatim frame, F == T) reads the first tap's frame and entries again.
template <bool CONT>
__global__ __launch_bounds__(kBlock) void k_spatial_mix(float *__restrict__ dst, uint32_t to_ch, uint32_t out_frames, const SpTable tbl, uint32_t n_sources) {
    const uint64_t total = (uint64_t)out_frames * to_ch;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    {
        // (k_wide_mix: the table is read through the scalar cache, and the first wave of a CU would miss on its lines one after the
        //  other.  One word of every line is asked for here, all requests in flight at once.)
        const uint32_t *w = reinterpret_cast<const uint32_t *>(&tbl);
        constexpr uint32_t kLines = (sizeof(SpTable) + 63) / 64;
        uint32_t t[kLines], touch = 0;
#pragma unroll
        for (uint32_t q = 0; q < kLines; ++q) t[q] = w[q * 16u];
#pragma unroll
        for (uint32_t q = 0; q < kLines; ++q) touch |= t[q];
        asm volatile("" ::"s"(touch));
    }
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += stride) {
        const uint32_t j = (uint32_t)(o / to_ch);
        const uint32_t c = (uint32_t)(o - (uint64_t)j * to_ch);
        uint32_t il[kSpRates];
        float w[kSpRates];  // num as a float (math.rs:25 multiplies by it, then divides by T)
#pragma unroll
        for (uint32_t q = 0; q < kSpRates; ++q) {
            const uint32_t p = tbl.r[q].r0 + j * tbl.r[q].F;  // (host: fits 32 bits)
            il[q] = p / tbl.r[q].T;
            w[q] = (float)(p - il[q] * tbl.r[q].T);
        }
        float acc = CONT ? dst[o] : 0.0f;
        for (uint32_t s0 = 0; s0 < n_sources; s0 += kSpGroup) {  // (host: n_sources is a whole number of groups)
            const float *pa[kSpGroup], *pb[kSpGroup];
            float a0[kSpGroup], a1[kSpGroup], b0[kSpGroup], b1[kSpGroup], ga[kSpGroup], gb[kSpGroup], fa[kSpGroup], fb[kSpGroup], wv[kSpGroup];
            bool on[kSpGroup], lerp[kSpGroup];
#pragma unroll
            for (int u = 0; u < kSpGroup; ++u) {
                const SpDesc d = tbl.d[s0 + u];
                const uint32_t q = d.rate;
                const uint32_t i = q == 0 ? il[0] : (q == 1 ? il[1] : (q == 2 ? il[2] : il[3]));
                wv[u] = q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
                on[u] = j < d.frames;
                lerp[u] = on[u] && d.Tf != 0.0f && i < d.last;
                const uint32_t ia = on[u] ? i : 0u, ib = lerp[u] ? ia + 1u : ia;
                pa[u] = d.data + (uint64_t)ia * d.ch;
                pb[u] = d.data + (uint64_t)ib * d.ch;
                const uint32_t second = d.ch > 1u ? 1u : 0u;
                a0[u] = pa[u][0];
                a1[u] = pa[u][second];
                b0[u] = pb[u][0];
                b1[u] = pb[u][second];
                const uint32_t ka = ia * to_ch + c, kb = ib * to_ch + c;  // (host: below 2^30)
                ga[u] = d.gains[(size_t)d.g.step(ka) * to_ch + c];
                gb[u] = d.gains[(size_t)d.g.step(kb) * to_ch + c];
                const float *fp = d.factors ? d.factors : d.gains;  // (no Amplify: something readable, not used)
                fa[u] = fp[d.factors ? d.f.step(ka) : 0u];
                fb[u] = fp[d.factors ? d.f.step(kb) : 0u];
            }
#pragma unroll
            for (int u = 0; u < kSpGroup; ++u) {
                const SpDesc d = tbl.d[s0 + u];
                const float n = (float)d.ch;
                float ma = 0.0f + a0[u];  // channel_volume.rs:75-81: ((0 + s0) + s1 + ..) / channels, once per source frame
                if (d.ch > 1u) ma = ma + a1[u];
                for (uint32_t k = 2; k < d.ch; ++k) ma = ma + pa[u][k];
                ma = ma / n;
                float x = ma * ga[u];  // channel_volume.rs:85, then Amplify (amplify.rs:64)
                if (d.factors) x = x * fa[u];
                float v = x;
                if (lerp[u]) {
                    float mb = 0.0f + b0[u];
                    if (d.ch > 1u) mb = mb + b1[u];
                    for (uint32_t k = 2; k < d.ch; ++k) mb = mb + pb[u][k];
                    mb = mb / n;
                    float y = mb * gb[u];
                    if (d.factors) y = y * fb[u];
                    v = x + (y - x) * wv[u] / d.Tf;
                }
                acc += on[u] ? v : 0.0f;
            }
        }
        dst[o] = acc;
    }
}

// ---- what a scene is: MONO sources of one rate into a STEREO mix, every source of the launch reaching every frame with both taps.
// A lane takes an output FRAME: both taps are loaded once and serve both ears, the tap offset and the weight are the lane's own, the
// store is 8 bytes.  A block is short (64 Ki frames: a wave per SIMD if a workgroup took 256 of them) and a lane that walked 32 sources
// would wait for memory group after group with nothing beside it, so a workgroup takes 64 frames and its four WAVES share the sources:
// wave w works out the terms of sources 8 w .. 8 w + 7 -- their sixteen taps and their table entries in flight together --, then the
// waves add in turn, each continuing the sum of the one before through LDS: the additions keep the insertion order.
// The four samples a lane takes from an emitter -- (i, 0), (i, 1), (i + 1, 0), (i + 1, 1): consecutive in its output -- almost always
// lie in one step: the steps of the first and the last are worked out, the entries they need asked for with the taps, and only a lane
// that sees the two differ works out the two in between.  The same operations in the same order as k_spatial_mix.
struct SpFastSrc {
    const float *data, *gains, *factors;
    StepDiv g, f;
};
struct SpFastTable {
    uint32_t F, T, r0;
    float Tf;
    SpFastSrc d[kSpChunk];
};
constexpr int kSpFastGroup = 8;                      // sources a wave takes
constexpr uint32_t kSpFastWaves = kBlock / 64;       // ... of the four of a workgroup
constexpr uint32_t kSpFastFrames = 64;               // frames a workgroup takes at a time
static_assert(kSpFastGroup * kSpFastWaves == kSpChunk, "the waves of a workgroup share a launch's sources");
template <bool CONT, bool LERP>
__global__ __launch_bounds__(kBlock) void k_spatial_mix_mono2(float2 *__restrict__ dst, uint32_t out_frames, const SpFastTable tbl, uint32_t n_sources) {
    __shared__ float2 part[kSpFastFrames];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (a scalar: the wave's descriptors come through the scalar cache)
    const uint32_t s0 = wave * kSpFastGroup;
    const bool mine = s0 < n_sources;  // (wave-uniform: a wave without sources only keeps the barriers)
    if (mine) {
        // (k_spatial_mix: a word of every line of the wave's descriptors, all requests in flight at once, instead of missing the scalar
        //  cache line after line on the way through them)
        const uint32_t *w = reinterpret_cast<const uint32_t *>(&tbl.d[s0]);
        constexpr uint32_t kLines = (kSpFastGroup * sizeof(SpFastSrc)) / 64;
        uint32_t t[kLines + 1], touch = 0;
        t[kLines] = tbl.F;
#pragma unroll
        for (uint32_t q = 0; q < kLines; ++q) t[q] = w[q * 16u];
#pragma unroll
        for (uint32_t q = 0; q <= kLines; ++q) touch |= t[q];
        asm volatile("" ::"s"(touch));
    }
    for (uint32_t base = blockIdx.x * kSpFastFrames; base < out_frames; base += gridDim.x * kSpFastFrames) {  // (host: out_frames < 2^31; the same trips for every lane)
        const bool act = base + lane < out_frames;
        const uint32_t j = act ? base + lane : out_frames - 1u;  // (a lane behind the block's end works on its last frame and stores nothing)
        float v0[kSpFastGroup], v1[kSpFastGroup];
        if (mine) {
            const uint32_t p = tbl.r0 + j * tbl.F;
            const uint32_t il = LERP ? p / tbl.T : j;
            const float w = LERP ? (float)(p - il * tbl.T) : 0.0f;
            const uint32_t k0 = 2u * il, k3 = LERP ? k0 + 3u : k0 + 1u;  // the first and the last sample of the emitter's output this frame takes
            float a[kSpFastGroup], b[kSpFastGroup], g00[kSpFastGroup], g01[kSpFastGroup], g31[kSpFastGroup], f0[kSpFastGroup], f3[kSpFastGroup];
            uint32_t q0[kSpFastGroup], q3[kSpFastGroup], h0[kSpFastGroup], h3[kSpFastGroup];
#pragma unroll
            for (int u = 0; u < kSpFastGroup; ++u) {  // (the slots behind the launch's last source repeat its first one: read, not added)
                const SpFastSrc d = tbl.d[s0 + u];
                a[u] = d.data[il];
                b[u] = LERP ? d.data[il + 1u] : 0.0f;
                q0[u] = d.g.step(k0), q3[u] = d.g.step(k3);
                g00[u] = d.gains[2 * (size_t)q0[u]];
                g01[u] = d.gains[2 * (size_t)q0[u] + 1];
                g31[u] = d.gains[2 * (size_t)q3[u] + 1];
                h0[u] = d.factors ? d.f.step(k0) : 0u, h3[u] = d.factors ? d.f.step(k3) : 0u;
                const float *fp = d.factors ? d.factors : d.gains;
                f0[u] = fp[h0[u]];
                f3[u] = fp[h3[u]];
            }
#pragma unroll
            for (int u = 0; u < kSpFastGroup; ++u) {
                const SpFastSrc d = tbl.d[s0 + u];
                // gains and factors of (i, 0), (i, 1) and, with a second tap, (i + 1, 0), (i + 1, 1)
                float ga0 = g00[u], ga1 = LERP ? g01[u] : g31[u], gb0 = g00[u], gb1 = g31[u];
                float fa0 = f0[u], fa1 = LERP ? f0[u] : f3[u], fb0 = f0[u], fb1 = f3[u];
                if (LERP && q3[u] != q0[u]) {
                    ga1 = d.gains[2 * (size_t)d.g.step(k0 + 1u) + 1];
                    gb0 = d.gains[2 * (size_t)d.g.step(k0 + 2u)];
                }
                if (LERP && h3[u] != h0[u]) {
                    fa1 = d.factors[d.f.step(k0 + 1u)];
                    fb0 = d.factors[d.f.step(k0 + 2u)];
                }
                float ma = 0.0f + a[u];
                ma = ma / 1.0f;
                float x0 = ma * ga0, x1 = ma * ga1;
                if (d.factors) x0 = x0 * fa0, x1 = x1 * fa1;
                v0[u] = x0, v1[u] = x1;
                if (LERP) {
                    float mb = 0.0f + b[u];
                    mb = mb / 1.0f;
                    float y0 = mb * gb0, y1 = mb * gb1;
                    if (d.factors) y0 = y0 * fb0, y1 = y1 * fb1;
                    v0[u] = x0 + (y0 - x0) * w / tbl.Tf;
                    v1[u] = x1 + (y1 - x1) * w / tbl.Tf;
                }
            }
        }
        // the ordered sum: wave 0 starts it (from the stored partial sum behind an earlier launch), every wave continues the one before
#pragma unroll
        for (uint32_t turn = 0; turn < kSpFastWaves; ++turn) {
            if (wave == turn) {
                float2 acc = make_float2(0.0f, 0.0f);
                if (turn == 0) {
                    if (CONT) acc = dst[j];
                } else {
                    acc = part[lane];
                }
                if (mine) {
#pragma unroll
                    for (int u = 0; u < kSpFastGroup; ++u) {
                        const bool is = s0 + u < n_sources;
                        acc.x += is ? v0[u] : 0.0f;  // (+ 0.0 leaves a sum that started at + 0.0 as it is)
                        acc.y += is ? v1[u] : 0.0f;
                    }
                }
                if (turn + 1 < kSpFastWaves) part[lane] = acc;
                else if (act) dst[j] = acc;
            }
            __syncthreads();
        }
    }
}

// Entries of a table that covers samples [0, n) of a stream whose first sample lies `at` (< period) behind a boundary.
uint64_t steps_needed(uint64_t at, uint64_t period, uint64_t n) { return n ? (at + n - 1) / period + 1 : 0; }

struct Red {
    uint32_t F, T;
    uint64_t g0, f0;  // gain_first % gain_period, factor_first % factor_period: the rule needs no more of them
};

}  // namespace

rh_status rh_spatial_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs_host, uint32_t n_sources, const float *const *gains_dev_host,
                               const uint64_t *gain_steps_host, const float *const *factors_dev_host, const uint64_t *factor_steps_host, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (out_frames == 0) return RH_OK;
    if (!dst || channels == 0 || channels > 16 || to_rate == 0 || (n_sources && (!srcs_host || !gains_dev_host || !gain_steps_host))) return RH_ERR_INVALID;
    if (out_frames > 0x7fffffffull) return RH_ERR_UNSUPPORTED;
    // Everything is checked before the first launch: a call that fails has written nothing.
    auto factors_of = [&](uint32_t s) { return factors_dev_host ? factors_dev_host[s] : nullptr; };
    // (worked out where it is needed, not kept: the call allocates nothing)
    auto red_of = [&](uint32_t s, const mp::Rate &rt) {  // (rt: the source's slot, which holds its reduced rates)
        Red r{rt.F, rt.T, gain_steps_host[3 * (size_t)s] % gain_steps_host[3 * (size_t)s + 1], 0};
        if (factors_of(s)) r.f0 = factor_steps_host[3 * (size_t)s] % factor_steps_host[3 * (size_t)s + 1];
        return r;
    };
    uint64_t step = out_frames;  // output frames per launch: r0 + j F and the sample indices of the step rule must fit 32 bits for every source
    for (uint32_t s = 0; s < n_sources; ++s) {
        const rh_wide_src &x = srcs_host[s];
        if (x.frames == 0) continue;
        // the fields the entry shares with rh_wide_mix_block
        uint32_t F, T;
        uint64_t fit;
        const rh_status shared = mp::check_src(x, to_rate, out_frames, &F, &T, &fit);
        if (shared != RH_OK) return shared;
        // ... and the step rule's: the last source frame a launch touches, i <= (T - 1 + (nf - 1) F) / T + 1, times `channels` stays below 2^30
        const uint64_t fit_steps = (kMaxLaunchSamples / channels - 2) * T / F + 1;
        if (fit_steps < fit) fit = fit_steps;
        if (fit < step) step = fit;
        // the emitter: its Amplify is the factor table, so the shared `gain` has nothing to say
        if (x.gain != 1.0f || !gains_dev_host[s]) return RH_ERR_INVALID;
        const uint64_t gp = gain_steps_host[3 * (size_t)s + 1], gn = gain_steps_host[3 * (size_t)s + 2];
        if (gp == 0) return RH_ERR_INVALID;
        const uint64_t g0 = gain_steps_host[3 * (size_t)s] % gp;
        // the source frames the block's taps touch: 0 .. the first tap of the last frame it reaches, and the second one where that frame has it
        const uint64_t pl = (uint64_t)x.phase + (x.frames - 1) * F, il = pl / T;
        if (il > (1ull << 56)) return RH_ERR_UNSUPPORTED;
        const uint64_t touched = (il + (F != T && il < x.last ? 1 : 0) + 1) * channels;  // samples of the emitter's output
        if (steps_needed(g0, gp, touched) > gn) return RH_ERR_INVALID;
        if (factors_of(s)) {
            if (!factor_steps_host) return RH_ERR_INVALID;
            const uint64_t fp = factor_steps_host[3 * (size_t)s + 1], fn = factor_steps_host[3 * (size_t)s + 2];
            if (fp == 0) return RH_ERR_INVALID;
            if (steps_needed(factor_steps_host[3 * (size_t)s] % fp, fp, touched) > fn) return RH_ERR_INVALID;
        }
    }
    if (step == 0) return RH_ERR_UNSUPPORTED;
    // Alike sources (mono, one rate and phase, into a stereo mix on an 8-byte boundary): the frames in front of the first one that ends -- or
    // whose last frame a tap reaches -- go to the fast kernel as a launch of their own, the rest to the general one (rh_wide_mix_block's cut).
    const bool fast_ok = channels == 2 && (reinterpret_cast<uintptr_t>(dst) & 7u) == 0;
    const uint64_t j_uni = fast_ok ? mp::alike_cut(srcs_host, n_sources, 1, to_rate, out_frames) : 0;
    hipStream_t st = rh::as_stream(stream);
    for (uint64_t j0 = 0; j0 < out_frames;) {
        const uint64_t seg_end = j0 < j_uni ? j_uni : out_frames;
        const uint32_t nf = (uint32_t)(seg_end - j0 < step ? seg_end - j0 : step);
        mp::walk_rates<mp::RateLaunch>(
            n_sources, true,  // (no source reaches these frames: the mix is +0.0 there)
            [&](uint32_t s, uint32_t *F, uint32_t *T, uint32_t *r0, uint64_t *i0) {
                if (srcs_host[s].frames <= j0) return false;
                mp::reduce(srcs_host[s].from_rate, to_rate, F, T);
                mp::tap_of(srcs_host[s].phase, j0, *F, *T, i0, r0);  // position of frame j0 between its taps, from the block's first tap on
                return true;
            },
            [&](const mp::RateLaunch &L) {
                SpTable tbl;
                for (uint32_t q = 0; q < kSpRates; ++q) tbl.r[q] = L.r[q];
                uint32_t k = 0;
                bool mono = true;
                for (; k < L.n; ++k) {
                    const uint32_t s = L.src[k];
                    const rh_wide_src &x = srcs_host[s];
                    const Red red = red_of(s, L.r[L.rate[k]]);
                    const uint64_t i0 = L.i0[k];  // (what key worked out: no second gcd, no second division)
                    const uint32_t r0 = L.r[L.rate[k]].r0;
                    SpDesc &d = tbl.d[k];
                    d.data = x.data + i0 * x.channels;
                    d.ch = x.channels;
                    d.frames = (uint32_t)(x.frames - j0 < nf ? x.frames - j0 : nf);
                    d.last = x.last == 0xffffffffu ? 0xffffffffu : (x.last >= i0 ? (uint32_t)(x.last - i0) : 0u);
                    d.rate = L.rate[k];
                    d.Tf = red.F == red.T ? 0.0f : (float)red.T;
                    d.pad = 0;
                    // the step tables from the launch's first source frame on: sample K0 = i0 * channels of the emitter's output
                    const uint64_t K0 = i0 * channels;
                    const uint64_t reach = (((uint64_t)r0 + (uint64_t)(d.frames - 1) * red.F) / red.T + 2) * channels;  // (<= 2^30: `step`)
                    const uint64_t gp = gain_steps_host[3 * (size_t)s + 1];
                    d.gains = gains_dev_host[s] + ((red.g0 + K0) / gp) * channels;
                    d.g = step_div(red.g0 + K0, gp, reach);
                    d.factors = nullptr;
                    d.f = mp::kStepNone;
                    if (const float *f = factors_of(s)) {
                        const uint64_t fp = factor_steps_host[3 * (size_t)s + 1];
                        d.factors = f + (red.f0 + K0) / fp;
                        d.f = step_div(red.f0 + K0, fp, reach);
                    }
                    mono = mono && x.channels == 1;
                }
                // the fast case (k_spatial_mix_mono2): mono sources of one rate, a stereo mix, no source that ends inside the launch
                bool fast = fast_ok && k > 0 && L.nr == 1 && mono;
                const bool lerp = L.r[0].F != L.r[0].T;
                const uint64_t il_max = mp::last_tap(L.r[0], nf);
                for (uint32_t q = 0; q < k && fast; ++q) fast = tbl.d[q].frames == nf && (!lerp || il_max < tbl.d[q].last);
                if (fast) {
                    SpFastTable u;
                    u.F = L.r[0].F, u.T = L.r[0].T, u.r0 = L.r[0].r0, u.Tf = L.r[0].Tf;
                    for (uint32_t q = 0; q < kSpChunk; ++q) {
                        const SpDesc &d = tbl.d[q < k ? q : 0];
                        u.d[q] = SpFastSrc{d.data, d.gains, d.factors, d.g, d.f};
                    }
                    const dim3 grid(rh::grid_for((size_t)nf, kSpFastFrames, 256u * 16u));
                    float2 *d = reinterpret_cast<float2 *>(dst + j0 * 2);
                    if (L.cont && lerp) hipLaunchKernelGGL((k_spatial_mix_mono2<true, true>), grid, dim3(kBlock), 0, st, d, nf, u, k);
                    else if (L.cont) hipLaunchKernelGGL((k_spatial_mix_mono2<true, false>), grid, dim3(kBlock), 0, st, d, nf, u, k);
                    else if (lerp) hipLaunchKernelGGL((k_spatial_mix_mono2<false, true>), grid, dim3(kBlock), 0, st, d, nf, u, k);
                    else hipLaunchKernelGGL((k_spatial_mix_mono2<false, false>), grid, dim3(kBlock), 0, st, d, nf, u, k);
                    return;
                }
                // whole groups: slots that reach no frame (and point at something readable: the first source's first tap and entries)
                while (k % kSpGroup) tbl.d[k++] = SpDesc{tbl.d[0].data, tbl.d[0].gains, nullptr, 1u, 0u, 0u, 0u, 0.0f, 0u, tbl.d[0].g, mp::kStepNone};
                const uint64_t total = (uint64_t)nf * channels;
                const dim3 grid(rh::grid_for((size_t)total, kBlock, 256u * 16u));
                float *d = dst + j0 * channels;
                if (L.cont) hipLaunchKernelGGL(k_spatial_mix<true>, grid, dim3(kBlock), 0, st, d, channels, nf, tbl, k);
                else hipLaunchKernelGGL(k_spatial_mix<false>, grid, dim3(kBlock), 0, st, d, channels, nf, tbl, k);
            });
        RH_CHECK_LAUNCH();
        j0 += nf;
    }
    return RH_OK;
}
