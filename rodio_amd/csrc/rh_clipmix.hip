// rh_clipmix.hip -- a block of a mixer whose sources may be CLIPS ON A TIMELINE, a resident sound that starts after a delay, is cut to a
// duration and may fade out over it:
//     mixer.add(sound.amplify(g).take_duration(len) /* .set_filter_fadeout() */ .delay(at))       delay.rs, take.rs, amplify.rs:64
//     out[m][c] = ((0.0 + v_0[m][c]) + v_1[m][c]) + ...                                                 mixer.rs:185-198, insertion order
//     v_s       = ChannelCountConverter(SampleRateConverter(stream of the clip))                        uniform.rs:58-67
// A clip is NOT "zeros, then the converted sound": the stream is Z samples of +0.0 and then the admitted samples, read as frames BY STREAM
// POSITION (an odd Z shifts a stereo sound by one channel), and UniformSourceIterator cuts it into converter chains at every multiple of
// 32768 samples from the stream's start (rule G) or not at all (rule C) -- rh_clip_mix_plan.h states both and holds locate(), the position
// of an output frame's taps counted from the chain in progress at the block's first frame, as 32-bit arithmetic over per-source constants
// with exact multiply-high reciprocals, and fade_ms(), the fade-out's millisecond step of ONE tap: the two taps of a lerp may lie on either
// side of a step, so each carries its own factor.  No position here depends on Z or on how long the clip has played.
// The kernel is k_loop_mix's shape: a lane per output SAMPLE walks the sources in insertion order, groups of four whose tap loads leave
// together; per tap, with s its stream sample counted from the chain in progress,
//     s <  zrel :  +0.0, as Delay emits it: no gain, no fade (delay.rs:68-75)
//     otherwise :  (x[s - zrel] * gain) [* R / Tt]                                      amplify.rs:64, take.rs:33-41: mul, then the IEEE divide
// then    i <  the chain's last frame :  a + (b - a) * num / T                                  math.rs:25
//         otherwise                   :  a, verbatim (sample_rate.rs:193-200);   F == T: a (sample_rate.rs:133-136)
// and the channel rule of channels.rs:59-70.
// CHAINS THAT LIE WHOLLY IN THE DELAY are not skipped and need not be: both taps are +0.0, the lerp gives 0 + (0 - 0) * num / T = +0.0, and
// the sum, which starts at +0.0 and is never -0.0, is left as it is by + +0.0.  Their taps load nothing -- a lane whose tap lies in the delay
// issues no load --, so they cost positions only, and the number of launches stays a function of the number of sources.  A source that is
// not a clip is the same descriptor with zrel = 0 and one chain: k_wide_mix's arithmetic.  The table travels by value as a kernel argument
// (32 sources a launch; more continue from the stored partial sum).
#include "rh_common.h"
#include "rh_clip_mix_plan.h"
#include "rh_mix_dev.h"

namespace {

namespace cm = rh::clipmix;
namespace md = rh::mixdev;

constexpr int kBlock = 256;
constexpr int kGroup = (int)cm::kGroup;

struct ClipTable {
    cm::Desc d[cm::kChunk];
};
static_assert(sizeof(ClipTable) + 64 <= 4096, "the table and the other arguments share one 4 KiB kernel-argument segment");

template <bool CONT>
__global__ __launch_bounds__(kBlock) void k_clip_mix(float *__restrict__ dst, uint32_t to_ch, uint32_t out_frames, const ClipTable tbl, uint32_t n_sources) {
    const uint64_t total = (uint64_t)out_frames * to_ch;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    md::touch_table(tbl);  // (the first wave of a CU would miss on the table's lines one after the other)
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += stride) {
        const uint32_t m = (uint32_t)(o / to_ch);
        const uint32_t c = (uint32_t)(o - (uint64_t)m * to_ch);
        float acc = CONT ? dst[o] : 0.0f;
        for (uint32_t s0 = 0; s0 < n_sources; s0 += kGroup) {  // (host: n_sources is a whole number of groups)
            float a[kGroup], b[kGroup], wv[kGroup];
            uint64_t ka[kGroup];  // the first tap's sample of the sound, counted from data (the second one's is ka + ch)
            bool on[kGroup], lerp[kGroup], ra[kGroup], rb[kGroup];
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const cm::Desc &d = tbl.d[s0 + u];
                const cm::Taps t = cm::locate(d, m);
                wv[u] = (float)t.num;  // math.rs:25 multiplies by it, then divides by T
                const uint32_t k = md::in_channel(c, d.ch);
                on[u] = m < d.frames && md::has_channel(c, d.ch);
                lerp[u] = on[u] && t.lerp;
                const uint64_t sa = cm::tap_sample(d, t.ia, k), sb = sa + d.ch;  // stream samples, counted from the chain in progress
                ra[u] = on[u] && sa >= d.zrel;                       // in front of zrel: the delay's +0.0, nothing is loaded
                rb[u] = lerp[u] && sb >= d.zrel;
                ka[u] = sa - d.zrel;  // (in front of zrel: wrapped, and not used; ka + ch is right again where only the second tap is read)
                a[u] = ra[u] ? d.data[ka[u]] : 0.0f;
                b[u] = rb[u] ? d.data[ka[u] + d.ch] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const cm::Desc &d = tbl.d[s0 + u];
                // Amplify (amplify.rs:64), then the fade-out of the tap's OWN millisecond (take.rs:33-41), in front of the converter
                float x = ra[u] ? a[u] * d.gain : 0.0f;
                float y = rb[u] ? b[u] * d.gain : 0.0f;
                if (d.fade != cm::kNoFade) {
                    if (ra[u]) x = x * cm::fade_ms(d, (uint32_t)ka[u]) / d.Ttf;  // (a clip: below 2^32)
                    if (rb[u]) y = y * cm::fade_ms(d, (uint32_t)ka[u] + d.ch) / d.Ttf;
                }
                float v = x;
                if (lerp[u]) v = x + (y - x) * wv[u] / d.Tf;
                acc += on[u] ? v : 0.0f;
            }
        }
        dst[o] = acc;
    }
}

}  // namespace

rh_status rh_clip_plan(uint64_t *words, uint64_t n_samples, uint32_t channels, uint32_t rate, uint64_t span_len, uint64_t delay_ns, uint64_t take_ns, uint32_t flags) {
    return cm::clip_plan(words, n_samples, channels, rate, span_len, delay_ns, take_ns, flags);
}

rh_status rh_clip_advance(uint64_t *words, uint32_t channels, uint32_t from_rate, uint32_t to_rate, uint64_t out_frames) {
    return cm::clip_advance(words, channels, from_rate, to_rate, out_frames);
}

rh_status rh_clip_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs_host, uint32_t n_sources, const uint64_t *clips_host,
                            rh_stream stream) {
    RH_REQUIRE_INIT();
    if (out_frames == 0) return RH_OK;
    // Everything is checked before the first launch: a call that fails has written nothing.
    const rh_status ok = cm::check(dst, channels, to_rate, out_frames, srcs_host, n_sources, clips_host);
    if (ok != RH_OK) return ok;
    hipStream_t st = rh::as_stream(stream);
    const uint32_t nf = (uint32_t)out_frames;
    cm::walk(srcs_host, n_sources, [&](const cm::Launch &L) {
        ClipTable tbl;
        uint32_t k = 0;
        for (; k < L.n; ++k) (void)cm::describe(srcs_host[L.src[k]], clips_host + (size_t)RH_CLIP_WORDS * L.src[k], channels, to_rate, out_frames, &tbl.d[k]);
        for (uint32_t q = k; q < cm::kChunk; ++q) tbl.d[q] = cm::pad_slot();  // whole groups, and behind n_sources: touched, not walked
        while (k % cm::kGroup) ++k;
        const uint64_t total = (uint64_t)nf * channels;
        const dim3 grid(rh::grid_for((size_t)total, kBlock, 256u * 16u));
        if (L.cont) hipLaunchKernelGGL(k_clip_mix<true>, grid, dim3(kBlock), 0, st, dst, channels, nf, tbl, k);
        else hipLaunchKernelGGL(k_clip_mix<false>, grid, dim3(kBlock), 0, st, dst, channels, nf, tbl, k);
    });
    RH_CHECK_LAUNCH();
    return RH_OK;
}
