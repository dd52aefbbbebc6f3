// rh_loopmix.hip -- a block of a mixer whose sources may be LOOPS, source.repeat_infinite() (repeat.rs:15-26), read from ONE resident pass:
//     out[m][c] = ((0.0 + v_0[m][c]) + v_1[m][c]) + ...                                                 mixer.rs:185-198, insertion order
//     v_s       = ChannelCountConverter(SampleRateConverter(Amplify(x_s)))                              uniform.rs:58-67, amplify.rs:64
// Repeat sits on Buffered (repeat.rs:19-23), and UniformSourceIterator re-builds its converter chain from what those two report
// (uniform.rs:56), so a loop is NOT a modulo on the tap index: chains either start over at every pass (rule 0) or run on across the seam in
// steps of 32768 samples of the unrolled stream (rule 1) -- rh_loop_mix_plan.h states both and holds locate(), the position of an output
// frame's taps, as plain 32-bit arithmetic over per-source constants: three or four divisions by constants a source and sample, each an exact
// multiply-high reciprocal worked out on the host.  The kernel is k_wide_mix's shape around it: a lane per output SAMPLE walks the sources in
// insertion order, groups of four whose tap loads leave together; per tap
//     i <  the chain's last frame :  a + (b - a) * num / T      (math.rs:25; a, b: the taps behind x * gain)
//     otherwise                   :  a, verbatim (sample_rate.rs:193-200);   F == T: a (sample_rate.rs:133-136)
// with the channel rule of channels.rs:59-70: the reference's rounding sequence, bit for bit.  A source that is not a loop (loop_frames == 0)
// is the same descriptor with quotients that answer 0: k_wide_mix's arithmetic.  The table travels by value as a kernel argument (32 sources
// a launch; more continue from the stored partial sum).
#include "rh_common.h"
#include "rh_loop_mix_plan.h"

namespace {

namespace lm = rh::loopmix;

constexpr int kBlock = 256;
constexpr int kGroup = (int)lm::kGroup;

struct LoopTable {
    lm::Desc d[lm::kChunk];
};
static_assert(sizeof(LoopTable) + 64 <= 4096, "the table and the other arguments share one 4 KiB kernel-argument segment");

// One lane per output SAMPLE, as k_wide_mix: coalesced stores for any layout, and loads that are coalesced wherever a wave lies inside a
// chain.  A source that does not reach the sample -- it is silent there, or the channel is one it does not have -- reads its own first
// float and adds +0.0, which leaves a sum that started at +0.0 as it is; a tap that is not taken (verbatim frame, F == T) reads the first
// one again.
template <bool CONT>
__global__ __launch_bounds__(kBlock) void k_loop_mix(float *__restrict__ dst, uint32_t to_ch, uint32_t out_frames, const LoopTable tbl, uint32_t n_sources) {
    const uint64_t total = (uint64_t)out_frames * to_ch;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    {
        // (k_wide_mix: the table is read through the scalar cache, and the first wave of a CU would miss on its lines one after the
        //  other.  One word of every line is asked for here, all requests in flight at once.)
        const uint32_t *w = reinterpret_cast<const uint32_t *>(&tbl);
        constexpr uint32_t kLines = (sizeof(LoopTable) + 63) / 64;
        uint32_t t[kLines], touch = 0;
#pragma unroll
        for (uint32_t q = 0; q < kLines; ++q) t[q] = w[q * 16u];
#pragma unroll
        for (uint32_t q = 0; q < kLines; ++q) touch |= t[q];
        asm volatile("" ::"s"(touch));
    }
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += stride) {
        const uint32_t m = (uint32_t)(o / to_ch);
        const uint32_t c = (uint32_t)(o - (uint64_t)m * to_ch);
        float acc = CONT ? dst[o] : 0.0f;
        for (uint32_t s0 = 0; s0 < n_sources; s0 += kGroup) {  // (host: n_sources is a whole number of groups)
            float a[kGroup], b[kGroup], wv[kGroup];
            bool on[kGroup], lerp[kGroup];
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const lm::Desc &d = tbl.d[s0 + u];
                const lm::Taps t = lm::locate(d, m);
                wv[u] = (float)t.num;  // math.rs:25 multiplies by it, then divides by T
                const uint32_t k = c < d.ch ? c : 0u;                          // channels.rs:59-70: k < from: the input channel; k == 1 of a mono source: its only one;
                on[u] = m < d.frames && (c < d.ch || (c == 1u && d.ch == 1u));  // otherwise 0.0
                lerp[u] = on[u] && t.lerp;
                const uint32_t ia = on[u] ? t.ia : 0u, ib = lerp[u] ? t.ib : ia;
                a[u] = d.data[(uint64_t)ia * d.ch + (on[u] ? k : 0u)];
                b[u] = d.data[(uint64_t)ib * d.ch + (on[u] ? k : 0u)];
            }
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const lm::Desc &d = tbl.d[s0 + u];
                const float x = a[u] * d.gain;  // Amplify (amplify.rs:64) in front of the converter
                float v = x;
                if (lerp[u]) {
                    const float y = b[u] * d.gain;
                    v = x + (y - x) * wv[u] / d.Tf;
                }
                acc += on[u] ? v : 0.0f;
            }
        }
        dst[o] = acc;
    }
}

}  // namespace

rh_status rh_loop_plan(uint64_t n_samples, uint32_t channels, uint64_t span_len, uint64_t *words) { return lm::loop_plan(n_samples, channels, span_len, words); }

rh_status rh_loop_advance(uint64_t *words, uint32_t from_rate, uint32_t to_rate, uint64_t out_frames) { return lm::loop_advance(words, from_rate, to_rate, out_frames); }

rh_status rh_loop_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs_host, uint32_t n_sources, const uint64_t *loops_host,
                            rh_stream stream) {
    RH_REQUIRE_INIT();
    if (out_frames == 0) return RH_OK;
    // Everything is checked before the first launch: a call that fails has written nothing.
    const rh_status ok = lm::check(dst, channels, to_rate, out_frames, srcs_host, n_sources, loops_host);
    if (ok != RH_OK) return ok;
    hipStream_t st = rh::as_stream(stream);
    const uint32_t nf = (uint32_t)out_frames;
    lm::walk(srcs_host, n_sources, [&](const lm::Launch &L) {
        LoopTable tbl;
        uint32_t k = 0;
        for (; k < L.n; ++k) (void)lm::describe(srcs_host[L.src[k]], loops_host + (size_t)RH_LOOP_WORDS * L.src[k], channels, to_rate, out_frames, &tbl.d[k]);
        // whole groups: slots that reach no frame (and point at something readable: the first source's first tap, or dst where there is no source)
        const float *readable = L.n ? tbl.d[0].data : dst;
        while (k % lm::kGroup) tbl.d[k++] = lm::pad_slot(readable);
        for (uint32_t q = k; q < lm::kChunk; ++q) tbl.d[q] = lm::pad_slot(readable);  // (behind n_sources: touched, not walked)
        const uint64_t total = (uint64_t)nf * channels;
        const dim3 grid(rh::grid_for((size_t)total, kBlock, 256u * 16u));
        if (L.cont) hipLaunchKernelGGL(k_loop_mix<true>, grid, dim3(kBlock), 0, st, dst, channels, nf, tbl, k);
        else hipLaunchKernelGGL(k_loop_mix<false>, grid, dim3(kBlock), 0, st, dst, channels, nf, tbl, k);
    });
    RH_CHECK_LAUNCH();
    return RH_OK;
}
