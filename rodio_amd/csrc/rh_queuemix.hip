// rh_queuemix.hip -- a block of a mixer whose sources may be QUEUES of resident sounds played back to back (src/queue.rs; what Player::append
// feeds its mixer), in one launch:
//     out[m][c] = ((0.0 + v_0[m][c]) + v_1[m][c]) + ...                                                 mixer.rs:185-198, insertion order
//     v_s       = ChannelCountConverter(SampleRateConverter(queue of Amplify(x_k)))                     uniform.rs:58-67, amplify.rs:64
// UniformSourceIterator cuts its converter chains from what the queue reports when the previous chain runs dry (uniform.rs:56,
// queue.rs:130-192, buffer.rs:76-82), so a chain may run across sounds of other formats and lerp across the seams: rh_queue_mix_plan.h
// states the rule and turns (sounds, cursor, block) into two flat tables -- SEGMENTS, runs of output frames that lie in one chain, and
// PIECES, runs of a chain's samples that lie in one sound (or are the +0.0 of a keep-alive tail).  The kernel knows only those: a lane per
// output SAMPLE walks the sources in insertion order; per source its wave finds the segments by output frame, a lane its taps by locate(),
// the wave the pieces of the taps by sample index, and then a lane does what k_wide_mix does:
//     i <  the chain's last frame :  a + (b - a) * num / T      (math.rs:25; a, b: the taps behind x * gain of THEIR sound)
//     otherwise                   :  a, verbatim (sample_rate.rs:193-200);   F == T: a (sample_rate.rs:133-136)
// with the channel rule of channels.rs:59-70: the reference's rounding sequence, bit for bit.  A plain source is one segment of one piece.
// The tables live in device memory: one copy in front of the launch on the same stream, as rh_wide_mix_batch takes its tables there, so
// neither sources nor sounds nor seams multiply launches.
#include <cstring>

#include "rh_common.h"
#include "rh_mix_dev.h"
#include "rh_queue_mix_plan.h"

namespace {

namespace qm = rh::queuemix;
namespace md = rh::mixdev;

constexpr int kBlock = 256;

// A pointer that was loaded from a table is a generic one to the compiler (flat loads); the sounds are device memory.
typedef const float __attribute__((address_space(1))) *global_in;

// The samples [start, end) of a chain that piece k of n holds.
struct Span {
    qm::Piece p;
    uint32_t end;
};
__device__ __forceinline__ Span span_of(const qm::Piece *__restrict__ p, uint32_t n, uint32_t k) { return Span{p[k], k + 1u < n ? p[k + 1u].start : 0xffffffffu}; }

// One lane per output SAMPLE, as k_wide_mix and k_loop_mix: coalesced stores for any layout, and loads that are coalesced wherever a wave
// lies inside a piece.  The lanes of a wave hold consecutive samples, so their output frames -- and with them their frames inside a chain --
// do not decrease from lane to lane: a wave lies in one segment and one piece except at a seam.  The tables are therefore walked PER WAVE:
// the segment of the first lane, then the following ones while a lane lies behind; inside a segment the piece of the first lane's frame,
// then the following ones while a tap lies behind.  Every index is the same in all lanes (__builtin_amdgcn_readfirstlane, __any), so what
// is read of the tables arrives through scalar loads, and the taps are the only vector loads.  A source that does not reach the sample --
// it is silent there, or the channel is one it does not have -- adds +0.0, which leaves a sum that started at +0.0 as it is.
__global__ __launch_bounds__(kBlock) void k_queue_mix(float *__restrict__ dst, uint32_t to_ch, uint32_t out_frames, const qm::Src *__restrict__ srcs, const qm::Seg *__restrict__ segs,
                                                     const qm::Piece *__restrict__ pieces, uint32_t n_sources) {
    const uint64_t total = (uint64_t)out_frames * to_ch;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += stride) {
        const uint32_t m = (uint32_t)(o / to_ch);
        const uint32_t c = (uint32_t)(o - (uint64_t)m * to_ch);
        const uint32_t m_first = __builtin_amdgcn_readfirstlane(m);  // (the smallest of the wave)
        float acc = 0.0f;
        for (uint32_t s = 0; s < n_sources; ++s) {
            const qm::Src d = srcs[s];
            float v = 0.0f;
            if (d.seg_count) {
                const qm::Seg *__restrict__ gs = segs + d.seg_first;
                // the first segment that ends behind the wave's first frame
                uint32_t q = 0;
                if (d.seg_count > 1u) {
                    uint32_t hi = d.seg_count;
                    while (q < hi) {
                        const uint32_t mid = (q + hi) >> 1;
                        if (gs[mid].m0 + gs[mid].count <= m_first) q = mid + 1u;
                        else hi = mid;
                    }
                }
                for (; q < d.seg_count; ++q) {
                    const qm::Seg g = gs[q];
                    if (m - g.m0 < g.count && md::has_channel(c, g.ch)) {
                        const qm::Taps t = qm::locate(g, m);
                        const uint64_t ea = (uint64_t)t.i * g.ch + md::in_channel(c, g.ch), eb = t.lerp ? ea + g.ch : ea;
                        const qm::Piece *__restrict__ p = pieces + g.piece_first;
                        float x = 0.0f, y = 0.0f;  // (the +0.0 of a keep-alive tail meets no gain)
                        if (g.piece_count == 1u) {  // (a plain source, or a chain inside one sound: the indices may leave 32 bits)
                            const qm::Piece pc = p[0];
                            if (pc.data) {
                                x = ((global_in)pc.data)[ea] * pc.gain;  // Amplify (amplify.rs:64) in front of the converter
                                y = ((global_in)pc.data)[eb] * pc.gain;
                            }
                        } else {
                            // the piece of the first lane's frame (no tap of the wave lies in front of its channel 0), then on while a tap lies behind
                            uint32_t k = qm::find_piece(p, g.piece_count, (uint64_t)__builtin_amdgcn_readfirstlane(t.i) * g.ch);
                            for (; k < g.piece_count; ++k) {
                                const Span sp = span_of(p, g.piece_count, k);
                                if (sp.p.data) {
                                    if (ea >= sp.p.start && ea < sp.end) x = ((global_in)sp.p.data)[ea - sp.p.start] * sp.p.gain;
                                    if (eb >= sp.p.start && eb < sp.end) y = ((global_in)sp.p.data)[eb - sp.p.start] * sp.p.gain;
                                }
                                if (!__any(eb >= sp.end)) break;
                            }
                        }
                        v = t.lerp ? x + (y - x) * (float)t.num / g.Tf : x;  // math.rs:25: multiply, IEEE divide, add
                    }
                    if (!__any(m >= g.m0 + g.count)) break;
                }
            }
            acc += v;
        }
        dst[o] = acc;
    }
}

inline size_t pad64(size_t bytes) { return (bytes + 63) & ~(size_t)63; }

}  // namespace

rh_status rh_queue_plan(uint64_t *words, uint32_t keep_alive) { return qm::queue_plan(words, keep_alive); }

rh_status rh_queue_advance(uint64_t *words, const uint64_t *sounds_host, uint32_t n_sounds, uint32_t to_rate, uint64_t out_frames, uint32_t *dropped) {
    return qm::queue_advance(words, sounds_host, n_sounds, to_rate, out_frames, dropped);
}

rh_status rh_queue_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs_host, uint32_t n_sources, const uint64_t *sounds_host,
                             const float *sound_gains_host, const uint32_t *sound_counts_host, const uint64_t *cursors_host, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (out_frames == 0) return RH_OK;
    static thread_local qm::Plan plan;  // (its vectors keep their capacity: a warmed call allocates nothing)
    // everything is decided here, before the copy and the launch: a refused call writes nothing
    const rh_status ok = qm::plan(dst, channels, to_rate, out_frames, srcs_host, n_sources, sounds_host, sound_gains_host, sound_counts_host, cursors_host, &plan);
    if (ok != RH_OK) return ok;
    hipStream_t s = rh::as_stream(stream);
    const uint32_t nf = (uint32_t)out_frames;
    const uint64_t total = (uint64_t)nf * channels;
    const dim3 grid(rh::grid_for((size_t)total, kBlock, 256u * 16u));
    if (plan.segs.empty()) {  // no source reaches the block: zeros, and no table to take along
        hipLaunchKernelGGL(k_queue_mix, grid, dim3(kBlock), 0, s, dst, channels, nf, (const qm::Src *)nullptr, (const qm::Seg *)nullptr, (const qm::Piece *)nullptr, 0u);
        RH_CHECK_LAUNCH();
        return RH_OK;
    }
    const size_t segs_at = pad64(plan.srcs.size() * sizeof(qm::Src)), pieces_at = segs_at + plan.segs.size() * sizeof(qm::Seg);
    const size_t bytes = pad64(pieces_at + plan.pieces.size() * sizeof(qm::Piece));
    std::unique_lock<std::mutex> hold;
    void *scratch = nullptr;
    RH_HIP_TRY(rh::stream_scratch(s, bytes, &scratch, hold));
    char *host = nullptr;  // the tables' way to the device: the stream's table ring (rh_common.h)
    RH_HIP_TRY(rh::table_stage(s, bytes, &host));
    memcpy(host, plan.srcs.data(), plan.srcs.size() * sizeof(qm::Src));
    memcpy(host + segs_at, plan.segs.data(), plan.segs.size() * sizeof(qm::Seg));
    memcpy(host + pieces_at, plan.pieces.data(), plan.pieces.size() * sizeof(qm::Piece));
    RH_HIP_TRY(rh::table_send(s, scratch));
    const char *base = static_cast<const char *>(scratch);
    hipLaunchKernelGGL(k_queue_mix, grid, dim3(kBlock), 0, s, dst, channels, nf, reinterpret_cast<const qm::Src *>(base), reinterpret_cast<const qm::Seg *>(base + segs_at),
                       reinterpret_cast<const qm::Piece *>(base + pieces_at), n_sources);
    RH_CHECK_LAUNCH();
    return RH_OK;
}
