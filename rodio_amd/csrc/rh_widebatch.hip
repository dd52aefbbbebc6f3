// rh_widebatch.hip -- the current block of MANY mixers of any channel count in one launch: rh_wide_mix_batch.
//     out_b[m][c] = ((0.0 + v_0[m][c]) + v_1[m][c]) + ...        per mixer b, mixer.rs:185-198, insertion order
//     v_s         = ChannelCountConverter(SampleRateConverter(Amplify(x_s)))
// k_wide_mix's arithmetic (rh_widemix.hip), operation for operation -- Amplify, the lerp in math.rs:25's order with the IEEE division, the
// verbatim last frame, the pass-through for F == T, channels.rs:59-70, the ordered sum from +0.0 -- so a mixer's block holds the bits
// rh_wide_mix_block writes for it.  One mixer's block at callback sizes is a handful of waves on 256 CUs, and a launch per mixer (per 32
// sources, per four rates) is what it costs; here the tables live in device memory -- a mixer, a source and a tile each, planned by
// rh_wide_batch_plan.h and copied in front of the launch on the same stream -- so neither the number of mixers nor the number of sources of
// a mixer multiplies launches.  A workgroup serves one tile of one mixer: what it reads of the tables is the same in every lane and arrives
// through scalar loads.  Bytes as rh_widemix.hip counts them: 4 C_s N_s per source in, 4 C M per mixer out.
#include <cstring>

#include "rh_common.h"
#include "rh_mix_dev.h"
#include "rh_wide_batch_plan.h"

namespace {

namespace wb = rh::widebatch;
namespace md = rh::mixdev;

// A pointer that was loaded from a table is a generic one to the compiler (flat loads); the rows and the destinations are device memory.
typedef const float __attribute__((address_space(1))) *global_in;
typedef float __attribute__((address_space(1))) *global_out;

// sample t of a tile: its frame and channel (c0 + t fits 32 bits where the mixer has fewer than 2^31 channels: a tile is at most 2^20 samples)
__device__ __forceinline__ void frame_of(const wb::Tile &tile, uint32_t to_ch, uint32_t t, uint32_t *j, uint32_t *c) {
    if (to_ch < (1u << 31)) {
        const uint32_t x = tile.c0 + t, dj = x / to_ch;
        *j = tile.j0 + dj, *c = x - dj * to_ch;
    } else {
        const uint64_t x = (uint64_t)tile.c0 + t, dj = x / to_ch;
        *j = tile.j0 + (uint32_t)dj, *c = (uint32_t)(x - dj * to_ch);
    }
}

// A tile of a mixer of alike sources (rh_wide_batch_plan.h: the mixer's layout, one (rate, phase) pair, no source that ends inside the block):
// k_wide_mix_uniform's walk -- the tap offset and the weight are the lane's own, once, and a source costs two loads, the lerp and the add; the
// general walk below spends ~35 vector instructions per source and sample on the cases it must tell apart.  The same operations in the same order.
template <bool LERP>
__device__ __forceinline__ void tile_uniform(global_out dst, const wb::Tile &tile, const wb::Mixer &m, const wb::Src *__restrict__ sd) {
    const uint32_t ch = m.ch;
    for (uint32_t t = threadIdx.x; t < tile.n; t += wb::kBlock) {
        uint32_t j, c;
        frame_of(tile, ch, t, &j, &c);
        const uint32_t p = m.r[0].r0 + j * m.r[0].F;  // (host: fits 32 bits)
        const uint32_t il = LERP ? p / m.r[0].T : j;
        const float w = LERP ? (float)(p - il * m.r[0].T) : 0.0f;
        const uint64_t off = (uint64_t)il * ch + c;
        float acc = 0.0f;
        for (uint32_t s0 = 0; s0 < m.src_slots; s0 += wb::kUniGroup) {  // (host: whole groups; a slot behind the last source repeats the first one: read, not added)
            float a[wb::kUniGroup], b[wb::kUniGroup], g[wb::kUniGroup];
            bool on[wb::kUniGroup];
#pragma unroll
            for (uint32_t u = 0; u < wb::kUniGroup; ++u) {
                const wb::Src d = sd[s0 + u];
                const global_in x = (global_in)d.data;
                g[u] = d.gain;
                on[u] = d.frames != 0;
                a[u] = x[on[u] ? off : 0ull];
                b[u] = LERP ? x[on[u] ? off + ch : 0ull] : 0.0f;
            }
#pragma unroll
            for (uint32_t u = 0; u < wb::kUniGroup; ++u) {
                const float v = md::amp_lerp(a[u], b[u], g[u], LERP, w, m.r[0].Tf);
                acc += on[u] ? v : 0.0f;  // (+ 0.0 leaves a sum that started at + 0.0 as it is)
            }
        }
        dst[t] = acc;
    }
}

__global__ __launch_bounds__(wb::kBlock) void k_wide_batch(const wb::Tile *__restrict__ tiles, const wb::Mixer *__restrict__ mixers, const wb::Src *__restrict__ srcs) {
    const wb::Tile tile = tiles[blockIdx.x];
    const wb::Mixer m = mixers[tile.mixer];
    const wb::Src *__restrict__ sd = srcs + m.src_first;
    {
        // (k_wide_mix: the descriptors are read through the scalar cache one after the other, and the first wave of a CU would miss on every
        //  line of them in turn.  A word of every line of this mixer's slots is asked for here, eight requests in flight at a time.)
        const uint32_t *w = reinterpret_cast<const uint32_t *>(sd);
        const uint32_t lines = (m.src_slots * (uint32_t)sizeof(wb::Src) + 63u) / 64u;
        uint32_t touch = 0;
        for (uint32_t q0 = 0; q0 < lines; q0 += 8) {
            uint32_t t[8];
#pragma unroll
            for (uint32_t u = 0; u < 8; ++u) t[u] = w[(q0 + u < lines ? q0 + u : lines - 1) * 16u];
#pragma unroll
            for (uint32_t u = 0; u < 8; ++u) touch |= t[u];
        }
        asm volatile("" ::"s"(touch));
    }
    const uint32_t to_ch = m.ch;
    const global_out dst = (global_out)m.dst + ((uint64_t)tile.j0 * to_ch + tile.c0);
    if (m.uniform) {  // (the same in every lane of the workgroup)
        if (m.r[0].F != m.r[0].T) tile_uniform<true>(dst, tile, m, sd);
        else tile_uniform<false>(dst, tile, m, sd);
        return;
    }
    for (uint32_t t = threadIdx.x; t < tile.n; t += wb::kBlock) {
        uint32_t j, c;
        frame_of(tile, to_ch, t, &j, &c);
        uint32_t il[wb::kRates];
        float w[wb::kRates];  // num as a float (math.rs:25 multiplies by it, then divides by T)
#pragma unroll
        for (uint32_t q = 0; q < wb::kRates; ++q) {
            const uint32_t p = m.r[q].r0 + j * m.r[q].F;  // (host: fits 32 bits)
            il[q] = p / m.r[q].T;
            w[q] = (float)(p - il[q] * m.r[q].T);
        }
        float acc = 0.0f;
        for (uint32_t s0 = 0; s0 < m.src_slots; s0 += wb::kGroup) {  // (host: whole groups)
            float a[wb::kGroup], b[wb::kGroup], wv[wb::kGroup], Tf[wb::kGroup], g[wb::kGroup];
            bool on[wb::kGroup], lerp[wb::kGroup];
#pragma unroll
            for (uint32_t u = 0; u < wb::kGroup; ++u) {
                const wb::Src d = sd[s0 + u];
                const uint32_t q = d.rate;
                uint32_t i;
                if (q >= wb::kOwnRate) {  // (the same in every lane) a fifth pair of its mixer: the same integers, worked out here
                    const uint32_t p = d.r0 + j * d.F;
                    i = p / d.T;
                    wv[u] = (float)(p - i * d.T);
                } else {
                    i = q == 0 ? il[0] : (q == 1 ? il[1] : (q == 2 ? il[2] : il[3]));
                    wv[u] = q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
                }
                Tf[u] = d.Tf;
                g[u] = d.gain;
                const uint32_t k = md::in_channel(c, d.ch);
                on[u] = j < d.frames && md::has_channel(c, d.ch);
                lerp[u] = on[u] && d.Tf != 0.0f && i < d.last;
                const global_in pa = (global_in)d.data + (on[u] ? (uint64_t)i * d.ch + k : 0ull);
                a[u] = *pa;
                b[u] = pa[lerp[u] ? d.ch : 0u];
            }
#pragma unroll
            for (uint32_t u = 0; u < wb::kGroup; ++u) {
                const float v = md::amp_lerp(a[u], b[u], g[u], lerp[u], wv[u], Tf[u]);
                acc += on[u] ? v : 0.0f;
            }
        }
        dst[t] = acc;
    }
}

inline size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

}  // namespace

rh_status rh_wide_mix_batch(float *const *dsts_host, const uint32_t *channels_host, const uint32_t *to_rates_host, const uint64_t *out_frames_host, const uint32_t *src_counts_host,
                            uint32_t n_mixers, const rh_wide_src *srcs_host, rh_stream stream) {
    RH_REQUIRE_INIT();
    static thread_local wb::Plan plan;  // (its vectors keep their capacity: a warmed call allocates nothing)
    // everything is decided here, before the first copy or launch: a refused batch writes nothing
    const rh_status st = wb::plan(dsts_host, channels_host, to_rates_host, out_frames_host, src_counts_host, n_mixers, srcs_host, &plan);
    if (st != RH_OK) return st;
    if (plan.tiles.empty()) return RH_OK;
    // A call that is one mixer: the table copy in front of the launch costs more than it saves (16 sources x 1 Ki or 16 Ki frames of 5.1:
    // 0.0128 / 0.0133 ms here, 0.0049 / 0.0048 ms there -- profiles/wide_batch.txt).  The same bits; what this entry refuses is refused above.
    // (Measured for sources that fit one launch of that entry; a mixer that would take several there stays here: one launch a call.)
    if (wb::one_mixer_goes_alone(plan)) return rh_wide_mix_block(dsts_host[0], channels_host[0], to_rates_host[0], out_frames_host[0], srcs_host, src_counts_host[0], stream);
    const size_t mixers_at = 0, srcs_at = pad16(plan.mixers.size() * sizeof(wb::Mixer)), tiles_at = srcs_at + pad16(plan.srcs.size() * sizeof(wb::Src));
    const size_t bytes = tiles_at + pad16(plan.tiles.size() * sizeof(wb::Tile));
    hipStream_t s = rh::as_stream(stream);
    std::unique_lock<std::mutex> hold;
    void *scratch = nullptr;
    RH_HIP_TRY(rh::stream_scratch(s, bytes, &scratch, hold));
    char *host = nullptr;  // the tables' way to the device: the stream's table ring (rh_common.h)
    RH_HIP_TRY(rh::table_stage(s, bytes, &host));
    memcpy(host + mixers_at, plan.mixers.data(), plan.mixers.size() * sizeof(wb::Mixer));
    if (!plan.srcs.empty()) memcpy(host + srcs_at, plan.srcs.data(), plan.srcs.size() * sizeof(wb::Src));
    memcpy(host + tiles_at, plan.tiles.data(), plan.tiles.size() * sizeof(wb::Tile));
    RH_HIP_TRY(rh::table_send(s, scratch));
    const char *base = static_cast<const char *>(scratch);
    hipLaunchKernelGGL(k_wide_batch, dim3((uint32_t)plan.tiles.size()), dim3(wb::kBlock), 0, s, reinterpret_cast<const wb::Tile *>(base + tiles_at),
                       reinterpret_cast<const wb::Mixer *>(base + mixers_at), reinterpret_cast<const wb::Src *>(base + srcs_at));
    RH_CHECK_LAUNCH();
    return RH_OK;
}
