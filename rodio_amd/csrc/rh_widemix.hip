// rh_widemix.hip -- a block of a mixer of ANY channel count in one launch (round 6):
//     out[m][c] = ((0.0 + v_0[m][c]) + v_1[m][c]) + ...                                        mixer.rs:185-198, insertion order
//     v_s       = ChannelCountConverter(SampleRateConverter(Amplify(x_s)))                     uniform.rs:58-67, amplify.rs:64
// for continuous sources (current_span_len() == None: one converter for the whole stream, uniform.rs:56) of any rate and layout.
// Until now a mixer of more than two channels (mixer::mixer(nz!(6), rate), mixer.rs:25) ran every source as a chain of its own --
// an amplify launch, a converter launch, a device copy per source and block -- and rh_mix_sum added the rows.  Here the converter
// is a pure function of the output frame, as everywhere in this library:
//     i = floor(m F / T), num = (m F) mod T     (F / T = from / to reduced, sample_rate.rs:74)
//     i <= N - 2 :  a + (b - a) * num / T       (math.rs:25, in that order; a = g x[i][k], b = g x[i+1][k])
//     i == N - 1 :  a, verbatim, and the source is over (sample_rate.rs:193-200)
//     F == T     :  a (sample_rate.rs:133-136: the converter passes every sample through)
// followed by channels.rs:59-70 (k < from: the input channel; k == 1 of a narrower source: its first channel; otherwise 0.0,
// which leaves an f32 sum that started at +0.0 as it is) -- so one lane per output SAMPLE walks the sources in insertion order
// and adds: the reference's rounding sequence, bit for bit, with fully coalesced loads and stores.  HBM-bound: every input byte
// is read once from memory (the second tap of a frame is the first tap of the next: L1 / L2), 4 S C_s N_s bytes in, 4 C M out.
// The source table travels by value as a kernel argument (32 sources a launch; more continue from the stored partial sum).
#include <cstring>
#include <vector>

#include "rh_common.h"
#include "rh_mix_dev.h"
#include "rh_mix_plan.h"

namespace {

namespace mp = rh::mixplan;
namespace md = rh::mixdev;

constexpr int kBlock = 256;
constexpr uint32_t kWideChunk = mp::kChunk;  // sources a launch
constexpr int kWideGroup = (int)mp::kGroup;  // ... walked in groups of this many, whose tap loads leave together
constexpr uint32_t kWideRates = mp::kRates;  // ... of at most this many different (rate, phase) pairs: the position of an output frame between its taps is worked out once per pair
using WideRate = mp::Rate;

struct WideDesc {
    const float *data;  // the frame that holds the first tap of the launch's first output frame
    uint32_t ch;        // channels of the source
    uint32_t frames;    // output frames of this launch the source reaches (0: a slot that pads the table to whole groups)
    uint32_t last;      // ended sources: index (relative to data) of the LAST frame; live ones: 0xffffffff
    uint32_t rate;      // index into WideTable::r
    float gain;
    float Tf;           // T of its rate as a float; 0: the converter passes through (F == T, sample_rate.rs:133-136)
};
struct WideTable {
    WideRate r[kWideRates];
    WideDesc d[kWideChunk];
};

// The sources are walked in groups of kWideGroup whose loads leave together: a lane's additions stay in insertion order (the reference's rounding
// sequence), but nothing about one source's taps depends on the sum so far.  A source that does not reach the sample -- it has ended, or the
// channel is one it does not have -- reads its own first float and adds +0.0, which leaves a sum that started at +0.0 as it is.
template <bool CONT>
__global__ __launch_bounds__(kBlock) void k_wide_mix(float *__restrict__ dst, uint32_t to_ch, uint32_t out_frames, const WideTable tbl, uint32_t n_sources) {
    const uint64_t total = (uint64_t)out_frames * to_ch;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    md::touch_table(tbl);  // (the first wave of a CU would miss on the table's lines one after the other)
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += stride) {
        const uint32_t j = (uint32_t)(o / to_ch);
        const uint32_t c = (uint32_t)(o - (uint64_t)j * to_ch);
        uint32_t il[kWideRates];
        float w[kWideRates];  // num as a float (math.rs:25 multiplies by it, then divides by T)
#pragma unroll
        for (uint32_t q = 0; q < kWideRates; ++q) {
            const uint32_t p = tbl.r[q].r0 + j * tbl.r[q].F;  // (host: fits 32 bits)
            il[q] = p / tbl.r[q].T;
            w[q] = (float)(p - il[q] * tbl.r[q].T);
        }
        float acc = CONT ? dst[o] : 0.0f;
        // (two groups in flight -- the taps of the group behind requested before the group in front is added -- and groups of eight were
        //  measured: no faster.  At block sizes a launch is a few waves per CU walking the table; 0.27 us per source is their instruction stream.)
        for (uint32_t s0 = 0; s0 < n_sources; s0 += kWideGroup) {  // (host: n_sources is a whole number of groups)
            float a[kWideGroup], b[kWideGroup], wv[kWideGroup], Tf[kWideGroup], g[kWideGroup];
            bool on[kWideGroup], lerp[kWideGroup];
#pragma unroll
            for (int u = 0; u < kWideGroup; ++u) {
                const WideDesc d = tbl.d[s0 + u];
                const uint32_t q = d.rate;
                const uint32_t i = q == 0 ? il[0] : (q == 1 ? il[1] : (q == 2 ? il[2] : il[3]));
                wv[u] = q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
                Tf[u] = d.Tf;
                g[u] = d.gain;
                const uint32_t k = md::in_channel(c, d.ch);
                on[u] = j < d.frames && md::has_channel(c, d.ch);
                lerp[u] = on[u] && d.Tf != 0.0f && i < d.last;
                const float *pa = d.data + (on[u] ? (uint64_t)i * d.ch + k : 0ull);
                a[u] = *pa;
                b[u] = pa[lerp[u] ? d.ch : 0u];
            }
#pragma unroll
            for (int u = 0; u < kWideGroup; ++u) {
                const float v = md::amp_lerp(a[u], b[u], g[u], lerp[u], wv[u], Tf[u]);
                acc += on[u] ? v : 0.0f;
            }
        }
        dst[o] = acc;
    }
}

// ---- the uniform case: every source of the launch has the mixer's channel count and ONE rate, and reaches every frame of the launch with both
// taps (no source ends inside it).  Then the tap offset and the weight are the lane's own, once, and a source costs two loads, the lerp and
// the add: what a mixer of many alike sources runs (k_wide_mix spends ~35 vector instructions per source and sample on the cases it must
// tell apart, which is what bounds it at scale: 0.41 of the roofline for 256 stereo sources).  The same operations in the same order.
struct WideUniSrc {
    const float *data;
    float gain;
    uint32_t pad;
};
struct WideUniTable {
    uint32_t F, T, r0, ch;
    float Tf;
    uint32_t pad[3];
    WideUniSrc d[kWideChunk];
};
constexpr int kUniGroup = 8;  // sources whose taps are in flight together (sixteen loads a lane; four: 0.44 of the roofline at 64 x 64 Ki frames of 5.1, eight: see profiles/r06_bench_wide.txt)
template <bool CONT, bool LERP>
__global__ __launch_bounds__(kBlock) void k_wide_mix_uniform(float *__restrict__ dst, uint32_t out_frames, const WideUniTable tbl, uint32_t n_sources) {
    const uint32_t ch = tbl.ch;
    const uint64_t total = (uint64_t)out_frames * ch;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += stride) {
        const uint32_t j = (uint32_t)(o / ch);
        const uint32_t c = (uint32_t)(o - (uint64_t)j * ch);
        const uint32_t p = tbl.r0 + j * tbl.F;
        const uint32_t il = LERP ? p / tbl.T : j;
        const float w = LERP ? (float)(p - il * tbl.T) : 0.0f;
        const uint64_t off = (uint64_t)il * ch + c;
        float acc = CONT ? dst[o] : 0.0f;
        uint32_t nv = n_sources;
        asm volatile("" : "+v"(nv));  // (a vector register: "is this slot a source" below is a select, not a branch that would split the group's loads)
        for (uint32_t s0 = 0; s0 < n_sources; s0 += kUniGroup) {  // (the slots behind the last source of a short last group repeat the first source: read, not added)
            float a[kUniGroup], b[kUniGroup], g[kUniGroup];
#pragma unroll
            for (int u = 0; u < kUniGroup; ++u) {
                const WideUniSrc d = tbl.d[s0 + u];
                g[u] = d.gain;
                a[u] = d.data[off];
                b[u] = LERP ? d.data[off + ch] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < kUniGroup; ++u) {
                const float v = md::amp_lerp(a[u], b[u], g[u], LERP, w, tbl.Tf);
                acc += s0 + u < nv ? v : 0.0f;  // (+ 0.0 leaves a sum that started at + 0.0 as it is)
            }
        }
        dst[o] = acc;
    }
}

// ---- sources of a launch converted into ROWS instead of a sum (rh_wide_mix_block_filtered: a filter sits between the converter and the mix).
// k_wide_mix's arithmetic -- Amplify, the lerp in math.rs:25's order with the IEEE division, the verbatim last frame, the pass-through
// for F == T, channels.rs:59-70 -- stored per source: one lane per output sample of the rows of ONE GROUP of kWideGroup sources (blockIdx.y),
// whose tap loads leave together; a wave's store to a row is 256 contiguous bytes.  A source that reaches fewer frames than the block
// writes only those.  The first workgroup of a group also copies its sources' carried filter states (4 floats a channel; NULL: zeros)
// to where the filter's batches expect them side by side.
struct WideRowDesc {
    const float *data;   // as WideDesc::data
    float *row;          // out_frames x to_ch floats of the mixer's layout (a slot that pads the table: not written, frames == 0)
    const float *state;  // the source's carried state, or nullptr
    float *state_row;    // where the filter reads it (nullptr: no state is carried in this call)
    uint32_t ch, frames, last, rate;
    float gain, Tf;
};
struct WideRowTable {
    WideRate r[kWideRates];
    WideRowDesc d[kWideChunk];
};
__global__ __launch_bounds__(kBlock) void k_wide_rows(uint32_t to_ch, uint32_t out_frames, const WideRowTable tbl) {
    const uint64_t total = (uint64_t)out_frames * to_ch;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint32_t s0 = blockIdx.y * kWideGroup;
    {
        // (k_wide_mix: the table is read through the scalar cache, and the first wave of a CU would miss on its lines one after the other.
        //  This workgroup reads the rates and its own group's descriptors: a word of each of those lines, all in flight at once.)
        const uint32_t *w = reinterpret_cast<const uint32_t *>(&tbl);
        constexpr uint32_t kLines = (sizeof(WideRowTable) + 63) / 64;
        constexpr uint32_t kMine = (kWideGroup * sizeof(WideRowDesc) + 63) / 64 + 1;  // lines a group's descriptors can touch
        const uint32_t q0 = (uint32_t)((sizeof(WideRate) * kWideRates + s0 * sizeof(WideRowDesc)) / 64);
        uint32_t t[kMine + 1], touch = 0;
        t[kMine] = w[0];
#pragma unroll
        for (uint32_t q = 0; q < kMine; ++q) t[q] = w[(q0 + q < kLines ? q0 + q : kLines - 1) * 16u];
#pragma unroll
        for (uint32_t q = 0; q <= kMine; ++q) touch |= t[q];
        asm volatile("" ::"s"(touch));
    }
    if (blockIdx.x == 0) {
#pragma unroll
        for (int u = 0; u < kWideGroup; ++u) {
            const WideRowDesc d = tbl.d[s0 + u];
            if (d.state_row)
                for (uint32_t t = threadIdx.x; t < 4u * to_ch; t += kBlock) d.state_row[t] = d.state ? d.state[t] : 0.0f;
        }
    }
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += stride) {
        const uint32_t j = (uint32_t)(o / to_ch);
        const uint32_t c = (uint32_t)(o - (uint64_t)j * to_ch);
        uint32_t il[kWideRates];
        float w[kWideRates];  // num as a float (math.rs:25 multiplies by it, then divides by T)
#pragma unroll
        for (uint32_t q = 0; q < kWideRates; ++q) {
            const uint32_t p = tbl.r[q].r0 + j * tbl.r[q].F;  // (host: fits 32 bits)
            il[q] = p / tbl.r[q].T;
            w[q] = (float)(p - il[q] * tbl.r[q].T);
        }
        float a[kWideGroup], b[kWideGroup], wv[kWideGroup], Tf[kWideGroup], g[kWideGroup];
        float *row[kWideGroup];
        bool reach[kWideGroup], on[kWideGroup], lerp[kWideGroup];
#pragma unroll
        for (int u = 0; u < kWideGroup; ++u) {
            const WideRowDesc d = tbl.d[s0 + u];
            const uint32_t q = d.rate;
            const uint32_t i = q == 0 ? il[0] : (q == 1 ? il[1] : (q == 2 ? il[2] : il[3]));
            wv[u] = q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
            Tf[u] = d.Tf;
            g[u] = d.gain;
            row[u] = d.row;
            const uint32_t k = md::in_channel(c, d.ch);
            reach[u] = j < d.frames;
            on[u] = reach[u] && md::has_channel(c, d.ch);
            lerp[u] = on[u] && d.Tf != 0.0f && i < d.last;
            const float *pa = d.data + (on[u] ? (uint64_t)i * d.ch + k : 0ull);
            a[u] = *pa;
            b[u] = pa[lerp[u] ? d.ch : 0u];
        }
#pragma unroll
        for (int u = 0; u < kWideGroup; ++u) {
            const float v = md::amp_lerp(a[u], b[u], g[u], lerp[u], wv[u], Tf[u]);
            if (reach[u]) row[u][o] = on[u] ? v : 0.0f;
        }
    }
}

// the carried states back to their sources, behind the filters: 4 * to_ch floats each
struct WideStateTable {
    const float *from[kWideChunk];
    float *to[kWideChunk];
};
__global__ __launch_bounds__(64) void k_wide_state_out(uint32_t to_ch, const WideStateTable tbl) {
    const float *from = tbl.from[blockIdx.x];
    float *to = tbl.to[blockIdx.x];
    for (uint32_t t = threadIdx.x; t < 4u * to_ch; t += 64) to[t] = from[t];
}

inline uint64_t wide_row_pitch(uint32_t channels, uint64_t out_frames) { return (out_frames * channels + 3) & ~3ull; }
inline uint64_t wide_filtered_bytes(uint32_t channels, uint64_t out_frames, uint64_t n) { return n * (2 * wide_row_pitch(channels, out_frames) + 4ull * channels) * sizeof(float); }

}  // namespace

rh_status rh_wide_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs_host, uint32_t n_sources, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (out_frames == 0) return RH_OK;
    if (!dst || channels == 0 || to_rate == 0 || (n_sources && !srcs_host)) return RH_ERR_INVALID;
    if (out_frames > 0x7fffffffull) return RH_ERR_UNSUPPORTED;
    struct Red {
        uint32_t F, T;
    };
    std::vector<Red> red(n_sources);
    uint64_t step = out_frames;  // output frames per launch: r0 + j F must fit 32 bits for every source
    for (uint32_t s = 0; s < n_sources; ++s) {
        if (srcs_host[s].frames == 0) continue;
        uint64_t fit;
        const rh_status st = mp::check_src(srcs_host[s], to_rate, out_frames, &red[s].F, &red[s].T, &fit);
        if (st != RH_OK) return st;
        if (fit < step) step = fit;
    }
    if (step == 0) return RH_ERR_UNSUPPORTED;
    // Alike sources (one rate and phase, the mixer's layout): the frames in front of the first one that ends -- or whose last frame a tap reaches --
    // go to the uniform kernel as a launch of their own, the rest to the general one.
    const uint64_t j_uni = mp::alike_cut(srcs_host, n_sources, channels, to_rate, out_frames);
    hipStream_t st = rh::as_stream(stream);
    for (uint64_t j0 = 0; j0 < out_frames;) {
        const uint64_t seg_end = j0 < j_uni ? j_uni : out_frames;
        const uint32_t nf = (uint32_t)(seg_end - j0 < step ? seg_end - j0 : step);
        float *const d0 = dst + j0 * channels;
        const uint64_t total = (uint64_t)nf * channels;
        mp::walk_rates<mp::RateLaunch>(
            n_sources, true,  // (no source reaches these frames: the mix is +0.0 there)
            [&](uint32_t s, uint32_t *F, uint32_t *T, uint32_t *r0, uint64_t *i0) {
                if (srcs_host[s].frames <= j0) return false;
                *F = red[s].F, *T = red[s].T;
                mp::tap_of(srcs_host[s].phase, j0, *F, *T, i0, r0);  // position of frame j0 between its taps, from the block's first tap on
                return true;
            },
            [&](const mp::RateLaunch &L) {
                WideTable tbl;
                for (uint32_t q = 0; q < kWideRates; ++q) tbl.r[q] = L.r[q];
                uint32_t k = 0;
                for (; k < L.n; ++k) {
                    const uint32_t s = L.src[k];
                    const rh_wide_src &x = srcs_host[s];
                    const uint64_t i0 = L.i0[k];
                    tbl.d[k] = WideDesc{x.data + i0 * x.channels, x.channels, (uint32_t)(x.frames - j0 < nf ? x.frames - j0 : nf),
                                        x.last == 0xffffffffu ? 0xffffffffu : (x.last >= i0 ? (uint32_t)(x.last - i0) : 0u), L.rate[k], x.gain, red[s].F == red[s].T ? 0.0f : (float)red[s].T};
                }
                // the uniform case (k_wide_mix_uniform): one rate, the mixer's layout, no source that ends inside the launch
                bool uni = k > 0 && L.nr == 1 && !rh::knob(rh::K_WIDE_GENERAL);
                const bool lerp = L.r[0].F != L.r[0].T;
                const uint64_t il_max = mp::last_tap(L.r[0], nf);
                for (uint32_t q = 0; q < k && uni; ++q) uni = tbl.d[q].ch == channels && tbl.d[q].frames == nf && (!lerp || il_max < tbl.d[q].last);
                if (uni) {
                    WideUniTable u;
                    u.F = L.r[0].F, u.T = L.r[0].T, u.r0 = L.r[0].r0, u.ch = channels, u.Tf = L.r[0].Tf;
                    u.pad[0] = u.pad[1] = u.pad[2] = 0;
                    for (uint32_t q = 0; q < kWideChunk; ++q) u.d[q] = WideUniSrc{tbl.d[q < k ? q : 0].data, q < k ? tbl.d[q].gain : 0.0f, 0u};
                    const dim3 grid(rh::grid_for((size_t)total, kBlock, 256u * 16u));
                    if (L.cont && lerp) hipLaunchKernelGGL((k_wide_mix_uniform<true, true>), grid, dim3(kBlock), 0, st, d0, nf, u, k);
                    else if (L.cont) hipLaunchKernelGGL((k_wide_mix_uniform<true, false>), grid, dim3(kBlock), 0, st, d0, nf, u, k);
                    else if (lerp) hipLaunchKernelGGL((k_wide_mix_uniform<false, true>), grid, dim3(kBlock), 0, st, d0, nf, u, k);
                    else hipLaunchKernelGGL((k_wide_mix_uniform<false, false>), grid, dim3(kBlock), 0, st, d0, nf, u, k);
                    return;
                }
                // whole groups: slots that reach no frame (and point at something readable: the first source's first tap)
                while (k % kWideGroup) tbl.d[k++] = WideDesc{tbl.d[0].data, 1u, 0u, 0u, 0u, 0.0f, 0.0f};
                const dim3 grid(rh::grid_for((size_t)total, kBlock, 256u * 16u));
                if (L.cont) hipLaunchKernelGGL(k_wide_mix<true>, grid, dim3(kBlock), 0, st, d0, channels, nf, tbl, k);
                else hipLaunchKernelGGL(k_wide_mix<false>, grid, dim3(kBlock), 0, st, d0, channels, nf, tbl, k);
            });
        RH_CHECK_LAUNCH();
        j0 += nf;
    }
    return RH_OK;
}

rh_status rh_wide_mix_filtered_scratch_bytes(uint32_t channels, uint64_t out_frames, uint32_t n_filtered, uint64_t *bytes) {
    if (!bytes || channels == 0 || out_frames > 0x7fffffffull) return RH_ERR_INVALID;
    *bytes = wide_filtered_bytes(channels, out_frames, n_filtered);
    return RH_OK;
}

rh_status rh_wide_mix_block_filtered(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs_host, uint32_t n_sources, const int32_t *kinds_host,
                                     const float *coeffs5_host, float *const *states_host, int32_t mode, void *scratch, uint64_t scratch_bytes, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (out_frames == 0) return RH_OK;
    if (!dst || channels == 0 || to_rate == 0 || (n_sources && (!srcs_host || !kinds_host)) || (mode != 0 && mode != 1)) return RH_ERR_INVALID;
    if (out_frames > 0x7fffffffull) return RH_ERR_UNSUPPORTED;
    bool any = false;
    for (uint32_t s = 0; s < n_sources; ++s) {
        if (kinds_host[s] < -1 || kinds_host[s] > 1 || (kinds_host[s] >= 0 && !coeffs5_host)) return RH_ERR_INVALID;
        any = any || kinds_host[s] >= 0;
    }
    if (!any) return rh_wide_mix_block(dst, channels, to_rate, out_frames, srcs_host, n_sources, stream);
    // Everything is checked before the first launch: a call that fails has written nothing, neither a sample nor a state.
    struct Row {
        uint32_t s, F, T;  // the source, its reduced rates
        bool whole;        // it spans the block (a row that ends inside it is filtered on its own)
    };
    std::vector<Row> rows;  // the filtered sources that reach the block, in insertion order
    bool carried = false;
    for (uint32_t s = 0; s < n_sources; ++s) {
        const rh_wide_src &x = srcs_host[s];
        if (x.frames == 0) continue;
        uint32_t F, T;
        uint64_t fit;
        const rh_status st = mp::check_src(x, to_rate, out_frames, &F, &T, &fit);
        if (st != RH_OK) return st;
        if (fit == 0) return RH_ERR_UNSUPPORTED;
        if (kinds_host[s] < 0) continue;
        if (fit < x.frames) return RH_ERR_UNSUPPORTED;
        rows.push_back(Row{s, F, T, x.frames == out_frames});
        carried = carried || (states_host && states_host[s]);
    }
    if (rows.empty()) return rh_wide_mix_block(dst, channels, to_rate, out_frames, srcs_host, n_sources, stream);
    if (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 15u)) return RH_ERR_INVALID;
    if (scratch_bytes < wide_filtered_bytes(channels, out_frames, rows.size())) return RH_ERR_CAPACITY;
    // The rows, grouped by coefficient set (sets in order of first appearance; in a set the rows that span the block first): what one
    // rh_biquad call filters lies back to back.
    auto co = [&](const Row &r) { return coeffs5_host + 5 * (size_t)r.s; };
    auto same = [&](const Row &a, const Row &b) { return memcmp(co(a), co(b), 5 * sizeof(float)) == 0 && kinds_host[a.s] == kinds_host[b.s]; };
    {
        std::vector<Row> grouped;
        std::vector<bool> taken(rows.size(), false);
        for (size_t i = 0; i < rows.size(); ++i) {
            if (taken[i]) continue;
            for (int whole = 1; whole >= 0; --whole)
                for (size_t k = i; k < rows.size(); ++k)
                    if (!taken[k] && rows[k].whole == (whole == 1) && same(rows[i], rows[k])) grouped.push_back(rows[k]);
            for (size_t k = i; k < rows.size(); ++k)
                if (same(rows[i], rows[k])) taken[k] = true;
        }
        rows.swap(grouped);
    }
    const uint64_t pitch = wide_row_pitch(channels, out_frames);
    const size_t R = rows.size();
    float *const conv = static_cast<float *>(scratch), *const filt = conv + R * pitch, *const states = filt + R * pitch;
    hipStream_t hs = rh::as_stream(stream);
    // 1. the converter: a launch per 32 rows (or per four different (rate, phase) pairs)
    mp::walk_rates<mp::RateLaunch>(
        (uint32_t)R, false,
        [&](uint32_t i, uint32_t *F, uint32_t *T, uint32_t *r0, uint64_t *) {
            *F = rows[i].F, *T = rows[i].T, *r0 = srcs_host[rows[i].s].phase;
            return true;
        },
        [&](const mp::RateLaunch &L) {
            WideRowTable tbl;
            for (uint32_t q = 0; q < kWideRates; ++q) tbl.r[q] = L.r[q];
            uint32_t k = 0;
            for (; k < L.n; ++k) {
                const size_t i = L.src[k];
                const rh_wide_src &x = srcs_host[rows[i].s];
                tbl.d[k] = WideRowDesc{x.data, conv + i * pitch, states_host ? states_host[rows[i].s] : nullptr, carried ? states + i * 4 * (size_t)channels : nullptr,
                                       x.channels, (uint32_t)x.frames, x.last, L.rate[k], x.gain, rows[i].F == rows[i].T ? 0.0f : (float)rows[i].T};
            }
            while (k % kWideGroup) tbl.d[k++] = WideRowDesc{tbl.d[0].data, nullptr, nullptr, nullptr, 1u, 0u, 0u, 0u, 0.0f, 0.0f};  // (whole groups: slots that reach no frame)
            const uint64_t total = out_frames * channels;
            hipLaunchKernelGGL(k_wide_rows, dim3(rh::grid_for((size_t)total, kBlock, 256u * 16u), k / kWideGroup), dim3(kBlock), 0, hs, channels, (uint32_t)out_frames, tbl);
        });
    RH_CHECK_LAUNCH();
    // 2. the filter: a batch per coefficient set where the rows lie back to back on 16-byte boundaries, and the rows that end inside the
    //    block one by one.  Mode 1 only for what the contract covers; rh_biquad itself continues in mode 0 where its scan kernel declines.
    for (size_t i = 0; i < R;) {
        size_t whole = 0, n = 0;
        while (i + n < R && same(rows[i], rows[i + n])) whole += rows[i + n].whole ? 1 : 0, ++n;
        const int32_t m = mode == 1 && channels <= 8 && rh::filter_scan_ok_coeffs(kinds_host[rows[i].s], co(rows[i])) ? 1 : 0;
        const size_t batch = whole && (pitch == out_frames * channels || whole == 1) ? whole : 0;
        for (size_t k = 0; k < n; k += (k < batch ? batch : 1)) {
            const uint32_t n_streams = k < batch ? (uint32_t)batch : 1u;
            const rh_status st = rh_biquad(filt + (i + k) * pitch, conv + (i + k) * pitch, srcs_host[rows[i + k].s].frames, channels, n_streams, co(rows[i]),
                                           carried ? states + (i + k) * 4 * (size_t)channels : nullptr, m, stream);
            if (st != RH_OK) return st;
        }
        i += n;
    }
    // 3. the mix: the caller's table with every filtered source replaced by its row -- the mixer's layout and rate, gain 1: it passes through
    {
        std::vector<rh_wide_src> mixed(srcs_host, srcs_host + n_sources);
        for (size_t i = 0; i < R; ++i) {
            rh_wide_src &x = mixed[rows[i].s];
            x.data = filt + i * pitch;
            x.channels = channels;
            x.from_rate = to_rate;
            x.phase = 0;
            x.last = x.last == 0xffffffffu ? 0xffffffffu : (uint32_t)(x.frames - 1);
            x.gain = 1.0f;
        }
        const rh_status st = rh_wide_mix_block(dst, channels, to_rate, out_frames, mixed.data(), n_sources, stream);
        if (st != RH_OK) return st;
    }
    // 4. the states go back to their sources
    if (carried) {
        WideStateTable tbl;
        uint32_t k = 0;
        for (size_t i = 0; i < R; ++i) {
            float *to = states_host[rows[i].s];
            if (to) tbl.from[k] = states + i * 4 * (size_t)channels, tbl.to[k++] = to;
            if (k == kWideChunk || (k && i + 1 == R)) {
                hipLaunchKernelGGL(k_wide_state_out, dim3(k), dim3(64), 0, hs, channels, tbl);
                k = 0;
            }
        }
        RH_CHECK_LAUNCH();
    }
    return RH_OK;
}
