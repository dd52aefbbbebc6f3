// rh_mix2.hip -- the Source trait's two-input combinators:
//   Source::mix(other)                          src/source/mod.rs:255, src/source/mix.rs:10-22,43-53
//   Source::take_crossfade_with(other, d)       src/source/mod.rs:448, src/source/crossfade.rs:10-23
// Mix::next (mix.rs:43-53) has four arms: both inputs Some -> s1 + s2 (no leading zero: -0.0 + -0.0 stays -0.0, unlike the mixer's
// ((0 + v0) + v1)); one Some -> that sample VERBATIM (not s + 0.0); both None -> None.  Both inputs are UniformSourceIterators in the
// first input's format (mix.rs:14-21): the first one's wrapper is the identity on samples, the second one's is the span-by-span
// conversion of uniform.rs:50-97.
//   rh_mix_pair      the four arms over two rows already in the mix's format
//   rh_uniform_row   UniformSourceIterator over a resident row, chain by chain (a chain that cuts a frame included), as a table of
//                    rh_uniform_segments segments: what the second input goes through
//   rh_crossfade     crossfade(a, b, d) = mix(a.take_duration(d) with the fade-out filter, b.take_duration(d).fade_in(d)) for a batch
//                    of pairs in ONE launch (k_crossfade); pairs the kernel does not take run through the stand-alone calls instead
// The arithmetic of the fused kernel is rh_rows_dev.h's, which the stand-alone kernels call as well.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "rh_common.h"
#include "rh_rows_dev.h"

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ float4 row4(const float *__restrict__ p, size_t i, size_t n, bool aligned) {
    return aligned && i + 4 <= n ? rh::ld_nt(reinterpret_cast<const float4 *>(p + i)) : rh::ld4_at(p, (int64_t)i, n);
}
__device__ __forceinline__ void store4(float *__restrict__ dst, size_t i, size_t total, bool aligned, const float (&e)[4]) {
    if (aligned && i + 4 <= total) {
        rh::st_nt(reinterpret_cast<float4 *>(dst + i), make_float4(e[0], e[1], e[2], e[3]));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j < total) dst[i + j] = e[j];
    }
}

// Four consecutive samples a lane, a vector a lane (rh::grid_tiles).  A lane reads and writes its own four samples only, so dst may be
// either input.  vec: bit 0 = a starts on a 16-byte boundary, bit 1 = b, bit 2 = dst.
__global__ __launch_bounds__(kBlock) void k_mix_pair(float *dst, const float *a, size_t na, const float *b, size_t nb, int vec) {
    const size_t total = na > nb ? na : nb, nvec = (total + 3) / 4, stride = (size_t)gridDim.x * kBlock;
    for (size_t v = (size_t)blockIdx.x * kBlock + threadIdx.x; v < nvec; v += stride) {
        const size_t i = 4 * v;
        const float4 xa = row4(a, i, na, vec & 1), xb = row4(b, i, nb, vec & 2);
        const float x[4] = {xa.x, xa.y, xa.z, xa.w}, y[4] = {xb.x, xb.y, xb.z, xb.w};
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = i + j < na ? (i + j < nb ? x[j] + y[j] : x[j]) : y[j];  // mix.rs:47-52
        store4(dst, i, total, vec & 4, e);
    }
}

// ---- the fused crossfade ------------------------------------------------------------------------------------------------------
// One pair of the batch as the kernel sees it.  `a` is in the output's format: its sample o is faded by what the duration has left
// at o (take.rs:33-41).  `b` arrives in its own format: output frame m lies in chain m / chain_out of the second input's
// UniformSourceIterator (chains of chain_frames input frames, each a fresh converter that ends with its last frame verbatim), and
// both taps of its lerp carry the fade-in factor of their OWN frame of b (the ramp runs in front of the converter).
struct CfPlan {
    const float *a, *b;
    float *dst;
    uint64_t a_take;        // samples of a the duration admits (whole frames)
    uint64_t b_frames;      // frames of b the duration admits
    uint64_t b_out_frames;  // ... and the output frames they convert to
    uint64_t out_samples;   // max(a_take, b_out_frames * ca)
    uint64_t chain_frames, chain_out;
    uint64_t dps_a, duration_ns;
    rhrows::Ramp ramp;
    uint32_t ca, cb, F, T;
    float total_ms, Tf;
};
static_assert(sizeof(CfPlan) % 8 == 0, "copied to LDS in 8-byte words");

struct CfTap {  // where an output frame lies in b
    const float *p;  // first tap
    float g0, g1, numf;
    bool on, lerp;
};
__device__ __forceinline__ CfTap cf_tap(const CfPlan &g, uint64_t m) {
    CfTap t;
    t.on = m < g.b_out_frames;
    t.lerp = false;
    t.p = g.b;
    t.g0 = t.g1 = t.numf = 0.0f;
    if (!t.on) return t;
    const uint64_t chain = m / g.chain_out, ml = m - chain * g.chain_out;
    const uint64_t first = chain * g.chain_frames;
    const uint64_t nf = g.b_frames - first < g.chain_frames ? g.b_frames - first : g.chain_frames;
    uint64_t i = ml;
    uint32_t num = 0;
    if (g.F != g.T) {  // (F == T: the converter passes through, sample_rate.rs:133-136)
        const uint64_t pp = ml * g.F;  // (host: fits 64 bits)
        i = pp / g.T;
        num = (uint32_t)(pp - i * g.T);
    }
    t.lerp = g.F != g.T && i + 1 < nf;  // otherwise the chain's last frame, verbatim (sample_rate.rs:193-200)
    t.p = g.b + (first + i) * g.cb;
    t.g0 = rhrows::ramp_factor(g.ramp, first + i);
    t.g1 = t.lerp ? rhrows::ramp_factor(g.ramp, first + i + 1) : 0.0f;
    t.numf = (float)num;
    return t;
}
// channel c of the output frame (channels.rs:57-85: c < from: the input channel; c == 1 of a mono source: its only one; otherwise 0.0)
__device__ __forceinline__ float cf_b_value(const CfPlan &g, const CfTap &t, uint32_t c) {
    const bool has = c < g.cb || (c == 1u && g.cb == 1u);
    if (!has) return 0.0f;
    const uint32_t k = c < g.cb ? c : 0u;
    const float x = t.p[k] * t.g0;  // linear_ramp.rs:105-109 in front of the converter
    return t.lerp ? rhrows::lerp(x, t.p[g.cb + k] * t.g1, t.numf, g.Tf) : x;
}

constexpr uint32_t kCfTile = 4 * kBlock;  // output samples a workgroup: four a lane
__global__ __launch_bounds__(kBlock) void k_crossfade(const CfPlan *__restrict__ plans) {
    __shared__ CfPlan g;
    if (threadIdx.x < sizeof(CfPlan) / 8) reinterpret_cast<uint64_t *>(&g)[threadIdx.x] = reinterpret_cast<const uint64_t *>(plans + blockIdx.y)[threadIdx.x];
    __syncthreads();
    const uint64_t o0 = (uint64_t)blockIdx.x * kCfTile + 4u * threadIdx.x;
    if (o0 >= g.out_samples) return;
    const bool a_vec = (reinterpret_cast<uintptr_t>(g.a) & 15u) == 0, d_vec = (reinterpret_cast<uintptr_t>(g.dst) & 15u) == 0;
    const float4 xa = row4(g.a, o0, g.a_take, a_vec);
    const float x[4] = {xa.x, xa.y, xa.z, xa.w};
    uint64_t m = o0 / g.ca;
    uint32_t c = (uint32_t)(o0 - m * g.ca);
    CfTap t = cf_tap(g, m);
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t o = o0 + j;
        const float s1 = rhrows::take_fade(x[j], g.duration_ns - o * g.dps_a, g.total_ms);
        const float s2 = t.on ? cf_b_value(g, t, c) : 0.0f;
        e[j] = o < g.a_take ? (t.on ? s1 + s2 : s1) : s2;  // mix.rs:47-52
        if (++c == g.ca) {
            c = 0;
            if (j < 3) t = cf_tap(g, ++m);
        }
    }
    store4(g.dst, o0, g.out_samples, d_vec, e);
}

// ---- host: UniformSourceIterator over a row, as segments ---------------------------------------------------------------------
struct Reduced {
    uint64_t F, T;
};
rh_status reduce(uint32_t from_rate, uint32_t to_rate, Reduced *r) {
    if (from_rate == 0 || to_rate == 0) return RH_ERR_INVALID;
    const uint32_t gc = std::gcd(from_rate, to_rate);
    r->F = from_rate / gc, r->T = to_rate / gc;
    return r->F * r->T > 0xffffffffull ? RH_ERR_UNSUPPORTED : RH_OK;  // the reference's u32 products overflow (sample_rate.rs:45-47)
}
// The chains of uniform.rs:56-67 over n samples: every min(span_len, 32768) samples a fresh converter, the last one over what is left.
// segs == nullptr only counts.  A chain of whole frames is one complete span; a chain that ends t samples into a frame is its whole
// frames as an open span and the tail segment behind them (rodio_hip.h, rh_uniform_seg), and the next chain starts behind the cut.
rh_status plan_uniform_row(float *dst, const float *src, uint64_t n, uint32_t from_ch, uint32_t from_rate, uint32_t to_ch, uint32_t to_rate, uint64_t span_len,
                           std::vector<rh_uniform_seg> *segs, uint64_t *out_samples) {
    if (from_ch == 0 || to_ch == 0) return RH_ERR_INVALID;
    Reduced r;
    rh_status st = reduce(from_rate, to_rate, &r);
    if (st != RH_OK) return st;
    uint64_t chain = span_len ? std::min<uint64_t>(span_len, 32768) : n;
    if (chain == 0 || chain > n) chain = n;
    uint64_t out = 0;
    for (uint64_t s0 = 0; s0 < n; s0 += chain) {
        const uint64_t len = std::min(chain, n - s0), q = len / from_ch;
        const uint32_t t = (uint32_t)(len % from_ch);
        rh_uniform_seg g{};
        g.from_rate = from_rate, g.to_rate = to_rate, g.from_ch = from_ch, g.to_ch = to_ch, g.gain = 1.0f;
        uint64_t of = 0;
        if (q) {
            if ((st = rh_uniform_span_frames(q, from_rate, to_rate, t == 0, &of)) != RH_OK) return st;
            if (of && segs) {
                g.src = src + s0, g.dst = dst + out, g.src_frame0 = 0, g.src_frames = q, g.m0 = 0, g.m1 = of;
                g.span_frames = t == 0 ? q : UINT64_MAX;
                segs->push_back(g);
            }
            out += of * to_ch;
        }
        if (t) {
            uint64_t ts = 0;
            if ((st = rh_uniform_cut_tail_samples(q, t, from_rate, to_rate, from_ch, to_ch, &ts)) != RH_OK) return st;
            if (ts && segs) {
                const uint64_t sf = q ? 1 : 0;
                g.src = src + s0 + (q - sf) * from_ch, g.dst = dst + out, g.src_frame0 = q - sf, g.src_frames = sf, g.m0 = 0, g.m1 = ts;
                g.span_frames = q, g.reserved = t;
                segs->push_back(g);
            }
            out += ts;
        }
    }
    *out_samples = out;
    return RH_OK;
}

// A pair of the host table (rodio_hip.h: RH_CROSSFADE_PAIR_WORDS words), decoded.
struct CfPair {
    const float *a;
    uint64_t a_samples;
    uint32_t a_channels, a_rate;
    const float *b;
    uint64_t b_samples;
    uint32_t b_channels, b_rate;
    uint64_t b_span_len;
    float *dst;
    uint64_t dst_capacity;
};
CfPair decode_pair(const uint64_t *w) {
    auto u32 = [](uint64_t v) { return v > 0xffffffffull ? 0u : (uint32_t)v; };  // (no such channel count or rate: refused as a zero is)
    CfPair p;
    p.a = reinterpret_cast<const float *>((uintptr_t)w[0]), p.a_samples = w[1], p.a_channels = u32(w[2]), p.a_rate = u32(w[3]);
    p.b = reinterpret_cast<const float *>((uintptr_t)w[4]), p.b_samples = w[5], p.b_channels = u32(w[6]), p.b_rate = u32(w[7]);
    p.b_span_len = w[8];
    p.dst = reinterpret_cast<float *>((uintptr_t)w[9]), p.dst_capacity = w[10];
    return p;
}
// What a crossfade makes of one pair, on the host.
struct CfShape {
    uint64_t a_take, b_take, b_span, b_out, out;
    uint64_t dps_a;
};
rh_status cf_shape(const CfPair &p, uint64_t duration_ns, CfShape *s) {
    if (p.a_channels == 0 || p.a_rate == 0 || p.b_channels == 0 || p.b_rate == 0) return RH_ERR_INVALID;  // NonZero in rodio
    const uint64_t dps_a = 1000000000ull / ((uint64_t)p.a_rate * p.a_channels), dps_b = 1000000000ull / ((uint64_t)p.b_rate * p.b_channels);  // take.rs:63-67
    if (dps_a == 0 || dps_b == 0) return RH_ERR_UNSUPPORTED;  // above 1 GHz*channel the reference never expires
    const uint64_t admits_a = duration_ns / dps_a, admits_b = duration_ns / dps_b;
    s->dps_a = dps_a;
    s->a_take = std::min(p.a_samples, admits_a);
    s->b_take = std::min(p.b_samples, admits_b);
    // TakeDuration::current_span_len (take.rs:180-196), which LinearGainRamp passes on (linear_ramp.rs:121-123): what the duration
    // admits unless the input's span is shorter
    s->b_span = p.b_span_len && p.b_span_len < admits_b ? p.b_span_len : admits_b;
    const rh_status st = plan_uniform_row(nullptr, nullptr, s->b_take, p.b_channels, p.b_rate, p.a_channels, p.a_rate, s->b_span, nullptr, &s->b_out);
    if (st != RH_OK) return st;
    s->out = std::max(s->a_take, s->b_out);
    return RH_OK;
}
// Does k_crossfade take the pair?  b of 1 or 2 channels, a of up to 8, whole frames on both sides and in every chain.
bool cf_fused_ok(const CfPair &p, const CfShape &s, CfPlan *g, uint64_t duration_ns) {
    if (p.b_channels > 2 || p.a_channels > 8 || s.a_take % p.a_channels || s.b_take % p.b_channels || s.out >= (1ull << 40)) return false;
    const uint64_t chain = s.b_span ? std::min<uint64_t>(s.b_span, 32768) : s.b_take;
    const bool one_chain = chain == 0 || chain >= s.b_take;
    if (!one_chain && chain % p.b_channels) return false;
    Reduced r;
    if (reduce(p.b_rate, p.a_rate, &r) != RH_OK) return false;
    g->a = p.a, g->b = p.b, g->dst = p.dst;
    g->a_take = s.a_take, g->b_frames = s.b_take / p.b_channels, g->b_out_frames = s.b_out / p.a_channels, g->out_samples = s.out;
    g->chain_frames = one_chain ? std::max<uint64_t>(g->b_frames, 1) : chain / p.b_channels;
    uint64_t co = 1;
    (void)rh_uniform_span_frames(g->chain_frames, p.b_rate, p.a_rate, 1, &co);
    g->chain_out = std::max<uint64_t>(co, 1);
    g->dps_a = s.dps_a, g->duration_ns = duration_ns;
    g->ramp = rhrows::make_ramp(p.b_rate, duration_ns, 0.0f, 1.0f, false);  // fade_in (fadein.rs:11-13)
    g->ca = p.a_channels, g->cb = p.b_channels, g->F = (uint32_t)r.F, g->T = (uint32_t)r.T;
    g->total_ms = (float)(duration_ns / 1000000ull), g->Tf = (float)r.T;
    return true;
}

inline int vec3(const void *a, const void *b, const void *dst) {
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    return (al(a) ? 1 : 0) | (al(b) ? 2 : 0) | (al(dst) ? 4 : 0);
}

}  // namespace

extern "C" {

rh_status rh_mix_pair(float *dst, const float *a, size_t na, const float *b, size_t nb, rh_stream stream) {
    RH_REQUIRE_INIT();
    const size_t total = std::max(na, nb);
    if (total == 0) return RH_OK;
    if (!dst || (na && !a) || (nb && !b)) return RH_ERR_INVALID;
    if (!a) a = b;  // (a row of no samples is never read; the kernel still forms its address)
    if (!b) b = a;
    hipLaunchKernelGGL(k_mix_pair, dim3(rh::grid_tiles((total + 3) / 4)), dim3(kBlock), 0, rh::as_stream(stream), dst, a, na, b, nb, vec3(a, b, dst));
    RH_CHECK_LAUNCH();
    return RH_OK;
}

rh_status rh_uniform_row_out_samples(uint64_t n_samples, uint32_t from_ch, uint32_t from_rate, uint32_t to_ch, uint32_t to_rate, uint64_t span_len, uint64_t *out_samples) {
    if (!out_samples) return RH_ERR_INVALID;
    return plan_uniform_row(nullptr, nullptr, n_samples, from_ch, from_rate, to_ch, to_rate, span_len, nullptr, out_samples);
}

rh_status rh_uniform_row(float *dst, uint64_t dst_capacity, const float *src, uint64_t n_samples, uint32_t from_ch, uint32_t from_rate, uint32_t to_ch, uint32_t to_rate,
                         uint64_t span_len, uint64_t *out_samples, rh_stream stream) {
    RH_REQUIRE_INIT();
    uint64_t out = 0;
    rh_status st = plan_uniform_row(nullptr, nullptr, n_samples, from_ch, from_rate, to_ch, to_rate, span_len, nullptr, &out);
    if (st != RH_OK) return st;
    if (out > dst_capacity) return RH_ERR_INVALID;
    if (out_samples) *out_samples = out;
    if (out == 0) return RH_OK;
    if (!dst || !src) return RH_ERR_INVALID;
    std::vector<rh_uniform_seg> segs;
    if ((st = plan_uniform_row(dst, src, n_samples, from_ch, from_rate, to_ch, to_rate, span_len, &segs, &out)) != RH_OK) return st;
    if (segs.size() > 0xffffffffull) return RH_ERR_UNSUPPORTED;
    return rh_uniform_segments(segs.data(), (uint32_t)segs.size(), stream);
}

rh_status rh_crossfade_out_samples(const uint64_t *pair_host, uint64_t duration_ns, uint64_t *out_samples) {
    if (!pair_host || !out_samples) return RH_ERR_INVALID;
    CfShape s;
    const rh_status st = cf_shape(decode_pair(pair_host), duration_ns, &s);
    if (st == RH_OK) *out_samples = s.out;
    return st;
}

rh_status rh_crossfade(const uint64_t *pairs_words_host, uint32_t n_pairs, uint64_t duration_ns, uint64_t *out_samples_host, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (n_pairs == 0) return RH_OK;
    if (!pairs_words_host) return RH_ERR_INVALID;
    std::vector<CfPair> pairs_host(n_pairs);
    for (uint32_t k = 0; k < n_pairs; ++k) pairs_host[k] = decode_pair(pairs_words_host + (size_t)k * RH_CROSSFADE_PAIR_WORDS);
    // every pair is checked before anything is launched: a refused batch writes nothing
    std::vector<CfShape> shapes(n_pairs);
    std::vector<CfPlan> fused;
    std::vector<uint32_t> composed;
    uint64_t most = 0;
    size_t rows_bytes = 0;  // the composed pairs run one after the other on the stream: they share one set of rows
    auto pad16 = [](uint64_t samples) { return (size_t)((samples * 4 + 15) & ~15ull); };
    for (uint32_t k = 0; k < n_pairs; ++k) {
        const CfPair &p = pairs_host[k];
        const rh_status st = cf_shape(p, duration_ns, &shapes[k]);
        if (st != RH_OK) return st;
        const CfShape &s = shapes[k];
        if (p.dst_capacity < s.out || (s.out && !p.dst) || (s.a_take && !p.a) || (s.b_take && !p.b)) return RH_ERR_INVALID;
        if (s.out == 0) continue;
        CfPlan g;
        if (cf_fused_ok(p, s, &g, duration_ns)) {
            if (!g.a) g.a = g.b;  // (never read: a_take == 0; the kernel still forms the address)
            if (!g.b) g.b = g.a;
            fused.push_back(g);
            most = std::max(most, s.out);
        } else {
            composed.push_back(k);
            rows_bytes = std::max(rows_bytes, pad16(s.a_take + p.a_channels) + pad16(s.b_take + p.b_channels) + pad16(s.b_out));
        }
    }
    if (out_samples_host)
        for (uint32_t k = 0; k < n_pairs; ++k) out_samples_host[k] = shapes[k].out;
    hipStream_t s = rh::as_stream(stream);
    const size_t table_bytes = (fused.size() * sizeof(CfPlan) + 15) & ~(size_t)15;
    if (table_bytes + rows_bytes == 0) return RH_OK;
    std::unique_lock<std::mutex> hold;
    void *scratch = nullptr;
    RH_HIP_TRY(rh::stream_scratch(s, table_bytes + rows_bytes, &scratch, hold));
    if (!fused.empty()) {
        char *host = nullptr;  // the plan table's way to the device: the stream's table ring (rh_common.h)
        RH_HIP_TRY(rh::table_stage(s, fused.size() * sizeof(CfPlan), &host));
        memcpy(host, fused.data(), fused.size() * sizeof(CfPlan));
        RH_HIP_TRY(rh::table_send(s, scratch));
        const uint64_t tiles = (most + kCfTile - 1) / kCfTile;
        if (tiles > 0x7fffffffull) return RH_ERR_UNSUPPORTED;
        for (size_t first = 0; first < fused.size(); first += 65535) {
            const uint32_t n = (uint32_t)std::min<size_t>(fused.size() - first, 65535);
            hipLaunchKernelGGL(k_crossfade, dim3((uint32_t)tiles, n), dim3(kBlock), 0, s, static_cast<const CfPlan *>(scratch) + first);
            RH_CHECK_LAUNCH();
        }
    }
    for (uint32_t k : composed) {  // never an error, the same bits, slower: the stand-alone calls on the stream's scratch
        const CfPair &p = pairs_host[k];
        const CfShape &sh = shapes[k];
        float *ta = reinterpret_cast<float *>(static_cast<char *>(scratch) + table_bytes);
        float *tb = reinterpret_cast<float *>(reinterpret_cast<char *>(ta) + pad16(sh.a_take + p.a_channels));
        float *ub = reinterpret_cast<float *>(reinterpret_cast<char *>(tb) + pad16(sh.b_take + p.b_channels));
        uint64_t got = 0;
        rh_status st = rh_take_duration(ta, p.a, sh.a_take, 0, p.a_channels, p.a_rate, duration_ns, 1, &got, nullptr, stream);
        if (st != RH_OK) return st;
        if ((st = rh_take_duration(tb, p.b, sh.b_take, 0, p.b_channels, p.b_rate, duration_ns, 0, &got, nullptr, stream)) != RH_OK) return st;
        if (sh.b_take && (st = rh_linear_gain_ramp(tb, tb, sh.b_take, 0, p.b_channels, p.b_rate, duration_ns, 0.0f, 1.0f, 0, stream)) != RH_OK) return st;
        if ((st = rh_uniform_row(ub, sh.b_out, tb, sh.b_take, p.b_channels, p.b_rate, p.a_channels, p.a_rate, sh.b_span, &got, stream)) != RH_OK) return st;
        if ((st = rh_mix_pair(p.dst, ta, sh.a_take, ub, sh.b_out, stream)) != RH_OK) return st;
    }
    return RH_OK;
}

}  // extern "C"
