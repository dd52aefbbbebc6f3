// rh_live.hip -- parameters that change while a source plays (rodio's Player / SpatialPlayer chains):
//   Amplify::set_factor / set_log_factor under PeriodicAccess       (src/source/amplify.rs:27-35,64; periodic.rs:63-77)
//   ChannelVolume::set_volume / Spatial::set_positions, + a factor  (src/source/channel_volume.rs:71-88; spatial.rs:48-69)
//   BltFilter::to_low_pass / to_high_pass (+ _with_q)               (src/source/blt.rs:68-91, 234-252; apply :559)
// The value of a parameter is a TABLE of steps in device memory: sample `first + i` of the stream takes entry
// (first + i) / period - first / period.  The index is a 32-bit quotient relative to the block, by a multiplier the host
// computes once per launch (no 64-bit division per sample).  The arithmetic per sample is the reference's: x * factor;
// ((0 + s0) + s1 + ..) / C_in * gain[k], then * factor -- the same bits as rh_amplify / rh_channel_volume with that step's values.
#include <cstdint>
#include <mutex>

#include "rh_common.h"
#include "rh_mix_plan.h"

namespace {

constexpr int kBlock = 256;
// A launch covers at most this many samples (output samples for the channel volume): every in-block index, plus the phase of the
// first sample inside its period, then fits in 32 bits.
constexpr uint64_t kMaxLaunchSamples = 1ull << 30;

// The step index (rh_mix_plan.h): x / d for x < 2^32, 1 <= d <= 2^31 by the round-up method (Granlund-Montgomery), exact for every x
// (tests/test_gpu_live.py checks the boundaries), and the table index of sample i (< n <= 2^30) of a block whose first sample is the
// stream's sample `first`: step_div(first, period, n).
using rh::mixplan::StepDiv;
using rh::mixplan::step_div;

// Entries of a table that covers samples [first, first + n) at `period`.
uint64_t steps_needed(uint64_t first, uint64_t period, uint64_t n) { return n ? (first + n - 1) / period - first / period + 1 : 0; }

// ----------------------------------------------------------- stepped Amplify ----
// rh::map4's shape (four consecutive samples a lane, one 16-byte load and store, rows that start anywhere, in place).
// WIDE (period >= 4): the four samples of a lane cross at most one boundary -- two table loads a lane (the second one only where the
// lane crosses), not four.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_amplify_steps(float *__restrict__ dst, const float *__restrict__ src, size_t n, StepDiv sd, const float *__restrict__ factors, int vec) {
    if (!WIDE) {
        rh::map4<kBlock>(dst, src, n, vec, [=](size_t i, float x) { return x * factors[sd.step((uint32_t)i)]; });
        return;
    }
    const size_t nvec = (n + 3) / 4, stride = (size_t)gridDim.x * kBlock;
    for (size_t v = (size_t)blockIdx.x * kBlock + threadIdx.x; v < nvec; v += stride) {
        const size_t i = 4 * v;
        if (i + 4 <= n) {
            const float4 x = (vec & 1) ? rh::ld_nt(reinterpret_cast<const float4 *>(src) + v) : rh::ld4_at(src, (int64_t)i, n);
            const uint32_t q0 = sd.step((uint32_t)i), q3 = sd.step((uint32_t)i + 3u);
            const float fa = factors[q0], fb = q3 != q0 ? factors[q3] : fa;
            const float4 y = make_float4(x.x * fa, x.y * (sd.step((uint32_t)i + 1u) == q0 ? fa : fb), x.z * (sd.step((uint32_t)i + 2u) == q0 ? fa : fb), x.w * fb);
            if (vec & 2) {
                rh::st_nt(reinterpret_cast<float4 *>(dst) + v, y);
            } else {
                dst[i] = y.x, dst[i + 1] = y.y, dst[i + 2] = y.z, dst[i + 3] = y.w;
            }
        } else {
            for (int j = 0; j < 4; ++j)
                if (i + j < n) dst[i + j] = src[i + j] * factors[sd.step((uint32_t)(i + j))];
        }
    }
}

// ---------------------------------------------- stepped ChannelVolume (+ factor) ----
// out[j] = (mean(frame j / out_ch) * gains[step_g(j)][j % out_ch]) * factors[step_f(j)]; factors == nullptr: no factor.
struct Tables {
    const float *gains;    // [steps][out_ch]
    const float *factors;  // [steps] or nullptr
    StepDiv g, f;
    __device__ __forceinline__ float apply(float m, uint32_t j, uint32_t k, uint32_t out_ch) const {
        const float y = m * gains[(size_t)g.step(j) * out_ch + k];
        return factors ? y * factors[f.step(j)] : y;
    }
};
// Stereo in / stereo out (the SpatialPlayer tail): two frames a lane, one 16-byte load, one 16-byte store (k_channel_volume_2x2's shape).
__global__ __launch_bounds__(kBlock) void k_channel_volume_steps_2x2(float *__restrict__ dst, const float *__restrict__ src, size_t frames, Tables t, int vec_ok) {
    const size_t nvec = (frames + 1) / 2, stride = (size_t)gridDim.x * kBlock;
    for (size_t v = (size_t)blockIdx.x * kBlock + threadIdx.x; v < nvec; v += stride) {
        const uint32_t j = 4u * (uint32_t)v;
        auto one = [&](float l, float r, uint32_t jj, float &ol, float &orr) {
            float m = (0.0f + l) + r;
            m = m / 2.0f;
            ol = t.apply(m, jj, 0, 2), orr = t.apply(m, jj + 1, 1, 2);
        };
        if (vec_ok && 2 * v + 2 <= frames) {
            const float4 x = rh::ld_nt(reinterpret_cast<const float4 *>(src) + v);
            float4 y;
            one(x.x, x.y, j, y.x, y.y);
            one(x.z, x.w, j + 2, y.z, y.w);
            rh::st_nt(reinterpret_cast<float4 *>(dst) + v, y);
        } else {
            for (size_t f = 2 * v; f < 2 * v + 2 && f < frames; ++f) one(src[2 * f], src[2 * f + 1], 2u * (uint32_t)f, dst[2 * f], dst[2 * f + 1]);
        }
    }
}
// Any layout: k_channel_volume_tile's shape -- the tile's input comes in as aligned 16-byte vectors into LDS, a lane per frame takes the
// mean, a lane per four output samples applies the steps and stores 16 bytes.
__global__ __launch_bounds__(kBlock) void k_channel_volume_steps_tile(float *__restrict__ dst, const float *__restrict__ src, size_t frames, uint32_t in_ch, uint32_t out_ch, Tables t,
                                                                      uint32_t tile_frames, uint32_t in_floats, int vec_ok) {
    extern __shared__ uint4 cvs_tile[];
    float *lds = reinterpret_cast<float *>(cvs_tile);
    float *means = lds + in_floats;
    const size_t f0 = (size_t)blockIdx.x * tile_frames;  // (a multiple of 4 frames)
    const uint32_t nf = (uint32_t)(frames - f0 < tile_frames ? frames - f0 : tile_frames);
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(src + f0 * in_ch), a0 = p0 & ~(uintptr_t)15;
    const uint32_t shift = (uint32_t)(p0 - a0) / 4u, nvec = (shift + nf * in_ch + 3u) / 4u;
    for (uint32_t v = threadIdx.x; v < nvec; v += kBlock) cvs_tile[v] = rh::ld_nt(reinterpret_cast<const uint4 *>(a0) + v);
    __syncthreads();
    for (uint32_t f = threadIdx.x; f < nf; f += kBlock) {
        const float *x = lds + shift + f * in_ch;
        float m = 0.0f;
        for (uint32_t c = 0; c < in_ch; ++c) m = m + x[c];
        means[f] = m / (float)in_ch;
    }
    __syncthreads();
    const uint32_t total = nf * out_ch, nv = (total + 3u) / 4u, j0 = (uint32_t)(f0 * out_ch);
    float *out = dst + f0 * out_ch;
    for (uint32_t v = threadIdx.x; v < nv; v += kBlock) {
        const uint32_t o0 = 4u * v;
        uint32_t f = o0 / out_ch, k = o0 - f * out_ch;
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = o0 + j < total ? t.apply(means[f], j0 + o0 + j, k, out_ch) : 0.0f;
            if (++k == out_ch) k = 0, ++f;
        }
        if (vec_ok && o0 + 4u <= total) {
            rh::st_nt(reinterpret_cast<float4 *>(out + o0), make_float4(e[0], e[1], e[2], e[3]));
        } else {
            for (int j = 0; j < 4; ++j)
                if (o0 + j < total) out[o0 + j] = e[j];
        }
    }
}
// Frames of hundreds of channels (a tile would not fit): a lane per frame.
__global__ __launch_bounds__(kBlock) void k_channel_volume_steps(float *__restrict__ dst, const float *__restrict__ src, size_t frames, uint32_t in_ch, uint32_t out_ch, Tables t) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t f = (size_t)blockIdx.x * kBlock + threadIdx.x; f < frames; f += stride) {
        float m = 0.0f;
        for (uint32_t c = 0; c < in_ch; ++c) m = m + src[f * in_ch + c];
        m = m / (float)in_ch;
        for (uint32_t k = 0; k < out_ch; ++k) dst[f * out_ch + k] = t.apply(m, (uint32_t)(f * out_ch + k), k, out_ch);
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ------------------------------------------------------------- stepped BltFilter ----
// The filter's formula is replaced while it plays and its memory stays (set_formula, blt.rs:234-252): sample i of a stream's block is
// filtered with the table entry of ITS step, so a change may fall between the channels of one frame.  `row` floats lie between two
// streams' blocks, `table_stride` between their tables (0: one table for all).
struct Biquad5 {
    float b0, b1, b2, a1, a2;
};
__device__ __forceinline__ Biquad5 load5(const float *t) { return Biquad5{t[0], t[1], t[2], t[3], t[4]}; }
constexpr int kLane = 64;  // mode 0: one wave a workgroup, as rh_biquad's kernels (few streams over many CUs)

// Mode 0, any layout: one lane per (stream, channel), 4-byte accesses (k_biquad_seq's shape).
__global__ __launch_bounds__(kLane) void k_biquad_steps_seq(float *dst, const float *src, uint64_t frames, uint64_t row, uint32_t channels, uint32_t n_streams, StepDiv sd,
                                                            const float *__restrict__ coeffs, uint64_t table_stride, float *state) {
    const uint32_t id = blockIdx.x * kLane + threadIdx.x;
    if (id >= n_streams * channels) return;
    const uint32_t stream = id / channels, c = id - stream * channels;
    const float *x = src + (uint64_t)stream * row + c;
    float *y = dst + (uint64_t)stream * row + c;
    const float *tab = coeffs + (uint64_t)stream * table_stride;
    float x1 = 0.f, x2 = 0.f, y1 = 0.f, y2 = 0.f;
    float *st = state ? state + (uint64_t)id * 4 : nullptr;
    if (st) x1 = st[0], x2 = st[1], y1 = st[2], y2 = st[3];
    uint32_t cur = sd.step(c);
    Biquad5 k = load5(tab + 5 * (size_t)cur);
    for (uint64_t n = 0; n < frames; ++n) {
        const uint32_t q = sd.step((uint32_t)(n * channels) + c);
        if (q != cur) cur = q, k = load5(tab + 5 * (size_t)q);
        const float xn = x[n * channels];
        const float r = k.b0 * xn + k.b1 * x1 + k.b2 * x2 - k.a1 * y1 - k.a2 * y2;  // blt.rs:559, left to right
        y2 = y1;
        x2 = x1;
        y1 = r;
        x1 = xn;
        y[n * channels] = r;
    }
    if (st) st[0] = x1, st[1] = x2, st[2] = y1, st[3] = y2;
}

// Mode 0, rows on 16-byte boundaries and C | 16: k_biquad_vec's shape -- one lane per stream, its C channels C independent chains, 16
// samples per 16-byte loads, here issued four blocks ahead.  The step of a block's first and last sample decide whether its 16 samples
// look the table up at all; n_entries: the entries the launch reaches (the next step's entry is read ahead, never past them).
typedef float v4s_t __attribute__((ext_vector_type(4)));
template <int C>
__global__ __launch_bounds__(kLane) void k_biquad_steps_vec(float *dst, const float *src, uint64_t frames, uint64_t row, uint32_t n_streams, StepDiv sd, const float *__restrict__ coeffs,
                                                            uint64_t table_stride, uint32_t n_entries, float *state) {
    static_assert(16 % C == 0, "a block of 16 samples is whole frames");
    const uint32_t stream = blockIdx.x * kLane + threadIdx.x;
    if (stream >= n_streams) return;
    const uint64_t total = frames * C;
    const float *x = src + (uint64_t)stream * row;
    float *y = dst + (uint64_t)stream * row;
    const float *tab = coeffs + (uint64_t)stream * table_stride;
    float x1[C], x2[C], y1[C], y2[C];
    float *st = state ? state + (uint64_t)stream * C * 4 : nullptr;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        x1[c] = st ? st[4 * c] : 0.f;
        x2[c] = st ? st[4 * c + 1] : 0.f;
        y1[c] = st ? st[4 * c + 2] : 0.f;
        y2[c] = st ? st[4 * c + 3] : 0.f;
    }
    // the entry of the current step, and the next one requested as soon as a step begins: the change finds it in registers
    uint32_t cur = sd.step(0);
    Biquad5 k = load5(tab + 5 * (size_t)cur), kn = k;
    if (cur + 1 < n_entries) kn = load5(tab + 5 * (size_t)(cur + 1));
    auto pick = [&](uint32_t q) {
        if (q != cur) {
            if (q != cur + 1) kn = load5(tab + 5 * (size_t)q);  // (a jump over a step does not come through the look-ahead)
            k = kn;
            cur = q;
            if (q + 1 < n_entries) kn = load5(tab + 5 * (size_t)(q + 1));
        }
    };
    auto step = [&](float xn, int c) {
        const float r = k.b0 * xn + k.b1 * x1[c] + k.b2 * x2[c] - k.a1 * y1[c] - k.a2 * y2[c];  // blt.rs:559, left to right
        y2[c] = y1[c];
        x2[c] = x1[c];
        y1[c] = r;
        x1[c] = xn;
        return r;
    };
    const uint64_t blocks = total / 16;
    const v4s_t *xv = reinterpret_cast<const v4s_t *>(x);
    v4s_t *yv = reinterpret_cast<v4s_t *>(y);
    // kAhead blocks in flight: one lane works through a block in far less time than a load takes to arrive
    constexpr int kAhead = 4;
    v4s_t ring[kAhead][4];
    auto fetch = [&](v4s_t (&to)[4], uint64_t b) {
#pragma unroll
        for (int j = 0; j < 4; ++j) to[j] = __builtin_nontemporal_load(xv + b * 4 + j);
    };
    auto work = [&](const v4s_t (&in)[4], uint64_t b) {
        const uint32_t i0 = (uint32_t)(b * 16);
        const uint32_t qa = sd.step(i0), qb = sd.step(i0 + 15u);
        if (qa == qb) {  // one step for the whole block (the usual case: a period is hundreds of samples)
            pick(qa);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v4s_t o;
                o.x = step(in[j].x, (4 * j + 0) % C);
                o.y = step(in[j].y, (4 * j + 1) % C);
                o.z = step(in[j].z, (4 * j + 2) % C);
                o.w = step(in[j].w, (4 * j + 3) % C);
                yv[b * 4 + j] = o;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v4s_t o;
                pick(sd.step(i0 + 4 * j + 0)), o.x = step(in[j].x, (4 * j + 0) % C);
                pick(sd.step(i0 + 4 * j + 1)), o.y = step(in[j].y, (4 * j + 1) % C);
                pick(sd.step(i0 + 4 * j + 2)), o.z = step(in[j].z, (4 * j + 2) % C);
                pick(sd.step(i0 + 4 * j + 3)), o.w = step(in[j].w, (4 * j + 3) % C);
                yv[b * 4 + j] = o;
            }
        }
    };
#pragma unroll
    for (int u = 0; u < kAhead; ++u)
        if ((uint64_t)u < blocks) fetch(ring[u], u);
    uint64_t b = 0;
    for (; b + kAhead <= blocks; b += kAhead) {
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {  // (in place: a block is read before it is written, and the blocks ahead lie behind every store so far)
            work(ring[u], b + u);
            if (b + u + kAhead < blocks) fetch(ring[u], b + u + kAhead);
        }
    }
#pragma unroll
    for (int u = 0; u < kAhead - 1; ++u)
        if (b + u < blocks) work(ring[u], b + u);
    // (fewer than 16 samples, whole frames: the channel of sample i is i % C with a compile-time count per frame)
    for (uint64_t f = blocks * (16 / C); f < frames; ++f) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const uint64_t i = f * C + c;
            pick(sd.step((uint32_t)i));
            y[i] = step(x[i], c);
        }
    }
    if (st) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            st[4 * c] = x1[c];
            st[4 * c + 1] = x2[c];
            st[4 * c + 2] = y1[c];
            st[4 * c + 3] = y2[c];
        }
    }
}

// Mode 1: the time-varying recurrence evaluated in f64, time-parallel inside a tile.  One workgroup per stream walks the stream's
// tiles in order and carries the y state from tile to tile itself (no workgroup waits for another: no tickets, no look-back).  In a
// tile each lane owns a run of kRun consecutive frames; per channel it computes, with each sample's own coefficients, the end state of
// its run from a zero y state (p) and the 2x2 transition of the y state (M) -- the x history is the input's, or the carried state's at
// the block's start.  An inclusive scan of the affine maps s -> M s + p (shuffles of the doubles' halves inside a wave, LDS across the
// four waves) gives every lane its true start state; it runs its frames again from there and stores f32.  No change of basis: the
// maps are products of the filters' own companion matrices, in f64 (a time-varying filter has no common eigenbasis to move to).
constexpr int kScanBlock = 256;
constexpr int kRun = 8;                              // frames a lane owns in a tile
constexpr uint32_t kScanTile = kScanBlock * kRun;    // frames a tile
constexpr uint32_t kScanMaxCh = 8;
struct Aff {  // s = (y[n-1], y[n-2]) -> M s + p
    double m00, m01, m10, m11, p0, p1;
};
__device__ __forceinline__ Aff aff_after(const Aff &b, const Aff &a) {  // a first, then b
    Aff r;
    r.m00 = b.m00 * a.m00 + b.m01 * a.m10;
    r.m01 = b.m00 * a.m01 + b.m01 * a.m11;
    r.m10 = b.m10 * a.m00 + b.m11 * a.m10;
    r.m11 = b.m10 * a.m01 + b.m11 * a.m11;
    r.p0 = b.m00 * a.p0 + b.m01 * a.p1 + b.p0;
    r.p1 = b.m10 * a.p0 + b.m11 * a.p1 + b.p1;
    return r;
}
__device__ __forceinline__ Aff aff_up(const Aff &a, unsigned d) {
    return Aff{__shfl_up(a.m00, d), __shfl_up(a.m01, d), __shfl_up(a.m10, d), __shfl_up(a.m11, d), __shfl_up(a.p0, d), __shfl_up(a.p1, d)};
}
__global__ __launch_bounds__(kScanBlock) void k_biquad_steps_scan(float *__restrict__ dst, const float *__restrict__ src, uint64_t frames, uint64_t row, uint32_t channels, StepDiv sd,
                                                                  const float *__restrict__ coeffs, uint64_t table_stride, float *state) {
    __shared__ double s_wave[kScanBlock / 64][6];
    __shared__ double s_carry[kScanMaxCh][2];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const float *x = src + (uint64_t)blockIdx.x * row;
    float *y = dst + (uint64_t)blockIdx.x * row;
    const float *tab = coeffs + (uint64_t)blockIdx.x * table_stride;
    float *st = state ? state + (uint64_t)blockIdx.x * channels * 4 : nullptr;
    if (t < channels) {
        s_carry[t][0] = st ? (double)st[4 * t + 2] : 0.0;
        s_carry[t][1] = st ? (double)st[4 * t + 3] : 0.0;
    }
    __syncthreads();
    uint32_t cur = 0xffffffffu;
    Biquad5 k{0.f, 0.f, 0.f, 0.f, 0.f};
    for (uint64_t f0 = 0; f0 < frames; f0 += kScanTile) {
        const uint64_t fs = f0 + (uint64_t)t * kRun;  // the lane's first frame
        const uint32_t nr = fs >= frames ? 0u : (frames - fs < (uint64_t)kRun ? (uint32_t)(frames - fs) : (uint32_t)kRun);
        for (uint32_t c = 0; c < channels; ++c) {
            const uint64_t i0 = fs * channels + c;  // the lane's first sample of this channel (< 2^30 where nr > 0)
            float xr[kRun];
#pragma unroll
            for (int j = 0; j < kRun; ++j) xr[j] = (uint32_t)j < nr ? x[i0 + (uint64_t)j * channels] : 0.0f;
            float h1 = 0.0f, h2 = 0.0f;  // the two frames in front of the run
            if (nr) {
                h1 = fs >= 1 ? x[i0 - channels] : (st ? st[4 * c] : 0.0f);
                h2 = fs >= 2 ? x[i0 - 2 * (uint64_t)channels] : (st ? st[4 * c + (fs == 1 ? 0 : 1)] : 0.0f);
            }
            // the run from a zero y state, and the transition of the y state across it
            Aff a{1.0, 0.0, 0.0, 1.0, 0.0, 0.0};
            {
                double x1 = (double)h1, x2 = (double)h2;
#pragma unroll
                for (int j = 0; j < kRun; ++j) {
                    if ((uint32_t)j < nr) {
                        const uint32_t q = sd.step((uint32_t)i0 + (uint32_t)j * channels);
                        if (q != cur) cur = q, k = load5(tab + 5 * (size_t)q);
                        const double xn = (double)xr[j], a1 = (double)k.a1, a2 = (double)k.a2;
                        const double r = (double)k.b0 * xn + (double)k.b1 * x1 + (double)k.b2 * x2 - a1 * a.p0 - a2 * a.p1;
                        a.p1 = a.p0, a.p0 = r;
                        const double n00 = -a1 * a.m00 - a2 * a.m10, n01 = -a1 * a.m01 - a2 * a.m11;
                        a.m10 = a.m00, a.m11 = a.m01, a.m00 = n00, a.m01 = n01;
                        x2 = x1, x1 = xn;
                    }
                }
            }
            // inclusive scan over the wave, then over the waves in front
#pragma unroll
            for (unsigned d = 1; d < 64; d <<= 1) {
                const Aff e = aff_up(a, d);
                if (lane >= d) a = aff_after(a, e);
            }
            if (lane == 63u) {
                double *o = s_wave[w];
                o[0] = a.m00, o[1] = a.m01, o[2] = a.m10, o[3] = a.m11, o[4] = a.p0, o[5] = a.p1;
            }
            Aff ex = aff_up(a, 1);  // the lanes in front of this one, inside the wave
            if (lane == 0u) ex = Aff{1.0, 0.0, 0.0, 1.0, 0.0, 0.0};
            __syncthreads();
            Aff all{1.0, 0.0, 0.0, 1.0, 0.0, 0.0}, pre = all;  // the whole tile (thread 0 carries it on); the waves in front of this one
            for (uint32_t v = 0; v < kScanBlock / 64; ++v) {
                const double *o = s_wave[v];
                const Aff wv{o[0], o[1], o[2], o[3], o[4], o[5]};
                all = aff_after(wv, all);
                if (v + 1 == w) pre = all;
            }
            ex = aff_after(ex, pre);
            const double c0 = s_carry[c][0], c1 = s_carry[c][1];
            double y1 = ex.m00 * c0 + ex.m01 * c1 + ex.p0, y2 = ex.m10 * c0 + ex.m11 * c1 + ex.p1;
            __syncthreads();
            if (t == 0) {
                s_carry[c][0] = all.m00 * c0 + all.m01 * c1 + all.p0;
                s_carry[c][1] = all.m10 * c0 + all.m11 * c1 + all.p1;
            }
            // the run again from its true start state
            {
                double x1 = (double)h1, x2 = (double)h2;
#pragma unroll
                for (int j = 0; j < kRun; ++j) {
                    if ((uint32_t)j < nr) {
                        const uint32_t q = sd.step((uint32_t)i0 + (uint32_t)j * channels);
                        if (q != cur) cur = q, k = load5(tab + 5 * (size_t)q);
                        const double xn = (double)xr[j];
                        const double r = (double)k.b0 * xn + (double)k.b1 * x1 + (double)k.b2 * x2 - (double)k.a1 * y1 - (double)k.a2 * y2;
                        y2 = y1, y1 = r, x2 = x1, x1 = xn;
                        y[i0 + (uint64_t)j * channels] = (float)r;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (st && t < channels) {  // mode 0's layout: the last two inputs, the last two outputs rounded to f32
        const float old1 = st[4 * t];
        st[4 * t] = x[(frames - 1) * channels + t];
        st[4 * t + 1] = frames >= 2 ? x[(frames - 2) * channels + t] : old1;
        st[4 * t + 2] = (float)s_carry[t][0];
        st[4 * t + 3] = (float)s_carry[t][1];
    }
}

}  // namespace

uint64_t rh_periodic_update_samples(uint64_t period_ns, uint32_t sample_rate, uint32_t channels) {
    // periodic.rs:14-22: (period.as_secs_f32() * rate as f32 * channels as f32) as usize, at least 1.  Duration::as_secs_f32 is
    // secs as f32 + subsec_nanos as f32 / 1e9 (f32); `as usize` saturates.
    const float secs = (float)(period_ns / 1000000000ull) + (float)(uint32_t)(period_ns % 1000000000ull) / 1000000000.0f;
    const float u = secs * (float)sample_rate * (float)channels;
    if (!(u >= 1.0f)) return 1;
    if (u >= 18446744073709551616.0f) return UINT64_MAX;
    return (uint64_t)u;
}

rh_status rh_amplify_steps(float *dst, const float *src, size_t n, uint64_t first, uint64_t period, const float *factors_dev, uint32_t n_factors, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (period == 0) return RH_ERR_INVALID;
    if (n == 0) return RH_OK;
    if (!dst || !src || !factors_dev || steps_needed(first, period, n) > n_factors) return RH_ERR_INVALID;
    for (uint64_t i0 = 0; i0 < n; i0 += kMaxLaunchSamples) {
        const uint64_t m = n - i0 < kMaxLaunchSamples ? n - i0 : kMaxLaunchSamples;
        const uint64_t at = first + i0;
        const StepDiv sd = step_div(at, period, m);
        if (period >= 4)
            hipLaunchKernelGGL(k_amplify_steps<true>, dim3(rh::grid_tiles((m + 3) / 4)), dim3(kBlock), 0, rh::as_stream(stream), dst + i0, src + i0, (size_t)m, sd,
                               factors_dev + (at / period - first / period), rh::rows_vec_bits(dst + i0, src + i0));
        else
            hipLaunchKernelGGL(k_amplify_steps<false>, dim3(rh::grid_tiles((m + 3) / 4)), dim3(kBlock), 0, rh::as_stream(stream), dst + i0, src + i0, (size_t)m, sd,
                               factors_dev + (at / period - first / period), rh::rows_vec_bits(dst + i0, src + i0));
        RH_CHECK_LAUNCH();
    }
    return RH_OK;
}

rh_status rh_channel_volume_steps(float *dst, const float *src, size_t frames, uint32_t in_ch, uint32_t out_ch, uint64_t first, uint64_t gain_period, const float *gains_dev,
                                  uint32_t n_gains, uint64_t factor_first, uint64_t factor_period, const float *factors_dev, uint32_t n_factors, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (in_ch == 0 || out_ch == 0 || out_ch > 16 || gain_period == 0 || (factors_dev && factor_period == 0)) return RH_ERR_INVALID;
    if (frames == 0) return RH_OK;
    const uint64_t total = (uint64_t)frames * out_ch;
    if (!dst || !src || !gains_dev || steps_needed(first, gain_period, total) > n_gains) return RH_ERR_INVALID;
    if (factors_dev && steps_needed(factor_first, factor_period, total) > n_factors) return RH_ERR_INVALID;
    // launches of whole frames, a multiple of 4 (the tile's first output sample starts a 16-byte vector), <= 2^30 output samples
    const uint64_t chunk = (kMaxLaunchSamples / out_ch) & ~3ull;
    for (uint64_t f0 = 0; f0 < frames; f0 += chunk) {
        const uint64_t nf = frames - f0 < chunk ? frames - f0 : chunk, j = f0 * out_ch, m = nf * out_ch;
        Tables t{gains_dev + (size_t)((first + j) / gain_period - first / gain_period) * out_ch, nullptr, step_div(first + j, gain_period, m), StepDiv{0, 1, 0, 0}};
        if (factors_dev) {
            t.factors = factors_dev + ((factor_first + j) / factor_period - factor_first / factor_period);
            t.f = step_div(factor_first + j, factor_period, m);
        }
        float *d = dst + j;
        const float *s = src + f0 * in_ch;
        if (in_ch == 2 && out_ch == 2) {
            hipLaunchKernelGGL(k_channel_volume_steps_2x2, dim3(rh::grid_tiles((nf + 1) / 2)), dim3(kBlock), 0, rh::as_stream(stream), d, s, (size_t)nf, t, (int)(aligned16(d) && aligned16(s)));
        } else {
            const uint64_t tf = (10240ull / (4ull * (in_ch + out_ch))) & ~3ull;  // ~10 KiB in + out a tile, as rh_channel_volume
            if (tf >= 8) {
                const uint32_t in_floats = (uint32_t)((tf * in_ch + 4 + 3) & ~3ull);
                const size_t lds = ((size_t)in_floats + tf) * 4;
                hipLaunchKernelGGL(k_channel_volume_steps_tile, dim3((unsigned)((nf + tf - 1) / tf)), dim3(kBlock), lds, rh::as_stream(stream), d, s, (size_t)nf, in_ch, out_ch, t,
                                   (uint32_t)tf, in_floats, (int)aligned16(d));
            } else {
                hipLaunchKernelGGL(k_channel_volume_steps, dim3(rh::grid_for(nf)), dim3(kBlock), 0, rh::as_stream(stream), d, s, (size_t)nf, in_ch, out_ch, t);
            }
        }
        RH_CHECK_LAUNCH();
    }
    return RH_OK;
}

rh_status rh_biquad_steps(float *dst, const float *src, uint64_t frames, uint32_t channels, uint32_t n_streams, uint64_t first, uint64_t period, const float *coeffs_dev,
                          uint32_t n_steps, uint64_t table_stride, float *state, int32_t mode, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (period == 0 || channels == 0 || (mode != 0 && mode != 1)) return RH_ERR_INVALID;
    if (frames == 0 || n_streams == 0) return RH_OK;
    const uint64_t row = frames * channels;
    if (!dst || !src || !coeffs_dev || steps_needed(first, period, row) > n_steps) return RH_ERR_INVALID;
    if (table_stride != 0 && table_stride < 5ull * n_steps) return RH_ERR_INVALID;
    hipStream_t s = rh::as_stream(stream);
    if (mode == 1) {  // what the time-parallel kernel does not take continues in the reference's order: the same state layout, the exact bits
        const uint64_t total = row * n_streams;
        const bool overlap = dst < src + total && src < dst + total;  // in place: a lane's history frames are its neighbour's outputs by then
        if (channels > kScanMaxCh || overlap) mode = 0;
    }
    // launches of whole frames, <= 2^30 samples of a stream each (StepDiv); a stream's state goes from one to the next -- the caller's, or for
    // a state-less call of more than one launch the stream's scratch
    const uint64_t chunk = (kMaxLaunchSamples / channels) & ~3ull;
    float *st = state;
    std::unique_lock<std::mutex> scratch_hold;
    if (!st && frames > chunk) {
        const size_t bytes = sizeof(float) * 4 * (size_t)channels * n_streams;
        RH_HIP_TRY(rh::stream_scratch(s, bytes, reinterpret_cast<void **>(&st), scratch_hold));
        RH_HIP_TRY(rh::fill_async(st, 0, bytes, s));
    }
    for (uint64_t f0 = 0; f0 < frames; f0 += chunk) {
        const uint64_t nf = frames - f0 < chunk ? frames - f0 : chunk, at = first + f0 * channels;
        const StepDiv sd = step_div(at, period, nf * channels);
        const float *tab = coeffs_dev + 5 * (at / period - first / period);
        const uint32_t reach = (uint32_t)steps_needed(at, period, nf * channels);  // entries of `tab` this launch reaches
        float *d = dst + f0 * channels;
        const float *x = src + f0 * channels;
        if (mode == 1) {
            hipLaunchKernelGGL(k_biquad_steps_scan, dim3(n_streams), dim3(kScanBlock), 0, s, d, x, nf, row, channels, sd, tab, table_stride, st);
        } else {
            const bool vec = aligned16(d) && aligned16(x) && (n_streams == 1 || row % 4 == 0);
            const dim3 grid_v((n_streams + kLane - 1) / kLane);
            if (vec && channels == 1) hipLaunchKernelGGL(k_biquad_steps_vec<1>, grid_v, dim3(kLane), 0, s, d, x, nf, row, n_streams, sd, tab, table_stride, reach, st);
            else if (vec && channels == 2) hipLaunchKernelGGL(k_biquad_steps_vec<2>, grid_v, dim3(kLane), 0, s, d, x, nf, row, n_streams, sd, tab, table_stride, reach, st);
            else if (vec && channels == 4) hipLaunchKernelGGL(k_biquad_steps_vec<4>, grid_v, dim3(kLane), 0, s, d, x, nf, row, n_streams, sd, tab, table_stride, reach, st);
            else if (vec && channels == 8) hipLaunchKernelGGL(k_biquad_steps_vec<8>, grid_v, dim3(kLane), 0, s, d, x, nf, row, n_streams, sd, tab, table_stride, reach, st);
            else {
                const uint64_t lanes = (uint64_t)n_streams * channels;
                if (lanes > 0xffffffffull) return RH_ERR_INVALID;
                hipLaunchKernelGGL(k_biquad_steps_seq, dim3((unsigned)((lanes + kLane - 1) / kLane)), dim3(kLane), 0, s, d, x, nf, row, channels, n_streams, sd, tab, table_stride, st);
            }
        }
        RH_CHECK_LAUNCH();
    }
    return RH_OK;
}
