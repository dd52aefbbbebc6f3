// rh_clip_mix_plan.h -- what rh_clip_mix_block (rh_clipmix.hip) decides on the host, as plain functions over the caller's arrays: the words of
// a clip -- a resident sound behind delay(at), cut by take_duration(len), maybe with the fade-out filter -- (clip_plan), the cursor behind a
// block (clip_advance), the status of a call, the descriptor of a source with its positions REBASED on the block's first converter chain,
// where an output frame's taps lie (locate(): the one function the kernel and the tests share) and the fade's millisecond step of a tap
// (fade_ms()).  No HIP: tests/cpp/clip_mix_plan_test.cpp runs it without a GPU.  Building the kernel table and launching are
// rh_clip_mix_block's.  Nothing here allocates.
//
// The stream of a clip (include/rodio_hip.h has the Rust lines): Z samples of +0.0, then the N admitted samples x_k * g (* R_k / Tt with the
// fade-out), read as frames of `ch` samples BY STREAM POSITION.  Converter chains cut it
//   rule G  at every multiple of 32768 samples from stream position 0, the last chain over what is left;
//   rule C  nowhere: the stream is one chain.
// A chain of f frames emits span_out(f) output frames; output frame j of it reads frames i = floor(j F / T) and i + 1 of the chain, the frame
// with i == f - 1 verbatim.  The cursor is ONE number, the output frames the clip has emitted: the chain in progress, the frame inside it
// (rule G) and the first tap with its phase (rule C) follow from it by exact integer arithmetic on the host, in 128 bits where 64 would not
// do, and the kernel sees positions counted from that chain's (that tap's) first sample only.
#pragma once
#include <cstdint>

#include "../../include/rodio_hip.h"
#include "rh_mix_plan.h"

namespace rh {
namespace clipmix {

namespace lm = rh::mixplan;  // the rules the block mixers share
using lm::Div;
using lm::div_u32;
using lm::kChainSamples;
using lm::kChunk;  // sources a launch
using lm::kDivZero;
using lm::kGroup;  // ... walked in groups of this many
using lm::Launch;  // every source brings its own positions: a launch is full at kChunk sources and for no other reason
using lm::make_div;
using lm::walk;
typedef unsigned __int128 u128;

constexpr uint64_t kMaxStream = 1ull << 62;  // Z, N and Z + N stay below this: every sum below fits 64 bits
constexpr uint64_t kNsPerMs = 1000000ull;
// floor(x / 10^6) for every x < 2^32 (lm::make_div(10^6), spelled out so that the kernel holds it as two literals)
constexpr Div kDivMs = Div{0x0c6f7a0cu, 1u | (19u << 8)};
static_assert(kDivMs.m == (uint32_t)(((1ull << 32) * ((1ull << 20) - kNsPerMs)) / kNsPerMs + 1) && (1ull << 19) < kNsPerMs && kNsPerMs <= (1ull << 20), "the round-up reciprocal of 10^6");

enum Kind : uint64_t { kPlain = 0, kRuleG = 1, kRuleC = 2 };
enum Flags : uint64_t { kTake = 1, kFade = 2 };
enum FadeMode : uint32_t { kNoFade = 0, kFade32 = 1, kFade64 = 2 };

// The words of a source.
struct Words {
    uint64_t kind, Z, N, take_ns, flags, done, total;
};
inline Words words_of(const uint64_t *w) { return Words{w[0], w[1], w[2], w[3], w[4], w[5], w[6]}; }

// Output frames of a complete chain of n input frames, rh_uniform_span_frames(n, F, T, 1, ..), for any n below 2^62 (lm::span_out in 128 bits).
inline u128 span_out_wide(uint64_t n, uint64_t F, uint64_t T) {
    if (F == T || n == 0) return n;
    u128 c = ((u128)(n - 1) * T + F - 1) / F;
    if (c * F < (u128)n * T) c += 1;
    return c;
}

inline uint64_t ns_per_sample(uint32_t channels, uint32_t rate) { return 1000000000ull / ((uint64_t)rate * channels); }  // take.rs:63-67

// What the words say of a clip whatever the block is.
struct Shape {
    uint64_t Ls;     // samples of the stream, Z + N
    uint64_t Lf;     // ... in frames
    uint64_t c;      // frames of a whole chain (rule C, or a stream of at most 32768 samples: Lf)
    uint64_t M;      // output frames of a whole chain
    uint64_t total;  // ... of the clip
    uint64_t dps;    // ns a sample (0 without a take)
};
// RH_ERR_INVALID for words no plan gives, RH_ERR_UNSUPPORTED for a chain that ends inside a frame or counts that leave 64 bits.
inline rh_status shape_of(const Words &w, uint32_t channels, uint32_t from_rate, uint64_t F, uint64_t T, Shape *out) {
    if (w.kind > kRuleC || w.flags > 3 || ((w.flags & kFade) && !(w.flags & kTake)) || channels == 0 || from_rate == 0) return RH_ERR_INVALID;
    if (w.kind == kRuleC && (w.flags & kTake)) return RH_ERR_INVALID;  // TakeDuration always answers Some: rule G
    if (w.Z > kMaxStream || w.N > kMaxStream || w.Z + w.N > kMaxStream) return RH_ERR_UNSUPPORTED;
    Shape s{};
    if (w.flags & kTake) {
        s.dps = ns_per_sample(channels, from_rate);
        if (s.dps == 0) return RH_ERR_UNSUPPORTED;            // above 1 GHz * channel the reference never expires (rh_take_duration's answer)
        if (w.N > w.take_ns / s.dps) return RH_ERR_INVALID;  // more samples than the duration admits
    }
    s.Ls = w.Z + w.N;
    if (s.Ls % channels) return RH_ERR_UNSUPPORTED;  // the last chain ends inside a frame
    s.Lf = s.Ls / channels;
    if (w.kind == kRuleG && s.Ls > kChainSamples) {
        if (kChainSamples % channels) return RH_ERR_UNSUPPORTED;  // every chain does
        s.c = kChainSamples / channels;
    } else {
        s.c = s.Lf;
    }
    if (s.c == 0) {
        *out = s;  // an empty stream: no output frame, nothing else to hold
        return w.done == 0 ? RH_OK : RH_ERR_INVALID;
    }
    const u128 M = span_out_wide(s.c, F, T);
    const u128 total = (u128)(s.Lf / s.c) * M + span_out_wide(s.Lf % s.c, F, T);
    if (total > ((u128)1 << 63)) return RH_ERR_UNSUPPORTED;
    s.M = (uint64_t)M, s.total = (uint64_t)total;
    if (w.kind == kRuleG && s.M * F > 0xffffffffull) return RH_ERR_UNSUPPORTED;  // j F of every output frame of a chain (M <= 2^15 T + 1: no overflow here)
    if (w.done > s.total) return RH_ERR_INVALID;
    *out = s;
    return RH_OK;
}

// The words of a sound of n_samples samples with `channels` channels at `rate`, as rodio plays
//     sound.amplify(g).take_duration(take_ns) [.set_filter_fadeout()] .delay(delay_ns)
// span_len is what the sound answers to current_span_len() (0: None; >= n_samples: its whole length).  The cursor starts at 0; word 6, the
// clip's output frames, depends on the mixer's rate: clip_advance writes it.
inline rh_status clip_plan(uint64_t *words, uint64_t n_samples, uint32_t channels, uint32_t rate, uint64_t span_len, uint64_t delay_ns, uint64_t take_ns, uint32_t flags) {
    if (!words || channels == 0 || rate == 0 || flags > 3 || ((flags & kFade) && !(flags & kTake))) return RH_ERR_INVALID;
    if (span_len != 0 && span_len < n_samples) return RH_ERR_UNSUPPORTED;  // spans shorter than the sound cut chains elsewhere
    const u128 Z = (u128)delay_ns * channels * rate / 1000000000ull;  // delay.rs:8-16
    if (n_samples > kMaxStream || Z > kMaxStream || (uint64_t)Z + n_samples > kMaxStream) return RH_ERR_UNSUPPORTED;
    uint64_t N = n_samples;
    if (flags & kTake) {
        const uint64_t dps = ns_per_sample(channels, rate);
        if (dps == 0) return RH_ERR_UNSUPPORTED;
        const uint64_t left = take_ns / dps;  // take.rs:107-147: a sample is taken while remaining >= dps
        N = left < N ? left : N;
    }
    const uint64_t kind = ((flags & kTake) || span_len != 0) ? kRuleG : kRuleC;
    const uint64_t Ls = (uint64_t)Z + N;
    if (Ls % channels) return RH_ERR_UNSUPPORTED;
    if (kind == kRuleG && Ls > kChainSamples && kChainSamples % channels) return RH_ERR_UNSUPPORTED;
    words[0] = kind, words[1] = (uint64_t)Z, words[2] = N, words[3] = (flags & kTake) ? take_ns : 0, words[4] = flags, words[5] = 0, words[6] = 0;
    return RH_OK;
}

struct Rates {
    uint64_t F, T;
};
inline rh_status rates_of(uint32_t from_rate, uint32_t to_rate, Rates *r) {
    if (from_rate == 0 || to_rate == 0) return RH_ERR_INVALID;
    uint32_t F, T;
    lm::reduce(from_rate, to_rate, &F, &T);
    r->F = F, r->T = T;
    return r->F * r->T > 0xffffffffull ? RH_ERR_UNSUPPORTED : RH_OK;  // the reference multiplies in u32 (sample_rate.rs:157,173)
}

// The cursor behind a block of out_frames frames (it stops at the clip's end), and the clip's output frames at this pair of rates.
inline rh_status clip_advance(uint64_t *words, uint32_t channels, uint32_t from_rate, uint32_t to_rate, uint64_t out_frames) {
    if (!words) return RH_ERR_INVALID;
    const Words w = words_of(words);
    if (w.kind == kPlain) return RH_OK;  // not a clip: data and phase move, as for rh_wide_mix_block
    Rates r;
    rh_status st = rates_of(from_rate, to_rate, &r);
    if (st != RH_OK) return st;
    Shape s;
    st = shape_of(w, channels, from_rate, r.F, r.T, &s);
    if (st != RH_OK) return st;
    const uint64_t left = s.total - w.done;
    words[5] = w.done + (out_frames < left ? out_frames : left), words[6] = s.total;
    return RH_OK;
}

// One slot of the kernel's table: a source, clip or not, as the positions of locate().  Stream samples are counted from `base`, the first
// sample of the chain in progress at the block's first frame (rule C: of the frame of the block's first tap).
struct Desc {
    const float *data;  // clips: the sound's sample max(base - Z, 0); plain sources: the frame of the block's first tap
    uint32_t ch;        // channels of the source
    uint32_t frames;    // output frames the source reaches (0: a slot that pads the table to whole groups)
    float gain;
    float Tf;           // T as a float; 0: the converter passes through (F == T)
    uint32_t F, T;      // reduced rates
    uint32_t r0;        // plain sources and rule C: the block's phase; rule G: 0 (every chain starts a converter)
    uint32_t x0;        // rule G: output frames of the chain in progress that earlier blocks emitted; otherwise 0
    uint32_t M;         // rule G: output frames of a whole chain; otherwise 0 (with dM = kDivZero: everything is chain 0)
    uint32_t c;         // rule G: input frames of a whole chain; otherwise 0
    uint32_t klast;     // the stream's last chain, counted from the chain in progress (0xffffffff: out of the block's reach)
    uint32_t nl;        // the last frame of a whole chain, c - 1: verbatim (plain: `last`)
    uint32_t nl_last;   // ... of the stream's last chain (rule C: of the stream, counted from base)
    uint32_t zrel;      // stream samples below this, counted from base, are the delay's +0.0: min(max(Z - base, 0), 2^32 - 1)
    uint32_t fade;      // FadeMode
    uint32_t dps;       // ns a sample
    uint32_t ns_pad;    // 999999 - (remaining ns at data[0]) mod 10^6
    float Ttf;          // float(floor(take_ns / 10^6))
    uint64_t ms0;       // floor(remaining ns at data[0] / 10^6)
    Div dM, dT;
};
static_assert(sizeof(Desc) == 104, "32 of them and the other arguments share one 4 KiB kernel-argument segment");

struct Taps {
    uint32_t ia;   // the frame of the first tap, counted from base; the second one is the next frame (read only where lerp is set)
    bool lerp;     // false: frame ia verbatim (a chain's last frame, F == T)
    uint32_t num;  // (position) mod T: the lerp's weight over T
};
// Output frame m of the block.  Every intermediate fits 32 bits for a call check() has passed.
RH_MIX_HD Taps locate(const Desc &d, uint32_t m) {
    const uint32_t x = d.x0 + m;
    const uint32_t k = div_u32(x, d.dM), j = x - k * d.M;  // the chain and the frame inside it
    const uint32_t pos = d.r0 + j * d.F;
    const uint32_t i = div_u32(pos, d.dT);
    Taps t;
    t.num = pos - i * d.T;
    t.lerp = d.Tf != 0.0f && i < (k == d.klast ? d.nl_last : d.nl);
    t.ia = k * d.c + i;
    return t;
}
// The stream sample of channel k of frame ia, counted from the descriptor's origin.  64 bits: a clip's stays below 2^32 (describe() refuses
// the block otherwise), a plain source's need not -- rh_wide_mix_block bounds its positions phase + j F, not frame * channels, and a plain
// source is read as that entry reads it.
RH_MIX_HD uint64_t tap_sample(const Desc &d, uint32_t ia, uint32_t k) { return (uint64_t)ia * d.ch + k; }
// take.rs:33-41 for the sound's sample data[krel]: float(floor(remaining / 10^6)), remaining = ms0 10^6 + (999999 - ns_pad) - krel dps, which is
// ms0 - floor((krel dps + ns_pad) / 10^6): 0 <= ns_pad <= 999999, so the numerator is never negative.  kFade32: it and ms0 fit 32 bits.
RH_MIX_HD float fade_ms(const Desc &d, uint32_t krel) {
    if (d.fade == kFade32) return (float)((uint32_t)d.ms0 - div_u32(krel * d.dps + d.ns_pad, kDivMs));
    return (float)(d.ms0 - ((uint64_t)krel * d.dps + d.ns_pad) / kNsPerMs);
}

// The status of one source with frames > 0 (anything but RH_OK: nothing may be launched), and its descriptor.
inline rh_status describe(const rh_wide_src &x, const uint64_t *words, uint32_t channels, uint32_t to_rate, uint64_t out_frames, Desc *out) {
    const Words w = words_of(words);
    Desc d{};
    if (w.kind == kPlain) {  // rh_wide_mix_block's source
        lm::Reach r;
        const rh_status st = lm::check_src(x, channels, to_rate, out_frames, &r);
        if (st != RH_OK) return st;
        d.data = x.data, d.ch = x.channels, d.frames = (uint32_t)x.frames, d.gain = x.gain, d.Tf = r.F == r.T ? 0.0f : (float)r.T, d.F = r.F, d.T = r.T, d.r0 = x.phase;
        d.klast = 0u, d.nl = d.nl_last = x.last, d.dM = kDivZero, d.dT = make_div(r.T);
        *out = d;
        return RH_OK;
    }
    rh_wide_src y = x;
    y.phase = 0;  // (a clip's positions come from its words: the field is not read)
    uint32_t F32, T32;
    uint64_t fit;
    rh_status st = lm::check_src(y, to_rate, out_frames, &F32, &T32, &fit);
    if (st != RH_OK) return st;
    const Rates r{F32, T32};
    Shape s;
    st = shape_of(w, x.channels, x.from_rate, r.F, r.T, &s);
    if (st != RH_OK) return st;
    if (x.frames > s.total - w.done) return RH_ERR_INVALID;  // behind its last chain the clip has ended
    const uint64_t F = r.F, T = r.T, ch = x.channels;
    uint64_t base, reach;  // the first stream sample of the descriptor's origin; stream samples from there on that a tap may touch
    d.data = x.data, d.ch = x.channels, d.frames = (uint32_t)x.frames, d.gain = x.gain, d.Tf = F == T ? 0.0f : (float)T, d.F = (uint32_t)F, d.T = (uint32_t)T, d.dT = make_div(T);
    if (w.kind == kRuleG) {
        const uint64_t q0 = w.done / s.M, j0 = w.done - q0 * s.M;
        const uint64_t x_last = j0 + x.frames - 1;
        if (x_last > 0xffffffffull) return RH_ERR_UNSUPPORTED;
        base = q0 * s.c * ch;
        reach = (x_last / s.M + 1) * s.c * ch;
        const uint64_t tail = s.Lf % s.c, kl = (tail ? s.Lf / s.c : s.Lf / s.c - 1) - q0;
        d.x0 = (uint32_t)j0, d.M = (uint32_t)s.M, d.c = (uint32_t)s.c, d.dM = make_div(s.M);
        d.klast = kl > 0xffffffffull ? 0xffffffffu : (uint32_t)kl, d.nl = (uint32_t)s.c - 1u, d.nl_last = (uint32_t)(tail ? tail : s.c) - 1u;
    } else {
        const u128 pos = (u128)w.done * F;
        const uint64_t i0 = (uint64_t)(pos / T), r0 = (uint64_t)(pos % T);
        const uint64_t p_last = r0 + (x.frames - 1) * F;  // (r0 < 2^32, frames < 2^31, F < 2^32)
        if (p_last > 0xffffffffull) return RH_ERR_UNSUPPORTED;
        base = i0 * ch;
        reach = (p_last / T + 2) * ch;
        const uint64_t left = s.Lf - i0 - 1;  // (i0 < Lf: the clip has frames left)
        d.r0 = (uint32_t)r0, d.dM = kDivZero, d.klast = 0u, d.nl = d.nl_last = left > 0xffffffffull ? 0xffffffffu : (uint32_t)left;
    }
    if (reach > s.Ls - base) reach = s.Ls - base;
    if (reach > 0xffffffffull) return RH_ERR_UNSUPPORTED;  // a sample index of the block, counted from base, leaves 32 bits
    d.zrel = w.Z > base ? (w.Z - base > 0xffffffffull ? 0xffffffffu : (uint32_t)(w.Z - base)) : 0u;
    const uint64_t kbase = base > w.Z ? base - w.Z : 0;  // (below N wherever the block reaches a sample of the sound)
    d.data = x.data + kbase;
    if (w.flags & kFade) {
        const uint64_t rem0 = w.take_ns - kbase * s.dps;  // (kbase < N <= take_ns / dps)
        d.ms0 = rem0 / kNsPerMs, d.ns_pad = (uint32_t)(kNsPerMs - 1 - rem0 % kNsPerMs), d.dps = (uint32_t)s.dps, d.Ttf = (float)(w.take_ns / kNsPerMs);
        d.fade = (d.ms0 <= 0xffffffffull && reach * s.dps + d.ns_pad <= 0xffffffffull) ? kFade32 : kFade64;  // (reach < 2^32, dps <= 10^9: no overflow here)
    }
    *out = d;
    return RH_OK;
}
// A slot that reaches no frame (its data is never read).
inline Desc pad_slot() {
    Desc d{};
    d.ch = 1u, d.F = 1u, d.T = 1u, d.dM = kDivZero, d.dT = make_div(1);
    return d;
}

// The status of a call.  out_frames == 0 is answered by the caller: nothing is looked at.
inline rh_status check(const float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs, uint32_t n_sources, const uint64_t *clips) {
    if (!dst || channels == 0 || to_rate == 0 || (n_sources && (!srcs || !clips))) return RH_ERR_INVALID;
    if (out_frames > 0x7fffffffull) return RH_ERR_UNSUPPORTED;
    for (uint32_t s = 0; s < n_sources; ++s) {
        if (srcs[s].frames == 0) continue;  // not looked at
        Desc d;
        const rh_status st = describe(srcs[s], clips + (size_t)RH_CLIP_WORDS * s, channels, to_rate, out_frames, &d);
        if (st != RH_OK) return st;
    }
    return RH_OK;
}

}  // namespace clipmix
}  // namespace rh
