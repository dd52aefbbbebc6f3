// rh_loop_mix_plan.h -- what rh_loop_mix_block (rh_loopmix.hip) decides on the host, as plain functions over the caller's arrays: the rule
// and the chain length of a sound handed to repeat_infinite() (rh_loop_plan), the cursor behind a block (rh_loop_advance), the status of a
// call, the descriptor of a source -- its positions with their exact reciprocals --, where an output frame's taps lie (locate(): the one
// function the kernel and the tests share), and the sources of every launch.  No HIP: tests/cpp/loop_mix_plan_test.cpp runs it without a
// GPU.  Building the kernel table and launching are rh_loop_mix_block's.  Nothing here allocates.
//
// The two rules (include/rodio_hip.h has the Rust lines).  A pass is the L frames of the sound; a CHAIN is what one converter of
// UniformSourceIterator takes: n input frames in, span_out(n) output frames out, output frame j of it reading frames i = floor(j F / T) and
// i + 1 of the chain, the frame with i == n - 1 verbatim.
//   rule 0  chains start over at every pass: floor(L / c) chains of c frames and one of L mod c where that is not 0.  A pass emits
//           P = floor(L / c) span_out(c) + span_out(L mod c) frames, and output frame x of the stream lies at p = x mod P of its pass, in
//           chain k = floor(p / span_out(c)) -- the tail chain is never longer than a whole one, so the quotient is right for it too.
//   rule 1  chains of c frames of the UNROLLED stream: chain k behind the cursor's starts at frame (chain_start + k c) mod L, and both
//           taps are taken mod L.
#pragma once
#include <cstdint>

#include "../../include/rodio_hip.h"
#include "rh_mix_plan.h"

namespace rh {
namespace loopmix {

using mixplan::Div;
using mixplan::div_u32;
using mixplan::kChainSamples;
using mixplan::kChunk;  // sources a launch
using mixplan::kDivZero;
using mixplan::kGroup;  // ... walked in groups of this many: a launch's slots are whole groups
using mixplan::Launch;  // every source brings its own positions: a launch is full at kChunk sources and for no other reason
using mixplan::make_div;
using mixplan::span_out;
using mixplan::walk;

constexpr uint64_t kMaxLoopFrames = 1ull << 31;  // base + i + 1 < 2 L stays inside 32 bits

// The words of a source.
struct Words {
    uint64_t L, c, rule, chain_start, chain_out;
};
inline Words words_of(const uint64_t *w) { return Words{w[0], w[1], w[2], w[3], w[4]}; }

// The rule and the chain length rodio plays a sound of n_samples samples with, handed to repeat_infinite() while it answers span_len to
// current_span_len() (0: None).  The cursor starts at 0.
inline rh_status loop_plan(uint64_t n_samples, uint32_t channels, uint64_t span_len, uint64_t *words) {
    if (!words || channels == 0 || n_samples == 0) return RH_ERR_INVALID;
    if (n_samples % channels) return RH_ERR_UNSUPPORTED;  // the pass itself ends inside a frame
    uint64_t chain = 0, rule = 0;
    if (span_len == 0 || span_len == n_samples) {
        // Buffered over None: spans of 32768 samples (buffered.rs:97-126).  Over a SamplesBuffer: ONE span, and a chain every 32768 samples of
        // the unrolled stream (buffered.rs:207-214, uniform.rs:56).
        chain = n_samples <= kChainSamples ? n_samples : kChainSamples;
        rule = (span_len != 0 && n_samples > kChainSamples) ? 1 : 0;
    } else if (span_len <= kChainSamples) {
        chain = span_len < n_samples ? span_len : n_samples;  // constant spans (decoder packets): every span a chain, the last one shorter
    } else {
        return RH_ERR_UNSUPPORTED;
    }
    if (chain % channels) return RH_ERR_UNSUPPORTED;  // a chain that cuts a frame: the unrolled path plays those (rh_uniform_row)
    words[0] = n_samples / channels, words[1] = chain / channels, words[2] = rule, words[3] = 0, words[4] = 0;
    return RH_OK;
}

// What the words must satisfy whatever the block is: RH_ERR_INVALID for a broken rule, chain or cursor, RH_ERR_UNSUPPORTED for a loop or a
// chain whose positions leave 32 bits.  M receives span_out(c), P the output frames of a pass (rule 0; 0 under rule 1).
inline rh_status check_words(const Words &w, uint32_t channels, uint64_t F, uint64_t T, uint64_t *M, uint64_t *P) {
    if (w.rule > 1 || w.c == 0 || w.c > kChainSamples || w.c * channels > kChainSamples) return RH_ERR_INVALID;
    if (w.rule == 1 && w.L < w.c) return RH_ERR_INVALID;
    if (w.chain_start >= w.L) return RH_ERR_INVALID;
    if (w.rule == 0 && w.chain_start % w.c) return RH_ERR_INVALID;
    const uint64_t n = (w.rule == 0 && w.chain_start + w.c > w.L) ? w.L - w.chain_start : w.c;  // the chain in progress
    if (w.chain_out >= span_out(n, F, T)) return RH_ERR_INVALID;
    if (w.L > kMaxLoopFrames) return RH_ERR_UNSUPPORTED;
    *M = span_out(w.c, F, T);
    if (*M * F > 0xffffffffull) return RH_ERR_UNSUPPORTED;  // M itself and j F of every output frame of a chain (M <= c T + 1 < 2^48: no overflow here)
    *P = 0;
    if (w.rule == 0) {
        *P = (w.L / w.c) * *M + span_out(w.L % w.c, F, T);  // (M < 2^32, L <= 2^31)
        if (*P > 0xffffffffull) return RH_ERR_UNSUPPORTED;
    }
    return RH_OK;
}

// The cursor behind a block of out_frames frames.  Any cut of a stream into blocks gives the positions of one pass.
inline rh_status loop_advance(uint64_t *words, uint32_t from_rate, uint32_t to_rate, uint64_t out_frames) {
    if (!words || from_rate == 0 || to_rate == 0) return RH_ERR_INVALID;
    Words w = words_of(words);
    if (w.L == 0) return RH_OK;  // not a loop: data and phase move, as for rh_wide_mix_block
    uint32_t F, T;
    mixplan::reduce(from_rate, to_rate, &F, &T);
    if ((uint64_t)F * T > 0xffffffffull) return RH_ERR_UNSUPPORTED;
    // (the channel count only bounds c: 1 admits every chain the entry can take)
    uint64_t M, P;
    const rh_status st = check_words(w, 1, F, T, &M, &P);
    if (st != RH_OK) return st;
    if (w.rule == 0) {
        const uint64_t off = ((w.chain_start / w.c) * M + w.chain_out + out_frames % P) % P;
        const uint64_t k = off / M;
        words[3] = k * w.c, words[4] = off - k * M;
    } else {
        const uint64_t q = w.chain_out + out_frames;  // (chain_out < 2^48)
        const uint64_t k = q / M;
        words[3] = (w.chain_start + (k % w.L) * w.c) % w.L, words[4] = q - k * M;
    }
    return RH_OK;
}

// One slot of the kernel's table: a source, loop or not, as the positions of locate().
struct Desc {
    const float *data;  // loops: frame 0 of the pass; plain sources: the frame of the block's first tap
    uint32_t ch;        // channels of the source
    uint32_t frames;    // output frames the source reaches (0: a slot that pads the table to whole groups)
    float gain;
    float Tf;           // T as a float; 0: the converter passes through (F == T)
    uint32_t F, T;      // reduced rates
    uint32_t r0;        // plain sources: the block's phase; loops: 0 (every chain starts a converter)
    uint32_t x0;        // output frames between the cursor's origin -- rule 0: the pass's first frame, rule 1: the chain's -- and the block
    uint32_t P;         // rule 0: output frames of a pass; otherwise 0
    uint32_t M;         // output frames of a whole chain (plain: 0)
    uint32_t c;         // input frames of a whole chain (plain: 0)
    uint32_t cs;        // rule 1: chain_start; otherwise 0
    uint32_t L;         // loop_frames; plain: 0xffffffff (no tap wraps)
    uint32_t nfull;     // rule 0: the index of the pass's tail chain, floor(L / c); otherwise 0xffffffff
    uint32_t nl;        // the last frame of a whole chain, c - 1: verbatim (plain: `last`)
    uint32_t nl_tail;   // ... of the tail chain
    Div dP, dM, dL, dT;
};
static_assert(sizeof(Desc) == 104, "32 of them and the other arguments share one 4 KiB kernel-argument segment");

struct Taps {
    uint32_t ia, ib;  // the frames of the two taps, counted from data (ib is read only where lerp is set)
    bool lerp;        // false: frame ia verbatim (a chain's last frame, F == T)
    uint32_t num;     // (position) mod T: the lerp's weight over T
};
// Output frame m of the block.  Every intermediate fits 32 bits for a call check() has passed.
RH_MIX_HD Taps locate(const Desc &d, uint32_t m) {
    const uint32_t x = d.x0 + m;
    const uint32_t p = x - div_u32(x, d.dP) * d.P;           // rule 0: inside the pass
    const uint32_t k = div_u32(p, d.dM), j = p - k * d.M;    // the chain and the frame inside it
    const uint32_t b = d.cs + k * d.c;
    const uint32_t base = b - div_u32(b, d.dL) * d.L;        // rule 1: the chain's first frame, mod L (dL answers 0 otherwise)
    const uint32_t pos = d.r0 + j * d.F;
    const uint32_t i = div_u32(pos, d.dT);
    Taps t;
    t.num = pos - i * d.T;
    t.lerp = d.Tf != 0.0f && i < (k == d.nfull ? d.nl_tail : d.nl);
    uint32_t ia = base + i;
    ia = ia >= d.L ? ia - d.L : ia;
    t.ia = ia;
    t.ib = ia + 1u == d.L ? 0u : ia + 1u;                    // the second tap of the pass's last frame is frame 0
    return t;
}

// The status of one source with frames > 0 (anything but RH_OK: nothing may be launched), and its descriptor.
inline rh_status describe(const rh_wide_src &x, const uint64_t *words, uint32_t channels, uint32_t to_rate, uint64_t out_frames, Desc *out) {
    const Words w = words_of(words);
    Desc d{};
    if (w.L == 0) {  // rh_wide_mix_block's source
        mixplan::Reach r;
        const rh_status st = mixplan::check_src(x, channels, to_rate, out_frames, &r);
        if (st != RH_OK) return st;
        d = Desc{x.data, x.channels, (uint32_t)x.frames, x.gain, r.F == r.T ? 0.0f : (float)r.T, r.F, r.T, x.phase, 0u, 0u, 0u, 0u, 0u, 0xffffffffu, 0xffffffffu, x.last, x.last,
                 kDivZero, kDivZero, kDivZero, make_div(r.T)};
        *out = d;
        return RH_OK;
    }
    rh_wide_src y = x;
    y.phase = 0;  // (a loop's positions come from its words: the field is not read)
    uint32_t F, T;
    uint64_t fit, M, P;
    rh_status st = mixplan::check_src(y, to_rate, out_frames, &F, &T, &fit);
    if (st != RH_OK) return st;
    st = check_words(w, x.channels, F, T, &M, &P);
    if (st != RH_OK) return st;
    const uint64_t x0 = w.rule == 0 ? (w.chain_start / w.c) * M + w.chain_out : w.chain_out;
    const uint64_t x_last = x0 + x.frames - 1;
    if (x_last > 0xffffffffull) return RH_ERR_UNSUPPORTED;
    if (w.rule == 1 && w.chain_start + (x_last / M) * w.c > 0xffffffffull) return RH_ERR_UNSUPPORTED;
    const uint64_t tail = w.L % w.c;
    d = Desc{x.data, x.channels, (uint32_t)x.frames, x.gain, F == T ? 0.0f : (float)T, F, T, 0u, (uint32_t)x0, (uint32_t)P, (uint32_t)M, (uint32_t)w.c,
             w.rule == 1 ? (uint32_t)w.chain_start : 0u, (uint32_t)w.L, w.rule == 0 ? (uint32_t)(w.L / w.c) : 0xffffffffu, (uint32_t)w.c - 1u, (uint32_t)(tail ? tail : w.c) - 1u,
             w.rule == 0 ? make_div(P) : kDivZero, make_div(M), w.rule == 1 ? make_div(w.L) : kDivZero, make_div(T)};
    *out = d;
    return RH_OK;
}
// A slot that reaches no frame and points at something readable.
inline Desc pad_slot(const float *readable) {
    return Desc{readable, 1u, 0u, 0.0f, 0.0f, 1u, 1u, 0u, 0u, 0u, 0u, 0u, 0u, 0xffffffffu, 0xffffffffu, 0u, 0u, kDivZero, kDivZero, kDivZero, make_div(1)};
}

// The status of a call.  out_frames == 0 is answered by the caller: nothing is looked at.
inline rh_status check(const float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs, uint32_t n_sources, const uint64_t *loops) {
    if (!dst || channels == 0 || to_rate == 0 || (n_sources && (!srcs || !loops))) return RH_ERR_INVALID;
    if (out_frames > 0x7fffffffull) return RH_ERR_UNSUPPORTED;
    for (uint32_t s = 0; s < n_sources; ++s) {
        if (srcs[s].frames == 0) continue;  // not looked at
        Desc d;
        const rh_status st = describe(srcs[s], loops + (size_t)RH_LOOP_WORDS * s, channels, to_rate, out_frames, &d);
        if (st != RH_OK) return st;
    }
    return RH_OK;
}

}  // namespace loopmix
}  // namespace rh
