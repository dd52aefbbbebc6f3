// rh_mix_plan.h -- the host rules every block mixer shares (rh_widemix, rh_widebatch, rh_spatialmix, rh_playermix, rh_loopmix, rh_queuemix,
// rh_clipmix .hip and their *_plan.h), once: what the shared fields of an rh_wide_src must satisfy (check_src) and what a block's taps
// reach of it (Reach), the exact round-up reciprocals (Div for a quotient, StepDiv for the index of a step table), the output frames of a
// converter chain (span_out), the (F, T, r0) slots and the sources of every launch (walk_rates, walk) and the cut in front of the first of
// a table of alike sources that ends (alike_cut).  No HIP: tests/cpp/mix_plan_test.cpp and the plan programs run it without a GPU.
// Nothing here allocates.
#pragma once
#include <cstdint>
#include <numeric>

#include "../../include/rodio_hip.h"

#if defined(__HIPCC__)
#define RH_MIX_HD __host__ __device__ __forceinline__
#else
#define RH_MIX_HD inline
#endif

namespace rh {
namespace mixplan {

constexpr uint32_t kChunk = 32;            // sources a launch (the table travels by value in the kernel-argument segment)
constexpr uint32_t kGroup = 4;             // ... walked in groups of this many, whose tap loads leave together: a launch's slots are whole groups
constexpr uint32_t kRates = 4;             // ... of at most this many different (F, T, r0): the position of an output frame between its taps is worked out once per slot
constexpr uint64_t kChainSamples = 32768;  // uniform.rs:56: what a converter chain takes at most

// ---- the source rule ------------------------------------------------------------------------------------------------------------------------
// from_rate / to_rate reduced (both not 0).  The one gcd of the family.
inline void reduce(uint32_t from_rate, uint32_t to_rate, uint32_t *F, uint32_t *T) {
    const uint32_t g = std::gcd(from_rate, to_rate);
    *F = from_rate / g, *T = to_rate / g;
}
// What the fields every block entry shares must satisfy in a source with frames > 0 (one with none is not looked at), for to_rate != 0.
// fit: the output frames a launch may cover before the source's position r0 + j F leaves 32 bits.  It is 0 for 2^32 - 1 Hz into 1 Hz and
// for nothing else; the caller refuses that (RH_ERR_UNSUPPORTED) where it judges fit: an entry that cuts a block into launches behind
// its table, one that does not at once.
inline rh_status check_src(const rh_wide_src &x, uint32_t to_rate, uint64_t out_frames, uint32_t *F, uint32_t *T, uint64_t *fit) {
    if (!x.data || x.channels == 0 || x.from_rate == 0 || x.frames > out_frames) return RH_ERR_INVALID;
    reduce(x.from_rate, to_rate, F, T);
    if ((uint64_t)*F * *T > 0xffffffffull) return RH_ERR_UNSUPPORTED;  // the reference multiplies in u32 (sample_rate.rs:157,173)
    if (x.phase >= *T) return RH_ERR_INVALID;
    *fit = (0xffffffffull - *T) / *F;
    return RH_OK;
}

// What the taps of a block reach of one source.
struct Reach {
    uint32_t F, T;     // from_rate / to_rate reduced
    uint64_t frames;   // source frames, counted from data: 0 .. frames - 1
    uint64_t samples;  // samples of the source's stream, counted from data, up to the last one a tap reads: what a factor table must cover
};
// check_src for an entry that does not cut a block into launches -- one whose positions phase + j F leave 32 bits is refused --, and the
// reach of the block's taps into a mix of `channels`.
inline rh_status check_src(const rh_wide_src &x, uint32_t channels, uint32_t to_rate, uint64_t out_frames, Reach *r) {
    uint64_t fit;
    const rh_status st = check_src(x, to_rate, out_frames, &r->F, &r->T, &fit);
    if (st != RH_OK) return st;
    if (out_frames > fit) return RH_ERR_UNSUPPORTED;
    // the first tap of the last frame the source reaches, and the second one where that frame has it
    const uint64_t il = ((uint64_t)x.phase + (x.frames - 1) * r->F) / r->T;
    const uint64_t lastf = il + (r->F != r->T && il < x.last ? 1 : 0);
    r->frames = lastf + 1;
    // channels.rs:59-70: output channel c reads input channel c (c < from), channel 1 of a mono source its only one: the highest input channel read
    // is min(from, to) - 1
    r->samples = lastf * x.channels + (x.channels < channels ? x.channels : channels);
    return RH_OK;
}

// ---- exact reciprocals ------------------------------------------------------------------------------------------------------------------------
// x / d for every x < 2^32 and 1 <= d < 2^32 without a division (the round-up method: m = floor(2^32 (2^l - d) / d) + 1 with
// l = ceil(log2 d); q = (t + ((x - t) >> min(l, 1))) >> max(l - 1, 0) with t = the high word of x m).  sh = s1 | s2 << 8.
struct Div {
    uint32_t m, sh;
};
RH_MIX_HD uint32_t div_u32(uint32_t x, Div d) {
    const uint32_t t = (uint32_t)(((uint64_t)x * d.m) >> 32);
    return (t + ((x - t) >> (d.sh & 0xffu))) >> (d.sh >> 8);
}
inline Div make_div(uint64_t d) {
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    const uint64_t m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
    return Div{(uint32_t)m, (l < 1 ? l : 1u) | ((l > 1 ? l - 1 : 0u) << 8)};
}
constexpr Div kDivZero = Div{0u, 31u | (31u << 8)};  // the quotient 0 for every x: a position a source does not have

// The step rule's index (rh_live.hip): sample i of a launch takes entry (phase + i) / d of its table, the same reciprocal with the two
// shifts apart.  Exact for every phase + i < 2^32 and 1 <= d <= 2^31 (tests/test_gpu_live.py checks the boundaries).
struct StepDiv {
    uint32_t phase;  // (first % period), reduced as below
    uint32_t m, s1, s2;
    RH_MIX_HD uint32_t step(uint32_t i) const {
        const uint32_t x = phase + i;
        const uint32_t t = (uint32_t)(((uint64_t)x * m) >> 32);
        return (t + ((x - t) >> s1)) >> s2;
    }
};
constexpr StepDiv kStepNone = StepDiv{0u, 1u, 0u, 0u};  // a slot without a table: step(i) is i (period 1), and never asked -- the kernels read no entry where the table pointer is null
// The table index of sample i (< n <= 2^30) of a launch whose first sample lies `at` samples behind a multiple of `period` (>= 1).
inline StepDiv step_div(uint64_t at, uint64_t period, uint64_t n) {
    uint64_t d = period, phase = at % period;
    if (d > (1ull << 31)) {
        // at most one boundary inside the launch, at i = period - phase: the same quotient with d = 2^31 and the phase moved so that the
        // boundary stays where it is (i < 2^30 keeps phase + i below 2^32)
        const uint64_t t = d - phase;
        d = 1ull << 31;
        phase = t >= n ? 0 : d - t;
    }
    const Div r = make_div(d);
    return StepDiv{(uint32_t)phase, r.m, r.sh & 0xffu, r.sh >> 8};
}

// Output frames of a complete chain of n input frames: rh_uniform_span_frames(n, F, T, 1, ..) for reduced F / T (n <= 2^31, T < 2^32).
inline uint64_t span_out(uint64_t n, uint64_t F, uint64_t T) {
    if (F == T || n == 0) return n;
    uint64_t c = ((n - 1) * T + F - 1) / F;  // the frames with floor(j F / T) <= n - 2
    if (c * F < n * T) c += 1;               // ... and the one that lands on the last frame, where one does
    return c;
}

// ---- the launches of a call ---------------------------------------------------------------------------------------------------------------
// Sources that bring their own positions (rh_loop_mix_block, rh_clip_mix_block): up to kChunk of them in insertion order.
struct Launch {
    uint32_t n;            // sources (0: no source reaches the block, the launch writes zeros)
    uint32_t src[kChunk];  // their indices in the caller's table
    bool cont;             // it continues from the partial sum an earlier launch of the call stored
};
// The launches of a call, in order: emit(const Launch &) for each.  A launch is full at kChunk sources and for no other reason.
template <class Emit>
inline void walk(const rh_wide_src *srcs, uint32_t n_sources, Emit &&emit) {
    Launch L;
    L.n = 0, L.cont = false;
    for (uint32_t s = 0; s < n_sources; ++s) {
        if (srcs[s].frames == 0) continue;
        L.src[L.n] = s;
        if (++L.n == kChunk) {
            emit(static_cast<const Launch &>(L));
            L.n = 0, L.cont = true;
        }
    }
    if (L.n || !L.cont) emit(static_cast<const Launch &>(L));
}

// Sources whose positions are one of a launch's kRates slots: the kernel divides once per slot and output frame, not once per source.
struct Rate {
    uint32_t F, T;  // reduced rates (an unused slot: F = 0, T = 1)
    uint32_t r0;    // the phase of the launch's first output frame
    float Tf;
};
struct RateLaunch {
    Rate r[kRates];
    uint32_t nr;            // slots of r in use
    uint32_t n;             // sources (0: no source reaches the frames, the launch writes zeros)
    uint32_t src[kChunk];   // their indices in the caller's table
    uint32_t rate[kChunk];  // their slots
    uint64_t i0[kChunk];    // ... and the source frame of the first tap of the launch's first output frame, as `key` gave it
    bool cont;              // it continues from the partial sum an earlier launch of the call stored
};
// Where output frame j0 of a block lies between the taps of a source of (phase, F, T): the frame of its first tap and its phase.
inline void tap_of(uint32_t phase, uint64_t j0, uint32_t F, uint32_t T, uint64_t *i0, uint32_t *r0) {
    const uint64_t p = (uint64_t)phase + j0 * F;
    *i0 = p / T;
    *r0 = (uint32_t)(p - *i0 * T);
}
// The launches of n_sources sources, in order: emit(L) for each, L a RateLaunch or a structure derived from it.  key(s, &F, &T, &r0, &i0)
// says whether source s takes part, its slot's key and its first tap (tap_of: worked out once, here).  A launch is full at kChunk sources, and goes early when a source brings a fifth
// (F, T, r0): what has been gathered goes first, and the sum continues from the stored partial sum.  always: a call that no source takes
// part in still emits one launch (the mix is +0.0 there).
template <class L, class Key, class Emit>
inline void walk_rates(uint32_t n_sources, bool always, Key &&key, Emit &&emit) {
    L l;
    bool cont = false;
    auto clear = [&]() {
        for (uint32_t q = 0; q < kRates; ++q) l.r[q] = Rate{0u, 1u, 0u, 1.0f};
        l.nr = 0, l.n = 0;
    };
    auto flush = [&]() {
        l.cont = cont;
        emit(l);
        cont = true;
        clear();
    };
    clear();
    for (uint32_t s = 0; s < n_sources; ++s) {
        uint32_t F, T, r0;
        uint64_t i0 = 0;
        if (!key(s, &F, &T, &r0, &i0)) continue;
        uint32_t q = 0;
        while (q < l.nr && !(l.r[q].F == F && l.r[q].T == T && l.r[q].r0 == r0)) ++q;
        if (q == l.nr && l.nr == kRates) {
            flush();
            q = 0;
        }
        if (q == l.nr) l.r[l.nr++] = Rate{F, T, r0, (float)T};
        l.src[l.n] = s, l.rate[l.n] = q, l.i0[l.n] = i0;
        if (++l.n == kChunk) flush();
    }
    if (l.n || (always && !cont)) flush();
}

// The last first tap of a launch of nf frames in slot r: a launch whose sources all reach it with both taps has no source that ends inside.
inline uint64_t last_tap(const Rate &r, uint64_t nf) { return ((uint64_t)r.r0 + (nf - 1) * r.F) / r.T; }

// Alike sources -- `channels` channels, one rate and phase -- in a table that check_src has passed: the frames in front of the first one
// that ends, or whose last frame a tap reaches, can go to a kernel for alike sources as a launch of their own.  The cut, or 0 where
// there is none: the sources are not alike, none ends inside the block, or fewer than kAlikeMin frames lie in front.
constexpr uint64_t kAlikeMin = 1024;
inline uint64_t alike_cut(const rh_wide_src *srcs, uint32_t n_sources, uint32_t channels, uint32_t to_rate, uint64_t out_frames) {
    const rh_wide_src *first = nullptr;
    uint64_t upto = out_frames;
    for (uint32_t s = 0; s < n_sources; ++s) {
        const rh_wide_src &x = srcs[s];
        if (x.frames == 0) continue;
        if (!first) first = &x;
        if (x.channels != channels || x.from_rate != first->from_rate || x.phase != first->phase) return 0;
        uint32_t F, T;
        reduce(x.from_rate, to_rate, &F, &T);
        uint64_t u = x.frames;
        if (x.last != 0xffffffffu && F != T) {  // il(j) >= last  <=>  phase + j F >= last T
            const uint64_t need = (uint64_t)x.last * T;
            const uint64_t jl = need > x.phase ? (need - x.phase + F - 1) / F : 0;
            if (jl < u) u = jl;
        }
        if (u < upto) upto = u;
    }
    return first && upto >= kAlikeMin && upto < out_frames ? upto : 0;
}

}  // namespace mixplan
}  // namespace rh
