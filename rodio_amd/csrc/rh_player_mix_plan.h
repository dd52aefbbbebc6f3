// rh_player_mix_plan.h -- what rh_player_mix_block (rh_playermix.hip) decides on the host, as plain functions over the caller's arrays: the
// status of the call, what a block's taps reach of a source and of its factor table, when a ramp is a constant, the sources and the
// (F, T, r0) slots of every launch, and the kernel a launch takes.  No HIP: tests/cpp/player_mix_plan_test.cpp runs it without a GPU.
// Building the kernel tables and launching are rh_player_mix_block's.  Nothing here allocates.
#pragma once
#include <cstdint>

#include "../../include/rodio_hip.h"
#include "rh_mix_plan.h"

namespace rh {
namespace playermix {

using mixplan::check_src;  // the fields the entry shares with rh_wide_mix_block, and the reach of the block's taps: a block is not cut into launches
using mixplan::kChunk;     // sources a launch
using mixplan::kGroup;     // ... walked in groups of this many by the general kernel: a launch's slots are whole groups
using mixplan::kRates;     // ... of at most this many different (F, T, r0)
using mixplan::Rate;
using mixplan::Reach;
// The step rule's index -- sample k = f * src_channels + c, counted from `data` -- stays below this for every tap of a block (rh_live.hip's
// bound: with the phase of the first sample inside its period it then fits 32 bits).
constexpr uint64_t kMaxStepSamples = 1ull << 30;

enum Kernel { kGeneral = 0, kStereo = 1 };  // k_player_mix / k_player_mix_stereo

// Entries of a table that covers samples [0, n) of a stream whose first sample lies `at` behind a multiple of the period (rh_amplify_steps' rule).
inline uint64_t steps_needed(uint64_t at, uint64_t period, uint64_t n) { return n ? (at + n - 1) / period + 1 : 0; }
inline uint64_t entries_needed(uint64_t first, uint64_t period, uint64_t n) { return steps_needed(first % period, period, n); }

// A ramp of `kind` (0 none, 1 LinearGainRamp, 2 ... with clamp_end) at the block's first frame, given what rhrows::make_ramp made of it
// (step_ns = 1e9 / rate, done_frame = ceil(duration / step_ns)): 0 no multiply, 1 ONE constant factor for the whole block -- the ramp has run
// out before the block's first frame, where rhrows::ramp_factor returns `after` for every frame --, 2 the factor of every tap's frame.
enum RampMode { kRampNone = 0, kRampConstant = 1, kRampLive = 2 };
inline RampMode ramp_mode(uint64_t kind, uint64_t step_ns, uint64_t done_frame, uint64_t first_frame) {
    if (kind == 0) return kRampNone;
    return step_ns != 0 && first_frame >= done_frame ? kRampConstant : kRampLive;
}

// The status of a call (anything but RH_OK: nothing may be launched).  out_frames == 0 is answered by the caller: nothing is looked at.
inline rh_status check(const float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs, uint32_t n_sources, const uint64_t *ramps,
                       const float *ramp_gains, const float *const *factors_dev, const uint64_t *factor_steps) {
    if (!dst || channels == 0 || to_rate == 0 || (n_sources && !srcs)) return RH_ERR_INVALID;
    if (out_frames > 0x7fffffffull) return RH_ERR_UNSUPPORTED;
    for (uint32_t s = 0; s < n_sources; ++s) {
        const rh_wide_src &x = srcs[s];
        if (x.frames == 0) continue;  // not looked at
        Reach r;
        const rh_status st = check_src(x, channels, to_rate, out_frames, &r);
        if (st != RH_OK) return st;
        if (ramps) {
            const uint64_t kind = ramps[4 * (size_t)s], rate = ramps[4 * (size_t)s + 3];
            if (kind > 2) return RH_ERR_INVALID;
            if (kind != 0 && (rate == 0 || rate > 0xffffffffull || !ramp_gains)) return RH_ERR_INVALID;
        }
        if (factors_dev && factors_dev[s]) {
            if (!factor_steps) return RH_ERR_INVALID;
            const uint64_t first = factor_steps[3 * (size_t)s], period = factor_steps[3 * (size_t)s + 1], entries = factor_steps[3 * (size_t)s + 2];
            if (period == 0) return RH_ERR_INVALID;
            if (r.samples > kMaxStepSamples) return RH_ERR_UNSUPPORTED;
            if (entries_needed(first, period, r.samples) > entries) return RH_ERR_INVALID;
        }
    }
    return RH_OK;
}

// One launch: up to kChunk sources in insertion order, each with its slot of r (mixplan::RateLaunch), and its kernel.
struct Launch : mixplan::RateLaunch {
    Kernel kernel;
};

// The specialised kernel's case: a stereo mix on an 8-byte boundary, and every source of the launch stereo, on an 8-byte boundary itself (its
// taps are 8-byte loads), of ONE (F, T, r0), reaching every frame of the block with both taps (none ends inside it).
inline Kernel kernel_of(const Launch &L, uint32_t channels, uint64_t out_frames, const rh_wide_src *srcs, bool dst_on_8) {
    if (L.n == 0 || L.nr != 1 || channels != 2 || !dst_on_8) return kGeneral;
    const Rate &r = L.r[0];
    const uint64_t il_max = ((uint64_t)r.r0 + (out_frames - 1) * r.F) / r.T;
    for (uint32_t q = 0; q < L.n; ++q) {
        const rh_wide_src &x = srcs[L.src[q]];
        if (x.channels != 2 || (reinterpret_cast<uintptr_t>(x.data) & 7u) != 0 || x.frames != out_frames || (r.F != r.T && il_max >= x.last)) return kGeneral;
    }
    return kStereo;
}

// The launches of a call that check() has passed, in order: emit(const Launch &) for each (mixplan::walk_rates: full at kChunk sources, early
// at a fifth (F, T, r0)).
template <class Emit>
inline void walk(uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs, uint32_t n_sources, bool dst_on_8, Emit &&emit) {
    mixplan::walk_rates<Launch>(
        n_sources, true,
        [&](uint32_t s, uint32_t *F, uint32_t *T, uint32_t *r0, uint64_t *) {
            if (srcs[s].frames == 0) return false;
            mixplan::reduce(srcs[s].from_rate, to_rate, F, T);
            *r0 = srcs[s].phase;
            return true;
        },
        [&](Launch &L) {
            L.kernel = kernel_of(L, channels, out_frames, srcs, dst_on_8);
            emit(static_cast<const Launch &>(L));
        });
}

}  // namespace playermix
}  // namespace rh
