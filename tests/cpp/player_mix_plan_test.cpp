// player_mix_plan_test.cpp -- the host decisions of rh_player_mix_block (rodio_amd/csrc/rh_player_mix_plan.h) without a GPU: every refusal
// of the header is answered, what a block's taps reach of a source and of its factor table is counted a second way (by walking the output
// frames), a ramp is a constant exactly from done_frame on, the launches hold every source that reaches the block once, in insertion
// order, at most 32 a launch and at most four (F, T, r0) a launch, and a launch takes the specialised kernel exactly in its case.
// TEST INFRASTRUCTURE: plain g++, no HIP, no library.  Pointers are never followed.
//
//     player_mix_plan_test [seed [random calls]]
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "rh_player_mix_plan.h"

using namespace rh::playermix;

static int g_failures = 0;
#define EXPECT(cond, ...)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++g_failures <= 20) {                      \
                std::fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
                std::fprintf(stderr, __VA_ARGS__);         \
                std::fprintf(stderr, "\n");                \
            }                                              \
        }                                                  \
    } while (0)

static float *out_ptr(uint64_t off = 0) { return reinterpret_cast<float *>((uintptr_t)(0x100000000ull + off)); }
static const float *in_ptr(uint64_t k, uint64_t off = 0) { return reinterpret_cast<const float *>((uintptr_t)(0x800000000000ull + 0x100000ull * k + off)); }
static const float *table_ptr(uint64_t k) { return reinterpret_cast<const float *>((uintptr_t)(0x400000000000ull + 0x1000ull * k)); }
static rh_wide_src src(uint64_t k, uint32_t ch, uint32_t rate, uint32_t phase, uint64_t frames, uint32_t last = 0xffffffffu, float gain = 1.0f) {
    return rh_wide_src{in_ptr(k), ch, rate, phase, frames, last, gain};
}

// A call's arrays.
struct Call {
    uint32_t channels = 2, to_rate = 48000;
    uint64_t out_frames = 1000;
    float *dst = out_ptr();
    std::vector<rh_wide_src> srcs;
    std::vector<uint64_t> ramps, fsteps;
    std::vector<float> gains;
    std::vector<const float *> factors;
    void add(const rh_wide_src &x, uint64_t kind = 0, uint64_t ns = 0, uint64_t first_frame = 0, uint64_t rate = 44100, const float *f = nullptr, uint64_t first = 0, uint64_t period = 1,
             uint64_t entries = 0) {
        srcs.push_back(x);
        ramps.insert(ramps.end(), {kind, ns, first_frame, rate});
        gains.insert(gains.end(), {0.0f, 1.0f});
        factors.push_back(f);
        fsteps.insert(fsteps.end(), {first, period, entries});
    }
    rh_status check(bool with_ramps = true, bool with_gains = true, bool with_factors = true, bool with_fsteps = true) const {
        return rh::playermix::check(dst, channels, to_rate, out_frames, srcs.empty() ? nullptr : srcs.data(), (uint32_t)srcs.size(), with_ramps ? ramps.data() : nullptr,
                                    with_gains ? gains.data() : nullptr, with_factors ? factors.data() : nullptr, with_fsteps ? fsteps.data() : nullptr);
    }
    std::vector<Launch> launches() const {
        std::vector<Launch> out;
        walk(channels, to_rate, out_frames, srcs.data(), (uint32_t)srcs.size(), (reinterpret_cast<uintptr_t>(dst) & 7u) == 0, [&](const Launch &L) { out.push_back(L); });
        return out;
    }
};

// ---- every refusal of rodio_hip.h, and the calls next to them that pass -------------------------------------------------------------------
static int test_refusals() {
    int n = 0;
    auto base = [] {
        Call c;
        c.add(src(0, 2, 44100, 0, 1000), 1, 5000000, 0, 44100, table_ptr(0), 0, 441, 5);  // 1000 frames at 147 / 160: the taps reach frames 0 .. 918, 1838 samples, 5 entries of 441
        c.add(src(1, 1, 44100, 0, 1000));
        return c;
    };
    auto refused = [&](rh_status want, const char *what, auto &&edit, bool ramps = true, bool gains = true, bool factors = true, bool fsteps = true) {
        Call c = base();
        edit(c);
        const rh_status got = c.check(ramps, gains, factors, fsteps);
        EXPECT(got == want, "%s: status %d, expected %d", what, (int)got, (int)want);
        ++n;
    };
    auto nothing = [](Call &) {};
    EXPECT(base().check() == RH_OK, "the base call");
    EXPECT(base().check(false, false, false, false) == RH_OK, "no adapters at all");
    refused(RH_ERR_INVALID, "dst NULL", [](Call &c) { c.dst = nullptr; });
    refused(RH_ERR_INVALID, "channels 0", [](Call &c) { c.channels = 0; });
    refused(RH_ERR_INVALID, "to_rate 0", [](Call &c) { c.to_rate = 0; });
    refused(RH_ERR_UNSUPPORTED, "out_frames beyond 31 bits", [](Call &c) { c.out_frames = 0x80000000ull; });
    // what rh_wide_mix_block refuses of the shared fields
    refused(RH_ERR_INVALID, "data NULL", [](Call &c) { c.srcs[1].data = nullptr; });
    refused(RH_ERR_INVALID, "source channels 0", [](Call &c) { c.srcs[1].channels = 0; });
    refused(RH_ERR_INVALID, "from_rate 0", [](Call &c) { c.srcs[1].from_rate = 0; });
    refused(RH_ERR_INVALID, "frames > out_frames", [](Call &c) { c.srcs[1].frames = 1001; });
    refused(RH_ERR_INVALID, "phase >= T", [](Call &c) { c.srcs[1].phase = 160; });
    refused(RH_ERR_UNSUPPORTED, "F T beyond 32 bits", [](Call &c) { c.srcs[1].from_rate = 4294967291u; });
    refused(RH_ERR_UNSUPPORTED, "phase + j F leaves 32 bits", [](Call &c) {
        c.out_frames = 0x7fffffffull;  // (2^32 - 1 - 160) / 147 = 29 217 463 frames fit
        c.srcs = {src(0, 1, 44100, 0, 10)};
        c.ramps.resize(4), c.gains.resize(2), c.factors.resize(1), c.fsteps.resize(3);
        c.ramps[0] = 0, c.factors[0] = nullptr;
    });
    // the ramp
    refused(RH_ERR_INVALID, "kind 3", [](Call &c) { c.ramps[0] = 3; });
    refused(RH_ERR_INVALID, "ramp rate 0", [](Call &c) { c.ramps[3] = 0; });
    refused(RH_ERR_INVALID, "ramp rate beyond 32 bits", [](Call &c) { c.ramps[3] = 1ull << 32; });
    refused(RH_ERR_INVALID, "a ramp without gains", nothing, true, false);
    refused(RH_OK, "kind 0 everywhere needs no gains", [](Call &c) { c.ramps[0] = 0; }, true, false);
    refused(RH_OK, "kind 0 reads neither rate nor duration", [](Call &c) { c.ramps[4 + 3] = 0; });
    refused(RH_OK, "a duration of 0 is a ramp that has run out", [](Call &c) { c.ramps[1] = 0; });
    // the factors
    refused(RH_ERR_INVALID, "factors without steps", nothing, true, true, true, false);
    refused(RH_OK, "no factors array: the steps are not read", nothing, true, true, false, false);
    refused(RH_ERR_INVALID, "period 0", [](Call &c) { c.fsteps[1] = 0; });
    refused(RH_ERR_INVALID, "a table one entry short", [](Call &c) { c.fsteps[2] = 4; });
    refused(RH_ERR_INVALID, "a table of no entries", [](Call &c) { c.fsteps[2] = 0; });
    refused(RH_ERR_UNSUPPORTED, "the step rule's index leaves 2^30", [](Call &c) {
        c.to_rate = 44100, c.out_frames = 0x7fffffffull;
        c.srcs[0] = src(0, 2, 44100, 0, (1u << 29) + 1);  // 2^29 + 1 stereo frames: 2^30 + 2 samples
        c.fsteps[1] = 1ull << 40, c.fsteps[2] = 1;
        c.srcs[1].from_rate = 44100;
    });
    refused(RH_OK, "... and 2^30 samples stay", [](Call &c) {
        c.to_rate = 44100, c.out_frames = 0x7fffffffull;
        c.srcs[0] = src(0, 2, 44100, 0, 1u << 29);
        c.fsteps[1] = 1ull << 40, c.fsteps[2] = 1;
        c.srcs[1].from_rate = 44100;
    });
    // a source with frames == 0 is not looked at
    refused(RH_OK, "frames == 0: nothing of the source is read", [](Call &c) {
        c.srcs[0] = rh_wide_src{nullptr, 0, 0, 99999, 0, 0, 0.0f};
        c.ramps[0] = 9, c.ramps[3] = 0, c.fsteps[1] = 0;
    });
    refused(RH_OK, "no sources", [](Call &c) { c.srcs.clear(); });
    return n;
}

// ---- reach and table sizes against a walk of the output frames ------------------------------------------------------------------------------
static long test_reach(uint32_t seed, int rounds) {
    std::mt19937_64 rng(seed * 7919u + 1);
    const uint32_t rates[] = {44100, 48000, 8000, 96000, 22050, 66150, 32000};
    long n = 0;
    for (int it = 0; it < rounds; ++it) {
        const uint32_t from = rates[rng() % 7], to = rates[rng() % 7], ch = 1 + rng() % 6, to_ch = 1 + rng() % 6;
        const uint32_t g = std::gcd(from, to), F = from / g, T = to / g;
        const uint64_t frames = 1 + rng() % 700, phase = rng() % T;
        const bool ended = rng() % 3 == 0;
        uint64_t last = 0xffffffffu;
        if (ended) last = ((phase + (frames - 1) * F) / T) + (rng() % 2);  // the last frame is the last frame's first tap (verbatim) or the one behind it
        rh_wide_src x = src(0, ch, from, (uint32_t)phase, frames, (uint32_t)last);
        Reach r;
        EXPECT(check_src(x, to_ch, to, frames + rng() % 5, &r) == RH_OK, "a plain source");
        uint64_t top_frame = 0, top_sample = 0;
        for (uint64_t j = 0; j < frames; ++j) {
            const uint64_t i = (phase + j * F) / T;
            const uint64_t hi = i + ((F != T && i < last) ? 1 : 0);
            for (uint32_t c = 0; c < to_ch; ++c) {
                if (!(c < ch || (c == 1 && ch == 1))) continue;
                const uint64_t k = hi * ch + (c < ch ? c : 0);
                if (k > top_sample) top_sample = k;
            }
            if (hi > top_frame) top_frame = hi;
        }
        EXPECT(r.F == F && r.T == T && r.frames == top_frame + 1 && r.samples == top_sample + 1, "reach: %llu frames %llu samples, walked %llu / %llu (ch %u -> %u, %u -> %u)",
               (unsigned long long)r.frames, (unsigned long long)r.samples, (unsigned long long)top_frame + 1, (unsigned long long)top_sample + 1, ch, to_ch, from, to);
        // the table: the entry of the last sample reached, by the rule itself
        const uint64_t period = 1 + rng() % 900, first = (rng() % 3 == 0 ? (1ull << 40) : 0) + rng() % 5000;
        const uint64_t need = (first + top_sample) / period - first / period + 1;
        EXPECT(entries_needed(first, period, r.samples) == need, "entries_needed(%llu, %llu, %llu)", (unsigned long long)first, (unsigned long long)period, (unsigned long long)r.samples);
        Call c;
        c.channels = to_ch, c.to_rate = to, c.out_frames = frames;
        c.add(x, 0, 0, 0, from, table_ptr(0), first, period, need);
        EXPECT(c.check() == RH_OK, "a table of exactly the entries reached");
        c.fsteps[2] = need - 1;
        EXPECT(c.check() == RH_ERR_INVALID, "a table one entry short");
        ++n;
    }
    EXPECT(steps_needed(0, 7, 0) == 0 && steps_needed(6, 7, 1) == 1 && steps_needed(6, 7, 2) == 2, "steps_needed at a boundary");
    return n;
}

// ---- the ramp that is a constant --------------------------------------------------------------------------------------------------------------
static int test_ramp_modes() {
    int n = 0;
    // rhrows::make_ramp's words for 44.1 kHz and 5 ms: step_ns = 22675, done_frame = ceil(5e6 / 22675) = 221
    const uint64_t step_ns = 1000000000ull / 44100, done = (5000000 + step_ns - 1) / step_ns;
    EXPECT(step_ns == 22675 && done == 221, "the words");
    auto is = [&](RampMode got, RampMode want, const char *what) {
        EXPECT(got == want, "%s: mode %d, expected %d", what, (int)got, (int)want);
        ++n;
    };
    for (uint64_t kind = 1; kind <= 2; ++kind) {
        is(ramp_mode(kind, step_ns, done, 0), kRampLive, "the block starts with the ramp");
        is(ramp_mode(kind, step_ns, done, done - 1), kRampLive, "one frame of the ramp is left");
        is(ramp_mode(kind, step_ns, done, done), kRampConstant, "the first frame behind the ramp");
        is(ramp_mode(kind, step_ns, done, 1ull << 40), kRampConstant, "long after");
        is(ramp_mode(kind, step_ns, 0, 0), kRampConstant, "a duration of 0");
        is(ramp_mode(kind, 0, 0, 1ull << 40), kRampLive, "a rate above 1 GHz: the ramp never advances");
    }
    is(ramp_mode(0, step_ns, done, 0), kRampNone, "kind 0");
    is(ramp_mode(0, 0, 0, 0), kRampNone, "kind 0 of no rate");
    return n;
}

// ---- the launches -----------------------------------------------------------------------------------------------------------------------------
static void check_launches(const Call &c, const std::vector<Launch> &Ls) {
    std::vector<uint32_t> live;
    for (uint32_t s = 0; s < c.srcs.size(); ++s)
        if (c.srcs[s].frames) live.push_back(s);
    EXPECT(!Ls.empty(), "a call has at least one launch (zeros where no source reaches the block)");
    size_t at = 0;
    for (size_t l = 0; l < Ls.size(); ++l) {
        const Launch &L = Ls[l];
        EXPECT(L.cont == (l > 0), "launch %zu: cont", l);
        EXPECT(L.n <= kChunk && L.nr <= kRates && (L.n > 0 || Ls.size() == 1), "launch %zu: %u sources, %u slots", l, L.n, L.nr);
        std::vector<bool> used(kRates, false);
        for (uint32_t q = 0; q < L.n; ++q) {
            EXPECT(at < live.size() && L.src[q] == live[at], "launch %zu slot %u: the sources that reach the block, once, in insertion order", l, q);
            ++at;
            const rh_wide_src &x = c.srcs[L.src[q]];
            const uint32_t g = std::gcd(x.from_rate, c.to_rate);
            EXPECT(L.rate[q] < L.nr, "launch %zu slot %u: rate slot %u of %u", l, q, L.rate[q], L.nr);
            if (L.rate[q] >= L.nr) continue;
            const Rate &r = L.r[L.rate[q]];
            used[L.rate[q]] = true;
            EXPECT(r.F == x.from_rate / g && r.T == c.to_rate / g && r.r0 == x.phase && r.Tf == (float)r.T, "launch %zu slot %u: its (F, T, r0)", l, q);
        }
        for (uint32_t q = 0; q < kRates; ++q) {
            EXPECT(q >= L.nr || used[q], "launch %zu: slot %u of r is nobody's", l, q);
            EXPECT(q < L.nr || (L.r[q].F == 0 && L.r[q].T == 1), "launch %zu: an unused slot of r divides by its T", l);
            for (uint32_t p = 0; p < q && q < L.nr; ++p) EXPECT(!(L.r[p].F == L.r[q].F && L.r[p].T == L.r[q].T && L.r[p].r0 == L.r[q].r0), "launch %zu: slots %u and %u are one", l, p, q);
        }
        // a launch that is neither full nor the last one went early for a fifth (F, T, r0)
        if (L.n < kChunk && l + 1 < Ls.size()) EXPECT(L.nr == kRates, "launch %zu went early with %u slots", l, L.nr);
        // the kernel, from the definition
        bool fast = L.n > 0 && L.nr == 1 && c.channels == 2 && (reinterpret_cast<uintptr_t>(c.dst) & 7u) == 0;
        for (uint32_t q = 0; q < L.n && fast; ++q) {
            const rh_wide_src &x = c.srcs[L.src[q]];
            const Rate &r = L.r[0];
            fast = x.channels == 2 && (reinterpret_cast<uintptr_t>(x.data) & 7u) == 0 && x.frames == c.out_frames;
            if (r.F != r.T)
                for (uint64_t j = 0; j < c.out_frames && fast; ++j) fast = (r.r0 + j * r.F) / r.T < x.last;  // both taps of every frame
        }
        EXPECT((L.kernel == kStereo) == fast, "launch %zu: kernel %d, the definition says %d", l, (int)L.kernel, (int)fast);
    }
    EXPECT(at == live.size(), "%zu of %zu sources launched", at, live.size());
}

static long g_stereo = 0;
static long test_random(uint32_t seed, int calls) {
    std::mt19937_64 rng(seed);
    const uint32_t rates[] = {44100, 48000, 8000, 96000, 22050, 66150};
    long n = 0;
    for (int it = 0; it < calls; ++it) {
        Call c;
        c.out_frames = 300 + rng() % 700;
        c.channels = rng() % 3 ? 2 : 1 + rng() % 6;
        c.dst = out_ptr(rng() % 4 ? 0 : 4);
        const uint32_t S = rng() % 80, variety = 1 + rng() % 6;
        const bool scene = rng() % 2;  // stereo sources of one rate: the specialised kernel's case, spoiled now and then
        for (uint32_t s = 0; s < S; ++s) {
            const uint32_t from = scene ? 44100 : rates[rng() % variety];
            const uint32_t g = std::gcd(from, c.to_rate), T = c.to_rate / g, F = from / g;
            rh_wide_src x = src(s, scene ? 2 : 1 + rng() % 3, from, scene ? 7 % T : (uint32_t)(rng() % T), c.out_frames);
            if (rng() % 40 == 0) x.frames = 0;
            else if (rng() % 40 == 0) x.frames = 1 + rng() % c.out_frames, x.last = (uint32_t)((x.phase + (x.frames - 1) * F) / T);
            else if (rng() % 40 == 0) x.last = (uint32_t)((x.phase + (c.out_frames - 1) * F) / T);  // every frame, but the last one verbatim
            if (rng() % 60 == 0) x.data = in_ptr(s, 4);
            c.add(x, rng() % 3, 5000000, rng() % 400, from);
        }
        EXPECT(c.check() == RH_OK, "a random call");
        const std::vector<Launch> Ls = c.launches();
        check_launches(c, Ls);
        for (const Launch &L : Ls) g_stereo += L.kernel == kStereo;
        ++n;
    }
    return n;
}

// ---- the shapes of the GPU tests and of the benchmark -----------------------------------------------------------------------------------------
static int test_shapes() {
    int n = 0;
    auto scene = [](uint32_t S, uint64_t M, uint64_t dst_off = 0) {
        Call c;
        c.out_frames = M, c.dst = out_ptr(dst_off);
        for (uint32_t s = 0; s < S; ++s) c.add(src(s, 2, 44100, 0, M), s % 2, 5000000, 0, 44100);
        return c;
    };
    for (uint32_t S : {1u, 16u, 32u, 33u, 37u, 256u}) {
        const Call c = scene(S, 17832);
        const std::vector<Launch> Ls = c.launches();
        check_launches(c, Ls);
        EXPECT(Ls.size() == (S + 31) / 32, "%u alike sources: %zu launches", S, Ls.size());
        for (const Launch &L : Ls) EXPECT(L.kernel == kStereo, "a scene takes the specialised kernel");
        const Call off = scene(S, 17832, 4);
        for (const Launch &L : off.launches()) EXPECT(L.kernel == kGeneral, "dst 4 bytes off an 8-byte boundary: the general kernel");
        ++n;
    }
    {  // five rates in one call: the fifth starts a launch
        Call c;
        const uint32_t r5[] = {44100, 48000, 8000, 96000, 22050};
        for (uint32_t s = 0; s < 10; ++s) c.add(src(s, 2, r5[s % 5], 0, 1000));
        const std::vector<Launch> Ls = c.launches();
        check_launches(c, Ls);
        EXPECT(Ls.size() == 3 && Ls[0].n == 4 && Ls[1].n == 4 && Ls[2].n == 2, "five rates: %zu launches, the first of %u", Ls.size(), Ls[0].n);
        ++n;
    }
    {  // one source of a scene ends inside the block, or has its last frame under the block's last tap: that launch is general, the others are not
        Call c = scene(64, 1000);
        c.srcs[40].frames = 500, c.srcs[40].last = (500 - 1) * 147 / 160;
        std::vector<Launch> Ls = c.launches();
        check_launches(c, Ls);
        EXPECT(Ls.size() == 2 && Ls[0].kernel == kStereo && Ls[1].kernel == kGeneral, "the launch with the source that ends");
        c = scene(64, 1000);
        c.srcs[3].last = (999 * 147) / 160;
        Ls = c.launches();
        check_launches(c, Ls);
        EXPECT(Ls[0].kernel == kGeneral && Ls[1].kernel == kStereo, "the last frame verbatim");
        c.srcs[3].last += 1;
        EXPECT(c.launches()[0].kernel == kStereo, "... and one frame later both taps are there");
        c = scene(8, 1000);
        c.srcs[5].channels = 1;
        EXPECT(c.launches()[0].kernel == kGeneral, "a mono source among them");
        c = scene(8, 1000);
        c.srcs[5].data = in_ptr(5, 4);
        EXPECT(c.launches()[0].kernel == kGeneral, "a row off its 8-byte boundary");
        c = scene(8, 1000);
        c.channels = 6;
        EXPECT(c.launches()[0].kernel == kGeneral, "a mix of six channels");
        c = scene(8, 1000);
        c.to_rate = 44100;
        EXPECT(c.launches()[0].kernel == kStereo, "F == T: no second tap to miss");
        n += 7;
    }
    {  // no source, and sources that reach nothing: one launch of zeros
        Call c;
        EXPECT(c.launches().size() == 1 && c.launches()[0].n == 0 && !c.launches()[0].cont && c.launches()[0].kernel == kGeneral, "no sources");
        c.add(rh_wide_src{nullptr, 0, 0, 0, 0, 0, 0.0f});
        EXPECT(c.check() == RH_OK && c.launches().size() == 1 && c.launches()[0].n == 0, "a source of no frames");
        n += 2;
    }
    return n;
}

int main(int argc, char **argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 0;
    const int calls = argc > 2 ? std::atoi(argv[2]) : 400;
    const int refusals = test_refusals();
    const long reach = test_reach(seed, calls);
    const int ramps = test_ramp_modes();
    const long walked = test_random(seed, calls);
    const int shapes = test_shapes();
    std::printf("failures %d refusals %d reach %ld ramps %d calls %ld stereo %ld shapes %d\n", g_failures, refusals, reach, ramps, walked, g_stereo, shapes);
    return g_failures ? 1 : 0;
}
