// wide_batch_plan_test.cpp -- the plan of rh_wide_mix_batch (rodio_amd/csrc/rh_wide_batch_plan.h) without a GPU: every output sample of every
// mixer lies in exactly one tile and no tile crosses a mixer, the source ranges are the prefix sums of the counts, the slots are the sources
// that reach the block in insertion order with the rate each one reads, every refusal of the header is answered, and the 32-bit fit is
// check_src's formula (rh_mix_plan.h) written out a second time.  TEST INFRASTRUCTURE: plain g++, no HIP, no library.  Pointers are never followed.
//
//     wide_batch_plan_test [seed [random batches]]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "rh_wide_batch_plan.h"

using namespace rh::widebatch;

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

static float *out_ptr(uint64_t k) { return reinterpret_cast<float *>((uintptr_t)(0x100000000ull + 0x1000000ull * k)); }
static const float *in_ptr(uint64_t k) { return reinterpret_cast<const float *>((uintptr_t)(0x800000000000ull + 0x1000ull * k)); }

struct Batch {
    std::vector<float *> dsts;
    std::vector<uint32_t> ch, rate, counts;
    std::vector<uint64_t> frames;
    std::vector<rh_wide_src> srcs;
    rh_status plan(Plan *p) const {
        return rh::widebatch::plan(dsts.data(), ch.data(), rate.data(), frames.data(), counts.data(), (uint32_t)dsts.size(), srcs.empty() ? nullptr : srcs.data(), p);
    }
    void add(uint32_t c, uint32_t r, uint64_t f, const std::vector<rh_wide_src> &s) {
        dsts.push_back(out_ptr(dsts.size())), ch.push_back(c), rate.push_back(r), frames.push_back(f), counts.push_back((uint32_t)s.size());
        srcs.insert(srcs.end(), s.begin(), s.end());
    }
};
static rh_wide_src src(uint64_t k, uint32_t ch, uint32_t rate, uint32_t phase, uint64_t frames, uint32_t last = 0xffffffffu, float gain = 1.0f) {
    return rh_wide_src{in_ptr(k), ch, rate, phase, frames, last, gain};
}

// Every property of an accepted plan that does not depend on how the batch was made.  Returns the samples it walked.
static uint64_t check_plan(const Batch &b, const Plan &p, bool mark) {
    const size_t B = b.dsts.size();
    EXPECT(p.mixers.size() == B && p.in_first.size() == B + 1, "sizes");
    if (p.mixers.size() != B || p.in_first.size() != B + 1) return 0;
    uint64_t at = 0, samples = 0;
    for (size_t m = 0; m < B; ++m) {  // the source ranges are the prefix sums of the counts
        EXPECT(p.in_first[m] == at, "mixer %zu: in_first %llu, prefix sum %llu", m, (unsigned long long)p.in_first[m], (unsigned long long)at);
        at += b.counts[m];
    }
    EXPECT(p.in_first[B] == at, "the total");
    EXPECT(p.tile_samples >= kBlock && p.tile_samples % kBlock == 0 && p.tile_samples <= kBlock * kMaxPer && ((p.tile_samples / kBlock) & (p.tile_samples / kBlock - 1)) == 0,
           "tile_samples %u", p.tile_samples);
    std::vector<uint32_t> seen_tiles(B, 0);
    uint32_t slots_before = 0xffffffffu;
    int64_t last_mixer = -1;
    for (size_t t = 0; t < p.tiles.size(); ++t) {
        const Tile &tl = p.tiles[t];
        EXPECT(tl.mixer < B, "tile %zu: mixer %u", t, tl.mixer);
        if (tl.mixer >= B) return samples;
        const Mixer &m = p.mixers[tl.mixer];
        const uint64_t total = (uint64_t)m.frames * m.ch, o = (uint64_t)tl.j0 * m.ch + tl.c0;
        EXPECT(tl.c0 < m.ch && tl.n >= 1 && tl.n <= p.tile_samples && o + tl.n <= total, "tile %zu crosses its mixer: [%llu, +%u) of %llu", t, (unsigned long long)o, tl.n, (unsigned long long)total);
        // a mixer's tiles are one run of the table, in the order of its samples, each starting where the one before ended
        EXPECT(t >= m.tile_first && t < (uint64_t)m.tile_first + m.n_tiles, "tile %zu outside its mixer's range [%u, +%u)", t, m.tile_first, m.n_tiles);
        EXPECT(o == (uint64_t)(t - m.tile_first) * p.tile_samples, "tile %zu does not start where the one before it ended", t);
        EXPECT(tl.n == std::min<uint64_t>(p.tile_samples, total - o), "tile %zu: %u samples", t, tl.n);
        if ((int64_t)tl.mixer != last_mixer) {  // the mixers with the most sources first
            uint32_t live = 0;
            for (uint64_t s = p.in_first[tl.mixer]; s < p.in_first[tl.mixer + 1]; ++s) live += b.srcs[s].frames ? 1 : 0;
            EXPECT(live <= slots_before, "tile %zu: a mixer of %u sources behind one of %u", t, live, slots_before);
            slots_before = live, last_mixer = tl.mixer;
        }
        ++seen_tiles[tl.mixer];
        samples += tl.n;
    }
    if (mark) {  // sample by sample: exactly one tile each
        for (size_t k = 0; k < B; ++k) {
            const Mixer &m = p.mixers[k];
            std::vector<uint8_t> hit((size_t)m.frames * m.ch, 0);
            for (const Tile &tl : p.tiles)
                if (tl.mixer == k)
                    for (uint32_t i = 0; i < tl.n; ++i) {
                        const uint64_t o = (uint64_t)tl.j0 * m.ch + tl.c0 + i;
                        if (o < hit.size()) ++hit[o];
                    }
            EXPECT(std::all_of(hit.begin(), hit.end(), [](uint8_t h) { return h == 1; }), "mixer %zu: a sample in no tile or in two", k);
        }
    }
    uint64_t want_samples = 0;
    for (size_t k = 0; k < B; ++k) {
        const Mixer &m = p.mixers[k];
        const uint64_t total = b.frames[k] * b.ch[k] * (b.frames[k] ? 1 : 0);
        want_samples += b.frames[k] ? total : 0;
        EXPECT(seen_tiles[k] == m.n_tiles && m.n_tiles == (total + p.tile_samples - 1) / p.tile_samples, "mixer %zu: %u tiles seen, %u planned", k, seen_tiles[k], m.n_tiles);
        if (b.frames[k] == 0) {
            EXPECT(m.frames == 0 && m.src_slots == 0 && m.n_tiles == 0, "a skipped mixer with work");
            continue;
        }
        EXPECT(m.dst == b.dsts[k] && m.ch == b.ch[k] && m.frames == b.frames[k], "mixer %zu: dst / channels / frames", k);
        EXPECT(m.src_slots % (m.uniform ? kUniGroup : kGroup) == 0 && (uint64_t)m.src_first + m.src_slots <= p.srcs.size(), "mixer %zu: slots", k);
        {  // alike sources, written out a second time: the mixer's layout, one pair, every frame of the block with both taps
            bool alike = false, first = true;
            uint32_t F0 = 0, T0 = 1, ph0 = 0;
            for (uint64_t s = p.in_first[k]; s < p.in_first[k + 1]; ++s) {
                const rh_wide_src &x = b.srcs[s];
                if (x.frames == 0) continue;
                const uint32_t g = std::gcd(x.from_rate, b.rate[k]), F = x.from_rate / g, T = b.rate[k] / g;
                if (first) alike = true, first = false, F0 = F, T0 = T, ph0 = x.phase;
                const uint64_t i_last = ((uint64_t)x.phase + (b.frames[k] - 1) * F) / T;  // the first tap of the block's last frame
                alike = alike && x.channels == b.ch[k] && F == F0 && T == T0 && x.phase == ph0 && x.frames == b.frames[k] && (F == T || i_last < x.last);
            }
            EXPECT((m.uniform != 0) == alike, "mixer %zu: uniform %u, alike %d", k, m.uniform, (int)alike);
        }
        // the slots: the sources that reach the block, in insertion order, then slots that reach nothing
        uint32_t slot = m.src_first;
        std::vector<Rate> pairs;
        for (uint64_t s = p.in_first[k]; s < p.in_first[k + 1]; ++s) {
            const rh_wide_src &x = b.srcs[s];
            if (x.frames == 0) continue;
            EXPECT(slot < m.src_first + m.src_slots, "mixer %zu: a source without a slot", k);
            if (slot >= m.src_first + m.src_slots) break;
            const Src &d = p.srcs[slot++];
            const uint32_t g = std::gcd(x.from_rate, b.rate[k]), F = x.from_rate / g, T = b.rate[k] / g;
            EXPECT(d.data == x.data && d.ch == x.channels && d.frames == x.frames && d.last == x.last && d.gain == x.gain, "mixer %zu source %llu: fields", k, (unsigned long long)s);
            EXPECT(d.F == F && d.T == T && d.r0 == x.phase && d.Tf == (F == T ? 0.0f : (float)T), "mixer %zu source %llu: rate", k, (unsigned long long)s);
            EXPECT(d.rate <= kOwnRate, "rate index %u", d.rate);
            if (d.rate < kRates) EXPECT(m.r[d.rate].F == F && m.r[d.rate].T == T && m.r[d.rate].r0 == x.phase && m.r[d.rate].Tf == (float)T, "mixer %zu source %llu reads another pair", k, (unsigned long long)s);
            if (std::none_of(pairs.begin(), pairs.end(), [&](const Rate &r) { return r.F == F && r.T == T && r.r0 == x.phase; })) pairs.push_back(Rate{F, T, x.phase, 0.0f});
            // a source divides for itself only when its pair is not among the first kRates distinct ones
            const size_t idx = (size_t)(std::find_if(pairs.begin(), pairs.end(), [&](const Rate &r) { return r.F == F && r.T == T && r.r0 == x.phase; }) - pairs.begin());
            EXPECT(d.rate == (idx < kRates ? idx : kOwnRate), "mixer %zu source %llu: pair %zu, index %u", k, (unsigned long long)s, idx, d.rate);
            // the 32-bit fit: every position the kernel forms stays below 2^32
            EXPECT((uint64_t)x.phase + (b.frames[k] - 1) * F + 0ull <= 0xffffffffull, "mixer %zu source %llu: phase + j F leaves 32 bits", k, (unsigned long long)s);
        }
        EXPECT(m.src_first + m.src_slots - slot < (m.uniform ? kUniGroup : kGroup), "mixer %zu: %u slots behind its last source", k, m.src_first + m.src_slots - slot);
        for (; slot < m.src_first + m.src_slots; ++slot) EXPECT(p.srcs[slot].frames == 0 && p.srcs[slot].data != nullptr && p.srcs[slot].T != 0 && p.srcs[slot].rate < kRates, "mixer %zu: a padding slot with work", k);
        for (uint32_t q = 0; q < kRates; ++q) EXPECT(m.r[q].T != 0, "mixer %zu: a pair that divides by zero", k);
    }
    EXPECT(samples == want_samples, "%llu samples in tiles, %llu in the batch", (unsigned long long)samples, (unsigned long long)want_samples);
    return samples;
}

static const uint32_t kRatesHz[] = {8000, 11025, 22050, 32000, 44100, 48000, 96000};

static long g_uniform = 0;  // mixers of alike sources among the random ones
static long test_random(uint32_t seed, int n) {
    std::mt19937 rng(seed);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
    long accepted = 0;
    Plan p;
    for (int it = 0; it < n; ++it) {
        Batch b;
        const uint32_t B = pick(1, 12);
        for (uint32_t m = 0; m < B; ++m) {
            const uint32_t ch = pick(1, 8), rate = kRatesHz[rng() % 7];
            const uint64_t frames = (rng() % 5 == 0) ? 0 : (rng() % 4 == 0 ? pick(1, 40000) : pick(1, 700));
            std::vector<rh_wide_src> s;
            const uint32_t ns = rng() % 6 == 0 ? pick(30, 45) : pick(0, 9);
            const bool alike = rng() % 3 == 0;  // (mostly) the mixer's layout, one rate and phase, whole blocks
            const uint32_t from0 = kRatesHz[rng() % 7], phase0 = rng() % (rate / std::gcd(from0, rate));
            for (uint32_t k = 0; k < ns; ++k) {
                const uint32_t from = alike ? from0 : kRatesHz[rng() % 7], T = rate / std::gcd(from, rate);
                const uint64_t f = frames == 0 || rng() % (alike ? 40 : 5) == 0 ? 0 : (rng() % (alike ? 40 : 3) == 0 ? pick(1, (uint32_t)frames) : frames);
                s.push_back(src(b.srcs.size() + k, alike ? ch : pick(1, 6), from, alike ? phase0 : rng() % T, f, rng() % (alike ? 20 : 3) ? 0xffffffffu : pick(0, 100), (float)pick(0, 4) - 2.0f));
            }
            b.add(ch, rate, frames, s);
        }
        const rh_status st = b.plan(&p);
        EXPECT(st == RH_OK, "a valid batch refused: %d", (int)st);
        if (st == RH_OK) {
            ++accepted, check_plan(b, p, true);
            for (const Mixer &m : p.mixers) g_uniform += m.uniform;
        }
    }
    return accepted;
}

// a fresh plan object per refusal: nothing of an earlier plan may make a refused batch look planned
static rh_status status_of(const Batch &b) {
    Plan p;
    return b.plan(&p);
}

static int test_refusals() {
    int n = 0;
    Plan p;
    auto good = [] {
        Batch b;
        b.add(2, 48000, 100, {src(0, 2, 44100, 0, 100), src(1, 1, 48000, 0, 50, 49)});
        b.add(6, 48000, 64, {src(2, 6, 44100, 3, 64)});
        return b;
    };
    EXPECT(status_of(good()) == RH_OK, "the good batch");
    // n_mixers == 0: RH_OK, whatever the arrays are
    EXPECT(rh::widebatch::plan(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &p) == RH_OK && p.tiles.empty(), "n_mixers == 0");
    {  // a NULL array with n_mixers > 0
        const Batch b = good();
        const uint32_t B = 2;
        EXPECT(rh::widebatch::plan(nullptr, b.ch.data(), b.rate.data(), b.frames.data(), b.counts.data(), B, b.srcs.data(), &p) == RH_ERR_INVALID, "dsts NULL"); ++n;
        EXPECT(rh::widebatch::plan(b.dsts.data(), nullptr, b.rate.data(), b.frames.data(), b.counts.data(), B, b.srcs.data(), &p) == RH_ERR_INVALID, "channels NULL"); ++n;
        EXPECT(rh::widebatch::plan(b.dsts.data(), b.ch.data(), nullptr, b.frames.data(), b.counts.data(), B, b.srcs.data(), &p) == RH_ERR_INVALID, "to_rates NULL"); ++n;
        EXPECT(rh::widebatch::plan(b.dsts.data(), b.ch.data(), b.rate.data(), nullptr, b.counts.data(), B, b.srcs.data(), &p) == RH_ERR_INVALID, "out_frames NULL"); ++n;
        EXPECT(rh::widebatch::plan(b.dsts.data(), b.ch.data(), b.rate.data(), b.frames.data(), nullptr, B, b.srcs.data(), &p) == RH_ERR_INVALID, "src_counts NULL"); ++n;
        EXPECT(rh::widebatch::plan(b.dsts.data(), b.ch.data(), b.rate.data(), b.frames.data(), b.counts.data(), B, nullptr, &p) == RH_ERR_INVALID, "srcs NULL"); ++n;
        const uint32_t none[2] = {0, 0};
        EXPECT(rh::widebatch::plan(b.dsts.data(), b.ch.data(), b.rate.data(), b.frames.data(), none, B, nullptr, &p) == RH_OK, "srcs NULL without sources");
    }
    auto refused = [&](const char *what, rh_status want, auto change) {
        Batch b = good();
        change(b);
        const rh_status st = status_of(b);
        EXPECT(st == want, "%s: status %d, expected %d", what, (int)st, (int)want);
        ++n;
    };
    refused("a NULL dst with out_frames > 0", RH_ERR_INVALID, [](Batch &b) { b.dsts[1] = nullptr; });
    refused("channels of 0", RH_ERR_INVALID, [](Batch &b) { b.ch[1] = 0; });
    refused("to_rate of 0", RH_ERR_INVALID, [](Batch &b) { b.rate[0] = 0; });
    refused("a source without data", RH_ERR_INVALID, [](Batch &b) { b.srcs[2].data = nullptr; });
    refused("a source of 0 channels", RH_ERR_INVALID, [](Batch &b) { b.srcs[0].channels = 0; });
    refused("a source of rate 0", RH_ERR_INVALID, [](Batch &b) { b.srcs[1].from_rate = 0; });
    refused("a source that reaches more frames than the block has", RH_ERR_INVALID, [](Batch &b) { b.srcs[2].frames = 65; });
    refused("a phase that is no remainder mod T", RH_ERR_INVALID, [](Batch &b) { b.srcs[0].phase = 160; });
    refused("F * T beyond 32 bits", RH_ERR_UNSUPPORTED, [](Batch &b) { b.srcs[0].from_rate = 4294967291u; });
    refused("out_frames beyond 2^31 - 1", RH_ERR_UNSUPPORTED, [](Batch &b) { b.frames[1] = 0x80000000ull; });
    refused("a block too long for 32-bit positions", RH_ERR_UNSUPPORTED, [](Batch &b) {
        b.ch[0] = 1, b.frames[0] = 70000, b.srcs[0] = src(0, 1, 65521, 0, 70000), b.srcs[1].frames = 0;
    });
    // what is NOT refused: a mixer with out_frames == 0 is not looked at (NULL dst, zero channels and rate, sources that would be refused)
    {
        Batch b = good();
        b.frames[1] = 0, b.dsts[1] = nullptr, b.ch[1] = 0, b.rate[1] = 0, b.srcs[2].data = nullptr, b.srcs[2].channels = 0;
        const rh_status st = b.plan(&p);
        EXPECT(st == RH_OK, "a skipped mixer was looked at: %d", (int)st);
        if (st == RH_OK) check_plan(b, p, true);
    }
    {  // ... nor is a source with frames == 0 (NULL data, zero channels and rate)
        Batch b = good();
        b.srcs[1] = rh_wide_src{nullptr, 0, 0, 99999, 0, 0, 0.0f};
        const rh_status st = b.plan(&p);
        EXPECT(st == RH_OK, "a source of no frames was looked at: %d", (int)st);
        if (st == RH_OK) {
            check_plan(b, p, true);
            EXPECT(p.mixers[0].uniform == 1 && p.mixers[0].src_slots == kUniGroup, "one source of the mixer's layout is left: %u slots", p.mixers[0].src_slots);
        }
    }
    return n;
}

// The fit against check_src's formula (rh_mix_plan.h), (2^32 - 1 - T) / F, on both sides of the boundary, and its meaning: the last position fits.
static long test_fit() {
    long n = 0;
    const uint32_t pairs[][2] = {{65521, 48000}, {96000, 8000}, {48000, 44100}, {4294967291u, 1}, {65535, 65537}, {192000, 1}, {3, 2}};
    for (const auto &pr : pairs) {
        const uint32_t from = pr[0], to = pr[1], g = std::gcd(from, to), F = from / g, T = to / g;
        const uint64_t fit = (0xffffffffull - T) / F;
        uint32_t F2, T2;
        uint64_t fit2;
        EXPECT(check_src(src(0, 1, from, 0, 1), to, 1, &F2, &T2, &fit2) == RH_OK && F2 == F && T2 == T && fit2 == fit, "check_src(%u, %u)", from, to);
        EXPECT((uint64_t)(T - 1) + (fit - 1) * F <= 0xffffffffull, "fit admits a position beyond 32 bits");
        for (uint64_t frames : {fit - 1, fit, fit + 1}) {
            if (frames == 0 || frames > 0x7fffffffull) continue;
            Batch b;
            b.add(1, to, frames, {src(0, 1, from, T - 1, frames)});
            const rh_status st = status_of(b);
            EXPECT(st == (frames <= fit ? RH_OK : RH_ERR_UNSUPPORTED), "from %u to %u, %llu frames (fit %llu): %d", from, to, (unsigned long long)frames, (unsigned long long)fit, (int)st);
            ++n;
        }
    }
    return n;
}

// Batches at the sizes of the benchmark and of the tests: the tile count stays bounded, the long pole goes first.
static long test_shapes() {
    long n = 0;
    Plan p;
    for (uint32_t B : {1u, 8u, 64u, 256u, 1000u})
        for (uint64_t frames : {33ull, 1024ull, 16384ull, 70000ull}) {
            Batch b;
            for (uint32_t m = 0; m < B; ++m) {
                std::vector<rh_wide_src> s;
                for (uint32_t k = 0; k < (m % 3 == 0 ? 40u : 16u); ++k) s.push_back(src(m * 64 + k, 6, 44100, 0, frames));
                b.add(6, 48000, frames, s);
            }
            EXPECT(b.plan(&p) == RH_OK, "B %u frames %llu", B, (unsigned long long)frames);
            check_plan(b, p, false);
            const uint64_t at_block = (uint64_t)B * ((frames * 6 + kBlock - 1) / kBlock);
            EXPECT(p.tiles.size() <= std::max<uint64_t>(kMaxTiles, B) + B, "B %u frames %llu: %zu tiles", B, (unsigned long long)frames, p.tiles.size());
            EXPECT(at_block > kMaxTiles || p.tile_samples == kBlock, "a small batch in large tiles: %u", p.tile_samples);
            EXPECT(p.mixers[p.tiles[0].mixer].src_slots == 40, "the mixers with 40 sources go first");
            EXPECT(!one_mixer_goes_alone(p), "B %u: 40 sources are more than a launch of rh_wide_mix_block holds", B);
            ++n;
        }
    {  // a call of one mixer goes to rh_wide_mix_block exactly where that entry takes one launch
        auto alone = [&](const std::vector<rh_wide_src> &s, uint32_t mixers = 1) {
            Batch b;
            for (uint32_t m = 0; m < mixers; ++m) b.add(2, 48000, 2000, s);
            EXPECT(b.plan(&p) == RH_OK, "a one-mixer batch");
            ++n;
            return one_mixer_goes_alone(p);
        };
        std::vector<rh_wide_src> alike(16, src(0, 2, 44100, 0, 2000)), pairs5, ending = alike;
        for (uint32_t k = 0; k < 5; ++k) pairs5.push_back(src(k, 1, kRatesHz[k], 0, 2000));
        ending[3].frames = 1500, ending[3].last = 1400;
        EXPECT(alone(alike), "alike sources: one launch there");
        EXPECT(!alone(alike, 2), "two mixers are a batch");
        EXPECT(alone({src(0, 2, 44100, 0, 2000), src(1, 1, 22050, 0, 1000, 400), src(2, 6, 48000, 0, 2000)}), "three layouts, three pairs: one launch there");
        EXPECT(alone({}), "no sources: one launch of zeros there");
        EXPECT(!alone(pairs5), "five pairs: two launches there");
        EXPECT(!alone(ending), "alike sources of which one ends inside the block: two launches there");
    }
    {  // the ragged grid of the GPU test: 300 mixers of 33 frames and one of 70 000
        Batch b;
        for (uint32_t m = 0; m < 300; ++m) b.add(2, 48000, 33, {src(2 * m, 2, 44100, 0, 33), src(2 * m + 1, 1, 48000, 0, 33)});
        b.add(2, 48000, 70000, {src(1000, 2, 44100, 0, 70000), src(1001, 2, 22050, 0, 70000), src(1002, 1, 48000, 0, 70000)});
        EXPECT(b.plan(&p) == RH_OK, "the ragged batch");
        check_plan(b, p, true);
        EXPECT(p.tiles.size() == 300 + (70000 * 2 + kBlock - 1) / kBlock && p.tiles[0].mixer == 300, "the ragged batch: %zu tiles, the first of mixer %u", p.tiles.size(), p.tiles[0].mixer);
        ++n;
    }
    return n;
}

int main(int argc, char **argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 0;
    const int batches = argc > 2 ? std::atoi(argv[2]) : 400;
    static_assert(sizeof(Mixer) == 104 && sizeof(Src) == 48 && sizeof(Tile) == 16, "the tables' layout");
    const long accepted = test_random(seed, batches);
    const int refusals = test_refusals();
    const long fits = test_fit();
    const long shapes = test_shapes();
    std::printf("failures %d batches %ld uniform %ld refusals %d fits %ld shapes %ld\n", g_failures, accepted, g_uniform, refusals, fits, shapes);
    return g_failures ? 1 : 0;
}
