// clip_mix_plan_test.cpp -- rodio_amd/csrc/rh_clip_mix_plan.h without a GPU: the words of a clip (plan), the cursor (advance), the refusals
// with their exact 32-bit bounds, and the kernel's position arithmetic -- describe(), locate() and fade_ms() as the kernel calls them --
// against a model that walks the clip's stream chain by chain and output frame by output frame, over seeded random clips and random cuts
// into blocks: any cut must give the positions of one pass.  A plain g++ program (TEST INFRASTRUCTURE: nothing of the product links it).
//     clip_mix_plan_test [seed [clips]]                      the whole run; prints its counters, exit status 1 on a failure
//     clip_mix_plan_test plan n ch rate span_len delay_ns take_ns flags      -> status and the words
//     clip_mix_plan_test advance w0 .. w6 ch from_rate to_rate out_frames    -> status and the words
//     clip_mix_plan_test locate w0 .. w6 ch from_rate to_ch to_rate frames out_frames m ..
//                          -> status, then "fade x0 M c klast zrel data-offset ms0" of describe(), then per output frame m of the block
//                             "ia lerp num R": locate(), and the bits of fade_ms() of the first tap's channel 0 (0 where it meets none)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "rh_clip_mix_plan.h"

using namespace rh::clipmix;

static int g_failures = 0, g_divs = 0, g_clips = 0, g_blocks = 0, g_taps = 0, g_faded = 0, g_delay_taps = 0, g_refusals = 0, g_bounds = 0, g_fade64 = 0;

#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            if (++g_failures <= 20) {                           \
                std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                       \
                std::printf("\n");                              \
            }                                                   \
        }                                                       \
    } while (0)

static float kSound[8];  // an address that is never read through: the host only moves it

// ---- the model: the clip's stream, chain by chain, output frame by output frame ------------------------------------------------------------
struct Frame {
    uint64_t sa;  // stream sample of the first tap's channel 0
    bool lerp;
    uint64_t num;
};
struct Clip {
    uint64_t n, span_len, delay_ns, take_ns;
    uint32_t ch, rate, to_rate, flags;
};
static std::vector<Frame> model(const Words &w, uint32_t ch, uint64_t F, uint64_t T) {
    std::vector<Frame> out;
    const uint64_t Ls = w.Z + w.N;
    for (uint64_t p = 0; p < Ls;) {
        const uint64_t n = w.kind == kRuleG ? (Ls - p < 32768 ? Ls - p : 32768) : Ls - p;  // uniform.rs:56
        const uint64_t f = n / ch;
        for (uint64_t j = 0;; ++j) {  // a fresh converter: frames while both taps exist, then the last frame once, verbatim
            const uint64_t i = j * F / T, num = j * F % T;
            if (i + 1 < f) out.push_back(Frame{p + i * ch, F != T, num});
            else {
                if (i + 1 == f) out.push_back(Frame{p + i * ch, false, num});
                if (F != T || i + 1 >= f) break;
            }
        }
        p += n;
    }
    return out;
}

// One block of a clip through describe / locate / fade_ms against the model's frames [done, done + frames).
static void check_block(const Words &w, const std::vector<Frame> &fr, uint32_t ch, uint32_t rate, uint32_t to_rate, uint32_t to_ch, uint64_t frames, uint64_t out_frames, std::mt19937_64 &rng) {
    uint64_t words[RH_CLIP_WORDS] = {w.kind, w.Z, w.N, w.take_ns, w.flags, w.done, w.total};
    rh_wide_src x{};
    x.data = kSound, x.channels = ch, x.from_rate = rate, x.frames = frames, x.gain = 0.5f, x.phase = 12345u, x.last = 7u;  // (phase and last are not read)
    Desc d;
    const rh_status st = describe(x, words, to_ch, to_rate, out_frames, &d);
    CHECK(st == RH_OK, "describe %d: kind %d Z %" PRIu64 " N %" PRIu64 " done %" PRIu64 " frames %" PRIu64 " ch %u %u -> %u", (int)st, (int)w.kind, w.Z, w.N, w.done, frames, ch, rate, to_rate);
    if (st != RH_OK) return;
    ++g_blocks;
    const uint64_t kbase = (uint64_t)(d.data - kSound);
    CHECK(!(kbase && d.zrel), "both a delay and an offset");
    const uint64_t base = d.zrel ? w.Z - d.zrel : w.Z + kbase;  // (no clip of this run has a delay beyond 32 bits)
    const uint64_t dps = (w.flags & kTake) ? ns_per_sample(ch, rate) : 0;
    if (d.fade == kFade64) ++g_fade64;
    const uint64_t step = frames > 3000 ? 1 + rng() % 7 : 1;
    for (uint64_t m = 0; m < frames; m += (m + 40 > frames || m < 40) ? 1 : step) {
        const Taps t = locate(d, (uint32_t)m);
        const Frame &want = fr[w.done + m];
        const uint64_t sa = base + (uint64_t)t.ia * ch;
        CHECK(sa == want.sa && t.lerp == want.lerp && (!t.lerp || t.num == want.num), "frame %" PRIu64 "+%" PRIu64 ": tap %" PRIu64 " (%" PRIu64 ") lerp %d (%d) num %u (%" PRIu64 ")", w.done, m,
              sa, want.sa, (int)t.lerp, (int)want.lerp, t.num, want.num);
        if (sa != want.sa) return;
        for (uint32_t c = 0; c < ch; c += (ch > 2 ? ch - 1 : 1)) {
            for (int tap = 0; tap < (t.lerp ? 2 : 1); ++tap) {
                const uint64_t sr64 = tap_sample(d, t.ia, c) + (uint64_t)tap * d.ch;  // the kernel's stream sample: a clip's fits 32 bits
                CHECK(sr64 <= 0xffffffffull, "a clip's sample beyond 32 bits");
                const uint32_t sr = (uint32_t)sr64;
                const uint64_t s = want.sa + (uint64_t)tap * ch + c;
                CHECK(base + sr == s && s < w.Z + w.N, "sample %" PRIu64, s);
                ++g_taps;
                if (s < w.Z) {
                    CHECK(sr < d.zrel, "a tap of the delay is read");
                    ++g_delay_taps;
                    continue;
                }
                CHECK(sr >= d.zrel, "a tap of the sound is taken for the delay");
                const uint32_t krel = sr - d.zrel;
                const uint64_t k = s - w.Z;
                CHECK(kbase + krel == k && k < w.N, "sound sample %" PRIu64, k);
                if (w.flags & kFade) {
                    const float R = (float)((w.take_ns - k * dps) / 1000000ull);
                    const float got = fade_ms(d, krel);
                    CHECK(got == R && d.Ttf == (float)(w.take_ns / 1000000ull), "fade of sample %" PRIu64 ": %g (%g)", k, (double)got, (double)R);
                    ++g_faded;
                } else {
                    CHECK(d.fade == kNoFade, "a fade nobody set");
                }
            }
        }
    }
}

static const uint32_t kChannels[7] = {1, 2, 2, 2, 4, 6, 8}, kMixChannels[3] = {1, 2, 6};
static const uint32_t kRates[][2] = {{44100, 48000}, {48000, 44100}, {48000, 48000}, {8000, 48000}, {96000, 44100}, {65521, 48000}, {48000, 65521}, {44100, 11025}};

static void test_divs(std::mt19937_64 &rng) {
    for (int q = 0; q < 200000; ++q) {
        const uint32_t x = q < 2000 ? (uint32_t)(0xffffffffu - q) : (q < 4000 ? (uint32_t)(q - 2000) * 1000000u + (uint32_t)(rng() % 3) - 1u : (uint32_t)rng());
        CHECK(div_u32(x, kDivMs) == x / 1000000u, "%u / 10^6", x);
        ++g_divs;
    }
    CHECK(make_div(1000000).m == kDivMs.m && make_div(1000000).sh == kDivMs.sh, "kDivMs is not make_div(10^6)");
}

static void test_clips(std::mt19937_64 &rng, int clips) {
    for (int q = 0; q < clips; ++q) {
        Clip c{};
        c.ch = kChannels[rng() % 7];
        const uint32_t *rt = kRates[rng() % 8];
        c.rate = rt[0], c.to_rate = rt[1];
        const uint64_t cap = (c.ch == 6) ? 30000 : 120000;  // 6 channels: one chain only
        c.n = rng() % (q % 5 == 0 ? 300 : cap);
        const uint64_t Zwant = (q % 4 == 0) ? 0 : rng() % (q % 3 == 0 ? 70 : (c.ch == 6 ? 2700 : 100000));
        c.delay_ns = (Zwant * 1000000000ull + (uint64_t)c.ch * c.rate - 1) / ((uint64_t)c.ch * c.rate);
        c.flags = (uint32_t)(rng() % 4);
        if (c.flags == kFade) c.flags = kTake | kFade;
        const uint64_t dps = ns_per_sample(c.ch, c.rate);
        c.take_ns = (c.flags & kTake) ? (rng() % (c.n + c.n / 2 + 2)) * dps + rng() % dps : 0;
        if (q % 17 == 0 && (c.flags & kTake)) c.take_ns = rng() % 1500000;  // around and under a millisecond
        c.span_len = (rng() & 1) ? c.n : 0;
        uint64_t words[RH_CLIP_WORDS];
        rh_status st = clip_plan(words, c.n, c.ch, c.rate, c.span_len, c.delay_ns, c.take_ns, c.flags);
        // what the plan must say, from the rule
        const uint64_t Z = (uint64_t)((unsigned __int128)c.delay_ns * c.ch * c.rate / 1000000000ull);
        const uint64_t N = (c.flags & kTake) ? (c.take_ns / dps < c.n ? c.take_ns / dps : c.n) : c.n;
        const bool G = (c.flags & kTake) || c.span_len;
        const bool cut = (Z + N) % c.ch || (G && Z + N > 32768 && 32768 % c.ch);
        CHECK(Z == Zwant, "Z");
        CHECK(st == (cut ? RH_ERR_UNSUPPORTED : RH_OK), "plan %d, cut %d", (int)st, (int)cut);
        if (st != RH_OK) {  // make it a clip of whole frames: move the delay
            c.delay_ns = ((Zwant + c.ch - (Z + N) % c.ch) * 1000000000ull + (uint64_t)c.ch * c.rate - 1) / ((uint64_t)c.ch * c.rate);
            if (clip_plan(words, c.n, c.ch, c.rate, c.span_len, c.delay_ns, c.take_ns, c.flags) != RH_OK) continue;
        }
        Words w = words_of(words);
        CHECK(w.kind == (G ? kRuleG : kRuleC) && w.N == N && w.flags == c.flags && w.done == 0 && w.take_ns == c.take_ns, "words");
        const uint32_t g = std::gcd(c.rate, c.to_rate);
        const uint64_t F = c.rate / g, T = c.to_rate / g;
        const std::vector<Frame> fr = model(w, c.ch, F, T);
        st = clip_advance(words, c.ch, c.rate, c.to_rate, 0);
        CHECK(st == RH_OK && words[6] == fr.size() && words[5] == 0, "total %" PRIu64 " (%zu)", words[6], fr.size());
        if (st != RH_OK || words[6] != fr.size()) continue;
        ++g_clips;
        const uint32_t to_ch = kMixChannels[rng() % 3];
        // the whole clip in one block, then random cuts: the same positions either way (both are held against the one model)
        for (int pass = 0; pass < 2; ++pass) {
            uint64_t cur[RH_CLIP_WORDS];
            std::memcpy(cur, words, sizeof cur);
            while (cur[5] < cur[6]) {
                const uint64_t left = cur[6] - cur[5];
                uint64_t frames = pass == 0 ? left : 1 + rng() % (rng() % 3 ? 2000 : left);
                if (frames > left) frames = left;
                if (w.kind == kRuleC && frames > (0xffffffffull - T) / F) frames = (0xffffffffull - T) / F;  // (one chain: a block's positions r0 + j F stay inside 32 bits)
                check_block(words_of(cur), fr, c.ch, c.rate, c.to_rate, to_ch, frames, frames + rng() % 3, rng);
                const uint64_t before = cur[5];
                CHECK(clip_advance(cur, c.ch, c.rate, c.to_rate, frames) == RH_OK && cur[5] == before + frames, "advance");
                if (cur[5] != before + frames) break;
            }
            CHECK(clip_advance(cur, c.ch, c.rate, c.to_rate, 99) == RH_OK && cur[5] == cur[6], "the cursor stops at the end");
        }
    }
}

// Positions do not depend on the delay or on the play time: a clip moved by whole chains (rule G) or by whole periods of the converter
// (rule C), its cursor moved with it, has the same descriptor, however far it is moved.
static void test_shifts(std::mt19937_64 &rng) {
    for (int q = 0; q < 200; ++q) {
        const uint32_t ch = 2, rate = 44100, to_rate = 48000;
        const uint64_t F = 147, T = 160;
        const bool G = q & 1;
        const uint64_t Z = (G ? 32769 : 1) + 2 * (rng() % 50000), N = 1 + 2 * (rng() % 60000);  // (rule G: more than one chain before the move, too)
        const uint64_t take_ns = (N + 5) * ns_per_sample(ch, rate);
        uint64_t a[RH_CLIP_WORDS] = {G ? (uint64_t)kRuleG : (uint64_t)kRuleC, Z, N, G ? take_ns : 0, G ? (uint64_t)(kTake | kFade) : 0, 0, 0};
        CHECK(clip_advance(a, ch, rate, to_rate, rng() % 100000) == RH_OK, "advance");
        if (a[5] == a[6]) continue;
        const uint64_t far = 1 + rng() % (1ull << 38);
        uint64_t b[RH_CLIP_WORDS];
        std::memcpy(b, a, sizeof b);
        if (G) b[1] += far * 32768, b[5] += far * (uint64_t)lm::span_out(16384, F, T);
        else b[1] += far * F * ch, b[5] += far * T;
        rh_wide_src x{};
        x.data = kSound, x.channels = ch, x.from_rate = rate, x.gain = 1.0f;
        x.frames = 1 + rng() % (a[6] - a[5]);
        Desc da, db;
        const rh_status sa = describe(x, a, 2, to_rate, x.frames, &da), sb = describe(x, b, 2, to_rate, x.frames, &db);
        CHECK(sa == RH_OK && sb == RH_OK, "describe %d %d", (int)sa, (int)sb);
        if (sa != RH_OK || sb != RH_OK) continue;
        const uint64_t base_a = da.zrel ? Z - da.zrel : Z + (uint64_t)(da.data - kSound);
        if (Z > base_a && !G) continue;  // (rule C: the shifted clip's first tap lies deeper in its delay, zrel differs by design)
        CHECK(da.data == db.data && da.x0 == db.x0 && da.r0 == db.r0 && da.M == db.M && da.c == db.c && da.klast == db.klast && da.nl == db.nl && da.nl_last == db.nl_last &&
                  da.zrel == db.zrel && da.fade == db.fade && da.ms0 == db.ms0 && da.ns_pad == db.ns_pad,
              "a descriptor that depends on the delay");
        ++g_blocks;
    }
}

static rh_status call(const rh_wide_src *srcs, uint32_t n, const uint64_t *clips, uint64_t out_frames, uint32_t ch = 2, uint32_t to_rate = 48000, const float *dst = kSound) {
    return check(dst, ch, to_rate, out_frames, srcs, n, clips);
}

static void test_refusals() {
    const uint32_t rate = 44100;
    const uint64_t dps = ns_per_sample(2, rate);
    rh_wide_src good[2]{};
    good[0].data = kSound, good[0].channels = 2, good[0].from_rate = rate, good[0].frames = 100, good[0].gain = 1.0f, good[0].last = 0xffffffffu;  // a plain source
    good[1] = good[0];
    uint64_t words[2 * RH_CLIP_WORDS] = {0};
    uint64_t *w = words + RH_CLIP_WORDS;
    CHECK(clip_plan(w, 4000, 2, rate, 4000, 10000000, 3000 * dps, 3) == RH_OK, "plan");
    CHECK(call(good, 2, words, 100) == RH_OK, "the good call");
    auto refused = [&](rh_status want, auto &&edit, uint64_t out_frames = 100, uint32_t ch = 2, uint32_t to_rate = 48000) {
        rh_wide_src s[2] = {good[0], good[1]};
        uint64_t ww[2 * RH_CLIP_WORDS];
        std::memcpy(ww, words, sizeof ww);
        edit(s, ww + RH_CLIP_WORDS);
        const rh_status st = call(s, 2, ww, out_frames, ch, to_rate);
        CHECK(st == want, "status %d, wanted %d (refusal %d)", (int)st, (int)want, g_refusals);
        ++g_refusals;
    };
    auto none = [](rh_wide_src *, uint64_t *) {};
    CHECK(call(good, 2, words, 100, 2, 48000, nullptr) == RH_ERR_INVALID, "dst NULL"); ++g_refusals;
    CHECK(call(nullptr, 2, words, 100) == RH_ERR_INVALID, "srcs NULL"); ++g_refusals;
    CHECK(call(good, 2, nullptr, 100) == RH_ERR_INVALID, "clips NULL"); ++g_refusals;
    refused(RH_ERR_INVALID, none, 100, 0);
    refused(RH_ERR_INVALID, none, 100, 2, 0);
    for (int k = 0; k < 2; ++k) {  // the shared fields, of the plain source and of the clip
        refused(RH_ERR_INVALID, [&](rh_wide_src *s, uint64_t *) { s[k].data = nullptr; });
        refused(RH_ERR_INVALID, [&](rh_wide_src *s, uint64_t *) { s[k].channels = 0; });
        refused(RH_ERR_INVALID, [&](rh_wide_src *s, uint64_t *) { s[k].from_rate = 0; });
        refused(RH_ERR_INVALID, [&](rh_wide_src *s, uint64_t *) { s[k].frames = 101; });
        refused(RH_ERR_UNSUPPORTED, [&](rh_wide_src *s, uint64_t *) { s[k].from_rate = 4294967291u; });  // F T beyond 32 bits
    }
    refused(RH_ERR_INVALID, [](rh_wide_src *s, uint64_t *) { s[0].phase = 160; });
    // the words
    refused(RH_ERR_INVALID, [](rh_wide_src *, uint64_t *x) { x[0] = 3; });                  // kind
    refused(RH_ERR_INVALID, [](rh_wide_src *, uint64_t *x) { x[4] = 4; });                  // flags above 3
    refused(RH_ERR_INVALID, [](rh_wide_src *, uint64_t *x) { x[4] = 2; });                  // the fade-out without a take
    refused(RH_ERR_INVALID, [](rh_wide_src *, uint64_t *x) { x[0] = kRuleC; });             // rule C with a take
    refused(RH_ERR_INVALID, [&](rh_wide_src *, uint64_t *x) { x[2] = 3002, x[1] += 1000; }); // more samples than the duration admits
    refused(RH_ERR_INVALID, [](rh_wide_src *, uint64_t *x) { x[5] = 1u << 30; });           // done > total
    refused(RH_ERR_INVALID, [&](rh_wide_src *s, uint64_t *x) { x[5] = 4200, s[1].frames = 100; });  // frames > total - done
    refused(RH_ERR_UNSUPPORTED, [](rh_wide_src *, uint64_t *x) { x[1] += 1; });             // Ls odd
    refused(RH_ERR_UNSUPPORTED, [](rh_wide_src *s, uint64_t *x) { s[1].channels = 6, x[1] = 60000, x[2] = 600, x[3] = 1000000000; });  // Ls > 32768 with 6 channels
    refused(RH_ERR_UNSUPPORTED, [](rh_wide_src *, uint64_t *x) { x[1] = (1ull << 62) + 2; });
    refused(RH_ERR_UNSUPPORTED, [](rh_wide_src *s, uint64_t *x) { s[1].from_rate = 1000000000u, x[2] = 0, x[1] = 4000; });  // dps == 0 with a take
    refused(RH_ERR_UNSUPPORTED, none, 0x80000000ull);
    refused(RH_ERR_UNSUPPORTED, [](rh_wide_src *s, uint64_t *) { s[1].frames = 0; }, 0x7fffffffull);  // the plain source: out_frames > (2^32 - 1 - T) / F
    // an empty clip has no frame to reach
    refused(RH_ERR_INVALID, [](rh_wide_src *s, uint64_t *x) { x[1] = 0, x[2] = 0, s[1].frames = 1; });
    // the plan's own refusals
    uint64_t p[RH_CLIP_WORDS];
    CHECK(clip_plan(nullptr, 10, 2, rate, 0, 0, 0, 0) == RH_ERR_INVALID, "words NULL"); ++g_refusals;
    CHECK(clip_plan(p, 10, 0, rate, 0, 0, 0, 0) == RH_ERR_INVALID && clip_plan(p, 10, 2, 0, 0, 0, 0, 0) == RH_ERR_INVALID, "channels, rate"); ++g_refusals;
    CHECK(clip_plan(p, 10, 2, rate, 0, 0, 0, 4) == RH_ERR_INVALID && clip_plan(p, 10, 2, rate, 0, 0, 0, 2) == RH_ERR_INVALID, "flags"); ++g_refusals;
    CHECK(clip_plan(p, 1000, 2, rate, 999, 0, 0, 0) == RH_ERR_UNSUPPORTED && clip_plan(p, 1000, 2, rate, 1, 0, 0, 0) == RH_ERR_UNSUPPORTED, "a span inside the sound"); ++g_refusals;
    CHECK(clip_plan(p, 1001, 2, rate, 0, 0, 0, 0) == RH_ERR_UNSUPPORTED && clip_plan(p, 60000, 6, rate, 60000, 0, 0, 0) == RH_ERR_UNSUPPORTED, "a cut frame"); ++g_refusals;
    CHECK(clip_plan(p, 60000, 6, rate, 0, 0, 0, 0) == RH_OK && p[0] == kRuleC, "six channels under rule C are one chain"); ++g_refusals;
    CHECK(clip_plan(p, 1000, 2, 1000000000u, 0, ~0ull, 0, 0) == RH_ERR_UNSUPPORTED, "a delay beyond 2^62 samples"); ++g_refusals;
    CHECK(clip_advance(nullptr, 2, rate, 48000, 1) == RH_ERR_INVALID && clip_advance(w, 2, 0, 48000, 1) == RH_ERR_INVALID && clip_advance(w, 0, rate, 48000, 1) == RH_ERR_INVALID, "advance"); ++g_refusals;
    uint64_t plain[RH_CLIP_WORDS] = {0, 9, 9, 9, 9, 9, 9};
    CHECK(clip_advance(plain, 0, 0, 0, 5) == RH_OK && plain[5] == 9, "a plain source's words are left alone");
}

// The exact 32-bit bounds of include/rodio_hip.h: the last value that passes and the first that does not.
static void test_bounds() {
    rh_wide_src x{};
    x.data = kSound, x.channels = 2, x.gain = 1.0f;
    Desc d;
    auto st_of = [&](uint64_t *w, uint32_t from, uint32_t to, uint64_t frames) {
        x.from_rate = from, x.frames = frames;
        return describe(x, w, 2, to, 0x7fffffffull, &d);
    };
    {  // rule C: r0 + (frames - 1) F <= 2^32 - 1.  F = 65521, T = 65519, done = 1: r0 = 2
        uint64_t w[RH_CLIP_WORDS] = {kRuleC, 0, 1ull << 40, 0, 0, 1, 0};
        const uint64_t ok = (0xffffffffull - 2) / 65521 + 1;
        CHECK(st_of(w, 65521, 65519, ok) == RH_OK, "rule C, the last block that fits"); ++g_bounds;
        CHECK(st_of(w, 65521, 65519, ok + 1) == RH_ERR_UNSUPPORTED, "rule C, the first that does not"); ++g_bounds;
    }
    {  // rule C: the samples the block spans, (floor(p_last / T) + 2) ch <= 2^32 - 1.  8 -> 1 Hz: F = 8, T = 1, every output frame 8 input frames
        uint64_t w[RH_CLIP_WORDS] = {kRuleC, 0, 1ull << 40, 0, 0, 0, 0};
        // (frames - 1) * 8 + 2 <= (2^32 - 1) / 2 = 2147483647  ->  frames - 1 <= 268435455
        CHECK(st_of(w, 8, 1, 268435456) == RH_OK, "rule C samples, the last"); ++g_bounds;
        CHECK(st_of(w, 8, 1, 268435457) == RH_ERR_UNSUPPORTED, "rule C samples, the first beyond"); ++g_bounds;
    }
    {  // rule G: M F <= 2^32 - 1.  1 -> T Hz mono... c = 16384 stereo frames, F = 1: M = 16383 T + 1
        uint64_t w[RH_CLIP_WORDS] = {kRuleG, 0, 1ull << 20, 0, 0, 0, 0};
        CHECK(st_of(w, 1, 262159, 10) == RH_OK, "rule G, M F inside"); ++g_bounds;  // M = 16383 * 262159 + 1 = 4294950898
        CHECK(st_of(w, 1, 262161, 10) == RH_ERR_UNSUPPORTED, "rule G, M F beyond"); ++g_bounds;  // 16383 * 262161 + 1 = 4294983664
    }
    {  // rule G: j0 + frames - 1 <= 2^32 - 1 with M next to 2^32: done = M - 1
        uint64_t w[RH_CLIP_WORDS] = {kRuleG, 0, 1ull << 20, 0, 0, 4294950897ull, 0};
        CHECK(st_of(w, 1, 262159, 16399) == RH_OK, "rule G, x_last == 2^32 - 1"); ++g_bounds;
        CHECK(st_of(w, 1, 262159, 16400) == RH_ERR_UNSUPPORTED, "rule G, x_last == 2^32"); ++g_bounds;
    }
    {  // rule G: the samples the block's chains span.  8 -> 1 Hz: M = 2048 a chain of 32768 samples; 2^31 - 1 frames span 1048576 chains = 2^35 samples
        uint64_t w[RH_CLIP_WORDS] = {kRuleG, 0, 1ull << 40, 0, 0, 0, 0};
        CHECK(st_of(w, 8, 1, 2048ull * 131071) == RH_OK, "rule G samples, 131071 chains"); ++g_bounds;        // 131071 * 32768 = 2^32 - 32768
        CHECK(st_of(w, 8, 1, 2048ull * 131071 + 1) == RH_ERR_UNSUPPORTED, "rule G samples, one frame more"); ++g_bounds;
    }
    {  // a PLAIN source is read as rh_wide_mix_block reads it: its positions phase + j F are bounded, frame * channels is not, and the
       // sample index of a tap is formed in 64 bits -- no refusal, no wrap
        uint64_t w[RH_CLIP_WORDS] = {0};
        x.channels = 8, x.last = 0xffffffffu;
        CHECK(st_of(w, 48000, 48000, (1ull << 29) + 10) == RH_OK, "F == T, 8 channels, more than 2^29 frames");
        Taps t = locate(d, (1u << 29) + 5u);
        CHECK(t.ia == (1u << 29) + 5u && !t.lerp && tap_sample(d, t.ia, 7) == (1ull << 32) + 47, "8 channels: sample %" PRIu64, tap_sample(d, t.ia, 7)); ++g_bounds;
        CHECK(tap_sample(d, (1u << 29) - 1u, 7) == 0xffffffffull, "the last sample inside 32 bits"); ++g_bounds;
        x.channels = 2;
        CHECK(st_of(w, 96000, 48000, (1ull << 30) + 10) == RH_OK, "96 -> 48 kHz stereo, more than 2^30 frames");
        t = locate(d, (1u << 30) + 3u);
        CHECK(t.ia == (1u << 31) + 6u && tap_sample(d, t.ia, 1) + d.ch == (1ull << 32) + 15, "stereo: sample %" PRIu64, tap_sample(d, t.ia, 1)); ++g_bounds;
        x.last = 0;
    }
    {  // the fade's arithmetic: 32 bits while (samples) * dps + 999999 fits, 64 beyond; never refused
        const uint64_t dps = ns_per_sample(2, 44100);
        uint64_t w[RH_CLIP_WORDS] = {kRuleG, 0, 1ull << 30, (1ull << 30) * dps, 3, 0, 0};
        CHECK(st_of(w, 44100, 48000, 17833 * 11) == RH_OK && d.fade == kFade32, "eleven chains fade in 32 bits"); ++g_bounds;  // 11 * 32768 * 11337 = 4.09e9
        CHECK(st_of(w, 44100, 48000, 17833 * 11 + 1) == RH_OK && d.fade == kFade64, "twelve in 64"); ++g_bounds;
        const float R = fade_ms(d, 300000u);
        CHECK(R == (float)((w[3] - 300000ull * dps) / 1000000ull), "the 64-bit fade"); ++g_fade64;
        w[3] = (1ull << 33) * 1000000ull + 5, w[2] = 1000;  // more than 2^32 ms remain
        CHECK(st_of(w, 44100, 48000, 10) == RH_OK && d.fade == kFade64 && fade_ms(d, 3u) == (float)((w[3] - 3 * dps) / 1000000ull), "milliseconds beyond 32 bits"); ++g_bounds;
    }
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "plan") == 0 && argc == 9) {
        uint64_t w[RH_CLIP_WORDS] = {0};
        const rh_status st = clip_plan(w, std::strtoull(argv[2], nullptr, 10), (uint32_t)std::strtoul(argv[3], nullptr, 10), (uint32_t)std::strtoul(argv[4], nullptr, 10),
                                       std::strtoull(argv[5], nullptr, 10), std::strtoull(argv[6], nullptr, 10), std::strtoull(argv[7], nullptr, 10), (uint32_t)std::strtoul(argv[8], nullptr, 10));
        std::printf("%d", (int)st);
        for (int k = 0; k < RH_CLIP_WORDS; ++k) std::printf(" %" PRIu64, w[k]);
        std::printf("\n");
        return 0;
    }
    if (argc >= 2 && std::strcmp(argv[1], "advance") == 0 && argc == 2 + RH_CLIP_WORDS + 4) {
        uint64_t w[RH_CLIP_WORDS];
        for (int k = 0; k < RH_CLIP_WORDS; ++k) w[k] = std::strtoull(argv[2 + k], nullptr, 10);
        const char *const *a = argv + 2 + RH_CLIP_WORDS;
        const rh_status st = clip_advance(w, (uint32_t)std::strtoul(a[0], nullptr, 10), (uint32_t)std::strtoul(a[1], nullptr, 10), (uint32_t)std::strtoul(a[2], nullptr, 10), std::strtoull(a[3], nullptr, 10));
        std::printf("%d", (int)st);
        for (int k = 0; k < RH_CLIP_WORDS; ++k) std::printf(" %" PRIu64, w[k]);
        std::printf("\n");
        return 0;
    }
    if (argc >= 2 && std::strcmp(argv[1], "locate") == 0 && argc >= 2 + RH_CLIP_WORDS + 6) {
        uint64_t w[RH_CLIP_WORDS];
        for (int k = 0; k < RH_CLIP_WORDS; ++k) w[k] = std::strtoull(argv[2 + k], nullptr, 10);
        const char *const *a = argv + 2 + RH_CLIP_WORDS;
        rh_wide_src x{};
        x.data = kSound, x.channels = (uint32_t)std::strtoul(a[0], nullptr, 10), x.from_rate = (uint32_t)std::strtoul(a[1], nullptr, 10), x.frames = std::strtoull(a[4], nullptr, 10), x.gain = 1.0f;
        Desc d;
        const rh_status st = describe(x, w, (uint32_t)std::strtoul(a[2], nullptr, 10), (uint32_t)std::strtoul(a[3], nullptr, 10), std::strtoull(a[5], nullptr, 10), &d);
        std::printf("%d\n", (int)st);
        if (st != RH_OK) return 0;
        std::printf("%u %u %u %u %u %u %" PRIu64 " %" PRIu64 "\n", d.fade, d.x0, d.M, d.c, d.klast, d.zrel, (uint64_t)(d.data - kSound), d.ms0);
        for (int k = 2 + RH_CLIP_WORDS + 6; k < argc; ++k) {
            const Taps t = locate(d, (uint32_t)std::strtoul(argv[k], nullptr, 10));
            const uint64_t sa = tap_sample(d, t.ia, 0);
            const float R = (d.fade != kNoFade && sa >= d.zrel) ? fade_ms(d, (uint32_t)(sa - d.zrel)) : 0.0f;
            uint32_t rb;
            std::memcpy(&rb, &R, 4);
            std::printf("%u %d %u %u\n", t.ia, t.lerp ? 1 : 0, t.num, rb);
        }
        return 0;
    }
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const int clips = argc > 2 ? std::atoi(argv[2]) : 400;
    std::mt19937_64 rng(seed);
    test_divs(rng);
    test_clips(rng, clips);
    test_shifts(rng);
    test_refusals();
    test_bounds();
    std::printf("failures %d divs %d clips %d blocks %d taps %d faded %d delay_taps %d refusals %d bounds %d fade64 %d\n", g_failures, g_divs, g_clips, g_blocks, g_taps, g_faded, g_delay_taps,
                g_refusals, g_bounds, g_fade64);
    return g_failures ? 1 : 0;
}
