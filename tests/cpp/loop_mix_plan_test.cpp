// loop_mix_plan_test.cpp -- the host decisions of rh_loop_mix_block (rodio_amd/csrc/rh_loop_mix_plan.h) without a GPU: the reciprocals
// divide exactly, a chain's output count is counted a second way (by walking the converter), locate() -- the function the kernel runs per
// source and sample -- names the taps a chain-by-chain walk of the unrolled stream names, under both rules, for any cursor and for plain
// sources; rh_loop_advance over any cut is the walk's cursor; rh_loop_plan's branches; every refusal of the header; the 32-bit bound at
// its edge and one past it; the launch split at 32 / 33 / 40 sources.
// TEST INFRASTRUCTURE: plain g++, no HIP, no library.  Pointers are never followed.
//
//     loop_mix_plan_test [seed [random cases]]
//     loop_mix_plan_test plan n_samples channels span_len              -> status L c rule chain_start chain_out
//     loop_mix_plan_test advance L c rule start out from to out_frames -> status L c rule chain_start chain_out
//     loop_mix_plan_test locate L c rule start out ch from to_ch to frames out_frames m ..
//                          -> status, then "x0 P M" of describe(), then per output frame m of the block "ia ib lerp num" of locate()
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "rh_loop_mix_plan.h"

using namespace rh::loopmix;

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

static float *out_ptr() { return reinterpret_cast<float *>((uintptr_t)0x100000000ull); }
static const float *in_ptr(uint64_t k) { return reinterpret_cast<const float *>((uintptr_t)(0x800000000000ull + 0x100000ull * k)); }
static rh_wide_src src(uint64_t k, uint32_t ch, uint32_t rate, uint64_t frames, uint32_t phase = 0, uint32_t last = 0xffffffffu) {
    return rh_wide_src{in_ptr(k), ch, rate, phase, frames, last, 1.0f};
}

// The converter of one chain of n frames, walked frame by frame: output frame j of it (false: the chain is over in front of j).
struct Out {
    uint64_t i, num;
    bool lerp;
};
static bool chain_frame(uint64_t n, uint64_t F, uint64_t T, uint64_t j, Out *o) {
    const uint64_t i = j * F / T, num = j * F % T;
    if (i >= n) return false;
    if (F == T) {
        *o = Out{i, 0, false};
        return true;
    }
    // the first output frame that lands on the last frame is verbatim and ends the chain: one behind it does not exist
    if (i + 1 == n && j > 0 && (j - 1) * F / T == i) return false;
    *o = Out{i, num, i + 1 < n};
    return true;
}
static uint64_t walk_chain(uint64_t n, uint64_t F, uint64_t T) {
    uint64_t j = 0;
    Out o;
    while (chain_frame(n, F, T, j, &o)) ++j;
    return j;
}

// The stream of a loop from its cursor on, chain by chain: what the walk names for the next `frames` output frames, and the cursor behind them.
struct Tap {
    uint64_t ia, ib, num;
    bool lerp;
};
static std::vector<Tap> walk_loop(uint64_t *w, uint64_t F, uint64_t T, uint64_t frames) {
    std::vector<Tap> t;
    t.reserve(frames);
    uint64_t L = w[0], c = w[1], rule = w[2], start = w[3], out = w[4];
    while (true) {
        const uint64_t n = rule == 0 ? (c < L - start ? c : L - start) : c;
        Out o;
        for (; chain_frame(n, F, T, out, &o); ++out) {
            if (t.size() == frames) {
                w[3] = start, w[4] = out;
                return t;
            }
            t.push_back(Tap{(start + o.i) % L, (start + o.i + 1) % L, o.num, o.lerp});
        }
        out = 0;
        start = (start + n) % L;
    }
}

static int g_divs = 0, g_spans = 0, g_located = 0, g_cuts = 0, g_plans = 0, g_refusals = 0, g_bounds = 0, g_launches = 0;

static void test_divs(std::mt19937_64 &rng) {
    const uint64_t ds[] = {1, 2, 3, 5, 7, 160, 147, 32768, 65535, 65536, 65537, (1ull << 24) + 1, (1ull << 31) - 1, 1ull << 31, (1ull << 31) + 1, 0xfffffffeull, 0xffffffffull};
    std::vector<uint64_t> all(ds, ds + sizeof(ds) / sizeof(ds[0]));
    for (int k = 0; k < 300; ++k) all.push_back(1 + rng() % (1ull << (1 + rng() % 32)));
    for (uint64_t d : all) {
        const Div v = make_div(d);
        std::vector<uint64_t> xs = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 0x7fffffffull, 0x80000000ull, 0xfffffffeull, 0xffffffffull};
        for (int k = 0; k < 200; ++k) xs.push_back(rng());
        for (uint64_t k = 1; k < 40; ++k) xs.push_back((0xffffffffull / d) * d - 1 + k % 3), xs.push_back(k * d), xs.push_back(k * d - 1);
        for (uint64_t x64 : xs) {
            const uint32_t x = (uint32_t)x64;
            EXPECT(div_u32(x, v) == x / (uint32_t)d, "%u / %llu", x, (unsigned long long)d);
            ++g_divs;
        }
    }
    for (uint64_t x : {0ull, 1ull, 0x7fffffffull, 0x80000000ull, 0xffffffffull}) EXPECT(div_u32((uint32_t)x, kDivZero) == 0, "the zero quotient of %llu", (unsigned long long)x);
}

static void test_spans() {
    const uint64_t rates[][2] = {{147, 160}, {160, 147}, {1, 1}, {1, 6}, {6, 1}, {10, 1}, {3, 16777259}, {2, 3}};
    for (auto &r : rates)
        for (uint64_t n = 0; n <= (r[1] > 1000 ? 2 : 40); ++n) {  // (the walk of a chain is T / F steps a frame)
            EXPECT(span_out(n, r[0], r[1]) == walk_chain(n, r[0], r[1]), "n %llu F %llu T %llu", (unsigned long long)n, (unsigned long long)r[0], (unsigned long long)r[1]);
            ++g_spans;
        }
}

static void expect_located(const rh_wide_src &x, uint64_t *w, uint32_t to_rate, uint64_t out_frames, const char *what) {
    Desc d;
    const rh_status st = describe(x, w, 2, to_rate, out_frames, &d);
    EXPECT(st == RH_OK, "%s: status %d", what, (int)st);
    if (st != RH_OK) return;
    const uint64_t g = std::gcd(x.from_rate, to_rate), F = x.from_rate / g, T = to_rate / g;
    uint64_t cur[5] = {w[0], w[1], w[2], w[3], w[4]};
    const std::vector<Tap> want = walk_loop(cur, F, T, x.frames);
    for (uint64_t m = 0; m < x.frames; ++m) {
        const Taps t = locate(d, (uint32_t)m);
        const bool same = t.ia == want[m].ia && t.lerp == want[m].lerp && (!t.lerp || (t.ib == want[m].ib && t.num == want[m].num));
        EXPECT(same && t.ia < w[0] && t.ib < w[0], "%s: L %llu c %llu rule %llu cursor %llu %llu F %llu T %llu frame %llu: %u %u %d %u, walked %llu %llu %d %llu", what,
               (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2], (unsigned long long)w[3], (unsigned long long)w[4], (unsigned long long)F,
               (unsigned long long)T, (unsigned long long)m, t.ia, t.ib, (int)t.lerp, t.num, (unsigned long long)want[m].ia, (unsigned long long)want[m].ib, (int)want[m].lerp,
               (unsigned long long)want[m].num);
        if (!same) return;
    }
    ++g_located;
}

static void test_locate(std::mt19937_64 &rng, int cases) {
    const uint32_t rates[][2] = {{44100, 48000}, {48000, 44100}, {48000, 48000}, {8000, 48000}, {48000, 8000}, {3, 16777259}, {96000, 44100}};
    const uint64_t shapes[][3] = {{1, 1, 0}, {5, 5, 0}, {10, 4, 0}, {9, 4, 0}, {3, 7, 0}, {4, 4, 1}, {5, 4, 1}, {10, 4, 1}, {7, 1, 1}, {20000, 16384, 1}, {20000, 16384, 0}};
    for (auto &r : rates)
        for (auto &s : shapes) {
            uint64_t w[5] = {s[0], s[1], s[2], 0, 0};
            const uint64_t frames = s[0] > 100 ? 70000 : 300;
            if (s[1] > 100 && r[1] > (1u << 24)) {  // a chain of 16384 frames at T > 2^24 emits more than 2^32 frames: refused, not walked
                Desc d;
                EXPECT(describe(src(0, 2, r[0], frames), w, 2, r[1], frames, &d) == RH_ERR_UNSUPPORTED, "a chain whose positions leave 32 bits");
                continue;
            }
            expect_located(src(0, 2, r[0], frames), w, r[1], frames, "fresh");
            // ... and from the cursor behind every cut of a stream into three blocks: the cursor is the walk's, the taps continue
            uint64_t a[5] = {s[0], s[1], s[2], 0, 0}, b[5] = {s[0], s[1], s[2], 0, 0};
            const uint64_t g = std::gcd(r[0], r[1]);
            for (uint64_t n : {(uint64_t)(1 + rng() % 50), (uint64_t)(rng() % 3), (uint64_t)(1 + rng() % 40000)}) {
                EXPECT(loop_advance(a, r[0], r[1], n) == RH_OK, "advance");
                (void)walk_loop(b, r[0] / g, r[1] / g, n);
                EXPECT(std::memcmp(a, b, sizeof(a)) == 0, "L %llu c %llu rule %llu by %llu: cursor %llu %llu, walked %llu %llu", (unsigned long long)s[0], (unsigned long long)s[1],
                       (unsigned long long)s[2], (unsigned long long)n, (unsigned long long)a[3], (unsigned long long)a[4], (unsigned long long)b[3], (unsigned long long)b[4]);
                ++g_cuts;
                expect_located(src(0, 2, r[0], 200), a, r[1], 200, "behind a cut");
            }
        }
    for (int k = 0; k < cases; ++k) {
        const auto &r = rates[rng() % 7];
        const uint64_t rule = rng() % 2, c = 1 + rng() % 12, L = rule ? c + rng() % 20 : 1 + rng() % 30;
        uint64_t w[5] = {L, c, rule, 0, 0};
        EXPECT(loop_advance(w, r[0], r[1], rng() % 100000) == RH_OK, "advance");
        expect_located(src(0, 1 + rng() % 6, r[0], 1 + rng() % 400), w, r[1], 400, "random");
    }
    // a source that is not a loop: k_wide_mix's positions
    for (auto &r : rates) {
        const uint64_t g = std::gcd(r[0], r[1]), F = r[0] / g, T = r[1] / g;
        uint64_t w[5] = {0, 99, 99, 99, 99};  // (the other words are ignored)
        const uint32_t phase = (uint32_t)(rng() % T), last = 57;
        const uint64_t frames = 60 * T / F < 300 ? 60 * T / F : 300;
        Desc d;
        EXPECT(describe(src(0, 2, r[0], frames, phase, last), w, 2, r[1], 400, &d) == RH_OK, "plain");
        for (uint64_t m = 0; m < frames; ++m) {
            const uint64_t p = phase + m * F;
            const Taps t = locate(d, (uint32_t)m);
            const bool lerp = F != T && p / T < last;
            EXPECT(t.ia == p / T && t.lerp == lerp && (!lerp || (t.ib == p / T + 1 && t.num == p % T)), "plain F %llu T %llu frame %llu", (unsigned long long)F, (unsigned long long)T,
                   (unsigned long long)m);
        }
        ++g_located;
    }
}

static void test_plans() {
    struct {
        uint64_t n, ch, span;
        rh_status st;
        uint64_t L, c, rule;
    } cases[] = {
        {20000, 2, 0, RH_OK, 10000, 10000, 0},      {40000, 2, 0, RH_OK, 20000, 16384, 0},      {32768, 2, 0, RH_OK, 16384, 16384, 0},  {32770, 2, 0, RH_OK, 16385, 16384, 0},
        {20000, 2, 20000, RH_OK, 10000, 10000, 0},  {40000, 2, 40000, RH_OK, 20000, 16384, 1},  {32768, 1, 32768, RH_OK, 32768, 32768, 0}, {32769, 1, 32769, RH_OK, 32769, 32768, 1},
        {40000, 2, 1152, RH_OK, 20000, 576, 0},     {1000, 2, 1152, RH_OK, 500, 500, 0},        {40000, 2, 32768, RH_OK, 20000, 16384, 0}, {88200, 2, 88200, RH_OK, 44100, 16384, 1},
        {39999, 2, 0, RH_ERR_UNSUPPORTED, 0, 0, 0}, {60000, 6, 0, RH_ERR_UNSUPPORTED, 0, 0, 0}, {60000, 6, 60000, RH_ERR_UNSUPPORTED, 0, 0, 0}, {30000, 6, 0, RH_OK, 5000, 5000, 0},
        {60000, 3, 60000, RH_ERR_UNSUPPORTED, 0, 0, 0}, {60000, 5, 0, RH_ERR_UNSUPPORTED, 0, 0, 0}, {70000, 7, 0, RH_ERR_UNSUPPORTED, 0, 0, 0}, {60000, 4, 60000, RH_OK, 15000, 8192, 1},
        {40000, 2, 1001, RH_ERR_UNSUPPORTED, 0, 0, 0}, {40000, 2, 50000, RH_ERR_UNSUPPORTED, 0, 0, 0}, {40000, 2, 32769, RH_ERR_UNSUPPORTED, 0, 0, 0}, {0, 2, 0, RH_ERR_INVALID, 0, 0, 0},
        {100, 0, 0, RH_ERR_INVALID, 0, 0, 0},
    };
    for (auto &p : cases) {
        uint64_t w[5] = {9, 9, 9, 9, 9};
        const rh_status st = loop_plan(p.n, (uint32_t)p.ch, p.span, w);
        EXPECT(st == p.st, "plan %llu %llu %llu: %d", (unsigned long long)p.n, (unsigned long long)p.ch, (unsigned long long)p.span, (int)st);
        if (st == RH_OK)
            EXPECT(w[0] == p.L && w[1] == p.c && w[2] == p.rule && w[3] == 0 && w[4] == 0, "plan %llu %llu %llu: %llu %llu %llu", (unsigned long long)p.n, (unsigned long long)p.ch,
                   (unsigned long long)p.span, (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2]);
        else
            EXPECT(w[0] == 9, "a refused plan writes nothing");
        ++g_plans;
    }
    EXPECT(loop_plan(100, 2, 0, nullptr) == RH_ERR_INVALID, "no words");
    ++g_plans;
}

struct Call {
    uint32_t channels = 2, to_rate = 48000;
    uint64_t out_frames = 1000;
    float *dst = out_ptr();
    std::vector<rh_wide_src> srcs;
    std::vector<uint64_t> words;
    void add(const rh_wide_src &x, uint64_t L = 0, uint64_t c = 0, uint64_t rule = 0, uint64_t start = 0, uint64_t out = 0) {
        srcs.push_back(x);
        words.insert(words.end(), {L, c, rule, start, out});
    }
    rh_status check(bool with_words = true) const {
        return rh::loopmix::check(dst, channels, to_rate, out_frames, srcs.empty() ? nullptr : srcs.data(), (uint32_t)srcs.size(), with_words ? words.data() : nullptr);
    }
};
#define REFUSED(call, status, what)                                       \
    do {                                                                  \
        const rh_status st_ = (call);                                     \
        EXPECT(st_ == (status), "%s: status %d", what, (int)st_);         \
        ++g_refusals;                                                     \
    } while (0)

static void test_refusals() {
    auto one = [](const rh_wide_src &x, uint64_t L, uint64_t c, uint64_t rule, uint64_t start, uint64_t out) {
        Call k;
        k.add(src(1, 2, 44100, 1000, 0, 999));  // a plain source in front
        k.add(x, L, c, rule, start, out);
        return k;
    };
    const rh_wide_src ok = src(0, 2, 44100, 1000);
    EXPECT(one(ok, 10, 4, 0, 8, 1).check() == RH_OK && one(ok, 10, 4, 1, 9, 4).check() == RH_OK, "the calls the refusals are variations of");
    {  // the shared fields
        Call k = one(ok, 10, 4, 0, 0, 0);
        k.dst = nullptr;
        REFUSED(k.check(), RH_ERR_INVALID, "no dst");
        k = one(ok, 10, 4, 0, 0, 0), k.channels = 0;
        REFUSED(k.check(), RH_ERR_INVALID, "no channels");
        k = one(ok, 10, 4, 0, 0, 0), k.to_rate = 0;
        REFUSED(k.check(), RH_ERR_INVALID, "no rate");
        REFUSED(rh::loopmix::check(out_ptr(), 2, 48000, 10, nullptr, 1, k.words.data()), RH_ERR_INVALID, "no sources");
        REFUSED(one(ok, 10, 4, 0, 0, 0).check(false), RH_ERR_INVALID, "no words");
        k = one(ok, 10, 4, 0, 0, 0), k.out_frames = 0x80000000ull;
        REFUSED(k.check(), RH_ERR_UNSUPPORTED, "a block of 2^31 frames");
        rh_wide_src x = ok;
        x.data = nullptr;
        REFUSED(one(x, 10, 4, 0, 0, 0).check(), RH_ERR_INVALID, "a loop without data");
        x = ok, x.channels = 0;
        REFUSED(one(x, 10, 4, 0, 0, 0).check(), RH_ERR_INVALID, "a loop without channels");
        x = ok, x.from_rate = 0;
        REFUSED(one(x, 10, 4, 0, 0, 0).check(), RH_ERR_INVALID, "a loop without a rate");
        x = ok, x.frames = 1001;
        REFUSED(one(x, 10, 4, 0, 0, 0).check(), RH_ERR_INVALID, "a loop that reaches behind the block");
        x = ok, x.from_rate = 65537;
        k = one(x, 10, 4, 0, 0, 0), k.to_rate = 65539;
        REFUSED(k.check(), RH_ERR_UNSUPPORTED, "F T beyond 32 bits");
        x = ok, x.phase = 160;
        REFUSED(one(x, 0, 0, 0, 0, 0).check(), RH_ERR_INVALID, "a plain source's phase beyond T");
        EXPECT(one(x, 10, 4, 0, 0, 0).check() == RH_OK, "a loop's phase is not read");
        x = ok, x.frames = 0, x.data = nullptr, x.channels = 0;
        EXPECT(one(x, 10, 0, 7, 99, 99).check() == RH_OK, "a source with frames == 0 is not looked at");
    }
    REFUSED(one(ok, 10, 4, 2, 0, 0).check(), RH_ERR_INVALID, "rule 2");
    REFUSED(one(ok, 10, 0, 0, 0, 0).check(), RH_ERR_INVALID, "c == 0");
    REFUSED(one(ok, 20000, 16385, 0, 0, 0).check(), RH_ERR_INVALID, "c * channels > 32768");
    EXPECT(one(ok, 20000, 16384, 0, 0, 0).check() == RH_OK, "c * channels == 32768");
    REFUSED(one(ok, 3, 4, 1, 0, 0).check(), RH_ERR_INVALID, "rule 1 with L < c");
    EXPECT(one(ok, 3, 4, 0, 0, 0).check() == RH_OK, "rule 0 with L < c: one chain of L");
    REFUSED(one(ok, 10, 4, 0, 10, 0).check(), RH_ERR_INVALID, "chain_start == L");
    REFUSED(one(ok, 10, 4, 1, 10, 0).check(), RH_ERR_INVALID, "chain_start == L under rule 1");
    REFUSED(one(ok, 10, 4, 0, 5, 0).check(), RH_ERR_INVALID, "rule 0: chain_start not a multiple of c");
    // 44100 -> 48000: a chain of 4 emits 5 frames (0, 0.92, 1.84, 2.76 and, verbatim, 3.675), the tail of 2 emits 3
    EXPECT(span_out(4, 147, 160) == 5 && span_out(2, 147, 160) == 3, "the chains of the cursor bounds");
    REFUSED(one(ok, 10, 4, 0, 0, 5).check(), RH_ERR_INVALID, "chain_out == M(c)");
    EXPECT(one(ok, 10, 4, 0, 0, 4).check() == RH_OK, "chain_out == M(c) - 1");
    REFUSED(one(ok, 10, 4, 0, 8, 3).check(), RH_ERR_INVALID, "chain_out == M(tail)");
    EXPECT(one(ok, 10, 4, 0, 8, 2).check() == RH_OK, "chain_out == M(tail) - 1");
    REFUSED(one(ok, 10, 4, 1, 8, 5).check(), RH_ERR_INVALID, "rule 1: chain_out == M(c)");
    EXPECT(one(ok, 10, 4, 1, 8, 4).check() == RH_OK, "rule 1 has no tail chain");
    uint64_t w[5] = {10, 4, 0, 5, 0};
    REFUSED(loop_advance(w, 44100, 48000, 10), RH_ERR_INVALID, "advance: a cursor outside its bounds");
    REFUSED(loop_advance(nullptr, 44100, 48000, 10), RH_ERR_INVALID, "advance: no words");
    w[3] = 4;
    REFUSED(loop_advance(w, 0, 48000, 10), RH_ERR_INVALID, "advance: no rate");
    w[0] = 0, w[1] = 77;
    EXPECT(loop_advance(w, 44100, 48000, 10) == RH_OK && w[1] == 77 && w[3] == 4, "advance leaves a plain source's words");
}

// The 32-bit bound, term by term, at its edge and one past it.
static void test_bounds() {
    auto st = [](uint32_t from, uint32_t to, uint64_t frames, uint64_t out_frames, uint64_t L, uint64_t c, uint64_t rule, uint64_t start, uint64_t out) {
        Call k;
        k.to_rate = to, k.out_frames = out_frames;
        k.add(src(0, 1, from, frames), L, c, rule, start, out);
        return k.check();
    };
    auto edge = [&](rh_status at, rh_status past, const char *what) {
        EXPECT(at == RH_OK && past == RH_ERR_UNSUPPORTED, "%s: %d at the edge, %d past it", what, (int)at, (int)past);
        ++g_bounds;
    };
    edge(st(1, 1, 10, 10, 1ull << 31, 4, 1, 0, 0), st(1, 1, 10, 10, (1ull << 31) + 1, 4, 1, 0, 0), "L <= 2^31");
    // M(c) F <= 2^32 - 1.  F = 1: a chain of 2 frames emits T + 1
    EXPECT(span_out(2, 1, 0xfffffffeull) == 0xffffffffull, "the chain of the chain bound");
    edge(st(1, 0xfffffffeu, 10, 10, 10, 2, 1, 0, 0), st(1, 0xffffffffu, 10, 10, 10, 2, 1, 0, 0), "M(c) F <= 2^32 - 1");
    edge(st(1, 0xfffffffeu, 10, 10, 2, 2, 0, 0, 0), st(1, 0xfffffffeu, 10, 10, 2, 3, 0, 0, 0), "M(c) F <= 2^32 - 1, by the chain");
    // rule 0: P <= 2^32 - 1.  1 -> 4 Hz, c = 2: M = 5, P = 5 L / 2; 5 * 858993459 = 2^32 - 1
    EXPECT(span_out(2, 1, 4) == 5, "the chain of the pass bound");
    edge(st(1, 4, 10, 10, 1717986918, 2, 0, 0, 0), st(1, 4, 10, 10, 1717986920, 2, 0, 0, 0), "rule 0: P <= 2^32 - 1");
    // rule 0: offset + frames - 1 <= 2^32 - 1.  The cursor on the pass's last output frame: offset = P - 1 = 2^32 - 2
    edge(st(1, 4, 2, 10, 1717986918, 2, 0, 1717986916, 4), st(1, 4, 3, 10, 1717986918, 2, 0, 1717986916, 4), "rule 0: offset + frames - 1 <= 2^32 - 1");
    // rule 1: chain_out + frames - 1 <= 2^32 - 1.  M = 2^32 - 1, the cursor on the chain's last output frame
    edge(st(1, 0xfffffffeu, 2, 10, 10, 2, 1, 0, 0xfffffffeull), st(1, 0xfffffffeu, 3, 10, 10, 2, 1, 0, 0xfffffffeull), "rule 1: chain_out + frames - 1 <= 2^32 - 1");
    // rule 1: chain_start + floor((chain_out + frames - 1) / M) c <= 2^32 - 1.  2 -> 1 Hz, c = 32768: M = 16384; the longest block is in chain 131071,
    // 131071 * 32768 = 2^32 - 32768
    EXPECT(span_out(32768, 2, 1) == 16384, "the chain of the chain-start bound");
    edge(st(2, 1, 0x7fffffff, 0x7fffffff, 1ull << 31, 32768, 1, 0x7fff, 0), st(2, 1, 0x7fffffff, 0x7fffffff, 1ull << 31, 32768, 1, 0x8000, 0), "rule 1: chain_start + k c <= 2^32 - 1");
    // ... and at those edges the positions are still the walk's: nothing wraps at 2^32 - 1
    {
        uint64_t w0[5] = {1717986918, 2, 0, 1717986916, 4}, w1[5] = {10, 2, 1, 0, 0xfffffffeull};
        expect_located(src(0, 1, 1, 2), w0, 4, 10, "rule 0 at the edge");
        expect_located(src(0, 1, 1, 2), w1, 0xfffffffeu, 10, "rule 1 at the edge");
        uint64_t w2[5] = {1ull << 31, 32768, 1, 0x7fff, 0};
        Desc d;
        EXPECT(describe(src(0, 1, 2, 0x7fffffff), w2, 1, 1, 0x7fffffff, &d) == RH_OK, "the longest block");
        for (uint64_t m : {0x7ffffffeull, 0x7ffffffeull - 16384, 0x7ffffffeull - 8191, 65536ull * 16384 - 1, 65536ull * 16384}) {
            const uint64_t k = m / 16384, j = m % 16384, base = (0x7fff + k * 32768) % (1ull << 31), i = 2 * j;  // 2 -> 1 Hz: every output frame on an input frame
            const Taps t = locate(d, (uint32_t)m);
            EXPECT(t.ia == (base + i) % (1ull << 31) && t.lerp == (i + 1 < 32768) && t.ib == (base + i + 1) % (1ull << 31) && t.num == 0, "frame %llu of the longest block", (unsigned long long)m);
        }
        ++g_located;
    }
    // a plain source: rh_player_mix_block's answer, out_frames <= (2^32 - 1 - T) / F
    {
        Call k;
        k.to_rate = 3, k.out_frames = (0xffffffffull - 3) / 16777259;
        k.add(src(0, 1, 16777259, 10));
        const rh_status at = k.check();
        k.out_frames += 1;
        edge(at, k.check(), "a plain source: out_frames <= (2^32 - 1 - T) / F");
    }
}

static void test_launches() {
    for (uint32_t live : {0u, 1u, 32u, 33u, 40u, 64u, 65u}) {
        Call k;
        std::vector<uint32_t> want;
        for (uint32_t s = 0; want.size() < live; ++s) {
            if (s % 5 == 2) {
                k.add(src(s, 2, 44100, 0));  // reaches nothing: not in any launch
            } else {
                want.push_back(s);
                k.add(src(s, 2, 44100, 100), s % 2 ? 10 : 0, 4, s % 3 ? 1 : 0, 0, 0);
            }
        }
        std::vector<Launch> ls;
        walk(k.srcs.data(), (uint32_t)k.srcs.size(), [&](const Launch &L) { ls.push_back(L); });
        EXPECT(ls.size() == (live ? (live + 31) / 32 : 1u), "%u sources: %zu launches", live, ls.size());
        std::vector<uint32_t> got;
        for (size_t q = 0; q < ls.size(); ++q) {
            EXPECT(ls[q].cont == (q > 0) && ls[q].n <= kChunk && (ls[q].n == kChunk || q + 1 == ls.size()), "%u sources, launch %zu: %u", live, q, ls[q].n);
            for (uint32_t u = 0; u < ls[q].n; ++u) got.push_back(ls[q].src[u]);
        }
        EXPECT(got == want, "%u sources: every one once, in insertion order", live);
        ++g_launches;
    }
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "plan") == 0 && argc == 5) {
        uint64_t w[5] = {0, 0, 0, 0, 0};
        const rh_status st = loop_plan(std::strtoull(argv[2], nullptr, 10), (uint32_t)std::strtoul(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10), w);
        std::printf("%d %llu %llu %llu %llu %llu\n", (int)st, (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2], (unsigned long long)w[3], (unsigned long long)w[4]);
        return 0;
    }
    if (argc >= 2 && std::strcmp(argv[1], "advance") == 0 && argc == 10) {
        uint64_t w[5];
        for (int k = 0; k < 5; ++k) w[k] = std::strtoull(argv[2 + k], nullptr, 10);
        const rh_status st = loop_advance(w, (uint32_t)std::strtoul(argv[7], nullptr, 10), (uint32_t)std::strtoul(argv[8], nullptr, 10), std::strtoull(argv[9], nullptr, 10));
        std::printf("%d %llu %llu %llu %llu %llu\n", (int)st, (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2], (unsigned long long)w[3], (unsigned long long)w[4]);
        return 0;
    }
    if (argc >= 2 && std::strcmp(argv[1], "locate") == 0 && argc >= 13) {  // locate L c rule chain_start chain_out ch from_rate to_ch to_rate frames out_frames m ..
        uint64_t w[5];
        for (int k = 0; k < 5; ++k) w[k] = std::strtoull(argv[2 + k], nullptr, 10);
        static float sound[8];  // an address that is never read through
        rh_wide_src x{};
        x.data = sound, x.channels = (uint32_t)std::strtoul(argv[7], nullptr, 10), x.from_rate = (uint32_t)std::strtoul(argv[8], nullptr, 10), x.frames = std::strtoull(argv[11], nullptr, 10), x.gain = 1.0f;
        Desc d;
        const rh_status st = describe(x, w, (uint32_t)std::strtoul(argv[9], nullptr, 10), (uint32_t)std::strtoul(argv[10], nullptr, 10), std::strtoull(argv[12], nullptr, 10), &d);
        std::printf("%d\n", (int)st);
        if (st != RH_OK) return 0;
        std::printf("%u %u %u\n", d.x0, d.P, d.M);  // then per output frame m of the block: ia ib lerp num
        for (int k = 13; k < argc; ++k) {
            const Taps t = locate(d, (uint32_t)std::strtoul(argv[k], nullptr, 10));
            std::printf("%u %u %d %u\n", t.ia, t.ib, t.lerp ? 1 : 0, t.num);
        }
        return 0;
    }
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const int cases = argc > 2 ? std::atoi(argv[2]) : 400;
    std::mt19937_64 rng(seed);
    test_divs(rng);
    test_spans();
    test_locate(rng, cases);
    test_plans();
    test_refusals();
    test_bounds();
    test_launches();
    std::printf("failures %d divs %d spans %d located %d cuts %d plans %d refusals %d bounds %d launches %d\n", g_failures, g_divs, g_spans, g_located, g_cuts, g_plans, g_refusals, g_bounds,
                g_launches);
    return g_failures ? 1 : 0;
}
