// queue_mix_plan_test.cpp -- rh_queue_mix_plan.h without a GPU: the chains of a queue of sounds, the cursor, the two tables and the refusals.
//     queue_mix_plan_test [rounds [max_frames]]   the self-check: prints "name count" pairs, `failures` among them
//     queue_mix_plan_test plan to_rate channels out_frames n_sources { frames n_sounds w0 w1 w2 w3 ch rate phase last gain_bits { samples ch rate gain_bits } }
//                                                 the status and the tables of a call (tests/test_queue_mix_cpu.py compares them with the restatement)
//     queue_mix_plan_test advance to_rate out_frames w0 w1 w2 w3 n_sounds { samples ch rate }      status, the words, dropped
// The self-check holds the tables against a MODEL that plays the queue the way the Rust does it, sample by sample: a queue position, and per
// chain a Take of min(current sound's whole length, 32768) samples pulled one at a time (queue.rs:218-241, uniform.rs:56), then the converter's
// tap positions in 64-bit arithmetic.  Sounds have no memory here: a sound's `data` is a made-up address that only says which sound it is.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "rh_queue_mix_plan.h"

namespace qm = rh::queuemix;

static long failures = 0, located = 0, cuts = 0, refusals = 0, bounds = 0, chains_seen = 0, seams = 0, tails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            if (failures++ < 20) fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                               \
    } while (0)

struct TSound {
    uint64_t samples;
    uint32_t ch, rate;
    float gain;
};
static const uint64_t kBase = 0x100000000ull;  // sound k of a call "lies" at (k + 1) * kBase
static uint64_t addr(size_t k) { return (uint64_t)(k + 1) * kBase; }

struct Call {
    std::vector<uint64_t> words;  // RH_QUEUE_SOUND_WORDS a sound
    std::vector<float> gains;
    void add(const TSound &s, bool null = false) {
        const size_t k = gains.size();
        words.insert(words.end(), {null ? 0 : addr(k), s.samples, s.ch, s.rate});
        gains.push_back(s.gain);
    }
};

// A tap as the model names it: sample `off` of sound `sound` (-1: injected silence), or of the plain source (-2).
struct Ref {
    long sound;
    uint64_t off;
    bool operator==(const Ref &o) const { return sound == o.sound && (sound == -1 || off == o.off); }
};
struct Frame {  // one output frame of a queue by the model: per channel of the chain the two taps
    uint32_t ch, num, T;
    bool lerp;
    std::vector<Ref> a, b;
};
// The model.  Returns false where a chain cuts a frame (what the entry refuses).  `frames` output frames at most; *ended: the stream is over.
static bool model(const std::vector<TSound> &s, bool keep, uint32_t to_rate, uint64_t frames, std::vector<Frame> *out, std::vector<uint64_t> *chain_ends) {
    size_t k = 0;
    uint64_t off = 0;
    auto skip = [&]() { while (k < s.size() && off >= s[k].samples) ++k, off = 0; };
    skip();
    while (k < s.size() && out->size() < frames) {
        const uint32_t ch = s[k].ch, rate = s[k].rate;
        const uint64_t want = s[k].samples < 32768 ? s[k].samples : 32768;
        std::vector<Ref> taken;
        for (uint64_t q = 0; q < want; ++q) {  // Take::next over the queue
            skip();
            if (k < s.size()) taken.push_back(Ref{(long)k, off++});
            else if (keep) taken.push_back(Ref{-1, 0});
            else break;
        }
        skip();
        if (taken.size() % ch) return false;
        const uint64_t n = taken.size() / ch;
        const uint32_t g = std::gcd(rate, to_rate);
        const uint64_t F = rate / g, T = to_rate / g;
        // (sample_rate.rs:131-201: a frame whose first tap is frame i <= n - 2 lerps; the first one whose first tap is the chain's last frame comes out
        //  verbatim and ends the chain)
        for (uint64_t j = 0; out->size() < frames; ++j) {
            const uint64_t i = j * F / T;
            if (i >= n) break;
            Frame f;
            f.ch = ch, f.num = (uint32_t)((j * F) % T), f.T = (uint32_t)T, f.lerp = F != T && i + 1 < n;
            for (uint32_t c = 0; c < ch; ++c) {
                f.a.push_back(taken[i * ch + c]);
                f.b.push_back(f.lerp ? taken[(i + 1) * ch + c] : Ref{-3, 0});
            }
            out->push_back(f);
            if (i == n - 1) break;
        }
        chain_ends->push_back(out->size());
        ++chains_seen;
        if (taken.back().sound == -1) break;  // silent from here on
    }
    return true;
}

static Ref decode(const qm::Piece &p, uint64_t e, size_t first_sound) {
    if (!p.data) return Ref{-1, 0};
    const uint64_t a = (uint64_t)reinterpret_cast<uintptr_t>(p.data);
    const uint64_t k = a / kBase - 1;
    return Ref{(long)(k - first_sound), (a - addr(k)) / 4 + (e - p.start)};
}

// The taps the tables give output frame m of source `src`, against the model's frame (nullptr: the source must not reach m).
static void hold_frame(const qm::Plan &p, uint32_t src, uint32_t m, const Frame *want, size_t first_sound, const std::vector<TSound> &s) {
    const qm::Src d = p.srcs[src];
    const uint32_t q = d.seg_count ? qm::find_seg(p.segs.data() + d.seg_first, d.seg_count, m) : 0;
    if (!want) {
        CHECK(q == d.seg_count);
        return;
    }
    CHECK(q < d.seg_count);
    if (q >= d.seg_count) return;
    const qm::Seg &g = p.segs[d.seg_first + q];
    const qm::Taps t = qm::locate(g, m);
    CHECK(g.ch == want->ch && t.num == want->num && g.T == want->T && t.lerp == want->lerp && (g.Tf == 0.0f) == (g.F == g.T));
    for (uint32_t ch = 0; ch < g.ch; ++ch) {
        const uint64_t e = (uint64_t)t.i * g.ch + ch;
        const qm::Piece *pc = p.pieces.data() + g.piece_first;
        const qm::Piece &pa = pc[qm::find_piece(pc, g.piece_count, e)];
        const Ref ra = decode(pa, e, first_sound);
        CHECK(ra == want->a[ch]);
        if (ra.sound >= 0) CHECK(pa.gain == s[ra.sound].gain && ra.off < s[ra.sound].samples);
        if (t.lerp) {
            const qm::Piece &pb = pc[qm::find_piece(pc, g.piece_count, e + g.ch)];
            const Ref rb = decode(pb, e + g.ch, first_sound);
            CHECK(rb == want->b[ch]);
            if (rb.sound >= 0) CHECK(rb.off < s[rb.sound].samples);
            if (!(ra.sound == rb.sound)) ++seams;
        }
        ++located;
    }
}

static const uint32_t kRates[] = {44100, 48000, 8000, 22050, 96000, 11025};

// One queue, alone in its call: one pass against the model, then the stream cut into three unequal blocks with queue_advance between them.
static void one_queue(const std::vector<TSound> &s, bool keep, uint32_t to_rate, uint64_t total, std::mt19937 &rng) {
    std::vector<Frame> want;
    std::vector<uint64_t> ends;
    const bool whole = model(s, keep, to_rate, total, &want, &ends);
    Call c;
    for (const TSound &x : s) c.add(x);
    float dst;
    uint64_t cur[4];
    CHECK(qm::queue_plan(cur, keep) == RH_OK);
    rh_wide_src x{};
    x.frames = total;
    const uint32_t n = (uint32_t)s.size();
    static qm::Plan p;
    const rh_status st = qm::plan(&dst, 2, to_rate, total, &x, 1, c.words.data(), c.gains.data(), &n, cur, &p);
    if (!whole) {
        CHECK(st == RH_ERR_UNSUPPORTED);
        ++refusals;
        return;
    }
    CHECK(st == RH_OK);
    if (st != RH_OK) return;
    if (want.size() < total && keep) ++tails;
    for (uint64_t m = 0; m < total; ++m) hold_frame(p, 0, (uint32_t)m, m < want.size() ? &want[m] : nullptr, 0, s);
    // three unequal blocks: the cuts near a chain's end where there is one
    for (int round = 0; round < 6; ++round) {
        uint64_t c1 = rng() % (total + 1), c2 = rng() % (total + 1);
        if (!ends.empty() && round < 4) {
            const uint64_t e = ends[rng() % ends.size()];
            c1 = e > 2 ? e - 2 + rng() % 5 : rng() % 3;
            if (c1 > total) c1 = total;
        }
        if (c1 > c2) std::swap(c1, c2);
        const uint64_t cut[4] = {0, c1, c2, total};
        uint64_t w[4];
        qm::queue_plan(w, keep);
        size_t first = 0;  // sounds dropped so far
        for (int b = 0; b < 3; ++b) {
            const uint64_t len = cut[b + 1] - cut[b];
            const uint32_t left = (uint32_t)(s.size() - first);
            rh_wide_src y{};
            y.frames = left ? len : 0;  // (a count of 0 is a plain source: a queue whose sounds are all dropped reaches no frame)
            if (len) {
                const rh_status sb = qm::plan(&dst, 2, to_rate, len, &y, 1, c.words.data() + 4 * first, c.gains.data() + first, &left, w, &p);
                CHECK(sb == RH_OK);
                if (sb != RH_OK) return;
                const std::vector<TSound> rest(s.begin() + first, s.end());
                for (uint64_t m = 0; m < len; ++m) {
                    const uint64_t at = cut[b] + m;
                    Frame f;
                    if (at < want.size()) {
                        f = want[at];
                        for (Ref &r : f.a) if (r.sound >= 0) r.sound -= (long)first;
                        for (Ref &r : f.b) if (r.sound >= 0) r.sound -= (long)first;
                    }
                    hold_frame(p, 0, (uint32_t)m, at < want.size() ? &f : nullptr, first, rest);
                }
            }
            uint32_t dropped = 99;
            CHECK(qm::queue_advance(w, c.words.data() + 4 * first, left, to_rate, len, &dropped) == RH_OK);
            CHECK(dropped <= left);
            first += dropped;
            CHECK(w[2] <= 2 && w[3] == (keep ? 1u : 0u) && w[1] <= 32768ull * 48 && (w[2] == 0 || (w[0] == 0 && w[1] == 0)));
            if (w[2] == 0 && first < s.size()) CHECK(w[0] < s[first].samples || (w[0] == 0 && s[first].samples == 0));
            ++cuts;
        }
    }
}

static void random_queues(int rounds, uint64_t max_frames, uint32_t seed) {
    std::mt19937 rng(seed);
    for (int r = 0; r < rounds; ++r) {
        std::vector<TSound> s;
        const int n = 1 + rng() % 6;
        const bool even = rng() % 2;  // lengths that are whole frames of every format in the queue: no chain is cut
        for (int k = 0; k < n; ++k) {
            const uint32_t ch = 1 + rng() % (even ? 2 : 3);
            uint64_t len = rng() % 14;
            if (even) len = (len / 2) * 2;
            s.push_back(TSound{len, ch, kRates[rng() % 6], 0.25f * (float)(1 + rng() % 7)});
        }
        one_queue(s, rng() % 2, kRates[rng() % 2], 1 + rng() % max_frames, rng);
    }
}

static void the_crossing_chain() {
    // A = 32776 samples stereo at 44.1 kHz, B = 6 mono at 8 kHz, C = 10 stereo at 22.05 kHz: chain 1 is samples 0 .. 32768 of A, chain 2 the next 24
    // samples of the stream -- 8 of A, all of B and all of C -- as 12 stereo frames at 44.1 kHz.
    std::mt19937 rng(5);
    const std::vector<TSound> s{{32776, 2, 44100, 0.5f}, {6, 1, 8000, -1.5f}, {10, 2, 22050, 0.75f}};
    Call c;
    for (const TSound &x : s) c.add(x);
    uint64_t cur[4];
    qm::queue_plan(cur, 0);
    const uint64_t M1 = qm::span_out(16384, 147, 160), M2 = qm::span_out(12, 147, 160);
    rh_wide_src x{};
    x.frames = M1 + M2;
    float dst;
    const uint32_t n = 3;
    static qm::Plan p;
    CHECK(qm::plan(&dst, 2, 48000, M1 + M2 + 5, &x, 1, c.words.data(), c.gains.data(), &n, cur, &p) == RH_OK);
    CHECK(p.segs.size() == 2 && p.pieces.size() == 4);
    if (p.segs.size() == 2 && p.pieces.size() == 4) {
        CHECK(p.segs[0].count == M1 && p.segs[0].nl == 16383 && p.segs[0].piece_count == 1 && p.segs[1].m0 == M1 && p.segs[1].count == M2 && p.segs[1].nl == 11 && p.segs[1].ch == 2);
        CHECK(p.pieces[1].start == 0 && p.pieces[2].start == 8 && p.pieces[3].start == 14 && p.pieces[2].gain == -1.5f);
    }
    for (uint32_t to_rate : {48000u, 44100u}) one_queue(s, false, to_rate, 36000, rng);
    one_queue(s, true, 48000, 36000, rng);
    // a keep-alive tail: A and B alone, the second chain starts inside A and takes 32768 samples, 32754 of them silence
    one_queue({s[0], s[1]}, true, 48000, 36000, rng);
}

static void check_refusals() {
    float dst;
    static qm::Plan p;
    const std::vector<TSound> s{{8, 1, 48000, 1.0f}, {12, 2, 44100, 0.5f}, {5, 1, 44100, 2.0f}};
    Call c;
    for (const TSound &x : s) c.add(x);
    uint64_t cur[8] = {0, 0, 0, 1, 0, 0, 0, 0};
    rh_wide_src x[2]{};
    x[0].frames = 20;
    float row[64];
    x[1].data = row, x[1].channels = 2, x[1].from_rate = 44100, x[1].frames = 20, x[1].last = 0xffffffffu, x[1].gain = 1.0f;
    uint32_t n[2] = {3, 0};
    auto call = [&](uint64_t frames = 20, uint32_t ch = 2, uint32_t to_rate = 48000) { return qm::plan(&dst, ch, to_rate, frames, x, 2, c.words.data(), c.gains.data(), n, cur, &p); };
    auto refused = [&](rh_status want, rh_status got) {
        CHECK(got == want);
        ++refusals;
    };
    CHECK(call() == RH_OK);
    CHECK(p.srcs.size() == 2 && p.srcs[1].seg_count == 1 && p.segs.back().piece_count == 1 && p.pieces.back().data == row);
    refused(RH_ERR_INVALID, qm::plan(nullptr, 2, 48000, 20, x, 2, c.words.data(), c.gains.data(), n, cur, &p));
    refused(RH_ERR_INVALID, call(20, 0));
    refused(RH_ERR_INVALID, call(20, 2, 0));
    refused(RH_ERR_INVALID, qm::plan(&dst, 2, 48000, 20, nullptr, 2, c.words.data(), c.gains.data(), n, cur, &p));
    refused(RH_ERR_INVALID, qm::plan(&dst, 2, 48000, 20, x, 2, nullptr, c.gains.data(), n, cur, &p));
    refused(RH_ERR_INVALID, qm::plan(&dst, 2, 48000, 20, x, 2, c.words.data(), c.gains.data(), nullptr, cur, &p));
    refused(RH_ERR_INVALID, qm::plan(&dst, 2, 48000, 20, x, 2, c.words.data(), c.gains.data(), n, nullptr, &p));
    CHECK(qm::plan(&dst, 2, 48000, 20, x, 2, c.words.data(), nullptr, n, cur, &p) == RH_OK && p.pieces[0].gain == 1.0f);  // no gains: 1
    refused(RH_ERR_UNSUPPORTED, call(0x80000000ull));
    refused(RH_ERR_UNSUPPORTED, call(0x7fffffffull));  // the plain source: out_frames > (2^32 - 1 - T) / F
    x[0].frames = 21;
    refused(RH_ERR_INVALID, call());
    x[0].frames = 20;
    const uint64_t broken[][2] = {{0, 0}, {2, 0}, {3, 0}, {2, 1ull << 32}, {3, 1ull << 32}};  // of sound 1: data 0 with samples, channels 0, rate 0, either beyond 32 bits
    for (const auto &b : broken) {
        const uint64_t kept = c.words[4 + b[0]];
        c.words[4 + b[0]] = b[1];
        refused(RH_ERR_INVALID, call());
        c.words[4 + b[0]] = kept;
    }
    // the cursor: state, flags, chain_start, chain_out (the first chain: 8 mono frames at 48 kHz emit 8), words of a queue that is not playing
    const uint64_t bad[][4] = {{0, 0, 3, 1}, {0, 0, 0, 2}, {8, 0, 0, 1}, {0, 8, 0, 1}, {1, 0, 1, 1}, {0, 1, 2, 0}};
    for (const auto &b : bad) {
        memcpy(cur, b, sizeof b);
        refused(RH_ERR_INVALID, call());
    }
    const uint64_t good[][4] = {{7, 0, 0, 1}, {0, 7, 0, 1}, {0, 0, 1, 1}, {0, 0, 2, 0}};
    for (const auto &b : good) {
        memcpy(cur, b, sizeof b);
        CHECK(call() == RH_OK);
    }
    memcpy(cur, good[2], sizeof good[2]);  // a silent queue reaches nothing
    CHECK(call() == RH_OK && p.srcs[0].seg_count == 0);
    const uint64_t fresh[4] = {0, 0, 0, 1};
    memcpy(cur, fresh, sizeof fresh);
    // the plain source's own refusals
    x[1].phase = 160;
    refused(RH_ERR_INVALID, call());
    x[1].phase = 0, x[1].data = nullptr;
    refused(RH_ERR_INVALID, call());
    x[1].data = row, x[1].from_rate = 4294967291u;
    refused(RH_ERR_UNSUPPORTED, call());
    x[1].from_rate = 44100;
    // F T beyond 32 bits of a chain
    refused(RH_ERR_UNSUPPORTED, call(20, 2, 4294967291u));
    // a queue that reaches no frame is not looked at
    x[0].frames = 0;
    c.words[6] = 0;
    CHECK(call() == RH_OK);
    c.words[6] = 1, x[0].frames = 20;
    // chains that cut a frame: a 6-channel sound of 32772 samples (its first chain takes 32768: 5461 frames and 2 samples); a stereo sound of more
    // than a chain followed by a mono sound of odd length that ends the seam chain
    {
        Call d;
        d.add(TSound{32772, 6, 48000, 1.0f});
        uint32_t one = 1;
        rh_wide_src y{};
        y.frames = 10;
        refused(RH_ERR_UNSUPPORTED, qm::plan(&dst, 2, 48000, 10, &y, 1, d.words.data(), d.gains.data(), &one, fresh, &p));
        Call e;
        e.add(TSound{32776, 2, 44100, 1.0f}), e.add(TSound{5, 1, 44100, 1.0f});
        uint32_t two = 2;
        uint64_t w[4] = {0, 0, 0, 0};
        y.frames = 40000;
        refused(RH_ERR_UNSUPPORTED, qm::plan(&dst, 2, 48000, 40000, &y, 1, e.words.data(), e.gains.data(), &two, w, &p));
        y.frames = 17000;  // ... a block that does not reach the seam chain is taken
        CHECK(qm::plan(&dst, 2, 48000, 40000, &y, 1, e.words.data(), e.gains.data(), &two, w, &p) == RH_OK);
        uint32_t dropped;
        refused(RH_ERR_UNSUPPORTED, qm::queue_advance(w, e.words.data(), 2, 48000, 40000, &dropped));
        CHECK(w[0] == 0 && w[1] == 0);
        // with keep_alive the chain is filled up: 24 samples, 12 frames
        w[3] = 1;
        CHECK(qm::plan(&dst, 2, 48000, 40000, &y, 1, e.words.data(), e.gains.data(), &two, w, &p) == RH_OK);
    }
    refused(RH_ERR_INVALID, qm::queue_plan(nullptr, 1));
    refused(RH_ERR_INVALID, qm::queue_plan(cur, 2));
    uint32_t dropped;
    refused(RH_ERR_INVALID, qm::queue_advance(nullptr, c.words.data(), 3, 48000, 5, &dropped));
    refused(RH_ERR_INVALID, qm::queue_advance(cur, c.words.data(), 3, 48000, 5, nullptr));
    refused(RH_ERR_INVALID, qm::queue_advance(cur, c.words.data(), 3, 0, 5, &dropped));
    refused(RH_ERR_INVALID, qm::queue_advance(cur, nullptr, 3, 48000, 5, &dropped));
}

// M F at the edge of 32 bits: a mono sound of n frames from rate 1 (F = 1 against an odd T) emits M = (n - 1) T + 1 frames.
static void check_bounds() {
    float dst;
    static qm::Plan p;
    for (uint32_t nfr : {2u, 3u, 1000u, 32768u}) {
        // the largest T with ((n - 1) T + 1) * 1 <= 2^32 - 1, and the next one
        const uint64_t t_ok = (0xffffffffull - 1) / (nfr - 1);
        for (uint64_t T : {t_ok, t_ok + 1}) {
            if (T > 0xffffffffull) continue;
            Call c;
            c.add(TSound{nfr, 1, 1, 1.0f});
            uint64_t cur[4] = {0, 0, 0, 1};
            rh_wide_src x{};
            x.frames = 100;
            uint32_t one = 1;
            const rh_status st = qm::plan(&dst, 1, (uint32_t)T, 100, &x, 1, c.words.data(), c.gains.data(), &one, cur, &p);
            const uint64_t M = qm::span_out(nfr, 1, T);
            CHECK(M == (uint64_t)(nfr - 1) * T + 1);
            CHECK(st == (M <= 0xffffffffull ? RH_OK : RH_ERR_UNSUPPORTED));
            if (st == RH_OK) {  // the chain's last output frames: the cursor just in front of them
                cur[1] = M - 100;
                CHECK(qm::plan(&dst, 1, (uint32_t)T, 100, &x, 1, c.words.data(), c.gains.data(), &one, cur, &p) == RH_OK);
                const qm::Seg &g = p.segs[0];
                const qm::Taps last = qm::locate(g, 99), before = qm::locate(g, 98);
                CHECK(g.count == 100 && last.i == nfr - 1 && !last.lerp && last.num == 0 && before.i == nfr - 2 && before.lerp && before.num == T - 1);
            }
            ++bounds;
        }
    }
}

static int cmd_plan(int argc, char **argv) {
    int a = 2;
    auto next = [&]() -> uint64_t { return a < argc ? strtoull(argv[a++], nullptr, 10) : 0; };
    const uint32_t to_rate = (uint32_t)next(), channels = (uint32_t)next();
    const uint64_t out_frames = next();
    const uint32_t n_sources = (uint32_t)next();
    std::vector<rh_wide_src> srcs(n_sources);
    std::vector<uint32_t> counts(n_sources);
    std::vector<uint64_t> cursors(4 * (size_t)n_sources + 4);
    Call c;
    for (uint32_t s = 0; s < n_sources; ++s) {
        rh_wide_src &x = srcs[s];
        x.frames = next(), counts[s] = (uint32_t)next();
        for (int w = 0; w < 4; ++w) cursors[4 * s + w] = next();
        x.channels = (uint32_t)next(), x.from_rate = (uint32_t)next(), x.phase = (uint32_t)next(), x.last = (uint32_t)next();
        const uint32_t gb = (uint32_t)next();
        memcpy(&x.gain, &gb, 4);
        x.data = counts[s] ? nullptr : reinterpret_cast<const float *>((uintptr_t)0x1000);
        for (uint32_t k = 0; k < counts[s]; ++k) {
            TSound t;
            t.samples = next(), t.ch = (uint32_t)next(), t.rate = (uint32_t)next();
            const uint32_t b = (uint32_t)next();
            memcpy(&t.gain, &b, 4);
            c.add(t);
        }
    }
    float dst;
    qm::Plan p;
    const rh_status st = qm::plan(&dst, channels, to_rate, out_frames, srcs.data(), n_sources, c.words.data(), c.gains.data(), counts.data(), cursors.data(), &p);
    printf("%d\n", (int)st);
    if (st != RH_OK) return 0;
    size_t first_sound = 0;
    for (uint32_t s = 0; s < n_sources; ++s) {
        printf("src %u\n", p.srcs[s].seg_count);
        for (uint32_t q = 0; q < p.srcs[s].seg_count; ++q) {
            const qm::Seg &g = p.segs[p.srcs[s].seg_first + q];
            printf("seg %u %u %u %u %u %u %u %u %d\n", g.m0, g.count, g.prior, g.ch, g.F, g.T, g.nl, g.piece_count, (int)((g.Tf == 0.0f) == (g.F == g.T) && g.r0 == (counts[s] ? 0u : srcs[s].phase)));
            for (uint32_t k = 0; k < g.piece_count; ++k) {
                const qm::Piece &pc = p.pieces[g.piece_first + k];
                uint32_t gb;
                memcpy(&gb, &pc.gain, 4);
                if (!counts[s]) printf("piece -2 0 %u %u\n", pc.start, gb);
                else {
                    const Ref r = decode(pc, pc.start, first_sound);
                    printf("piece %ld %" PRIu64 " %u %u\n", r.sound, r.sound < 0 ? 0 : r.off, pc.start, gb);
                }
            }
        }
        first_sound += counts[s];
    }
    return 0;
}

static int cmd_advance(int argc, char **argv) {
    int a = 2;
    auto next = [&]() -> uint64_t { return a < argc ? strtoull(argv[a++], nullptr, 10) : 0; };
    const uint32_t to_rate = (uint32_t)next();
    const uint64_t out_frames = next();
    uint64_t w[4];
    for (uint64_t &v : w) v = next();
    const uint32_t n = (uint32_t)next();
    Call c;
    for (uint32_t k = 0; k < n; ++k) {
        TSound t;
        t.samples = next(), t.ch = (uint32_t)next(), t.rate = (uint32_t)next(), t.gain = 1.0f;
        c.add(t, true);  // (the cursor's arithmetic reads no sample: no address needed)
    }
    uint32_t dropped = 0;
    const rh_status st = qm::queue_advance(w, c.words.data(), n, to_rate, out_frames, &dropped);
    printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", (int)st, w[0], w[1], w[2], w[3], dropped);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "plan")) return cmd_plan(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "advance")) return cmd_advance(argc, argv);
    const int rounds = argc > 1 ? atoi(argv[1]) : 400;
    const uint64_t max_frames = argc > 2 ? strtoull(argv[2], nullptr, 10) : 60;
    random_queues(rounds, max_frames, 1);
    the_crossing_chain();
    check_refusals();
    check_bounds();
    printf("failures %ld located %ld cuts %ld refusals %ld bounds %ld chains %ld seams %ld tails %ld\n", failures, located, cuts, refusals, bounds, chains_seen, seams, tails);
    return failures ? 1 : 0;
}
