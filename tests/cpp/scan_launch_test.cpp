// scan_launch_test.cpp -- the scan kernels' host protocol (rodio_amd/csrc/rh_scan_launch.h) against a small model of the device, and the
// variant pick against the rule written out as a brute-force scan.  TEST INFRASTRUCTURE: plain g++, no HIP, no library.
//
//     scan_launch_test [seed [random sequences]]
//
// The model: a scratch is an address, a ticket counter and two hand-off tables, each either all "not yet" or used.  The kernel in front of
// a launch sets the counter to 0 and clears both tables; a launch without a carried state on table p marks p used, clears p ^ 1 and advances
// the counter by total + 2 * grid; one with a carried state uses table 0 and clears nothing.  Before every launch: its table is all "not
// yet", its ticket_base is the counter, and the kernel in front is left out exactly when the launch directly before it on that scratch was
// the same kernel and shape, carried no state and succeeded (and this one carries none and does not force the initialisation).
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "rh_scan_launch.h"

namespace scan = rh::scan;

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

// ---- the protocol ----------------------------------------------------------------------------------------------------------
struct Shape {
    uint32_t n_streams, tiles, channels;
    bool operator==(const Shape &o) const { return n_streams == o.n_streams && tiles == o.tiles && channels == o.channels; }
};
enum Kernel { LIMIT = 0, BIQUAD = 1 };
// what each unit asks for (rh_limit.hip: states [n][2], records of Rec<C>::stride floats -- 5 C rounded up to 4 stands in for it here;
// rh_biquad_scan.hip: [n][6], 2 C)
static size_t own_bytes(Kernel k, const Shape &s) { return (size_t)s.n_streams * s.channels * (k == LIMIT ? 2 : 6) * 4; }
static size_t rec_floats(Kernel k, const Shape &s) { return k == LIMIT ? (5 * s.channels + 3) / 4 * 4 : 2 * s.channels; }
static uint64_t seed_of(Kernel k) { return k == LIMIT ? scan::kSeedLimit : scan::kSeedBiquad; }

struct Device {  // what is in the scratch's memory
    uint32_t counter = 0xdeadbeefu;
    bool used[2] = {true, true};
    void garbage(uint32_t c) { counter = c, used[0] = used[1] = true; }
};
struct Last {  // the launch directly before, on this scratch
    bool valid = false, carried = false, ok = false;
    Kernel kernel = LIMIT;
    Shape shape{0, 0, 0};
};
struct Step {
    enum What { LAUNCH, FOREIGN, REALLOC, DISTRUST } what = LAUNCH;
    Kernel kernel = LIMIT;
    Shape shape{1, 1, 1};
    bool carried = false, force_init = false;
    int fail = 0;           // 1: the kernel in front fails to launch, 2: the scan kernel does
    int tickets_left = -1;  // >= 0: RH_COUNTER_JUMP falls on this launch
    uint32_t grid = 1;
};
struct Counts {
    uint64_t launches = 0, inits = 0, skipped = 0, jumps = 0, failed = 0;
};

struct Stream {  // one stream's scratch as rh::stream_scratch keeps it
    rh::ScratchAux aux{0, 0, 0};
    uint64_t address = 0x7f0000100000ull;
    Device dev;
    Last last;

    void run(const Step &st, Counts &n, int seq, int pos) {
        if (st.what == Step::FOREIGN) {  // a caller that passes no `aux`: stream_scratch zeroes it; the caller writes where it likes
            aux = rh::ScratchAux{0, 0, 0};
            dev.garbage(dev.counter * 2654435761u + 12345u);
            last.valid = false;
            return;
        }
        if (st.what == Step::REALLOC) {  // the buffer grows: another address, fresh memory
            aux = rh::ScratchAux{0, 0, 0};
            address += 0x200000;
            dev.garbage(0xa5a5a5a5u);
            last.valid = false;
            return;
        }
        if (st.what == Step::DISTRUST) {  // a lost hand-off was reported (rh_runtime.hip: distrust_stream_scratch)
            aux = rh::ScratchAux{0, 0, 0};
            last.valid = false;
            return;
        }
        // the launcher's order (rh_scan_common.h: scan_launch)
        const uint64_t total = (uint64_t)st.shape.tiles * st.shape.n_streams;
        const scan::Layout lay = scan::layout(own_bytes(st.kernel, st.shape), (size_t)total * rec_floats(st.kernel, st.shape) * 4);
        const uint64_t tag = scan::shape_tag(seed_of(st.kernel), st.shape.n_streams, st.shape.tiles, st.shape.channels, lay, address);
        const scan::Begin b = scan::begin(&aux, tag, st.carried, st.force_init);
        bool ok = true;
        if (b.init) {
            ++n.inits;
            if (st.fail == 1) ok = false;
            else dev.counter = 0, dev.used[0] = dev.used[1] = false;
        } else {
            ++n.skipped;
        }
        if (st.tickets_left >= 0) {
            const uint32_t d = scan::jump(&aux, (uint32_t)st.tickets_left);
            if (ok) dev.counter += d;  // rh::counters_add
            ++n.jumps;
        }
        const uint32_t ticket_base = aux.ticket_base;
        const bool want_skip = last.valid && last.ok && !last.carried && last.kernel == st.kernel && last.shape == st.shape && !st.carried && !st.force_init;
        EXPECT(b.init == !want_skip, "sequence %d step %d: init %d, expected %d", seq, pos, (int)b.init, (int)!want_skip);
        EXPECT(b.table < 2 && (st.carried ? (b.table == 0 && b.other == -1) : b.other == (int)(b.table ^ 1u)), "sequence %d step %d: tables %u %d", seq, pos, b.table, b.other);
        if (ok) {  // the scan kernel is about to be launched
            EXPECT(!dev.used[b.table & 1], "sequence %d step %d: table %u is not clean", seq, pos, b.table);
            EXPECT(ticket_base == dev.counter, "sequence %d step %d: ticket_base %u, counter %u", seq, pos, ticket_base, dev.counter);
            if (st.tickets_left >= 0) EXPECT(ticket_base == 0u - (uint32_t)st.tickets_left, "sequence %d step %d: jump to %u", seq, pos, ticket_base);
            if (st.fail == 2) ok = false;
        }
        if (ok) {
            ++n.launches;
            dev.used[b.table & 1] = true;
            if (b.other >= 0) dev.used[b.other] = false;
            dev.counter += (uint32_t)(total + 2 * (uint64_t)st.grid);
            scan::launched(&aux, st.carried, total, st.grid);
        } else {
            ++n.failed;
            scan::failed(&aux);
        }
        last.valid = true, last.ok = ok, last.carried = st.carried, last.kernel = st.kernel, last.shape = st.shape;
    }
};

static Step launch(Kernel k, Shape s, bool carried = false, bool force = false, int fail = 0, int left = -1, uint32_t grid = 7) {
    Step st;
    st.kernel = k, st.shape = s, st.carried = carried, st.force_init = force, st.fail = fail, st.tickets_left = left, st.grid = grid;
    return st;
}
static Step other(Step::What w) {
    Step st;
    st.what = w;
    return st;
}

static void scripted(Counts &n) {
    const Shape A{3, 4, 2}, B{3, 5, 2}, C{5, 4, 2};
    const std::vector<std::vector<Step>> scripts = {
        // the same shape again and again: one initialisation
        {launch(BIQUAD, A), launch(BIQUAD, A), launch(BIQUAD, A), launch(BIQUAD, A)},
        // a carried state in between; the launches behind it start over
        {launch(BIQUAD, A), launch(BIQUAD, A), launch(BIQUAD, A, true), launch(BIQUAD, A), launch(BIQUAD, A)},
        // the other kernel with the same shape numbers, and back
        {launch(LIMIT, A), launch(BIQUAD, A), launch(BIQUAD, A), launch(LIMIT, A), launch(LIMIT, A)},
        // another shape of the same kernel, and back
        {launch(LIMIT, C), launch(LIMIT, C), launch(LIMIT, B), launch(LIMIT, C), launch(LIMIT, C)},
        // a foreign user of the scratch, a reallocation, a distrusted scratch
        {launch(LIMIT, A), launch(LIMIT, A), other(Step::FOREIGN), launch(LIMIT, A), launch(LIMIT, A), other(Step::REALLOC), launch(LIMIT, A), launch(LIMIT, A), other(Step::DISTRUST),
         launch(LIMIT, A), launch(LIMIT, A)},
        // force_init every time, then not
        {launch(BIQUAD, A, false, true), launch(BIQUAD, A, false, true), launch(BIQUAD, A), launch(BIQUAD, A)},
        // failures of either kernel: the next call starts over
        {launch(LIMIT, A), launch(LIMIT, A, false, false, 2), launch(LIMIT, A), launch(LIMIT, A), launch(LIMIT, A, false, false, 1), launch(LIMIT, A), launch(LIMIT, A, true, false, 1),
         launch(LIMIT, A), launch(LIMIT, A, true, false, 2), launch(LIMIT, A)},
        // the counter jump on a clean launch, on a first one, with a carried state, in front of a failure
        {launch(LIMIT, A), launch(LIMIT, A, false, false, 0, 3), launch(LIMIT, A), launch(LIMIT, A), launch(LIMIT, B, false, false, 0, 0), launch(LIMIT, B), launch(LIMIT, B, true, false, 0, 9),
         launch(LIMIT, B), launch(LIMIT, B, false, false, 2, 5), launch(LIMIT, B), launch(LIMIT, B, false, false, 1, 5), launch(LIMIT, B), launch(LIMIT, B)},
        // the sequence of tests/test_gpu_scan_fuzz.py::test_launches_without_init_match_forced_init
        {launch(BIQUAD, A), launch(BIQUAD, A), launch(BIQUAD, A), launch(BIQUAD, A, true), launch(BIQUAD, A), launch(BIQUAD, A), launch(LIMIT, C), launch(LIMIT, C),
         launch(LIMIT, Shape{5, 5, 2}), launch(LIMIT, C), launch(LIMIT, C), launch(BIQUAD, A)},
    };
    int seq = 0;
    for (const auto &script : scripts) {
        Stream s;
        int pos = 0;
        for (const Step &st : script) s.run(st, n, -1 - seq, pos++);
        ++seq;
    }
    // one initialisation for four launches, and the tables alternate
    Stream s;
    Counts c;
    for (int i = 0; i < 4; ++i) s.run(launch(BIQUAD, A), c, -100, i);
    EXPECT(c.inits == 1 && c.skipped == 3 && c.launches == 4, "inits %llu skipped %llu", (unsigned long long)c.inits, (unsigned long long)c.skipped);
    EXPECT(s.aux.parity == 0 && s.aux.ticket_base == 4 * (12 + 14), "parity %u base %u", s.aux.parity, s.aux.ticket_base);
}

static void random_sequences(uint64_t seed, int count, Counts &n) {
    std::mt19937_64 rng(seed);
    auto pick = [&](uint32_t k) { return (uint32_t)(rng() % k); };
    const Shape shapes[] = {{3, 4, 2}, {3, 5, 2}, {5, 4, 2}, {1, 1, 1}, {700, 3, 8}, {64, 128, 2}};
    for (int seq = 0; seq < count; ++seq) {
        Stream s;
        Step prev = launch(LIMIT, shapes[0]);
        const int len = 8 + (int)pick(40);
        for (int pos = 0; pos < len; ++pos) {
            Step st = prev;
            st.what = Step::LAUNCH, st.carried = false, st.force_init = false, st.fail = 0, st.tickets_left = -1;
            st.grid = 1 + pick(2048);
            switch (pick(16)) {
                case 0: case 1: case 2: case 3: case 4: break;                              // the same shape again
                case 5: case 6: st.shape = shapes[pick(6)]; break;                          // another shape of the same kernel
                case 7: case 8: st.kernel = st.kernel == LIMIT ? BIQUAD : LIMIT; break;     // the other kernel, equal shape numbers
                case 9: st.carried = true; break;
                case 10: st.what = Step::FOREIGN; break;
                case 11: st.what = pick(2) ? Step::REALLOC : Step::DISTRUST; break;
                case 12: st.force_init = true; break;
                case 13: st.fail = 1 + (int)pick(2), st.carried = pick(4) == 0; break;
                case 14: st.tickets_left = (int)pick(10); break;
                default: st.tickets_left = (int)pick(10), st.carried = pick(3) == 0, st.fail = pick(5) == 0 ? 1 + (int)pick(2) : 0; break;
            }
            s.run(st, n, seq, pos);
            if (st.what == Step::LAUNCH) prev = st;
        }
    }
}

// ---- arithmetic ------------------------------------------------------------------------------------------------------------
static void arithmetic() {
    for (size_t own : {size_t(0), size_t(1), size_t(63), size_t(64), size_t(65), size_t(4800)})
        for (size_t tab : {size_t(4), size_t(64), size_t(100), size_t(1) << 33}) {
            const scan::Layout l = scan::layout(own, tab);
            EXPECT(l.head % 64 == 0 && l.gran_bytes % 64 == 0, "alignment");
            EXPECT(l.head >= scan::kOwnOffset + own && l.head < scan::kOwnOffset + own + 64, "head %zu for %zu", l.head, own);
            EXPECT(l.gran_bytes >= tab && l.gran_bytes < tab + 64, "table %zu for %zu", l.gran_bytes, tab);
            EXPECT(l.table(0) == l.head && l.table(1) == l.head + l.gran_bytes && l.total() == l.head + 2 * l.gran_bytes, "offsets");
            EXPECT(l.n_words() * 4 == 2 * l.gran_bytes, "words");
        }
    EXPECT(scan::tickets_fit(0x7fffffffull, 1) && !scan::tickets_fit(0x80000000ull, 1), "tiles per stream");
    EXPECT(scan::tickets_fit(0xfff00000ull / 16 - 1, 16) && !scan::tickets_fit(0xfff00000ull / 16, 16) && scan::tickets_fit(1, 0xffefffffu) && !scan::tickets_fit(1, 0xfff00000u), "tickets per launch");
    EXPECT(!scan::tickets_fit(0x7fffffffull, 0xffffffffu), "the product does not wrap");
    const scan::Layout l = scan::layout(48, 960);
    const uint64_t t = scan::shape_tag(scan::kSeedLimit, 3, 4, 2, l, 0x1000);
    EXPECT((t & 1) && t != scan::shape_tag(scan::kSeedBiquad, 3, 4, 2, l, 0x1000), "seed");
    EXPECT(t != scan::shape_tag(scan::kSeedLimit, 4, 3, 2, l, 0x1000) && t != scan::shape_tag(scan::kSeedLimit, 3, 4, 2, l, 0x2000), "shape and address");
    {  // FNV-1a over the six values, from the definition
        uint64_t h = scan::kSeedLimit;
        const uint64_t vals[6] = {3, 4, 2, l.head, l.gran_bytes, 0x1000};
        for (uint64_t v : vals) h = (h ^ v) * 1099511628211ull;
        EXPECT(t == (h | 1), "tag");
    }
    // workgroups per CU: the runtime's answer, at least 1, at most 16 waves a CU; the knob wins
    EXPECT(scan::per_cu(0, 8, 0) == 1 && scan::per_cu(1, 8, 0) == 1 && scan::per_cu(2, 8, 0) == 2 && scan::per_cu(3, 8, 0) == 2, "8 waves");
    EXPECT(scan::per_cu(8, 1, 0) == 8 && scan::per_cu(32, 1, 0) == 16 && scan::per_cu(5, 4, 0) == 4 && scan::per_cu(1, 16, 0) == 1 && scan::per_cu(2, 16, 0) == 1, "other block sizes");
    EXPECT(scan::per_cu(2, 8, 5) == 5 && scan::per_cu(2, 8, -1) == 2, "knob");
    EXPECT(scan::launch_grid(256, 2, 1000) == 512 && scan::launch_grid(256, 2, 100) == 100 && scan::launch_grid(256, 1, 256) == 256, "grid");
    EXPECT(rh::kSpinLimit == 1u << 22, "spin limit");
}

// ---- the variant pick ------------------------------------------------------------------------------------------------------
struct V {
    int C, R, NW, NIO;
};
// rh_limit.hip: kVariants (the first one has I/O waves)
static const V kLimit[] = {
    {2, 16, 6, 2}, {1, 8, 8, 0}, {1, 16, 8, 0}, {1, 16, 16, 0}, {1, 8, 1, 0}, {2, 8, 8, 0}, {2, 8, 16, 0}, {2, 8, 4, 0}, {2, 8, 1, 0}, {2, 16, 8, 0}, {2, 16, 4, 0}, {3, 4, 8, 0},
    {3, 4, 1, 0},  {4, 4, 8, 0}, {4, 4, 1, 0},  {5, 4, 8, 0},   {5, 4, 1, 0}, {6, 4, 8, 0}, {6, 4, 1, 0},  {7, 4, 8, 0}, {7, 4, 1, 0}, {8, 4, 8, 0},  {8, 4, 1, 0},
};
// rh_biquad_scan.hip: kVariants
static const V kBiquad[] = {
    {1, 16, 8, 0}, {1, 16, 1, 0}, {2, 8, 8, 0}, {2, 16, 8, 0}, {2, 8, 4, 0}, {2, 8, 1, 0}, {3, 4, 8, 0}, {3, 4, 1, 0}, {4, 4, 8, 0},
    {4, 4, 1, 0},  {5, 4, 8, 0},  {5, 4, 1, 0}, {6, 4, 8, 0},  {6, 4, 1, 0}, {7, 4, 8, 0}, {7, 4, 1, 0}, {8, 4, 8, 0}, {8, 4, 1, 0},
};

// The rule, written out: among the variants of this channel count that may be chosen, the longest tile that the stream fills at least half
// of, more frames per lane among equals; nothing fits: the shortest.  The first in the table among what is still equal.
template <size_t N>
static const V *brute_default(const V (&tab)[N], int channels, uint64_t frames, bool limiter) {
    std::vector<const V *> cand;
    for (const V &v : tab)
        if (v.C == channels && !(limiter && (v.NW > 8 || v.NIO))) cand.push_back(&v);
    if (cand.empty()) return nullptr;
    uint64_t longest_fit = 0, shortest = ~0ull;
    for (const V *v : cand) {
        const uint64_t tile = 64ull * v->R * v->NW;
        if (2 * frames >= tile && tile > longest_fit) longest_fit = tile;
        if (tile < shortest) shortest = tile;
    }
    const uint64_t tile_wanted = longest_fit ? longest_fit : shortest;
    int most_R = 0;
    for (const V *v : cand)
        if (64ull * v->R * v->NW == tile_wanted && v->R > most_R) most_R = v->R;
    for (const V *v : cand)
        if (64ull * v->R * v->NW == tile_wanted && v->R == most_R) return v;
    return nullptr;
}
// ... with a request: the smallest 10 |NW - want| + |R - want|, I/O-wave variants left out
template <size_t N>
static const V *brute_request(const V (&tab)[N], int channels, int want_R, int want_NW) {
    int best = 1 << 30;
    for (const V &v : tab)
        if (v.C == channels && !v.NIO) {
            const int sc = 10 * (v.NW > want_NW ? v.NW - want_NW : want_NW - v.NW) + (v.R > want_R ? v.R - want_R : want_R - v.R);
            if (sc < best) best = sc;
        }
    for (const V &v : tab)
        if (v.C == channels && !v.NIO && 10 * (v.NW > want_NW ? v.NW - want_NW : want_NW - v.NW) + (v.R > want_R ? v.R - want_R : want_R - v.R) == best) return &v;
    return nullptr;
}

template <size_t N>
static uint64_t variant_pick(const V (&tab)[N], bool limiter) {
    uint64_t checked = 0;
    std::vector<uint64_t> frames = {1, 2, 63, 64, 100, 1ull << 20, 1ull << 40};
    for (const V &v : tab) {
        const uint64_t tile = 64ull * v.R * v.NW;
        for (uint64_t f : {tile / 2 - 1, tile / 2, tile / 2 + 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1}) frames.push_back(f);
    }
    for (int ch = 0; ch <= 9; ++ch) {  // (0 and 9: no variant)
        for (uint64_t f : frames) {
            const V *got = limiter ? scan::pick_variant(tab, (uint32_t)ch, f, nullptr, [](const V &c) { return !c.NIO && c.NW <= 8; })  // rh_limit.hip's predicate
                                   : scan::pick_variant(tab, (uint32_t)ch, f, nullptr, [](const V &) { return true; });
            const V *want = brute_default(tab, ch, f, limiter);
            EXPECT(got == want, "%s, %d channels, %llu frames: variant %d, expected %d", limiter ? "limiter" : "biquad", ch, (unsigned long long)f, got ? (int)(got - tab) : -1,
                   want ? (int)(want - tab) : -1);
            EXPECT((got != nullptr) == (ch >= 1 && ch <= 8), "%d channels", ch);
            ++checked;
        }
        for (int R : {1, 4, 5, 8, 12, 16, 32})
            for (int NW : {1, 2, 3, 4, 6, 8, 12, 16, 20}) {
                const scan::Request rq{R, NW};
                const V *got = scan::pick_variant(tab, (uint32_t)ch, 12345, &rq, [](const V &c) { return !c.NIO; });
                const V *want = brute_request(tab, ch, R, NW);
                EXPECT(got == want, "%s, %d channels, request R %d NW %d: variant %d, expected %d", limiter ? "limiter" : "biquad", ch, R, NW, got ? (int)(got - tab) : -1,
                       want ? (int)(want - tab) : -1);
                ++checked;
            }
    }
    return checked;
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 20240607ull;
    const int count = argc > 2 ? std::atoi(argv[2]) : 4000;
    Counts n;
    scripted(n);
    random_sequences(seed, count, n);
    arithmetic();
    const uint64_t picks = variant_pick(kLimit, true) + variant_pick(kBiquad, false);
    // the default geometry of the headline shapes, spelled out (8192-frame tiles with 16 frames per lane for stereo)
    const V *stereo = scan::pick_variant(kLimit, 2, 1u << 20, nullptr, [](const V &c) { return !c.NIO && c.NW <= 8; });
    EXPECT(stereo && stereo->R == 16 && stereo->NW == 8, "stereo limiter geometry");
    const V *block = scan::pick_variant(kBiquad, 2, 480, nullptr, [](const V &) { return true; });
    EXPECT(block && block->R == 8 && block->NW == 1, "a pull shim's block");
    std::printf("launches %llu inits %llu skipped %llu jumps %llu failed %llu picks %llu failures %d\n", (unsigned long long)n.launches, (unsigned long long)n.inits,
                (unsigned long long)n.skipped, (unsigned long long)n.jumps, (unsigned long long)n.failed, (unsigned long long)picks, g_failures);
    return g_failures ? 1 : 0;
}
