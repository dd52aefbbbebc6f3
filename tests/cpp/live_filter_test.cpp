// Driver for tests/test_live_filter_cpu.py (linked against tests/cpp/fake_device.cpp + fake_live.cpp + fake_live_filter.cpp:
// live_filter_test_fake) and tests/test_gpu_live_filter.py (linked against the library: live_filter_test): chains of
// include/rodio_hip.hpp with live_low_pass / live_high_pass and periodic_access(), the filter sweep of rodio's BltFilter::to_low_pass /
// to_high_pass.  Test infrastructure: the expected values come from the Python side.
//
//   live_filter_test run <dir> <case> <block_frames> [<pull>]
//       <dir>/src_0.f32 (2 ch 48000) -> <dir>/out.f32, <dir>/calls.txt (one line per closure call: "<access> <index>").  <pull>: samples
//       per read() (0, the default: next() sample by sample).
//       cases: sweep       live_low_pass(100) -> periodic_access(5 ms, to_low_pass(sweep_freq(k)))
//              sweep_tp    sweep with live_filters_time_parallel()
//              switch      live_low_pass(1000) -> periodic_access(5 ms): to_low_pass(1000 + 50 k) for k < 30, then to_high_pass(1000 + 20 (k - 30))
//              two_access  live_low_pass(500) -> periodic_access(5 ms, to_low_pass_with_q(sweep_freq(k), 0.707)) -> periodic_access(7 ms, to_low_pass(8000 - sweep_freq(k) / 2))
//              behind_amplify  live_amplify(1) -> live_low_pass(300) -> periodic_access(5 ms: set_factor(0.5 + 0.125 (k % 5)), to_low_pass(sweep_freq(k)))
//              fixed       live_low_pass(200), no access point; <dir>/plain.f32: exact_filters().low_pass(200)
//              seek        sweep, try_seek(500 ms) after <dir>/seek.txt samples
//   live_filter_test args       rh_biquad_steps with arguments it refuses (and an empty block): one status per line, then the untouched state
//   live_filter_test refuse     a spanned upstream that changes its format in front of live_low_pass: exit 3 with RH_ERR_UNSUPPORTED
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rodio_hip.hpp"

namespace rh = rodio_hip;
using Nanos = rh::Nanos;

static std::vector<float> read_f32(const std::string &path) {
    std::vector<float> v;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / 4);
    if (n && std::fread(v.data(), 4, v.size(), f) != v.size()) throw std::runtime_error("short read " + path);
    std::fclose(f);
    return v;
}
static void write_f32(const std::string &path, const std::vector<float> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    if (!v.empty()) std::fwrite(v.data(), 4, v.size(), f);
    std::fclose(f);
}
static std::vector<float> drain(rh::Source &s, std::size_t pull) {
    std::vector<float> out;
    if (!pull) {
        while (std::optional<float> v = s.next()) out.push_back(*v);
        return out;
    }
    std::vector<float> buf(pull);
    for (;;) {
        const std::size_t k = s.read(buf.data(), pull);
        out.insert(out.end(), buf.begin(), buf.begin() + (std::ptrdiff_t)k);
        if (k < pull) return out;
    }
}

// The schedules of the closures (tests/test_live_filter_cpu.py restates them): functions of the access index, in integers
static std::uint32_t sweep_freq(std::uint64_t k) {  // 100 Hz, about 6 % up per access, to 8 kHz
    std::uint32_t f = 100;
    for (std::uint64_t i = 0; i < k && f < 8000; ++i) f = std::min<std::uint32_t>(8000, f + f / 16 + 1);
    return f;
}

struct Log {
    std::vector<std::pair<int, std::uint64_t>> calls;
    std::function<void(rh::Controls &)> wrap(int id, std::function<void(rh::Controls &)> f) {
        return [this, id, f](rh::Controls &c) {
            calls.emplace_back(id, c.access_index());
            f(c);
        };
    }
    void write(const std::string &path) const {
        std::FILE *f = std::fopen(path.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + path);
        for (const auto &c : calls) std::fprintf(f, "%d %llu\n", c.first, (unsigned long long)c.second);
        std::fclose(f);
    }
};

// two spans of different channel counts: what a queue of sounds hands on
struct TwoFormats : rh::Source {
    std::size_t i = 0;
    std::optional<float> next() override { return i < 128 ? std::optional<float>(0.25f * (float)(i++ % 4)) : std::nullopt; }
    std::uint16_t channels() const override { return i < 64 ? 2 : 1; }
    std::uint32_t sample_rate() const override { return 48000; }
    std::optional<std::size_t> current_span_len() const override { return i < 64 ? 64 - i : 128 - i; }
    std::optional<Nanos> total_duration() const override { return std::nullopt; }
};

static void sweep_chain(rh::GpuSource &g, Log &log) {
    g.live_low_pass(100).periodic_access(Nanos(5000000), log.wrap(5, [](rh::Controls &c) { c.filter().to_low_pass(sweep_freq(c.access_index())); }));
}

int main(int argc, char **argv) {
    try {
        if (argc < 2) throw std::runtime_error("bad arguments");
        const std::string mode = argv[1];
        rh::init(0);
        if (mode == "refuse") {
            try {
                rh::GpuSource g(std::make_unique<TwoFormats>(), 256);
                g.live_low_pass(1000);
                (void)drain(g, 0);
            } catch (const rh::Error &e) {
                std::printf("%d %s\n", (int)e.status, e.what());
                return 3;
            }
            return 0;
        }
        if (mode == "args") {  // (every call returns before it touches memory: host buffers do, with the library too)
            float x[16] = {0}, y[16], tab[15] = {0}, st[8] = {1, 2, 3, 4, 5, 6, 7, 8};
            std::printf("%d\n", (int)rh_biquad_steps(y, x, 8, 2, 1, 0, 0, tab, 3, 0, st, 0, nullptr));    // period 0
            std::printf("%d\n", (int)rh_biquad_steps(y, x, 8, 2, 1, 5, 10, tab, 2, 0, st, 0, nullptr));   // 16 samples from 5 at period 10 reach 3 entries
            std::printf("%d\n", (int)rh_biquad_steps(y, x, 4, 2, 2, 5, 10, tab, 2, 9, st, 1, nullptr));   // a stride below 5 * n_steps
            std::printf("%d\n", (int)rh_biquad_steps(y, x, 8, 0, 1, 0, 4, tab, 3, 0, st, 0, nullptr));    // no channels
            std::printf("%d\n", (int)rh_biquad_steps(y, x, 8, 2, 1, 0, 8, tab, 3, 0, st, 2, nullptr));    // no such mode
            std::printf("%d\n", (int)rh_biquad_steps(y, x, 0, 2, 1, 0, 4, tab, 0, 0, st, 1, nullptr));    // an empty block: nothing happens
            for (float v : st) std::printf("%g ", v);
            std::printf("\n");
            return 0;
        }
        if (mode != "run" || argc < 5 || argc > 6) throw std::runtime_error("bad arguments");
        const std::string dir = argv[2], c = argv[3];
        const std::size_t block = (std::size_t)std::atoll(argv[4]), pull = argc == 6 ? (std::size_t)std::atoll(argv[5]) : 0;
        Log log;
        rh::GpuSource g(std::make_unique<rh::SamplesBuffer>(2, 48000, read_f32(dir + "/src_0.f32")), block);
        std::vector<float> out;
        if (c == "sweep" || c == "sweep_tp") {
            if (c == "sweep_tp") g.live_filters_time_parallel();
            sweep_chain(g, log);
        } else if (c == "switch") {
            g.live_low_pass(1000).periodic_access(Nanos(5000000), log.wrap(5, [](rh::Controls &x) {
                const std::uint64_t k = x.access_index();
                if (k < 30) x.filter().to_low_pass(1000 + 50 * (std::uint32_t)k);
                else x.filter().to_high_pass(1000 + 20 * (std::uint32_t)std::min<std::uint64_t>(k - 30, 200));
            }));
        } else if (c == "two_access") {
            g.live_low_pass(500)
                .periodic_access(Nanos(5000000), log.wrap(5, [](rh::Controls &x) { x.filter().to_low_pass_with_q(sweep_freq(x.access_index()), 0.707f); }))
                .periodic_access(Nanos(7000000), log.wrap(7, [](rh::Controls &x) { x.filter().to_low_pass(8000 - sweep_freq(x.access_index()) / 2); }));
        } else if (c == "behind_amplify") {
            g.live_amplify(1.0f).live_low_pass(300).periodic_access(Nanos(5000000), log.wrap(5, [](rh::Controls &x) {
                x.amplify().set_factor(0.5f + 0.125f * (float)(x.access_index() % 5));
                x.filter().to_low_pass(sweep_freq(x.access_index()));
            }));
        } else if (c == "fixed") {
            g.live_low_pass(200);
            rh::GpuSource plain(std::make_unique<rh::SamplesBuffer>(2, 48000, read_f32(dir + "/src_0.f32")), block);
            plain.exact_filters().low_pass(200);
            write_f32(dir + "/plain.f32", drain(plain, pull));
        } else if (c == "seek") {
            sweep_chain(g, log);
            std::FILE *sf = std::fopen((dir + "/seek.txt").c_str(), "r");
            unsigned long long at = 0;
            if (!sf || std::fscanf(sf, "%llu", &at) != 1) throw std::runtime_error("seek.txt");
            std::fclose(sf);
            for (unsigned long long k = 0; k < at; ++k) out.push_back(*g.next());
            if (!g.try_seek(Nanos(500000000))) throw std::runtime_error("try_seek refused");
        } else {
            throw std::runtime_error("unknown case " + c);
        }
        const std::vector<float> rest = drain(g, pull);
        out.insert(out.end(), rest.begin(), rest.end());
        write_f32(dir + "/out.f32", out);
        log.write(dir + "/calls.txt");
        std::printf("%zu samples %zu calls\n", out.size(), log.calls.size());
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "live_filter_test: %s\n", e.what());
        return 1;
    }
}
