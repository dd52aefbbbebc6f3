// Driver for tests/test_live_params_cpu.py (linked against tests/cpp/fake_device.cpp + fake_live.cpp: live_test_fake) and
// tests/test_gpu_live.py (linked against the library: live_test): chains of include/rodio_hip.hpp with adjustable stages and
// periodic_access(), as rodio's Player / SpatialPlayer build them.  Test infrastructure: the expected values come from the Python side.
//
//   live_test run <dir> <case> <block_frames>
//       <dir>/src_<i>.f32 -> <dir>/out.f32, <dir>/calls.txt (one line per closure call: "<access> <index>"), and for `seek`
//       <dir>/plain.f32 (the same pulls through the chain with a fixed amplify(1.0))
//       cases: player     2 ch 44100, live_amplify(1) -> periodic_access(5 ms, volume(k))
//              lowpass    2 ch 44100, live_amplify(1) -> low_pass(200) (reference order) -> periodic_access(5 ms, volume(k))
//              seek       player, try_seek(500 ms) after <dir>/seek.txt samples
//              spatial    2 ch 48000, live_spatial -> periodic_access(10 ms, emitter(k)) -> live_amplify(1) -> periodic_access(5 ms, volume(k))
//              spatial_mixer  spatial, handed to GpuMixer(2, 48000) on the device with src_1, src_2 (plain stereo 48 kHz)
//              stereo_access  periodic.rs:143-171 (SamplesBuffer 2 ch 1 Hz, 1 s); fast_access  periodic.rs:173-181 (1 ch 1 Hz, 5 ms)
//                         (out.f32: the samples; counts.txt: calls after every next(), the None included)
//   live_test refuse [cv]          live_amplify -> convert_channels -> periodic_access (cv: mono live_amplify -> periodic_access ->
//                                  live_channel_volume({1, 1})): exit 3 with RH_ERR_UNSUPPORTED
//   live_test steps <seconds> <block_frames> <player|spatial>   the steps a long stream keeps (see the mode)
//   live_test hints <dir> <block_frames>
//       <dir>/src_0.f32 (2 ch 44100) through amplify -> low_pass and through live_amplify -> low_pass -> periodic_access: size_hint,
//       current_span_len and total_duration before every 1000th sample, both chains (<dir>/hints_plain.txt, hints_live.txt)
//   live_test launches <block_frames>  (fake build) stepped launches per block of the spatial chain
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rodio_hip.hpp"

namespace rh = rodio_hip;
using Nanos = rh::Nanos;

extern "C" __attribute__((weak)) uint64_t fake_live_launches(void);  // (fake_live.cpp only)

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
static std::vector<float> drain(rh::Source &s) {
    std::vector<float> out;
    while (std::optional<float> v = s.next()) out.push_back(*v);
    return out;
}

// The schedules of the closures (tests/test_live_params_cpu.py restates them): functions of the access index
static void volume(rh::Controls &c) {
    const std::uint64_t k = c.access_index();
    if (k % 7 == 3) c.amplify().set_factor(0.0f);
    else if (k % 5 == 1) c.amplify().set_factor(-0.75f);
    else if (k % 11 == 4) c.amplify().set_log_factor(-6.0f);
    else c.amplify().set_factor(0.5f + 0.125f * (float)(k % 5));
}
static const float kLeft[3] = {-1.0f, 0.0f, 0.0f}, kRight[3] = {1.0f, 0.0f, 0.0f};
static void emitter(std::uint64_t k, float e[3]) {
    e[0] = (float)(k % 17) * 0.25f - 2.0f;
    e[1] = 1.0f + (float)(k % 5) * 0.5f;
    e[2] = 0.0f;
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

static std::unique_ptr<rh::GpuSource> spatial_chain(rh::BoxSource src, std::size_t block, Log &log) {
    auto g = std::make_unique<rh::GpuSource>(std::move(src), block);
    float e0[3];
    emitter(0, e0);
    g->live_spatial(e0, kLeft, kRight)
        .periodic_access(Nanos(10000000), log.wrap(10, [](rh::Controls &c) {
            float e[3];
            emitter(c.access_index(), e);
            c.spatial().set_positions(e, kLeft, kRight);
        }))
        .live_amplify(1.0f)
        .periodic_access(Nanos(5000000), log.wrap(5, volume));
    return g;
}

int main(int argc, char **argv) {
    try {
        if (argc < 2) throw std::runtime_error("bad arguments");
        const std::string mode = argv[1];
        rh::init(0);
        if (mode == "refuse") {
            const bool cv = argc == 3 && std::string(argv[2]) == "cv";
            rh::GpuSource g(std::make_unique<rh::SamplesBuffer>(cv ? 1 : 2, 44100, std::vector<float>(64, 0.5f)), 256);
            try {
                if (cv) {
                    g.live_amplify(1.0f).periodic_access(Nanos(5000000), volume);
                    g.live_channel_volume({1.0f, 1.0f});
                } else {
                    g.live_amplify(1.0f).convert_channels(1);
                    g.periodic_access(Nanos(5000000), volume);
                }
            } catch (const rh::Error &e) {
                std::printf("%d %s\n", (int)e.status, e.what());
                return 3;
            }
            return 0;
        }
        if (mode == "launches" && argc == 3) {
            if (!fake_live_launches) throw std::runtime_error("launches: the fake build only");
            const std::size_t block = (std::size_t)std::atoll(argv[2]);
            Log log;
            auto g = spatial_chain(std::make_unique<rh::SamplesBuffer>(2, 48000, std::vector<float>(2 * block * 4, 0.25f)), block, log);
            const std::uint64_t before = fake_live_launches();
            const std::vector<float> out = drain(*g);
            const std::uint64_t blocks = g->timing().blocks, launches = fake_live_launches() - before;
            std::printf("%zu samples %llu blocks %llu launches %llu\n", out.size(), (unsigned long long)blocks, (unsigned long long)launches,
                        (unsigned long long)(launches + blocks - 1) / blocks);
            return 0;
        }
        if (mode == "steps" && argc == 5) {
            // live_test steps <seconds> <block_frames> <chain: player | spatial>: a factor (and emitter) that changes at every access, over a long
            // stream of 44.1 kHz stereo; prints the samples, the closure calls and the most steps the chain held at any point
            const std::size_t secs = (std::size_t)std::atoll(argv[2]), block = (std::size_t)std::atoll(argv[3]);
            const bool spatial = std::string(argv[4]) == "spatial";
            std::vector<float> x(2 * 44100 * secs);
            for (std::size_t i = 0; i < x.size(); ++i) x[i] = (float)(i % 200) / 100.0f - 1.0f;
            Log log;
            std::unique_ptr<rh::GpuSource> g;
            if (spatial) {
                g = spatial_chain(std::make_unique<rh::SamplesBuffer>(2, 44100, std::move(x)), block, log);
            } else {
                g = std::make_unique<rh::GpuSource>(std::make_unique<rh::SamplesBuffer>(2, 44100, std::move(x)), block);
                g->live_amplify(1.0f).periodic_access(Nanos(5000000), [](rh::Controls &c) { c.amplify().set_factor((float)(c.access_index() % 1000)); });
            }
            std::size_t n = 0, most = 0;
            while (g->next()) {
                if (++n % 4096 == 0) most = std::max(most, g->periodic_steps_held());
            }
            std::printf("%zu samples %llu calls %zu steps\n", n, (unsigned long long)g->periodic_calls(), std::max(most, g->periodic_steps_held()));
            return 0;
        }
        if (mode == "hints" && argc == 4) {
            const std::string dir = argv[2];
            const std::size_t block = (std::size_t)std::atoll(argv[3]);
            for (int live = 0; live < 2; ++live) {
                rh::GpuSource g(std::make_unique<rh::SamplesBuffer>(2, 44100, read_f32(dir + "/src_0.f32")), block);
                if (live) g.live_amplify(1.0f).low_pass(200).periodic_access(Nanos(5000000), volume);
                else g.amplify(1.0f).low_pass(200);
                std::FILE *f = std::fopen((dir + (live ? "/hints_live.txt" : "/hints_plain.txt")).c_str(), "w");
                for (std::size_t i = 0;; ++i) {
                    if (i % 1000 == 0 || i < 4) {
                        const rh::SizeHint h = g.size_hint();
                        const std::optional<std::size_t> sp = g.current_span_len();
                        const std::optional<Nanos> d = g.total_duration();
                        std::fprintf(f, "%zu %zu %lld %lld %lld\n", i, h.lower, h.upper ? (long long)*h.upper : -1LL, sp ? (long long)*sp : -1LL, d ? (long long)d->count() : -1LL);
                    }
                    if (!g.next()) break;
                }
                std::fclose(f);
            }
            return 0;
        }
        if (mode != "run" || argc != 5) throw std::runtime_error("bad arguments");
        const std::string dir = argv[2], c = argv[3];
        const std::size_t block = (std::size_t)std::atoll(argv[4]);
        Log log;
        std::vector<float> out;
        if (c == "stereo_access" || c == "fast_access") {
            const bool st = c == "stereo_access";
            rh::GpuSource g(std::make_unique<rh::SamplesBuffer>(st ? 2 : 1, 1, std::vector<float>{10.0f, -10.0f, 10.0f, -10.0f, 20.0f, -20.0f}), block);
            g.periodic_access(Nanos(st ? 1000000000 : 5000000), log.wrap(0, [](rh::Controls &) {}));
            std::FILE *f = std::fopen((dir + "/counts.txt").c_str(), "w");
            std::fprintf(f, "%llu\n", (unsigned long long)g.periodic_calls());
            for (int k = 0; k < 7; ++k) {
                const std::optional<float> v = g.next();
                if (v) out.push_back(*v);
                std::fprintf(f, "%llu\n", (unsigned long long)g.periodic_calls());
                if (!v) break;
            }
            std::fclose(f);
        } else if (c == "player" || c == "lowpass" || c == "seek") {
            for (int live = c == "seek" ? 0 : 1; live < 2; ++live) {
                rh::GpuSource g(std::make_unique<rh::SamplesBuffer>(2, 44100, read_f32(dir + "/src_0.f32")), block);
                if (!live) g.amplify(1.0f);
                else if (c == "lowpass") g.exact_filters().live_amplify(1.0f).low_pass(200).periodic_access(Nanos(5000000), log.wrap(5, volume));
                else g.live_amplify(1.0f).periodic_access(Nanos(5000000), log.wrap(5, volume));
                std::vector<float> o;
                if (c == "seek") {
                    std::FILE *sf = std::fopen((dir + "/seek.txt").c_str(), "r");
                    unsigned long long at = 0;
                    if (!sf || std::fscanf(sf, "%llu", &at) != 1) throw std::runtime_error("seek.txt");
                    std::fclose(sf);
                    for (unsigned long long k = 0; k < at; ++k) o.push_back(*g.next());
                    if (!g.try_seek(Nanos(500000000))) throw std::runtime_error("try_seek refused");
                }
                const std::vector<float> rest = drain(g);
                o.insert(o.end(), rest.begin(), rest.end());
                if (live) out = o;
                else write_f32(dir + "/plain.f32", o);
            }
        } else if (c == "spatial") {
            auto g = spatial_chain(std::make_unique<rh::SamplesBuffer>(2, 48000, read_f32(dir + "/src_0.f32")), block, log);
            out = drain(*g);
        } else if (c == "spatial_mixer") {
            rh::GpuMixer::Options opt;
            opt.block_frames = block;
            rh::GpuMixer mixer(2, 48000, opt);
            auto g = spatial_chain(std::make_unique<rh::SamplesBuffer>(2, 48000, read_f32(dir + "/src_0.f32")), block, log);
            mixer.add(std::move(g), 1.0f, rh::GpuMixer::Filter{-1, 0, 0.5f});
            for (int i = 1; i < 3; ++i) mixer.add(std::make_unique<rh::SamplesBuffer>(2, 48000, read_f32(dir + "/src_" + std::to_string(i) + ".f32")), 1.0f);
            out = drain(mixer);
        } else {
            throw std::runtime_error("unknown case " + c);
        }
        write_f32(dir + "/out.f32", out);
        log.write(dir + "/calls.txt");
        std::printf("%zu samples %zu calls\n", out.size(), log.calls.size());
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "live_test: %s\n", e.what());
        return 1;
    }
}
