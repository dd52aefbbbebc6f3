// Driver for tests/test_mix_cpu.py (linked against tests/cpp/fake_device.cpp + fake_generators.cpp + fake_noise.cpp + fake_mix.cpp:
// mix_mirror_test_fake) and tests/test_gpu_mix.py (linked against the library: mix_mirror_test): Mix and Crossfade of
// include/rodio_hip.hpp.  Test infrastructure: it prints what it sees, and the Python side holds the expected values.
//
//   mix_mirror_test run <dir> <mix|crossfade> <ca> <ra> <span_a> <cb> <rb> <span_b> <duration_ns> <block_frames> <pull> <outer_take_ns>
//       a = <dir>/a.f32, b = <dir>/b.f32 as host sources; span: -1 None (a TestSource), -2 a SamplesBuffer, > 0 a constant Some(span),
//       -3 None and ENDLESS (the samples repeat; needs outer_take_ns > 0: GpuSource(Mix).take_duration(outer_take_ns)).
//       pull 0: read() in blocks of block_frames frames; pull 1: next(), one sample at a time, asking the trait before every sample:
//       <dir>/lower.u64 receives size_hint().lower at every position; prints "spans_some <n>" (positions where current_span_len() was
//       Some), "uppers_some <n>", "duration <ns|-1>", "seek <0|1>", "format <ch> <rate>", "uploaded <n>".  The samples go to <dir>/out.f32.
//   mix_mirror_test generators <dir>
//       SineWave(440).mix(WhiteUniform(48000, seed 9)) under take_duration(100 ms) through a GpuSource (<dir>/dev.f32; "uploaded <n>" of
//       the chain and of the Mix's inputs, "generated <n>"), the same Mix pulled by next() (<dir>/twin.f32), and the host's own
//       next() of the two generators, added (<dir>/host.f32)
//   mix_mirror_test mixer <dir>
//       GpuMixer(2, 48000).add(Mix(a.f32 stereo 48 kHz, b.f32 mono 44.1 kHz)) (<dir>/mix.f32) and the same mixer over the Mix's collected
//       samples as a host source (<dir>/host.f32); and a Mix of generators inside a chain, added bare: "uploaded_gen <n>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rodio_hip.hpp"

namespace rh = rodio_hip;
using Nanos = rh::Nanos;

static std::vector<float> read_f32(const std::string &path) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("open " + path);
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> v((std::size_t)bytes / 4);
    if (std::fread(v.data(), 4, v.size(), f) != v.size()) throw std::runtime_error("read " + path);
    std::fclose(f);
    return v;
}
template <typename T>
static void write_vec(const std::string &path, const std::vector<T> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) throw std::runtime_error("write " + path);
    std::fclose(f);
}

// benches/shared.rs TestSource (span None, the trait's default size_hint), or a source that reports a constant span; endless: the samples repeat
class VecSource : public rh::Source {
public:
    VecSource(std::uint16_t ch, std::uint32_t rate, std::vector<float> x, long span, bool endless = false) : ch_(ch), rate_(rate), x_(std::move(x)), span_(span), endless_(endless) {}
    std::optional<float> next() override {
        if (i_ == x_.size()) {
            if (!endless_ || x_.empty()) return std::nullopt;
            i_ = 0;
        }
        return x_[i_++];
    }
    std::optional<std::size_t> current_span_len() const override { return span_ > 0 ? std::optional<std::size_t>((std::size_t)span_) : std::nullopt; }
    std::uint16_t channels() const override { return ch_; }
    std::uint32_t sample_rate() const override { return rate_; }
    rh::SizeHint size_hint() const override {  // (the oracle's spanned source counts its samples; its TestSource answers the trait's default)
        return span_ > 0 ? rh::SizeHint{x_.size() - i_, x_.size() - i_} : rh::SizeHint{};
    }
    std::optional<Nanos> total_duration() const override {  // (... and knows its length)
        if (span_ <= 0) return std::nullopt;
        return Nanos((std::int64_t)(1000000000ull * (std::uint64_t)x_.size() / rate_ / ch_));
    }

private:
    std::uint16_t ch_;
    std::uint32_t rate_;
    std::vector<float> x_;
    long span_;
    bool endless_;
    std::size_t i_ = 0;
};

static rh::BoxSource host_source(const std::string &path, std::uint16_t ch, std::uint32_t rate, long span) {
    std::vector<float> x = read_f32(path);
    if (span == -2) return std::make_unique<rh::SamplesBuffer>(ch, rate, std::move(x));
    return std::make_unique<VecSource>(ch, rate, std::move(x), span, span == -3);
}

static std::vector<float> collect(rh::Source &s, std::size_t block) {
    std::vector<float> out, buf(block);
    for (;;) {
        const std::size_t k = s.read(buf.data(), block);
        out.insert(out.end(), buf.begin(), buf.begin() + (std::ptrdiff_t)k);
        if (k < block) return out;
    }
}

int main(int argc, char **argv) {
    try {
        if (argc < 3) throw std::runtime_error("bad arguments");
        const std::string mode = argv[1], dir = argv[2];
        rh::init(0);
        if (mode == "run" && argc == 14) {
            const bool cross = std::string(argv[3]) == "crossfade";
            const std::uint16_t ca = (std::uint16_t)std::atoi(argv[4]), cb = (std::uint16_t)std::atoi(argv[7]);
            const std::uint32_t ra = (std::uint32_t)std::atoll(argv[5]), rb = (std::uint32_t)std::atoll(argv[8]);
            const long span_a = std::atol(argv[6]), span_b = std::atol(argv[9]);
            const Nanos d(std::atoll(argv[10])), outer(std::atoll(argv[13]));
            const std::size_t block_frames = (std::size_t)std::atoll(argv[11]);
            const int pull = std::atoi(argv[12]);
            rh::BoxSource a = host_source(dir + "/a.f32", ca, ra, span_a), b = host_source(dir + "/b.f32", cb, rb, span_b);
            std::unique_ptr<rh::Mix> m;
            if (cross) m = rh::take_crossfade_with(std::move(a), std::move(b), d, block_frames);
            else m = rh::mix(std::move(a), std::move(b), block_frames);
            rh::Mix *const mx = m.get();
            std::printf("format %u %u\n", (unsigned)mx->channels(), (unsigned)mx->sample_rate());
            std::printf("duration %lld\n", mx->total_duration() ? (long long)mx->total_duration()->count() : -1ll);
            std::vector<float> out;
            if (outer.count() > 0) {  // the Mix as the head of a chain
                rh::GpuSource g(std::move(m), block_frames);
                g.take_duration(outer);
                out = collect(g, block_frames * ca);
                std::printf("uploaded %llu\n", (unsigned long long)(g.timing().uploaded_samples));
            } else if (pull == 0) {
                out = collect(*mx, block_frames * ca);
            } else {
                std::vector<std::uint64_t> lower;
                std::size_t spans_some = 0, uppers_some = 0;
                for (;;) {
                    const rh::SizeHint h = mx->size_hint();
                    lower.push_back(h.lower);
                    uppers_some += h.upper.has_value();
                    spans_some += mx->current_span_len().has_value();
                    const std::optional<float> v = mx->next();
                    if (!v) break;
                    out.push_back(*v);
                }
                write_vec(dir + "/lower.u64", lower);
                std::printf("spans_some %zu\nuppers_some %zu\n", spans_some, uppers_some);
            }
            if (outer.count() <= 0) std::printf("seek %d\nuploaded %llu\n", (int)mx->try_seek(Nanos(1000000)), (unsigned long long)mx->uploaded_samples());
            write_vec(dir + "/out.f32", out);
            return 0;
        }
        if (mode == "generators" && argc == 3) {
            const Nanos take(100000000);
            auto make = [] { return std::make_unique<rh::Mix>(std::make_unique<rh::SineWave>(440.0f), std::make_unique<rh::WhiteUniform>(48000, 9), 4096); };
            {
                rh::GpuSource g(make(), 4096);
                g.take_duration(take);
                write_vec(dir + "/dev.f32", collect(g, 1000));
                rh::Mix &mx = dynamic_cast<rh::Mix &>(g.inner());
                std::printf("uploaded %llu %llu\ngenerated %llu %llu\n", (unsigned long long)g.timing().uploaded_samples, (unsigned long long)mx.uploaded_samples(),
                            (unsigned long long)g.timing().generated_samples, (unsigned long long)mx.generated_samples());
            }
            std::vector<float> twin, host;
            auto t = make();
            rh::SineWave s(440.0f);
            rh::WhiteUniform w(48000, 9);
            for (int i = 0; i < 4800; ++i) {
                twin.push_back(*t->next());
                host.push_back(*s.next() + *w.next());
            }
            write_vec(dir + "/twin.f32", twin);
            write_vec(dir + "/host.f32", host);
            return 0;
        }
        if (mode == "mixer" && argc == 3) {
            auto make = [&] { return std::make_unique<rh::Mix>(host_source(dir + "/a.f32", 2, 48000, -1), host_source(dir + "/b.f32", 1, 44100, -1), 4096); };
            std::vector<float> collected = collect(*make(), 4096);
            rh::GpuMixer::Options opt;
            rh::GpuMixer a(2, 48000, opt), b(2, 48000, opt), c(2, 48000, opt);
            a.add(make(), 0.5f);
            b.add(std::make_unique<VecSource>(2, 48000, collected, -1), 0.5f);
            write_vec(dir + "/mix.f32", collect(a, 4096));
            write_vec(dir + "/host.f32", collect(b, 4096));
            write_vec(dir + "/collected.f32", collected);
            auto chain = std::make_unique<rh::GpuSource>(std::make_unique<rh::Mix>(std::make_unique<rh::SineWave>(440.0f), std::make_unique<rh::WhiteUniform>(48000, 9), 4096), 4096);
            chain->take_duration(Nanos(50000000)).amplify(0.5f);
            c.add(std::move(chain), 1.0f);
            write_vec(dir + "/gen.f32", collect(c, 4096));
            std::printf("uploaded_gen %llu\n", (unsigned long long)c.timing().uploaded_samples);
            return 0;
        }
        throw std::runtime_error("bad arguments");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
