// Driver for tests/test_generators_cpu.py (linked against tests/cpp/fake_device.cpp + fake_generators.cpp: generators_mirror_test_fake)
// and tests/test_gpu_generators.py (linked against the library: generators_mirror_test): the generators of include/rodio_hip.hpp.
// Test infrastructure: it prints what it sees, and the Python side holds the expected values.
//
//   generators_mirror_test trait
//       one line per question: "<name> <value>" -- size_hint, total_duration, span, channels, rate and try_seek of every generator
//   generators_mirror_test chain <out.f32> <block_frames>
//       GpuSource(SignalGenerator(44100, 441.7, Triangle)): 100000 samples by read(), a try_seek(2.5 s), 50000 more, to <out.f32>;
//       prints "uploaded <n>" and "generated <n>" of the chain's Timing
//   generators_mirror_test mixer <dir>
//       GpuMixer(2, 48000) of 8 generators added bare (<dir>/gen.f32) and of the same samples from continuous host sources (<dir>/host.f32),
//       48000 frames each; prints "uploaded_gen <n>" and "uploaded_host <n>" of the two mixers' Timing
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rodio_hip.hpp"

namespace rh = rodio_hip;
using Nanos = rh::Nanos;

static void hint(const char *name, const rh::Source &s) {
    const rh::SizeHint h = s.size_hint();
    std::printf("%s.size_hint %llu %lld\n", name, (unsigned long long)h.lower, h.upper ? (long long)*h.upper : -1ll);
    const auto d = s.total_duration();
    std::printf("%s.total_duration %lld\n", name, d ? (long long)d->count() : -1ll);
    std::printf("%s.span %lld\n", name, s.current_span_len() ? (long long)*s.current_span_len() : -1ll);
    std::printf("%s.format %u %u\n", name, (unsigned)s.channels(), (unsigned)s.sample_rate());
}

static void write_f32(const std::string &path, const std::vector<float> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), 4, v.size(), f) != v.size()) throw std::runtime_error("write " + path);
    std::fclose(f);
}

// The host's samples as a continuous source (no spans, endless size_hint): what a generator is, minus the device path.
class Continuous : public rh::Source {
public:
    Continuous(std::uint32_t rate, std::vector<float> x) : rate_(rate), x_(std::move(x)) {}
    std::optional<float> next() override { return i_ < x_.size() ? std::optional<float>(x_[i_++]) : std::nullopt; }
    std::uint16_t channels() const override { return 1; }
    std::uint32_t sample_rate() const override { return rate_; }

private:
    std::uint32_t rate_;
    std::vector<float> x_;
    std::size_t i_ = 0;
};

struct Tone {
    std::uint32_t rate;
    float freq;
    rh::Function fn;
};
static const Tone kTones[8] = {{48000, 440.0f, rh::Function::Triangle}, {44100, 1000.0f, rh::Function::Square}, {48000, 20.0f, rh::Function::Sawtooth},
                               {44100, 3999.0f, rh::Function::Triangle}, {48000, 12345.0f, rh::Function::Square}, {44100, 55.0f, rh::Function::Sawtooth},
                               {48000, 7000.5f, rh::Function::Triangle}, {44100, 261.6f, rh::Function::Square}};

int main(int argc, char **argv) {
    try {
        if (argc < 2) throw std::runtime_error("bad arguments");
        const std::string mode = argv[1];
        rh::init(0);
        if (mode == "trait") {
            rh::SignalGenerator g(2000, 500.0f, rh::Function::Square);
            hint("signal", g);
            rh::SineWave sw(440.0f);
            rh::SquareWave qw(440.0f);
            rh::TriangleWave tw(440.0f);
            rh::SawtoothWave aw(440.0f);
            hint("sine", sw), hint("square", qw), hint("triangle", tw), hint("sawtooth", aw);
            for (rh::SignalGenerator *x : {(rh::SignalGenerator *)&sw, (rh::SignalGenerator *)&qw, (rh::SignalGenerator *)&tw, (rh::SignalGenerator *)&aw, &g}) {
                const bool ok = x->try_seek(Nanos(123456789));
                std::printf("seek %d %.9g\n", (int)ok, (double)x->phase());
            }
            try {
                rh::SignalGenerator bad(48000, 0.0f, rh::Function::Sine);
                std::printf("refused 0\n");
            } catch (const rh::Error &e) {
                std::printf("refused %d\n", (int)e.status);
            }
            rh::Chirp c(48000, 20.0f, 20000.0f, Nanos(1500000001));
            hint("chirp", c);
            for (int k = 0; k < 10; ++k) (void)c.next();
            hint("chirp_after10", c);
            const bool ok = c.try_seek(Nanos(1000000000));
            std::printf("chirp_seek %d %llu\n", (int)ok, (unsigned long long)c.elapsed_samples());
            hint("chirp_sought", c);
            (void)c.try_seek(Nanos(100000000000ll));
            hint("chirp_end", c);
            std::printf("chirp_next_at_end %d\n", (int)c.next().has_value());
            rh::Chirp big(48000, 100.0f, 200.0f, Nanos(200000ll * 1000000000ll));
            big.seek_sample((1ull << 32) + 7);
            hint("chirp_big", big);
            return 0;
        }
        if (mode == "chain" && argc == 4) {
            rh::GpuSource g(std::make_unique<rh::SignalGenerator>(44100, 441.7f, rh::Function::Triangle), (std::size_t)std::atoll(argv[3]));
            std::vector<float> out(150000);
            std::size_t k = g.read(out.data(), 100000);
            if (!g.try_seek(Nanos(2500000000ll))) throw std::runtime_error("try_seek");
            k += g.read(out.data() + k, 50000);
            if (k != out.size()) throw std::runtime_error("short read");
            write_f32(argv[2], out);
            hint("chain", g);
            std::printf("uploaded %llu\ngenerated %llu\n", (unsigned long long)g.timing().uploaded_samples, (unsigned long long)g.timing().generated_samples);
            return 0;
        }
        if (mode == "mixer" && argc == 3) {
            const std::string dir = argv[2];
            const std::size_t frames = 48000;
            rh::GpuMixer::Options opt;
            rh::GpuMixer a(2, 48000, opt), b(2, 48000, opt);
            for (const Tone &t : kTones) {
                a.add(std::make_unique<rh::SignalGenerator>(t.rate, t.freq, t.fn), 0.125f);
                rh::SignalGenerator host(t.rate, t.freq, t.fn);  // the same samples, computed on the host (bit-exact functions)
                std::vector<float> x(frames * 2);
                for (float &v : x) v = *host.next();
                b.add(std::make_unique<Continuous>(t.rate, std::move(x)), 0.125f);
            }
            std::vector<float> ya(frames * 2), yb(frames * 2);
            const std::size_t na = a.read(ya.data(), ya.size()), nb = b.read(yb.data(), yb.size());
            if (na != ya.size() || nb != yb.size()) throw std::runtime_error("short mix");
            write_f32(dir + "/gen.f32", ya);
            write_f32(dir + "/host.f32", yb);
            std::printf("uploaded_gen %llu\nuploaded_host %llu\n", (unsigned long long)a.timing().uploaded_samples, (unsigned long long)b.timing().uploaded_samples);
            return 0;
        }
        throw std::runtime_error("bad arguments");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
