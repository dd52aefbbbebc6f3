// Driver for tests/test_noise_cpu.py (linked against tests/cpp/fake_device.cpp + fake_noise.cpp: noise_mirror_test_fake) and
// tests/test_gpu_noise.py (linked against the library: noise_mirror_test): the noise sources of include/rodio_hip.hpp.
// Test infrastructure: it prints what it sees, and the Python side holds the expected values.
//
//   noise_mirror_test trait
//       one line per question: size_hint, total_duration, span, format, std_dev / mean, try_seek and the refusals
//   noise_mirror_test follow <kind> <rate> <seed> <dir>
//       the same schedule of fill_device / next() / try_seek on one source (<dir>/mixed.f32: the device's blocks copied back) and next()
//       alone on a twin (<dir>/host.f32): the host's state follows the device's
//   noise_mirror_test serial <kind> <rate> <seed> <n> <dir>
//       n samples of host next() (rodio's serial f32 recurrence for the integrators) to <dir>/f32.bin, and for an integrator the same
//       recurrence in f64 on the same white samples, with the stream's f32 leak and scale, to <dir>/f64.bin
//   noise_mirror_test chain <kind> <out.f32> <block_frames>
//       GpuSource(kind, 48000, seed 77): 100000 samples by read(), a try_seek(1 s), 50000 more, to <out.f32>; prints the source's k right
//       after the seek ("k_at_seek <k>"), and "uploaded <n>" and "generated <n>" of the chain's Timing
//   noise_mirror_test mixer <dir>
//       GpuMixer(2, 48000) of 9 noise sources added bare (<dir>/gen.f32) and of the same samples, made by twins on the device and copied
//       back, from continuous host sources (<dir>/host.f32), 48000 frames each; prints "uploaded_gen <n>" and "uploaded_host <n>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static const char *kNames[9] = {"WhiteUniform", "WhiteTriangular", "WhiteGaussian", "Pink", "Blue", "Violet", "Brownian", "Red", "Velvet"};

static std::unique_ptr<rh::NoiseSource> make(int kind, std::uint32_t rate, std::uint64_t seed) {
    return std::make_unique<rh::NoiseSource>((rh::NoiseKind)kind, rate, seed);
}

// the next n samples of `s` through its device path, copied back
static void device_block(rh::NoiseSource &s, std::size_t n, std::vector<float> &out) {
    rh::detail::DeviceBuf d(n);
    s.fill_device(d.get(), n, nullptr);
    std::vector<float> h(n);
    rh::check(rh_memcpy_d2h(h.data(), d.get(), n * sizeof(float), nullptr), "rh_memcpy_d2h");
    rh::check(rh_stream_synchronize(nullptr), "rh_stream_synchronize");
    out.insert(out.end(), h.begin(), h.end());
}

int main(int argc, char **argv) {
    try {
        if (argc < 2) throw std::runtime_error("bad arguments");
        const std::string mode = argv[1];
        rh::init(0);
        if (mode == "trait") {
            for (int kind = 0; kind < 9; ++kind) {
                auto s = make(kind, 44100, 5);
                hint(kNames[kind], *s);
                std::printf("%s.seek %d\n", kNames[kind], (int)s->try_seek(Nanos(1000000000)));
            }
            rh::WhiteUniform wu(44100);
            rh::WhiteTriangular wt(44100, 1);
            rh::WhiteGaussian wg(44100, 1);
            std::printf("std_dev %.9g %.9g %.9g\nmean %.9g\n", (double)wu.std_dev(), (double)wt.std_dev(), (double)wg.std_dev(), (double)wg.mean());
            rh::Pink p(48000);
            rh::Blue b(48000);
            rh::Violet v(48000);
            rh::Brownian br(48000);
            rh::Red r(48000);
            rh::Velvet ve(48000);
            rh::Velvet vd(48000, 1000u, 9);
            std::printf("entropy_seeds_differ %d\n", (int)(rh::WhiteUniform(48000).state()[0] != wu.state()[0] || rh::WhiteUniform(48000).state()[1] != wu.state()[1]));
            std::printf("velvet_grid %u %u\n", ve.state()[5], vd.state()[5]);
            for (int bad = 0; bad < 3; ++bad) {
                try {
                    if (bad == 0) rh::Velvet x(48000, 0u, 1);
                    if (bad == 1) rh::Red x(0, 1);
                    if (bad == 2) rh::NoiseSource x((rh::NoiseKind)9, 48000, 1);
                    std::printf("refused %d 0\n", bad);
                } catch (const rh::Error &e) {
                    std::printf("refused %d %d\n", bad, (int)e.status);
                }
            }
            return 0;
        }
        if (mode == "follow" && argc == 6) {
            const int kind = std::atoi(argv[2]);
            const std::uint32_t rate = (std::uint32_t)std::atoll(argv[3]);
            const std::uint64_t seed = std::strtoull(argv[4], nullptr, 10);
            const std::string dir = argv[5];
            auto a = make(kind, rate, seed), b = make(kind, rate, seed);
            std::vector<float> ya, yb;
            auto host = [](rh::NoiseSource &s, std::size_t n, std::vector<float> &out) {
                for (std::size_t i = 0; i < n; ++i) out.push_back(*s.next());
            };
            device_block(*a, 1000, ya), host(*b, 1000, yb);
            host(*a, 500, ya), host(*b, 500, yb);
            device_block(*a, 3000, ya), host(*b, 3000, yb);
            (void)a->try_seek(Nanos(250000000)), (void)b->try_seek(Nanos(250000000));
            device_block(*a, 700, ya), host(*b, 700, yb);
            host(*a, 300, ya), host(*b, 300, yb);
            write_f32(dir + "/mixed.f32", ya);
            write_f32(dir + "/host.f32", yb);
            std::printf("k %llu %llu\n", (unsigned long long)a->k(), (unsigned long long)b->k());
            return 0;
        }
        if (mode == "serial" && argc == 7) {
            const int kind = std::atoi(argv[2]);
            const std::uint32_t rate = (std::uint32_t)std::atoll(argv[3]);
            const std::uint64_t seed = std::strtoull(argv[4], nullptr, 10);
            const std::size_t n = (std::size_t)std::atoll(argv[5]);
            const std::string dir = argv[6];
            auto s = make(kind, rate, seed);
            float leak, scale;
            std::memcpy(&leak, &s->state()[5], 4), std::memcpy(&scale, &s->state()[6], 4);
            std::vector<float> y(n);
            for (float &v : y) v = *s->next();
            write_f32(dir + "/f32.bin", y);
            if (kind == RH_NOISE_RED || kind == RH_NOISE_BROWNIAN) {
                std::vector<double> z(n);
                double acc = 0.0;
                for (std::size_t i = 0; i < n; ++i) {
                    const std::uint64_t h = rh::detail::noise::hash(seed, i);
                    const double w = kind == RH_NOISE_BROWNIAN ? (double)rh::detail::noise::gaussian(h) : (double)rh::detail::noise::u1(h);
                    acc = acc * (double)leak + w;
                    z[i] = acc * (double)scale;
                }
                FILE *f = std::fopen((dir + "/f64.bin").c_str(), "wb");
                if (!f || std::fwrite(z.data(), 8, n, f) != n) throw std::runtime_error("write f64");
                std::fclose(f);
            }
            return 0;
        }
        if (mode == "chain" && argc == 5) {
            const int kind = std::atoi(argv[2]);
            rh::GpuSource g(make(kind, 48000, 77), (std::size_t)std::atoll(argv[4]));
            std::vector<float> out(150000);
            std::size_t k = g.read(out.data(), 100000);
            if (!g.try_seek(Nanos(1000000000ll))) throw std::runtime_error("try_seek");
            std::printf("k_at_seek %llu\n", (unsigned long long)dynamic_cast<rh::NoiseSource &>(g.inner()).k());  // (what the chain pulled ahead is gone)
            k += g.read(out.data() + k, 50000);
            if (k != out.size()) throw std::runtime_error("short read");
            write_f32(argv[3], out);
            hint("chain", g);
            std::printf("uploaded %llu\ngenerated %llu\n", (unsigned long long)g.timing().uploaded_samples, (unsigned long long)g.timing().generated_samples);
            return 0;
        }
        if (mode == "mixer" && argc == 3) {
            const std::string dir = argv[2];
            const std::size_t frames = 48000;
            rh::GpuMixer::Options opt;
            rh::GpuMixer a(2, 48000, opt), b(2, 48000, opt);
            for (int kind = 0; kind < 9; ++kind) {
                const std::uint32_t rate = kind % 2 ? 44100 : 48000;
                a.add(make(kind, rate, 1000 + kind), 0.125f);
                auto twin = make(kind, rate, 1000 + kind);  // the same samples, made on the device and copied back
                std::vector<float> x;
                device_block(*twin, frames * 2, x);
                b.add(std::make_unique<Continuous>(rate, std::move(x)), 0.125f);
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
