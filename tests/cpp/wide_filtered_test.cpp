// Driver for tests/test_wide_filtered_cpu.py (linked against tests/cpp/fake_device.cpp + fake_widemix_filtered.cpp:
// wide_filtered_test_fake): GpuMixer of more than two channels with Options::wide_filters -- filtered and plain continuous sources in
// one-launch generations (rh_wide_mix_block_filtered), a late join, sources that end inside a block.  Test infrastructure: it writes
// what it sees, and the Python side holds the expected values.
//
//   wide_filtered_test <dir> <n_first> <n_late> <channels> <rate> <block_frames> <pull_first> <wide_filters 0|1>
//       <dir>/spec.txt: a line `ch rate gain kind freq q` per source (kind -1 none, 0 low_pass, 1 high_pass), <dir>/src_<i>.f32 its samples
//       (a TestSource: current_span_len() None, the trait's default size_hint()).  The first n_first sources are added before the first
//       sample, the n_late others after pull_first samples.  <dir>/out.f32: every sample; <dir>/hints.i64: size_hint() (lower, upper or
//       -1) in front of every sample and behind the last; <dir>/stats.txt: the mixer's counters as JSON.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rodio_hip.hpp"

namespace rh = rodio_hip;

class TestSource : public rh::SamplesBuffer {  // benches/shared.rs:14-21
public:
    using rh::SamplesBuffer::SamplesBuffer;
    std::optional<std::size_t> current_span_len() const override { return std::nullopt; }
    rh::SizeHint size_hint() const override { return rh::SizeHint{}; }
};

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

int main(int argc, char **argv) {
    try {
        if (argc != 9) throw std::runtime_error("bad arguments");
        const std::string dir = argv[1];
        const int n_first = std::atoi(argv[2]), n_late = std::atoi(argv[3]);
        const std::uint16_t channels = (std::uint16_t)std::atoi(argv[4]);
        const std::uint32_t rate = (std::uint32_t)std::atoll(argv[5]);
        const std::size_t pull_first = (std::size_t)std::atoll(argv[7]);
        rh::init(0);
        rh::GpuMixer::Options opt;
        opt.block_frames = (std::size_t)std::atoll(argv[6]);
        opt.wide_filters = std::atoi(argv[8]) != 0;
        rh::GpuMixer mixer(channels, rate, opt);
        FILE *spec = std::fopen((dir + "/spec.txt").c_str(), "r");
        if (!spec) throw std::runtime_error("open spec.txt");
        int next_src = 0;
        auto add = [&](int count) {
            for (int k = 0; k < count; ++k, ++next_src) {
                unsigned ch = 0, r = 0, freq = 0;
                int kind = -1;
                float gain = 1.0f, q = 0.5f;
                if (std::fscanf(spec, "%u %u %f %d %u %f", &ch, &r, &gain, &kind, &freq, &q) != 6) throw std::runtime_error("spec.txt");
                auto src = std::make_unique<TestSource>((std::uint16_t)ch, r, read_f32(dir + "/src_" + std::to_string(next_src) + ".f32"));
                mixer.add(std::move(src), gain, rh::GpuMixer::Filter{kind, freq, q});
            }
        };
        std::vector<float> out;
        std::vector<long long> hints;
        auto note = [&]() {
            const rh::SizeHint h = mixer.size_hint();
            hints.push_back((long long)h.lower);
            hints.push_back(h.upper ? (long long)*h.upper : -1);
        };
        add(n_first);
        for (bool joined = n_late == 0;;) {
            if (!joined && out.size() == pull_first) add(n_late), joined = true;
            note();
            const std::optional<float> v = mixer.next();
            if (!v) break;
            out.push_back(*v);
        }
        std::fclose(spec);
        write_vec(dir + "/out.f32", out);
        write_vec(dir + "/hints.i64", hints);
        FILE *st = std::fopen((dir + "/stats.txt").c_str(), "w");
        if (!st) throw std::runtime_error("write stats.txt");
        std::fprintf(st, "{\"wide_fused_blocks\": %llu, \"wide_filtered_blocks\": %llu, \"chains\": %llu, \"total_duration_none\": %d}\n", (unsigned long long)mixer.wide_fused_blocks(),
                     (unsigned long long)mixer.wide_filtered_blocks(), (unsigned long long)mixer.chain_stats().chains, mixer.total_duration() ? 0 : 1);
        std::fclose(st);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
