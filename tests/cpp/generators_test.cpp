// generators_test -- the host build of the phase walk (rodio_amd/csrc/rh_generators.h) against brute-force f32 stepping.
//
//   generators_test walk     stdin: "<step bits hex> <phase bits hex> <n>" per line
//                            stdout: "<advance bits hex> <brute-force bits hex>" per line
//   generators_test phases   stdin: one line "<step bits hex> <phase bits hex> <n>"; stdout: the n phases rodio's next() sees,
//                            raw little-endian f32 (the serial restatement the GPU tests compare the kernels with)
//
// Brute force is rodio's own line (signal_generator.rs:137), `(phase + phase_step).rem_euclid(1.0)`, with rem_euclid as Rust's
// f32 defines it (r = x % 1; r < 0 ? r + 1 : r): not the header's x - floor(x).  Built with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rh_generators.h"

static float rem_euclid1(float x) {
    const float r = std::fmod(x, 1.0f);
    return r < 0.0f ? r + 1.0f : r;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    unsigned sb, pb;
    unsigned long long n;
    if (!std::strcmp(argv[1], "walk")) {
        while (std::scanf("%x %x %llu", &sb, &pb, &n) == 3) {
            const float s = rhgen::u2f(sb), p0 = rhgen::u2f(pb);
            float p = p0;
            for (unsigned long long i = 0; i < n; ++i) p = rem_euclid1(p + s);
            std::printf("%08x %08x\n", rhgen::f2u(rhgen::advance(p0, s, n)), rhgen::f2u(p));
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "phases")) {
        if (std::scanf("%x %x %llu", &sb, &pb, &n) != 3) return 2;
        const float s = rhgen::u2f(sb);
        float p = rhgen::u2f(pb);
        std::vector<float> out(1 << 16);
        for (unsigned long long i = 0; i < n;) {
            std::size_t m = 0;
            for (; m < out.size() && i < n; ++m, ++i) {
                out[m] = p;
                p = rem_euclid1(p + s);
            }
            std::fwrite(out.data(), 4, m, stdout);
        }
        return 0;
    }
    return 2;
}
