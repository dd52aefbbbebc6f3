// fake_mix.cpp -- TEST INFRASTRUCTURE ONLY.  The CPU stand-in (see fake_device.cpp) for rh_mix_pair of rh_mix2.hip, the one new entry
// the C++ mirror calls (Mix runs rh_mix_pair over two blocks; Crossfade streams through the stand-alone calls fake_device.cpp already
// stands in for).  Linked with fake_device.cpp, fake_generators.cpp and fake_noise.cpp into tests/cpp/mix_mirror_test_fake and into
// nothing else: it lets Mix and Crossfade of include/rodio_hip.hpp (their trait answers, their end-of-stream rules, the device path
// of a chain or a mixer over them) run in the `-m "not gpu"` suite.
//
// Build: g++ -std=c++17 -O2 -ffp-contract=off -I include -I rodio_amd/csrc tests/cpp/mix_mirror_test.cpp tests/cpp/fake_device.cpp
//        tests/cpp/fake_generators.cpp tests/cpp/fake_noise.cpp tests/cpp/fake_mix.cpp -o tests/cpp/mix_mirror_test_fake
#include <cstddef>

#include "rodio_hip.h"

extern "C" {

// mix.rs:43-53: s1 + s2 while both rows run, then the longer one's rest verbatim.  In place on either input: sample by sample.
rh_status rh_mix_pair(float *dst, const float *a, size_t na, const float *b, size_t nb, rh_stream) {
    const size_t total = na > nb ? na : nb;
    if (total == 0) return RH_OK;
    if (!dst || (na && !a) || (nb && !b)) return RH_ERR_INVALID;
    for (size_t i = 0; i < total; ++i) dst[i] = i < na ? (i < nb ? a[i] + b[i] : a[i]) : b[i];
    return RH_OK;
}
}
