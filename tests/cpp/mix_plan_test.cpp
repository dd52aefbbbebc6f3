// What rodio_amd/csrc/rh_mix_plan.h -- the host rules the block mixers share -- answers, printed for tests/test_mix_plan_cpu.py to hold
// against Python integers.  No GPU, no HIP.
//   stepdiv PERIOD AT N K..     step_div(AT, PERIOD, N).step(K) for every K
//   stepwords PERIOD AT N       step_div(AT, PERIOD, N) itself: "phase m s1 s2"
//   stepsweep PERIOD AT N       the K < N whose step differs from the quotient (AT % PERIOD + K) / PERIOD, counted up sample by sample: their number
//   check TO_RATE OUT_FRAMES DATA CHANNELS FROM_RATE PHASE FRAMES LAST
//                               check_src of that source: "status F T fit", or "skip" for a source of no frames (walk's rule: not looked at)
//   slots TO_RATE FROM:PHASE:FRAMES..
//                               walk_rates over that table, a line per launch: "cont nr n F:T:r0.. | src:slot.."
//   cut CHANNELS TO_RATE OUT_FRAMES CH:FROM:PHASE:FRAMES:LAST..
//                               alike_cut of that table
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rh_mix_plan.h"

namespace mp = rh::mixplan;

static uint64_t num(const char *s) { return strtoull(s, nullptr, 0); }

// "a:b:c.." -> the numbers
static std::vector<uint64_t> fields(const char *s) {
    std::vector<uint64_t> v;
    for (const char *p = s; *p;) {
        char *end;
        v.push_back(strtoull(p, &end, 0));
        p = *end ? end + 1 : end;
    }
    return v;
}

static float g_sample[4];  // something for `data` to point at: nothing reads it

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const char *cmd = argv[1];
    if (!strcmp(cmd, "stepdiv") && argc >= 5) {
        const mp::StepDiv d = mp::step_div(num(argv[3]), num(argv[2]), num(argv[4]));
        for (int k = 5; k < argc; ++k) printf("%u\n", d.step((uint32_t)num(argv[k])));
        return 0;
    }
    if (!strcmp(cmd, "stepwords") && argc == 5) {
        const mp::StepDiv d = mp::step_div(num(argv[3]), num(argv[2]), num(argv[4]));
        printf("%u %u %u %u\n", d.phase, d.m, d.s1, d.s2);
        return 0;
    }
    if (!strcmp(cmd, "stepsweep") && argc == 5) {
        const uint64_t period = num(argv[2]), at = num(argv[3]), n = num(argv[4]);
        const mp::StepDiv d = mp::step_div(at, period, n);
        uint64_t bad = 0, q = 0, r = at % period;  // (the quotient by counting: no division a sample)
        for (uint64_t k = 0; k < n; ++k) {
            bad += d.step((uint32_t)k) != q;
            if (++r == period) r = 0, ++q;
        }
        printf("%" PRIu64 "\n", bad);
        return 0;
    }
    if (!strcmp(cmd, "check") && argc == 10) {
        rh_wide_src x{};
        x.data = num(argv[4]) ? g_sample : nullptr;
        x.channels = (uint32_t)num(argv[5]), x.from_rate = (uint32_t)num(argv[6]), x.phase = (uint32_t)num(argv[7]), x.frames = num(argv[8]), x.last = (uint32_t)num(argv[9]);
        if (x.frames == 0) {
            printf("skip\n");
            return 0;
        }
        uint32_t F = 0, T = 0;
        uint64_t fit = 0;
        const rh_status st = mp::check_src(x, (uint32_t)num(argv[2]), num(argv[3]), &F, &T, &fit);
        printf("%d %u %u %" PRIu64 "\n", (int)st, F, T, fit);
        return 0;
    }
    if (!strcmp(cmd, "slots") && argc >= 3) {
        const uint32_t to_rate = (uint32_t)num(argv[2]);
        std::vector<rh_wide_src> srcs;
        for (int k = 3; k < argc; ++k) {
            const std::vector<uint64_t> f = fields(argv[k]);
            if (f.size() != 3) return 2;
            rh_wide_src x{};
            x.data = g_sample, x.channels = 2, x.from_rate = (uint32_t)f[0], x.phase = (uint32_t)f[1], x.frames = f[2], x.last = 0xffffffffu, x.gain = 1.0f;
            srcs.push_back(x);
        }
        mp::walk_rates<mp::RateLaunch>(
            (uint32_t)srcs.size(), true,
            [&](uint32_t s, uint32_t *F, uint32_t *T, uint32_t *r0, uint64_t *) {
                if (srcs[s].frames == 0) return false;
                mp::reduce(srcs[s].from_rate, to_rate, F, T);
                *r0 = srcs[s].phase;
                return true;
            },
            [&](const mp::RateLaunch &L) {
                printf("%d %u %u", L.cont ? 1 : 0, L.nr, L.n);
                for (uint32_t q = 0; q < mp::kRates; ++q) printf(" %u:%u:%u", L.r[q].F, L.r[q].T, L.r[q].r0);
                printf(" |");
                for (uint32_t q = 0; q < L.n; ++q) printf(" %u:%u", L.src[q], L.rate[q]);
                printf("\n");
            });
        return 0;
    }
    if (!strcmp(cmd, "cut") && argc >= 5) {
        std::vector<rh_wide_src> srcs;
        for (int k = 5; k < argc; ++k) {
            const std::vector<uint64_t> f = fields(argv[k]);
            if (f.size() != 5) return 2;
            rh_wide_src x{};
            x.data = g_sample, x.channels = (uint32_t)f[0], x.from_rate = (uint32_t)f[1], x.phase = (uint32_t)f[2], x.frames = f[3], x.last = (uint32_t)f[4], x.gain = 1.0f;
            srcs.push_back(x);
        }
        printf("%" PRIu64 "\n", mp::alike_cut(srcs.data(), (uint32_t)srcs.size(), (uint32_t)num(argv[2]), (uint32_t)num(argv[3]), num(argv[4])));
        return 0;
    }
    return 2;
}
