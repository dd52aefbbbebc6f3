// rh_generators.h -- the phase of rodio's SignalGenerator (src/source/signal_generator.rs:134-139), n steps ahead, exactly.
//
//   next():  phase = (phase + phase_step).rem_euclid(1.0)        (f32, no contraction)
//
// The recurrence is not associative: sample i's phase is not i * step, and the kernels cannot simply multiply.  This header
// advances the SERIAL recurrence, bit for bit, faster than one step at a time.  It is __host__ __device__: the library's walk
// kernel (rh_generators.hip), rh_signal_phase_advance (host) and tests/cpp/generators_test.cpp (against brute-force stepping)
// all compile this one copy.
//
// One step.  For a phase p >= 0 and a step s >= 0, x = RN(p + s) >= 0 and rem_euclid(x, 1) = fmod(x, 1) = x - floor(x): the
// fractional part of a float is a float, so both are exact (and +inf / NaN give NaN, as rodio's).  For s < 1 every phase lies
// in [0, 1), x < 2 and the step is `x >= 1 ? x - 1 : x`.
//
// Fast-forward (s < 1 only).  Let p, q = step(p), r = step(q) lie in ONE binade [2^e, 2^(e+1)), ulp u (so all three are on
// its grid).  While a step stays inside the binade, RN(v + s) = v + RN_u(s) for v on the grid: a constant increment, except
// that a tie (s / u = m + 1/2) rounds to the EVEN neighbour of v / u + m.  p is on the grid, so q is even after a tie; from q
// on, every increment is the same (D = r - q: the even one of m, m + 1) and keeps the parity.  So from r, k more steps land on
// r + k * D as long as r + k * D stays below the binade's top; the step that reaches the top (or the wrap through 1) rounds
// on another grid and is taken one at a time again.  D == 0 (s below half an ulp): the phase never moves again.
// s == 0 (a period of inf): the phase is reduced once and stays.  For s >= 1 (a frequency above the sample rate) x leaves [0, 2) and the phase is stepped one sample at a time; so it is for
// s >= 1/32, where no binade holds enough steps to pay for the bookkeeping.
#ifndef RH_GENERATORS_H
#define RH_GENERATORS_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RH_GEN_HD __host__ __device__
#else
#define RH_GEN_HD
#endif

namespace rhgen {

RH_GEN_HD inline uint32_t f2u(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}
RH_GEN_HD inline float u2f(uint32_t u) {
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

// One step of signal_generator.rs:137, for phase >= 0 (or NaN) and step >= 0 (or +inf / NaN).
RH_GEN_HD inline float step(float p, float s) {
    const float x = p + s;
    return x - __builtin_floorf(x);
}

// A walk of the recurrence that keeps its place: advance(n) moves the phase n steps on, bit-identical to n calls of step(p, s).
// Between calls it keeps the binade run it is in (the steady increment and the steps left to the binade's top), so a caller that
// walks in short pieces (k_gen_walk: 64 samples) skips as far as one long call would.
struct Walk {
    float p, s;
    uint32_t run = 0;   // in-binade steps taken one at a time since the last binade change
    uint32_t left = 0;  // steps of the current fast-forward left (p on the binade's grid, increment d)
    uint32_t d = 0;
    RH_GEN_HD Walk(float phase, float phase_step) : p(phase), s(phase_step) {}
    RH_GEN_HD __attribute__((always_inline)) void advance(uint64_t n) {
        if (!n) return;
        // (on locals: the walk is the kernel's critical path, nothing of it may live in memory)
        float p = this->p;
        const float s = this->s;
        uint32_t run = this->run, left = this->left, d = this->d;
        if (s == 0.0f) {  // (freq so small that the period is inf): one step reduces p, and then it never moves
            this->p = step(p, s);
            return;
        }
        if (!(s < 0.03125f)) {  // s >= 1, +inf or NaN; or fewer than 32 steps a cycle, where a binade holds too few steps to skip: one at a time
            for (; n && p == p; --n) p = step(p, s);  // (NaN stays NaN)
            this->p = p;
            return;
        }
        while (n) {
            if (left) {  // inside a fast-forward: k steps are k * d on the grid
                const uint32_t k = left < n ? left : (uint32_t)n;
                const uint32_t b = f2u(p), m = ((b & 0x7fffffu) | 0x800000u) + k * d;
                p = u2f((b & 0xff800000u) | (m & 0x7fffffu));
                left -= k, n -= k;
                continue;
            }
            const float q = step(p, s);
            --n;
            const uint32_t bp = f2u(p), bq = f2u(q);
            // same binade of normal numbers: same exponent field, and not zero / subnormal (exponent 0)
            run = ((bp >> 23) == (bq >> 23) && (bp >> 23) != 0u && q == q) ? run + 1 : 0;
            p = q;
            if (run >= 2) {
                // the step into p and the one before it were in this binade: d = q - p_before is the steady increment (see above)
                const uint32_t mp = (bp & 0x7fffffu) | 0x800000u, mq = (bq & 0x7fffffu) | 0x800000u;
                d = mq - mp;
                if (d == 0u) break;  // stuck for good
                left = (0x1000000u - 1u - mq) / d;  // steps that stay below the top of the binade
                run = 1;  // (when they are used up, the next in-binade step may fast-forward again)
            }
        }
        this->p = p, this->run = run, this->left = left, this->d = d;
    }
};

// The phase after n steps from p.  Bit-identical to n calls of step(p, s).
RH_GEN_HD inline float advance(float p, float s, uint64_t n) {
    Walk w(p, s);
    w.advance(n);
    return w.p;
}

// rodio's Function, as the ABI numbers it (include/rodio_hip.h: RH_GEN_*): signal_generator.rs:24-63.  TAU = 6.2831855f32.
RH_GEN_HD inline float triangle(float phase) { return 4.0f * __builtin_fabsf(phase - __builtin_floorf(phase + 0.5f)) - 1.0f; }
RH_GEN_HD inline float square(float phase) { return __builtin_fmodf(phase, 1.0f) < 0.5f ? 1.0f : -1.0f; }
RH_GEN_HD inline float sawtooth(float phase) { return 2.0f * (phase - __builtin_floorf(phase + 0.5f)); }
RH_GEN_HD inline float sine(float phase) {
#if defined(__HIP_DEVICE_COMPILE__)
    return sinf(6.2831855f * phase);  // the device library's accurate sinf (not __sinf, not the v_sin_f32 an intrinsic would become)
#else
    return __builtin_sinf(6.2831855f * phase);
#endif
}
// A function code outside RH_GEN_* gives NaN samples (the ABI cannot read a device array to refuse it).
RH_GEN_HD inline float value(int32_t fn, float phase) {
    switch (fn) {
        case 0: return sine(phase);
        case 1: return triangle(phase);
        case 2: return square(phase);
        case 3: return sawtooth(phase);
        default: return __builtin_nanf("");
    }
}

// Duration::from_secs_f64(v) for 0 <= v < 2^64 (host only): the exact value of the f64, rounded to the nearest nanosecond, ties to even
// (Rust's float -> Duration conversion).
inline void duration_from_secs_f64(double v, uint64_t *secs, uint32_t *nanos) {
    *secs = 0, *nanos = 0;
    if (!(v > 0.0)) return;
    int e;
    const double fr = __builtin_frexp(v, &e);               // v = fr * 2^e, fr in [0.5, 1)
    const uint64_t m = (uint64_t)__builtin_ldexp(fr, 53);  // v = m / 2^sh, m < 2^53
    const int sh = 53 - e;
    if (sh <= 0) {
        *secs = m << -sh;
        return;
    }
    if (sh > 120) return;  // below 2^-67 s
    const unsigned __int128 whole = (unsigned __int128)m >> sh, rem = (unsigned __int128)m - (whole << sh);
    const unsigned __int128 num = rem * 1000000000u;  // nanoseconds = num / 2^sh
    uint64_t ns = (uint64_t)(num >> sh);
    const unsigned __int128 r = num - ((unsigned __int128)ns << sh), half = ((unsigned __int128)1 << sh) >> 1;
    if (r > half || (r == half && (ns & 1u))) ++ns;
    uint64_t s = (uint64_t)whole;
    if (ns == 1000000000u) ++s, ns = 0;
    *secs = s, *nanos = (uint32_t)ns;
}

}  // namespace rhgen

#endif
