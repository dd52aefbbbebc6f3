// rh_noise.hip -- sources that start on the device: rodio's noise generators (src/source/noise.rs, feature `noise`).
//   WhiteUniform, WhiteTriangular, WhiteGaussian, Pink, Blue, Violet, Brownian, Red, Velvet
// The contract is rh_noise.h's: sample k of a stream is a pure function of (seed, k), except for the two integrators, which run a
// first-order recurrence over that white stream.  Built with -ffp-contract=off (rodio_amd/build.py): no expression below is fused.
//
// rh_noise_generate is three launches on one stream, over a [n_streams, ld] block whose row g receives stream g:
//   k_noise_fill   grid (tiles, streams).  By the stream's kind:
//                    white x3, blue, violet, velvet: elementwise, four samples a lane, one 16-byte store where the row allows it;
//                    pink: a tile of kPinkTile samples ALIGNED on the stream's sample index k.  The draws its 16 generators use
//                          (about 2 kPinkTile of them) are hashed once into LDS; each sample then adds its 16 values in order;
//                    red, brownian: the first pass of a per-row scan of the maps x -> x * leak + w: a workgroup composes its tile's
//                          maps (16 samples a lane) into one (A, B) and leaves it in the stream's scratch;
//   k_noise_carry  a wave per stream: k moves on by n; for an integrator, the tiles' maps are applied in order to the stream's acc
//                  (the carry into every tile is left in the scratch, the last one is the new acc);
//   k_noise_scan   red, brownian: each tile again, from its carry in: the lane's carry is the tile's composed with the maps of the
//                  lanes before it, and the lane runs the literal recurrence (multiply, then add) over its 16 samples; the tile goes
//                  out through LDS, four consecutive samples a lane.
// The integrators are therefore not rodio's serial f32 sums: DESIGN.md states their bound (4e-5 absolute of the f64 recurrence).
// No private segment, no spill, no dynamic stack (tests/test_code_objects.py).
#include <cstdint>
#include <cstring>

#include "rh_common.h"
#include "rh_noise.h"

namespace {

using namespace rhnoise;

constexpr int kBlock = 256;
constexpr uint32_t kElemTile = 4 * kBlock;  // samples a workgroup of the elementwise kinds (four a lane)
constexpr int kPinkLog = 10;
constexpr uint32_t kPinkTile = 1u << kPinkLog;  // == kElemTile: the two kinds share the grid
// LDS image of a pink tile: generator i < kPinkLog holds kPinkTile >> i values (one per 2^i samples) at pink_off(i); the generators
// i >= kPinkLog are constant over the tile: one value each, at pink_off(kPinkLog) + i - kPinkLog.
__host__ __device__ constexpr uint32_t pink_off(int i) { return 2 * kPinkTile - ((2 * kPinkTile) >> i); }
constexpr uint32_t kPinkSlots = pink_off(kPinkLog) + (kPinkGenerators - kPinkLog);
constexpr int kScanPer = 16;                       // samples a lane of the integrator scan
constexpr uint32_t kScanTile = kBlock * kScanPer;  // samples a workgroup of the integrator scan

struct Stream {
    uint64_t seed, k;
    int32_t kind;
    uint32_t p5, p6;
    float acc;
};
__device__ __forceinline__ Stream load_stream(const uint32_t *__restrict__ st) {
    Stream s;
    s.seed = (uint64_t)st[W_SEED_LO] | ((uint64_t)st[W_SEED_HI] << 32);
    s.k = (uint64_t)st[W_K_LO] | ((uint64_t)st[W_K_HI] << 32);
    s.kind = (int32_t)st[W_KIND];
    s.p5 = st[W_PARAM];
    s.p6 = st[W_SCALE];
    s.acc = __uint_as_float(st[W_ACC]);
    return s;
}

// four samples of row `row` at i .. i+3 (< n where valid): one 16-byte store if the row is aligned and all four are in
__device__ __forceinline__ void store4(float *__restrict__ row, int64_t i, uint64_t n, const float (&y)[4]) {
    const bool vec = ((reinterpret_cast<uintptr_t>(row + i) & 15u) == 0) && i >= 0 && (uint64_t)i + 4 <= n;
    if (vec) {
        rh::st_nt(reinterpret_cast<float4 *>(row + i), make_float4(y[0], y[1], y[2], y[3]));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j >= 0 && (uint64_t)(i + j) < n) row[i + j] = y[j];
    }
}

// ---- the stateless kinds, four samples a lane ----------------------------------------------------------------------------------
__device__ __forceinline__ void fill_elementwise(float *__restrict__ row, uint64_t n, const Stream &s) {
    const uint64_t i = (uint64_t)blockIdx.x * kElemTile + 4u * threadIdx.x;
    if (i >= n) return;
    const uint64_t k = s.k + i;
    float y[4];
    if (s.kind == WHITE_UNIFORM || s.kind == WHITE_TRIANGULAR || s.kind == WHITE_GAUSSIAN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t h = hash(s.seed, k + j);
            y[j] = s.kind == WHITE_UNIFORM ? u1(h) : s.kind == WHITE_TRIANGULAR ? triangular(h) : gaussian(h);
        }
    } else if (s.kind == BLUE || s.kind == VIOLET) {
        // w[q] = W(k - 2 + q), 0 for a negative index; b[q] = B(k - 1 + q) = w[q + 1] - w[q]
        float w[6], b[5];
#pragma unroll
        for (int q = 0; q < 6; ++q) w[q] = (k + q >= 2) ? white(s.seed, k + q - 2) : 0.0f;
#pragma unroll
        for (int q = 0; q < 5; ++q) b[q] = w[q + 1] - w[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = s.kind == BLUE ? b[j + 1] : b[j + 1] - b[j];
    } else if (s.kind == VELVET) {
        const uint64_t grid = (uint64_t)s.p5 | ((uint64_t)s.p6 << 32);
        uint64_t c = k / grid, at = k - c * grid;  // the cell and the place in it
        uint64_t hc = hash(s.seed, c), pos = velvet_pos(hc, grid);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            y[j] = at == pos ? velvet_sign(hc) : 0.0f;
            if (++at == grid) at = 0, hc = hash(s.seed, ++c), pos = velvet_pos(hc, grid);
        }
    } else {  // not a kind: NaN
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = __uint_as_float(0x7fc00000u);
    }
    store4(row, (int64_t)i, n, y);
}

// ---- pink: a tile aligned on k ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fill_pink(float *__restrict__ row, uint64_t n, const Stream &s, float *__restrict__ lds) {
    const uint64_t first = ((s.k >> kPinkLog) + blockIdx.x) << kPinkLog;  // the tile's first sample index
    if (first >= s.k + n) return;
    for (uint32_t q = threadIdx.x; q < kPinkSlots; q += kBlock) {
        int i;
        uint64_t m;
        if (q < pink_off(kPinkLog)) {
            i = 0;
            while (q >= pink_off(i + 1)) ++i;
            m = first + ((uint64_t)(q - pink_off(i)) << i);
        } else {
            i = kPinkLog + (int)(q - pink_off(kPinkLog));
            m = first & ~((1ull << i) - 1);
        }
        lds[q] = m == 0 ? 0.0f : white(s.seed, pink_draws_before(m) + (uint64_t)i);
    }
    __syncthreads();
    const uint32_t t0 = 4u * threadIdx.x;  // this lane's samples in the tile
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < kPinkGenerators; ++i) sum += i < kPinkLog ? lds[pink_off(i) + ((t0 + j) >> i)] : lds[pink_off(kPinkLog) + (i - kPinkLog)];
        y[j] = sum / 16.0f;
    }
    store4(row, (int64_t)(first + t0 - s.k), n, y);
}

// ---- red / brownian: the maps x -> x * leak + w of a tile ------------------------------------------------------------------------
// The map of a run of L samples is x -> x * leak^L + b.  A map carries L, not leak^L: composing powers (leak^16 a lane, then the products
// of the scan) would carry the relative error of leak^16 into leak^4096 times 256, systematically, and the integrator's accumulator is
// large (sigma ~ 1 / scale: 32 at 192 kHz).  leak^L is instead the f32 of the f64 exp2(L log2 leak), correctly rounded or one ulp off,
// wherever it is needed: the scan then stays within ~2.5e-6 of the f64 recurrence over 2^24 samples at 8-192 kHz, where rodio's own
// serial f32 loop is 4e-6 to 2e-5 away (a numpy restatement of this scan; tests/test_gpu_noise.py measures the device).
struct Aff {
    uint32_t len;
    float b;
};
// Powers: leak^(16 m), m = 0 .. 256 (every run of whole lanes in a tile), in an LDS table filled once per workgroup; any other length (the
// lanes that end a row inside their 16 samples) is computed where it is needed.
constexpr uint32_t kPowSlots = kBlock + 1;
struct Pow {
    double lg;  // log2(leak)
    const float *tab;
    __device__ __forceinline__ float operator()(uint32_t len) const {
        return ((len & (kScanPer - 1)) == 0 && len <= kScanTile) ? tab[len / kScanPer] : (float)exp2((double)len * lg);
    }
};
__device__ __forceinline__ Pow make_pow(float leak, float *__restrict__ tab) {
    const double lg = log2((double)leak);
    for (uint32_t m = threadIdx.x; m < kPowSlots; m += kBlock) tab[m] = (float)exp2((double)(m * kScanPer) * lg);
    __syncthreads();
    return Pow{lg, tab};
}
__device__ __forceinline__ Aff then(Aff p, Aff q, const Pow &pw) { return Aff{p.len + q.len, p.b * pw(q.len) + q.b}; }  // p first, then q
// the block's maps in lane order: inclusive result; `excl` = the lanes before this one; `tot` = the whole block (lds: 8 words)
__device__ __forceinline__ Aff block_scan(Aff v, Aff &excl, Aff &tot, const Pow &lg, float *__restrict__ lds) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t pl = (uint32_t)__shfl_up((int)v.len, d, 64);
        const float pb = __shfl_up(v.b, d, 64);
        if (lane >= d) v = then(Aff{pl, pb}, v, lg);
    }
    if (lane == 63) lds[2 * wv] = __uint_as_float(v.len), lds[2 * wv + 1] = v.b;
    const uint32_t el = (uint32_t)__shfl_up((int)v.len, 1, 64);
    const float eb = __shfl_up(v.b, 1, 64);
    __syncthreads();
    Aff pre{0u, 0.0f};
    tot = Aff{0u, 0.0f};
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        const Aff x{__float_as_uint(lds[2 * w]), lds[2 * w + 1]};
        if (w < wv) pre = w ? then(pre, x, lg) : x;
        tot = w ? then(tot, x, lg) : x;
    }
    const Aff mine = lane ? Aff{el, eb} : Aff{0u, 0.0f};
    excl = wv ? (lane ? then(pre, mine, lg) : pre) : mine;
    return wv ? then(pre, v, lg) : v;
}
// this lane's white samples and its map; cnt = how many of its kScanPer samples are in the block
__device__ __forceinline__ Aff lane_map(const Stream &s, uint64_t i, uint64_t n, float leak, float (&w)[kScanPer], int &cnt) {
    cnt = i >= n ? 0 : (n - i < (uint64_t)kScanPer ? (int)(n - i) : kScanPer);
    Aff m{(uint32_t)cnt, 0.0f};
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        w[j] = j < cnt ? integrator_white(s.kind, s.seed, s.k + i + j) : 0.0f;
        if (j < cnt) m.b = m.b * leak + w[j];
    }
    return m;
}

__device__ __forceinline__ void scan_first_pass(uint64_t n, const Stream &s, float *__restrict__ tiles, float *__restrict__ lds) {
    const uint64_t t = blockIdx.x;
    if (t * kScanTile >= n) return;
    const float leak = __uint_as_float(s.p5);
    const Pow pw = make_pow(leak, lds + 8);
    float w[kScanPer];
    int cnt;
    const Aff m = lane_map(s, t * kScanTile + (uint64_t)threadIdx.x * kScanPer, n, leak, w, cnt);
    Aff excl, tot;
    (void)block_scan(m, excl, tot, pw, lds);
    if (threadIdx.x == 0) tiles[2 * t] = pw(tot.len), tiles[2 * t + 1] = tot.b;
}

// scratch: per stream, 2 * tiles_per_row floats (the tiles' maps, then their carries in), and the stream's k before the call (2 words)
__global__ __launch_bounds__(kBlock) void k_noise_fill(float *__restrict__ dst, uint64_t ld, uint64_t n, const uint32_t *__restrict__ states, float *__restrict__ scratch,
                                                       uint64_t tiles_per_row) {
    __shared__ float lds[kPinkSlots];
    const uint32_t g = blockIdx.y;
    const Stream s = load_stream(states + (size_t)g * STATE_WORDS);
    float *row = dst + (size_t)g * ld;
    if (s.kind == PINK) {
        fill_pink(row, n, s, lds);
    } else if (s.kind == RED || s.kind == BROWNIAN) {
        scan_first_pass(n, s, scratch + (size_t)g * 2 * tiles_per_row, lds);
    } else {
        fill_elementwise(row, n, s);
    }
}

// a wave per stream: the tiles' maps 64 at a time into the wave's lanes, then applied in order (every lane runs the same serial chain, with
// the map of step j read from lane j): one load latency per 64 tiles instead of one per tile.
__global__ __launch_bounds__(64) void k_noise_carry(uint64_t n, uint32_t *__restrict__ states, uint32_t n_streams, float *__restrict__ scratch, uint64_t tiles_per_row) {
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    uint32_t *st = states + (size_t)g * STATE_WORDS;
    const Stream s = load_stream(st);
    if (lane == 0) {
        uint32_t *k_before = reinterpret_cast<uint32_t *>(scratch + (size_t)n_streams * 2 * tiles_per_row) + 2 * (size_t)g;
        k_before[0] = (uint32_t)s.k, k_before[1] = (uint32_t)(s.k >> 32);
        const uint64_t k = s.k + n;
        st[W_K_LO] = (uint32_t)k, st[W_K_HI] = (uint32_t)(k >> 32);
    }
    if (s.kind != RED && s.kind != BROWNIAN) return;
    float *tiles = scratch + (size_t)g * 2 * tiles_per_row;
    const uint64_t used = (n + kScanTile - 1) / kScanTile;
    float acc = s.acc;
    for (uint64_t t0 = 0; t0 < used; t0 += 64) {
        const uint64_t t = t0 + lane;
        const float a = t < used ? tiles[2 * t] : 1.0f, b = t < used ? tiles[2 * t + 1] : 0.0f;
        const int steps = used - t0 < 64 ? (int)(used - t0) : 64;
        float in = 0.0f;
        for (int j = 0; j < steps; ++j) {
            if ((int)lane == j) in = acc;  // the carry into tile t0 + j
            acc = acc * __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), j)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), j));
        }
        if (t < used) tiles[2 * t] = in;
    }
    if (lane == 0) st[W_ACC] = __float_as_uint(acc);
}

__global__ __launch_bounds__(kBlock) void k_noise_scan(float *__restrict__ dst, uint64_t ld, uint64_t n, const uint32_t *__restrict__ states, uint32_t n_streams,
                                                       const float *__restrict__ scratch, uint64_t tiles_per_row) {
    constexpr uint32_t kPitch = kScanPer + 4;                  // a lane's 16 outputs in LDS, rows 16-byte aligned
    constexpr uint32_t kOut = (8 + kPowSlots + 3) & ~3u;       // where they start
    __shared__ __attribute__((aligned(16))) float lds[kOut + kBlock * kPitch];
    const uint32_t g = blockIdx.y;
    Stream s = load_stream(states + (size_t)g * STATE_WORDS);  // (k has moved on: the k of the call is in the scratch)
    if (s.kind != RED && s.kind != BROWNIAN) return;
    const uint64_t t = blockIdx.x;
    if (t * kScanTile >= n) return;
    const uint32_t *k_before = reinterpret_cast<const uint32_t *>(scratch + (size_t)n_streams * 2 * tiles_per_row) + 2 * (size_t)g;
    s.k = (uint64_t)k_before[0] | ((uint64_t)k_before[1] << 32);
    const float leak = __uint_as_float(s.p5), scale = __uint_as_float(s.p6);
    const Pow pw = make_pow(leak, lds + 8);
    const float carry = scratch[(size_t)g * 2 * tiles_per_row + 2 * t];
    const uint64_t i0 = t * kScanTile;
    float w[kScanPer];
    int cnt;
    const Aff m = lane_map(s, i0 + (uint64_t)threadIdx.x * kScanPer, n, leak, w, cnt);
    Aff excl, tot;
    (void)block_scan(m, excl, tot, pw, lds);
    float acc = excl.len ? carry * pw(excl.len) + excl.b : carry;
    float *mine = lds + kOut + threadIdx.x * kPitch;
#pragma unroll
    for (int q = 0; q < kScanPer / 4; ++q) {
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc = acc * leak + w[4 * q + j];
            y[j] = acc * scale;
        }
        *reinterpret_cast<float4 *>(mine + 4 * q) = make_float4(y[0], y[1], y[2], y[3]);
    }
    __syncthreads();
    // the tile back out in the order of the row: four consecutive samples a lane, a wave's 1 KiB contiguous
    float *row = dst + (size_t)g * ld;
#pragma unroll
    for (uint32_t r = 0; r < kScanTile / (4 * kBlock); ++r) {
        const uint32_t q = 4 * threadIdx.x + r * 4 * kBlock;  // sample of the tile
        const float4 v = *reinterpret_cast<const float4 *>(lds + kOut + (q / kScanPer) * kPitch + q % kScanPer);
        const float y[4] = {v.x, v.y, v.z, v.w};
        store4(row, (int64_t)(i0 + q), n, y);
    }
}

}  // namespace

rh_status rh_noise_init(uint32_t state[8], int32_t kind, uint32_t sample_rate, uint64_t seed, uint32_t density) {
    if (!state || kind < WHITE_UNIFORM || kind > VELVET || sample_rate == 0 || (kind == VELVET && density == 0)) return RH_ERR_INVALID;
    for (int q = 0; q < STATE_WORDS; ++q) state[q] = 0;
    state[W_SEED_LO] = (uint32_t)seed, state[W_SEED_HI] = (uint32_t)(seed >> 32);
    state[W_KIND] = (uint32_t)kind;
    if (kind == VELVET) {
        const uint64_t grid = velvet_grid(sample_rate, density);
        state[W_PARAM] = (uint32_t)grid, state[W_SCALE] = (uint32_t)(grid >> 32);
    } else if (kind == RED || kind == BROWNIAN) {
        const float leak = integrator_leak(sample_rate), scale = integrator_scale(leak, kind == RED ? uniform_std_dev() : 0.6f);
        std::memcpy(&state[W_PARAM], &leak, 4);
        std::memcpy(&state[W_SCALE], &scale, 4);
    }
    return RH_OK;
}

rh_status rh_noise_generate(float *dst, uint64_t ld, uint64_t n, uint32_t *states_dev, uint32_t n_streams, rh_stream stream) {
    RH_REQUIRE_INIT();
    if (n == 0 || n_streams == 0) return RH_OK;
    if (!dst || !states_dev || ld < n || n_streams > 65535u) return RH_ERR_INVALID;
    // one more tile than n needs: a pink tile is aligned on k, so the block's samples may touch one tile more
    const uint64_t gx = (n + kElemTile - 1) / kElemTile + 1, tiles = (n + kScanTile - 1) / kScanTile;
    if (gx > 0x7fffffffull) return RH_ERR_INVALID;
    hipStream_t hs = rh::as_stream(stream);
    float *scratch = nullptr;
    std::unique_lock<std::mutex> hold;
    RH_HIP_TRY(rh::stream_scratch(hs, sizeof(float) * (size_t)n_streams * (2 * tiles + 2), reinterpret_cast<void **>(&scratch), hold));
    hipLaunchKernelGGL(k_noise_fill, dim3((unsigned)gx, n_streams), dim3(kBlock), 0, hs, dst, ld, n, states_dev, scratch, tiles);
    RH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_noise_carry, dim3(n_streams), dim3(64), 0, hs, n, states_dev, n_streams, scratch, tiles);
    RH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_noise_scan, dim3((unsigned)tiles, n_streams), dim3(kBlock), 0, hs, dst, ld, n, states_dev, n_streams, scratch, tiles);
    RH_CHECK_LAUNCH();
    return RH_OK;
}
