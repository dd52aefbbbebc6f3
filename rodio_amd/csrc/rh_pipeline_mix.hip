// rh_pipeline_mix.hip -- the small kernels around the fused launches: k_mix_rows / k_mix_ring sum a batch at the input rate ("mix first"),
// k_rlm_state / k_rlm_state_sum carry a stream's per-source filter states across a block boundary.  With the host functions that launch them.
#include "rh_pipeline_dev.h"

namespace {

// =================================================================================================
// k_mix_rows -- "mix first".  The converter and the filter are linear and, for a batch of equal-length sources of one format,
// the same for every source (same taps, same weights, same span seams, same end):
//     sum_s filter(resample(g_s * x_s)) = filter(resample(sum_s g_s * x_s)).
// So a filtered equal-length batch (the benchmark) is mixed at the INPUT rate first -- this kernel: y[n] = sum_s g_s * x_s[n],
// sources in insertion order, one pass over every input byte as whole aligned 16-byte vectors, nothing else to do per byte --
// and the fused kernel then converts and filters ONE stream (y: 1/S of the input).  The streaming pass is what the roofline
// prices: S * N * C * 4 bytes in, N * C * 4 out.  (Without a filter the batch stays on the per-source path: that one is
// bit-exact with rodio's ordered sum of converted samples; the filtered path is compared at 1e-5 either way.)
// =================================================================================================
// Short rows (a stream's block: 64 Ki frames are 128 workgroups at one vector per lane, half the chip) are cut the other way as well: gridDim.y
// GROUPS of sources, group g summing its share of the source list into partial row g (y + g * group_stride, descriptor ydesc[g]); the fused launch
// behind takes the partial rows as its sources and adds them in order.  One group: the whole list into one row, as before.
template <int U>
__global__ __launch_bounds__(256) void k_mix_rows(const SrcDesc *__restrict__ srcs_all, const uint32_t n_sources_all, float *__restrict__ y_all, const uint64_t n_floats, SrcDesc *__restrict__ ydesc_all,
                                                  const uint32_t frames, const uint32_t out_frames, const float *desc_row_all, const uint64_t group_stride, const uint64_t src_off) {
    // (src_off: bytes added to every source pointer of the table -- a stream whose sources all moved on by the same amount since the table was
    // uploaded passes the distance instead of uploading it again: rh_pipeline_stream.hip)
    typedef __attribute__((address_space(4))) const uint64_t cu64;
    typedef __attribute__((address_space(4))) const float cf32;
    typedef RH_GLB const v4f glb_cf4;
    const uint32_t per_group = (n_sources_all + gridDim.y - 1) / gridDim.y, s_first = blockIdx.y * per_group;
    const uint32_t n_sources = s_first < n_sources_all ? (n_sources_all - s_first < per_group ? n_sources_all - s_first : per_group) : 0u;
    const SrcDesc *const srcs = srcs_all + s_first;
    float *const y = y_all + (uint64_t)blockIdx.y * group_stride;
    SrcDesc *const ydesc = ydesc_all + blockIdx.y;
    const float *const desc_row = desc_row_all + (uint64_t)blockIdx.y * group_stride;
    cu64 *const desc = (cu64 *)(uintptr_t)srcs;
    cf32 *const dgain = (cf32 *)(uintptr_t)srcs;
    const uint64_t nvec = n_floats / 4;
    const uint64_t base = (uint64_t)blockIdx.x * (256u * U) + threadIdx.x;
    v4f acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = v4f{0.f, 0.f, 0.f, 0.f};
    constexpr int SB = 8 / U > 2 ? 8 / U : 2;  // sources per step: 8 (or 2*U) vector loads per lane
    if (base + (uint64_t)(U - 1) * 256u < nvec) {  // every vector of this lane is whole and inside
        // Two register sets: while the vectors of one step are summed, the loads of the next are in flight and the pointers
        // and gains of the step after that are on their way through the scalar cache (the body is written out twice so that
        // the sets swap without moves).
        const uint32_t steps = n_sources / SB;
        uint64_t pN[SB];
        float gN[SB];
        auto fetch_desc = [&](uint32_t j) {
#pragma unroll
            for (int k = 0; k < SB; ++k) {
                pN[k] = desc[4 * (uint64_t)(j * SB + k)] + src_off;
                gN[k] = dgain[8 * (uint64_t)(j * SB + k) + 4];
            }
        };
        auto issue = [&](v4f (&v)[SB][U], float (&g)[SB]) {
#pragma unroll
            for (int k = 0; k < SB; ++k) {
                glb_cf4 *const ptr = (glb_cf4 *)(uintptr_t)pN[k];
                g[k] = gN[k];
#pragma unroll
                for (int u = 0; u < U; ++u) v[k][u] = __builtin_nontemporal_load(ptr + base + (uint64_t)u * 256u);
            }
        };
        auto consume = [&](const v4f (&v)[SB][U], const float (&g)[SB]) {
#pragma unroll
            for (int k = 0; k < SB; ++k)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    acc[u].x = fma_(g[k], v[k][u].x, acc[u].x);
                    acc[u].y = fma_(g[k], v[k][u].y, acc[u].y);
                    acc[u].z = fma_(g[k], v[k][u].z, acc[u].z);
                    acc[u].w = fma_(g[k], v[k][u].w, acc[u].w);
                }
        };
        v4f vA[SB][U], vB[SB][U];
        float gA[SB], gB[SB];
        // (the loads of the next step are issued unconditionally inside the loop: a conditional issue makes the compiler wait
        // for the newest load of either path, which drains the pipeline every step)
        if (steps) {
            fetch_desc(0);
            issue(vA, gA);
            if (steps > 1) fetch_desc(1);
            uint32_t j = 0;
            for (; j + 2 < steps; j += 2) {
                issue(vB, gB);         // step j+1
                fetch_desc(j + 2);
                consume(vA, gA);       // step j
                issue(vA, gA);         // step j+2
                fetch_desc(j + 3 < steps ? j + 3 : steps - 1);
                consume(vB, gB);       // step j+1
            }
            if (j + 1 < steps) {  // two steps left: A in flight, B's descriptors fetched
                issue(vB, gB);
                consume(vA, gA);
                consume(vB, gB);
            } else {
                consume(vA, gA);
            }
        }
        for (uint32_t s = steps * SB; s < n_sources; ++s) {
            glb_cf4 *const ptr = (glb_cf4 *)(uintptr_t)(desc[4 * (uint64_t)s] + src_off);
            const float g = dgain[8 * (uint64_t)s + 4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const v4f v = __builtin_nontemporal_load(ptr + base + (uint64_t)u * 256u);
                acc[u].x = fma_(g, v.x, acc[u].x);
                acc[u].y = fma_(g, v.y, acc[u].y);
                acc[u].z = fma_(g, v.z, acc[u].z);
                acc[u].w = fma_(g, v.w, acc[u].w);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) *reinterpret_cast<v4f *>(y + 4 * (base + (uint64_t)u * 256u)) = acc[u];
    } else {  // the last workgroup: vector by vector, guarded
        for (int u = 0; u < U; ++u) {
            const uint64_t i = base + (uint64_t)u * 256u;
            if (i >= nvec) break;
            v4f a = v4f{0.f, 0.f, 0.f, 0.f};
            for (uint32_t s = 0; s < n_sources; ++s) {
                glb_cf4 *const ptr = (glb_cf4 *)(uintptr_t)(desc[4 * (uint64_t)s] + src_off);
                const float g = dgain[8 * (uint64_t)s + 4];
                const v4f v = ptr[i];
                a.x = fma_(g, v.x, a.x), a.y = fma_(g, v.y, a.y), a.z = fma_(g, v.z, a.z), a.w = fma_(g, v.w, a.w);
            }
            *reinterpret_cast<v4f *>(y + 4 * i) = a;
        }
    }
    if (blockIdx.x == 0) {
        const uint64_t t = nvec * 4 + threadIdx.x;  // the floats behind the last whole vector (a mono batch of a length not divisible by 4)
        if (t < n_floats) {
            float a = 0.f;
            for (uint32_t s = 0; s < n_sources; ++s) a = fma_(dgain[8 * (uint64_t)s + 4], ((glb_cf32 *)(uintptr_t)(desc[4 * (uint64_t)s] + src_off))[t], a);
            y[t] = a;
        }
        if (threadIdx.x == 0) {  // the one-entry descriptor table the fused launch behind this one reads
            ydesc->data = desc_row;  // the row the launch behind this one reads: the mix, or what a filter makes of it
            ydesc->frames = frames;
            ydesc->out_frames = out_frames;
            ydesc->gain = 1.0f;
            ydesc->pad[0] = ydesc->pad[1] = ydesc->pad[2] = 0;
        }
    }
}

// k_mix_rows over rows of 16-bit PCM (rh_rlm_set_sources_pcm16; SrcDesc::data holds the int16 row, n_floats counts samples): the same cut, groups,
// partial rows and guarded last workgroup, written out a second time so that k_mix_rows compiles to what it always did.  A lane's vector is the
// 8 bytes of the four samples the f32 kernel's lane reads as 16: rows on 8-byte boundaries, of any length (the samples behind the last four go
// one by one, as the floats do there); no load reaches past sample n_floats - 1.  float(s) / 32768 is exact (dasp's i16 -> f32), so the sum has
// the bits of converting first.
struct MixPcm16 {
    typedef RH_GLB const v4i16 GV;  // the four samples of an accumulator
    typedef v4i16 V;
    typedef RH_GLB const short GS;
    static __device__ __forceinline__ v4f f(V v) { return v4f{pcm16_f32(v.x), pcm16_f32(v.y), pcm16_f32(v.z), pcm16_f32(v.w)}; }
    static __device__ __forceinline__ float f1(short s) { return pcm16_f32(s); }
};
template <int U>
__global__ __launch_bounds__(256) void k_mix_rows_pcm16(const SrcDesc *__restrict__ srcs_all, const uint32_t n_sources_all, float *__restrict__ y_all, const uint64_t n_floats, SrcDesc *__restrict__ ydesc_all,
                                                        const uint32_t frames, const uint32_t out_frames, const float *desc_row_all, const uint64_t group_stride) {
    typedef MixPcm16 IN;
    typedef IN::V VIN;
    typedef __attribute__((address_space(4))) const uint64_t cu64;
    typedef __attribute__((address_space(4))) const float cf32;
    typedef IN::GV glb_cf4;  // (the four samples of an accumulator)
    const uint32_t per_group = (n_sources_all + gridDim.y - 1) / gridDim.y, s_first = blockIdx.y * per_group;
    const uint32_t n_sources = s_first < n_sources_all ? (n_sources_all - s_first < per_group ? n_sources_all - s_first : per_group) : 0u;
    const SrcDesc *const srcs = srcs_all + s_first;
    float *const y = y_all + (uint64_t)blockIdx.y * group_stride;
    SrcDesc *const ydesc = ydesc_all + blockIdx.y;
    const float *const desc_row = desc_row_all + (uint64_t)blockIdx.y * group_stride;
    cu64 *const desc = (cu64 *)(uintptr_t)srcs;
    cf32 *const dgain = (cf32 *)(uintptr_t)srcs;
    const uint64_t nvec = n_floats / 4;
    const uint64_t base = (uint64_t)blockIdx.x * (256u * U) + threadIdx.x;
    v4f acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = v4f{0.f, 0.f, 0.f, 0.f};
    // sources per step: 8 / U as there, and twice that where the scalar registers hold the pointers and gains of two such steps (U >= 2): half the
    // bytes a load, the same bytes in flight in the same vector registers
    constexpr int SB = U == 1 ? 8 : 2 * (8 / U > 2 ? 8 / U : 2);
    if (base + (uint64_t)(U - 1) * 256u < nvec) {  // every vector of this lane is whole and inside
        // Two register sets: while the vectors of one step are summed, the loads of the next are in flight and the pointers
        // and gains of the step after that are on their way through the scalar cache (the body is written out twice so that
        // the sets swap without moves).
        const uint32_t steps = n_sources / SB;
        uint64_t pN[SB];
        float gN[SB];
        auto fetch_desc = [&](uint32_t j) {
#pragma unroll
            for (int k = 0; k < SB; ++k) {
                pN[k] = desc[4 * (uint64_t)(j * SB + k)];
                gN[k] = dgain[8 * (uint64_t)(j * SB + k) + 4];
            }
        };
        auto issue = [&](VIN (&v)[SB][U], float (&g)[SB]) {
#pragma unroll
            for (int k = 0; k < SB; ++k) {
                glb_cf4 *const ptr = (glb_cf4 *)(uintptr_t)pN[k];
                g[k] = gN[k];
#pragma unroll
                for (int u = 0; u < U; ++u) v[k][u] = __builtin_nontemporal_load(ptr + base + (uint64_t)u * 256u);
            }
        };
        auto consume = [&](const VIN (&v)[SB][U], const float (&g)[SB]) {
#pragma unroll
            for (int k = 0; k < SB; ++k)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const v4f x = IN::f(v[k][u]);
                    acc[u].x = fma_(g[k], x.x, acc[u].x);
                    acc[u].y = fma_(g[k], x.y, acc[u].y);
                    acc[u].z = fma_(g[k], x.z, acc[u].z);
                    acc[u].w = fma_(g[k], x.w, acc[u].w);
                }
        };
        VIN vA[SB][U], vB[SB][U];
        float gA[SB], gB[SB];
        // (the loads of the next step are issued unconditionally inside the loop: a conditional issue makes the compiler wait
        // for the newest load of either path, which drains the pipeline every step)
        if (steps) {
            fetch_desc(0);
            issue(vA, gA);
            if (steps > 1) fetch_desc(1);
            uint32_t j = 0;
            for (; j + 2 < steps; j += 2) {
                issue(vB, gB);         // step j+1
                fetch_desc(j + 2);
                consume(vA, gA);       // step j
                issue(vA, gA);         // step j+2
                fetch_desc(j + 3 < steps ? j + 3 : steps - 1);
                consume(vB, gB);       // step j+1
            }
            if (j + 1 < steps) {  // two steps left: A in flight, B's descriptors fetched
                issue(vB, gB);
                consume(vA, gA);
                consume(vB, gB);
            } else {
                consume(vA, gA);
            }
        }
        for (uint32_t s = steps * SB; s < n_sources; ++s) {
            glb_cf4 *const ptr = (glb_cf4 *)(uintptr_t)(desc[4 * (uint64_t)s]);
            const float g = dgain[8 * (uint64_t)s + 4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const v4f v = IN::f(__builtin_nontemporal_load(ptr + base + (uint64_t)u * 256u));
                acc[u].x = fma_(g, v.x, acc[u].x);
                acc[u].y = fma_(g, v.y, acc[u].y);
                acc[u].z = fma_(g, v.z, acc[u].z);
                acc[u].w = fma_(g, v.w, acc[u].w);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) *reinterpret_cast<v4f *>(y + 4 * (base + (uint64_t)u * 256u)) = acc[u];
    } else {  // the last workgroup: vector by vector, guarded
        for (int u = 0; u < U; ++u) {
            const uint64_t i = base + (uint64_t)u * 256u;
            if (i >= nvec) break;
            v4f a = v4f{0.f, 0.f, 0.f, 0.f};
            for (uint32_t s = 0; s < n_sources; ++s) {
                glb_cf4 *const ptr = (glb_cf4 *)(uintptr_t)(desc[4 * (uint64_t)s]);
                const float g = dgain[8 * (uint64_t)s + 4];
                const v4f v = IN::f(ptr[i]);
                a.x = fma_(g, v.x, a.x), a.y = fma_(g, v.y, a.y), a.z = fma_(g, v.z, a.z), a.w = fma_(g, v.w, a.w);
            }
            *reinterpret_cast<v4f *>(y + 4 * i) = a;
        }
    }
    if (blockIdx.x == 0) {
        const uint64_t t = nvec * 4 + threadIdx.x;  // the floats behind the last whole vector (a mono batch of a length not divisible by 4)
        if (t < n_floats) {
            float a = 0.f;
            for (uint32_t s = 0; s < n_sources; ++s) a = fma_(dgain[8 * (uint64_t)s + 4], IN::f1(((IN::GS *)(uintptr_t)(desc[4 * (uint64_t)s]))[t]), a);
            y[t] = a;
        }
        if (threadIdx.x == 0) {  // the one-entry descriptor table the fused launch behind this one reads
            ydesc->data = desc_row;  // the row the launch behind this one reads: the mix, or what a filter makes of it
            ydesc->frames = frames;
            ydesc->out_frames = out_frames;
            ydesc->gain = 1.0f;
            ydesc->pad[0] = ydesc->pad[1] = ydesc->pad[2] = 0;
        }
    }
}

// The same sum for long rows, in the shape that reaches the read ceiling of this part (tools/ubench/stream_ring: 7.19 TB/s):
// one wave owns chunk t -- 8 KiB, aligned -- of EVERY source; it pulls the chunks through a ring of NS LDS stages with LDS-DMA
// (8 instructions of 1 KiB per source, no registers held by data in flight), reads its own 8 vectors of a landed stage back
// and accumulates.  A row of n_floats gives ceil(n_floats / 2048) waves: for rows that fill the chip (the host decides).
template <int NS>
__global__ __launch_bounds__(64) void k_mix_ring(const SrcDesc *__restrict__ srcs, const uint32_t n_sources, float *__restrict__ y, const uint64_t n_floats, SrcDesc *__restrict__ ydesc,
                                                 const uint32_t frames, const uint32_t out_frames, const float *desc_row, const uint64_t src_off) {
    constexpr int KV = 8;
    constexpr uint32_t kStage = KV * 1024;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * kStage];
    lds_u8 *const lds = (lds_u8 *)smem;
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;
    typedef __attribute__((address_space(4))) const uint64_t cu64;
    typedef __attribute__((address_space(4))) const float cf32;
    cu64 *const desc = (cu64 *)(uintptr_t)srcs;
    cf32 *const dgain = (cf32 *)(uintptr_t)srcs;
    const int lane = threadIdx.x;
    const uint64_t nvec = n_floats / 4;
    const uint64_t v0 = (uint64_t)blockIdx.x * (KV * 64);  // first vector of this wave's chunk
    // byte offsets of this lane's KV vectors inside a row; vectors past the end of the row re-fetch its last one (never stored)
    uint32_t goff[KV];
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        uint64_t j = v0 + (uint64_t)k * 64 + lane;
        j = j < nvec ? j : nvec - 1;
        goff[k] = (uint32_t)(j * 16);  // rows are < 2^32 bytes (frames < 2^29)
    }
    auto stage_source = [&](uint32_t s_, uint32_t stage) {
        const void *data = (const void *)(uintptr_t)(desc[4 * (uint64_t)s_] + src_off);
#pragma unroll
        for (int k = 0; k < KV; ++k) glds16(data, goff[k], lds0 + stage * kStage + k * 1024);
    };
    v4f acc[KV];
#pragma unroll
    for (int k = 0; k < KV; ++k) acc[k] = v4f{0.f, 0.f, 0.f, 0.f};
    if (v0 < nvec) {
#pragma unroll
        for (int d = 0; d < NS - 1; ++d)
            if ((uint32_t)d < n_sources) stage_source(d, d);
        uint32_t st = 0;
        float g_next = n_sources ? dgain[4] : 0.f;
        for (uint32_t s_ = 0; s_ < n_sources; ++s_) {
            const float g = g_next;
            g_next = s_ + 1 < n_sources ? dgain[8 * (uint64_t)(s_ + 1) + 4] : 0.f;
            // the stage that source s_-1 was read from is free (its reads were waited for): source s_+NS-1 goes there
            if (s_ + NS - 1 < n_sources) {
                uint32_t into = st + NS - 1;
                into = into >= (uint32_t)NS ? into - NS : into;
                stage_source(s_ + NS - 1, into);
                wait_vm<KV *(NS - 1)>();
            } else {
                const uint32_t left = n_sources - 1 - s_;  // groups issued after this source's
                wait_groups<KV, NS>((int)left);
            }
            const lds_u8 *buf = lds + st * kStage;
            v4f v[KV];
#pragma unroll
            for (int k = 0; k < KV; ++k) v[k] = *(const lds_f4 *)(buf + k * 1024 + lane * 16);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the stage may be re-targeted by the next DMA
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                acc[k].x = fma_(g, v[k].x, acc[k].x);
                acc[k].y = fma_(g, v[k].y, acc[k].y);
                acc[k].z = fma_(g, v[k].z, acc[k].z);
                acc[k].w = fma_(g, v[k].w, acc[k].w);
            }
            st = st + 1 == (uint32_t)NS ? 0 : st + 1;
        }
        wait_vm<0>();
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const uint64_t j = v0 + (uint64_t)k * 64 + lane;
            if (j < nvec) *reinterpret_cast<v4f *>(y + 4 * j) = acc[k];
        }
    }
    if (blockIdx.x == 0) {
        const uint64_t t = nvec * 4 + lane;  // the floats behind the last whole vector
        if (t < n_floats) {
            float a = 0.f;
            for (uint32_t s_ = 0; s_ < n_sources; ++s_) a = fma_(dgain[8 * (uint64_t)s_ + 4], ((glb_cf32 *)(uintptr_t)(desc[4 * (uint64_t)s_] + src_off))[t], a);
            y[t] = a;
        }
        if (lane == 0) {
            ydesc->data = desc_row;  // the row the launch behind this one reads: the mix, or what a filter makes of it
            ydesc->frames = frames;
            ydesc->out_frames = out_frames;
            ydesc->gain = 1.0f;
            ydesc->pad[0] = ydesc->pad[1] = ydesc->pad[2] = 0;
        }
    }
}

// Block streaming with per-source filter states (k_rlm_wave): after a block of n_tiles whole tiles, the state of
// source s at the block's end is what tile n_tiles would have received as its carry -- the look-back over the
// aggregates the block has just published (and, for short blocks, the previous block-start state in column 0).
// One lane per source; the result becomes column 0 of the next launch (tagged with ITS epoch).  col_next = 0
// writes the zero state a stream starts from.
__global__ __launch_bounds__(64) void k_rlm_state(unsigned long long *gran, const Tables *__restrict__ tabs, uint32_t n_sources, uint32_t ncol, uint32_t col_next, uint32_t J,
                                                  uint32_t epoch, uint32_t next_epoch) {
    const uint32_t s = blockIdx.x * 64u + threadIdx.x;
    if (s >= n_sources) return;
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    const uint32_t Jc = J < col_next ? J : col_next;
    unsigned long long *row = gran + (uint64_t)s * ncol * 4;
    for (uint32_t j = 0; j < Jc; ++j) {
        const unsigned long long *g = row + (uint64_t)(col_next - 1 - j) * 4;
        const unsigned long long g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
        // a source that had ended before that tile published nothing there: it has no state to carry either
        if ((uint32_t)(g0 >> 32) != epoch || (uint32_t)(g1 >> 32) != epoch || (uint32_t)(g2 >> 32) != epoch || (uint32_t)(g3 >> 32) != epoch) continue;
        const float kM[4] = {tabs->lookM[j][0], tabs->lookM[j][1], tabs->lookM[j][2], tabs->lookM[j][3]};
        mat_acc(kM, __uint_as_float((uint32_t)g0), __uint_as_float((uint32_t)g1), c[0], c[1]);
        mat_acc(kM, __uint_as_float((uint32_t)g2), __uint_as_float((uint32_t)g3), c[2], c[3]);
    }
    for (int q = 0; q < 4; ++q) row[q] = ((unsigned long long)next_epoch << 32) | __float_as_uint(c[q]);
}

// A stream with a state per source whose live sources run together again (the others have ended and given everything): the summed
// state the fused kernel streams on is the sum of the live sources' states -- column 0 of their rows, which k_rlm_state has just written
// (tagged `tag`).  A source the table marks with gain 0 is gone (or mute: its state is zero then) and stays out.  One workgroup.
__global__ __launch_bounds__(256) void k_rlm_state_sum(const unsigned long long *__restrict__ gran, const SrcDesc *__restrict__ srcs, uint32_t n_sources, uint32_t ncol, uint32_t tag,
                                                      float *__restrict__ w_out) {
    __shared__ float part[4][256];
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    for (uint32_t s = threadIdx.x; s < n_sources; s += 256u) {
        if (srcs[s].gain == 0.0f) continue;
        const unsigned long long *row = gran + (uint64_t)s * ncol * 4;
        const unsigned long long g0 = row[0], g1 = row[1], g2 = row[2], g3 = row[3];
        if ((uint32_t)(g0 >> 32) != tag || (uint32_t)(g1 >> 32) != tag || (uint32_t)(g2 >> 32) != tag || (uint32_t)(g3 >> 32) != tag) continue;
        c[0] += __uint_as_float((uint32_t)g0), c[1] += __uint_as_float((uint32_t)g1), c[2] += __uint_as_float((uint32_t)g2), c[3] += __uint_as_float((uint32_t)g3);
    }
    for (int q = 0; q < 4; ++q) part[q][threadIdx.x] = c[q];
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int q = 0; q < 4; ++q) part[q][threadIdx.x] += part[q][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 4) w_out[threadIdx.x] = part[threadIdx.x][0];
}

}  // namespace

namespace rhp {

// Mix first: a filtered batch of equal-length sources -- or a block of a stream on the summed state -- is summed at the input rate
// (k_mix_rows / k_mix_ring: the one pass over the input; filter_first: then filtered there), and `k` becomes the fused launch that converts
// and filters that ONE stream
rh::rlm::RowCut mixed_row_cut(const rh_rlm *p, uint32_t count, bool pre, const StreamArgs &sa) {
    const uint64_t n_floats = (uint64_t)p->eq_frames * p->cfg.channels;
    const char *ku = rh::knob(rh::K_MIX_U), *kg = rh::knob(rh::K_MIX_GROUPS);
    return rh::rlm::row_cut({n_floats, count, (uint32_t)rh::g_num_cus, pre, sa.mode != 0, (uint64_t)p->cfg.max_in_frames * p->cfg.channels, ku ? atoi(ku) : rh::rlm::kUnset,
                             kg ? atoi(kg) : rh::rlm::kUnset});
}

rh_status launch_mixed(rh_rlm *p, const Plan &pl, Params &k, bool pre, const StreamArgs &sa, rh_stream stream, bool pcm16) {
    hipStream_t s = rh::as_stream(stream);
    const uint32_t count = k.n_sources;
    const uint64_t n_floats = (uint64_t)p->eq_frames * p->cfg.channels;
    const rh::rlm::RowCut c = mixed_row_cut(p, count, pre, sa);
    if (pcm16 && (c.ring || pre || sa.mode)) return RH_ERR_UNSUPPORTED;  // (rh_rlm_pcm16.h sends only k_mix_rows' one-shot runs here)
    if (c.need > p->mix_floats) {
        const rh_status w = wait_idle(p);
        if (w != RH_OK) return w;
        if (p->d_mix) RH_HIP_TRY(hipFree(p->d_mix));
        p->d_mix = nullptr;
        RH_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p->d_mix), c.need * sizeof(float)));
        p->mix_floats = c.need;
    }
    SrcDesc *const ydesc = reinterpret_cast<SrcDesc *>(p->d_mix + rh::rlm::row_cut_desc_offset(p->mix_floats));
    float *const frow = pre ? p->d_mix + c.row : p->d_mix;  // the row the fused launch reads
    const uint32_t nf = p->eq_frames, mf = (uint32_t)p->out_frames;
    if (pcm16) {  // the int16 rows themselves, through their own table
        if (c.U == 1) hipLaunchKernelGGL(k_mix_rows_pcm16<1>, dim3(c.wgs, c.groups), dim3(256), 0, s, p->d_pcm, count, p->d_mix, n_floats, ydesc, nf, mf, frow, (uint64_t)c.row);
        else if (c.U == 2) hipLaunchKernelGGL(k_mix_rows_pcm16<2>, dim3(c.wgs, c.groups), dim3(256), 0, s, p->d_pcm, count, p->d_mix, n_floats, ydesc, nf, mf, frow, (uint64_t)c.row);
        else hipLaunchKernelGGL(k_mix_rows_pcm16<4>, dim3(c.wgs, c.groups), dim3(256), 0, s, p->d_pcm, count, p->d_mix, n_floats, ydesc, nf, mf, frow, (uint64_t)c.row);
    } else if (c.ring >= 3) hipLaunchKernelGGL(k_mix_ring<3>, dim3((uint32_t)c.ring_waves), dim3(64), 0, s, k.srcs, count, p->d_mix, n_floats, ydesc, nf, mf, frow, sa.src_off);
    else if (c.ring == 2) hipLaunchKernelGGL(k_mix_ring<2>, dim3((uint32_t)c.ring_waves), dim3(64), 0, s, k.srcs, count, p->d_mix, n_floats, ydesc, nf, mf, frow, sa.src_off);
    else if (c.U == 1) hipLaunchKernelGGL(k_mix_rows<1>, dim3(c.wgs, c.groups), dim3(256), 0, s, k.srcs, count, p->d_mix, n_floats, ydesc, nf, mf, frow, (uint64_t)c.row, sa.src_off);
    else if (c.U == 2) hipLaunchKernelGGL(k_mix_rows<2>, dim3(c.wgs, c.groups), dim3(256), 0, s, k.srcs, count, p->d_mix, n_floats, ydesc, nf, mf, frow, (uint64_t)c.row, sa.src_off);
    else hipLaunchKernelGGL(k_mix_rows<4>, dim3(c.wgs, c.groups), dim3(256), 0, s, k.srcs, count, p->d_mix, n_floats, ydesc, nf, mf, frow, (uint64_t)c.row, sa.src_off);
    RH_CHECK_LAUNCH();
    if (pre) {  // the filter of `src.low_pass(f)`, at from_rate, on the mix (time-parallel: rh_biquad mode 1, zero state)
        const rh_status fs = rh_biquad(frow, p->d_mix, p->eq_frames, p->cfg.channels, 1, p->pre_coeffs, nullptr, 1, stream);
        if (fs != RH_OK) return fs;
    }
    k.srcs = ydesc;
    k.n_sources = c.groups;  // (the partial rows, added in order by the fused launch; one row when the list was not cut)
    // every tile of the one-stream launch resident at once: no tickets (see Params::direct)
    k.direct = rh::rlm::all_resident(p->exclusive, p->n_tiles, (uint64_t)rh::g_num_cus, pl.resident_per_cu) ? 1u : 0u;
    return RH_OK;
}

void launch_state(hipStream_t s, unsigned long long *gran, const Tables *tabs, uint32_t n_sources, uint32_t cols, uint32_t last_col, uint32_t J, uint32_t epoch, uint32_t next_epoch) {
    hipLaunchKernelGGL(k_rlm_state, dim3((n_sources + 63) / 64), dim3(64), 0, s, gran, tabs, n_sources, cols, last_col, J, epoch, next_epoch);
}

void launch_state_sum(hipStream_t s, const unsigned long long *gran, const SrcDesc *srcs, uint32_t n_sources, uint32_t cols, uint32_t tag, float *w_out) {
    hipLaunchKernelGGL(k_rlm_state_sum, dim3(1), dim3(256), 0, s, gran, srcs, n_sources, cols, tag, w_out);
}

}  // namespace rhp
