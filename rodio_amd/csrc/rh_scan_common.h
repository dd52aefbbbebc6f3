// rh_scan_common.h -- device helpers shared by the time-parallel scan kernels (rh_limit.hip, rh_biquad_scan.hip):
// DPP cross-lane moves, wave reductions, the f32 hand-off words with their 0xFF "not yet" pattern, the swizzled LDS
// tile image and its LDS-DMA fetch; at the end the host's side of a launch: scan_launch() over the protocol of rh_scan_launch.h.
// gfx950 only; include inside an anonymous namespace of a .hip file.
#pragma once
#include <type_traits>

#include "rh_common.h"
#include "rh_lanes.h"  // fma_, dpp0 and its control words, readlane_f, mat_acc

// plain sums / maxima over the wave (all values >= 0: zero-fill is neutral)
__device__ __forceinline__ float wave_excl_sum(float v, float &total) {
    v += dpp0<kDppRowShr + 1, 0xf>(v);
    v += dpp0<kDppRowShr + 2, 0xf>(v);
    v += dpp0<kDppRowShr + 4, 0xf>(v);
    v += dpp0<kDppRowShr + 8, 0xf>(v);
    v += dpp0<kDppBcast15, 0xa>(v);
    v += dpp0<kDppBcast31, 0xc>(v);
    total = readlane_f(v, 63);
    return dpp0<kDppWaveShr1, 0xf>(v);
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp0<kDppRowShr + 1, 0xf>(v));
    v = fmaxf(v, dpp0<kDppRowShr + 2, 0xf>(v));
    v = fmaxf(v, dpp0<kDppRowShr + 4, 0xf>(v));
    v = fmaxf(v, dpp0<kDppRowShr + 8, 0xf>(v));
    v = fmaxf(v, dpp0<kDppBcast15, 0xa>(v));
    v = fmaxf(v, dpp0<kDppBcast31, 0xc>(v));
    return readlane_f(v, 63);
}

// ---- two channels per instruction ------------------------------------------------------------------------------------------
// The limiter spends most of its issue slots on vector arithmetic (r02 PMC: 47 instructions per sample), and gfx950 executes the f32
// multiply / add / FMA on PAIRS of registers at full rate (v_pk_mul_f32, v_pk_add_f32, v_pk_fma_f32).  With an even channel
// count the channels of a frame go through the per-sample arithmetic two at a time (T = f2); the operations are the same IEEE
// operations in the same order, so the bits do not change.  max, log2, exp2, compares and DPP moves have no packed form.
typedef float f2 __attribute__((ext_vector_type(2)));
template <int C>
struct Pk {
    static constexpr int W = C % 2 == 0 ? 2 : 1, N = C / W;
    typedef typename std::conditional<W == 2, f2, float>::type T;
};
template <class T>
__device__ __forceinline__ T splat(float s);
template <>
__device__ __forceinline__ float splat<float>(float s) { return s; }
template <>
__device__ __forceinline__ f2 splat<f2>(float s) { return (f2)(s); }
__device__ __forceinline__ float vfma(float a, float b, float c) { return fma_(a, b, c); }
__device__ __forceinline__ f2 vfma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float vmax(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ f2 vmax(f2 a, f2 b) {
    f2 r;
    r.x = fmaxf(a.x, b.x), r.y = fmaxf(a.y, b.y);
    return r;
}
__device__ __forceinline__ float comp(float v, int) { return v; }
__device__ __forceinline__ float comp(f2 v, int i) { return i ? v.y : v.x; }
__device__ __forceinline__ float pair_of(const float *p, float) { return p[0]; }
__device__ __forceinline__ f2 pair_of(const float *p, f2) {
    f2 r;
    r.x = p[0], r.y = p[1];
    return r;
}
template <int CTRL, int MASK>
__device__ __forceinline__ float vdpp(float v) { return dpp0<CTRL, MASK>(v); }
template <int CTRL, int MASK>
__device__ __forceinline__ f2 vdpp(f2 v) {
    f2 r;
    r.x = dpp0<CTRL, MASK>(v.x), r.y = dpp0<CTRL, MASK>(v.y);
    return r;
}
__device__ __forceinline__ float vsel(bool c, float a, float b) { return c ? a : b; }
__device__ __forceinline__ f2 vsel(bool c, f2 a, f2 b) { return c ? a : b; }


constexpr uint32_t kNotYet = 0xffffffffu;
__device__ __forceinline__ bool word_ok(float v) { return __float_as_uint(v) != kNotYet; }
__device__ __forceinline__ void word_store(float *p, float v) {
    v = v != v ? __uint_as_float(0x7fc00000u) : v;  // a NaN travels in canonical form, never as the sentinel
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// What a launch that is not "clean" (rh_scan_launch.h) finds in its scratch, written by ONE kernel of this library in front of it -- the
// unit's own, which also takes its snapshots: the control words (ticket counter, status) zeroed, every hand-off word of both tables "not
// yet".  Thread i0 of `step`.  Neither hipMallocAsync/hipFreeAsync per call nor hipMemsetAsync: with them ~7 % of short GpuSource chains
// carried a wrong state into one tile (a zero aggregate or a zeroed state snapshot where the launch had written something else); either
// change alone lowered the rate, only both removed it (profiles/archive/r02_limit_flake.md).
__device__ __forceinline__ void scan_scratch_init(uint32_t *ctl, uint32_t *words, uint64_t n_words, uint64_t i0, uint64_t step) {
    if (i0 < 16) ctl[i0] = 0u;
    for (uint64_t i = i0; i < n_words; i += step) words[i] = kNotYet;
}
typedef float v2f_ __attribute__((ext_vector_type(2)));
typedef float v4f_ __attribute__((ext_vector_type(4)));
// N consecutive words with agent-scope (sc1: served by L2, never by this CU's L1) loads of width W.  The loads are inline
// asm -- hipcc does not see them -- so wait_loads() must stand between them and the first use of the values.
template <int N, int W>
__device__ __forceinline__ void load_words(const float *p, float (&out)[N]) {
    static_assert(N % W == 0, "section width");
#pragma unroll
    for (int k = 0; k < N; k += W) {
        if (W == 4) {
            v4f_ r;
            asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(r) : "v"(p + k) : "memory");
            out[k] = r.x, out[k + 1] = r.y, out[k + 2] = r.z, out[k + 3] = r.w;
        } else if (W == 2) {
            v2f_ r;
            asm volatile("global_load_dwordx2 %0, %1, off sc1" : "=v"(r) : "v"(p + k) : "memory");
            out[k] = r.x, out[k + 1] = r.y;
        } else {
            float r;
            asm volatile("global_load_dword %0, %1, off sc1" : "=v"(r) : "v"(p + k) : "memory");
            out[k] = r;
        }
    }
}
template <int N>
__device__ __forceinline__ void wait_loads(float (&v)[N]) {  // the values are operands: nothing that uses them can move above the wait
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("" : "+v"(v[k]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("" : "+v"(v[k]));
}

// ... with at most YOUNGER vector-memory instructions of this wave still in flight: vmcnt retires in order, so loads that were issued in FRONT of
// YOUNGER others have arrived when the count is down to YOUNGER.  (The caller knows that at least that many were issued behind them.)
template <int YOUNGER, int N>
__device__ __forceinline__ void wait_loads_behind(float (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("" : "+v"(v[k]));
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(YOUNGER) : "memory");
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("" : "+v"(v[k]));
}

typedef float v4f __attribute__((ext_vector_type(4)));

// ---- the tile's samples in LDS -------------------------------------------------------------------------------------------
// A wave's share of a tile (64 lanes x V 16-byte vectors, V KiB) sits in LDS as 64*V slots.  Slot o*V + (j ^ f(o)) holds
// vector j of lane o's run; f swizzles the vectors of neighbouring runs so that the 16 lanes one ds_read_b128 / ds_write_b128
// pass serves hit 16 different bank groups although the rows are not padded (V a power of two <= 16; other V: f = 0, V odd is
// conflict-free anyway).  The image is written by LDS-DMA straight from HBM (global_load_lds_dwordx4: no VGPR round trip,
// issued a whole tile ahead) -- the DMA lane that fills slot q simply fetches the vector that belongs there.
template <int V>
__device__ __forceinline__ constexpr uint32_t slot_of(uint32_t o, uint32_t j) {
    return (V > 1 && V <= 16 && (V & (V - 1)) == 0) ? o * V + (j ^ ((o / (16 / V)) & (V - 1))) : o * V + j;
}
template <int V>
__device__ __forceinline__ constexpr uint32_t vec_in_slot(uint32_t q) {  // the inverse: which vector of the share lives in slot q
    const uint32_t o = q / V, jj = q % V;
    return (V > 1 && V <= 16 && (V & (V - 1)) == 0) ? o * V + (jj ^ ((o / (16 / V)) & (V - 1))) : q;
}
typedef __attribute__((address_space(3))) unsigned char lds_u8;
__device__ __forceinline__ const void *uniform_ptr(const void *q) {
    const uint64_t v = (uint64_t)(uintptr_t)q;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (const void *)(uintptr_t)(((uint64_t)hi << 32) | lo);
}
// One LDS-DMA instruction: 64 lanes x 16 bytes from sbase + voff (per lane) land at LDS byte address lds_dst + lane*16 (M0 is
// compiler-reserved: saved and restored inside the statement, cdna_hip_programming.md 5.7).  hipcc does not see the load;
// `nt`: every sample is read once (streaming fetch, +10 % on the achievable read rate on this part).
__device__ __forceinline__ void glds16(const void *sbase_, uint32_t voff, uint32_t lds_dst_) {
    const void *sbase = uniform_ptr(sbase_);
    const uint32_t lds_dst = __builtin_amdgcn_readfirstlane(lds_dst_);
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst)
                 : "memory");
}
template <int V>
__device__ __forceinline__ void dma_share(const float *src_share, v4f *buf, int lane) {
    asm volatile("" : "+v"(lane));  // not hoisted: see limit_tile
    const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_u8 *)buf;
#pragma unroll
    for (int k = 0; k < V; ++k) glds16(src_share, vec_in_slot<V>(k * 64 + lane) * 16u, lds0 + k * 1024);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- host: one launch ------------------------------------------------------------------------------------------------------
// The stream's scratch (rh::stream_scratch) as a launch sees it: rh::scan::Layout at an address
struct ScanScratch {
    unsigned char *base;
    rh::scan::Layout lay;
    uint32_t *ctl() const { return reinterpret_cast<uint32_t *>(base); }
    float *own() const { return reinterpret_cast<float *>(base + rh::scan::kOwnOffset); }
    uint32_t *words() const { return reinterpret_cast<uint32_t *>(base + lay.head); }
    float *table(uint32_t p) const { return reinterpret_cast<float *>(base + lay.table(p)); }
    // workgroups of 256 for the unit's pre-kernel: it walks both tables (scan_scratch_init) and n_own items of its own
    unsigned pre_wgs(uint64_t n_own) const {
        const uint64_t n = lay.n_words() > n_own ? lay.n_words() : n_own;
        return (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    }
};
inline int knob_int(rh::Knob k) { return rh::knob(k) ? atoi(rh::knob(k)) : 0; }  // 0: unset (or nonsense)

// Everything between a unit's argument block and its kernel on the stream.  `a` (LimitArgs, BqArgs) arrives with n_streams and tiles set
// (rh::scan::tickets_fit) and leaves with gran, gran_other, ticket_base, ctl, status, spin and dma_top; own_bytes is the unit's head of the
// scratch, rec_floats a tile's hand-off record.  pre(scratch) enqueues the unit's kernel in front of the launch (scan_scratch_init + its own
// snapshots) and is called only when that kernel is due -- always with a carried state.  fn stands for the variant in the occupancy query
// (asked once: `occupancy` is the caller's slot for this variant, 0 at first), kernel_for(grid) is what runs; wgs_knob / grid_knob: workgroups
// per CU and grid on request, 0 otherwise.  The caller keeps `hold` until its last launch that uses the scratch is enqueued.
// No std::function, no allocation: a pull shim calls this once per block.
template <class Args, class Pre, class KernelFor>
hipError_t scan_launch(hipStream_t s, std::unique_lock<std::mutex> &hold, uint64_t seed, uint32_t channels, size_t own_bytes, size_t rec_floats, bool carried_state, Args &a,
                       const void *fn, uint32_t block, int &occupancy, int wgs_knob, int grid_knob, Pre pre, KernelFor kernel_for) {
    namespace scan = rh::scan;
    const uint64_t total = (uint64_t)a.tiles * a.n_streams;
    ScanScratch sc{nullptr, scan::layout(own_bytes, (size_t)total * rec_floats * sizeof(float))};
    rh::ScratchAux *aux = nullptr;
    hipError_t e = rh::stream_scratch(s, sc.lay.total(), reinterpret_cast<void **>(&sc.base), hold, &aux);
    if (e != hipSuccess) return e;
    const char *init_knob = rh::knob(rh::K_LIMIT_INIT);  // RH_LIMIT_INIT=1: both scan kernels initialise their tables in front of every launch
    const uint64_t tag = scan::shape_tag(seed, a.n_streams, a.tiles, channels, sc.lay, (uint64_t)reinterpret_cast<uintptr_t>(sc.base));
    const scan::Begin b = scan::begin(aux, tag, carried_state, init_knob && init_knob[0] == '1');
    a.ctl = sc.ctl();
    a.status = rh::g_async_status;
    a.dma_top = rh::knob(rh::K_SCAN_DMA_TOP) ? (uint32_t)atoi(rh::knob(rh::K_SCAN_DMA_TOP)) : 1u;  // measured: 0.312 -> 0.286 ms (limiter), 0.234 -> 0.221 ms (biquad), 64 x 1 Mi frames
    a.spin = rh::knob(rh::K_SCAN_SPIN_LIMIT) ? (uint32_t)strtoul(rh::knob(rh::K_SCAN_SPIN_LIMIT), nullptr, 10) : rh::kSpinLimit;
    a.gran = sc.table(b.table);
    a.gran_other = b.other < 0 ? nullptr : sc.table((uint32_t)b.other);
    if (b.init) e = pre(sc);
    if (rh::scan_jump_due()) {  // RH_COUNTER_JUMP
        const uint32_t d = scan::jump(aux, rh::counter_jump().tickets_left);
        if (e == hipSuccess) e = rh::counters_add(a.ctl, d, 0, 0, s);
    }
    a.ticket_base = aux->ticket_base;
    if (e == hipSuccess && occupancy == 0) {
        int q = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, fn, (int)block, 0);
        occupancy = q < 1 ? 1 : q;
    }
    if (e == hipSuccess) {
        uint64_t grid = scan::launch_grid((uint64_t)rh::g_num_cus, scan::per_cu(occupancy, (int)(block / 64), wgs_knob), total);
        if (grid_knob > 0) grid = (uint64_t)grid_knob;  // diagnostics
        void *args[] = {&a};
        e = hipLaunchKernel(kernel_for(grid), dim3((uint32_t)grid), dim3(block), args, 0, s);
        if (e == hipSuccess) scan::launched(aux, carried_state, total, grid);
    }
    if (e != hipSuccess) scan::failed(aux);
    return e;
}
