// rh_pipeline_chunk.hip -- mix first in one kernel: k_rlm_chunk (the benchmark's kernel), k_rlm_chunk_multi and k_rlm_chunk_classes (the
// filter classes of a mixer in one launch), their instances and the host functions that launch them.
#include "rh_pipeline_dev.h"

namespace {

// =================================================================================================
// k_rlm_chunk -- mix first in ONE kernel, for rows long enough to fill the chip (stereo).  Tile t owns the ALIGNED 8 KiB chunk t
// of every source: it sums the chunks through the LDS-DMA ring exactly as k_mix_ring does (the pass that reaches the read
// ceiling, no re-fetched line), and then converts and filters ITS part of the one mixed stream itself -- no mixed row in memory,
// no second launch.  What makes that possible:
//   * a tile's output frames are those whose SECOND tap lies in its chunk (frames m_lo[t] .. m_lo[t+1]-1, a table of the host's:
//     1114 or 1115 of them at 44.1 -> 48 kHz): the only input a tile lacks is the end of the chunk before it -- the first tap of
//     its first frame, and the taps of the two frames x'[m_lo-1], x'[m_lo-2] the filter looks back at.  Those are MIXED frames:
//     the tile before publishes its last 4 of them (tagged words, like the aggregates) as soon as its source loop ends;
//   * lanes take runs of R frames as in k_rlm_fast; the tile's last lane takes what is left (v <= R frames) and the lanes behind
//     it idle.  The scan is the uniform one; only the tile aggregate needs the short run: A = B^v * (prefix of the lane before)
//     + (own run), one 2x2 product with a table of B^v;
//   * tiles have different lengths, so the look-back weights B^(m_lo[t] - m_lo[t-j]) come from a table per tile (host, f64).
// Waits only ever go to EARLIER tiles, and the host launches this kernel only when every tile is resident at once.
// =================================================================================================
struct ChunkArgs {
    const uint32_t *m_lo;      // [n_tiles + 1]: first output frame of every tile; m_lo[n_tiles] = out_frames
    unsigned long long *halo;  // [n_tiles][8] {epoch, f32 bits}: the last 4 mixed frames of the tile's chunk
    const float *lookT;        // [n_tiles][J][4]: B^(m_lo[t] - m_lo[t-j]), j = 0 .. J-1 (the weight of tile t-1-j's aggregate)
    const float *powM;         // [R + 1][4]: B^v
    const float *uni;          // the plan's Uniforms as an array of floats in device memory (Params::u holds the same values)
};
constexpr uint32_t kChunkMultiMax = 7;  // classes in one launch (k_rlm_chunk_multi): what fits the 4 KiB kernarg segment
struct ChunkMulti {
    struct Entry {
        Params p;
        ChunkArgs q;
    };
    uint32_t n;                          // classes in this launch
    uint32_t first[kChunkMultiMax + 1];  // first workgroup of every class (multiples of 8: a workgroup's XCD is its class-relative index's too); [n] = the grid
    float *sum_out;                      // k_rlm_chunk_classes: where the SUM of the classes' mixes goes (the classes' own rows stay unwritten)
    Entry e[kChunkMultiMax];
};
static_assert(sizeof(ChunkMulti) <= 4096, "the kernarg segment");
#if defined(RH_CHUNK_DIAG) && RH_CHUNK_DIAG == 3  // diagnostics builds: shader cycles per phase behind the source loop, summed over the tiles into ctl[8..15]
#define RH_CPH(i) { const unsigned long long cph_now = __builtin_readcyclecounter(); if (lane == 0) atomicAdd(p.ticket + 8 + (i), (uint32_t)(cph_now - cph_last)); cph_last = cph_now; }
#define RH_CPH_DECL unsigned long long cph_last = __builtin_readcyclecounter();
#else
#define RH_CPH(i)
#define RH_CPH_DECL
#endif
// C: channels of a frame; KV: KiB of a chunk (8 for stereo: 1024 frames; 4 for mono: 1024 frames too -- the tile stays at 64 runs of 18).
// ST: the sources' sample type.  float: k_rlm_chunk.  int16_t: k_rlm_chunk_pcm16 -- the rows are interleaved 16-bit PCM as they lie in a WAV data
// chunk; a chunk of P frames is half as many bytes, so the ring's bytes hold FOUR stages of KV * 512 bytes (KV / 2 DMA instructions a lane each:
// the same bytes in flight), and the lane reads the 8 bytes at k * 512 + lane * 8 of a landed stage for acc[k] -- the four samples whose floats
// the f32 kernel's lane reads there.  float(s) / 32768 is exact (dasp's i16 -> f32, rh_convert_i16_to_f32), so fma(g, float(s) / 32768, acc) in
// the sources' order gives the bits of converting first; only the source loop knows the sample type.
template <int R, int C, int KV, typename ST = float>
__device__ __forceinline__ void rlm_chunk_tile(const Params &p, const ChunkArgs &q, const uint32_t block) {
    typedef Chan<C> CH;
    typedef typename CH::V V;
    constexpr bool PCM = sizeof(ST) == 2;
    constexpr int NS = 2, H = 4;
    constexpr uint32_t FB = CH::kFB;
    constexpr uint32_t kStage = KV * 1024, P = kStage / FB;   // bytes of a ring stage = one chunk; frames per chunk
    constexpr int NSI = PCM ? 2 * NS : NS;                    // stages of the ring as the source loop cuts it, of kIn bytes each:
    constexpr uint32_t kIn = PCM ? kStage / 2 : kStage;       // ... a chunk of the sources' samples
    constexpr int G = PCM ? KV / 2 : KV;                      // DMA instructions (1 KiB) of a chunk
    static_assert(KV % 2 == 0 && NSI * kIn == NS * kStage, "the ring's bytes, cut for either sample type");
    constexpr uint32_t MB = NS * kStage + 64;                 // the mixed chunk: halo frames at MB - H * FB .. MB, 16 spare bytes behind it
    __shared__ __attribute__((aligned(1024))) unsigned char smem[MB + kStage + 64];
    lds_u8 *const lds = (lds_u8 *)smem;
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;
    typedef __attribute__((address_space(4))) const uint64_t cu64;
    typedef __attribute__((address_space(4))) const float cf32;
    typedef __attribute__((address_space(4))) const uint32_t cu32;
    cu64 *const desc = (cu64 *)(uintptr_t)p.srcs;
    cf32 *const dgain = (cf32 *)(uintptr_t)p.srcs;
    const int lane = threadIdx.x;
    // Every tile resident at once (the host knows): tile = workgroup.  More tiles than slots: tiles are handed out by a ticket, so
    // that a tile only ever waits for tiles that already run or have finished (its waits go to earlier tiles only).
    uint32_t tile = block;
    if (!p.direct) {
        // One device-scope counter hands out ~85 tickets per microsecond: 12 us for the 1024 tiles of the benchmark batch, 4 % of
        // the launch.  So the tickets come from EIGHT counters on separate cache lines, one per XCD: workgroup b takes ticket k of
        // counter b % 8 and works on tile b % 8 + 8 k.  Every XCD dispatches its own workgroups (those with its b % 8) in order, so a
        // workgroup's tile is its own index unless its neighbours of the same XCD overtake it -- and a tile still only ever waits
        // for tiles that hold a slot or are done: the lowest unfinished tile of a counter is held by a workgroup that runs, or all
        // earlier workgroups of that XCD have finished and the next one starts.  (The grid is rounded up to whole rounds of eight, so
        // that every counter advances by the same amount per launch: workgroups past the last tile leave.)
        const uint32_t x = block & 7u;
        const uint32_t k = __builtin_amdgcn_readfirstlane(lane == 0 ? atomicAdd(p.ticket + 32u * (1u + x), 1u) - p.shard_base : 0u);
        tile = x + 8u * k;
        if (tile >= p.n_tiles) return;
    }
#ifdef RH_CHUNK_RAGSIM  // diagnostics builds: the load profile of a ragged batch (lengths uniform in [N/2, N]) on the equal batch's data -- timing only
    const uint32_t Ns = p.eq_frames;
    const uint32_t S = 2u * tile < p.n_tiles ? p.n_sources : (uint32_t)(((uint64_t)p.n_sources * 2u * (p.n_tiles - tile)) / p.n_tiles);
#else
    const uint32_t Ns = p.eq_frames, S = p.n_sources;
#endif
    const uint32_t m_lo = ((cu32 *)(uintptr_t)q.m_lo)[tile], m_hi = ((cu32 *)(uintptr_t)q.m_lo)[tile + 1];
    const uint32_t m0 = m_lo + (uint32_t)lane * R;
    int nfl;  // frames of this lane's run
    // what the part behind the source loop needs of the tile's bounds lives in VECTOR registers across the loop (scalar registers
    // are short there, and a scalar load behind the loop is a memory round trip nothing hides): the frame count and B^v
    uint32_t n_t_v;
    float pwv[4];
    {
        const uint32_t n_t = m_hi - m_lo;  // <= 64 * R (host)
        nfl = (int)n_t - lane * R < 0 ? 0 : ((int)n_t - lane * R > R ? R : (int)n_t - lane * R);
        const uint32_t nl0 = (n_t + R - 1) / R;
        const uint32_t v = nl0 ? n_t - (nl0 - 1) * R : 0;  // frames of the last lane's run, 1 .. R
        n_t_v = n_t;
        asm volatile("v_mov_b32 %0, %1" : "=v"(n_t_v) : "s"(n_t));
        const float *pw = q.powM + 4 * v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pwv[k] = pw[k];
            asm volatile("" : "+v"(pwv[k]));  // (a vector load of a uniform address: the values stay in vector registers)
        }
    }
    const bool first = (m0 == 0);                              // stream start: x'[-1] = x'[-2] = 0

    // ---- the sum of chunk `tile` of every source (k_mix_ring) ----
    const uint32_t nvec = PCM ? Ns * C / 8 : Ns * C / 4;  // 16-byte vectors of a row (host: whole vectors -- of the sources' samples)
    const uint32_t v0 = tile * (G * 64);
    uint32_t goff[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        uint32_t j = v0 + (uint32_t)k * 64 + lane;
        j = j < nvec ? j : nvec - 1;  // past the end of the row: its last vector again (finite, never a tap of a stored frame)
        goff[k] = j * 16;
    }
    // every chunk but a row's last lies whole inside the row: its DMA instructions are 1 KiB apart in memory as in the LDS and go
    // out as one run (one M0, one offset register: glds16_run)
    const bool lin = v0 + (uint32_t)(G * 64) <= nvec;
    auto stage_source = [&](uint32_t s_, uint32_t stage) {
        const void *data = (const void *)(uintptr_t)desc[4 * (uint64_t)s_];
        if (lin) {
            glds16_run<G>(data, goff[0], lds0 + stage * kIn);
        } else {
#pragma unroll
            for (int k = 0; k < G; ++k) glds16(data, goff[k], lds0 + stage * kIn + k * 1024);
        }
    };
    if (S) stage_source(0, 0);  // the first two chunks are on their way while the lane works out its taps
    if (S > 1) stage_source(1, 1);
    if constexpr (PCM) {  // (four stages: the first four)
        if (S > 2) stage_source(2, 2);
        if (S > 3) stage_source(3, 3);
    }
    // the lane's rows of the filter tables and its look-back weight: fetched here, a source loop away from their use
    // Everything the part behind the source loop needs from the kernel arguments is worked out HERE and parked in vector
    // registers: a scalar load of a kernel argument behind the loop is a memory round trip that nothing hides (the compiler
    // re-loads arguments rather than keep them: twelve such trips, one after the other, before this was done).
    const Tables *__restrict__ tb = p.tabs;
    float lM[4], b15[4], b31[4], kM[4];
    constexpr int NHV = H * FB / 16;  // vectors that hold the chunk's last 4 frames: the last lanes' last vector
    const uint32_t Jc = p.J < tile ? p.J : tile;
    int want_look = (uint32_t)lane < Jc ? 1 : 0;
    uint64_t a_halo_pub = (uint64_t)(uintptr_t)(q.halo + (uint64_t)tile * 8 + (uint32_t)(lane >= 64 - NHV ? lane - (64 - NHV) : 0) * 4);
    uint64_t a_halo_poll = (uint64_t)(uintptr_t)(q.halo + (uint64_t)(tile ? tile - 1 : 0) * 8 + (lane < H * C ? lane : 0));
    uint64_t a_gran_pub = (uint64_t)(uintptr_t)(p.gran + (uint64_t)tile * 4 + (lane < 2 * C ? lane : 0));
    uint64_t a_gran_poll = (uint64_t)(uintptr_t)(p.gran + (uint64_t)(tile ? tile - 1 - (want_look ? lane : 0) : 0) * 4);
    uint64_t a_out = (uint64_t)(uintptr_t)(p.out + ((uint64_t)m_lo + (uint32_t)lane) * C);  // frame `lane` of the tile
    uint32_t epoch_v = p.epoch;
    float U = q.uni[lane < 61 ? lane : 60];  // lane l holds float l of the Uniforms: {b0, c1, c2, a1, a2, Tm[4], scanM[4][4], g[r][2] ...}
    asm volatile("" : "+v"(want_look), "+v"(a_halo_pub), "+v"(a_halo_poll), "+v"(a_gran_pub), "+v"(a_gran_poll), "+v"(a_out), "+v"(epoch_v), "+v"(U));
    {
        const uint32_t Jc0 = Jc;
        const float *kp = q.lookT + ((uint64_t)tile * p.J + ((uint32_t)lane < Jc0 ? lane : 0)) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lM[k] = tb->laneM[lane][k];
            b15[k] = tb->bc15M[lane][k];
            b31[k] = tb->bc31M[lane][k];
            kM[k] = kp[k];
        }
    }
    // ---- taps and weights of the lane's R + 2 frames: LDS offsets into [halo | chunk] ----
    int offA[R + 2];
    float wgt[R + 2];
    {
        const int64_t fbase = (int64_t)tile * P;
        Cursor c = cursor_at(first ? 0 : m0 - 2, p);
#pragma unroll
        for (int rr = 0; rr < R + 2; ++rr) {
#if defined(RH_CHUNK_DIAG) && RH_CHUNK_DIAG == 2
            offA[rr] = (int)MB + rr * 8;
            wgt[rr] = 0.5f;
            continue;
#endif
            const bool dummy = first && rr < 2;
            uint64_t i;
            uint32_t num;
            cursor_resolve(c, p, i, num);
            if (i + 1 >= Ns) {  // the last frame is emitted verbatim (sample_rate.rs:193-200); frames past it are never stored
                i = Ns - 1;
                num = 0;
            }
            int64_t f = (int64_t)i - fbase;
            f = f < -H ? -H : (f > (int64_t)P - 1 ? (int64_t)P - 1 : f);  // (only frames that are not stored leave the range)
            offA[rr] = dummy ? (int)MB : (int)MB + (int)f * (int)FB;
            wgt[rr] = dummy ? 0.0f : (float)num / p.Tf;
            if (!dummy) cursor_next(c, p);
        }
    }
    v4f acc[KV];
#pragma unroll
    for (int k = 0; k < KV; ++k) acc[k] = v4f{0.f, 0.f, 0.f, 0.f};
    if constexpr (!PCM) {
        uint32_t st = 0;
        float g_next = S ? dgain[4] : 0.f;
        for (uint32_t s_ = 0; s_ < S; ++s_) {
            const float g = g_next;
            g_next = s_ + 1 < S ? dgain[8 * (uint64_t)(s_ + 1) + 4] : 0.f;
            // source s_ has landed when at most the group behind it is outstanding (compiler-issued loads in between only make
            // the wait stricter)
            if (s_ + 1 < S) wait_vm<KV>();
            else wait_vm<0>();
            const lds_u8 *buf = lds + st * kStage;
            v4f v[KV];
#pragma unroll
            for (int k = 0; k < KV; ++k) v[k] = *(const lds_f4 *)(buf + k * 1024 + lane * 16);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the chunk is in registers: its stage is free ...
            if (s_ + 2 < S) stage_source(s_ + 2, st);           // ... for the source after next, requested before this one is summed
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                acc[k].x = fma_(g, v[k].x, acc[k].x);
                acc[k].y = fma_(g, v[k].y, acc[k].y);
                acc[k].z = fma_(g, v[k].z, acc[k].z);
                acc[k].w = fma_(g, v[k].w, acc[k].w);
            }
            st ^= 1u;
        }
    } else {
        uint32_t st = 0;
        float g_next = S ? dgain[4] : 0.f;
        for (uint32_t s_ = 0; s_ < S; ++s_) {
            const float g = g_next;
            g_next = s_ + 1 < S ? dgain[8 * (uint64_t)(s_ + 1) + 4] : 0.f;
            // source s_ has landed when at most the groups behind it are outstanding: those of the next three sources, or of what is left of them
            const uint32_t left = S - 1 - s_;
            wait_groups<G, NSI>((int)(left < (uint32_t)(NSI - 1) ? left : (uint32_t)(NSI - 1)));
            const lds_u8 *buf = lds + st * kIn;
            v4i16 v[KV];
#pragma unroll
            for (int k = 0; k < KV; ++k) v[k] = *(const RH_LDS v4i16 *)(buf + k * 512 + lane * 8);  // the samples of acc[k]: 8 bytes
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the chunk is in registers: its stage is free ...
            if (s_ + NSI < S) stage_source(s_ + NSI, st);        // ... for the source four on, requested before this one is summed
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                acc[k].x = fma_(g, pcm16_f32(v[k].x), acc[k].x);
                acc[k].y = fma_(g, pcm16_f32(v[k].y), acc[k].y);
                acc[k].z = fma_(g, pcm16_f32(v[k].z), acc[k].z);
                acc[k].w = fma_(g, pcm16_f32(v[k].w), acc[k].w);
            }
            st = (st + 1u) & (uint32_t)(NSI - 1);
        }
    }
    RH_CPH_DECL
#if defined(RH_CHUNK_DIAG) && RH_CHUNK_DIAG < 3  // diagnostics builds (tools/build_variant.sh): the source loop alone (+ the tap prologue unless RH_CHUNK_DIAG == 2)
    {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < KV; ++k) t += acc[k].x + acc[k].y + acc[k].z + acc[k].w;
#pragma unroll
        for (int rr = 0; rr < R + 2; ++rr) t += wgt[rr] + (float)offA[rr];
        p.out[(uint64_t)tile * 64 + lane] = t + lM[0] + b15[0] + b31[0] + kM[0] + (float)nfl + (first ? 1.f : 0.f);
        return;
    }
#endif
    // ---- the chunk's last 4 mixed frames to the tile behind (first: it is waiting for them); the mixed chunk into the LDS; the
    // last 4 frames of the tile in front ----
    if (lane >= 64 - NHV) {
        unsigned long long *hp = (unsigned long long *)(uintptr_t)a_halo_pub;
        const float e[4] = {acc[KV - 1].x, acc[KV - 1].y, acc[KV - 1].z, acc[KV - 1].w};
#pragma unroll
        for (int w = 0; w < 4; ++w) __hip_atomic_store(hp + w, ((unsigned long long)epoch_v << 32) | __float_as_uint(e[w]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int k = 0; k < KV; ++k) *(lds_f4 *)(lds + MB + (uint32_t)(k * 64 + lane) * 16) = acc[k];
    if (lane == 0) *(lds_f4 *)(lds + MB + kStage) = v4f{0.f, 0.f, 0.f, 0.f};  // the second tap of a verbatim last frame at the end of a chunk: finite, weight 0
    bool dead = false;
    if (tile == 0) {
        if (lane < H * C) *(RH_LDS float *)(lds + MB - H * FB + lane * 4) = 0.0f;
    } else {
        const bool want = lane < H * C;
        const unsigned long long *hp = (const unsigned long long *)(uintptr_t)a_halo_poll;
        unsigned long long hv = 0;
        bool ok = false;
        uint32_t spins = 0;
        while (true) {
            if (want && !ok) {
                hv = __hip_atomic_load(hp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = (uint32_t)(hv >> 32) == epoch_v;
            }
            if (__all(ok || !want)) break;
            if (++spins > kSpinLimit) {
                if (lane == 0) atomicOr(p.status, 1u);
                dead = true;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (want) *(RH_LDS float *)(lds + MB - H * FB + lane * 4) = dead ? __builtin_nanf("") : __uint_as_float((uint32_t)hv);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    RH_CPH(0)  // LDS image of the mixed chunk + the halo of the tile in front

    // ---- the lane's run of the mixed stream: lerp, zero-state biquad; the run-end state after nfl frames ----
    const float b0 = readlane_f(U, 0), c1 = readlane_f(U, 1), c2 = readlane_f(U, 2), na1 = -readlane_f(U, 3), na2 = -readlane_f(U, 4);
    V out[R];
    V E1 = CH::zero(), E2 = CH::zero();
    {
        V ta[R + 2], tb2[R + 2];
#pragma unroll
        for (int rr = 0; rr < R + 2; ++rr) {
            ta[rr] = CH::ld_lds(lds + offA[rr]);
            tb2[rr] = CH::ld_lds(lds + offA[rr] + FB);
        }
        auto tap = [&](int rr) -> V {
            V x;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) CH::set(x, ch, fma_(CH::get(tb2[rr], ch) - CH::get(ta[rr], ch), wgt[rr], CH::get(ta[rr], ch)));
            return x;
        };
        V x2 = first ? CH::zero() : tap(0);
        V x1 = first ? CH::zero() : tap(1);
        V w1 = CH::zero(), w2 = CH::zero();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const V x = tap(r + 2);
            V w;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const float wc = fma_(na1, CH::get(w1, ch), fma_(na2, CH::get(w2, ch), fma_(c2, CH::get(x2, ch), c1 * CH::get(x1, ch))));
                CH::set(w, ch, wc);
                CH::set(out[r], ch, fma_(b0, CH::get(x, ch), wc));
            }
            w2 = w1;
            w1 = w;
            x2 = x1;
            x1 = x;
            E1 = vsel(r + 1 == nfl, w1, E1);
            E2 = vsel(r + 1 == nfl, w2, E2);
        }
    }
    RH_CPH(1)  // taps, lerp, zero-state run
    // ---- scan of the run-end states (scan basis), as in k_rlm_fast ----
    float Pq[2 * C];
#pragma unroll
    for (int k = 0; k < 2 * C; ++k) Pq[k] = 0.f;
    {
        const float Tm[4] = {readlane_f(U, 5), readlane_f(U, 6), readlane_f(U, 7), readlane_f(U, 8)};
#pragma unroll
        for (int ch = 0; ch < C; ++ch) mat_acc(Tm, CH::get(E1, ch), CH::get(E2, ch), Pq[2 * ch], Pq[2 * ch + 1]);
    }
    float own[2 * C];
#pragma unroll
    for (int k = 0; k < 2 * C; ++k) own[k] = Pq[k];
    scan_states(Pq, ScanStepsLanes{U}, b15, b31);  // (the step matrices from U)
    {  // the tile aggregate: the short last run on top of the inclusive prefix of the lane before it
        const uint32_t n_t = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_t_v);
        float A[2 * C];
        tile_aggregate(own, Pq, pwv, (int)((n_t + R - 1) / R), A);
        if (lane < 2 * C) {
            float ev = A[0];
#pragma unroll
            for (int k = 1; k < 2 * C; ++k) ev = lane == k ? A[k] : ev;
            __hip_atomic_store((unsigned long long *)(uintptr_t)a_gran_pub, ((unsigned long long)epoch_v << 32) | __float_as_uint(ev), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    float Q[2 * C];
#pragma unroll
    for (int k = 0; k < 2 * C; ++k) Q[k] = dpp0<kDppWaveShr1, 0xf>(Pq[k]);  // exclusive: the prefix of the lanes before (all of them whole runs)
    RH_CPH(2)  // scan, aggregate, publish
    // ---- the tile carry: lane j < J polls tile-1-j, weights it with B^(m_lo[tile] - m_lo[tile-j]) ----
    float c[2 * C];
#pragma unroll
    for (int k = 0; k < 2 * C; ++k) c[k] = 0.f;
    if (tile > 0) {
        const bool want = want_look != 0;
        const unsigned long long *gp = (const unsigned long long *)(uintptr_t)a_gran_poll;
        unsigned long long gv[2 * C];
#pragma unroll
        for (int k = 0; k < 2 * C; ++k) gv[k] = 0;
        bool ok = false;
        uint32_t spins = 0;
        while (true) {
            if (want && !ok) {
                bool all = true;
#pragma unroll
                for (int k = 0; k < 2 * C; ++k) {
                    gv[k] = __hip_atomic_load(gp + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    all = all && ((uint32_t)(gv[k] >> 32) == epoch_v);
                }
                ok = all;
            }
            if (__all(ok || !want)) break;
            if (++spins > kSpinLimit) {
                if (lane == 0) atomicOr(p.status, 1u);
                dead = true;
                break;
            }
            __builtin_amdgcn_s_sleep(4);
        }
        if (lane == 0 && spins) atomicAdd(p.status + 1, spins);
        if (want && ok && !dead) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) mat_acc(kM, __uint_as_float((uint32_t)gv[2 * ch]), __uint_as_float((uint32_t)gv[2 * ch + 1]), c[2 * ch], c[2 * ch + 1]);
        }
#pragma unroll
        for (int k = 0; k < 2 * C; ++k) {  // sum over lanes 0..31 -> uniform (half_wave_sum, written out: as a call the stereo kernel grows by 9 instructions)
            c[k] += dpp0<kDppRowShr + 1, 0xf>(c[k]);
            c[k] += dpp0<kDppRowShr + 2, 0xf>(c[k]);
            c[k] += dpp0<kDppRowShr + 4, 0xf>(c[k]);
            c[k] += dpp0<kDppRowShr + 8, 0xf>(c[k]);
            c[k] = readlane_f(c[k], 15) + readlane_f(c[k], 31);
        }
    }
    if (dead) {  // a hand-off that never arrived: the status word fails the call, the tile is poisoned
#pragma unroll
        for (int k = 0; k < 2 * C; ++k) c[k] = __builtin_nanf("");
    }
    RH_CPH(3)  // look-back
#pragma unroll
    for (int ch = 0; ch < C; ++ch) mat_acc(lM, c[2 * ch], c[2 * ch + 1], Q[2 * ch], Q[2 * ch + 1]);  // start state of the lane's run = Q + B^(R*lane) * carry
    // out[r] + the homogeneous correction, through the (now idle) ring stages
    tile_store<R, C>(lds, lane, [&] { return (uint32_t)__builtin_amdgcn_readfirstlane((int)n_t_v); }, [&] { return (float *)(uintptr_t)a_out; }, [&](int r) {
        V y;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) CH::set(y, ch, fma_(readlane_f(U, 25 + 2 * r), Q[2 * ch], fma_(readlane_f(U, 26 + 2 * r), Q[2 * ch + 1], CH::get(out[r], ch))));
        return y;
    });
    RH_CPH(4)  // correction + stores (issue)
}
template <int R, int C, int KV>
__global__ __launch_bounds__(64, 2) void k_rlm_chunk(const Params p, const ChunkArgs q) {
    rlm_chunk_tile<R, C, KV>(p, q, blockIdx.x);
}
// The same tile over sources that are rows of 16-bit PCM (rh_rlm_set_sources_pcm16): whole 16-byte vectors of int16 on 16-byte boundaries
// (rh_rlm_pcm16.h decides).  The tiles, the tickets, m_lo and the look-back tables are the f32 plan's.
template <int R, int C, int KV>
__global__ __launch_bounds__(64, 2) void k_rlm_chunk_pcm16(const Params p, const ChunkArgs q) {
    rlm_chunk_tile<R, C, KV, int16_t>(p, q, blockIdx.x);
}
// Several batches in ONE launch (the filter classes of a mixer, rh_rlm_set_filters): workgroups first[k] .. first[k+1]-1 are class k's launch of
// k_rlm_chunk, with that class's arguments -- its own sources, tables, hand-off words, ticket counters and output row.  Nothing crosses
// between classes; what the one launch saves is the drain and the ramp between launches that each want the whole chip (four classes of the
// benchmark batch: 0.368 ms as four launches).  The arguments are read where they lie, in the kernarg segment: a class index that is not a
// constant would otherwise make the compiler copy the whole block to scratch.
template <int R, int C, int KV>
__global__ __launch_bounds__(64, 2) void k_rlm_chunk_multi(const ChunkMulti m) {
    uint32_t k = 0;
#pragma unroll
    for (uint32_t i = 1; i < kChunkMultiMax; ++i) k += (i < m.n && blockIdx.x >= m.first[i]) ? 1u : 0u;
    uint32_t b0 = 0;
#pragma unroll
    for (uint32_t i = 1; i < kChunkMultiMax; ++i) b0 = (i == k) ? m.first[i] : b0;
    k = __builtin_amdgcn_readfirstlane(k);
    typedef const __attribute__((address_space(4))) unsigned char *cbytes;
    cbytes e = (cbytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(ChunkMulti, e) + (size_t)k * sizeof(ChunkMulti::Entry);
    Params p;
    ChunkArgs q;
    typedef const __attribute__((address_space(4))) uint32_t *cwords;
    static_assert(sizeof(Params) % 4 == 0 && sizeof(ChunkArgs) % 4 == 0 && offsetof(ChunkMulti::Entry, q) % 4 == 0, "copied word by word");
    {
        cwords wp = (cwords)(e + offsetof(ChunkMulti::Entry, p)), wq = (cwords)(e + offsetof(ChunkMulti::Entry, q));
        uint32_t *dp = reinterpret_cast<uint32_t *>(&p), *dq = reinterpret_cast<uint32_t *>(&q);
#pragma unroll
        for (uint32_t i = 0; i < sizeof(Params) / 4; ++i) dp[i] = wp[i];  // (what the tile does not read is never loaded: the copy dissolves into scalar loads)
#pragma unroll
        for (uint32_t i = 0; i < sizeof(ChunkArgs) / 4; ++i) dq[i] = wq[i];
    }
    rlm_chunk_tile<R, C, KV>(p, q, blockIdx.x - b0);
}

// The classes of a mixer in one launch, TWO waves a tile, ONE output (round 6).  A class of 64 sources is a quarter of the headline's bytes, and
// every way of running four of them measured the same 0.36-0.37 ms against the headline's 0.31 for the same bytes: a launch per class,
// the launches lined up in one grid (k_rlm_chunk_multi), a wave that loads while another converts and filters.  The loaders alone take
// 0.308 ms; stamps per tile and class (tools/cls_stamps.py) showed where the rest goes: each class's mix was STORED -- 36 MB of writes in
// all, interleaved with 2 GiB of reads, took 40-55 us of the launch (a run's stores: 55 us a class while the loaders run, 1.5 us once they
// are done) -- and then read again by rh_mix_sum.  So: a workgroup owns chunk `tile` of EVERY class.  Wave 0 only ever loads: it sums the
// chunk over class k's sources through its ring -- the ring does not know about classes, the source after next goes out across a class's
// end -- and leaves the mixed chunk in one of two LDS images (two counters in the LDS, no barrier: it may be two classes ahead).  Wave 1
// converts and filters class k's chunk exactly as k_rlm_chunk's lone wave does (the same operations in the same order) and ADDS the result
// to a run of registers, 0.0 + class 0 + class 1 + ... -- rh_mix_sum's order, the same bits -- which leaves once, as whole lines, when the
// last class is done and the loaders have nothing left to read.  0.317 ms: the classes cost what the headline costs.  For classes of one
// geometry (equal lengths, one rate pair: one table of tile bounds) whose tiles are all resident at once (the host checks: tile =
// workgroup, no ticket); anything else takes k_rlm_chunk_multi and the classes' rows.
#if defined(RH_CLS_DIAG) && RH_CLS_DIAG == 9  // diagnostics builds: wall-clock stamps per (tile, class): loader {sum done, image written}, wave 1 {image seen, halo there, look-back there, done}
__device__ unsigned long long g_cls_stamp[2048 * 8 * 8];
#define RH_CLS_STAMP(i) { if (lane == 0 && tile < 2048 && k < 8) g_cls_stamp[((uint64_t)tile * 8 + k) * 8 + (i)] = wall_clock64(); }
#else
#define RH_CLS_STAMP(i)
#endif
#define RH_PARG(T, e, f) (*(const __attribute__((address_space(4))) T *)((e) + offsetof(ChunkMulti::Entry, p) + offsetof(Params, f)))
#define RH_QARG(T, e, f) (*(const __attribute__((address_space(4))) T *)((e) + offsetof(ChunkMulti::Entry, q) + offsetof(ChunkArgs, f)))
template <int R, int C, int KV>
__global__ __launch_bounds__(128, 2) void k_rlm_chunk_classes(const ChunkMulti m) {
    typedef Chan<C> CH;
    typedef typename CH::V V;
    constexpr int NS = 2, H = 4;
    constexpr uint32_t FB = CH::kFB;
    constexpr uint32_t kStage = KV * 1024, P = kStage / FB;
    // LDS: the loader's ring | two words the waves meet at | TWO images of a mixed chunk, [64 bytes: the 4 frames in front | the chunk | 64 bytes].
    // Two images and counters instead of barriers: the loader may be two classes ahead of wave 1 -- a tile's wave 1 waits for its NEIGHBOURS'
    // loaders (the frames in front of its chunk, their aggregates), and with one image and a barrier a class every loader was tied to within
    // a class of the slowest loader near it: measured 0.361 ms against 0.308 for the loaders alone.
    constexpr uint32_t kCtl = NS * kStage;
    constexpr uint32_t kImg = kStage + 128;
    constexpr uint32_t MB0 = kCtl + 64 + 64;         // the chunk of image 0 (its 4 frames in front at MB0 - H * FB)
    __shared__ __attribute__((aligned(1024))) unsigned char smem[kCtl + 64 + 2 * kImg];
    lds_u8 *const lds = (lds_u8 *)smem;
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;
    typedef __attribute__((address_space(4))) const uint64_t cu64;
    typedef __attribute__((address_space(4))) const float cf32;
    typedef __attribute__((address_space(4))) const uint32_t cu32;
    typedef const __attribute__((address_space(4))) unsigned char *cbytes;
    const cbytes kseg = (cbytes)__builtin_amdgcn_kernarg_segment_ptr();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t n_cls = m.n;
    const Params &p0 = m.e[0].p;  // the geometry the classes share
    const uint32_t tile = blockIdx.x;
    const uint32_t Ns = p0.eq_frames;
    auto entry = [&](uint32_t k) -> cbytes { return kseg + offsetof(ChunkMulti, e) + (size_t)k * sizeof(ChunkMulti::Entry); };
    // the two counters: classes handed over by the loader / finished by wave 1 (LDS words; a wave's LDS operations complete in order)
    auto ctl_read = [&](uint32_t which) -> uint32_t {
        uint32_t v;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(lds0 + kCtl + which * 4) : "memory");
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    };
    auto ctl_write = [&](uint32_t which, uint32_t v) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) *(RH_LDS uint32_t *)(lds + kCtl + which * 4) = v;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    if (wave == 0) {
        if (lane < 2) *(RH_LDS uint32_t *)(lds + kCtl + lane * 4) = 0u;
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (wave == 0) {
        // ---- the loader: the sum of chunk `tile` over every class's sources, class after class (k_rlm_chunk's source loop) ----
        const uint32_t nvec = Ns * C / 4;
        const uint32_t v0 = tile * (KV * 64);
        uint32_t goff[KV];
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            uint32_t j = v0 + (uint32_t)k * 64 + lane;
            j = j < nvec ? j : nvec - 1;
            goff[k] = j * 16;
        }
        const bool lin = v0 + (uint32_t)(KV * 64) <= nvec;
        auto stage_source = [&](cu64 *desc, uint32_t s_, uint32_t stage) {
            const void *data = (const void *)(uintptr_t)desc[4 * (uint64_t)s_];
            if (lin) {
                glds16_run<KV>(data, goff[0], lds0 + stage * kStage);
            } else {
#pragma unroll
                for (int k = 0; k < KV; ++k) glds16(data, goff[k], lds0 + stage * kStage + k * 1024);
            }
        };
        constexpr int NHV = H * FB / 16;
        // The ring does not know about classes: the source after next goes out as soon as a stage is free, across a class's end too (its last
        // two sources are summed while the next class's first two are on their way) -- only the hand-over of the mixed chunk happens per class.
        __builtin_amdgcn_s_setprio(3);  // (this wave's few instructions are the memory side's pace: in front of wave 1's arithmetic on the same SIMD)
        uint32_t kc = 0, sc = 0;        // the next source to request: source sc of class kc
        cu64 *ndesc = (cu64 *)(uintptr_t)RH_PARG(uint64_t, entry(0), srcs);
        uint32_t nS = RH_PARG(uint32_t, entry(0), n_sources);
        uint32_t nstage = 0;
        auto request_next = [&]() {  // (classes without sources are the host's to leave out)
            if (kc >= n_cls) return false;
            stage_source(ndesc, sc, nstage);
            nstage ^= 1u;
            if (++sc == nS) {
                sc = 0;
                if (++kc < n_cls) {
                    ndesc = (cu64 *)(uintptr_t)RH_PARG(uint64_t, entry(kc), srcs);
                    nS = RH_PARG(uint32_t, entry(kc), n_sources);
                }
            }
            return true;
        };
        uint32_t ahead = 0;  // groups of KV fetches in flight
        if (request_next()) ++ahead;
        if (request_next()) ++ahead;
        uint32_t st = 0;
        for (uint32_t k = 0; k < n_cls; ++k) {
            const cbytes e = entry(k);
            cf32 *const dgain = (cf32 *)(uintptr_t)RH_PARG(uint64_t, e, srcs);
            const uint32_t S = RH_PARG(uint32_t, e, n_sources);
            v4f acc[KV];
#pragma unroll
            for (int i = 0; i < KV; ++i) acc[i] = v4f{0.f, 0.f, 0.f, 0.f};
            float g_next = S ? dgain[4] : 0.f;
            for (uint32_t s_ = 0; s_ < S; ++s_) {
                const float g = g_next;
                g_next = s_ + 1 < S ? dgain[8 * (uint64_t)(s_ + 1) + 4] : 0.f;
                // this source has landed when at most the group behind it is outstanding (the few stores of a hand-over in between only make
                // the wait stricter)
                if (ahead > 1) wait_vm<KV>();
                else wait_vm<0>();
                --ahead;
                const lds_u8 *buf = lds + st * kStage;
                v4f v[KV];
#pragma unroll
                for (int i = 0; i < KV; ++i) v[i] = *(const lds_f4 *)(buf + i * 1024 + lane * 16);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the chunk is in registers: its stage is free ...
                if (request_next()) ++ahead;                        // ... for the source after next, of this class or the next one
#pragma unroll
                for (int i = 0; i < KV; ++i) {
                    acc[i].x = fma_(g, v[i].x, acc[i].x);
                    acc[i].y = fma_(g, v[i].y, acc[i].y);
                    acc[i].z = fma_(g, v[i].z, acc[i].z);
                    acc[i].w = fma_(g, v[i].w, acc[i].w);
                }
                st ^= 1u;
            }
            RH_CLS_STAMP(0)
            // the chunk's last 4 mixed frames to the tile behind (first: its wave 1 is waiting for them) ...
            if (lane >= 64 - NHV) {
                unsigned long long *hp = (unsigned long long *)(uintptr_t)RH_QARG(uint64_t, e, halo) + (uint64_t)tile * 8 + (uint32_t)(lane - (64 - NHV)) * 4;
                const uint32_t epoch = RH_PARG(uint32_t, e, epoch);
                const float ev[4] = {acc[KV - 1].x, acc[KV - 1].y, acc[KV - 1].z, acc[KV - 1].w};
#pragma unroll
                for (int w = 0; w < 4; ++w) __hip_atomic_store(hp + w, ((unsigned long long)epoch << 32) | __float_as_uint(ev[w]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // ... and the mixed chunk into the image wave 1 is not reading: it has finished class k - 2 (it may still be on class k - 1)
            if (k >= 2) {
                uint32_t spins = 0;
                while (ctl_read(1) + 2 <= k) {
                    if (++spins > kSpinLimit) break;  // (wave 1 reports what it waits for)
                    __builtin_amdgcn_s_sleep(8);
                }
            }
            {
                lds_u8 *img = lds + MB0 + (k & 1u) * kImg;
#pragma unroll
                for (int i = 0; i < KV; ++i) *(lds_f4 *)(img + (uint32_t)(i * 64 + lane) * 16) = acc[i];
                if (lane == 0) *(lds_f4 *)(img + kStage) = v4f{0.f, 0.f, 0.f, 0.f};
            }
            ctl_write(0, k + 1);
            RH_CLS_STAMP(1)
        }
        return;
    }
    // ---- wave 1: what k_rlm_chunk does behind its source loop, for every class in turn ----
    const ChunkArgs &q0 = m.e[0].q;
    const uint32_t m_lo = ((cu32 *)(uintptr_t)q0.m_lo)[tile], m_hi = ((cu32 *)(uintptr_t)q0.m_lo)[tile + 1];
    const uint32_t m0 = m_lo + (uint32_t)lane * R;
    const uint32_t n_t = m_hi - m_lo;  // <= 64 * R (host)
    const int nfl = (int)n_t - lane * R < 0 ? 0 : ((int)n_t - lane * R > R ? R : (int)n_t - lane * R);
    const uint32_t nl0 = (n_t + R - 1) / R;
    const uint32_t vlast = nl0 ? n_t - (nl0 - 1) * R : 0;  // frames of the last lane's run, 1 .. R
    const bool first = (m0 == 0);
    int offA[R + 2];
    float wgt[R + 2];
    {
        const int64_t fbase = (int64_t)tile * P;
        Cursor c = cursor_at(first ? 0 : m0 - 2, p0);
#pragma unroll
        for (int rr = 0; rr < R + 2; ++rr) {
            const bool dummy = first && rr < 2;
            uint64_t i;
            uint32_t num;
            cursor_resolve(c, p0, i, num);
            if (i + 1 >= Ns) {
                i = Ns - 1;
                num = 0;
            }
            int64_t f = (int64_t)i - fbase;
            f = f < -H ? -H : (f > (int64_t)P - 1 ? (int64_t)P - 1 : f);
            offA[rr] = dummy ? 0 : (int)f * (int)FB;  // (relative to the chunk in its image)
            wgt[rr] = dummy ? 0.0f : (float)num / p0.Tf;
            if (!dummy) cursor_next(c, p0);
        }
    }
    // The classes' mixes are ADDED here, in registers, in the classes' order (0.0 + class 0 + class 1 + ...: rh_mix_sum's order over the classes'
    // rows, bit for bit) and leave once, behind the last class -- when the loaders are done.  Measured with a row per class (tools/cls_stamps.py):
    // 36 MB of output stores interleaved with the 2 GiB of reads cost 40-55 us of a 310 us launch; written at the end, like k_rlm_chunk's, nothing.
    V ytot[R];
#pragma unroll
    for (int r = 0; r < R; ++r) ytot[r] = CH::zero();
    for (uint32_t k = 0; k < n_cls; ++k) {
        const cbytes e = entry(k);
        // the class's tables and addresses: fetched here, a class's loads away from their use
        const Tables *__restrict__ tb = (const Tables *)(uintptr_t)RH_PARG(uint64_t, e, tabs);
        const uint32_t J = RH_PARG(uint32_t, e, J), epoch = RH_PARG(uint32_t, e, epoch);
        const uint32_t Jc = J < tile ? J : tile;
        const bool want_look = (uint32_t)lane < Jc;
        unsigned long long *const halo = (unsigned long long *)(uintptr_t)RH_QARG(uint64_t, e, halo);
        unsigned long long *const gran = (unsigned long long *)(uintptr_t)RH_PARG(uint64_t, e, gran);
        uint32_t *const status = (uint32_t *)(uintptr_t)RH_PARG(uint64_t, e, status);
        const float U = ((const float *)(uintptr_t)RH_QARG(uint64_t, e, uni))[lane < 61 ? lane : 60];
        float lM[4], b15[4], b31[4], kM[4], pwv[4];
        {
            const float *kp = (const float *)(uintptr_t)RH_QARG(uint64_t, e, lookT) + ((uint64_t)tile * J + (want_look ? lane : 0)) * 4;
            const float *pw = (const float *)(uintptr_t)RH_QARG(uint64_t, e, powM) + 4 * vlast;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lM[i] = tb->laneM[lane][i];
                b15[i] = tb->bc15M[lane][i];
                b31[i] = tb->bc31M[lane][i];
                kM[i] = kp[i];
                pwv[i] = pw[i];
            }
        }
        lds_u8 *const img = lds + MB0 + (k & 1u) * kImg;  // the class's mixed chunk, when the loader says so
        {
            uint32_t spins = 0;
            while (ctl_read(0) <= k) {
                if (++spins > kSpinLimit) {
                    if (lane == 0) atomicOr(status, 1u);
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
            }
        }
#if defined(RH_CLS_DIAG) && RH_CLS_DIAG == 1  // diagnostics builds (wrong results): the loader's pace with nothing behind the hand-over
        CH::set(ytot[0], 0, CH::get(ytot[0], 0) + lM[0] + b15[0] + b31[0] + kM[0] + pwv[0] + U + (float)offA[0] + wgt[1] + (float)nfl + (want_look ? 1.f : 0.f) + (float)(uintptr_t)halo + (float)(uintptr_t)gran + (float)(uintptr_t)status + (float)epoch);
        ctl_write(1, k + 1);
        continue;
#endif
        RH_CLS_STAMP(2)
        // ---- the last 4 frames of the tile in front ----
        bool dead = false;
        if (tile == 0) {
            if (lane < H * C) *(RH_LDS float *)(img - H * FB + lane * 4) = 0.0f;
        } else {
            const bool want = lane < H * C;
            const unsigned long long *hp = halo + (uint64_t)(tile - 1) * 8 + (want ? lane : 0);
            unsigned long long hv = 0;
            bool ok = false;
            uint32_t spins = 0;
            while (true) {
                if (want && !ok) {
                    hv = __hip_atomic_load(hp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ok = (uint32_t)(hv >> 32) == epoch;
                }
                if (__all(ok || !want)) break;
                if (++spins > kSpinLimit) {
                    if (lane == 0) atomicOr(status, 1u);
                    dead = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (want) *(RH_LDS float *)(img - H * FB + lane * 4) = dead ? __builtin_nanf("") : __uint_as_float((uint32_t)hv);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        RH_CLS_STAMP(3)
        // ---- the lane's run of the mixed stream: lerp, zero-state biquad; the run-end state after nfl frames ----
        const float b0 = readlane_f(U, 0), c1 = readlane_f(U, 1), c2 = readlane_f(U, 2), na1 = -readlane_f(U, 3), na2 = -readlane_f(U, 4);
        V out[R];
        V E1 = CH::zero(), E2 = CH::zero();
        {
            V ta[R + 2], tb2[R + 2];
#pragma unroll
            for (int rr = 0; rr < R + 2; ++rr) {
                ta[rr] = CH::ld_lds(img + offA[rr]);
                tb2[rr] = CH::ld_lds(img + offA[rr] + FB);
            }
            auto tap = [&](int rr) -> V {
                V x;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) CH::set(x, ch, fma_(CH::get(tb2[rr], ch) - CH::get(ta[rr], ch), wgt[rr], CH::get(ta[rr], ch)));
                return x;
            };
            V x2 = first ? CH::zero() : tap(0);
            V x1 = first ? CH::zero() : tap(1);
            V w1 = CH::zero(), w2 = CH::zero();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const V x = tap(r + 2);
                V w;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const float wc = fma_(na1, CH::get(w1, ch), fma_(na2, CH::get(w2, ch), fma_(c2, CH::get(x2, ch), c1 * CH::get(x1, ch))));
                    CH::set(w, ch, wc);
                    CH::set(out[r], ch, fma_(b0, CH::get(x, ch), wc));
                }
                w2 = w1;
                w1 = w;
                x2 = x1;
                x1 = x;
                E1 = vsel(r + 1 == nfl, w1, E1);
                E2 = vsel(r + 1 == nfl, w2, E2);
            }
        }
        // ---- scan of the run-end states (scan basis) ----
        float Pq[2 * C];
#pragma unroll
        for (int i = 0; i < 2 * C; ++i) Pq[i] = 0.f;
        {
            const float Tm[4] = {readlane_f(U, 5), readlane_f(U, 6), readlane_f(U, 7), readlane_f(U, 8)};
#pragma unroll
            for (int ch = 0; ch < C; ++ch) mat_acc(Tm, CH::get(E1, ch), CH::get(E2, ch), Pq[2 * ch], Pq[2 * ch + 1]);
        }
        float own[2 * C];
#pragma unroll
        for (int i = 0; i < 2 * C; ++i) own[i] = Pq[i];
        // (scan_states, tile_aggregate and tile_store of rh_pipeline_dev.h, written out in this kernel: as calls they cost it registers and scalar spills --
        // profiles/refactor_scan_helpers.txt)
#define RH_CSCAN(K, N)                                                                             \
    {                                                                                              \
        float sq[2 * C];                                                                           \
        _Pragma("unroll") for (int i = 0; i < 2 * C; ++i) sq[i] = dpp0<kDppRowShr + N, 0xf>(Pq[i]); \
        const float sM[4] = {readlane_f(U, 9 + 4 * K), readlane_f(U, 10 + 4 * K), readlane_f(U, 11 + 4 * K), readlane_f(U, 12 + 4 * K)}; \
        _Pragma("unroll") for (int ch = 0; ch < C; ++ch) mat_acc(sM, sq[2 * ch], sq[2 * ch + 1], Pq[2 * ch], Pq[2 * ch + 1]); \
    }
        RH_CSCAN(0, 1)
        RH_CSCAN(1, 2)
        RH_CSCAN(2, 4)
        RH_CSCAN(3, 8)
#undef RH_CSCAN
        {
            float sq[2 * C];
#pragma unroll
            for (int i = 0; i < 2 * C; ++i) sq[i] = dpp0<kDppBcast15, 0xa>(Pq[i]);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) mat_acc(b15, sq[2 * ch], sq[2 * ch + 1], Pq[2 * ch], Pq[2 * ch + 1]);
        }
        {
            float sq[2 * C];
#pragma unroll
            for (int i = 0; i < 2 * C; ++i) sq[i] = dpp0<kDppBcast31, 0xc>(Pq[i]);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) mat_acc(b31, sq[2 * ch], sq[2 * ch + 1], Pq[2 * ch], Pq[2 * ch + 1]);
        }
        {  // the tile aggregate: the short last run on top of the inclusive prefix of the lane before it
            const int nl = (int)nl0;
            float A[2 * C];
#pragma unroll
            for (int i = 0; i < 2 * C; ++i) A[i] = 0.f;
            if (nl >= 1) {
#pragma unroll
                for (int i = 0; i < 2 * C; ++i) A[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(own[i]), nl - 1));
            }
            if (nl >= 2) {
                const float M[4] = {readfirstlane_f(pwv[0]), readfirstlane_f(pwv[1]), readfirstlane_f(pwv[2]), readfirstlane_f(pwv[3])};  // B^v
                float xp[2 * C];
#pragma unroll
                for (int i = 0; i < 2 * C; ++i) xp[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Pq[i]), nl - 2));
#pragma unroll
                for (int ch = 0; ch < C; ++ch) mat_acc(M, xp[2 * ch], xp[2 * ch + 1], A[2 * ch], A[2 * ch + 1]);
            }
            if (lane < 2 * C) {
                float ev = A[0];
#pragma unroll
                for (int i = 1; i < 2 * C; ++i) ev = lane == i ? A[i] : ev;
                __hip_atomic_store(gran + (uint64_t)tile * 4 + (uint32_t)lane, ((unsigned long long)epoch << 32) | __float_as_uint(ev), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        float Q[2 * C];
#pragma unroll
        for (int i = 0; i < 2 * C; ++i) Q[i] = dpp0<kDppWaveShr1, 0xf>(Pq[i]);
        // ---- the tile carry: lane j < J polls tile-1-j, weights it with B^(m_lo[tile] - m_lo[tile-j]) ----
        float c[2 * C];
#pragma unroll
        for (int i = 0; i < 2 * C; ++i) c[i] = 0.f;
        if (tile > 0) {
            const unsigned long long *gp = gran + (uint64_t)(tile - 1 - (want_look ? (uint32_t)lane : 0u)) * 4;
            unsigned long long gv[2 * C];
#pragma unroll
            for (int i = 0; i < 2 * C; ++i) gv[i] = 0;
            bool ok = false;
            uint32_t spins = 0;
            while (true) {
                if (want_look && !ok) {
                    bool all = true;
#pragma unroll
                    for (int i = 0; i < 2 * C; ++i) {
                        gv[i] = __hip_atomic_load(gp + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        all = all && ((uint32_t)(gv[i] >> 32) == epoch);
                    }
                    ok = all;
                }
                if (__all(ok || !want_look)) break;
                if (++spins > kSpinLimit) {
                    if (lane == 0) atomicOr(status, 1u);
                    dead = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(4);
            }
            if (lane == 0 && spins) atomicAdd(status + 1, spins);
            if (want_look && ok && !dead) {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) mat_acc(kM, __uint_as_float((uint32_t)gv[2 * ch]), __uint_as_float((uint32_t)gv[2 * ch + 1]), c[2 * ch], c[2 * ch + 1]);
            }
            half_wave_sum(c);  // sum over lanes 0..31 -> uniform
        }
        if (dead) {
#pragma unroll
            for (int i = 0; i < 2 * C; ++i) c[i] = __builtin_nanf("");
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) mat_acc(lM, c[2 * ch], c[2 * ch + 1], Q[2 * ch], Q[2 * ch + 1]);
        RH_CLS_STAMP(4)
        // the taps are in registers: the image is the loader's again
        ctl_write(1, k + 1);
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const float y = fma_(readlane_f(U, 25 + 2 * r), Q[2 * ch], fma_(readlane_f(U, 26 + 2 * r), Q[2 * ch + 1], CH::get(out[r], ch)));
                CH::set(ytot[r], ch, CH::get(ytot[r], ch) + y);
            }
        }
        RH_CLS_STAMP(5)
    }
    // ---- the sum leaves as whole lines through the ring (the loader has summed its last chunk: nothing is in flight into it) ----
    {
        constexpr uint32_t kRow = (R + 1) * FB;
        static_assert(64 * kRow <= kCtl + 64 + 2 * kImg, "the rows fit the LDS (the ring, and behind it the images: everything is free now)");
        lds_u8 *row = lds + (uint32_t)lane * kRow;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (C == 2) *(lds_f2 *)(row + r * FB) = v2f{CH::get(ytot[r], 0), CH::get(ytot[r], C - 1)};
            else *(RH_LDS float *)(row + r * FB) = CH::get(ytot[r], 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        float *ot = m.sum_out + ((uint64_t)m_lo + (uint32_t)lane) * C;  // this lane's frame of every group of 64
        for (uint32_t f0 = 0; f0 < n_t; f0 += 64) {
            const uint32_t f = f0 + (uint32_t)lane;
            if (f < n_t) {
                const lds_u8 *src2 = lds + (f / R) * kRow + (f % R) * FB;
                if (C == 2) {
                    const v2f a = *(const lds_f2 *)src2;
                    *reinterpret_cast<float2 *>(ot + (uint64_t)f0 * 2) = make_float2(a.x, a.y);
                } else {
                    ot[f0] = *(const RH_LDS float *)src2;
                }
            }
        }
    }
}
#undef RH_PARG
#undef RH_QARG

}  // namespace

namespace rhp {

// The instances of k_rlm_chunk, of its form for several classes in one launch and of the one that walks classes of one geometry itself
struct ChunkInst {
    uint32_t C;
    int R, KV;
    const void *one, *multi, *classes;  // (nullptr: no such instance)
    const void *pcm16 = nullptr;        // k_rlm_chunk_pcm16
};
#define RH_FN(k) reinterpret_cast<const void *>(&k)
static const ChunkInst kChunk[] = {
    {2, 9, 4, RH_FN((k_rlm_chunk<9, 2, 4>)), RH_FN((k_rlm_chunk_multi<9, 2, 4>)), nullptr},  // (RH_CHUNK_HALF, a tuning aid: PCM16 rows take the converted copy there)
    {2, 18, 8, RH_FN((k_rlm_chunk<18, 2, 8>)), RH_FN((k_rlm_chunk_multi<18, 2, 8>)), RH_FN((k_rlm_chunk_classes<18, 2, 8>)), RH_FN((k_rlm_chunk_pcm16<18, 2, 8>))},
    {2, 18, 4, RH_FN((k_rlm_chunk<18, 2, 4>)), RH_FN((k_rlm_chunk_multi<18, 2, 4>)), RH_FN((k_rlm_chunk_classes<18, 2, 4>)), RH_FN((k_rlm_chunk_pcm16<18, 2, 4>))},
    {1, 18, 4, RH_FN((k_rlm_chunk<18, 1, 4>)), RH_FN((k_rlm_chunk_multi<18, 1, 4>)), RH_FN((k_rlm_chunk_classes<18, 1, 4>)), RH_FN((k_rlm_chunk_pcm16<18, 1, 4>))},
    {1, 18, 2, RH_FN((k_rlm_chunk<18, 1, 2>)), RH_FN((k_rlm_chunk_multi<18, 1, 2>)), RH_FN((k_rlm_chunk_classes<18, 1, 2>)), RH_FN((k_rlm_chunk_pcm16<18, 1, 2>))},
};
#undef RH_FN
static const ChunkInst *chunk_inst(int R, uint32_t channels, int KV) {
    for (const ChunkInst &c : kChunk)
        if (c.C == channels && c.R == R && c.KV == KV) return &c;
    return nullptr;
}
const void *chunk_kernel(int R, uint32_t channels, int KV) {
    const ChunkInst *c = chunk_inst(R, channels, KV);
    return c ? c->one : nullptr;
}
const void *chunk_kernel_pcm16(int R, uint32_t channels, int KV) {
    const ChunkInst *c = chunk_inst(R, channels, KV);
    return c ? c->pcm16 : nullptr;
}

// The arguments of k_rlm_chunk for the batch that is set: the chunk plan's tables in place of the active plan's
static void chunk_params(const rh_rlm *p, Params &k, ChunkArgs &ca) {
    const ChunkPlan &c = p->chunk;
    k.tabs = c.d_tabs;
    k.gran = c.d_gran;
    k.n_tiles = c.n_tiles;
    k.J = c.J;
    k.u = c.uni;
    ca.m_lo = c.d_mlo;
    ca.halo = c.d_halo;
    ca.lookT = c.d_look;
    ca.powM = c.d_pow;
    ca.uni = c.d_uni;
    k.direct = (c.direct && p->exclusive) ? 1u : 0u;
}

rh_status chunk_launch_classes(rh_rlm *const *classes, float *const *rows, uint64_t row_capacity_frames, uint32_t n, float *dst_sum, rh_stream stream, bool *taken, bool *summed) {
    *taken = false;
    *summed = false;
    if (n < 2 || n > kChunkMultiMax || rh::knob(rh::K_CLASSES_ONE_BY_ONE)) return RH_OK;
    const ChunkInst *inst = nullptr;
    for (uint32_t k = 0; k < n; ++k) {  // every class a whole k_rlm_chunk run of one instance, or nothing is touched
        const rh_rlm *h = classes[k];
        if (!h || !h->cls.empty() || !h->plan || h->out_frames == 0 || row_capacity_frames < h->out_frames) return RH_OK;
        if (rh::rlm::route(route_in(h, *h->plan)) != rh::rlm::kChunk) return RH_OK;
        const ChunkInst *c = chunk_inst(h->chunk.R, h->cfg.channels, h->chunk.KV);
        if (!c || !c->multi || (inst && c->multi != inst->multi)) return RH_OK;
        inst = c;
    }
    RH_REQUIRE_INIT();
    for (uint32_t k = 0; k < n; ++k)
        if (!rows[k] || (reinterpret_cast<uintptr_t>(rows[k]) & 15u)) return RH_ERR_INVALID;
    hipStream_t s = rh::as_stream(stream);
    ChunkMulti m;
    memset(&m, 0, sizeof m);
    for (uint32_t k = 0; k < n; ++k) {  // this class's arguments behind the others', tiles by ticket
        rh_rlm *h = classes[k];
        rh_status w = pre_launch(h, s);
        if (w == RH_OK) w = next_epoch(h, s);
        if (w != RH_OK) return w;
        m.e[k].p = launch_params(h, *h->plan, 0, h->n_sources, rows[k], 0, 0, StreamArgs{});
        chunk_params(h, m.e[k].p, m.e[k].q);
        m.e[k].p.direct = 0;
        m.first[k + 1] = m.first[k] + rh::rlm::sharded_grid(h->chunk.n_tiles);
    }
    m.n = n;
    void *args[] = {&m};
    // Classes of ONE geometry (equal lengths, one rate pair, one chunk size: one table of tile bounds) whose tiles fit the chip at once: a
    // workgroup of two waves per tile walks the classes itself -- one wave loads, the other converts and filters (k_rlm_chunk_classes)
    const void *fn2 = rh::knob(rh::K_CLASSES_ONE_WAVE) ? nullptr : inst->classes;
    bool same = fn2 != nullptr;
    for (uint32_t k = 0; k < n && same; ++k) {
        const rh_rlm *h = classes[k], *h0 = classes[0];
        same = h->exclusive && h->eq_frames == h0->eq_frames && h->out_frames == h0->out_frames && h->F == h0->F && h->T == h0->T && h->chunk_in == h0->chunk_in &&
               h->chunk_out == h0->chunk_out && h->chunk.n_tiles == h0->chunk.n_tiles && h->chunk.R == h0->chunk.R && h->chunk.KV == h0->chunk.KV && h->n_sources >= 1;
    }
    if (same) {
        int per_cu = 0;
        same = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn2, 128, 0) == hipSuccess && per_cu >= 1 &&
               (uint64_t)classes[0]->chunk.n_tiles <= (uint64_t)per_cu * (uint64_t)rh::g_num_cus;
    }
    if (same) m.sum_out = dst_sum;  // (one workgroup per tile, all resident: no tickets)
    const hipError_t e = same ? hipLaunchKernel(fn2, dim3(classes[0]->chunk.n_tiles), dim3(128), args, 0, s) : hipLaunchKernel(inst->multi, dim3(m.first[n]), dim3(64), args, 0, s);
    if (e != hipSuccess) {
        rh::set_hip_error(e, "k_rlm_chunk_multi / k_rlm_chunk_classes launch");
        return RH_ERR_HIP;
    }
    *summed = same;
    for (uint32_t k = 0; k < n; ++k) {
        rh::rlm::booked(&classes[k]->tk, same, rh::rlm::kShards, m.first[k + 1] - m.first[k]);
        mark_launch(classes[k], s);
    }
    *taken = true;
    return RH_OK;
}

#if defined(RH_CLS_DIAG) && RH_CLS_DIAG == 9
extern "C" int rh_debug_cls_stamps(unsigned long long *dst, size_t n) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_cls_stamp), n * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif

// Mix first in one kernel: every tile sums its aligned chunk of every source, then converts and filters its part of the mix
rh_status launch_chunk(rh_rlm *p, Params &k, hipStream_t s, bool pcm16) {
    ChunkArgs ca;
    chunk_params(p, k, ca);
    if (pcm16) {  // the int16 rows themselves: their table, the instance that reads them, and its own residency
        k.srcs = p->d_pcm;
        k.direct = (p->chunk.direct_pcm && p->exclusive) ? 1u : 0u;
    }
    const uint32_t grid = k.direct ? k.n_tiles : rh::rlm::sharded_grid(k.n_tiles);  // by ticket: whole rounds of the eight counters (k_rlm_chunk)
    void *args[] = {&k, &ca};
    const hipError_t e = hipLaunchKernel(pcm16 ? p->chunk.fn_pcm : p->chunk.fn, dim3(grid), dim3(64), args, 0, s);
    if (e != hipSuccess) {
        rh::set_hip_error(e, "k_rlm_chunk launch");
        return RH_ERR_HIP;
    }
    rh::rlm::booked(&p->tk, k.direct != 0, rh::rlm::kShards, grid);
    return mark_launch(p, s);
}

}  // namespace rhp
