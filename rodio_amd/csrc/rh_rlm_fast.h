// rh_rlm_fast.h -- the text of k_rlm_fast (equal-length batches, and the first half of a ragged filtered batch: RAG / SUMF), of the ragged
// helpers it calls (rag_find_pairs, rag_run_pairs) and of k_rlm_resid, which runs the same helpers as a launch of its own.  Kernel text only,
// no tables: rh_pipeline_fast_lo.hip and rh_pipeline_fast_hi.hip (stereo, by R), rh_pipeline_fast1.hip (mono) and rh_pipeline_wave.hip (ragged: beside k_rlm_wave, see there) each
// instantiate their own instances from it, and no instance is instantiated twice.  The decomposition is described at the head of rh_pipeline.hip.
#pragma once
#include "rh_pipeline_dev.h"

namespace {

// =================================================================================================
// The (tile, source) pairs of a ragged filtered batch in which the source is NOT stable, i.e. ends inside the tile or within the J
// tiles after it.  There are at most J+2 such tiles per source, so this part is small however large the batch: a tile finds its
// pairs with a ballot over the descriptors (rag_find_pairs) and handles each one start to finish (rag_run_pairs) -- stage, lerp,
// zero-state run (masked past the end of the source), scan, publish the source's own aggregate, poll the predecessors that hold
// one, correct frame by frame -- adding onto the tile's mix of the stable sources.  Tile geometry, tables and aggregate rows are
// those of k_rlm_wave.  Two callers: k_rlm_fast<RAG, SUMF> itself, behind its own part of the tile (Params::rag_merge: the mix is
// still in registers, and the pairs fill in behind the stable sources of the lighter tiles); k_rlm_resid, a launch of its own
// behind a first half that has stored its tiles (RH_RAG_TWO_KERNELS, and the per-source first half of diagnostics builds).
// =================================================================================================
// The tile's pairs: their source indices, in source order, as a list in the LDS at `list_off` (the host keeps batches with more than
// 24 such sources in one tile on k_rlm_wave).  Returns how many.
constexpr uint32_t kMaxPairs = 32;
__device__ __forceinline__ uint32_t rag_find_pairs(const Params &p, const uint32_t m_tile0, const uint32_t m_stable, const int lane, lds_u8 *lds, const uint32_t list_off) {
    const uint32_t S = p.n_sources;
    const uint32_t *const dsrc = reinterpret_cast<const uint32_t *>(p.srcs);
    uint32_t n_pairs = 0;
    for (uint32_t b = 0; b < S; b += 64) {
        const uint32_t q = b + lane;
        const uint32_t ms = q < S ? dsrc[8 * (uint64_t)q + 3] : 0u;
        const bool mine = ms > m_tile0 && ms < m_stable;  // still here, not stable
        const unsigned long long mask = __ballot(mine);
        const uint32_t rank = n_pairs + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (mine && rank < kMaxPairs) *(RH_LDS uint32_t *)(lds + list_off + rank * 4u) = q;
        n_pairs += (uint32_t)__popcll(mask);
    }
    if (n_pairs > kMaxPairs && lane == 0) atomicOr(p.status, 1u);  // (never: the host counted them.  The status word fails the call)
    n_pairs = __builtin_amdgcn_readfirstlane(n_pairs < kMaxPairs ? n_pairs : kMaxPairs);
    if (n_pairs) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
    return n_pairs;
}
// The pairs one after the other, the span of the NEXT one already on its way (two stages of KV KiB at lds + 0 and lds + KV KiB): a
// pair costs a memory round trip to stage and another to poll, and nothing else of this tile could hide them.  `rows`: the
// per-source aggregate rows.  offA / wgt: taps and weights of the lane's R + 2 frames (the caller's: the tile geometry is shared).
template <int R, int KV, int C>
__device__ __forceinline__ void rag_run_pairs(const Params &p, unsigned long long *const rows, const uint32_t tile, const uint32_t n_pairs, const int lane, lds_u8 *lds, const uint32_t lds0,
                                              const uint32_t list_off, const uint32_t i_base, const uint32_t nvec, const uint32_t (&goff)[KV], const int (&offA)[R + 2], const float (&wgt)[R + 2],
                                              const float (&lM)[4], const float (&b15)[4], const float (&b31)[4], const float (&kM)[4], typename Chan<C>::V (&acc)[R]) {
    typedef Chan<C> CH;
    typedef typename CH::V V;
    constexpr uint32_t FB = CH::kFB, VF = CH::kVF;
    constexpr uint32_t L = 64u * R, kStage = KV * 1024;
    const uint32_t m_tile0 = tile * L, m0 = m_tile0 + (uint32_t)lane * R;
    const bool first = (m0 == 0);
    const uint32_t ncol = p.n_tiles;
    const uint32_t Jc = p.J < tile ? p.J : tile;
    typedef __attribute__((address_space(4))) const uint32_t cu32;
    cu32 *const desc = (cu32 *)(uintptr_t)p.srcs;
    const float b0 = p.u.b0, c1 = p.u.c1, c2 = p.u.c2, na1 = -p.u.a1, na2 = -p.u.a2;
    bool dead = false;
    auto stage_pair = [&](uint32_t s, uint32_t stage_off) {  // (lanes past the source's end re-fetch its last vector: finite data nothing valid reads)
        const uint64_t plo = desc[8 * (uint64_t)s], phi = desc[8 * (uint64_t)s + 1];
        const void *data = (const void *)(uintptr_t)(plo | (phi << 32));
        const uint32_t Ns = desc[8 * (uint64_t)s + 2];
        if (i_base + VF * nvec <= Ns) {
#pragma unroll
            for (int k = 0; k < KV; ++k) glds16(data, goff[k], lds0 + stage_off + k * 1024);
        } else {
            const uint32_t lastoff = ((Ns - 1) & ~(VF - 1u)) * FB;
#pragma unroll
            for (int k = 0; k < KV; ++k) glds16(data, goff[k] < lastoff ? goff[k] : lastoff, lds0 + stage_off + k * 1024);
        }
    };
    auto pair_at = [&](uint32_t i) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)*(const RH_LDS uint32_t *)(lds + list_off + i * 4u)); };
    stage_pair(pair_at(0), 0);
    for (uint32_t i = 0; i < n_pairs; ++i) {
        const uint32_t s = pair_at(i);
        const lds_u8 *const buf = lds + (i & 1u) * kStage;
        if (i + 1 < n_pairs) {
            stage_pair(pair_at(i + 1), ((i + 1) & 1u) * kStage);
            wait_vm<KV>();  // this pair's span has landed when only the next one's is outstanding
        } else {
            wait_vm<0>();
        }
        const uint32_t Ms = desc[8 * (uint64_t)s + 3];
        const uint32_t Ns = desc[8 * (uint64_t)s + 2];
        const float g = __uint_as_float(desc[8 * (uint64_t)s + 4]);
        const uint32_t dthr = Ns - 1 - i_base;  // Ms > m_tile0 => i_base <= Ns-1
        const int thr = (int)((dthr < (1u << 27) ? dthr : (1u << 27)) * FB);
        const int nvalid = Ms >= m0 + R ? R : (Ms > m0 ? (int)(Ms - m0) : 0);
        auto tap = [&](int rr) -> V {
            const V a = CH::ld_lds(buf + offA[rr]), b = CH::ld_lds(buf + offA[rr] + FB);
            const bool last = offA[rr] >= thr;  // the source's last frame is emitted verbatim (sample_rate.rs:193-200)
            V x;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const float ac = CH::get(a, ch), bc = CH::get(b, ch);
                const float l = fma_(bc - ac, wgt[rr], ac);
                CH::set(x, ch, last ? ac : l);
            }
            return x;
        };
        V x2 = first ? CH::zero() : tap(0);
        V x1 = first ? CH::zero() : tap(1);
        V w1 = CH::zero(), w2 = CH::zero();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const V x = tap(r + 2);
            V w;
            const bool v = r < nvalid;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const float wc = fma_(na1, CH::get(w1, ch), fma_(na2, CH::get(w2, ch), fma_(c2, CH::get(x2, ch), c1 * CH::get(x1, ch))));
                CH::set(w, ch, wc);
                const float y = v ? fma_(b0, CH::get(x, ch), wc) : 0.0f;
                CH::set(acc[r], ch, fma_(g, y, CH::get(acc[r], ch)));
            }
            w2 = w1;
            w1 = w;
            x2 = x1;
            x1 = x;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the stage is free for the pair after next
        float P[4] = {0.f, 0.f, 0.f, 0.f};  // (mono: the second channel's words stay zero and travel as zeros, as in k_rlm_wave)
        mat_acc(p.u.Tm, CH::get(w1, 0) * g, CH::get(w2, 0) * g, P[0], P[1]);
        if (C == 2) mat_acc(p.u.Tm, CH::get(w1, C - 1) * g, CH::get(w2, C - 1) * g, P[2], P[3]);
        scan_states(P, ScanStepsArgs{p.u}, b15, b31);  // (the step matrices from the argument block)
        unsigned long long *const row = rows + (uint64_t)s * ncol * 4;
        {  // this source's own aggregate for the tile (a later tile of it polls for it)
            const float e0 = readlane_f(P[0], 63), e1 = readlane_f(P[1], 63);
            const float e2 = readlane_f(P[2], 63), e3 = readlane_f(P[3], 63);
            if (lane < 4) {
                const float ev = lane == 0 ? e0 : lane == 1 ? e1 : lane == 2 ? e2 : e3;
                const unsigned long long word = ((unsigned long long)p.epoch << 32) | __float_as_uint(ev);
                __hip_atomic_store(row + (uint64_t)tile * 4 + lane, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        float Q[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) Q[q] = dpp0<kDppWaveShr1, 0xf>(P[q]);  // exclusive: lane 0 gets 0
        // predecessors in which the source was already on its own (in the others it was stable: its state came with the sums)
        const uint32_t tM = Ms / L;
        uint32_t have = tile + p.J > tM ? tile + p.J - tM : 0u;
        have = have < Jc ? have : Jc;
        float c[4] = {0.f, 0.f, 0.f, 0.f};
        if (have > 0) {
            const bool want = (uint32_t)lane < have;
            const unsigned long long *gp = row + (uint64_t)(tile - 1 - (want ? lane : 0)) * 4;
            unsigned long long gv[4] = {0, 0, 0, 0};
            bool ok = false;
            uint32_t spins = 0;
            while (!dead) {
                if (want && !ok) {
                    bool all = true;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        gv[q] = __hip_atomic_load(gp + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        all = all && ((uint32_t)(gv[q] >> 32) == p.epoch);
                    }
                    ok = all;
                }
                if (__all(ok || !want)) break;
                if (++spins > kSpinLimit) {
                    if (lane == 0) atomicOr(p.status, 1u);
                    dead = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
            }
            if (want && ok && !dead) {
                mat_acc(kM, __uint_as_float((uint32_t)gv[0]), __uint_as_float((uint32_t)gv[1]), c[0], c[1]);
                mat_acc(kM, __uint_as_float((uint32_t)gv[2]), __uint_as_float((uint32_t)gv[3]), c[2], c[3]);
            }
            if (dead) c[0] = c[1] = c[2] = c[3] = __builtin_nanf("");  // poison: see k_rlm_fast
            half_wave_sum(c);  // sum over lanes 0..31 -> uniform
        }
        mat_acc(lM, c[0], c[1], Q[0], Q[1]);
        mat_acc(lM, c[2], c[3], Q[2], Q[3]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool v = r < nvalid;
            const float hx = fma_(p.u.g[r][0], Q[0], p.u.g[r][1] * Q[1]), hy = fma_(p.u.g[r][0], Q[2], p.u.g[r][1] * Q[3]);
            CH::set(acc[r], 0, CH::get(acc[r], 0) + (v ? hx : 0.0f));
            if (C == 2) CH::set(acc[r], C - 1, CH::get(acc[r], C - 1) + (v ? hy : 0.0f));
        }
    }
}

// SUMF (with RAG): sum first -- the stable sources of a tile share the tile's span, taps and weights, so their spans are SUMMED as
// they land (one FMA per float) and the lerp, the zero-state filter and everything behind it run once, on the sum (§4.6).
template <int R, int KV, int NS, bool FILT, bool RAG = false, int C = 2, bool SUMF = false>
__global__ __launch_bounds__(64, (R <= 4 ? (KV <= 5 ? 5 : 4) : R <= 6 ? 3 : R <= 12 ? 2 : 1)) void k_rlm_fast(const Params p) {  // (no spills: tests/test_code_objects.py)
    typedef Chan<C> CH;
    typedef typename CH::V V;
    constexpr uint32_t FB = CH::kFB, VF = CH::kVF;
    static_assert(R <= kMaxR, "frames per lane");
    static_assert(NS >= 2 && NS <= 4, "ring depth");
    static_assert(KV * (NS - 1) < 64, "vmcnt range");
    constexpr uint32_t kStage = KV * 1024;  // bytes of one LDS input stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    lds_u8 *const lds = (lds_u8 *)smem;
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;

    const int lane = threadIdx.x;
    // batch mode (no mixer: every source keeps its own output row): tickets run tile-major over the
    // sources, so the predecessor tiles of a stream always hold earlier tickets.  One device-scope counter hands out ~85
    // tickets per microsecond (MI355X_MICROARCH.md "dequeue") -- 64 streams x 820 tiles would spend 0.6 ms on that alone --
    // so the streams are dealt over `shards` counters on separate cache lines, one per XCD (workgroup b runs on XCD b % 8):
    // a stream's tiles all come from one counter, which keeps the order that matters.
    uint32_t ticket, stream, tile;
    if (p.direct) {
        ticket = blockIdx.x;
        stream = 0;
        tile = ticket;
    } else if (p.shards > 1 && p.batch_streams == 0) {
        // one stream, tiles by ticket, eight counters (see k_rlm_chunk): workgroup b takes ticket k of counter b % 8 and works on tile
        // b % 8 + 8 k; the grid is whole rounds of eight, workgroups past the last tile leave
        const uint32_t x = blockIdx.x & 7u;
        const uint32_t k_ = __builtin_amdgcn_readfirstlane(lane == 0 ? atomicAdd(p.ticket + 32u * (1u + x), 1u) - p.shard_base : 0u);
        tile = x + 8u * k_;
        ticket = tile;
        stream = 0;
        if (tile >= p.n_tiles) return;
    } else if (p.shards > 1) {
        const uint32_t x = blockIdx.x % p.shards, per = p.batch_streams / p.shards;
        ticket = __builtin_amdgcn_readfirstlane(lane == 0 ? atomicAdd(p.ticket + 32u * (1u + x), 1u) - p.shard_base : 0u);
        stream = x + p.shards * (ticket % per);
        tile = ticket / per;
    } else {
        ticket = __builtin_amdgcn_readfirstlane(lane == 0 ? atomicAdd(p.ticket, 1u) - p.ticket_base : 0u);
        stream = p.batch_streams ? ticket % p.batch_streams : 0u;
        tile = p.batch_streams ? ticket / p.batch_streams : ticket;
    }
    ticket = __builtin_amdgcn_readfirstlane(ticket);  // wave-uniform by construction: say so (SGPRs, not VGPRs)
    stream = __builtin_amdgcn_readfirstlane(stream);
    tile = __builtin_amdgcn_readfirstlane(tile);
    constexpr uint32_t L = 64u * R;
    const uint32_t m_tile0 = tile * L;
    const uint32_t m0 = m_tile0 + (uint32_t)lane * R;
    const uint64_t mg0 = p.st_mode ? p.st_m0 : 0;  // block streaming: this launch starts at global output frame st_m0
    const uint64_t mfirst = p.st_mode ? p.st_mfirst : 0;
    const bool first = (mg0 + m0 == mfirst);  // stream start: x'[-1] = x'[-2] = 0
    const uint32_t Mout = (uint32_t)p.out_frames;
    const uint32_t Ns = p.eq_frames;  // every source has Ns frames (and Mout output frames)
    const uint64_t g0 = p.st_mode ? p.st_g0 : 0;  // ... and the buffers start at global input frame st_g0
    // mode 1: lanes at or past st_active belong to the next block (their input has not arrived yet)
    const bool lane_on = p.st_mode != 1 || m0 < p.st_active;
    const bool state_tile = p.st_mode == 1 && tile == p.st_active / L;  // holds the lane whose start state is the block's end state

    uint32_t i_base, nvec;
    {
        uint64_t ib, ie;
        uint32_t nn;
        cursor_resolve(cursor_at(mg0 + m_tile0 >= 2 ? mg0 + m_tile0 - 2 : 0, p), p, ib, nn);
        ib = ib > g0 ? ib - g0 : 0;  // index inside the buffers
        ib &= ~(uint64_t)(128u / FB - 1u);  // the staged span starts on a 128-byte line: every DMA instruction covers whole lines
        cursor_resolve(cursor_at(mg0 + m_tile0 + L - 1, p), p, ie, nn);
        ie = ie > g0 ? ie - g0 : 0;
        ie += 1;
        uint32_t nv = (uint32_t)((ie - ib + VF) / VF);
        if (nv > (uint32_t)(KV * 64)) nv = KV * 64;  // host sizes KV so this never bites
        i_base = __builtin_amdgcn_readfirstlane((uint32_t)ib);
        nvec = __builtin_amdgcn_readfirstlane(nv);
    }
    // The tile reaches past the end of the sources: lanes beyond it re-fetch the last 16-byte vector
    // (finite data no valid output reads), and the last frame's second tap is replaced by the first
    // (sample_rate.rs:193-200: the last frame is emitted verbatim).  Same for every source here.
    const bool edge = i_base + VF * nvec > Ns;
    const uint32_t lastoff = ((Ns - 1) & ~(VF - 1u)) * FB;
    uint32_t goff[KV];
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        uint32_t j = lane + k * 64;
        j = j < nvec ? j : nvec - 1;
        goff[k] = (i_base + VF * j) * FB;
        if (edge && goff[k] > lastoff) goff[k] = lastoff;
    }
    int offA[R + 2];
    float wgt[R + 2];
    const uint32_t dthr = Ns - 1 - i_base;
    const int thr = (int)((dthr < (1u << 27) ? dthr : (1u << 27)) * FB);  // LDS offset of the sources' last frame
    {
        Cursor c = cursor_at(first ? mfirst : mg0 + m0 - 2, p);
#pragma unroll
        for (int rr = 0; rr < R + 2; ++rr) {
            const bool dummy = first && rr < 2;
            uint64_t i;
            uint32_t num;
            cursor_resolve(c, p, i, num);
            offA[rr] = dummy ? 0 : (int)(((uint32_t)(i - g0) - i_base) * FB);
            if (edge && offA[rr] >= thr) num = 0;  // verbatim last frame (and frames past it, never stored)
            if (edge && offA[rr] > thr) offA[rr] = thr;
            wgt[rr] = dummy ? 0.0f : (FILT ? (float)num / p.Tf : (float)num);
            if (!dummy) cursor_next(c, p);
        }
    }
    const float b0 = p.u.b0, c1 = p.u.c1, c2 = p.u.c2, na1 = -p.u.a1, na2 = -p.u.a2;

    V acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = CH::zero();
    V E1 = CH::zero(), E2 = CH::zero();  // sum over the sources of the run-end states (w[-1], w[-2])

    const uint32_t S = p.batch_streams ? 1u : p.n_sources;
    typedef __attribute__((address_space(4))) const uint64_t cu64;
    cu64 *const desc = (cu64 *)(uintptr_t)(p.srcs + stream);  // 32-byte descriptors: the pointer is the first qword ...
    typedef __attribute__((address_space(4))) const float cf32;
    cf32 *const dgain = (cf32 *)(uintptr_t)(p.srcs + stream);  // ... the gain is float 4
    auto stage_source = [&](const void *data, uint32_t stage_off) {
#pragma unroll
        for (int k = 0; k < KV; ++k) glds16(data, goff[k], lds0 + stage_off + k * 1024);
    };
    const bool live = Mout > m_tile0 && Ns > 0;  // false only for the state tile of a block that ends on a tile boundary
    // The ring: NS stages, and -- because a source's taps are pulled into registers in one go -- NS
    // sources in flight: the stage of source s is re-targeted by the DMA of source s+NS as soon as the
    // taps of s have returned, BEFORE the arithmetic of s.
    uint32_t st_cur = 0;
    uint64_t ptr_pref = 0;
    float g_next = 1.0f;
    if (!RAG) {
#pragma unroll
        for (int d = 0; d < NS; ++d)
            if ((uint32_t)d < S && live) stage_source((const void *)(uintptr_t)desc[4 * d], d * kStage);
        ptr_pref = NS < S ? desc[4 * NS] : 0;  // fetched one iteration ahead of its use
        g_next = S ? dgain[4] : 1.0f;          // gain of source 0
    }
    RH_PH_DECL

    // Software pipeline over the sources: while source s is being computed, the taps of source s+1 are already on their
    // way from the LDS (two register sets, the loop body is written out twice so that they swap without moves).
    // Per iteration: taps(s) complete -> stage(s) is free -> DMA of source s+NS into it -> stage(s+1) landed ->
    // tap reads of s+1 issued -> arithmetic of s.
    auto read_taps = [&](uint32_t stage_off, V (&qa)[R + 2], V (&qb)[R + 2]) {
        const lds_u8 *buf = lds + stage_off;
#pragma unroll
        for (int rr = 0; rr < R + 2; ++rr) {
            qa[rr] = CH::ld_lds(buf + offA[rr]);
            qb[rr] = CH::ld_lds(buf + offA[rr] + FB);
        }
    };
    auto compute = [&](const V (&ta)[R + 2], const V (&tb2)[R + 2], const float g) {
        auto tap = [&](int rr) -> V {
            // the sources' last frame is emitted verbatim: its second tap lies behind the row (the rest of the row's last 16-byte vector, or
            // the re-fetched vector) and must not reach the arithmetic -- b = a gives a + (a - a) * 0 / T = a whatever lies there
            const V a = ta[rr], b = (edge && offA[rr] == thr) ? a : tb2[rr];
            V x;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float ac = CH::get(a, c), bc = CH::get(b, c);
                if (FILT) {
                    CH::set(x, c, fma_(bc - ac, wgt[rr], ac));
                } else {  // amplify.rs:64 then math.rs:25: first + (second - first) * num / den, exactly
                    const float ag = ac * g, bg = bc * g;
                    CH::set(x, c, ag + div_T((bg - ag) * wgt[rr], p.Tf, p.rcpT));
                }
            }
            return x;
        };
        if (FILT) {
            V x2 = first ? CH::zero() : tap(0);
            V x1 = first ? CH::zero() : tap(1);
            V w1 = CH::zero(), w2 = CH::zero();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const V x = tap(r + 2);
                V w;  // zero-state step of the recursive part; the w1 term goes last (shortest chain)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float wc = fma_(na1, CH::get(w1, c), fma_(na2, CH::get(w2, c), fma_(c2, CH::get(x2, c), c1 * CH::get(x1, c))));
                    CH::set(w, c, wc);
                    CH::set(acc[r], c, fma_(g, fma_(b0, CH::get(x, c), wc), CH::get(acc[r], c)));  // the source's gain rides on the mix (linear chain)
                }
                w2 = w1;
                w1 = w;
                x2 = x1;
                x1 = x;
            }
            E1 = vfma_s(g, w1, E1);
            E2 = vfma_s(g, w2, E2);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const V x = tap(r + 2);
                acc[r] += x;
            }
        }
    };
    auto iteration = [&](const uint32_t s, const V (&ca)[R + 2], const V (&cb)[R + 2], V (&na)[R + 2], V (&nb)[R + 2]) {
        // the taps of source s are in registers: its stage is free for source s+NS
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        RH_PH(2)
        if (s + NS < S) stage_source((const void *)(uintptr_t)ptr_pref, st_cur);
        ptr_pref = s + NS + 1 < S ? desc[4 * (uint64_t)(s + NS + 1)] : 0;
        const float g = g_next;  // Amplify factor of source s
        g_next = s + 1 < S ? dgain[8 * (uint64_t)(s + 1) + 4] : 1.0f;
        st_cur += kStage;
        if (st_cur >= NS * kStage) st_cur = 0;
        if (s + 1 < S) {  // the stage of source s+1 has landed when at most the groups issued after it are outstanding
            const uint32_t left = S - 2 - s;
            wait_groups<KV, NS>((int)(left < (uint32_t)(NS - 1) ? left : (uint32_t)(NS - 1)));
            read_taps(st_cur, na, nb);
        }
        RH_PH(1)
        compute(ca, cb, g);
        RH_PH(4)
    };
    V tA[R + 2], tB[R + 2], uA[R + 2], uB[R + 2];
    if (!RAG) {
        if (live && S) {
            const uint32_t left = S - 1;
            wait_groups<KV, NS>((int)(left < (uint32_t)(NS - 1) ? left : (uint32_t)(NS - 1)));
            read_taps(0, tA, tB);
        }
        for (uint32_t s = 0; s < S && live; s += 2) {
            iteration(s, tA, tB, uA, uB);
            if (s + 1 < S) iteration(s + 1, uA, uB, tA, tB);
        }
    } else if (live) {
        // The same pipeline over the SUBSEQUENCE of stable sources.  q[0] is the source being computed, q[1..NS-1] are
        // in flight, q[NS] is the next one to fetch (S: none left).  `issued` / `waited` count DMA groups.
        typedef __attribute__((address_space(4))) const uint32_t cu32;
        cu32 *const dwords = (cu32 *)(uintptr_t)p.srcs;
        // stable: whole for this tile and the J after it -- or until the mix itself ends (such sources share one length,
        // eq_frames: the host checks it; the end-of-source handling above is theirs)
        const uint32_t m_far = m_tile0 + (p.J + 1u) * L;
        const uint32_t m_stable = m_far < Mout ? m_far : Mout;
        auto next_stable = [&](uint32_t from) {
            uint32_t k = from;
            while (k < S && dwords[8 * (uint64_t)k + 3] < m_stable) ++k;
            return k;
        };
        // Inside a source (no tile edge, the span fills all but the last instruction) the DMA instructions of a stage lie 1 KiB apart
        // in memory as in the LDS: they go out as runs that share one M0 and one offset register (glds16_run) -- a tile in the middle
        // of the batch, i.e. nearly every one.
        constexpr int KF = KV - 1;
        const bool lin = SUMF && !edge && nvec >= (uint32_t)(KF * 64);
        auto stage_rag = [&](const void *data, uint32_t stage_off) {
            if (lin) {
                glds16_run<KF>(data, goff[0], lds0 + stage_off);
                glds16(data, goff[KV - 1], lds0 + stage_off + (KV - 1) * 1024);
            } else {
                stage_source(data, stage_off);
            }
        };
        uint32_t q[NS + 1];
        uint32_t issued = 0, waited = 0;
        {
            uint32_t nxt = next_stable(0);
#pragma unroll
            for (int d = 0; d < NS; ++d) {
                q[d] = nxt;
                if (nxt < S) {
                    stage_rag((const void *)(uintptr_t)desc[4 * (uint64_t)nxt], d * kStage);
                    ++issued;
                    nxt = next_stable(nxt + 1);
                }
            }
            q[NS] = nxt;
        }
        auto rag_iteration = [&](const V (&ca)[R + 2], const V (&cb)[R + 2], V (&na)[R + 2], V (&nb)[R + 2]) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the taps of q[0] are in registers: its stage is free
            if (q[NS] < S) {
                stage_source((const void *)(uintptr_t)desc[4 * (uint64_t)q[NS]], st_cur);
                ++issued;
            }
            const float g = dgain[8 * (uint64_t)q[0] + 4];
            st_cur += kStage;
            if (st_cur >= NS * kStage) st_cur = 0;
            if (q[1] < S) {  // the stage of q[1] has landed when only the groups issued after it are outstanding
                ++waited;
                wait_groups<KV, NS>((int)(issued - waited));
                read_taps(st_cur, na, nb);
            }
            compute(ca, cb, g);
#pragma unroll
            for (int d = 0; d < NS; ++d) q[d] = q[d + 1];
            q[NS] = q[NS] < S ? next_stable(q[NS] + 1) : S;
        };
        if constexpr (SUMF) {
            v4f accv[KV];
#pragma unroll
            for (int k = 0; k < KV; ++k) accv[k] = v4f{0.f, 0.f, 0.f, 0.f};
            // Descriptor words are scalar loads, and a scalar load that misses its cache is a round trip to L2 the wave sits out (the
            // phase profile of the first version: a third of a heavy tile's time between "the stage has landed" and "the next DMA is out").
            // So every word is asked for an iteration ahead of its use: the row of q[NS], the gain of q[1], the end of the source behind q[NS].
            uint64_t ptr_next = q[NS] < S ? desc[4 * (uint64_t)q[NS]] : 0;
            float g_cur = q[0] < S ? dgain[8 * (uint64_t)q[0] + 4] : 0.f;
            while (q[0] < S) {
                const uint32_t cand = q[NS] + 1;  // almost always stable too
                const uint32_t cand_end = cand < S ? dwords[8 * (uint64_t)cand + 3] : 0u;
                const float g_nxt = q[1] < S ? dgain[8 * (uint64_t)q[1] + 4] : 0.f;
                ++waited;
                wait_groups<KV, NS>((int)(issued - waited));  // the stage of q[0] has landed
                RH_PH(2)
                const lds_u8 *buf = lds + st_cur;
                v4f v[KV];
#pragma unroll
                for (int k = 0; k < KV; ++k) v[k] = *(const lds_f4 *)(buf + k * 1024 + lane * 16);
                const float g = g_cur;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the span is in registers: its stage is free
                if (q[NS] < S) {
                    stage_rag((const void *)(uintptr_t)ptr_next, st_cur);
                    ++issued;
                }
                RH_PH(1)
#pragma unroll
                for (int k = 0; k < KV; ++k) {
                    accv[k].x = fma_(g, v[k].x, accv[k].x);
                    accv[k].y = fma_(g, v[k].y, accv[k].y);
                    accv[k].z = fma_(g, v[k].z, accv[k].z);
                    accv[k].w = fma_(g, v[k].w, accv[k].w);
                }
                st_cur += kStage;
                if (st_cur >= NS * kStage) st_cur = 0;
#pragma unroll
                for (int d = 0; d < NS; ++d) q[d] = q[d + 1];
                q[NS] = cand >= S ? S : (cand_end >= m_stable ? cand : next_stable(cand + 1));
                ptr_next = q[NS] < S ? desc[4 * (uint64_t)q[NS]] : 0;
                g_cur = g_nxt;
                RH_PH(4)
            }
            wait_vm<0>();
            // the summed span takes the place of a source's in stage 0: one lerp, one zero-state run
#pragma unroll
            for (int k = 0; k < KV; ++k) *(lds_f4 *)(lds + k * 1024 + lane * 16) = accv[k];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            read_taps(0, tA, tB);
            compute(tA, tB, 1.0f);
        } else {
            if (q[0] < S) {
                ++waited;
                wait_groups<KV, NS>((int)(issued - waited));
                read_taps(0, tA, tB);
            }
            while (q[0] < S) {
                rag_iteration(tA, tB, uA, uB);
                if (q[0] < S) rag_iteration(uA, uB, tA, tB);
            }
        }
    }
    wait_vm<0>();  // nothing of this wave may still be in flight towards its LDS

    if (FILT && (live || state_tile)) {
        if (!lane_on) E1 = E2 = CH::zero();
        const Tables *__restrict__ tb = p.tabs;
        float lM[4], b15[4], b31[4], kM[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            lM[q] = tb->laneM[lane][q];
            b15[q] = tb->bc15M[lane][q];
            b31[q] = tb->bc31M[lane][q];
            kM[q] = tb->lookM[lane & (kMaxLook - 1)][q];
        }
        // ---- summed run-end states in the scan basis, then the wave64 inclusive scan (P[2c], P[2c+1]: channel c) ----
        float P[2 * C];
#pragma unroll
        for (int q = 0; q < 2 * C; ++q) P[q] = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) mat_acc(p.u.Tm, CH::get(E1, c), CH::get(E2, c), P[2 * c], P[2 * c + 1]);
        // (scan_states of rh_pipeline_dev.h, written out: as a call, 20 instances of this kernel compile to other code -- profiles/refactor_scan_helpers.txt)
#define RH_SCAN_STEP(K, N)                                                                          \
    {                                                                                               \
        float sq[2 * C];                                                                            \
        _Pragma("unroll") for (int q = 0; q < 2 * C; ++q) sq[q] = dpp0<kDppRowShr + N, 0xf>(P[q]);   \
        _Pragma("unroll") for (int c = 0; c < C; ++c) mat_acc(p.u.scanM[K], sq[2 * c], sq[2 * c + 1], P[2 * c], P[2 * c + 1]); \
    }
        RH_SCAN_STEP(0, 1)
        RH_SCAN_STEP(1, 2)
        RH_SCAN_STEP(2, 4)
        RH_SCAN_STEP(3, 8)
#undef RH_SCAN_STEP
        {  // rows 1 and 3 take the inclusive prefix of the row before them
            float sq[2 * C];
#pragma unroll
            for (int q = 0; q < 2 * C; ++q) sq[q] = dpp0<kDppBcast15, 0xa>(P[q]);
#pragma unroll
            for (int c = 0; c < C; ++c) mat_acc(b15, sq[2 * c], sq[2 * c + 1], P[2 * c], P[2 * c + 1]);
        }
        {  // rows 2 and 3 take the inclusive prefix of lanes 0..31
            float sq[2 * C];
#pragma unroll
            for (int q = 0; q < 2 * C; ++q) sq[q] = dpp0<kDppBcast31, 0xc>(P[q]);
#pragma unroll
            for (int c = 0; c < C; ++c) mat_acc(b31, sq[2 * c], sq[2 * c + 1], P[2 * c], P[2 * c + 1]);
        }
        {  // publish the tile aggregate (lane 63's inclusive prefix): 2C granules of the tile's 4-word slot, one store
            float e[2 * C];
#pragma unroll
            for (int q = 0; q < 2 * C; ++q) e[q] = readlane_f(P[q], 63);
            if (lane < 2 * C) {
                float ev = e[0];
#pragma unroll
                for (int q = 1; q < 2 * C; ++q) ev = lane == q ? e[q] : ev;
                const unsigned long long word = ((unsigned long long)p.epoch << 32) | __float_as_uint(ev);
                __hip_atomic_store(p.gran + ((uint64_t)stream * p.n_tiles + tile) * 4 + lane, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        float Q[2 * C];
#pragma unroll
        for (int q = 0; q < 2 * C; ++q) Q[q] = dpp0<kDppWaveShr1, 0xf>(P[q]);  // exclusive: lane 0 gets 0
        // ---- the tile carry: lane j < J polls predecessor tile-1-j (they finish about now) ----
        const uint32_t Jc = p.J < tile ? p.J : tile;
        float c[2 * C];
#pragma unroll
        for (int q = 0; q < 2 * C; ++q) c[q] = 0.f;
        if (Jc > 0) {
            const bool want = (uint32_t)lane < Jc;
            const unsigned long long *gp = p.gran + ((uint64_t)stream * p.n_tiles + (tile - 1 - (want ? lane : 0))) * 4;
            unsigned long long gv[2 * C];
#pragma unroll
            for (int q = 0; q < 2 * C; ++q) gv[q] = 0;
            bool ok = false, dead = false;
            uint32_t spins = 0;
            while (true) {
                if (want && !ok) {
                    bool all = true;
#pragma unroll
                    for (int q = 0; q < 2 * C; ++q) {
                        gv[q] = __hip_atomic_load(gp + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        all = all && ((uint32_t)(gv[q] >> 32) == p.epoch);
                    }
                    ok = all;
                }
                if (__all(ok || !want)) break;
                if (++spins > kSpinLimit) {
                    if (lane == 0) atomicOr(p.status, 1u);
                    dead = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
            }
            if (lane == 0 && spins) atomicAdd(p.status + 1, spins);  // statistics: polls that found nothing yet
            if (want && ok && !dead) {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) mat_acc(kM, __uint_as_float((uint32_t)gv[2 * ch]), __uint_as_float((uint32_t)gv[2 * ch + 1]), c[2 * ch], c[2 * ch + 1]);
            }
            // A carry that never arrived: the status word fails the call (rh_rlm_last_status), and the tile is poisoned so
            // that a block served without that check can never pass for audio.
            if (dead) {
#pragma unroll
                for (int q = 0; q < 2 * C; ++q) c[q] = __builtin_nanf("");
            }
            half_wave_sum(c);  // sum over lanes 0..31 -> uniform
        }
        if (p.st_mode && tile < p.J) {  // the stream's state at the block start still reaches this tile: + B^(L*tile) * W_in
            const float *M = tb->lookM[tile];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) mat_acc(M, p.st_win[2 * ch], p.st_win[2 * ch + 1], c[2 * ch], c[2 * ch + 1]);
        }
        // the merged homogeneous response: start state = Q + B^(R*lane) * carry
#pragma unroll
        for (int ch = 0; ch < C; ++ch) mat_acc(lM, c[2 * ch], c[2 * ch + 1], Q[2 * ch], Q[2 * ch + 1]);
        if (state_tile && (uint32_t)lane == (p.st_active % L) / R) {  // the first lane of the next block: its start state is the block's end state
#pragma unroll
            for (int q = 0; q < 2 * C; ++q) p.st_wout[q] = Q[q];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) CH::set(acc[r], ch, fma_(p.u.g[r][0], Q[2 * ch], fma_(p.u.g[r][1], Q[2 * ch + 1], CH::get(acc[r], ch))));
        }
        if constexpr (RAG && SUMF) {
            // The tile's own pairs in which a source is about to end, onto the mix in registers (the ring's first two stages and
            // 128 bytes behind the ring are theirs now).  Few tiles have any, and those are the lighter ones.
            const uint32_t m_far = m_tile0 + (p.J + 1u) * L;
            const uint32_t m_stable = m_far < Mout ? m_far : Mout;
            if (p.rag_merge && live && m_stable > p.rag_pairs_from && m_tile0 < p.rag_pairs_to) {
                RH_PH(5)
                const uint32_t n_pairs = rag_find_pairs(p, m_tile0, m_stable, lane, lds, NS * kStage);
                if (n_pairs)
                    rag_run_pairs<R, KV, C>(p, p.gran - (uint64_t)p.n_sources * p.n_tiles * 4, tile, n_pairs, lane, lds, lds0, NS * kStage, i_base, nvec, goff, offA, wgt, lM, b15, b31, kM, acc);
                RH_PH(3)
            }
        }
    }
#ifdef RH_PHASE_PROFILE
    RH_PH(5)
    if (p.prof && lane == 0) {
        unsigned xcc, hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        ph_t[6] = ((unsigned long long)xcc << 32) | hwid;
        ph_t[7] = ph_start;
        for (int i = 0; i < 8; ++i) p.prof[(uint64_t)ticket * 8 + i] = ph_t[i];
    }
#endif

    // ---- mixed output: R frames per lane -----------------------------------------------------
    float *o = p.out + (uint64_t)stream * p.out_stride + (uint64_t)m0 * C;
    if (C == 1) {  // mono: a lane's run is R floats; 16-byte stores where the run is whole vectors inside the mix (R % 4 == 0: m0 * 4 is 16-byte aligned)
        float *of = reinterpret_cast<float *>(o);
        if (R % 4 == 0) {
#pragma unroll
            for (int r = 0; r + 3 < R; r += 4) {
                const uint32_t m = m0 + r;
                if (m + 3 < Mout) *reinterpret_cast<float4 *>(of + r) = make_float4(CH::get(acc[r], 0), CH::get(acc[r + 1], 0), CH::get(acc[r + 2], 0), CH::get(acc[r + 3], 0));
                else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (m + k < Mout) of[r + k] = CH::get(acc[r + k], 0);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (m0 + r < Mout) of[r] = CH::get(acc[r], 0);
        }
        return;
    }
    if (R % 2 == 0 && !RAG && FILT && p.batch_streams) {
        // Batch mode writes as many bytes as it reads.  A lane's run is R*8 contiguous bytes, so a wave's float4 store hits
        // 64 different 128-byte lines with 16 bytes each: ten partial-line writes where one full line would do.  The runs
        // therefore go through the (now idle) LDS stage -- rows padded by 8 bytes -- and leave as whole lines: lane l stores
        // frames 2q, 2q+1 of the tile, q = k*64 + l.
        constexpr uint32_t kRow = R * 8 + 8;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        lds_u8 *row = lds + (uint32_t)lane * kRow;
#pragma unroll
        for (int r = 0; r < R; ++r) *(lds_f2 *)(row + r * 8) = v2f{CH::get(acc[r], 0), CH::get(acc[r], C - 1)};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        float *ot = p.out + (uint64_t)stream * p.out_stride + (uint64_t)m_tile0 * 2;
#pragma unroll
        for (int k = 0; k < R / 2; ++k) {
            const uint32_t f = 2u * (k * 64u + (uint32_t)lane);
            const lds_u8 *src2 = lds + (f / R) * kRow + (f % R) * 8u;
            const v2f a = *(const lds_f2 *)src2, b = *(const lds_f2 *)(src2 + 8);
            const uint32_t m = m_tile0 + f;
            if (m + 1 < Mout) *reinterpret_cast<float4 *>(ot + f * 2) = make_float4(a.x, a.y, b.x, b.y);
            else if (m < Mout) *reinterpret_cast<float2 *>(ot + f * 2) = make_float2(a.x, a.y);
        }
    } else if (R % 2 == 0) {
#pragma unroll
        for (int r = 0; r + 1 < R; r += 2) {
            const uint32_t m = m0 + r;
            if (m + 1 < Mout) {
                *reinterpret_cast<float4 *>(o + r * 2) = make_float4(CH::get(acc[r], 0), CH::get(acc[r], C - 1), CH::get(acc[r + 1], 0), CH::get(acc[r + 1], C - 1));
            } else if (m < Mout) {
                *reinterpret_cast<float2 *>(o + r * 2) = make_float2(CH::get(acc[r], 0), CH::get(acc[r], C - 1));
            }
        }
    } else {  // odd R: a lane's run starts on an 8-byte boundary only
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (m0 + r < Mout) *reinterpret_cast<float2 *>(o + r * 2) = make_float2(CH::get(acc[r], 0), CH::get(acc[r], C - 1));
    }
}

// k_rlm_resid -- the pairs as a launch of their own, on top of what a first half has stored.
template <int R, int KV>
__global__ __launch_bounds__(64) void k_rlm_resid(const Params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    lds_u8 *const lds = (lds_u8 *)smem;
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;
    const int lane = threadIdx.x;
    // tiles are numbered in arrival order, like everywhere else: a pair polls predecessor tiles, which then hold earlier tickets
    const uint32_t tile = __builtin_amdgcn_readfirstlane(lane == 0 ? atomicAdd(p.ticket, 1u) - p.ticket_base : 0u);
    constexpr uint32_t L = 64u * R;
    const uint32_t m_tile0 = tile * L;
    const uint32_t m0 = m_tile0 + (uint32_t)lane * R;
    const bool first = (m0 == 0);
    const uint32_t Mout = (uint32_t)p.out_frames;
    const uint32_t m_far = m_tile0 + (p.J + 1u) * L;
    const uint32_t m_stable = m_far < Mout ? m_far : Mout;  // sources that last as long as the mix are the first half's to the end
    constexpr uint32_t kList = 2 * KV * 1024;
    const uint32_t n_pairs = rag_find_pairs(p, m_tile0, m_stable, lane, lds, kList);
    if (!n_pairs) return;  // what k_rlm_fast<RAG> stored for this tile is final

    uint32_t i_base, nvec;
    {
        uint64_t ib, ie;
        uint32_t nn;
        cursor_resolve(cursor_at(m_tile0 >= 2 ? m_tile0 - 2 : 0, p), p, ib, nn);
        ib &= ~15ull;
        cursor_resolve(cursor_at((uint64_t)m_tile0 + L - 1, p), p, ie, nn);
        ie += 1;
        uint32_t nv = (uint32_t)((ie - ib + 2) / 2);
        if (nv > (uint32_t)(KV * 64)) nv = KV * 64;
        i_base = __builtin_amdgcn_readfirstlane((uint32_t)ib);
        nvec = __builtin_amdgcn_readfirstlane(nv);
    }
    uint32_t goff[KV];
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        uint32_t j = lane + k * 64;
        j = j < nvec ? j : nvec - 1;
        goff[k] = (i_base + 2u * j) * 8u;
    }
    int offA[R + 2];
    float wgt[R + 2];
    {
        Cursor c = cursor_at(first ? 0 : m0 - 2, p);
#pragma unroll
        for (int rr = 0; rr < R + 2; ++rr) {
            const bool dummy = first && rr < 2;
            uint64_t i;
            uint32_t num;
            cursor_resolve(c, p, i, num);
            offA[rr] = dummy ? 0 : (int)(((uint32_t)i - i_base) * 8u);
            wgt[rr] = dummy ? 0.0f : (float)num / p.Tf;
            if (!dummy) cursor_next(c, p);
        }
    }
    const Tables *__restrict__ tb = p.tabs;
    float lM[4], b15[4], b31[4], kM[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        lM[q] = tb->laneM[lane][q];
        b15[q] = tb->bc15M[lane][q];
        b31[q] = tb->bc31M[lane][q];
        kM[q] = tb->lookM[lane & (kMaxLook - 1)][q];
    }
    v2f acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        acc[r] = v2f{0.0f, 0.0f};
        if (m0 + r < Mout) {
            const float2 v = *reinterpret_cast<const float2 *>(p.out + (uint64_t)(m0 + r) * 2);
            acc[r] = v2f{v.x, v.y};
        }
    }
    rag_run_pairs<R, KV, 2>(p, p.gran, tile, n_pairs, lane, lds, lds0, kList, i_base, nvec, goff, offA, wgt, lM, b15, b31, kM, acc);
    float *o = p.out + (uint64_t)m0 * 2;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (m0 + r < Mout) *reinterpret_cast<float2 *>(o + r * 2) = make_float2(acc[r].x, acc[r].y);
}

}  // namespace
