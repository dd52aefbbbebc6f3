// rh_pipeline_wave.hip -- the ragged unit.  k_rlm_wave, the general fused kernel: ragged batches and streams with a state per source
// (per-source scan and per-(source, tile) carries, exchanged in groups of 8 sources; the decomposition it shares with k_rlm_fast is described
// at the head of rh_pipeline.hip), and the ragged instances of rh_rlm_fast.h: k_rlm_fast<RAG> (the first half of a ragged filtered batch) with
// k_rlm_resid (the pairs as a launch of their own), stereo and mono.
//
// Why the two share a unit: wait_groups<KV, NS> (rh_pipeline_dev.h) is always inlined, but the compiler first works out, per unit, what all
// of its callers pass, and simplifies it with that.  k_rlm_wave passes a population count, k_rlm_fast<RAG, SUMF> a difference of two counters
// (anything); with both callers in one unit wait_groups<KV, 2> is compiled for any argument, and k_rlm_wave<.., 2, ..> gets the code it has
// always had.  In a unit of its own, 52 of its 60 instances come out two instructions longer or shorter
// (profiles/refactor_pipeline_units.txt).  A cut of this unit has to keep every k_rlm_wave<R, KV, 2> beside a k_rlm_fast<.., RAG, .., SUMF>
// of the same KV.
#include "rh_rlm_fast.h"

namespace {

// (C = 1: the frames are mono; the per-source aggregates keep their 4-word slots, the second channel's words travel as zeros)
template <int R, int KV, int NS, bool FILT, int C = 2>
__global__ __launch_bounds__(64, (R <= 8 && KV <= 5 ? 3 : 2)) void k_rlm_wave(const Params p) {  // (no spills: tests/test_code_objects.py)
    typedef Chan<C> CH;
    typedef typename CH::V V;
    constexpr uint32_t FB = CH::kFB, VF = CH::kVF;
    static_assert(R <= kMaxR, "frames per lane");
    static_assert(NS >= 2 && NS <= 4, "ring depth");
    static_assert(KV * (NS - 1) < 64, "vmcnt range");
    constexpr uint32_t kStage = KV * 1024;        // bytes of one LDS input stage
    constexpr uint32_t kPubBase = NS * kStage;    // 8 x 16 B: this tile's aggregates of the current source group
    constexpr uint32_t kCntBase = kPubBase + 128;              // 32 B: per recent source, how many predecessor tiles hold its own aggregate
    constexpr uint32_t kLookBase = kCntBase + 32;              // kMaxLook x 16 B: B^(L*j)
    constexpr uint32_t kGranBase = kLookBase + kMaxLook * 16;  // NI x 1 KiB: predecessor aggregates of one source group
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // explicit LDS address space: a generic pointer here turns every tap into a flat_load
    lds_u8 *const lds = (lds_u8 *)smem;
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;  // LDS byte address of the dynamic region

    const int lane = threadIdx.x;
    const uint32_t tile = __builtin_amdgcn_readfirstlane(lane == 0 ? atomicAdd(p.ticket, 1u) - p.ticket_base : 0u);
    constexpr uint32_t L = 64u * R;
    const uint32_t m_tile0 = tile * L;  // host: out_frames < 2^31
    const uint32_t m0 = m_tile0 + (uint32_t)lane * R;
    const uint64_t mg0 = p.st_mode ? p.st_m0 : 0;  // block streaming: this launch starts at global output frame st_m0 ...
    const uint64_t g0 = p.st_mode ? p.st_g0 : 0;   // ... and the buffers start at global input frame st_g0
    const uint64_t mfirst = p.st_mode ? p.st_mfirst : 0;
    const bool first = (mg0 + m0 == mfirst);  // stream start: x'[-1] = x'[-2] = 0
    const uint32_t Mout = (uint32_t)p.out_frames;
    const uint32_t col = tile + p.col0;  // this tile's column in the per-source aggregate rows
    const uint32_t ncol = p.gran_cols;

    // ---- input span of this tile (identical for every source) -------------------------------
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
        i_base = __builtin_amdgcn_readfirstlane((uint32_t)ib);  // host: in_frames < 2^29
        nvec = __builtin_amdgcn_readfirstlane(nv);
    }

    // per-lane byte offsets of the KV staging vectors inside a source (surplus lanes re-fetch the
    // last vector into unused slots); 8*frames < 2^32
    uint32_t goff[KV];
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        uint32_t j = lane + k * 64;
        j = j < nvec ? j : nvec - 1;
        goff[k] = (i_base + VF * j) * FB;
    }

    // ---- per-lane tap table: LDS byte offset of frame i(m) and the lerp weight ----------------
    // FILT: weight = num/T (the lerp becomes one FMA, <= 1.5 ulp from math.rs:25 -- far inside
    // the 1e-5 budget of the filtered pipeline); !FILT: weight = num, divided exactly per sample
    // so that resample+mix alone stays bit-identical to the reference.
    int offA[R + 2];
    float wgt[R + 2];
    {
        Cursor c = cursor_at(first ? mfirst : mg0 + m0 - 2, p);
#pragma unroll
        for (int rr = 0; rr < R + 2; ++rr) {
            const bool dummy = first && rr < 2;
            uint64_t i;
            uint32_t num;
            cursor_resolve(c, p, i, num);
            offA[rr] = dummy ? 0 : (int)(((uint32_t)(i - g0) - i_base) * FB);
            wgt[rr] = dummy ? 0.0f : (FILT ? (float)num / p.Tf : (float)num);
            if (!dummy) cursor_next(c, p);
        }
    }

    // ---- carry look-back geometry ----------------------------------------------------------------
    // Aggregates travel in groups of 8 sources.  One LDS-DMA instruction fetches, for the 8 sources
    // of a group, the aggregates of 4 predecessor tiles: lane = src*8 + pred*2 + half (16 B each);
    // NI = ceil(J/4) instructions cover all J predecessors.  Lane l < 32 then owns the 32-byte set
    // (src = l>>2, pred = l&3) of every instruction.
    const uint32_t Jc = p.J < col ? p.J : col;  // uniform: predecessors that exist (streaming: + the block-start state)
    const uint32_t NI = (Jc + 3) >> 2;
    const uint32_t gsrc = lane >> 3, gpred = (lane >> 1) & 3;
    const uint32_t gr_off0 = gsrc * ncol * 32u + (Jc - 1 - gpred) * 32u + (lane & 1) * 16u;  // instruction 0; -128 per further one
    const uint32_t set_src = lane >> 2, set_pred = lane & 3;  // lanes < 32

    const Tables *__restrict__ tb = p.tabs;
    float lM[4], b15[4], b31[4];
    if (FILT) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            lM[q] = tb->laneM[lane][q];
            b15[q] = tb->bc15M[lane][q];
            b31[q] = tb->bc31M[lane][q];
        }
        if (lane < kMaxLook) *(lds_f4 *)(lds + kLookBase + lane * 16) = v4f{tb->lookM[lane][0], tb->lookM[lane][1], tb->lookM[lane][2], tb->lookM[lane][3]};
    }
    const float b0 = p.u.b0, c1 = p.u.c1, c2 = p.u.c2, na1 = -p.u.a1, na2 = -p.u.a2;

    V acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = CH::zero();
    // The homogeneous corrections of all sources share g[] and laneM, so they are summed as STATES
    // and applied once after the last source: Qacc = sum of the lanes' zero-carry start states,
    // Cacc = this lane's share (its sets) of the summed tile carries.
    float Qacc[4] = {0.f, 0.f, 0.f, 0.f}, Cacc[4] = {0.f, 0.f, 0.f, 0.f};
    // A source that stays whole for this tile and the next J ("stable") never needs an aggregate of its own: every
    // tile that consumes it applies its correction merged.  Such sources only add their run-end state to a sum that
    // is scanned and published ONCE per tile (row n_sources of the table), as in k_rlm_fast; the per-source scan and
    // exchange below is left to the few sources that end within J tiles.  Streaming keeps every source on its own
    // (the block-end states are per source).
    const bool indiv_all = p.col0 != 0;
    const uint32_t m_stable = m_tile0 + (p.J + 1u) * L;
    V E1s = CH::zero(), E2s = CH::zero();
    uint64_t mrg = 0;      // bit k: source s-1-k was merged into Qacc
    uint32_t pubmask = 0;  // bit (s&7): source s of the current group has an aggregate in the pub area
    uint32_t grp_mask = 0; // merged flags (bit 7-src) of the group whose aggregates are in flight
    uint32_t grp_first = 0;
    uint32_t iss = 0;      // bit d: the stage of source s+d was filled by LDS-DMA (KV operations)
    bool dead = false;     // a bounded wait expired: never spin again in this wave

    const uint32_t S = p.n_sources;

    // ---- staging: source frames [i_base, i_base + 2*nvec) -> LDS stage, 16 bytes per lane -------
    // Always KV LDS-DMA instructions.  If the tile reaches past the end of the source, the lanes
    // beyond it re-fetch the source's last 16-byte vector instead (an aligned 16-byte load that
    // starts inside the source cannot leave its page): their slots then hold finite data that no
    // valid output reads, except as the second tap of the source's last frame, which
    // sample_rate.rs:193-200 emits verbatim -- the edge variant of the run selects the first tap there.
    auto stage_source = [&](const void *data, uint32_t frames, uint32_t stage_off) {
        if (i_base + VF * nvec <= frames) {
#pragma unroll
            for (int k = 0; k < KV; ++k) glds16(data, goff[k], lds0 + stage_off + k * 1024);
        } else {
            const uint32_t lastoff = ((frames - 1) & ~(VF - 1u)) * FB;
#pragma unroll
            for (int k = 0; k < KV; ++k) glds16(data, goff[k] < lastoff ? goff[k] : lastoff, lds0 + stage_off + k * 1024);
        }
    };
    // The descriptor table is constant for the launch: read it through the constant address space so
    // that it is an s_load (lgkmcnt), not a vector load whose wait would drain the DMA ring.
    typedef __attribute__((address_space(4))) const uint32_t cu32;
    cu32 *const desc = (cu32 *)(uintptr_t)p.srcs;
    struct Desc {
        const void *data;
        uint32_t frames, out_frames;
        float gain;
    };
    auto load_desc = [&](uint32_t s) -> Desc {
        Desc d{nullptr, 0, 0, 1.0f};
        if (s < S) {
            const uint64_t lo = desc[8 * (uint64_t)s], hi = desc[8 * (uint64_t)s + 1];
            d.data = (const void *)(uintptr_t)(lo | (hi << 32));
            d.frames = desc[8 * (uint64_t)s + 2];
            d.out_frames = desc[8 * (uint64_t)s + 3];
            d.gain = __uint_as_float(desc[8 * (uint64_t)s + 4]);
        }
        return d;
    };

    // Poll one 32-byte aggregate per lane until it carries this launch's epoch (ordinary agent-scope
    // loads: hipcc waits for them, which also drains the DMA ring -- this is the slow path).
    auto poll_sets = [&](const unsigned long long *gp, bool want, unsigned long long (&gv)[4], bool &ok) {
        uint32_t spins = 0;
        if (lane == 0) atomicAdd(p.status + 1, 1u);  // statistics: carries that were not ready in time
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
#ifdef RH_PHASE_PROFILE
            if (lane == 0) atomicAdd(p.status + 2, 1u);  // statistics: polls that found nothing yet
#endif
            if (++spins > kSpinLimit) {
                if (lane == 0) atomicOr(p.status, 1u);
                dead = true;
                break;
            }
            __builtin_amdgcn_s_sleep(8);
        }
    };

    // ---- prologue: sources 0..NS-2 into stages 0..NS-2 -------------------------------------------
    uint32_t Ms_ring[NS], Ns_ring[NS];  // [d]: out_frames / frames of source s+d
    float g_ring[NS];                  // ... and its Amplify factor
#pragma unroll
    for (int d = 0; d < NS; ++d) {
        Ms_ring[d] = Ns_ring[d] = 0;
        g_ring[d] = 1.0f;
    }
    uint32_t st_cur = 0;  // LDS byte offset of the stage of source s
#pragma unroll
    for (int d = 0; d < NS - 1; ++d) {
        const Desc sd = load_desc(d);
        Ms_ring[d] = sd.out_frames;
        Ns_ring[d] = sd.frames;
        g_ring[d] = sd.gain;
        if (sd.out_frames > m_tile0) {
            stage_source(sd.data, sd.frames, d * kStage);
            iss |= 1u << d;
        }
    }
    Desc sd_pref = load_desc(NS - 1);  // fetched one iteration ahead of its use

    const uint32_t g_last = S ? (S - 1) >> 3 : 0;
    const uint32_t n_iter = FILT ? (S ? 8 * (g_last + kGroupLag) + 3 : 0) : S;
    RH_PH_DECL

    for (uint32_t s = 0; s < n_iter; ++s) {
        // (1) every 8th source: fetch the predecessor tiles' aggregates of the source group that was
        //     completed 8*(kGroupLag-1)+1 sources ago (consumed 2 iterations from now)
        if (FILT && (s & 7) == 0 && s >= 8 * kGroupLag) {
            grp_first = s - 8 * kGroupLag;
            grp_mask = (uint32_t)(mrg >> (8 * kGroupLag - 8)) & 0xffu;  // bit 7-src
            if (Jc > 0 && grp_mask && !dead) {
                const unsigned long long *gb = p.gran + ((uint64_t)grp_first * ncol + (col - Jc)) * 4;
                const bool src_on = (grp_mask >> (7 - gsrc)) & 1u;
                for (uint32_t i = 0; i < NI; ++i)
                    if (src_on && gpred + 4 * i < Jc) glds16_sc1(gb, gr_off0 - 128u * i, lds0 + kGranBase + 1024u * i);
            }
        }
        RH_PH(0)
        // (2) stage source s+NS-1 into the slot source s-1 has just left
        {
            uint32_t st_new = st_cur + (NS - 1) * kStage;
            if (st_new >= NS * kStage) st_new -= NS * kStage;
            Ms_ring[NS - 1] = sd_pref.out_frames;
            Ns_ring[NS - 1] = sd_pref.frames;
            g_ring[NS - 1] = sd_pref.gain;
            if (s + NS - 1 < S && sd_pref.out_frames > m_tile0) {
                stage_source(sd_pref.data, sd_pref.frames, st_new);
                iss |= 1u << (NS - 1);
            }
            sd_pref = load_desc(s + NS);
        }
        RH_PH(1)
        // (3) everything older than the newest (groups issued after source s) has landed: the stage
        //     of source s, and any aggregate fetch issued 2 or more iterations ago
        wait_groups<KV, NS>(__builtin_popcount(iss >> 1));
        RH_PH(2)
        // (3b) all lerp taps of source s leave for the LDS now, so that their latency overlaps the carry step
        const uint32_t Ms = Ms_ring[0];
        const bool active = s < S && Ms > m_tile0;  // this tile still holds frames of source s
        V ta[R + 2], tb2[R + 2];
        if (active) {
            const lds_u8 *buf = lds + st_cur;
#pragma unroll
            for (int rr = 0; rr < R + 2; ++rr) {
                ta[rr] = CH::ld_lds(buf + offA[rr]);
                tb2[rr] = CH::ld_lds(buf + offA[rr] + FB);
            }
            asm volatile("" ::: "memory");  // keep the reads above the carry step
        }
        // (4) every 8th source: the group's tile carries join Cacc (lane l < 32: source l>>2, predecessor l&3 + 4i)
        if (FILT && (s & 7) == 2 && s >= 8 * kGroupLag && Jc > 0 && grp_mask) {
            const bool src_on = lane < 32 && ((grp_mask >> (7 - set_src)) & 1u);
            for (uint32_t i = 0; i < NI; ++i) {
                // only the predecessors in which the source already ran on its own hold an aggregate of it
                const uint32_t have = src_on ? *(const RH_LDS unsigned char *)(lds + kCntBase + ((grp_first + set_src) & 31u)) : 0u;
                const bool want = src_on && set_pred + 4 * i < have;
                unsigned long long gv[4] = {0, 0, 0, 0};
                bool ok = false;
                if (want && !dead) {
                    const lds_u8 *gsl = lds + kGranBase + 1024u * i + lane * 32;
                    const v2u64 lo = *(const lds_u64x2 *)gsl, hi = *(const lds_u64x2 *)(gsl + 16);
                    gv[0] = lo.x; gv[1] = lo.y; gv[2] = hi.x; gv[3] = hi.y;
                    ok = true;
#pragma unroll
                    for (int q = 0; q < 4; ++q) ok = ok && ((uint32_t)(gv[q] >> 32) == p.epoch);
                }
#ifndef RH_DIAG_NO_CARRY_WAIT  // diagnostic build: free-running tiles (wrong results), to price the lock-step
                if (!dead && !__all(ok || !want)) {  // a neighbour is more than 8*(kGroupLag-1) sources behind
                    const unsigned long long *gp = p.gran + ((uint64_t)(grp_first + (want ? set_src : 0)) * ncol + (col - 1 - (want ? set_pred + 4 * i : 0))) * 4;
                    poll_sets(gp, want, gv, ok);
                }
#endif
                if (want && ok && !dead) {
                    const v4f k4 = *(const lds_f4 *)(lds + kLookBase + (set_pred + 4 * i) * 16);
                    const float kM[4] = {k4.x, k4.y, k4.z, k4.w};
                    mat_acc(kM, __uint_as_float((uint32_t)gv[0]), __uint_as_float((uint32_t)gv[1]), Cacc[0], Cacc[1]);
                    mat_acc(kM, __uint_as_float((uint32_t)gv[2]), __uint_as_float((uint32_t)gv[3]), Cacc[2], Cacc[3]);
                }
            }
        }
        RH_PH(3)

        // (5) source s: lerp, zero-state biquad run, ordered mix
        // frames past the end of the mix are never stored, so a source that ends with the mix needs no masking
        const bool full = Ms >= m_tile0 + L || Ms >= Mout;
        uint64_t merged = 0;
        if (active) {
            const uint32_t Ns = Ns_ring[0];
            const float g = g_ring[0];  // Amplify factor of source s: rides on the mix and on the run-end state
            // edge: some lane needs masking, or the staged span reaches past the source (verbatim last frame)
            const bool edge = !full || i_base + VF * nvec > Ns;
            const uint32_t dthr = Ns - 1 - i_base;  // active => i_base <= Ns-1
            const int thr = (int)((dthr < (1u << 27) ? dthr : (1u << 27)) * FB);
            auto tap = [&](int rr, auto edge_tag) -> V {
                const V a = ta[rr], b = tb2[rr];
                V x;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float ac = CH::get(a, c), bc = CH::get(b, c);
                    float xc;
                    if (FILT) {
                        xc = fma_(bc - ac, wgt[rr], ac);
                    } else {  // amplify.rs:64 then math.rs:25: first + (second - first) * num / den, exactly
                        const float ag = ac * g, bg = bc * g;
                        xc = ag + div_T((bg - ag) * wgt[rr], p.Tf, p.rcpT);
                    }
                    if (decltype(edge_tag)::value) {  // the source's last frame is emitted verbatim
                        const bool last = offA[rr] >= thr;
                        xc = last ? (FILT ? ac : ac * g) : xc;
                    }
                    CH::set(x, c, xc);
                }
                return x;
            };
            // lanes past the end of the source contribute nothing (the reference's iterator ended)
            const int nvalid = Ms >= m0 + R ? R : (Ms > m0 ? (int)(Ms - m0) : 0);
            if (FILT) {
                V w1 = CH::zero(), w2 = CH::zero();
                auto run = [&](auto masked) {
                    V x2 = first ? CH::zero() : tap(0, masked);
                    V x1 = first ? CH::zero() : tap(1, masked);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const V x = tap(r + 2, masked);
                        V w;  // zero-state step of the recursive part; the w1 term goes last (shortest chain)
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const float wc = fma_(na1, CH::get(w1, c), fma_(na2, CH::get(w2, c), fma_(c2, CH::get(x2, c), c1 * CH::get(x1, c))));
                            CH::set(w, c, wc);
                            float yc = fma_(b0, CH::get(x, c), wc);
                            if (decltype(masked)::value) yc = r < nvalid ? yc : 0.0f;
                            CH::set(acc[r], c, fma_(g, yc, CH::get(acc[r], c)));
                        }
                        w2 = w1;
                        w1 = w;
                        x2 = x1;
                        x1 = x;
                    }
                };
                if (!edge) run(std::false_type{});
                else run(std::true_type{});
                RH_PH(4)
                if (!indiv_all && Ms >= m_stable) {  // stable: joins the summed state, nothing else
                    E1s = vfma_s(g, w1, E1s);
                    E2s = vfma_s(g, w2, E2s);
                } else {
                {  // how many predecessor tiles saw this source as not stable (and published it on its own)
                    const uint32_t tM = Ms / L;
                    uint32_t have = indiv_all ? Jc : (tile + p.J > tM ? tile + p.J - tM : 0u);
                    have = have < Jc ? have : Jc;
                    if (lane == 0) *(RH_LDS unsigned char *)(lds + kCntBase + (s & 31u)) = (unsigned char)have;
                }
                // ---- run end state in the scan basis, then the wave64 inclusive scan ----
                float P[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < C; ++c) mat_acc(p.u.Tm, CH::get(w1, c) * g, CH::get(w2, c) * g, P[2 * c], P[2 * c + 1]);
                scan_states(P, ScanStepsArgs{p.u}, b15, b31);  // (the step matrices from the argument block)
                // the tile aggregate (lane 63's inclusive prefix) waits in LDS for the group's publication
                if (lane == 63) *(lds_f4 *)(lds + kPubBase + (s & 7) * 16) = v4f{P[0], P[1], P[2], P[3]};
                pubmask |= 1u << (s & 7);
                float Qnew[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) Qnew[q] = dpp0<kDppWaveShr1, 0xf>(P[q]);  // exclusive: lane 0 gets 0
                if (full) {
                    merged = 1;
#pragma unroll
                    for (int q = 0; q < 4; ++q) Qacc[q] += Qnew[q];
                } else {
                    // The source ends inside this tile while the mix goes on (at most one tile per
                    // source): its correction is masked per frame, so it cannot join the merged
                    // states.  Fetch its carry right now (lane j: predecessor j) and apply it exactly.
                    float c[4] = {0.f, 0.f, 0.f, 0.f};
                    if (Jc > 0) {
                        const bool want = (uint32_t)lane < Jc;
                        unsigned long long gv[4] = {0, 0, 0, 0};
                        bool ok = false;
                        poll_sets(p.gran + ((uint64_t)s * ncol + (col - 1 - (want ? lane : 0))) * 4, want, gv, ok);
                        if (want && ok && !dead) {
                            const v4f k4 = *(const lds_f4 *)(lds + kLookBase + lane * 16);
                            const float kM[4] = {k4.x, k4.y, k4.z, k4.w};
                            mat_acc(kM, __uint_as_float((uint32_t)gv[0]), __uint_as_float((uint32_t)gv[1]), c[0], c[1]);
                            mat_acc(kM, __uint_as_float((uint32_t)gv[2]), __uint_as_float((uint32_t)gv[3]), c[2], c[3]);
                        }
                        half_wave_sum(c);  // sum over lanes 0..31 -> uniform
                    }
                    mat_acc(lM, c[0], c[1], Qnew[0], Qnew[1]);
                    mat_acc(lM, c[2], c[3], Qnew[2], Qnew[3]);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const bool v = r < nvalid;
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const float h = fma_(p.u.g[r][0], Qnew[2 * c], p.u.g[r][1] * Qnew[2 * c + 1]);
                            CH::set(acc[r], c, CH::get(acc[r], c) + (v ? h : 0.0f));
                        }
                    }
                }
                }  // individual source
            } else {
                auto run = [&](auto masked) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        V x = tap(r + 2, masked);
                        if (decltype(masked)::value && !(r < nvalid)) continue;  // an ended source adds nothing, not even +0.0
                        acc[r] += x;
                    }
                };
                if (!edge) run(std::false_type{});
                else run(std::true_type{});
            }
        }
        // (6) the group is complete: publish this tile's aggregates, 8 sources x 4 granules in one store
        if (FILT && s < S && ((s & 7) == 7 || s == S - 1)) {
            if (lane < 32 && ((pubmask >> (lane >> 2)) & 1u)) {
                const float ev = *(const RH_LDS float *)(lds + kPubBase + lane * 4);
                const unsigned long long word = ((unsigned long long)p.epoch << 32) | __float_as_uint(ev);
                __hip_atomic_store(p.gran + ((uint64_t)((s & ~7u) + (lane >> 2)) * ncol + col) * 4 + (lane & 3), word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            pubmask = 0;
        }
        // rotate the rings
        mrg = (mrg << 1) | merged;
        iss >>= 1;
#pragma unroll
        for (int d = 0; d + 1 < NS; ++d) {
            Ms_ring[d] = Ms_ring[d + 1];
            Ns_ring[d] = Ns_ring[d + 1];
            g_ring[d] = g_ring[d + 1];
        }
        st_cur += kStage;
        if (st_cur >= NS * kStage) st_cur = 0;
        RH_PH(5)
    }
    wait_vm<0>();  // nothing of this wave may still be in flight towards its LDS
#ifdef RH_PHASE_PROFILE
    if (p.prof && lane == 0) {
        unsigned xcc, hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        ph_t[6] = ((unsigned long long)xcc << 32) | hwid;
        ph_t[7] = ph_start;
        for (int i = 0; i < 8; ++i) p.prof[(uint64_t)tile * 8 + i] = ph_t[i];
    }
#endif

    if (FILT && !indiv_all) {  // the stable sources' summed state: one scan, one published aggregate, one look-back
        float P[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < C; ++c) mat_acc(p.u.Tm, CH::get(E1s, c), CH::get(E2s, c), P[2 * c], P[2 * c + 1]);
        scan_states(P, ScanStepsArgs{p.u}, b15, b31);  // (the step matrices from the argument block)
        unsigned long long *const sum_row = p.gran + (uint64_t)S * ncol * 4;
        {
            const float e0 = readlane_f(P[0], 63), e1 = readlane_f(P[1], 63);
            const float e2 = readlane_f(P[2], 63), e3 = readlane_f(P[3], 63);
            if (lane < 4) {
                const float ev = lane == 0 ? e0 : lane == 1 ? e1 : lane == 2 ? e2 : e3;
                const unsigned long long word = ((unsigned long long)p.epoch << 32) | __float_as_uint(ev);
                __hip_atomic_store(sum_row + (uint64_t)col * 4 + lane, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) Qacc[q] += dpp0<kDppWaveShr1, 0xf>(P[q]);  // exclusive: lane 0 gets 0
        if (Jc > 0) {  // lane j < Jc: predecessor j's summed aggregate (they finish about now)
            const bool want = (uint32_t)lane < Jc;
            unsigned long long gv[4] = {0, 0, 0, 0};
            bool ok = false;
            poll_sets(sum_row + (uint64_t)(col - 1 - (want ? lane : 0)) * 4, want, gv, ok);
            if (want && ok && !dead) {
                const v4f k4 = *(const lds_f4 *)(lds + kLookBase + lane * 16);
                const float kM[4] = {k4.x, k4.y, k4.z, k4.w};
                mat_acc(kM, __uint_as_float((uint32_t)gv[0]), __uint_as_float((uint32_t)gv[1]), Cacc[0], Cacc[1]);
                mat_acc(kM, __uint_as_float((uint32_t)gv[2]), __uint_as_float((uint32_t)gv[3]), Cacc[2], Cacc[3]);
            }
        }
    }
    if (FILT) {  // the merged homogeneous response: start state = Qacc + B^(R*lane) * (summed tile carries)
        if (dead) Cacc[0] = Cacc[1] = Cacc[2] = Cacc[3] = __builtin_nanf("");  // a carry never arrived: poison the tile (the status word fails the call)
        half_wave_sum(Cacc);  // sum over lanes 0..31 -> uniform
        mat_acc(lM, Cacc[0], Cacc[1], Qacc[0], Qacc[1]);
        mat_acc(lM, Cacc[2], Cacc[3], Qacc[2], Qacc[3]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int c = 0; c < C; ++c) CH::set(acc[r], c, fma_(p.u.g[r][0], Qacc[2 * c], fma_(p.u.g[r][1], Qacc[2 * c + 1], CH::get(acc[r], c))));
        }
    }

    // ---- mixed output: R frames per lane -----------------------------------------------------
    float *o = p.out + (uint64_t)m0 * C;
    if (C == 1) {
        if (R % 4 == 0) {
#pragma unroll
            for (int r = 0; r + 3 < R; r += 4) {
                const uint32_t m = m0 + r;
                if (m + 3 < Mout) *reinterpret_cast<float4 *>(o + r) = make_float4(CH::get(acc[r], 0), CH::get(acc[r + 1], 0), CH::get(acc[r + 2], 0), CH::get(acc[r + 3], 0));
                else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (m + k < Mout) o[r + k] = CH::get(acc[r + k], 0);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (m0 + r < Mout) o[r] = CH::get(acc[r], 0);
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

// ------------------------------------------------------------------ the instances ----
#define RH_WAVE(r, kv, ns) Variant{r, kv, ns, &k_rlm_wave<r, kv, ns, true>, &k_rlm_wave<r, kv, ns, false>}
// The general kernel (ragged batches) is heavier; it ships in two tile sizes.
const Variant kWave[] = {
    RH_WAVE(6, 3, 2), RH_WAVE(6, 4, 2), RH_WAVE(6, 7, 2), RH_WAVE(6, 14, 2), RH_WAVE(8, 4, 2), RH_WAVE(8, 4, 3), RH_WAVE(8, 5, 2), RH_WAVE(8, 9, 2),
    RH_WAVE(9, 5, 2), RH_WAVE(9, 5, 3), RH_WAVE(10, 5, 2), RH_WAVE(10, 5, 3), RH_WAVE(10, 6, 2), RH_WAVE(12, 6, 2), RH_WAVE(12, 6, 3), RH_WAVE(12, 7, 2),
};
#define RH_WAVE1(r, kv, ns) Variant{r, kv, ns, &k_rlm_wave<r, kv, ns, true, 1>, &k_rlm_wave<r, kv, ns, false, 1>}
const Variant kWave1[] = {
    RH_WAVE1(6, 2, 2), RH_WAVE1(6, 4, 2), RH_WAVE1(6, 7, 2), RH_WAVE1(8, 2, 2),  RH_WAVE1(8, 3, 2),  RH_WAVE1(8, 5, 2),  RH_WAVE1(8, 10, 2),
    RH_WAVE1(9, 3, 2), RH_WAVE1(9, 5, 2), RH_WAVE1(10, 3, 2), RH_WAVE1(10, 6, 2), RH_WAVE1(12, 3, 2), RH_WAVE1(12, 4, 2), RH_WAVE1(12, 7, 2),
};
#undef RH_WAVE1
#undef RH_WAVE
// k_rlm_fast<.., RAG>: the first half of a ragged filtered batch, in the tile sizes of the general kernel (both halves
// share the tile geometry, the tables and the aggregate rows)
#ifdef RH_RAG_NO_SUMF  // diagnostics builds: the per-source first half
#define RH_RAGN(r, kv, ns) Variant{r, kv, ns, &k_rlm_fast<r, kv, ns, true, true>, &k_rlm_resid<r, kv>}
#else
#define RH_RAGN(r, kv, ns) Variant{r, kv, ns, &k_rlm_fast<r, kv, ns, true, true, 2, true>, &k_rlm_resid<r, kv>}
#endif
#define RH_RAG(r, kv) RH_RAGN(r, kv, 2)
// (Rings of 3 and 4 stages for the long runs were built and measured in round 4: no change -- a heavy tile is not held back by what
// ONE wave keeps in flight, DESIGN.md 4.4 -- and dropped again: the overrides of rh_rlm_config address the fast plan, which has no
// such geometries.)
const Variant kRag[] = {
    RH_RAG(6, 3), RH_RAG(6, 4), RH_RAG(6, 7), RH_RAG(6, 14), RH_RAG(8, 4), RH_RAG(8, 5), RH_RAG(8, 9), RH_RAG(9, 5), RH_RAG(10, 5), RH_RAG(10, 6), RH_RAG(12, 6), RH_RAG(12, 7),
    RH_RAG(14, 7), RH_RAG(14, 8), RH_RAG(18, 9), RH_RAG(18, 10),
};
// ... and for mono sources (no launch of its own for the pairs: they run inside the kernel)
const Variant kRag1[] = {
#define RH_RAG1(r, kv) Variant{r, kv, 2, &k_rlm_fast<r, kv, 2, true, true, 1, true>, nullptr}
    RH_RAG1(6, 2), RH_RAG1(8, 2), RH_RAG1(8, 3), RH_RAG1(10, 3), RH_RAG1(12, 3), RH_RAG1(12, 4), RH_RAG1(16, 4), RH_RAG1(16, 5), RH_RAG1(18, 5),
#undef RH_RAG1
};
#undef RH_RAG
#undef RH_RAGN

}  // namespace

namespace rhp {
VariantTab tab_wave() { return tab_of(kWave); }
VariantTab tab_wave1() { return tab_of(kWave1); }
VariantTab tab_rag() { return tab_of(kRag); }
VariantTab tab_rag1() { return tab_of(kRag1); }
}  // namespace rhp
