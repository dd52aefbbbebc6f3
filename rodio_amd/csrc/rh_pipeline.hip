// rh_pipeline.hip -- the headline kernel (BASELINE config 2): for every source
//       mixer.add(UniformSourceIterator::new(src, 2, to_rate).low_pass(freq))
// followed by the ordered mixer sum, as ONE launch that reads each input byte once.
//
// Replaces, per output sample, the reference call stack of SURVEY.md 3.1:
//   MixerSource::next            src/mixer.rs:120-136, :185-198   (ordered f32 sum)
//   BltFilter::next              src/source/blt.rs:397-451, :558-560 (biquad, Direct Form I)
//   UniformSourceIterator::next  src/source/uniform.rs:78-97        (span chunking)
//   SampleRateConverter::next    src/conversions/sample_rate.rs:131-201, src/math.rs:23-26
//
// Two kernels share the decomposition (rh_rlm_fast.h and rh_pipeline_wave.hip):
//   k_rlm_fast  equal-length batches (the benchmark): everything that couples lanes and tiles is done
//               once on the SUM over the sources; tiles never wait for each other inside the source loop
//   k_rlm_wave  ragged batches: per-source scan and per-(source, tile) carries, exchanged in groups of 8
//
// Work decomposition (wave64, no MFMA -- there is no contraction here):
//   * one WAVE (= one 64-lane workgroup) owns a tile of L = 64*R consecutive OUTPUT frames for
//     ALL sources; a lane owns a run of R consecutive frames.  The wave walks the sources in
//     insertion order and keeps the mix accumulators (R stereo frames per lane) in registers,
//     so the mixer sum costs no memory traffic.  Single-wave workgroups need no barrier at all.
//   * the input frames of (source, tile) are contiguous in HBM.  They are fetched with
//     global_load_lds_dwordx4 (LDS-DMA, no VGPR round trip) into a ring of NS LDS stages and retired
//     with a counted s_waitcnt vmcnt; the lerp taps are ds_read2_b64, all issued before the
//     arithmetic.  HBM traffic = input once + mixed output once (+ one 128-byte line per chunk).
//     The DMA is issued from inline asm so that hipcc neither drains it at the next load
//     (cdna_hip_programming.md "Pipelining across barriers") nor counts it: every wait for it
//     is placed by hand below.
//   * the biquad is a linear recurrence along time.  Each lane runs it over its run from a zero
//     state; the run-end states are combined with a wave64 Kogge-Stone scan (DPP, no LDS) over
//     the 2x2 state-matrix powers B^(R*2^k) (host-computed in f64), and tiles are chained
//     through HBM "granules" ({epoch,value} 8-byte words, one agent-scope relaxed store each;
//     cdna_hip_programming.md G16 form R2).  A tile needs only the zero-state aggregates of its
//     J predecessors, where J is the number of tiles after which ||B^(L*J)|| < 2^-40 (the filter
//     is stable, so older history is below f32 resolution): no chained inclusive prefix, hence
//     no serial dependency along the tiles.  The homogeneous response g1[r]*S1 + g2[r]*S2 to the
//     true start state S of a lane is added once, after the last source, from summed states.
//   * tiles are numbered by an atomic ticket, so a tile only ever waits for tiles that already
//     hold a wave slot: progress does not depend on dispatch order or residency.
//
// The map of the path: one translation unit per kernel family, all over rh_pipeline_dev.h (the device helpers they share):
//   rh_rlm_fast.h            the text of k_rlm_fast, rag_find_pairs / rag_run_pairs and k_rlm_resid; instantiated by
//     rh_pipeline_fast_lo.hip  the stereo instances of k_rlm_fast with R <= 9, rh_pipeline_fast_hi.hip those with R >= 10,
//     rh_pipeline_fast1.hip    the mono ones,
//     rh_pipeline_wave.hip     k_rlm_fast<RAG> + k_rlm_resid: the ragged pair, stereo and mono
//   rh_pipeline_wave.hip     the ragged unit: k_rlm_wave and its instances, beside the ragged pair's (why they share a unit: see there)
//   rh_pipeline_chunk.hip    k_rlm_chunk / _multi / _classes (mix first in one kernel), their instances, launch_chunk, chunk_launch_classes
//   rh_pipeline_mix.hip      k_mix_rows / k_mix_ring (mix first as a pass of its own: launch_mixed), k_rlm_state / k_rlm_state_sum
//   rh_pipeline_sblk.hip     k_rlm_sblk: a block of a stream on the summed state in one launch
// This unit holds no kernel: it reaches the instances through the units' table getters (variant_tab) and launches what the route says
// (rlm_launch).  The host side around it -- handles, plans and tables, filter classes, the one-shot entry points (rh_pipeline_plan.hip) and
// block streaming (rh_pipeline_stream.hip) -- shares rh_pipeline_internal.h with all of them.
#include "rh_pipeline_internal.h"

namespace rhp {

// The stereo table of k_rlm_fast, put together from its two units on first use (a plan keeps pointers into it)
static VariantTab tab_fast() {
    static const std::vector<Variant> both = [] {
        const VariantTab lo = tab_fast_lo(), hi = tab_fast_hi();
        std::vector<Variant> v(lo.v, lo.v + lo.n);
        v.insert(v.end(), hi.v, hi.v + hi.n);
        return v;
    }();
    return VariantTab{both.data(), both.size()};
}

VariantTab variant_tab(TabKind kind, bool mono) {
    switch (kind) {
    case kTabFast: return mono ? tab_fast1() : tab_fast();
    case kTabWave: return mono ? tab_wave1() : tab_wave();
    default: return mono ? tab_rag1() : tab_rag();
    }
}

rh::rlm::RouteIn route_in(const rh_rlm *p, const Plan &pl) {
    rh::rlm::RouteIn in{};
    in.plan = &pl == &p->fast ? rh::rlm::kPlanFast : &pl == &p->pair ? rh::rlm::kPlanPair : rh::rlm::kPlanWave;
    in.filt = p->filt;
    in.mix_first_on = p->mix_first_on;
    in.pre_filter = p->pre_filter;
    in.chunk_ok = p->chunk.ok;
    in.no_mix_first = rh::knob(rh::K_NO_MIX_FIRST) != nullptr;
    in.count = in.n_sources = p->n_sources;
    return in;
}

void params_common(const rh_rlm *p, const StreamArgs &sa, Params &k) {
    k.ticket = p->d_ctl;
    k.status = p->d_ctl + 1;
    k.F = p->F;
    k.T = p->T;
    k.qF = p->F / p->T;
    k.rF = p->F % p->T;
    k.Tf = (float)p->T;
    k.rcpT = rh::lerp_rcp(p->T);  // 0: this T did not pass the exhaustive check of the short division (rh_common.h)
    k.epoch = p->epoch;
    k.st_mode = sa.mode;
    k.st_active = sa.active;
    k.st_m0 = sa.m0;
    k.st_g0 = sa.g0;
    k.st_mfirst = sa.mode ? p->st_mfirst : 0;
    k.st_win = sa.win;
    k.st_wout = sa.wout;
}

// The arguments of a launch of the active plan's kernel over sources [first, first + count)
Params launch_params(const rh_rlm *p, const Plan &pl, uint32_t first, uint32_t count, float *dst, uint32_t batch_streams, uint64_t out_stride, const StreamArgs &sa) {
    Params k;
    params_common(p, sa, k);
    k.srcs = p->d_srcs + first;
    k.tabs = pl.d_tabs;
    k.out = dst;
    k.gran = p->d_gran;
    k.out_frames = p->out_frames;
    k.chunk_in = sa.mode ? p->st_chunk_in : p->chunk_in;  // a stream knows its spans whatever the block size
    k.chunk_out = sa.mode ? p->st_chunk_out : p->chunk_out;
    k.n_sources = count;
    k.n_tiles = p->n_tiles;
    k.J = pl.J;
    k.ticket_base = p->tk.ticket_base;
    k.direct = 0;
    k.rag_merge = k.rag_pairs_from = k.rag_pairs_to = 0;
    k.prof = p->d_prof;
    k.eq_frames = p->eq_frames;
    k.batch_streams = batch_streams;
    k.shards = rh::rlm::batch_shards(batch_streams, rh::knob(rh::K_NO_TICKET_SHARDS) != nullptr);
    k.shard_base = p->tk.shard_base;
    k.out_stride = out_stride;
    k.gran_cols = sa.gran_cols ? sa.gran_cols : p->n_tiles;
    k.col0 = sa.gran_cols ? 1u : 0u;
    k.u = pl.uni;
    return k;
}

// The ragged pair.  First half: the stable pairs, summed aggregates into the row behind the `count` per-source rows; second half: the few
// pairs in which a source is about to end, on top of the first (k_rlm_resid) -- or inside the first kernel (Params::rag_merge; mono: always)
static rh_status launch_pair(rh_rlm *p, const Plan &pl, Params &k, uint32_t grid, hipStream_t s) {
    Params k1 = k;
    k1.gran = p->d_gran + (uint64_t)k.n_sources * p->n_tiles * 4;
    k1.eq_frames = p->rag_frames;  // the sources that last as long as the mix (one length): the end-of-source handling is theirs
    void *args[] = {&k}, *args1[] = {&k1};
#ifdef RH_RAG_NO_SUMF
    const bool merge = false;
#else
    const bool merge = !rh::knob(rh::K_RAG_TWO_KERNELS) || !pl.v->plain;
#endif
    k1.rag_merge = merge ? 1u : 0u;
    k1.rag_pairs_from = p->rag_pairs_from;
    k1.rag_pairs_to = p->rag_pairs_to;
    uint32_t lds1 = pl.lds_bytes + 128u;  // (the pair list behind the ring)
    if (const char *w = rh::knob(rh::K_RAG_RESIDENT)) {  // tuning aid: at most this many tiles of the first half on a CU at once
        const int want = atoi(w);
        if (want >= 2 && want < 8) lds1 = std::max(lds1, (kLdsGranules / (uint32_t)want) * kLdsGranule);
    }
    const uint32_t grid8 = rh::rlm::sharded_grid(grid);  // tiles by ticket from eight counters (k_rlm_fast)
    k1.shards = rh::rlm::kShards;
    hipError_t e1 = hipLaunchKernel(reinterpret_cast<const void *>(pl.v->filt), dim3(grid8), dim3(64), args1, lds1, s);
    if (e1 == hipSuccess) rh::rlm::booked(&p->tk, false, k1.shards, grid8);
    if (e1 == hipSuccess && !merge) {
        e1 = hipLaunchKernel(reinterpret_cast<const void *>(pl.v->plain), dim3(grid), dim3(64), args, 2u * (uint32_t)pl.v->KV * 1024u + 128u /* two stages + the pair list */, s);
        rh::rlm::booked(&p->tk, false, 1, grid);
    }
    if (e1 != hipSuccess) {
        rh::set_hip_error(e1, "ragged batch launch");
        return RH_ERR_HIP;
    }
    return mark_launch(p, s);
}

// The active plan's fused kernel, one workgroup per tile (batch mode: per tile and source)
static rh_status launch_plain(rh_rlm *p, const Plan &pl, Params &k, uint32_t grid, hipStream_t s) {
    void *args[] = {&k};
    // batch mode fills the chip many times over: no residency shaping, the bare LDS request (one source per tile: one stage of the ring,
    // reused by the output transpose)
    const uint32_t lds = k.batch_streams ? std::max((uint32_t)pl.v->KV * 1024u, 64u * ((uint32_t)pl.v->R * 8u + 8u)) : p->launch_lds;
    const hipError_t e = hipLaunchKernel(pl.kernel, dim3(grid), dim3(64), args, lds, s);
    if (e != hipSuccess) {
        rh::set_hip_error(e, "k_rlm launch");
        return RH_ERR_HIP;
    }
    rh::rlm::booked(&p->tk, k.direct != 0, k.shards, grid);
    return mark_launch(p, s);
}

rh_status rlm_launch(rh_rlm *p, uint32_t first, uint32_t count, float *dst, uint64_t out_capacity_frames, uint64_t *out_frames, rh_stream stream, uint32_t batch_streams, uint64_t out_stride,
                     const StreamArgs &sa) {
    RH_REQUIRE_INIT();
    if (!p) return RH_ERR_INVALID;
    if (!p->cls.empty()) return RH_ERR_UNSUPPORTED;  // per-source filters: whole one-shot runs only (rh_rlm_run)
    if (first > p->n_sources || count > p->n_sources - first) return RH_ERR_INVALID;
    if (out_frames) *out_frames = p->out_frames;
    if (p->out_frames == 0) return RH_OK;
    if (!dst || (reinterpret_cast<uintptr_t>(dst) & 15u)) return RH_ERR_INVALID;
    if (out_capacity_frames < p->out_frames) return RH_ERR_CAPACITY;
    hipStream_t s = rh::as_stream(stream);
    const Plan &pl = *p->plan;
    rh::rlm::RouteIn in = route_in(p, pl);
    in.first = first;
    in.count = count;
    in.batch_streams = batch_streams;
    in.st_mode = sa.mode;
    in.gran_cols = sa.gran_cols;
    const rh::rlm::Route r = rh::rlm::route(in);
    // Sources set as 16-bit PCM (one-shot runs: a stream's block brings its own f32 rows): the rows themselves where a kernel reads them
    // (rh_rlm_pcm16.h), the converted copy -- made once -- everywhere else
    bool pcm16 = false;
    if (!sa.mode) {
        if (p->pcm) {
            if (!p->pcm_current()) return RH_ERR_INVALID;  // a stream's blocks have run on the handle since: set the sources again
            const int ring = r == rh::rlm::kMixed ? mixed_row_cut(p, count, false, sa).ring : 0;
            pcm16 = rh::rlm::pcm16_native({r, ring, p->cfg.channels, p->eq_frames, p->pcm_bits, false, first != 0 || count != p->n_sources}) == rh::rlm::kPcmNative &&
                    (r != rh::rlm::kChunk || p->chunk.fn_pcm);
            if (!pcm16 && r != rh::rlm::kUnsupported) {
                const rh_status c = pcm_f32_ready(p, s);
                if (c != RH_OK) return c;
            }
        }
        p->last_native = pcm16 ? 1 : 0;
    }
    rh_status w = pre_launch(p, s);
    if (w == RH_OK) w = next_epoch(p, s);
    if (w != RH_OK) return w;
    Params k = launch_params(p, pl, first, count, dst, batch_streams, out_stride, sa);
    const uint64_t grid = (uint64_t)p->n_tiles * (batch_streams ? batch_streams : 1);
    if (grid > 0x7fffffffull) return RH_ERR_UNSUPPORTED;
    switch (r) {
    case rh::rlm::kPair: return launch_pair(p, pl, k, (uint32_t)grid, s);
    case rh::rlm::kChunk: return launch_chunk(p, k, s, pcm16);
    case rh::rlm::kUnsupported: return RH_ERR_UNSUPPORTED;  // filter_first: one-shot runs of equal-length batches (rodio_hip.h)
    case rh::rlm::kMixed:
    case rh::rlm::kMixedFiltered:
        w = launch_mixed(p, pl, k, r == rh::rlm::kMixedFiltered, sa, stream, pcm16);
        if (w != RH_OK) return w;
        break;
    default: break;
    }
    return launch_plain(p, pl, k, (uint32_t)grid, s);
}

}  // namespace rhp
