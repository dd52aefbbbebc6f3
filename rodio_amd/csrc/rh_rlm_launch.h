// rh_rlm_launch.h -- the host-side decisions of the fused path (rh_pipeline*.hip) as plain functions over small structs of integers: which
// kernels a launch runs (route), how the mixed row of a summed-first launch is cut (row_cut), where the ticket counters stand behind a
// launch (Tickets, booked) and the geometry of a stream block in one kernel (sblk_geom).  No HIP and no handle: the callers fill the inputs
// from rh_rlm, and tests/cpp/rlm_launch_test.cpp runs all of it without a GPU.  The launches themselves are rlm_launch (rh_pipeline.hip) and
// sblk_try (rh_pipeline_sblk.hip).
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>

namespace rh {
namespace rlm {

constexpr int kUnset = INT_MIN;  // a tuning knob that is not set (one that is set travels as atoi of its text)

// ---- the route of a launch ---------------------------------------------------------------------------------------------------------
enum Route {
    kPair,           // ragged filtered one-shot batch: k_rlm_fast<RAG> [+ k_rlm_resid]
    kChunk,          // mix first in one kernel: k_rlm_chunk
    kMixed,          // k_mix_rows / k_mix_ring in front of a fused launch over the one mixed row
    kMixedFiltered,  // ... with the filter at from_rate on the mixed row in between (filter_first)
    kPlain,          // the active plan's fused kernel over the sources
    kBatch,          // ... one output row per source (no mixing)
    kUnsupported,    // filter_first outside one-shot runs of equal-length batches
    kRoutes
};
enum PlanKind { kPlanFast, kPlanWave, kPlanPair };
struct RouteIn {
    PlanKind plan;  // the active plan
    bool filt, mix_first_on, pre_filter, chunk_ok;
    bool no_mix_first;  // RH_NO_MIX_FIRST
    uint32_t first, count, n_sources, batch_streams;
    uint32_t st_mode, gran_cols;  // StreamArgs: a stream's block; != 0: a state per source
};
// Sum first: filtered equal-length batches, and blocks of a stream that carries ONE summed state (the state of the sum is the sum of the
// states) -- not where every source has a state of its own, and not in batch mode
inline bool sums_first(const RouteIn &in, bool per_source_states) {
    return in.plan == kPlanFast && in.filt && in.mix_first_on && !per_source_states && !in.batch_streams && in.count >= 2 && !in.no_mix_first;
}
inline Route route(const RouteIn &in) {
    if (in.plan == kPlanPair && !in.st_mode && !in.batch_streams) return kPair;
    if (in.chunk_ok && !in.st_mode && sums_first(in, false) && in.count == in.n_sources && in.first == 0) return kChunk;  // whole one-shot batches
    if (in.pre_filter) return (in.plan != kPlanFast || in.st_mode || in.batch_streams) ? kUnsupported : kMixedFiltered;
    if (sums_first(in, in.gran_cols != 0)) return kMixed;
    return in.batch_streams ? kBatch : kPlain;
}
// rh_rlm_geometry_info::mix_first of a whole one-shot run: 0 no, 1 k_mix_rows + fused, 2 k_rlm_chunk (a handle with pre_filter has no filt)
inline uint32_t mix_first_code(Route r) { return r == kChunk ? 2u : (r == kMixed || r == kMixedFiltered) ? 1u : 0u; }

// ---- the cut of the mixed row (k_mix_rows / k_mix_ring) ------------------------------------------------------------------------------
constexpr uint32_t kMixGroups = 16;
struct RowCutIn {
    uint64_t n_floats;  // eq_frames * channels
    uint32_t count, cus;
    bool pre;                // filter_first: a second row for the filtered mix
    bool stream;             // a block of a stream: the buffer is sized once, for its largest block ...
    uint64_t stream_floats;  // ... of max_in_frames * channels floats
    int knob_u, knob_groups;  // RH_MIX_U, RH_MIX_GROUPS (kUnset: not set)
};
struct RowCut {
    int U;          // vectors per lane of k_mix_rows (1 / 2, anything else: 4)
    uint32_t wgs;   // its workgroups along the row
    int ring;       // 0: k_mix_rows; 2 / >= 3: k_mix_ring of 2 / 3 stages
    uint64_t ring_waves;
    uint32_t groups;  // groups of sources side by side (partial rows, added in order by the fused launch)
    size_t row, rows_needed, need;  // floats per row; rows; floats of the whole buffer (rows, then the descriptors at its very end)
};
inline uint32_t vectors_per_wg(int U) { return 256u * (uint32_t)(U == 1 ? 1 : U == 2 ? 2 : 4); }
inline RowCut row_cut(const RowCutIn &in) {
    RowCut c;
    c.row = (size_t)(((in.stream ? in.stream_floats : in.n_floats) + 3) & ~3ull);
    const uint64_t nvec = in.n_floats / 4;
    c.U = 4;  // measured (256 x 1 Mi stereo frames): 0.410 / 0.409 / 0.342 ms for 1 / 2 / 4 vectors per lane
    // ... where the row fills the chip.  A stream's block is a short row (64 Ki frames: 128 workgroups at U = 4): fewer vectors per lane, more
    // workgroups, the same loads in flight per lane (8: the kernel takes 8 / U sources per step)
    while (c.U > 1 && (nvec + 256ull * c.U - 1) / (256ull * c.U) < 2ull * in.cus) c.U /= 2;
    if (in.knob_u != kUnset) c.U = in.knob_u;
    const uint32_t per = vectors_per_wg(c.U);
    c.wgs = (uint32_t)((nvec + per - 1) / per > 1 ? (nvec + per - 1) / per : 1);
    c.ring_waves = (nvec + 511) / 512;              // 8 KiB chunks
    c.ring = c.ring_waves >= 2ull * in.cus ? 2 : 0;  // ring depth; 0: the vector-load kernel (short rows: more, smaller pieces)
    if (in.knob_u != kUnset) c.ring = in.knob_u >= 10 ? in.knob_u - 10 : 0;  // tuning aid: 12 / 13 = ring of 2 / 3 stages, 1 / 2 / 4 = vector loads
    // short rows: groups of sources side by side until the launch holds two workgroups per CU (every group keeps at least 8 sources: the
    // kernel's pipeline of descriptor fetches and loads)
    c.groups = 1;
    const uint64_t per_cu = in.knob_groups != kUnset ? (uint64_t)(in.knob_groups > 1 ? in.knob_groups : 1) : 2ull;  // tuning aid: workgroups per CU the cut aims at
    if (!in.pre && !c.ring && in.knob_u == kUnset)
        while (c.groups < kMixGroups && (uint64_t)c.wgs * c.groups < per_cu * (uint64_t)in.cus && in.count / (c.groups * 2) >= 8) c.groups *= 2;
    // the mixed row (16-byte vectors) [, the filtered row] -- or the groups' partial rows --, then the descriptors (32 bytes each) at the very end
    c.rows_needed = in.pre ? 2 : (in.stream ? kMixGroups : c.groups);  // (a stream: sized once, for whatever its blocks will need)
    c.need = c.row * c.rows_needed + 64 + kMixGroups * 8;
    return c;
}
inline size_t row_cut_desc_offset(size_t buffer_floats) { return buffer_floats - 32 - kMixGroups * 8; }  // where the descriptors start

// ---- tickets ----------------------------------------------------------------------------------------------------------------------------
// A launch hands its tiles out by ticket -- from the one counter (*ticket), or from eight counters side by side (ticket + 32 * (1 + x):
// `shards`) of which each hands out an eighth --, unless every workgroup is resident at once (`direct`: tile = workgroup index).  The
// counters are never reset: the kernels subtract the value the host knows them to have when the launch starts.
struct Tickets {
    uint32_t ticket_base = 0;  // value of the one counter when the next launch starts
    uint32_t shard_base = 0;   // ... of every one of the eight
};
constexpr uint32_t kShards = 8;
inline uint32_t sharded_grid(uint32_t tiles) { return (tiles + kShards - 1) & ~(kShards - 1); }  // whole rounds of the eight counters
inline uint32_t batch_shards(uint32_t batch_streams, bool no_shards) { return (batch_streams >= 16 && batch_streams % kShards == 0 && !no_shards) ? kShards : 1u; }
// May a launch of `tiles` workgroups go without tickets?  Only if nothing else occupies CUs (rh_rlm_set_exclusive) and all fit at once:
// then no tile can wait for one that has no slot yet
inline bool all_resident(bool exclusive, uint64_t tiles, uint64_t cus, int per_cu) { return exclusive && tiles <= cus * (uint64_t)(per_cu > 0 ? per_cu : 0); }
// Behind a launch that was enqueued: every workgroup has taken exactly one ticket from its counter
inline void booked(Tickets *t, bool direct, uint32_t shards, uint32_t grid) {
    if (direct) return;
    if (shards > 1) t->shard_base += grid / shards;
    else t->ticket_base += grid;
}

// ---- a stream block in one kernel (k_rlm_sblk) ----------------------------------------------------------------------------------------
constexpr uint64_t kSblkHalo = 4;  // input frames two neighbouring windows share
enum SblkNo {
    kSblkYes,
    kSblkRows,      // rows that are no whole vectors, too short or too long
    kSblkRatio,     // from_rate / to_rate above 3 / 2
    kSblkRange,     // frame indices that leave the kernel's arithmetic
    kSblkInstance,  // no instance for the channel count (or the pinned one), or too many tiles
    kSblkLookBack,  // the filter reaches back over more than 32 tiles
    kSblkStart,     // the rows start behind the first tap of frame m0 - 2: not a block of this stream's own making
};
struct SblkIn {
    uint32_t C;
    uint64_t F, T;
    uint64_t avail, out;      // input frames per row, output frames
    uint64_t m0, g0, mfirst;  // global index of the first output frame / of input frame 0 of the rows / of the stream's first output frame
    uint32_t cus;
    int pin_kv;     // RH_SBLK_KV (kUnset: not set)
    uint32_t Dmax;  // frames after which the filter has forgotten
};
struct SblkGeom {
    size_t inst;  // index into the table of instances
    uint64_t reach, tiles, P, J;  // input frames the block reaches; windows, their stride; tiles a tile looks back at
    uint32_t ib, rb, mb_off;      // input frame (relative to the rows) and phase of output frame m0 - mb_off, the first the filter looks back at
};
inline bool sblk_too_long(bool direct, uint64_t tiles, uint64_t cus, int per_cu) { return !direct && tiles > 8ull * cus * (uint64_t)per_cu; }  // (the two-launch form reaches the chip's rate there)
// V: {C, R, KV, ...}.  The instance: the smallest window whose tiles fit the chip one per CU (more, smaller tiles would queue behind each
// other; fewer, larger ones leave CUs idle)
template <class V>
SblkNo sblk_geom(const V *tab, size_t n_tab, const SblkIn &in, SblkGeom *g) {
    const uint64_t C = in.C, F = in.F, T = in.T, H = kSblkHalo, FB = 4ull * C, avail = in.avail, out = in.out;
    if ((avail * C) % 4 != 0 || avail < 8 || avail >= (1ull << 29)) return kSblkRows;
    if (2 * F > 3 * T) return kSblkRatio;  // the two frames the filter looks back at start at most 3 input frames in front of a frame's first tap
    if (in.m0 + out >= (1ull << 44) || in.g0 >= (1ull << 40)) return kSblkRange;  // (m * F stays inside 64 bits)
    if ((out + 8) * F + T >= (1ull << 31) || (avail + 8) * T >= (1ull << 31)) return kSblkRange;  // (the tiles count in 32 bits, relative to the block)
    // the input frames the block's output reaches: up to the second tap of its last frame
    const uint64_t i_last = (uint64_t)(((unsigned __int128)(in.m0 + out - 1) * F) / T);
    uint64_t reach = i_last + 2 > in.g0 ? i_last + 2 - in.g0 : 1;
    reach = reach < avail ? reach : avail;
    bool picked = false;
    uint64_t tiles = 0, P = 0;
    for (size_t ii = 0; ii < n_tab; ++ii) {
        const V &v = tab[ii];
        if ((uint64_t)v.C != C) continue;
        if (in.pin_kv != kUnset && in.pin_kv != v.KV) continue;
        const uint64_t Wd = (uint64_t)v.KV * 1024 / FB, Pmax = Wd - H;
        uint64_t t = (reach > H ? reach - H + Pmax - 1 : Pmax) / Pmax;  // windows of stride Pmax that cover `reach` frames
        if (t == 0) t = 1;
        // ... at an even stride (whole 16-byte vectors), so that the tiles are of one size
        const uint64_t vf = 16 / FB;
        uint64_t Pe = ((reach > H ? reach - H : 1) + t - 1) / t;
        Pe = (Pe + vf - 1) / vf * vf;
        if (Pe > Pmax) Pe = Pmax / vf * vf;
        if ((Wd * T + F - 1) / F + 3 > 64ull * v.R) continue;  // more output frames in a window than 64 runs hold
        picked = true;
        g->inst = ii;
        tiles = t;
        P = Pe;
        if (t <= (uint64_t)in.cus) break;
    }
    if (!picked || tiles == 0 || tiles > 0x3fffffull) return kSblkInstance;
    // J: tiles in front of a tile that the filter has not forgotten (a tile owns at least (P - 1) T / F - 1 frames)
    const uint64_t n_min = (P - 1) * T / F >= 2 ? (P - 1) * T / F - 1 : 1;
    const uint64_t J = ((uint64_t)in.Dmax + n_min - 1) / n_min;
    if (J == 0 || J > 32) return kSblkLookBack;
    const uint64_t mb = in.m0 - (in.m0 - in.mfirst < 2 ? in.m0 - in.mfirst : 2);  // (fewer than two frames in front of the stream's first)
    const unsigned __int128 pp = (unsigned __int128)mb * F;
    const uint64_t ib_g = (uint64_t)(pp / T);
    if (ib_g < in.g0) return kSblkStart;
    g->reach = reach, g->tiles = tiles, g->P = P, g->J = J;
    g->ib = (uint32_t)(ib_g - in.g0);
    g->rb = (uint32_t)(pp % T);
    g->mb_off = (uint32_t)(in.m0 - mb);
    return kSblkYes;
}

}  // namespace rlm
}  // namespace rh
