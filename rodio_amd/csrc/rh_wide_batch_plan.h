// rh_wide_batch_plan.h -- what rh_wide_mix_batch (rh_widebatch.hip) decides on the host, as one plain function over the caller's arrays: the
// status of the call, the tables the kernel reads (a mixer, a source, a tile each) and the map from workgroup to (mixer, first output sample).
// No HIP: tests/cpp/wide_batch_plan_test.cpp runs it without a GPU.  The upload and the launch are rh_wide_mix_batch's.
//
// A TILE is up to tile_samples consecutive output samples of ONE mixer, served by one workgroup.  The map is a table, not a closed form over
// a 2-D grid (mixers x tiles of the longest one, early exit): a ragged batch -- 300 blocks of 33 frames beside one of 70 000 -- would launch
// 301 x 547 workgroups for the 847 that have something to do, and only a table lets the tiles of the mixers with the most sources go first.
// Its cost is 16 bytes a workgroup in the copy that carries the other two tables anyway.  (Reasoned, not measured against the closed form.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/rodio_hip.h"
#include "rh_mix_plan.h"

namespace rh {
namespace widebatch {

constexpr uint32_t kBlock = 256;        // lanes of a workgroup: one output sample each, `per` times
using mixplan::kGroup;                  // sources whose tap loads leave together; a mixer's slots are whole groups
constexpr uint32_t kUniGroup = 8;       // ... of a mixer of alike sources (k_wide_mix_uniform's kUniGroup: sixteen loads a lane)
using mixplan::kRates;                  // (rate, phase) pairs of a mixer whose division a lane does once per sample
constexpr uint32_t kOwnRate = kRates;   // Src::rate of a source beyond them: it divides for itself
constexpr uint32_t kMaxTiles = 16384;   // above this many tiles a lane takes 2, 4, .. samples (256 CUs x 8 workgroups x 8 rounds)
constexpr uint32_t kMaxPer = 4096;      // ... up to this many: a tile never exceeds 2^20 samples
using mixplan::Rate;
struct Mixer {  // 104 bytes
    float *dst;
    uint32_t ch, frames;
    uint32_t src_first, src_slots;  // its slots of the source table: the sources that reach the block in insertion order, padded to whole groups
    uint32_t tile_first, n_tiles;   // its tiles of the tile table (one run, in the order of its samples)
    uint32_t uniform, pad;          // 1: alike sources (below) -- r[0] is their pair, and the slots are whole groups of kUniGroup
    Rate r[kRates];
};
struct Src {  // 48 bytes: WideDesc of rh_widemix.hip, and the rate of a source that divides for itself
    const float *data;
    uint32_t ch, frames, last;
    uint32_t rate;  // index into Mixer::r, or kOwnRate
    float gain, Tf;  // Tf: T as a float; 0: the converter passes through (F == T)
    uint32_t F, T, r0;
    uint32_t pad;
};
struct Tile {  // 16 bytes: output samples [j0 * ch + c0, .. + n) of `mixer`
    uint32_t mixer, j0, c0, n;
};

struct Plan {
    std::vector<Mixer> mixers;       // one per mixer of the call (a skipped one: frames == 0, no slots, no tiles)
    std::vector<uint64_t> in_first;  // n_mixers + 1: where a mixer's sources lie in srcs_host (the prefix sums of the counts)
    std::vector<Src> srcs;
    std::vector<Tile> tiles;         // in launch order: the mixers with the most sources first
    uint32_t tile_samples = 0;
    std::vector<uint32_t> live;      // per mixer: the sources that reach its block
    std::vector<uint32_t> order;     // the mixers that have tiles, in launch order
};

using mixplan::check_src;  // (a block that does not fit one launch is refused behind the mixer's table: rh_wide_mix_block cuts such a block)

// Samples a lane takes (a tile is kBlock * per samples): 1, doubled while the batch would be more than kMaxTiles tiles.
inline uint64_t count_tiles(const std::vector<Mixer> &mixers, uint64_t tile_samples) {
    uint64_t n = 0;
    for (const Mixer &m : mixers) n += ((uint64_t)m.frames * m.ch + tile_samples - 1) / tile_samples;
    return n;
}

// The plan of one call.  Anything but RH_OK: the call is refused, and nothing of *p may be used.
inline rh_status plan(float *const *dsts, const uint32_t *channels, const uint32_t *to_rates, const uint64_t *out_frames, const uint32_t *src_counts, uint32_t n_mixers,
                      const rh_wide_src *srcs, Plan *p) {
    p->mixers.clear(), p->in_first.clear(), p->srcs.clear(), p->tiles.clear(), p->live.clear(), p->order.clear();
    p->tile_samples = kBlock;
    if (n_mixers == 0) return RH_OK;
    if (!dsts || !channels || !to_rates || !out_frames || !src_counts) return RH_ERR_INVALID;
    p->mixers.resize(n_mixers);
    p->in_first.resize((size_t)n_mixers + 1);
    p->live.assign(n_mixers, 0u);
    uint64_t at = 0;
    for (uint32_t b = 0; b < n_mixers; ++b) {
        p->in_first[b] = at;
        at += src_counts[b];
    }
    p->in_first[n_mixers] = at;
    if (at && !srcs) return RH_ERR_INVALID;
    for (uint32_t b = 0; b < n_mixers; ++b) {
        Mixer &m = p->mixers[b];
        m = Mixer{};
        for (uint32_t q = 0; q < kRates; ++q) m.r[q] = Rate{0u, 1u, 0u, 1.0f};
        if (out_frames[b] == 0) continue;  // (as rh_wide_mix_block: nothing of such a mixer is looked at)
        if (!dsts[b] || channels[b] == 0 || to_rates[b] == 0) return RH_ERR_INVALID;
        if (out_frames[b] > 0x7fffffffull) return RH_ERR_UNSUPPORTED;
        m.dst = dsts[b], m.ch = channels[b], m.frames = (uint32_t)out_frames[b];
        if (p->srcs.size() > 0xfffffff0ull) return RH_ERR_UNSUPPORTED;
        m.src_first = (uint32_t)p->srcs.size();
        uint32_t nr = 0;
        bool fits = true;
        for (uint64_t s = p->in_first[b]; s < p->in_first[b + 1]; ++s) {
            const rh_wide_src &x = srcs[s];
            if (x.frames == 0) continue;
            uint32_t F, T;
            uint64_t fit;
            const rh_status st = check_src(x, to_rates[b], out_frames[b], &F, &T, &fit);
            if (st != RH_OK) return st;
            fits = fits && fit >= out_frames[b];  // (rh_wide_mix_block cuts such a block into launches)
            uint32_t q = 0;
            while (q < nr && !(m.r[q].F == F && m.r[q].T == T && m.r[q].r0 == x.phase)) ++q;
            if (q == nr && nr < kRates) m.r[nr++] = Rate{F, T, x.phase, (float)T};
            p->srcs.push_back(Src{x.data, x.channels, (uint32_t)x.frames, x.last, q, x.gain, F == T ? 0.0f : (float)T, F, T, x.phase, 0u});
        }
        if (!fits) return RH_ERR_UNSUPPORTED;
        p->live[b] = (uint32_t)(p->srcs.size() - m.src_first);
        // Alike sources (k_wide_mix_uniform's case): the mixer's layout, ONE (rate, phase) pair, every source reaches every frame of the block with
        // both taps (none ends inside it).  Then the tap offset and the weight are the lane's own, once; the same operations in the same order.
        bool uni = p->live[b] > 0 && nr == 1;
        const uint64_t il_max = ((uint64_t)m.r[0].r0 + (uint64_t)(m.frames - 1) * m.r[0].F) / m.r[0].T;
        for (size_t s = m.src_first; s < p->srcs.size() && uni; ++s) {
            const Src &d = p->srcs[s];
            uni = d.ch == m.ch && d.frames == m.frames && (d.Tf == 0.0f || il_max < d.last);
        }
        m.uniform = uni ? 1u : 0u;
        while ((p->srcs.size() - m.src_first) % (uni ? kUniGroup : kGroup))  // whole groups: slots that reach no frame (and point at something readable: the first source's first tap)
            p->srcs.push_back(Src{p->srcs[m.src_first].data, 1u, 0u, 0u, 0u, 0.0f, 0.0f, 0u, 1u, 0u, 0u});
        m.src_slots = (uint32_t)(p->srcs.size() - m.src_first);
    }
    // the tiles: a lane takes `per` samples
    uint64_t per = 1, n_tiles = count_tiles(p->mixers, kBlock);
    while (n_tiles > kMaxTiles && per < kMaxPer) per *= 2, n_tiles = count_tiles(p->mixers, kBlock * per);
    if (n_tiles > 0x7fffffffull) return RH_ERR_UNSUPPORTED;
    p->tile_samples = (uint32_t)(kBlock * per);
    // ... issued mixer by mixer, the ones with the most sources first (the long pole does not start last); Mixer::tile_first says where
    for (uint32_t b = 0; b < n_mixers; ++b) {
        Mixer &m = p->mixers[b];
        m.n_tiles = (uint32_t)(((uint64_t)m.frames * m.ch + p->tile_samples - 1) / p->tile_samples);
        if (m.n_tiles) p->order.push_back(b);
    }
    std::stable_sort(p->order.begin(), p->order.end(), [&](uint32_t a, uint32_t b) { return p->live[a] > p->live[b]; });
    p->tiles.reserve((size_t)n_tiles);
    uint32_t first = 0;
    for (uint32_t b : p->order) {
        Mixer &m = p->mixers[b];
        m.tile_first = first;
        first += m.n_tiles;
        const uint64_t total = (uint64_t)m.frames * m.ch;
        for (uint32_t k = 0; k < m.n_tiles; ++k) {
            const uint64_t o = (uint64_t)k * p->tile_samples;
            p->tiles.push_back(Tile{b, (uint32_t)(o / m.ch), (uint32_t)(o % m.ch), (uint32_t)std::min<uint64_t>(total - o, p->tile_samples)});
        }
    }
    return RH_OK;
}

// A call of ONE mixer is handed to rh_wide_mix_block where that entry takes ONE launch for it -- there the table copy in front of the batch
// kernel costs more than it saves (profiles/wide_batch.txt) -- and stays a batch where it would take several: more than 32 sources, more than
// four (rate, phase) pairs, or alike sources of which one ends inside the block (that entry cuts such a block in two).
inline bool one_mixer_goes_alone(const Plan &p) {
    if (p.mixers.size() != 1 || p.live[0] > 32) return false;
    const Mixer &m = p.mixers[0];
    bool own_layout = true;
    for (uint32_t s = 0; s < p.live[0]; ++s) {
        if (p.srcs[m.src_first + s].rate >= kRates) return false;
        own_layout = own_layout && p.srcs[m.src_first + s].ch == m.ch;
    }
    const bool one_pair = m.r[0].F != 0 && m.r[1].F == 0;
    return m.uniform || !(one_pair && own_layout);
}

}  // namespace widebatch
}  // namespace rh
