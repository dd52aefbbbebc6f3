// rh_scan_launch.h -- the host-side protocol of the look-back scan kernels (rh_limit.hip, rh_biquad_scan.hip), as plain functions: which
// variant runs, what the per-stream scratch looks like, when the kernel that initialises it may be left out, which of the two hand-off
// tables a launch works on and where the ticket counter stands.  No HIP: tests/cpp/scan_launch_test.cpp runs all of it against a model of
// the device.  The launcher over it (stream_scratch, the pre-kernel, the grid, hipLaunchKernel) is scan_launch() in rh_scan_common.h.
//
// The protocol.  A launch works on ONE of two hand-off tables and sets the other one's records back to "not yet" as its tiles finish, so
// the next launch of the same kernel and shape on this stream finds its table clean and the ticket counter where the host knows it to be:
// no kernel in front of it (k_limit_init and its boundary were 5 % of a 0.27 ms call).  The first launch of a shape, a launch with a carried
// state (its snapshot is a kernel anyway), a launch behind another user of the stream's scratch and a launch behind a failed one
// initialise the counter and both tables.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>

namespace rh {

// What the last user of a stream's scratch left behind, for a user that can save itself work when IT was the last one (the scan
// kernels: hand-off tables that the launch before has already cleared).  Zeroed when the buffer is (re)allocated and by every call
// that does not ask for it (another user has written over the scratch since).  Read and written under the scratch's `hold`.
struct ScratchAux {
    uint64_t tag;          // who / what shape (0: nobody)
    uint32_t ticket_base;  // value of the scratch's ticket counter when the next launch starts
    uint32_t parity;       // which of two tables the next launch works on
};

// Polls of one hand-off before a tile gives up for good: x (~1 us load + s_sleep) = seconds.  Waits end by construction (a tile only
// waits for tiles with earlier tickets); the bound must outlast a GPU that is time-sliced with other processes.
constexpr uint32_t kSpinLimit = 1u << 22;

namespace scan {

constexpr uint64_t kSeedLimit = 0x4c494d4954ull;   // "LIMIT"
constexpr uint64_t kSeedBiquad = 0x4251554144ull;  // "BQUAD": a limiter launch never looks clean to a biquad launch of the same shape

// The scratch of a launch: 64 bytes of control words, the unit's own head (state snapshots), two hand-off tables.
struct Layout {
    size_t head, gran_bytes;  // offset of table 0; bytes per table (both multiples of 64)
    size_t total() const { return head + 2 * gran_bytes; }
    size_t table(uint32_t p) const { return head + p * gran_bytes; }
    uint64_t n_words() const { return 2 * gran_bytes / 4; }  // hand-off words of both tables
};
constexpr size_t kOwnOffset = 64;  // where the unit's own head starts
inline Layout layout(size_t own_bytes, size_t table_bytes) {
    return {64 + ((own_bytes + 63) & ~size_t(63)), (table_bytes + 63) & ~size_t(63)};
}

// Tickets are 32-bit: the tile index must stay positive as an int and one launch must take fewer than 2^32 of them (2 per workgroup ahead)
inline bool tickets_fit(uint64_t tiles, uint64_t n_streams) { return tiles <= 0x7fffffffull && tiles * n_streams < 0xfff00000ull; }

// Kernel and shape of a launch as one word (FNV-1a over the seed's successors), never 0
inline uint64_t shape_tag(uint64_t seed, uint64_t n_streams, uint64_t tiles, uint64_t channels, const Layout &l, uint64_t scratch_address) {
    uint64_t tag = seed;
    for (uint64_t v : {n_streams, tiles, channels, (uint64_t)l.head, (uint64_t)l.gran_bytes, scratch_address}) tag = (tag ^ v) * 0x100000001b3ull;
    return tag | 1;
}

struct Begin {
    bool init;             // the kernel that zeroes the control words and fills both tables with "not yet" is due in front of the launch
    uint32_t table;        // the launch's table
    int other;             // the table it clears for the next launch, or -1 (carried state: the next launch initialises its own)
    uint32_t ticket_base;  // value of the ticket counter when the launch starts
};
// In front of a launch.  Clean -- nothing to initialise -- only behind a launch of the same tag without a carried state that succeeded.
inline Begin begin(ScratchAux *aux, uint64_t tag, bool carried_state, bool force_init) {
    const bool clean = !carried_state && aux->tag == tag && !force_init;
    if (!clean) {
        aux->tag = carried_state ? 0 : tag;
        aux->ticket_base = 0;
        aux->parity = 0;
    }
    return {!clean, carried_state ? 0u : aux->parity, carried_state ? -1 : (int)(aux->parity ^ 1u), aux->ticket_base};
}
// RH_COUNTER_JUMP: the counter moves on as though launches had taken the tickets in between, to tickets_left before its wrap (which then
// falls inside this launch).  Returns what to add to the counter on the device; the launch starts at aux->ticket_base.
inline uint32_t jump(ScratchAux *aux, uint32_t tickets_left) {
    const uint32_t d = (0u - tickets_left) - aux->ticket_base;
    aux->ticket_base += d;
    return d;
}
// Behind a launch that was enqueued: every workgroup takes two tickets ahead and one per tile it works on
inline void launched(ScratchAux *aux, bool carried_state, uint64_t total_tiles, uint64_t grid) {
    if (carried_state) return;
    aux->ticket_base += (uint32_t)(total_tiles + 2 * grid);
    aux->parity ^= 1u;
}
// ... and behind one that was not: whatever state the tables are in, the next call starts over
inline void failed(ScratchAux *aux) { aux->tag = 0; }

// Resident workgroups per CU: what the runtime says fits, at most 16 waves a CU, or the *_WGS knob (0: unset)
inline int per_cu(int occupancy, int waves_per_wg, int knob) {
    int n = occupancy < 1 ? 1 : occupancy;
    if (n * waves_per_wg > 16) n = 16 / waves_per_wg > 0 ? 16 / waves_per_wg : 1;
    return knob > 0 ? knob : n;
}
inline uint64_t launch_grid(uint64_t cus, int per_cu, uint64_t total_tiles) {
    const uint64_t g = cus * (uint64_t)per_cu;
    return g > total_tiles ? total_tiles : g;
}

// Geometry: the LONGEST tile (64 * R * NW frames) that a stream fills at least half of; among equals, more frames per lane; nothing
// fits: the shortest.  Long tiles amortise the scans and the look-backs, and a slowly decaying recurrence (100 ms of release) reaches back
// over MANY short tiles: measured (profiles/r02_scan_geometry_midsize.txt) 8192-frame tiles win from 64 x 1 Mi frames down to
// 256 x 8192 (21 us against 49 us with single-wave tiles; the biquad: 0.240 ms with R = 16 against 0.261 ms with R = 8), although the
// short batches then have fewer tiles than the chip has CUs.  Single-wave tiles are for blocks of a few hundred frames (a pull shim's).
// With a request (the RH_*_R / RH_*_NW tuning aids): the variant closest to it.  Variants that `allowed` refuses are never chosen;
// nullptr: no variant for this channel count.
struct Request {
    int R, NW;
};
template <class V, size_t N, class Allowed>
const V *pick_variant(const V (&table)[N], uint32_t channels, uint64_t frames, const Request *want, Allowed allowed) {
    auto tile_of = [](const V &x) { return (uint64_t)64 * x.R * x.NW; };
    auto score = [&](const V &x) { return 10 * std::abs(x.NW - want->NW) + std::abs(x.R - want->R); };
    const V *v = nullptr;
    for (const V &c : table) {
        if (c.C != (int)channels || !allowed(c)) continue;
        if (!v) {
            v = &c;
            continue;
        }
        bool better;
        if (want) {
            better = score(c) < score(*v);
        } else {
            const bool fits_c = tile_of(c) <= 2 * frames, fits_v = tile_of(*v) <= 2 * frames;
            better = fits_c != fits_v ? fits_c
                                      : (fits_c ? (tile_of(c) > tile_of(*v) || (tile_of(c) == tile_of(*v) && c.R > v->R))  // the longest that fits
                                                : tile_of(c) < tile_of(*v));                                               // nothing fits: the shortest
        }
        if (better) v = &c;
    }
    return v;
}

}  // namespace scan
}  // namespace rh
