// rlm_launch_test.cpp -- the launch decisions of the fused path (rodio_amd/csrc/rh_rlm_launch.h) without a GPU: the route of a launch against
// the rule written out a second time (the nested conditions rlm_launch had, in their order), the cut of the mixed row by its properties and
// by hand-computed cases, the ticket accounting against a model of the device's counters, and the geometry of a stream block in one kernel
// by its properties.  TEST INFRASTRUCTURE: plain g++, no HIP, no library.
//
//     rlm_launch_test [seed [random launches]]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "rh_rlm_launch.h"

using namespace rh::rlm;

static int g_failures = 0;
#define EXPECT(cond, ...)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++g_failures <= 20) {                      \
                std::fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
                std::fprintf(stderr, __VA_ARGS__);         \
                std::fprintf(stderr, "\n");                \
            }                                              \
        }                                                  \
    } while (0)

// ---- the route ---------------------------------------------------------------------------------------------------------------
// The conditions as rlm_launch, rh_rlm_geometry, stream_block_summed and chunk_launch_classes spelt them before they shared route()
static bool old_mix_first_applies(const RouteIn &in, uint32_t count, bool per_source_states, bool batch) {
    return in.plan == kPlanFast && in.filt && in.mix_first_on && !per_source_states && !batch && count >= 2 && !in.no_mix_first;
}
static Route old_rlm_launch(const RouteIn &in) {
    if (in.plan == kPlanPair && !in.st_mode && !in.batch_streams) {
        return kPair;
    }
    if (in.chunk_ok && !in.st_mode && old_mix_first_applies(in, in.count, false, in.batch_streams != 0) && in.count == in.n_sources && in.first == 0) {
        return kChunk;
    }
    const bool pre = in.pre_filter;
    if (pre && (in.plan != kPlanFast || in.st_mode || in.batch_streams)) return kUnsupported;
    if (pre || old_mix_first_applies(in, in.count, in.gran_cols != 0, in.batch_streams != 0)) {
        return pre ? kMixedFiltered : kMixed;
    }
    return in.batch_streams ? kBatch : kPlain;
}
static uint32_t old_geometry_mix_first(const RouteIn &in) {
    return (in.pre_filter && in.plan == kPlanFast) ? 1u : old_mix_first_applies(in, in.n_sources, false, false) ? (in.chunk_ok ? 2u : 1u) : 0u;
}

static long test_route(long *reached) {
    long n = 0;
    const uint32_t sources[] = {0, 1, 2, 3, 5}, batches[] = {0, 1, 8, 16}, modes[] = {0, 1, 2}, cols[] = {0, 7};
    for (int plan = 0; plan < 3; ++plan)
        for (int bits = 0; bits < 32; ++bits)
            for (uint32_t ns : sources)
                for (uint32_t count : {0u, 1u, 2u, ns})
                    for (uint32_t first : {0u, 1u})
                        for (uint32_t batch : batches)
                            for (uint32_t mode : modes)
                                for (uint32_t gc : cols) {
                                    RouteIn in{};
                                    in.plan = (PlanKind)plan;
                                    in.filt = bits & 1, in.mix_first_on = bits & 2, in.pre_filter = bits & 4, in.chunk_ok = bits & 8, in.no_mix_first = bits & 16;
                                    in.first = first, in.count = count, in.n_sources = ns, in.batch_streams = batch, in.st_mode = mode, in.gran_cols = gc;
                                    const Route r = route(in), want = old_rlm_launch(in);
                                    EXPECT(r == want, "plan %d bits %d ns %u count %u first %u batch %u mode %u cols %u: %d, was %d", plan, bits, ns, count, first, batch, mode, gc, (int)r,
                                           (int)want);
                                    reached[r] += 1;
                                    n += 1;
                                    const bool whole = first == 0 && count == ns && !batch && !mode && !gc;
                                    // rh_rlm_geometry and the pre-check of chunk_launch_classes ask about a whole one-shot run (a handle with pre_filter has no filt)
                                    if (whole && !(in.pre_filter && in.filt)) EXPECT(mix_first_code(r) == old_geometry_mix_first(in), "plan %d bits %d ns %u", plan, bits, ns);
                                    if (whole) EXPECT((r == kChunk) == (in.chunk_ok && old_mix_first_applies(in, ns, false, false)), "plan %d bits %d ns %u", plan, bits, ns);
                                    // stream_block_summed: a block of a stream (no pre_filter: rh_rlm_stream_begin refuses it) on the fast plan
                                    if (plan == kPlanFast && first == 0 && count == ns && !batch && mode && !gc && !in.pre_filter)
                                        EXPECT((r == kMixed) == old_mix_first_applies(in, ns, false, false), "bits %d ns %u mode %u", bits, ns, mode);
                                }
    for (int r = 0; r < kRoutes; ++r) EXPECT(reached[r] > 0, "route %d never taken", r);
    return n;
}

// ---- the cut of the mixed row ---------------------------------------------------------------------------------------------------
static bool pow2(uint32_t x) { return x && !(x & (x - 1)); }
static void check_cut(const RowCutIn &in) {
    const RowCut c = row_cut(in);
    const uint64_t nvec = in.n_floats / 4, chip = 2ull * in.cus;
    const bool knob_u = in.knob_u != kUnset;
    EXPECT((uint64_t)c.wgs * vectors_per_wg(c.U) >= nvec && c.wgs >= 1, "n_floats %llu", (unsigned long long)in.n_floats);
    EXPECT(c.wgs == 1 || (uint64_t)(c.wgs - 1) * vectors_per_wg(c.U) < nvec, "n_floats %llu: a workgroup too many", (unsigned long long)in.n_floats);
    EXPECT(c.ring_waves * 512 >= nvec, "n_floats %llu", (unsigned long long)in.n_floats);
    if (!knob_u) {
        // the most vectors per lane (4, 2, 1) that still leave two workgroups per CU, else 1; the ring where 8 KiB chunks do
        int want = 1;
        for (int U : {2, 4})
            if ((nvec + 256ull * U - 1) / (256ull * U) >= chip) want = U;
        EXPECT(c.U == want, "n_floats %llu cus %u: U %d, want %d", (unsigned long long)in.n_floats, in.cus, c.U, want);
        EXPECT(c.ring == ((nvec + 511) / 512 >= chip ? 2 : 0), "n_floats %llu cus %u: ring %d", (unsigned long long)in.n_floats, in.cus, c.ring);
    } else {
        EXPECT(c.U == in.knob_u && c.ring == (in.knob_u >= 10 ? in.knob_u - 10 : 0) && c.groups == 1, "knob %d: U %d ring %d groups %u", in.knob_u, c.U, c.ring, c.groups);
    }
    EXPECT(pow2(c.groups) && c.groups <= 16, "groups %u", c.groups);
    if (c.groups > 1) EXPECT(in.count / c.groups >= 8, "count %u in %u groups", in.count, c.groups);
    if (c.ring || in.pre) EXPECT(c.groups == 1, "ring %d pre %d groups %u", c.ring, (int)in.pre, c.groups);
    if (!c.ring && !in.pre && !knob_u) {  // as many groups as it takes to reach the workgroups per CU aimed at, and no more
        const uint64_t aim = (in.knob_groups == kUnset ? 2ull : (uint64_t)std::max(1, in.knob_groups)) * in.cus;
        if (c.groups > 1) EXPECT((uint64_t)c.wgs * (c.groups / 2) < aim, "groups %u wgs %u", c.groups, c.wgs);
        if (c.groups < 16 && in.count / (c.groups * 2) >= 8) EXPECT((uint64_t)c.wgs * c.groups >= aim, "groups %u wgs %u count %u", c.groups, c.wgs, in.count);
    }
    // the buffer: the rows (whole vectors, every group's partial row or the filtered row among them), behind them the descriptors and 32 floats
    EXPECT(c.row % 4 == 0 && c.row >= (in.stream ? in.stream_floats : in.n_floats), "row %zu", c.row);
    EXPECT(c.rows_needed >= (in.pre ? 2u : c.groups), "rows %zu groups %u", c.rows_needed, c.groups);
    EXPECT(row_cut_desc_offset(c.need) >= c.row * c.rows_needed && row_cut_desc_offset(c.need) + kMixGroups * 8 <= c.need, "need %zu row %zu x %zu", c.need, c.row, c.rows_needed);
}
static long test_row_cut() {
    long n = 0;
    for (uint32_t cus : {1u, 8u, 256u}) {
        std::vector<uint64_t> edges = {0, 1, 2, 3};  // in vectors: where U, the ring or the number of workgroups changes
        for (uint64_t U : {1, 2, 4}) edges.push_back(256 * U * (2ull * cus - 1)), edges.push_back(256 * U * 2ull * cus), edges.push_back(256 * U);
        edges.push_back(512ull * (2ull * cus - 1)), edges.push_back(512ull * 2 * cus), edges.push_back(256ull * cus), edges.push_back(64ull * cus);
        for (uint64_t e : edges)
            for (int d = -2; d <= 2; ++d)
                for (uint32_t rest = 0; rest < 4; rest += 3)
                    for (uint32_t count : {2u, 8u, 15u, 16u, 17u, 32u, 255u, 256u})
                        for (int pre = 0; pre < 2; ++pre)
                            for (int stream = 0; stream < 2; ++stream)
                                for (int ku : {kUnset, 1, 2, 4, 0, 3, 12, 13})
                                    for (int kg : {kUnset, 0, 1, 4, 64}) {
                                        if ((int64_t)e + d < 0 || (pre && stream)) continue;
                                        const uint64_t n_floats = 4 * (e + d) + rest;
                                        check_cut({n_floats, count, cus, pre != 0, stream != 0, n_floats + 4096, ku, kg});
                                        n += 1;
                                    }
    }
    // by hand from the code this header took over.  The headline (256 sources x 1 Mi stereo frames on 256 CUs): 512 Ki vectors = 512
    // workgroups of 1024 -- two per CU at U = 4 -- and 1024 chunks of 8 KiB: the ring of two stages, one row
    RowCut c = row_cut({2ull << 20, 256, 256, false, false, 0, kUnset, kUnset});
    EXPECT(c.U == 4 && c.wgs == 512 && c.ring == 2 && c.ring_waves == 1024 && c.groups == 1 && c.row == (2u << 20) && c.rows_needed == 1 && c.need == (2u << 20) + 192, "headline: U %d wgs %u ring %d",
           c.U, c.wgs, c.ring);
    // a 64 Ki-frame stereo block of a stream of 256 sources: 32 Ki vectors, 128 workgroups at U = 1, four groups of 64 sources; sized for 16 rows
    c = row_cut({128u << 10, 256, 256, false, true, 128u << 10, kUnset, kUnset});
    EXPECT(c.U == 1 && c.wgs == 128 && c.ring == 0 && c.ring_waves == 64 && c.groups == 4 && c.row == (128u << 10) && c.rows_needed == 16 && c.need == (2u << 20) + 192,
           "stream block: U %d wgs %u ring %d groups %u", c.U, c.wgs, c.ring, c.groups);
    // ... of 16 sources: one group (a second would leave 8 sources a group, but 16 / 4 < 8 stops the next), ... of 32: two
    EXPECT(row_cut({128u << 10, 16, 256, false, true, 128u << 10, kUnset, kUnset}).groups == 2, "16 sources");
    EXPECT(row_cut({128u << 10, 15, 256, false, true, 128u << 10, kUnset, kUnset}).groups == 1, "15 sources");
    // filter_first, 16 x 8192 stereo frames: 4096 vectors, 16 workgroups, no groups, the mixed and the filtered row
    c = row_cut({16384, 16, 256, true, false, 0, kUnset, kUnset});
    EXPECT(c.U == 1 && c.wgs == 16 && c.ring == 0 && c.groups == 1 && c.rows_needed == 2 && c.need == 2 * 16384 + 192, "filter_first: U %d wgs %u", c.U, c.wgs);
    // RH_MIX_U=12: the ring of two stages whatever the length (U itself then only sizes the unused k_mix_rows grid: 1024 vectors a workgroup)
    c = row_cut({16384, 16, 256, false, false, 0, 12, kUnset});
    EXPECT(c.U == 12 && c.ring == 2 && c.wgs == 4 && c.groups == 1, "RH_MIX_U=12: U %d ring %d wgs %u", c.U, c.ring, c.wgs);
    return n + 6;
}

// ---- tickets -----------------------------------------------------------------------------------------------------------------------
// The device: the one counter and the eight sharded ones.  A launch that is not direct: workgroup w takes one ticket -- from counter w % 8
// when sharded (a workgroup's XCD), else from the one --, subtracts the base it was given and works on that tile; every tile exactly once.
struct Counters {
    uint32_t one, shard[kShards];
};
static void device_launch(Counters &d, bool direct, uint32_t shards, uint32_t grid, const Tickets &base) {
    if (direct) return;
    std::vector<uint8_t> seen(grid, 0);
    for (uint32_t w = 0; w < grid; ++w) {
        const uint32_t x = w % kShards;
        const uint32_t tile = shards > 1 ? (d.shard[x]++ - base.shard_base) * shards + x : d.one++ - base.ticket_base;
        EXPECT(tile < grid && !seen[tile], "grid %u shards %u: workgroup %u got tile %u", grid, shards, w, tile);
        if (tile < grid) seen[tile] = 1;
    }
}
static void in_step(const Counters &d, const Tickets &t, const char *what) {
    EXPECT(t.ticket_base == d.one, "%s: ticket_base %u, the counter %u", what, t.ticket_base, d.one);
    for (uint32_t x = 0; x < kShards; ++x) EXPECT(t.shard_base == d.shard[x], "%s: shard_base %u, counter %u at %u", what, t.shard_base, x, d.shard[x]);
}
// One launch of every shape the fused path has, booked the way its launch site books it
static long ticket_sequence(std::mt19937 &rng, uint32_t start, long launches, long *wraps) {
    Counters d;
    d.one = start;
    for (uint32_t &c : d.shard) c = start;
    Tickets t;
    t.ticket_base = t.shard_base = start;
    auto launch = [&](bool direct, uint32_t shards, uint32_t grid, const char *what) {
        const Tickets before = t;
        device_launch(d, direct, shards, grid, t);
        booked(&t, direct, shards, grid);
        in_step(d, t, what);
        if (t.ticket_base < before.ticket_base || t.shard_base < before.shard_base) *wraps += 1;
    };
    for (long i = 0; i < launches; ++i) {
        const uint32_t tiles = 1 + rng() % (rng() % 4 ? 300 : 5000);
        const bool direct = rng() % 3 == 0;
        switch (rng() % 6) {
        case 0:  // the ragged pair: the first half from the eight counters, k_rlm_resid (RH_RAG_TWO_KERNELS) from the one
            launch(false, kShards, sharded_grid(tiles), "pair");
            if (rng() % 2) launch(false, 1, tiles, "pair, second kernel");
            break;
        case 1: launch(direct, kShards, direct ? tiles : sharded_grid(tiles), "chunk"); break;
        case 2: {  // classes in one launch: every class's share of k_rlm_chunk_multi, or k_rlm_chunk_classes without tickets
            const uint32_t n = 2 + rng() % 6;
            for (uint32_t k = 0; k < n; ++k) launch(direct, kShards, sharded_grid(tiles + (direct ? 0 : rng() % 9)), "classes");
            break;
        }
        case 3: launch(direct, 1, tiles, "plain / mixed"); break;
        case 4: {  // batch mode: a ticket per tile and stream
            const uint32_t streams = 1 + rng() % 40, shards = batch_shards(streams, rng() % 4 == 0);
            EXPECT(shards == 1 || (tiles * streams) % shards == 0, "%u streams", streams);
            launch(false, shards, tiles * streams, "batch");
            break;
        }
        default: launch(direct, kShards, direct ? tiles : sharded_grid(tiles), "sblk"); break;
        }
    }
    return launches;
}

// ---- a stream block in one kernel -----------------------------------------------------------------------------------------------------
struct Inst {
    int R, C, KV;
};
static const Inst kInst[] = {{3, 2, 1}, {5, 2, 2}, {7, 2, 3}, {9, 2, 4}, {5, 1, 1}, {9, 1, 2}};  // the instances of k_rlm_sblk (rh_pipeline_sblk.hip)
static uint64_t gcd(uint64_t a, uint64_t b) { return b ? gcd(b, a % b) : a; }
static bool eligible(const Inst &v, const SblkIn &in) {
    const uint64_t Wd = (uint64_t)v.KV * 1024 / (4 * in.C);
    return (uint32_t)v.C == in.C && (in.pin_kv == kUnset || in.pin_kv == v.KV) && (Wd * in.T + in.F - 1) / in.F + 3 <= 64ull * v.R;
}
static uint64_t window(const Inst &v, const SblkIn &in) { return (uint64_t)v.KV * 1024 / (4 * in.C) - kSblkHalo; }  // a window's stride at most
static uint64_t reach0(const SblkIn &in) {  // input frames behind the halo that the block reaches (at least one)
    const uint64_t i_last = (uint64_t)(((unsigned __int128)(in.m0 + in.out - 1) * in.F) / in.T);
    const uint64_t reach = std::min<uint64_t>(in.avail, i_last + 2 > in.g0 ? i_last + 2 - in.g0 : 1);
    return reach > kSblkHalo ? reach - kSblkHalo : 1;
}
static long test_sblk(std::mt19937 &rng, long cases, long *accepted, long *refused) {
    const uint32_t rates[] = {8000, 11025, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 192000};
    for (long i = 0; i < cases; ++i) {
        SblkIn in{};
        const uint32_t from = rates[rng() % 10], to = rates[rng() % 10];
        in.C = 1 + rng() % 2;
        in.F = from / gcd(from, to), in.T = to / gcd(from, to);
        in.avail = (rng() % 8 == 0 ? 1 + rng() % 64 : 4ull * (2 + rng() % (rng() % 4 ? 1500 : 40000))) + (rng() % 16 == 0 ? 1 + rng() % 3 : 0);
        if (rng() % 64 == 0) in.avail = (1ull << 29) + 4 * (rng() % 3) - 4;
        in.m0 = rng() % 3 == 0 ? 0 : (rng() % 5 == 0 ? ((1ull << 44) - (rng() % 100000)) : rng() % (1ull << 33));
        in.mfirst = rng() % 4 == 0 ? in.m0 - std::min<uint64_t>(in.m0, rng() % 3) : 0;
        const uint64_t i0 = (uint64_t)(((unsigned __int128)in.m0 * in.F) / in.T);
        in.g0 = i0 - std::min<uint64_t>(i0, rng() % 8) + (rng() % 16 == 0 ? 1 + rng() % 3 : 0);  // the rows start a few frames in front of frame m0's first tap (or, rarely, behind it)
        const uint64_t can = in.avail * in.T / in.F;
        in.out = rng() % 32 == 0 ? (1ull << 31) / in.F : 1 + (can > 8 ? can - rng() % 8 : rng() % 8);
        in.cus = rng() % 3 ? 256 : 8;
        const int pins[] = {kUnset, kUnset, kUnset, kUnset, 1, 2, 3, 4, 7, 0};
        in.pin_kv = pins[rng() % 10];
        in.Dmax = rng() % 8 == 0 ? 20000 + rng() % 45000 : 40 + rng() % 3000;
        SblkGeom g{};
        const SblkNo no = sblk_geom(kInst, 6, in, &g);
        const uint64_t FB = 4ull * in.C, vf = 16 / FB, H = kSblkHalo;
        const bool rows = (in.avail * in.C) % 4 != 0 || in.avail < 8 || in.avail >= (1ull << 29), ratio = 2 * in.F > 3 * in.T;
        const bool range = in.m0 + in.out >= (1ull << 44) || in.g0 >= (1ull << 40) || (in.out + 8) * in.F + in.T >= (1ull << 31) || (in.avail + 8) * in.T >= (1ull << 31);
        const uint64_t mb = in.m0 - std::min<uint64_t>(2, in.m0 - in.mfirst);
        const unsigned __int128 pp = (unsigned __int128)mb * in.F;
        const bool behind = (uint64_t)(pp / in.T) < in.g0;
        refused[no] += 1;
        if (no != kSblkYes) {  // for the reason it names, and for the first that holds
            EXPECT((no == kSblkRows) == rows, "avail %llu: %d", (unsigned long long)in.avail, (int)no);
            if (!rows) EXPECT((no == kSblkRatio) == ratio, "F %llu T %llu: %d", (unsigned long long)in.F, (unsigned long long)in.T, (int)no);
            if (!rows && !ratio) EXPECT((no == kSblkRange) == range, "m0 %llu out %llu: %d", (unsigned long long)in.m0, (unsigned long long)in.out, (int)no);
            if (rows || ratio || range) continue;
            bool any = false;
            uint64_t fewest = 0;  // windows of the largest instance that may run
            for (const Inst &v : kInst)
                if (eligible(v, in)) any = true, fewest = std::max<uint64_t>(1, (reach0(in) + window(v, in) - 1) / window(v, in));
            if (no == kSblkInstance) EXPECT(!any || fewest > 0x3fffffull, "an instance fits: C %u pin %d, %llu windows", in.C, in.pin_kv, (unsigned long long)fewest);
            else EXPECT(any && fewest <= 0x3fffffull, "no instance: C %u pin %d, reason %d", in.C, in.pin_kv, (int)no);
            if (no == kSblkStart) EXPECT(behind, "m0 %llu g0 %llu", (unsigned long long)in.m0, (unsigned long long)in.g0);
            EXPECT(no == kSblkInstance || no == kSblkLookBack || no == kSblkStart, "reason %d", (int)no);
            continue;
        }
        *accepted += 1;
        EXPECT(!rows && !ratio && !range && !behind, "accepted: rows %d ratio %d range %d behind %d", (int)rows, (int)ratio, (int)range, (int)behind);
        const Inst &v = kInst[g.inst];
        EXPECT(eligible(v, in), "instance %zu", g.inst);
        const uint64_t Wd = (uint64_t)v.KV * 1024 / FB, Pmax = Wd - H;
        const uint64_t i_last = (uint64_t)(((unsigned __int128)(in.m0 + in.out - 1) * in.F) / in.T);
        const uint64_t reach = std::min<uint64_t>(in.avail, i_last + 2 > in.g0 ? i_last + 2 - in.g0 : 1);
        EXPECT(g.reach == reach, "reach %llu, want %llu", (unsigned long long)g.reach, (unsigned long long)reach);
        EXPECT(g.tiles >= 1 && g.tiles * g.P + H >= g.reach, "tiles %llu of stride %llu, reach %llu", (unsigned long long)g.tiles, (unsigned long long)g.P, (unsigned long long)g.reach);
        EXPECT(g.tiles == 1 || (g.tiles - 1) * Pmax + H < g.reach, "tiles %llu, a window too many for reach %llu", (unsigned long long)g.tiles, (unsigned long long)g.reach);
        EXPECT(g.P >= vf && g.P % vf == 0 && g.P <= Pmax, "P %llu Pmax %llu", (unsigned long long)g.P, (unsigned long long)Pmax);
        EXPECT((Wd * in.T + in.F - 1) / in.F + 3 <= 64ull * v.R, "a window's output frames, R %d", v.R);
        const uint64_t n_min = std::max<uint64_t>(1, (g.P - 1) * in.T / in.F >= 2 ? (g.P - 1) * in.T / in.F - 1 : 1);
        EXPECT(g.J >= 1 && g.J <= 32 && g.J * n_min >= in.Dmax && (g.J - 1) * n_min < in.Dmax, "J %llu Dmax %u", (unsigned long long)g.J, in.Dmax);
        EXPECT((uint64_t)(pp / in.T) == in.g0 + g.ib && g.rb == (uint32_t)(pp % in.T) && g.mb_off == in.m0 - mb && g.mb_off <= 2, "ib %u rb %u mb_off %u", g.ib, g.rb, g.mb_off);
        // the smallest window whose tiles fit the chip one per CU, else the largest there is
        for (size_t k = 0; k < 6; ++k) {
            if (!eligible(kInst[k], in)) continue;
            const uint64_t Pk = (uint64_t)kInst[k].KV * 1024 / FB - H, tk = std::max<uint64_t>(1, (reach > H ? reach - H + Pk - 1 : Pk) / Pk);
            if (k < g.inst) EXPECT(tk > in.cus, "instance %zu fits already (%llu tiles)", k, (unsigned long long)tk);
            if (k > g.inst) EXPECT(g.tiles <= in.cus, "instance %zu has larger windows", k);
        }
    }
    // the too-long test of sblk_try: by ticket, at most eight rounds of the chip
    EXPECT(!sblk_too_long(true, 1 << 20, 256, 1) && !sblk_too_long(false, 8 * 256 * 3, 256, 3) && sblk_too_long(false, 8 * 256 * 3 + 1, 256, 3), "too long");
    EXPECT(all_resident(true, 512, 256, 2) && !all_resident(true, 513, 256, 2) && !all_resident(false, 1, 256, 2) && !all_resident(true, 1, 256, -1), "all_resident");
    return cases;
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 20240u;
    const long random_n = argc > 2 ? std::atol(argv[2]) : 6000;
    std::mt19937 rng(seed);
    long reached[kRoutes] = {0};
    const long routes = test_route(reached);
    const long cuts = test_row_cut();
    long wraps = 0, launches = 0;
    for (uint32_t start : {0u, 0u - 100u, 0u - 5000u, 0x7ffffff0u}) launches += ticket_sequence(rng, start, random_n / 4, &wraps);
    long accepted = 0, refused[8] = {0};
    const long blocks = test_sblk(rng, random_n * 10, &accepted, refused);
    long reasons = 0;
    for (int r = kSblkRows; r <= kSblkStart; ++r) reasons += refused[r] > 0;
    std::printf("failures %d routes %ld routes_reached %d cuts %ld launches %ld wraps %ld blocks %ld accepted %ld refusal_reasons %ld\n", g_failures, routes,
                (int)std::count_if(reached, reached + kRoutes, [](long c) { return c > 0; }), cuts, launches, wraps, blocks, accepted, reasons);
    return g_failures ? 1 : 0;
}
