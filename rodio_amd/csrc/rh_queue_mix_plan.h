// rh_queue_mix_plan.h -- what rh_queue_mix_block (rh_queuemix.hip) decides on the host, as plain functions over the caller's arrays: the
// converter chains of a queue of sounds (walk_chains), the cursor behind a block (queue_advance), the status of a call, the two flat tables
// the kernel reads -- chain SEGMENTS and PIECES --, and where an output frame's taps lie (locate() and find_piece(): the functions the kernel
// and the tests share).  No HIP: tests/cpp/queue_mix_plan_test.cpp runs it without a GPU.  Taking the tables to the device and launching
// are rh_queue_mix_block's.  The kernel knows nothing of queues: a plain source is one segment of one piece.
//
// The chain rule (include/rodio_hip.h has the Rust lines).  The STREAM of a queue is its sounds' samples back to back.  A CHAIN is what one
// converter of UniformSourceIterator takes: one that starts at stream position p inside sound k takes min(samples_k, 32768) samples of the
// stream from p on, whatever sounds they come from, and reads them as frames of channels_k at rate_k; n input frames in, span_out(n) output
// frames out, output frame j of it reading frames i = floor(j F / T) and i + 1 of the chain, the frame with i == n - 1 verbatim.  Where the
// sounds run out inside a chain: with keep_alive the chain goes on to its full count over +0.0 samples (no gain touches them) and the queue
// is SILENT behind it; without, the chain ends with the sounds and the queue has ENDED.  Either way it adds nothing behind.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/rodio_hip.h"
#include "rh_mix_plan.h"

namespace rh {
namespace queuemix {

using mixplan::Div;
using mixplan::div_u32;
using mixplan::kChainSamples;
using mixplan::make_div;
using mixplan::span_out;

enum : uint64_t { kPlaying = 0, kSilent = 1, kEnded = 2 };

// The words of a queue.
struct Cursor {
    uint64_t chain_start, chain_out, state, flags;
};
inline Cursor cursor_of(const uint64_t *w) { return Cursor{w[0], w[1], w[2], w[3]}; }

inline rh_status queue_plan(uint64_t *words, uint32_t keep_alive) {
    if (!words || keep_alive > 1) return RH_ERR_INVALID;
    words[0] = 0, words[1] = 0, words[2] = kPlaying, words[3] = keep_alive;
    return RH_OK;
}

// A sound of a queue, and the sounds of one as the caller's arrays hold them: RH_QUEUE_SOUND_WORDS words {data, samples, channels, rate} and a
// gain each (no gains: 1).
struct Sound {
    const float *data;
    uint64_t samples, channels, rate;
    float gain;
};
struct Sounds {
    const uint64_t *w;
    const float *g;
    Sound operator[](uint32_t k) const {
        const uint64_t *x = w + (size_t)RH_QUEUE_SOUND_WORDS * k;
        return Sound{reinterpret_cast<const float *>(static_cast<uintptr_t>(x[0])), x[1], x[2], x[3], g ? g[k] : 1.0f};
    }
    Sounds from(uint64_t at) const { return Sounds{w ? w + (size_t)RH_QUEUE_SOUND_WORDS * at : nullptr, g ? g + at : nullptr}; }
};

// A run of a chain's samples that lies in one sound (sound < n_sounds), or the +0.0 samples a keep-alive chain lacks (sound == n_sounds).
struct Run {
    uint32_t sound;
    uint64_t off;    // the run's first sample inside the sound
    uint32_t start;  // ... inside the chain
    uint32_t count;
};
// One converter chain.
struct Chain {
    uint32_t k;         // the sound it starts in
    uint64_t off;       // ... at this sample
    uint32_t ch, rate;  // that sound's: the format the chain reads the stream in
    uint32_t n;         // samples it takes, the +0.0 ones included
    uint32_t k_next;    // where the stream stands behind it: the sound (n_sounds: the sounds have run out) and the sample
    uint64_t off_next;
};

// The first sound from (k, off) on that still has a sample (queue.rs:255-290: a sound that is exhausted is left at once).
inline void settle(const Sounds &s, uint32_t n, uint32_t *k, uint64_t *off) {
    while (*k < n && *off >= s[*k].samples) ++*k, *off = 0;
}

// The chain that starts at (k, off), a settled position with k < n_sounds.  run(const Run &) receives its runs in order.
template <class OnRun>
inline Chain chain_at(const Sounds &s, uint32_t n_sounds, uint32_t k, uint64_t off, bool keep_alive, OnRun &&run) {
    Chain c;
    c.k = k, c.off = off, c.ch = (uint32_t)s[k].channels, c.rate = (uint32_t)s[k].rate;
    const uint32_t want = (uint32_t)(s[k].samples < kChainSamples ? s[k].samples : kChainSamples);  // uniform.rs:56 over buffer.rs:76-82: the WHOLE length
    uint32_t have = 0;
    while (have < want && k < n_sounds) {
        const uint64_t left = s[k].samples - off;
        const uint32_t take = (uint32_t)(left < want - have ? left : want - have);
        if (take) run(Run{k, off, have, take});
        have += take, off += take;
        settle(s, n_sounds, &k, &off);
    }
    if (have < want && keep_alive) {  // queue.rs:218-241: Take draws the rest from the queue's injected silence
        run(Run{n_sounds, 0, have, want - have});
        have = want;
    }
    c.n = have, c.k_next = k, c.off_next = off;
    return c;
}

// What a chain is to a mix at to_rate; anything but RH_OK: the queue stays on the host path.
struct Conv {
    uint32_t F, T;
    uint32_t frames;  // input frames
    uint64_t M;       // output frames
};
inline rh_status convert(const Chain &c, uint32_t to_rate, Conv *v) {
    mixplan::reduce(c.rate, to_rate, &v->F, &v->T);
    if ((uint64_t)v->F * v->T > 0xffffffffull) return RH_ERR_UNSUPPORTED;  // the reference multiplies in u32 (sample_rate.rs:157,173)
    if (c.n % c.ch) return RH_ERR_UNSUPPORTED;                             // a chain that cuts a frame
    v->frames = c.n / c.ch;
    v->M = span_out(v->frames, v->F, v->T);
    if (v->M * v->F > 0xffffffffull) return RH_ERR_UNSUPPORTED;  // j F of every output frame of the chain stays inside 32 bits (M <= 2^15 T + 1: no overflow here)
    return RH_OK;
}

// What every sound and the cursor must satisfy whatever the block is (need_data: the call reads the sounds; the cursor's arithmetic does not).
inline rh_status check_queue(const Sounds &s, uint32_t n_sounds, const Cursor &c, bool need_data) {
    if (n_sounds && !s.w) return RH_ERR_INVALID;
    if (c.state > kEnded || c.flags > 1) return RH_ERR_INVALID;
    for (uint32_t k = 0; k < n_sounds; ++k)
        if ((need_data && s[k].samples && !s[k].data) || s[k].channels == 0 || s[k].rate == 0 || s[k].channels > 0xffffffffull || s[k].rate > 0xffffffffull) return RH_ERR_INVALID;
    if (c.state != kPlaying) return c.chain_start || c.chain_out ? RH_ERR_INVALID : RH_OK;
    if (c.chain_start && (n_sounds == 0 || c.chain_start >= s[0].samples)) return RH_ERR_INVALID;
    return RH_OK;
}

struct Scratch {  // (the runs of the chain in hand: a caller keeps it, so that a warmed walk allocates nothing)
    std::vector<Run> runs;
};
// The chains of `frames` output frames from the cursor on: seg(chain, conv, first output frame, count, frames of the chain emitted earlier,
// its runs) for each, in order.  *end receives the cursor behind the frames and *dropped the sounds in front of the chain then in progress.
template <class OnSeg>
inline rh_status walk_chains(const Sounds &s, uint32_t n_sounds, const Cursor &cur, uint32_t to_rate, uint64_t frames, bool need_data, Scratch *scr, Cursor *end, uint32_t *dropped, OnSeg &&seg) {
    rh_status st = check_queue(s, n_sounds, cur, need_data);
    if (st != RH_OK) return st;
    if (to_rate == 0) return RH_ERR_INVALID;
    const bool keep = cur.flags & 1;
    Cursor e = cur;
    uint32_t k = 0;
    uint64_t off = cur.chain_start, m = 0;
    if (e.state == kPlaying) settle(s, n_sounds, &k, &off);
    while (e.state == kPlaying) {
        if (k == n_sounds) {  // the sounds ran out on a chain boundary (queue.rs:233-240)
            if (e.chain_out) return RH_ERR_INVALID;
            e.state = keep ? kSilent : kEnded;
            break;
        }
        if (m == frames) break;
        scr->runs.clear();
        const Chain c = chain_at(s, n_sounds, k, off, keep, [&](const Run &r) { scr->runs.push_back(r); });
        Conv v;
        if ((st = convert(c, to_rate, &v)) != RH_OK) return st;
        if (e.chain_out >= v.M) return RH_ERR_INVALID;  // (only the cursor's own can be)
        const uint64_t cnt = v.M - e.chain_out < frames - m ? v.M - e.chain_out : frames - m;
        seg(c, v, m, cnt, e.chain_out, static_cast<const std::vector<Run> &>(scr->runs));
        m += cnt;
        if (e.chain_out + cnt < v.M) {  // the frames end inside the chain
            e.chain_out += cnt;
            break;
        }
        e.chain_out = 0;
        k = c.k_next, off = c.off_next;
    }
    if (e.state == kPlaying) {
        *dropped = k, e.chain_start = off;
    } else {
        *dropped = n_sounds, e.chain_start = 0, e.chain_out = 0;
    }
    *end = e;
    return RH_OK;
}

inline rh_status queue_advance(uint64_t *words, const uint64_t *sounds, uint32_t n_sounds, uint32_t to_rate, uint64_t out_frames, uint32_t *dropped) {
    if (!words || !dropped) return RH_ERR_INVALID;
    const Sounds s{sounds, nullptr};
    Scratch scr;
    Cursor end;
    uint32_t d = 0;
    const rh_status st = walk_chains(s, n_sounds, cursor_of(words), to_rate, out_frames, false, &scr, &end, &d, [](const Chain &, const Conv &, uint64_t, uint64_t, uint64_t, const std::vector<Run> &) {});
    if (st != RH_OK) return st;
    words[0] = end.chain_start, words[1] = end.chain_out, words[2] = end.state, words[3] = end.flags;
    *dropped = d;
    return RH_OK;
}

// ---- the kernel's tables --------------------------------------------------------------------------------------------------------------------
// Output frames [m0, m0 + count) of the block: a run of ONE converter chain (a plain source: the whole source).
struct Seg {
    uint32_t m0, count;
    uint32_t prior;        // output frames of the chain in front of m0 (plain: 0)
    uint32_t ch;           // channels the chain reads its samples in
    uint32_t F, T;         // reduced rates
    float Tf;              // T as a float; 0: the converter passes through (F == T)
    uint32_t r0;           // plain sources: the block's phase; chains: 0 (every chain starts a converter)
    uint32_t nl;           // the chain's last input frame: verbatim (plain: `last`)
    uint32_t piece_first;  // its pieces in the piece table
    uint32_t piece_count;
    Div dT;
    uint32_t pad[3];
};
static_assert(sizeof(Seg) == 64, "a segment is one cache line");
// Samples [start, the next piece's start) of a chain.
struct Piece {
    const float *data;  // the sample at `start`; NULL: +0.0, whatever the gain
    uint32_t start;
    float gain;
};
static_assert(sizeof(Piece) == 16, "");
// The segments of a source, in the order of their frames; count == 0: it reaches no frame.
struct Src {
    uint32_t seg_first, seg_count;
};

struct Taps {
    uint32_t i;    // the frame of the first tap inside the chain (the second is i + 1, read only where lerp is set)
    bool lerp;     // false: frame i verbatim (the chain's last frame, F == T)
    uint32_t num;  // (position) mod T: the lerp's weight over T
};
// Output frame m (m0 <= m < m0 + count) of a segment.  Every intermediate fits 32 bits for a call check() has passed.
RH_MIX_HD Taps locate(const Seg &g, uint32_t m) {
    const uint32_t j = g.prior + (m - g.m0);
    const uint32_t pos = g.r0 + j * g.F;
    Taps t;
    t.i = div_u32(pos, g.dT);
    t.num = pos - t.i * g.T;
    t.lerp = g.Tf != 0.0f && t.i < g.nl;
    return t;
}
// The segment of `n` that holds output frame m, or n where none does (segments are in order and do not overlap).
RH_MIX_HD uint32_t find_seg(const Seg *g, uint32_t n, uint32_t m) {
    uint32_t lo = 0, hi = n;  // the first segment that ends behind m
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (g[mid].m0 + g[mid].count <= m) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && g[lo].m0 <= m ? lo : n;
}
// The piece of `n` (n >= 1, the first one's start is 0) that holds sample e of the chain: the last one with start <= e.
RH_MIX_HD uint32_t find_piece(const Piece *p, uint32_t n, uint64_t e) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p[mid].start <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct Plan {
    std::vector<Src> srcs;
    std::vector<Seg> segs;
    std::vector<Piece> pieces;
    Scratch scr;
};

// The status of a call and its tables (anything but RH_OK: nothing may be launched).  out_frames == 0 is answered by the caller.
inline rh_status plan(const float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames, const rh_wide_src *srcs, uint32_t n_sources, const uint64_t *sounds,
                      const float *gains, const uint32_t *counts, const uint64_t *cursors, Plan *p) {
    p->srcs.clear(), p->segs.clear(), p->pieces.clear();
    if (!dst || channels == 0 || to_rate == 0 || (n_sources && (!srcs || !counts))) return RH_ERR_INVALID;
    if (out_frames > 0x7fffffffull) return RH_ERR_UNSUPPORTED;
    uint64_t at = 0;  // the source's first sound
    for (uint32_t s = 0; s < n_sources; ++s) {
        const rh_wide_src &x = srcs[s];
        const uint32_t n_sounds = counts[s];
        const Sounds q = Sounds{sounds, gains}.from(at);
        at += n_sounds;
        Src d{(uint32_t)p->segs.size(), 0u};
        if (n_sounds == 0) {  // rh_wide_mix_block's source
            if (x.frames) {
                mixplan::Reach r;
                const rh_status st = mixplan::check_src(x, channels, to_rate, out_frames, &r);
                if (st != RH_OK) return st;
                p->segs.push_back(Seg{0u, (uint32_t)x.frames, 0u, x.channels, r.F, r.T, r.F == r.T ? 0.0f : (float)r.T, x.phase, x.last, (uint32_t)p->pieces.size(), 1u, make_div(r.T), {0u, 0u, 0u}});
                p->pieces.push_back(Piece{x.data, 0u, x.gain});
            }
        } else if (x.frames) {  // (a queue that reaches no frame is not looked at either)
            if (!q.w || !cursors || x.frames > out_frames) return RH_ERR_INVALID;
            Cursor end;
            uint32_t dropped;
            const rh_status st = walk_chains(q, n_sounds, cursor_of(cursors + (size_t)RH_QUEUE_WORDS * s), to_rate, x.frames, true, &p->scr, &end, &dropped,
                                             [&](const Chain &c, const Conv &v, uint64_t m0, uint64_t cnt, uint64_t prior, const std::vector<Run> &runs) {
                                                 p->segs.push_back(Seg{(uint32_t)m0, (uint32_t)cnt, (uint32_t)prior, c.ch, v.F, v.T, v.F == v.T ? 0.0f : (float)v.T, 0u, v.frames - 1u,
                                                                       (uint32_t)p->pieces.size(), (uint32_t)runs.size(), make_div(v.T), {0u, 0u, 0u}});
                                                 for (const Run &r : runs) p->pieces.push_back(r.sound < n_sounds ? Piece{q[r.sound].data + r.off, r.start, q[r.sound].gain} : Piece{nullptr, r.start, 0.0f});
                                             });
            if (st != RH_OK) return st;
        }
        d.seg_count = (uint32_t)p->segs.size() - d.seg_first;
        p->srcs.push_back(d);
    }
    return RH_OK;
}

}  // namespace queuemix
}  // namespace rh
