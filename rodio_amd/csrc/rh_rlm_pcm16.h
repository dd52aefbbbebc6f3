// rh_rlm_pcm16.h -- sources set as 16-bit PCM (rh_rlm_set_sources_pcm16): does a one-shot run read the PCM16 rows themselves (k_rlm_chunk_pcm16,
// k_mix_rows_pcm16) or a converted f32 copy of them?  A plain function over integers, beside rh_rlm_launch.h: no HIP and no handle, the caller
// (rlm_launch, rh_pipeline.hip) fills the inputs, and tests/cpp/pcm16_launch_test.cpp runs it without a GPU.  Both answers give the same bits:
// the copy is what rh_convert_i16_to_f32 makes of the rows, and float(s) / 32768 is exact.
#pragma once
#include "rh_rlm_launch.h"

namespace rh {
namespace rlm {

enum Pcm16No {
    kPcmNative,   // the kernels read the int16 rows
    kPcmFilters,  // a handle with a filter per source (rh_rlm_set_filters): its classes run on rows of their own
    kPcmSubset,   // rh_rlm_run_subset over a part of the batch
    kPcmRoute,    // a route without a native kernel: kPair, kMixedFiltered, kPlain, kBatch
    kPcmRing,     // kMixed whose row_cut picks k_mix_ring
    kPcmRows,     // kChunk: rows that are no whole 16-byte vectors of int16 (frames * channels % 8 != 0)
    kPcmAlign,    // rows off the boundary the kernel's loads need: 16 bytes (k_rlm_chunk_pcm16's LDS-DMA), 8 bytes (k_mix_rows_pcm16's loads)
    kPcmReasons
};
constexpr uint64_t kPcmChunkAlign = 16, kPcmRowsAlign = 8;  // bytes
struct Pcm16In {
    Route route;         // of the run (rh::rlm::route)
    int ring;            // row_cut().ring of the run (kMixed; ignored elsewhere)
    uint32_t channels;
    uint64_t frames;     // the sources' common length (the native routes are those of equal-length batches)
    uint64_t addr_bits;  // the OR of the rows' addresses: a low bit that is set is set in some row
    bool filters;        // the handle has per-source filters
    bool subset;         // the run covers a part of the sources
};
inline Pcm16No pcm16_native(const Pcm16In &in) {
    if (in.filters) return kPcmFilters;
    if (in.subset) return kPcmSubset;
    if (in.route == kChunk) {
        if ((in.frames * in.channels) % 8 != 0) return kPcmRows;
        return (in.addr_bits & (kPcmChunkAlign - 1)) ? kPcmAlign : kPcmNative;
    }
    if (in.route == kMixed) {
        if (in.ring != 0) return kPcmRing;
        return (in.addr_bits & (kPcmRowsAlign - 1)) ? kPcmAlign : kPcmNative;
    }
    return kPcmRoute;
}

}  // namespace rlm
}  // namespace rh
