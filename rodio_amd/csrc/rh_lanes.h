// rh_lanes.h -- the lane-level primitives every wave64 kernel of the library is written in: the explicit FMA, cross-lane moves on the VALU data
// path (DPP) with their control words, v_readlane of a float, the 2x2 product.  gfx950 only.  No namespace of its own: rh_pipeline_dev.h and
// rh_scan_common.h include it where their own helpers live, inside the unnamed namespace of the unit.
#pragma once

// (-ffp-contract=off: a kernel that wants an FMA says so)
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// y += M * x for a row-major 2x2 (M: a pointer to four floats in any address space -- registers, or an argument block read from the constant one)
template <class MP>
__device__ __forceinline__ void mat_acc(MP M, float x1, float x2, float &y1, float &y2) {
    y1 = fma_(M[0], x1, fma_(M[1], x2, y1));
    y2 = fma_(M[2], x1, fma_(M[3], x2, y2));
}

// Cross-lane moves on the VALU data path (DPP), no LDS round trip.  Lanes whose source is out of
// range, or whose row is masked off, read 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp0(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true));
}
// v_readlane / v_readfirstlane of a float (the builtins take int: pass the bits, not the value)
__device__ __forceinline__ float readlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ float readfirstlane_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
constexpr int kDppRowShr = 0x110;    // row_shr:n  = 0x110 + n
constexpr int kDppWaveShr1 = 0x138;  // wave_shr:1
constexpr int kDppBcast15 = 0x142;   // lane 15 of each row -> the next row
constexpr int kDppBcast31 = 0x143;   // lane 31 -> rows 2 and 3
