// motion_tile.h -- what the motion family's kernels share: propagate_kernel.hip, temporal_fill_kernel.hip, temporal_smooth_kernel.hip
// and shot_kernel.hip.  include/lanpaint_hip.h states every rule once; this header is the one place under csrc/ that spells it.
//
//   codes      luma_of: Y = (77 c0 + 150 c1 + 29 c2 + 128) >> 8 of the 8-bit codes (code_of, lp_common.h) of a pixel's first three
//              channels, channel 0's code alone with fewer than three (lp_prop_luma, the checked fill, the robust smooth).
//   field      the per-pixel vector from the block field [gh, gw, 2] of 8 x 8 blocks: for pixel y, u = 2 y - 7 counts sixteenths of
//              a block from the centre of block 0, so block u >> 4 and its successor, both clamped to the grid, are interpolated with
//              the fraction u & 15, V = (bil + 128) >> 8 per component.  field_tap_of is the index rule, bil_sum / field_vector the
//              arithmetic; the loads stay with the caller: global pointers (lp_prop_advance), flags (weight_of: lp_prop_occlude,
//              lp_prop_merge_visible), int2 loads (the smooth kernels' step) or the LDS tile below.
//   field tile the 6 x 6 block vectors a 32 x 32 tile's pixels interpolate between, staged in LDS by the block's first 36 lanes and
//              read back per pixel (lp_tfill_carry, lp_tfill_carry_pair).
//   sample     the fp32 bilinear sample of a frame at a position in sixteenths of a pixel inside the plane, four channels at a time:
//              (16 - g) a + g b per axis, every product and sum rounded on its own, a tap with weight 0 not read, the result
//              times 1 / 256 (both fill kernels, both smooth kernels).
//   pyramid    level_side / level_offset: the layout of the byte pyramids lp_prop_pyramid_ws_bytes sizes (the propagate and the
//              temporal fill's known bits), for host and device.
//   host       the descriptor checks and launch helpers of the four files' dispatches.
// Integer arithmetic but for the sample, which never contracts (__fmul_rn / __fadd_rn).  Nothing here is indexed by a register.
#pragma once
#include "lp_common.h"

namespace lp {

static_assert(LP_PROP_BLOCK == 8, "u = 2 y - 7 and the shift by 4 are the rule for blocks of 8 pixels");

constexpr int kFieldTile = 32;                                                        // pixels per side of a staged tile
constexpr int kFieldTileBlocks = kFieldTile / LP_PROP_BLOCK + 2;                      // 6: the block centres a tile interpolates between

static_assert(kFieldTile % (2 * LP_PROP_BLOCK) == 0, "a tile starts on an even block, so its first pixel's lower block is 4 ty - 1");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ void cmpswap(int& a, int& b) {
    const int lo = min(a, b), hi = max(a, b);
    a = lo; b = hi;
}

// ---- codes ----------------------------------------------------------------------------------------------------------------------------
// The 8-bit luma of the pixel whose channels start at px; px[1] and px[2] are read with three channels or more only
__device__ __forceinline__ int luma_of(const float* px, int C) {
    const int y = code_of(px[0]);
    return C >= 3 ? (77 * y + 150 * code_of(px[1]) + 29 * code_of(px[2]) + 128) >> 8 : y;
}

// ---- the block field --------------------------------------------------------------------------------------------------------------------
// Where pixel y lies between the block centres: the lower block (-1 in front of block 0's centre: >> floors) and the fraction
struct field_at { int b, f; };
__device__ __forceinline__ field_at field_at_of(int y) {
    const int u = 2 * y - 7;
    return {u >> 4, u & 15};
}

// The index rule: the two blocks of a grid of g, clamped, and the fraction
struct field_tap { int b0, b1, f; };
__device__ __forceinline__ field_tap field_tap_of(int y, int g) {
    const field_at a = field_at_of(y);
    return {clampi(a.b, 0, g - 1), clampi(a.b + 1, 0, g - 1), a.f};
}

// 256 times the bilinear mean of four values, fractions in sixteenths
__device__ __forceinline__ int bil_sum(int a00, int a01, int a10, int a11, int fy, int fx) {
    return (16 - fy) * ((16 - fx) * a00 + fx * a01) + fy * ((16 - fx) * a10 + fx * a11);
}

// one component of the per-pixel vector from the four blocks' components
__device__ __forceinline__ int field_vector(int v00, int v01, int v10, int v11, int fy, int fx) {
    return (bil_sum(v00, v01, v10, v11, fy, fx) + 128) >> 8;
}

// ---- the field of one tile in LDS -----------------------------------------------------------------------------------------------------
// The block vectors around tile (blockIdx.y, blockIdx.x) into s_v[6 * 6 * 2]: row j is block clamp(4 ty - 1 + j).  The caller
// synchronises before field_tile_vector.
__device__ __forceinline__ void stage_field_tile(int32_t* s_v, const int32_t* __restrict__ vec, int gh, int gw) {
    if (threadIdx.x < kFieldTileBlocks * kFieldTileBlocks) {
        const int j = threadIdx.x / kFieldTileBlocks, i = threadIdx.x - j * kFieldTileBlocks;
        const int by = clampi(static_cast<int>(blockIdx.y) * (kFieldTile / LP_PROP_BLOCK) - 1 + j, 0, gh - 1);
        const int bx = clampi(static_cast<int>(blockIdx.x) * (kFieldTile / LP_PROP_BLOCK) - 1 + i, 0, gw - 1);
        const int32_t* v = vec + (static_cast<int64_t>(by) * gw + bx) * 2;
        s_v[threadIdx.x * 2] = v[0];
        s_v[threadIdx.x * 2 + 1] = v[1];
    }
}

// The vector of the tile's pixel (ly, lx).  A tile starts on a multiple of 32 pixels, so the index rule on the local coordinate
// gives the block counted from 4 ty: -1 .. 3, row b + 1 of s_v, which holds the clamp already.
__device__ __forceinline__ void field_tile_vector(const int32_t* s_v, int ly, int lx, int& Vy, int& Vx) {
    const field_at ay = field_at_of(ly), ax = field_at_of(lx);
    const int32_t *v00 = s_v + ((ay.b + 1) * kFieldTileBlocks + ax.b + 1) * 2, *v01 = v00 + 2, *v10 = v00 + kFieldTileBlocks * 2, *v11 = v10 + 2;
    Vy = field_vector(v00[0], v01[0], v10[0], v11[0], ay.f, ax.f);
    Vx = field_vector(v00[1], v01[1], v10[1], v11[1], ay.f, ax.f);
}

// ---- the sample ---------------------------------------------------------------------------------------------------------------------------
// (16 - f) a + f b, or 16 a without reading b's weight into it: the products and the sum rounded on their own
__device__ __forceinline__ float lerp16(float a, float b, int f) {
    if (f == 0) return __fmul_rn(16.0f, a);
    return __fadd_rn(__fmul_rn(static_cast<float>(16 - f), a), __fmul_rn(static_cast<float>(f), b));
}

// Where a frame is sampled: its two rows of taps
struct tap_rows {
    const float* r0;
    const float* r1;
    int nx, gy, gx;
};

// Frame f of images [frames, H, W, C] at q, which lies inside the plane: gy != 0 puts row qy / 16 + 1 inside it, as gx does the
// next column.  A caller whose position may leave the plane clamps it first.
__device__ __forceinline__ tap_rows taps_of(const float* __restrict__ images, int H, int W, int C, int f, int qy, int qx) {
    tap_rows t;
    t.gy = qy & 15;
    t.gx = qx & 15;
    t.r0 = images + ((static_cast<int64_t>(f) * H + (qy >> 4)) * W + (qx >> 4)) * C;
    t.r1 = t.r0 + (t.gy ? static_cast<int64_t>(W) * C : 0);
    t.nx = t.gx ? C : 0;
    return t;
}

// channels c0 .. c0 + 3 of the sample (0 beyond C): the four channels' taps are asked for before the first is used
__device__ __forceinline__ void sample4(const tap_rows& t, int C, int c0, float (&v)[4]) {
    float t00[4], t01[4], t10[4], t11[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool in = c0 + k < C;
        t00[k] = in ? t.r0[c0 + k] : 0.0f;
        t01[k] = in && t.gx ? t.r0[t.nx + c0 + k] : 0.0f;
        t10[k] = in && t.gy ? t.r1[c0 + k] : 0.0f;
        t11[k] = in && t.gy && t.gx ? t.r1[t.nx + c0 + k] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float top = lerp16(t00[k], t01[k], t.gx);
        const float s = t.gy == 0 ? __fmul_rn(16.0f, top)
                                  : __fadd_rn(__fmul_rn(static_cast<float>(16 - t.gy), top), __fmul_rn(static_cast<float>(t.gy), lerp16(t10[k], t11[k], t.gx)));
        v[k] = __fmul_rn(s, 1.0f / 256.0f);
    }
}

// ---- the byte pyramids' layout --------------------------------------------------------------------------------------------------------
__host__ __device__ inline int level_side(int n, int l) { return (n + (1 << l) - 1) >> l; }
__host__ __device__ inline int64_t level_offset(int h, int w, int l) {               // with l = levels: a frame's bytes
    int64_t off = 0;
    for (int k = 0; k < l; ++k) {
        const int64_t n = static_cast<int64_t>(level_side(h, k)) * level_side(w, k);
        off += (n + LP_PROP_ALIGN - 1) / LP_PROP_ALIGN * LP_PROP_ALIGN;
    }
    return off;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
inline bool side_ok(int s) { return s > 0 && s <= LP_VMASK_MAX_SIDE; }              // the video limit
inline bool levels_ok(int l) { return l >= 1 && l <= LP_PROP_MAX_LEVELS; }
inline int launched() { return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH; }
inline uint32_t blocks_of(int64_t n, int per) { return static_cast<uint32_t>((n + per - 1) / per); }

}  // namespace lp
