// temporal_fill_kernel.hip -- video temporal fill for gfx950 (lanpaint_amd/temporal_fill.py): what lies under the mask of a frame is
// borrowed from the nearest frame in which the same piece of background is visible.  include/lanpaint_hip.h (lp_tfill_*) states
// the rule.  The motion of the known pixels is the propagate section's block field, computed by lp_prop_match_batch and
// lp_prop_fill_batch unchanged with the known bits as weights; this file holds what is new.
//
//   known, down  one lane per pixel and frame: known = !(mask >= 0.5) into level 0 of every frame's pyramid, with the initial
//                source (the frame itself, or -1 under the mask) and remaining planes; then one launch per further level, the OR
//                over the propagate section's footprints.  1 + (levels - 1) launches for all frames.
//   carry        one step of one direction.  A block per 32 x 32 tile, a lane per pixel.  The block reads its known bytes
//                first and leaves when all are 1 -- most of a frame.  Else the 6 x 6 block vectors the tile's pixels interpolate
//                between go to LDS; a masked pixel follows its vector into the donor, takes over the donor's origin (implicit under
//                the donor's known pixels, a stored plane under its mask) and, where the pass writes, samples the origin's frame:
//                a gather bound by memory.  The arguments travel by value.
//   carry pair   the checked form's backward step (lp_tfill_carry_pair): the carry, with the forward pass's sample as a second
//                witness.  Where both exist their lumas are compared per 8 x 8 block, two integer sums through LDS, and a block
//                that disagrees is handed back to `remaining`.  The backward sample is gathered wherever it exists.
// Integer arithmetic decides everything but the sample, which is fp32 in a fixed order, every operation rounded on its own
// (__fmul_rn / __fadd_rn: nothing contracts).  No scratch, no atomics.
// Entry points defined here: lp_tfill_known, lp_tfill_carry, lp_tfill_carry_pair.
#include "motion_tile.h"

namespace lp {
namespace {

constexpr int kB = LP_PROP_BLOCK;                                                     // 8
constexpr int kTile = kFieldTile;                                                     // carry: pixels per tile side, 32

// ---- known bits and their pyramids --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lp_tfill_known_kernel(const float* __restrict__ mask, int64_t mask_step, uint8_t* __restrict__ pyr,
                                                             int64_t stride, int64_t plane, int frame0, int32_t* __restrict__ source,
                                                             float* __restrict__ remaining) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= plane) return;
    const int64_t f = blockIdx.y;
    const bool m = mask[f * mask_step + p] >= 0.5f;                                      // a NaN gives 0: known
    pyr[f * stride + p] = m ? 0 : 1;
    if (source) source[f * plane + p] = m ? -1 : frame0 + static_cast<int32_t>(f);
    if (remaining) remaining[f * plane + p] = m ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(256) void lp_tfill_down_kernel(uint8_t* __restrict__ pyr, int64_t stride, int64_t src_off, int64_t dst_off,
                                                            int sh, int sw, int dh, int dw) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= static_cast<int64_t>(dh) * dw) return;
    const int y = static_cast<int>(p / dw), x = static_cast<int>(p - static_cast<int64_t>(y) * dw);
    const uint8_t* src = pyr + static_cast<int64_t>(blockIdx.y) * stride + src_off;
    const int y0 = 2 * y, y1 = min(2 * y + 1, sh - 1), x0 = 2 * x, x1 = min(2 * x + 1, sw - 1);        // 2y <= sh - 1 always
    const uint8_t v = src[static_cast<int64_t>(y0) * sw + x0] | src[static_cast<int64_t>(y0) * sw + x1] |
                      src[static_cast<int64_t>(y1) * sw + x0] | src[static_cast<int64_t>(y1) * sw + x1];
    pyr[static_cast<int64_t>(blockIdx.y) * stride + dst_off + p] = v;
}

// ---- carry --------------------------------------------------------------------------------------------------------------------------
struct carry_args {
    const int32_t* vec;          // [gh, gw, 2]
    const uint8_t* known;        // frame t's bits [H, W]
    const uint8_t* donor_known;
    const int32_t* org_src;      // the donor's state, read under its mask; null: the donor has none there
    const int32_t* pos_src;
    int32_t*       org_dst;      // frame t's state, written under its mask
    int32_t*       pos_dst;
    const float*   images;       // [frames, H, W, C]
    float*         filled;       // frame t's planes
    int32_t*       source;
    float*         remaining;
    int32_t H, W, C, gh, gw, frames, t, donor, reach, nearer;
};

// Stage 3 for the masked pixel p = (y, x), (ly, lx) of its tile: it follows its vector (the propagate section's interpolation, from
// the tile's vectors in s_v) into the donor and takes over the donor's origin, implicit under the donor's known pixels, the stored
// state under its mask.  Writes frame t's state; returns the origin's frame, P its position there, or -1.
__device__ __forceinline__ int carry_origin(const carry_args& a, const int32_t* s_v, int ly, int lx, int y, int x, int64_t p, int& Py, int& Px) {
    int Vy, Vx;
    field_tile_vector(s_v, ly, lx, Vy, Vx);
    const int qy = 16 * y + Vy, qx = 16 * x + Vx;
    int f = -1;
    Py = Px = 0;
    if (qy >= 0 && qy <= 16 * (a.H - 1) && qx >= 0 && qx <= 16 * (a.W - 1)) {
        const int iy = (qy + 8) >> 4, ix = (qx + 8) >> 4;                // <= n - 1: inside the plane
        const int64_t dp = static_cast<int64_t>(iy) * a.W + ix;
        // the donor's byte and its state are asked for together; the state's values count under the donor's mask only
        const uint8_t dk = a.donor_known[dp];
        const int sf = a.org_src ? a.org_src[dp] : -1;
        const int spy = a.org_src ? a.pos_src[dp * 2] : 0, spx = a.org_src ? a.pos_src[dp * 2 + 1] : 0;
        f = dk ? a.donor : sf;
        Py = dk ? 16 * iy : spy;
        Px = dk ? 16 * ix : spx;
        if (f >= 0 && f < a.frames && abs(a.t - f) <= a.reach) {         // f < frames: a state plane this entry wrote holds no other
            Py += qy - 16 * iy;
            Px += qx - 16 * ix;
        } else {
            f = -1;
        }
    }
    a.org_dst[p] = f;
    a.pos_dst[p * 2] = f >= 0 ? Py : 0;
    a.pos_dst[p * 2 + 1] = f >= 0 ? Px : 0;
    return f;
}

// Where frame f is sampled for an origin at P: P clamped to the plane
__device__ __forceinline__ tap_rows origin_taps(const carry_args& a, int f, int Py, int Px) {
    return taps_of(a.images, a.H, a.W, a.C, f, clampi(Py, 0, 16 * (a.H - 1)), clampi(Px, 0, 16 * (a.W - 1)));
}

// One lane per pixel: a masked pixel's work is a chain of dependent reads (known byte, block vectors, the donor's byte and state, the
// taps), so the 1024 pixels of a tile go side by side on 16 waves rather than four after another on 4.
__global__ __launch_bounds__(kTile * kTile) void lp_tfill_carry_kernel(const carry_args a) {
    __shared__ int32_t s_v[kFieldTileBlocks * kFieldTileBlocks * 2];
    const int H = a.H, W = a.W, C = a.C;
    const int ly = threadIdx.x >> 5, lx = threadIdx.x & 31, y = blockIdx.y * kTile + ly, x = blockIdx.x * kTile + lx;
    const int64_t p = static_cast<int64_t>(y) * W + x;
    const bool masked = y < H && x < W && a.known[p] == 0;
    if (__syncthreads_and(!masked)) return;                              // the whole block: nothing under a mask here
    stage_field_tile(s_v, a.vec, a.gh, a.gw);
    __syncthreads();
    if (!masked) return;                                                 // known, or outside the plane
    const int cur = a.nearer ? a.source[p] : -1;                         // what an earlier pass found; read ahead of its use
    int Py, Px;
    const int f = carry_origin(a, s_v, ly, lx, y, x, p, Py, Px);
    if (f < 0) return;
    if (cur >= 0 && abs(a.t - f) >= abs(a.t - cur)) return;              // nearer: a tie stays with what is there
    const tap_rows taps = origin_taps(a, f, Py, Px);
    float* __restrict__ out = a.filled + p * C;
#pragma unroll 1
    for (int c0 = 0; c0 < C; c0 += 4) {
        float v[4];
        sample4(taps, C, c0, v);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < C) out[c0 + k] = v[k];
    }
    a.source[p] = f;
    a.remaining[p] = 0.0f;
}

// ---- carry, checked: the backward step with the forward pass as second witness -------------------------------------------------------
struct pair_args {
    carry_args c;                // nearer is not read: the step is the backward one
    int32_t*   witnesses;        // frame t's plane
    int32_t    agree;
};

// over the 8 lanes of one row of an 8 x 8 block: lane = 32 (ly & 1) + lx, so the xor stays inside the aligned group of 8
__device__ __forceinline__ int sum8(int v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}

// The carry's geometry.  A tile is 4 x 4 aligned blocks of 8 x 8, block b = 4 (ly >> 3) + (lx >> 3); its two sums go through s_nd
// (n in the low byte, D above it: n <= 64, so the arithmetic shift gives D back) and s_r.  No lane leaves between the barriers.
__global__ __launch_bounds__(kTile * kTile) void lp_tfill_carry_pair_kernel(const pair_args g) {
    __shared__ int32_t s_v[kFieldTileBlocks * kFieldTileBlocks * 2];
    __shared__ int32_t s_nd[(kTile / kB) * (kTile / kB)], s_r[(kTile / kB) * (kTile / kB)];
    const carry_args& a = g.c;
    const int H = a.H, W = a.W, C = a.C;
    const int ly = threadIdx.x >> 5, lx = threadIdx.x & 31, y = blockIdx.y * kTile + ly, x = blockIdx.x * kTile + lx;
    const int64_t p = static_cast<int64_t>(y) * W + x;
    const bool inside = y < H && x < W;
    const bool masked = inside && a.known[p] == 0;
    if (threadIdx.x < (kTile / kB) * (kTile / kB)) s_nd[threadIdx.x] = s_r[threadIdx.x] = 0;
    if (__syncthreads_and(!masked)) {                                    // the whole block: nothing under a mask here
        if (inside) g.witnesses[p] = 0;
        return;
    }
    stage_field_tile(s_v, a.vec, a.gh, a.gw);
    __syncthreads();
    // witness B: stage 3 as lp_tfill_carry_kernel has it.  A's frame and the first channels of its sample are asked for up front.
    int f = -1, Py = 0, Px = 0, cur = -1;
    float fa[3] = {0.0f, 0.0f, 0.0f};
    if (masked) {
        cur = a.source[p];
#pragma unroll
        for (int k = 0; k < 3; ++k) fa[k] = k < C ? a.filled[p * C + k] : 0.0f;
        f = carry_origin(a, s_v, ly, lx, y, x, p, Py, Px);
    }
    const bool has_b = f >= 0, both = has_b && cur >= 0;
    tap_rows taps = {};
    float sb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (has_b) {
        taps = origin_taps(a, f, Py, Px);
        sample4(taps, C, 0, sb);
    }
    const int d = both ? luma_of(sb, C) - luma_of(fa, C) : 0;
    const int b = (ly >> 3) * (kTile / kB) + (lx >> 3);
    const int nd_row = sum8(both ? d * 256 + 1 : 0);
    if ((lx & 7) == 0 && nd_row != 0) atomicAdd(&s_nd[b], nd_row);
    __syncthreads();
    const int nd = s_nd[b], n = nd & 255, D = nd >> 8;
    const bool enough = n >= LP_PROP_MIN_PIXELS;
    int mu = 0;
    if (enough) {
        const int num = 2 * D + n, den = 2 * n;
        mu = num / den;
        if (num - mu * den < 0) --mu;                                    // the mathematical floor
        mu = clampi(mu, -LP_PROP_VIS_MAX_BIAS, LP_PROP_VIS_MAX_BIAS);
    }
    const int r_row = sum8(both && enough ? abs(d - mu) : 0);
    if ((lx & 7) == 0 && r_row != 0) atomicAdd(&s_r[b], r_row);
    __syncthreads();
    if (!masked) {                                                       // known, or outside the plane
        if (inside) g.witnesses[p] = 0;
        return;
    }
    const bool disputed = both && enough && s_r[b] > g.agree * n;
    int wit = 0;
    if (disputed) {
        const float* __restrict__ own = a.images + (static_cast<int64_t>(a.t) * H * W + p) * C;
        float* __restrict__ out = a.filled + p * C;
#pragma unroll 1
        for (int c = 0; c < C; ++c) out[c] = own[c];
        a.source[p] = LP_TFILL_DISPUTED;
        a.remaining[p] = 1.0f;
    } else if (has_b && (cur < 0 || abs(a.t - f) < abs(a.t - cur))) {    // nearer: a tie stays with what is there
        float* __restrict__ out = a.filled + p * C;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < C) out[k] = sb[k];
#pragma unroll 1
        for (int c0 = 4; c0 < C; c0 += 4) {
            float v[4];
            sample4(taps, C, c0, v);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + k < C) out[c0 + k] = v[k];
        }
        a.source[p] = f;
        a.remaining[p] = 0.0f;
        wit = both && enough ? 2 : 1;
    } else if (cur >= 0) {
        wit = both && enough ? 2 : 1;
    } else {
        a.remaining[p] = 1.0f;
    }
    g.witnesses[p] = wit;
}

// The checks both carry entries share, and the kernel's arguments; `extra` is the checked form's sixth output (null: the plain form)
int carry_args_of(const lp_tfill_carry_desc& d, const void* extra, carry_args& a) {
    if (d.frames < 2 || !side_ok(d.height) || !side_ok(d.width) || d.channels < 1 || d.channels > LP_DETAIL_MAX_CHANNELS) return LP_E_INVALID;
    if (d.reach < 0 || d.reach > LP_TFILL_MAX_REACH || (d.nearer != 0 && d.nearer != 1)) return LP_E_INVALID;
    if (d.frames > 65535) return LP_E_UNSUPPORTED;
    if (d.frame < 0 || d.frame >= d.frames || d.donor < 0 || d.donor >= d.frames || (d.donor != d.frame - 1 && d.donor != d.frame + 1))
        return LP_E_INVALID;
    if (!d.vec || !d.known || !d.donor_known || !d.org_dst || !d.pos_dst || !d.images || !d.filled || !d.source || !d.remaining)
        return LP_E_INVALID;
    if ((d.org_src == nullptr) != (d.pos_src == nullptr)) return LP_E_INVALID;
    const void *outs[6] = {d.org_dst, d.pos_dst, d.filled, d.source, d.remaining, extra};
    const void *in[6] = {d.vec, d.known, d.donor_known, d.org_src, d.pos_src, d.images};
    for (int k = 0; k < 6; ++k) {
        if (!outs[k]) continue;                                          // `extra` of the plain form
        for (const void* p : in)
            if (outs[k] == p) return LP_E_INVALID;
        for (int m = k + 1; m < 6; ++m)
            if (outs[k] == outs[m]) return LP_E_INVALID;
    }
    const int64_t plane = static_cast<int64_t>(d.height) * d.width;
    a.vec = d.vec;
    a.known = d.known;
    a.donor_known = d.donor_known;
    a.org_src = d.org_src;
    a.pos_src = d.pos_src;
    a.org_dst = d.org_dst;
    a.pos_dst = d.pos_dst;
    a.images = d.images;
    a.filled = d.filled + d.frame * plane * d.channels;
    a.source = d.source + d.frame * plane;
    a.remaining = d.remaining + d.frame * plane;
    a.H = d.height;
    a.W = d.width;
    a.C = d.channels;
    a.gh = (d.height + kB - 1) / kB;
    a.gw = (d.width + kB - 1) / kB;
    a.frames = d.frames;
    a.t = d.frame;
    a.donor = d.donor;
    a.reach = d.reach ? d.reach : LP_TFILL_MAX_REACH;                    // 0: the whole clip; frames <= 65535, so no age exceeds it
    a.nearer = d.nearer;
    return LP_OK;
}

}  // namespace

extern "C" int lp_tfill_known(const lp_tfill_known_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_tfill_known_desc& d = *dp;
    if (d.frames <= 0 || !side_ok(d.height) || !side_ok(d.width) || !levels_ok(d.levels)) return LP_E_INVALID;
    if ((d.mask_frames != 1 && d.mask_frames != d.frames) || d.frame0 < 0) return LP_E_INVALID;
    if (!d.mask || !d.pyramid) return LP_E_INVALID;
    const void *in = d.mask, *outs[3] = {d.pyramid, d.source, d.remaining};
    for (int k = 0; k < 3; ++k) {                                        // source and remaining may be null; given, nothing aliases
        if (!outs[k]) continue;
        if (outs[k] == in) return LP_E_INVALID;
        for (int m = k + 1; m < 3; ++m)
            if (outs[k] == outs[m]) return LP_E_INVALID;
    }
    if (d.frames > 65535 || d.frame0 > 65535 - d.frames) return LP_E_UNSUPPORTED;
    const int64_t plane = static_cast<int64_t>(d.height) * d.width, stride = level_offset(d.height, d.width, d.levels);
    hipLaunchKernelGGL(lp_tfill_known_kernel, dim3(blocks_of(plane, 256), d.frames), dim3(256), 0, stream, d.mask,
                       d.mask_frames == 1 ? int64_t{0} : plane, d.pyramid, stride, plane, d.frame0, d.source, d.remaining);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    for (int l = 1; l < d.levels; ++l) {
        const int sh = level_side(d.height, l - 1), sw = level_side(d.width, l - 1), dh = level_side(d.height, l), dw = level_side(d.width, l);
        hipLaunchKernelGGL(lp_tfill_down_kernel, dim3(blocks_of(static_cast<int64_t>(dh) * dw, 256), d.frames), dim3(256), 0, stream,
                           d.pyramid, stride, level_offset(d.height, d.width, l - 1), level_offset(d.height, d.width, l), sh, sw, dh, dw);
        if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    }
    return LP_OK;
}

extern "C" int lp_tfill_carry(const lp_tfill_carry_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    carry_args a = {};
    const int status = carry_args_of(*dp, nullptr, a);
    if (status != LP_OK) return status;
    hipLaunchKernelGGL(lp_tfill_carry_kernel, dim3(blocks_of(dp->width, kTile), blocks_of(dp->height, kTile)), dim3(kTile * kTile), 0, stream, a);
    return launched();
}

extern "C" int lp_tfill_carry_pair(const lp_tfill_carry_pair_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    if (dp->agree < 1 || dp->agree > 255) return LP_E_INVALID;
    const lp_tfill_carry_desc d = {dp->frames, dp->height, dp->width, dp->channels, dp->frame, dp->donor, dp->reach, 1,
                                   dp->vec, dp->known, dp->donor_known, dp->org_src, dp->pos_src, dp->org_dst, dp->pos_dst,
                                   dp->images, dp->filled, dp->source, dp->remaining};
    pair_args g = {};
    const int status = carry_args_of(d, dp->witnesses, g.c);
    if (status != LP_OK) return status;
    if (!dp->witnesses || d.donor != d.frame + 1) return LP_E_INVALID;   // the step is the backward one
    g.witnesses = dp->witnesses + d.frame * (static_cast<int64_t>(d.height) * d.width);
    g.agree = dp->agree;
    hipLaunchKernelGGL(lp_tfill_carry_pair_kernel, dim3(blocks_of(d.width, kTile), blocks_of(d.height, kTile)), dim3(kTile * kTile), 0, stream, g);
    return launched();
}

}  // namespace lp
