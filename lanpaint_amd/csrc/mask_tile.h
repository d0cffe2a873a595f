// mask_tile.h -- the smoothed mask of one TH x TW tile in LDS, shared by lp_mask_blend (blend_kernel.hip) and
// lp_detail_stitch (detail_kernel.hip):  m = conv2d(max_pool2d(mask, k, 1, k/2), gaussian_kernel_2d(k), pad k/2).
//
// The mask tile plus a 2R halo (R = k/2: R for the dilation, R for the blur) is staged once; separable passes run in LDS
//   A (raw, -inf outside the image)  --row max-->  B  --col max, 0 outside the image-->  C  --row blur-->  D
// and the caller finishes with the column blur, m(ty, tx) = smoothed_mask_at(D, g, k, ty, tx).  The reference's 2-D kernel
// exp(-(x^2+y^2)/(2 s^2))/sum is exactly the outer product of the normalised 1-D profile, so the separable form differs from
// conv2d only in summation order.  (y0, x0) is the tile's origin in IMAGE coordinates, so padding applies at the image
// border wherever the tile lies.  256 threads.  lp_detail_stitch_regions reads the mask through an `Edit` (another region's
// components erased, detail_kernel.hip); the default, MaskAsIs, is the mask itself.
#pragma once
#include "lp_common.h"

namespace lp {

template <int TH, int TW>
constexpr size_t mask_tile_lds_bytes(int k) {
    const int R = k / 2;
    return sizeof(float) * (static_cast<size_t>(TH + 4 * R) * (TW + 4 * R) + static_cast<size_t>(TH + 4 * R) * (TW + 2 * R) + k);
}

// How a mask element enters pass A: Edit(value, flat index in the mask plane).  The default takes it as it is, and is the
// same for every window (region, image) of a launch (detail_kernel.hip).
struct MaskAsIs {
    __device__ __forceinline__ float operator()(float v, int64_t) const { return v; }
    __device__ __forceinline__ MaskAsIs view(int, int, int64_t) const { return *this; }
};

// Runs passes A..D on `lds` (mask_tile_lds_bytes<TH, TW>(k) bytes).  On return D (CH x TW, CH = TH + 2R, row-blurred) and g
// (k weights) are valid for every thread; the first AH x AW floats of `lds` (A) are free for the caller.
template <int TH, int TW, class Edit = MaskAsIs>
__device__ __forceinline__ void mask_tile_passes(float* lds, const float* __restrict__ mplane, int mask_h, int mask_w,
                                                 int nn_rule, int k, int x0, int y0, int H, int W, float*& D, float*& g,
                                                 const Edit edit = Edit()) {
    const int R = k / 2;
    const int AW = TW + 4 * R, AH = TH + 4 * R, BW = TW + 2 * R, CH = TH + 2 * R;
    float* A = lds;                   // AH x AW raw mask; later C: CH x BW dilated
    float* B = A + AH * AW;           // AH x BW row-max;  later D: CH x TW row-blurred
    g = B + AH * BW;                  // k normalised 1-D Gaussian weights
    D = B;
    const int tid = threadIdx.x;

    if (tid < k) {                    // gaussian_kernel_2d: sigma = (k-1)/4; identity for k <= 1
        float w = 1.0f;
        if (k > 1) {
            const float sigma = static_cast<float>(k - 1) / 4.0f, inv = 1.0f / (2.0f * sigma * sigma);
            float sum = 0.0f;
            for (int j = 0; j < k; ++j) sum += expf(-static_cast<float>((j - R) * (j - R)) * inv);
            w = expf(-static_cast<float>((tid - R) * (tid - R)) * inv) / sum;
        }
        g[tid] = w;
    }
    const bool resample = mask_h != H || mask_w != W;
    for (int idx = tid; idx < AH * AW; idx += 256) {
        const int ay = idx / AW, ax = idx - ay * AW;
        const int y = y0 - 2 * R + ay, x = x0 - 2 * R + ax;
        float v = -INFINITY;                                   // max_pool2d pads with -inf
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int sy = resample ? nearest_exact_index(y, mask_h, H, nn_rule) : y;
            const int sx = resample ? nearest_exact_index(x, mask_w, W, nn_rule) : x;
            const int64_t at = static_cast<int64_t>(sy) * mask_w + sx;
            v = edit(mplane[at], at);
        }
        A[idx] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < AH * BW; idx += 256) {           // row max over the k-wide window
        const int ay = idx / BW, bx = idx - ay * BW;
        const float* row = A + ay * AW + bx;
        float v = row[0];
        for (int j = 1; j < k; ++j) v = fmaxf(v, row[j]);
        B[idx] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < CH * BW; idx += 256) {           // column max; conv2d pads with ZERO
        const int cy = idx / BW, bx = idx - cy * BW;
        const int y = y0 - R + cy, x = x0 - R + bx;
        float v = 0.0f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            v = B[cy * BW + bx];
            for (int j = 1; j < k; ++j) v = fmaxf(v, B[(cy + j) * BW + bx]);
        }
        A[idx] = v;                                            // C
    }
    __syncthreads();
    for (int idx = tid; idx < CH * TW; idx += 256) {           // row blur
        const int cy = idx / TW, tx = idx - cy * TW;
        const float* row = A + cy * BW + tx;
        float v = 0.0f;
        for (int j = 0; j < k; ++j) v += g[j] * row[j];
        B[idx] = v;                                            // D
    }
    __syncthreads();
}

template <int TW>
__device__ __forceinline__ float smoothed_mask_at(const float* D, const float* g, int k, int ty, int tx) {   // column blur
    float m = 0.0f;
    for (int j = 0; j < k; ++j) m += g[j] * D[(ty + j) * TW + tx];
    return m;
}

}  // namespace lp
