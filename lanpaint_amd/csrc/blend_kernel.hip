// blend_kernel.hip -- post-decode mask blend for gfx950: dilate (max-pool) + Gaussian blur of the
// mask and the image lerp in ONE launch.  Restates MaskBlend.blend_images (reference
// nodes.py:610-638), merge_video_with_mask (nodes.py:1060-1088) and gaussian_kernel_2d (:1049-1057).
//
// A block owns a TH x TW tile of one image.  The mask tile plus a 2R halo (R = k/2: R for the
// dilation, R for the blur) is staged in LDS once and smoothed there by the separable passes of
// mask_tile.h (shared with lp_detail_stitch); then
//   D  --col blur--> m (registers)  --> out = image1*(1-m) + image2*m
// Entry point defined here: lp_mask_blend.
#include "lp_common.h"
#include "mask_tile.h"

namespace lp {

template <int TH, int TW>
__global__ __launch_bounds__(256) void lp_mask_blend_kernel(const lp_blend_desc d) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int k = d.k;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, b = blockIdx.z;
    const int H = d.height, W = d.width;
    const float* mplane = d.mask + static_cast<int64_t>(d.mask_batch == 1 ? 0 : b) * d.mask_h * d.mask_w;
    float *D, *g;
    mask_tile_passes<TH, TW>(lds, mplane, d.mask_h, d.mask_w, d.nn_rule, k, x0, y0, H, W, D, g);
    const int C = d.channels;
    for (int idx = tid; idx < TH * TW; idx += 256) {           // column blur + blend
        const int ty = idx / TW, tx = idx - ty * TW;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        const float m = smoothed_mask_at<TW>(D, g, k, ty, tx);
        const int64_t pix = (static_cast<int64_t>(b) * H + y) * W + x;
        if (d.smooth_out) d.smooth_out[pix] = m;
        if (d.out) {
            const float* p1 = d.image1 + pix * C;
            const float* p2 = d.image2 + pix * C;
            float* po = d.out + pix * C;
            for (int c = 0; c < C; ++c) po[c] = p1[c] * (1.0f - m) + p2[c] * m;
        }
    }
}

template <int TH, int TW>
static hipError_t launch_blend(const lp_blend_desc& d, hipStream_t stream) {
    const size_t lds = mask_tile_lds_bytes<TH, TW>(d.k);
    // above the default 64 KiB cap the dynamic-LDS limit has to be raised (160 KiB per CU on gfx950).  The attribute is
    // per DEVICE, so it is set on whatever device this launch goes to -- no process-wide "done" flag (the library
    // keeps no state; a second GPU of the same process would otherwise fail to launch)
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&lp_mask_blend_kernel<TH, TW>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const dim3 grid((d.width + TW - 1) / TW, (d.height + TH - 1) / TH, d.batch);
    hipLaunchKernelGGL((lp_mask_blend_kernel<TH, TW>), grid, dim3(256), lds, stream, d);
    return hipGetLastError();
}

extern "C" int lp_mask_blend(const lp_blend_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_blend_desc& d = *dp;
    if (d.batch <= 0 || d.height <= 0 || d.width <= 0 || d.channels <= 0 || !d.mask) return LP_E_INVALID;
    if (d.k < 1 || d.k > 51 || (d.k % 2) == 0) return LP_E_INVALID;
    if (d.mask_batch != 1 && d.mask_batch != d.batch) return LP_E_INVALID;
    if (d.mask_h <= 0 || d.mask_w <= 0) return LP_E_INVALID;
    if (d.nn_rule < LP_NN_ATEN_SCALAR || d.nn_rule > LP_NN_ATEN_CPU_GENERIC) return LP_E_INVALID;
    if (!d.out && !d.smooth_out) return LP_E_INVALID;
    if (d.out && (!d.image1 || !d.image2)) return LP_E_INVALID;
    if (d.batch > 65535 || (d.height + 7) / 8 > 65535) return LP_E_UNSUPPORTED;
    // small halos: wide tiles; large halos: the tile shrinks so tile + halo stays inside 160 KiB of LDS
    const hipError_t err = (d.k <= 15) ? launch_blend<16, 64>(d, stream) : launch_blend<8, 32>(d, stream);
    return err == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

}  // namespace lp
