// detail_kernel.hip -- Detailer crop / stitch for gfx950: inpaint at the resolution of the masked region.  Pixel space, once
// per job, around the sampler (lanpaint_amd/detail.py plans the region on the host).  Three jobs on the caller's stream:
//
//   lp_mask_bbox        rows / columns of mask > 0.5 over every plane: per wave a __ballot per column slot and an OR of row
//                       bits, per block one integer atomicMin / atomicMax per bound.  Integer-exact, order-free.
//   lp_detail_resample  a window of an NHWC image to another size with torch's antialiased bilinear / bicubic rule, from
//                       host-built fp32 tap tables.  Both passes in one launch: a block stages the horizontal pass of the
//                       source rows its output tile needs in LDS, then the vertical pass writes 16 B per lane.  Rows are
//                       indexed as flat fp32 streams of W * C elements, so reads and writes coalesce whatever C is.
//                       Same size in and out is a plain window copy (bitwise).
//   lp_detail_stitch    out = original outside the region (one streaming copy), original * (1 - m) + detail * m inside, m the
//                       MaskBlend-smoothed mask of the WHOLE image evaluated on the region's tiles (mask_tile.h, shared with
//                       lp_mask_blend).  No full-frame temporary; per-pixel work only over the region plus its halo.
//
// and the same two for several windows of one size (lp_detail_resample_regions, lp_detail_stitch_regions): the crops of all
// regions in one launch, window origins from a device table; the stitch as one copy, then region after region in place on
// the result.  Region r sees the mask with the components of other regions erased (EraseForeign reads the label image of
// label_kernel.hip and an owner table), evaluated where the mask is read: no per-region mask is ever written at frame size.
//
// and for a window that follows a moving mask through a video (lp_mask_bbox_frames, lp_detail_resample_track,
// lp_detail_stitch_track): a box per plane in one launch, then the regions crop and the single-window stitch with the origin
// looked up by image instead of by region.  Frames never overlap each other, so the whole stitch is one launch after the copy.
#include "lp_common.h"
#include "mask_tile.h"
#include "resample_tile.h"

namespace lp {
namespace {

constexpr int kBboxRows = 16;       // bbox tile: 16 rows x (256 lanes x V columns)
constexpr int kCopyBlocks = 2048;   // streaming copy: grid-stride, 8 blocks per CU

// ---- bounding box -------------------------------------------------------------------------------------------------------
__global__ void lp_detail_bbox_init_kernel(int32_t* __restrict__ bbox, int H, int W, int boxes) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, f = t & 3;
    if (t < 4 * boxes) bbox[t] = (f == 0) ? H : (f == 2) ? W : -1;
}

// Lane l of the block reads columns x .. x + V - 1 of 16 rows of one plane (V = 4: one 16 B load per row).  rowbits: the rows
// of the tile this lane saw set; hit[j]: whether column slot j was set in any row.  The tile's bounds go into `bbox`.
template <int V>
__device__ __forceinline__ void bbox_tile(const float* __restrict__ mask, int32_t* __restrict__ bbox, int H, int W) {
    __shared__ int32_t part[4][4];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int x = (blockIdx.x * 256 + threadIdx.x) * V, y0 = blockIdx.y * kBboxRows;
    const float* plane = mask + static_cast<int64_t>(blockIdx.z) * H * W;
    uint32_t rowbits = 0;
    bool hit[V];
#pragma unroll
    for (int j = 0; j < V; ++j) hit[j] = false;
    if (x < W) {
#pragma unroll
        for (int r = 0; r < kBboxRows; ++r) {
            if (y0 + r >= H) break;
            const float* p = plane + static_cast<int64_t>(y0 + r) * W + x;
            float v[V];
            if constexpr (V == 4) {                            // W % 4 == 0 and a 16 B aligned base: x + 3 < W
                const float4 q = *reinterpret_cast<const float4*>(p);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                v[0] = p[0];
            }
            bool any = false;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool s = v[j] > 0.5f;
                hit[j] |= s;
                any |= s;
            }
            rowbits |= any ? (1u << r) : 0u;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rowbits |= __shfl_xor(rowbits, off);
    int cmin = W, cmax = -1;
    const int wx = (blockIdx.x * 256 + wave * kWave) * V;      // first column of this wave
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const unsigned long long bal = __ballot(hit[j]);
        if (bal) {
            cmin = min(cmin, wx + __builtin_ctzll(bal) * V + j);
            cmax = max(cmax, wx + (63 - __builtin_clzll(bal)) * V + j);
        }
    }
    if (lane == 0) {
        part[wave][0] = rowbits ? y0 + __builtin_ctz(rowbits) : H;
        part[wave][1] = rowbits ? y0 + 31 - __builtin_clz(rowbits) : -1;
        part[wave][2] = cmin;
        part[wave][3] = cmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int r0 = H, r1 = -1, c0 = W, c1 = -1;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            r0 = min(r0, part[w][0]); r1 = max(r1, part[w][1]);
            c0 = min(c0, part[w][2]); c1 = max(c1, part[w][3]);
        }
        if (r1 >= 0) {                                         // one atomic per bound per block; empty tiles send none
            atomicMin(bbox + 0, r0); atomicMax(bbox + 1, r1);
            atomicMin(bbox + 2, c0); atomicMax(bbox + 3, c1);
        }
    }
}

template <int V>
__global__ __launch_bounds__(256) void lp_detail_bbox_kernel(const float* __restrict__ mask, int32_t* __restrict__ bbox, int H,
                                                             int W) {
    bbox_tile<V>(mask, bbox, H, W);                              // every plane into one box
}

template <int V>
__global__ __launch_bounds__(256) void lp_detail_bbox_frames_kernel(const float* __restrict__ mask, int32_t* __restrict__ boxes,
                                                                    int H, int W) {
    bbox_tile<V>(mask, boxes + 4 * blockIdx.z, H, W);            // plane p into row p
}

// ---- crop + resample ----------------------------------------------------------------------------------------------------
// torch's antialiased passes for resample_tile: fp32 NHWC source, fp32 sums from zero with the taps ascending, the horizontal
// pass parked as one float4.  The library is built with -ffp-contract=on, so a multiply-add fuses only inside one source
// expression: `ss += s[t * C] * w[t]` here and the tile's `acc += tap * wt` each are one, and have to stay one.
struct TorchAA {
    using Src = float;
    using Weight = float;
    using Acc = float;
    using Staged = float4;
    static __device__ __forceinline__ float acc0() { return 0.0f; }
    static __device__ __forceinline__ float hsum(const float* s, const float* w, int n, int C) {
        float ss = 0.0f;
        for (int t = 0; t < n; ++t) ss += s[t * C] * w[t];
        return ss;
    }
    static __device__ __forceinline__ float4 pack(const float (&v)[4]) { return make_float4(v[0], v[1], v[2], v[3]); }
    static __device__ __forceinline__ float tap(const float4& p, int j) { return j == 0 ? p.x : j == 1 ? p.y : j == 2 ? p.z : p.w; }
    static __device__ __forceinline__ float finish(float acc) { return acc; }
};

// One block: a 16 x 256 tile of image b's output (resample_tile.h), read from the window at (y0, x0) of the source image.
__global__ __launch_bounds__(256) void lp_detail_resample_kernel(const lp_detail_resample_desc d) {
    const int C = d.channels, b = blockIdx.z;
    const int rowE = d.out_w * C;
    resample_tile<TorchAA>(d.src + ((static_cast<int64_t>(b) * d.src_h + d.y0) * d.src_w + d.x0) * C,
                           static_cast<int64_t>(d.src_w) * C, C, d.win_h, d.win_w, d.out_h, rowE, d.bounds_x, d.weights_x,
                           d.ksize_x, d.bounds_y, d.weights_y, d.ksize_y, d.dst + static_cast<int64_t>(b) * d.out_h * rowE);
}

// Same size in and out: the window's rows copied as flat streams, one element per lane.
__global__ __launch_bounds__(256) void lp_detail_crop_kernel(const lp_detail_resample_desc d) {
    const int C = d.channels, rowE = d.win_w * C;
    const int e = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (e >= rowE) return;
    const float* s = d.src + ((static_cast<int64_t>(b) * d.src_h + d.y0 + y) * d.src_w + d.x0) * C;
    d.dst[(static_cast<int64_t>(b) * d.win_h + y) * rowE + e] = s[e];
}

// ---- stitch -------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void lp_detail_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if constexpr (VEC) {
        const int64_t n4 = n >> 2;
        for (int64_t q = i; q < n4; q += stride)
            reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(src)[q];
        i += n4 << 2;                                             // the tail, at most 3 elements
        if (i < n) dst[i] = src[i];
    } else {
        for (; i < n; i += stride) dst[i] = src[i];
    }
}

// A block owns a TH x TW tile of the REGION of image b; tile origins are image coordinates, so the smoothed mask is the
// whole image's.  m goes to LDS, then the tile's rows are blended as flat streams of TW * C elements.  `edit` is how a mask
// element enters the passes (mask_tile.h): as it is, or with another region's components erased.  out may be original: one
// thread reads and writes a given element, and the halo is read from the mask alone.  The window is at (wy0, wx0): the
// descriptor's, or one looked up per image.
template <int TH, int TW, class Edit>
__device__ __forceinline__ void stitch_tile(const lp_detail_stitch_desc& d, const int wy0, const int wx0, const Edit edit) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int k = d.k, tid = threadIdx.x;
    const int x0 = wx0 + blockIdx.x * TW, y0 = wy0 + blockIdx.y * TH, b = blockIdx.z;
    const int H = d.height, W = d.width, C = d.channels;
    const float* mplane = d.mask + static_cast<int64_t>(d.mask_batch == 1 ? 0 : b) * H * W;
    float *D, *g;
    mask_tile_passes<TH, TW, Edit>(lds, mplane, H, W, LP_NN_ATEN_SCALAR, k, x0, y0, H, W, D, g, edit);
    float* M = lds;                                               // the passes' A, free now: TH x TW smoothed mask
    for (int idx = tid; idx < TH * TW; idx += 256) {
        const int ty = idx / TW, tx = idx - ty * TW;
        M[idx] = smoothed_mask_at<TW>(D, g, k, ty, tx);
    }
    __syncthreads();
    const int ty_end = min(TH, wy0 + d.win_h - y0), tx_end = min(TW, wx0 + d.win_w - x0);
    const int rowE = tx_end * C;
    for (int idx = tid; idx < ty_end * rowE; idx += 256) {
        const int ty = idx / rowE, e = idx - ty * rowE;
        const float m = M[ty * TW + e / C];
        const int64_t io = ((static_cast<int64_t>(b) * H + y0 + ty) * W + x0) * C + e;
        const int64_t id = ((static_cast<int64_t>(b) * d.win_h + (y0 - wy0) + ty) * d.win_w + (x0 - wx0)) * C + e;
        d.out[io] = d.original[io] * (1.0f - m) + d.detail[id] * m;
    }
}

template <int TH, int TW>
__global__ __launch_bounds__(256) void lp_detail_stitch_kernel(const lp_detail_stitch_desc d) {
    stitch_tile<TH, TW>(d, d.y0, d.x0, MaskAsIs());
}

// Region `mine - 1`'s view of the mask: components that belong to another region, or to none, read as 0.  Label 0 -- every
// value at or below 0.5 -- is nobody's and stays, so feathered edges survive.
struct EraseForeign {
    const int32_t* labels;
    const int32_t* owner;
    int owner_len, mine;
    __device__ __forceinline__ float operator()(float v, int64_t at) const {
        const int label = labels[at];
        if (label == 0) return v;
        const int o = (label > 0 && label < owner_len) ? owner[label] : 0;
        return o == mine ? v : 0.0f;
    }
};

template <int TH, int TW>
__global__ __launch_bounds__(256) void lp_detail_stitch_region_kernel(const lp_detail_stitch_desc d, const EraseForeign erase) {
    stitch_tile<TH, TW>(d, d.y0, d.x0, erase);
}

template <int TH, int TW, class... Extra>
hipError_t launch_stitch(void (*kernel)(const lp_detail_stitch_desc, Extra...), const lp_detail_stitch_desc& d,
                         hipStream_t stream, Extra... extra) {
    const size_t lds = mask_tile_lds_bytes<TH, TW>(d.k);
    if (lds > 64 * 1024)                                          // per device, like lp_mask_blend
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const dim3 grid((d.win_w + TW - 1) / TW, (d.win_h + TH - 1) / TH, d.batch);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, d, extra...);
    return hipGetLastError();
}

// ---- regions: the same jobs for several windows of one size ----------------------------------------------------------------
__device__ __forceinline__ void region_origin(const int32_t* __restrict__ origins, int r, int H, int W, int h, int w, int& y0,
                                              int& x0) {                // clamped: a bad table reads nothing outside the image
    y0 = min(max(origins[2 * r], 0), H - h);
    x0 = min(max(origins[2 * r + 1], 0), W - w);
}

// blockIdx.z = region * batch + image; otherwise lp_detail_resample_kernel.  TRACK: one window per image, a table row per
// image (regions == 1, so blockIdx.z is the image).
template <bool TRACK>
__global__ __launch_bounds__(256) void lp_detail_resample_regions_kernel(const lp_detail_resample_regions_desc d) {
    const int C = d.channels, z = blockIdx.z, r = z / d.batch, b = z - r * d.batch;
    const int rowE = d.out_w * C;
    int y0, x0;
    region_origin(d.origins, TRACK ? b : r, d.src_h, d.src_w, d.win_h, d.win_w, y0, x0);
    resample_tile<TorchAA>(d.src + ((static_cast<int64_t>(b) * d.src_h + y0) * d.src_w + x0) * C,
                           static_cast<int64_t>(d.src_w) * C, C, d.win_h, d.win_w, d.out_h, rowE, d.bounds_x, d.weights_x,
                           d.ksize_x, d.bounds_y, d.weights_y, d.ksize_y, d.dst + static_cast<int64_t>(z) * d.out_h * rowE);
}

// The windows' rows copied as flat streams into dst [regions * batch, win_h, win_w, C]; ERASE (C == 1): through EraseForeign.
template <bool ERASE, bool TRACK>
__global__ __launch_bounds__(256) void lp_detail_crop_regions_kernel(const lp_detail_resample_regions_desc d, float* __restrict__ dst) {
    const int C = d.channels, rowE = d.win_w * C;
    const int e = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, z = blockIdx.z, r = z / d.batch, b = z - r * d.batch;
    if (e >= rowE) return;
    int y0, x0;
    region_origin(d.origins, TRACK ? b : r, d.src_h, d.src_w, d.win_h, d.win_w, y0, x0);
    const int64_t at = static_cast<int64_t>(y0 + y) * d.src_w + x0;    // of the window row's first pixel in its plane
    float v = d.src[(static_cast<int64_t>(b) * d.src_h * d.src_w + at) * C + e];
    if constexpr (ERASE) v = EraseForeign{d.labels, d.owner, d.owner_len, r + 1}(v, at + e);
    dst[(static_cast<int64_t>(z) * d.win_h + y) * rowE + e] = v;
}

// Image b's window is at origins[b]; otherwise lp_detail_stitch_kernel.  d.y0 / d.x0 are not read.
template <int TH, int TW>
__global__ __launch_bounds__(256) void lp_detail_stitch_track_kernel(const lp_detail_stitch_desc d, const int32_t* __restrict__ origins) {
    int y0, x0;
    region_origin(origins, blockIdx.z, d.height, d.width, d.win_h, d.win_w, y0, x0);
    stitch_tile<TH, TW>(d, y0, x0, MaskAsIs());
}

// One streaming copy original -> out on `stream`, the first launch of every stitch.
hipError_t launch_frame_copy(const float* original, float* out, int64_t n, hipStream_t stream) {
    const uint32_t blocks = static_cast<uint32_t>(min(static_cast<int64_t>(kCopyBlocks), (n + 1023) / 1024));
    if (aligned16(original) && aligned16(out))
        hipLaunchKernelGGL(lp_detail_copy_kernel<true>, dim3(blocks), dim3(256), 0, stream, original, out, n);
    else                                                          // a frame range of a larger tensor need not start on 16 bytes
        hipLaunchKernelGGL(lp_detail_copy_kernel<false>, dim3(blocks), dim3(256), 0, stream, original, out, n);
    return hipGetLastError();
}

// The unerased crops of `images` windows: the resample tile, or the plain copy when the size stays.
template <bool TRACK>
void launch_windows(const lp_detail_resample_regions_desc& d, int images, bool same, hipStream_t stream) {
    if (same) {
        const dim3 grid((d.win_w * d.channels + 255) / 256, d.win_h, images);
        hipLaunchKernelGGL((lp_detail_crop_regions_kernel<false, TRACK>), grid, dim3(256), 0, stream, d, d.dst);
    } else {
        const dim3 grid((d.out_w * d.channels + kResampleTX - 1) / kResampleTX, (d.out_h + kResampleTY - 1) / kResampleTY, images);
        hipLaunchKernelGGL(lp_detail_resample_regions_kernel<TRACK>, grid, dim3(256), 0, stream, d);
    }
}

bool side_ok(int s) { return s > 0 && s <= LP_DETAIL_MAX_SIDE; }
bool chan_ok(int c) { return c > 0 && c <= LP_DETAIL_MAX_CHANNELS; }
bool window_ok(int y0, int x0, int h, int w, int H, int W) {
    return y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && h <= H - y0 && w <= W - x0;
}

}  // namespace

int mask_bbox_dispatch(const float* mask, int planes, int H, int W, int32_t* bbox, hipStream_t stream) {
    if (!mask || !bbox || planes <= 0 || !side_ok(H) || !side_ok(W)) return LP_E_INVALID;
    if (planes > 65535) return LP_E_UNSUPPORTED;
    hipLaunchKernelGGL(lp_detail_bbox_init_kernel, dim3(1), dim3(kWave), 0, stream, bbox, H, W, 1);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    const uint32_t gy = (H + kBboxRows - 1) / kBboxRows;
    if ((W & 3) == 0 && aligned16(mask))
        hipLaunchKernelGGL(lp_detail_bbox_kernel<4>, dim3((W + 1023) / 1024, gy, planes), dim3(256), 0, stream, mask, bbox, H, W);
    else
        hipLaunchKernelGGL(lp_detail_bbox_kernel<1>, dim3((W + 255) / 256, gy, planes), dim3(256), 0, stream, mask, bbox, H, W);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

int mask_bbox_frames_dispatch(const float* mask, int planes, int H, int W, int32_t* boxes, hipStream_t stream) {
    if (!mask || !boxes || planes <= 0 || !side_ok(H) || !side_ok(W)) return LP_E_INVALID;
    if (planes > 65535) return LP_E_UNSUPPORTED;
    hipLaunchKernelGGL(lp_detail_bbox_init_kernel, dim3((4 * planes + 255) / 256), dim3(256), 0, stream, boxes, H, W, planes);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    const uint32_t gy = (H + kBboxRows - 1) / kBboxRows;
    if ((W & 3) == 0 && aligned16(mask))                          // then every plane starts on 16 bytes too
        hipLaunchKernelGGL(lp_detail_bbox_frames_kernel<4>, dim3((W + 1023) / 1024, gy, planes), dim3(256), 0, stream, mask, boxes, H, W);
    else
        hipLaunchKernelGGL(lp_detail_bbox_frames_kernel<1>, dim3((W + 255) / 256, gy, planes), dim3(256), 0, stream, mask, boxes, H, W);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

int detail_resample_dispatch(const lp_detail_resample_desc* dp, hipStream_t stream) {
    if (!dp) return LP_E_INVALID;
    const lp_detail_resample_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.src_h) || !side_ok(d.src_w) || !chan_ok(d.channels)) return LP_E_INVALID;
    if (!window_ok(d.y0, d.x0, d.win_h, d.win_w, d.src_h, d.src_w) || !side_ok(d.out_h) || !side_ok(d.out_w)) return LP_E_INVALID;
    if (!d.src || !d.dst) return LP_E_INVALID;
    const bool same = d.out_h == d.win_h && d.out_w == d.win_w;
    if (!same) {
        if (d.ksize_x <= 0 || d.ksize_y <= 0) return LP_E_INVALID;
        if (!d.bounds_x || !d.weights_x || !d.bounds_y || !d.weights_y) return LP_E_INVALID;
        if (!aligned16(d.dst)) return LP_E_ALIGN;
    }
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    const int rowE = d.out_w * d.channels;
    if (same) {
        hipLaunchKernelGGL(lp_detail_crop_kernel, dim3((rowE + 255) / 256, d.win_h, d.batch), dim3(256), 0, stream, d);
    } else {
        const dim3 grid((rowE + kResampleTX - 1) / kResampleTX, (d.out_h + kResampleTY - 1) / kResampleTY, d.batch);
        hipLaunchKernelGGL(lp_detail_resample_kernel, grid, dim3(256), 0, stream, d);
    }
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

int detail_stitch_dispatch(const lp_detail_stitch_desc* dp, hipStream_t stream) {
    if (!dp) return LP_E_INVALID;
    const lp_detail_stitch_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.height) || !side_ok(d.width) || !chan_ok(d.channels)) return LP_E_INVALID;
    if (!window_ok(d.y0, d.x0, d.win_h, d.win_w, d.height, d.width)) return LP_E_INVALID;
    if (d.k < 1 || d.k > 51 || (d.k % 2) == 0) return LP_E_INVALID;
    if (d.mask_batch != 1 && d.mask_batch != d.batch) return LP_E_INVALID;
    if (!d.mask || !d.original || !d.detail || !d.out || d.out == d.original) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    const int64_t n = static_cast<int64_t>(d.batch) * d.height * d.width * d.channels;
    if (launch_frame_copy(d.original, d.out, n, stream) != hipSuccess) return LP_E_LAUNCH;
    const hipError_t err = (d.k <= 15) ? launch_stitch<16, 64>(lp_detail_stitch_kernel<16, 64>, d, stream)
                                       : launch_stitch<8, 32>(lp_detail_stitch_kernel<8, 32>, d, stream);
    return err == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

int detail_resample_regions_dispatch(const lp_detail_resample_regions_desc* dp, hipStream_t stream) {
    if (!dp) return LP_E_INVALID;
    const lp_detail_resample_regions_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.src_h) || !side_ok(d.src_w) || !chan_ok(d.channels)) return LP_E_INVALID;
    if (d.regions < 1 || d.regions > LP_DETAIL_MAX_REGIONS || !d.origins) return LP_E_INVALID;
    if (!window_ok(0, 0, d.win_h, d.win_w, d.src_h, d.src_w) || !side_ok(d.out_h) || !side_ok(d.out_w)) return LP_E_INVALID;
    if (!d.src || !d.dst) return LP_E_INVALID;
    const bool same = d.out_h == d.win_h && d.out_w == d.win_w;
    if (d.labels && (d.channels != 1 || !d.owner || d.owner_len < 1 || (!same && !d.scratch))) return LP_E_INVALID;
    if (!same) {
        if (d.ksize_x <= 0 || d.ksize_y <= 0) return LP_E_INVALID;
        if (!d.bounds_x || !d.weights_x || !d.bounds_y || !d.weights_y) return LP_E_INVALID;
        if (!aligned16(d.dst) || (d.labels && !aligned16(d.scratch))) return LP_E_ALIGN;
    }
    if (static_cast<int64_t>(d.regions) * d.batch > 65535) return LP_E_UNSUPPORTED;
    const int images = d.regions * d.batch;
    const dim3 crop_grid((d.win_w * d.channels + 255) / 256, d.win_h, images);
    const dim3 tile_grid((d.out_w * d.channels + kResampleTX - 1) / kResampleTX, (d.out_h + kResampleTY - 1) / kResampleTY, images);
    if (d.labels) {                                               // erased windows: the result, or the resample's source
        hipLaunchKernelGGL((lp_detail_crop_regions_kernel<true, false>), crop_grid, dim3(256), 0, stream, d, same ? d.dst : d.scratch);
        if (!same) {
            if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
            lp_detail_resample_desc w = {images, d.win_h, d.win_w, 1, 0, 0, d.win_h, d.win_w, d.out_h, d.out_w, d.ksize_x,
                                         d.ksize_y, d.scratch, d.bounds_x, d.weights_x, d.bounds_y, d.weights_y, d.dst};
            hipLaunchKernelGGL(lp_detail_resample_kernel, tile_grid, dim3(256), 0, stream, w);
        }
    } else {
        launch_windows<false>(d, images, same, stream);
    }
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

int detail_stitch_regions_dispatch(const lp_detail_stitch_regions_desc* dp, hipStream_t stream) {
    if (!dp) return LP_E_INVALID;
    const lp_detail_stitch_regions_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.height) || !side_ok(d.width) || !chan_ok(d.channels)) return LP_E_INVALID;
    if (d.regions < 1 || d.regions > LP_DETAIL_MAX_REGIONS || !d.origins) return LP_E_INVALID;
    for (int r = 0; r < d.regions; ++r)
        if (!window_ok(d.origins[2 * r], d.origins[2 * r + 1], d.win_h, d.win_w, d.height, d.width)) return LP_E_INVALID;
    if (d.k < 1 || d.k > 51 || (d.k % 2) == 0) return LP_E_INVALID;
    if (d.mask_batch != 1 && d.mask_batch != d.batch) return LP_E_INVALID;
    if (!d.mask || !d.original || !d.detail || !d.out || d.out == d.original) return LP_E_INVALID;
    if (d.labels && (!d.owner || d.owner_len < 1)) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    const int64_t n = static_cast<int64_t>(d.batch) * d.height * d.width * d.channels;
    if (launch_frame_copy(d.original, d.out, n, stream) != hipSuccess) return LP_E_LAUNCH;
    const int64_t per_region = static_cast<int64_t>(d.batch) * d.win_h * d.win_w * d.channels;
    for (int r = 0; r < d.regions; ++r) {                         // in order, in place: out_{r+1} from out_r
        const lp_detail_stitch_desc s = {d.batch, d.height, d.width, d.channels, d.origins[2 * r], d.origins[2 * r + 1],
                                         d.win_h, d.win_w, d.k, d.mask_batch, d.mask, d.out, d.detail + r * per_region, d.out};
        hipError_t err;
        if (d.labels) {
            const EraseForeign erase = {d.labels, d.owner, d.owner_len, r + 1};
            err = (d.k <= 15) ? launch_stitch<16, 64>(lp_detail_stitch_region_kernel<16, 64>, s, stream, erase)
                              : launch_stitch<8, 32>(lp_detail_stitch_region_kernel<8, 32>, s, stream, erase);
        } else {
            err = (d.k <= 15) ? launch_stitch<16, 64>(lp_detail_stitch_kernel<16, 64>, s, stream)
                              : launch_stitch<8, 32>(lp_detail_stitch_kernel<8, 32>, s, stream);
        }
        if (err != hipSuccess) return LP_E_LAUNCH;
    }
    return LP_OK;
}

int detail_resample_track_dispatch(const lp_detail_resample_track_desc* dp, hipStream_t stream) {
    if (!dp) return LP_E_INVALID;
    const lp_detail_resample_track_desc& t = *dp;
    if (t.batch <= 0 || !side_ok(t.src_h) || !side_ok(t.src_w) || !chan_ok(t.channels) || !t.origins) return LP_E_INVALID;
    if (!window_ok(0, 0, t.win_h, t.win_w, t.src_h, t.src_w) || !side_ok(t.out_h) || !side_ok(t.out_w)) return LP_E_INVALID;
    if (!t.src || !t.dst) return LP_E_INVALID;
    const bool same = t.out_h == t.win_h && t.out_w == t.win_w;
    if (!same) {
        if (t.ksize_x <= 0 || t.ksize_y <= 0) return LP_E_INVALID;
        if (!t.bounds_x || !t.weights_x || !t.bounds_y || !t.weights_y) return LP_E_INVALID;
        if (!aligned16(t.dst)) return LP_E_ALIGN;
    }
    if (t.batch > 65535) return LP_E_UNSUPPORTED;
    const lp_detail_resample_regions_desc d = {t.batch, t.src_h, t.src_w, t.channels, 1, t.win_h, t.win_w, 0, t.out_h, t.out_w,
                                               t.ksize_x, t.ksize_y, t.origins, t.src, t.bounds_x, t.weights_x, t.bounds_y,
                                               t.weights_y, t.dst, nullptr, nullptr, nullptr};
    launch_windows<true>(d, t.batch, same, stream);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

int detail_stitch_track_dispatch(const lp_detail_stitch_track_desc* dp, hipStream_t stream) {
    if (!dp) return LP_E_INVALID;
    const lp_detail_stitch_track_desc& t = *dp;
    if (t.batch <= 0 || !side_ok(t.height) || !side_ok(t.width) || !chan_ok(t.channels) || !t.origins) return LP_E_INVALID;
    if (!window_ok(0, 0, t.win_h, t.win_w, t.height, t.width)) return LP_E_INVALID;
    if (t.k < 1 || t.k > 51 || (t.k % 2) == 0) return LP_E_INVALID;
    if (t.mask_batch != 1 && t.mask_batch != t.batch) return LP_E_INVALID;
    if (!t.mask || !t.original || !t.detail || !t.out || t.out == t.original) return LP_E_INVALID;
    if (t.batch > 65535) return LP_E_UNSUPPORTED;
    const int64_t n = static_cast<int64_t>(t.batch) * t.height * t.width * t.channels;
    if (launch_frame_copy(t.original, t.out, n, stream) != hipSuccess) return LP_E_LAUNCH;
    const lp_detail_stitch_desc d = {t.batch, t.height, t.width, t.channels, 0, 0, t.win_h, t.win_w, t.k, t.mask_batch,
                                     t.mask, t.original, t.detail, t.out};
    const hipError_t err = (t.k <= 15) ? launch_stitch<16, 64>(lp_detail_stitch_track_kernel<16, 64>, d, stream, t.origins)
                                       : launch_stitch<8, 32>(lp_detail_stitch_track_kernel<8, 32>, d, stream, t.origins);
    return err == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

}  // namespace lp
