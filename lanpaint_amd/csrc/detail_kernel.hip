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
//
// and per subject of a video (lp_subject_boxes, lp_detail_resample_subjects, lp_detail_stitch_subjects): the labels are a
// volume (lp_mask_components_frames), a subject is a set of its components, and window (s, f) follows subject s through frame
// f.  A box per (subject, frame) in one launch; the crops of every (subject, frame) in one launch, subject s seeing frame f's
// mask with foreign components erased through frame f's label plane; the stitch as one copy, then one launch per subject over
// all frames' windows, in subject order and in place.
//
// All four forms run the same three kernels (resample, same-size crop, stitch), templates over where block z's window is --
// WindowAt, or WindowFrom<OriginOf>: a device table indexed by region, by image or by z itself, clamped in one place -- and
// over how a mask element is read: MaskAsIs, or EraseForeign<PER_IMAGE> through one label plane or one per image, either
// asked for window (r, b)'s view.  The regions and subjects entries share their crop dispatcher and their stitch loop.
// Entry points defined here: lp_mask_bbox, lp_mask_bbox_frames, lp_subject_boxes, lp_detail_resample, lp_detail_stitch and
// their _regions, _track and _subjects forms.
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
// of the tile this lane saw set; hit[j]: whether column slot j was set in any row.  The tile's bounds go into one box for
// every plane, or PER_PLANE into row p of a table for plane p.
template <int V, bool PER_PLANE>
__global__ __launch_bounds__(256) void lp_detail_bbox_kernel(const float* __restrict__ mask, int32_t* __restrict__ bbox, int H,
                                                             int W) {
    __shared__ int32_t part[4][4];
    if constexpr (PER_PLANE) bbox += 4 * blockIdx.z;
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

// ---- a box per (subject, frame) ----------------------------------------------------------------------------------------------
// lp_detail_bbox_kernel's tile with labels for floats: lane l reads column x of 16 rows of frame blockIdx.z's label plane and
// looks each label's subject up (owner[label] = subject + 1; 0, or a label outside the table, is nobody's).  A lane keeps the
// rows of the first subject it meets as bits and sends the rare voxel of a second subject in its column by itself; a wave
// whose lanes carry one subject reduces to one set of four atomics, otherwise each lane sends its own.  Integer atomics only.
__global__ __launch_bounds__(256) void lp_detail_subject_boxes_kernel(const int32_t* __restrict__ labels,
                                                                      const int32_t* __restrict__ owner, int owner_len,
                                                                      int subjects, int32_t* __restrict__ boxes, int H, int W) {
    const int lane = threadIdx.x & (kWave - 1);
    const int x = blockIdx.x * 256 + threadIdx.x, y0 = blockIdx.y * kBboxRows, f = blockIdx.z, frames = gridDim.z;
    const int32_t* plane = labels + static_cast<int64_t>(f) * H * W;
    int mine = 0;
    uint32_t rowbits = 0;
    if (x < W) {
#pragma unroll
        for (int r = 0; r < kBboxRows; ++r) {
            if (y0 + r >= H) break;
            const int label = plane[static_cast<int64_t>(y0 + r) * W + x];
            int o = (label > 0 && label < owner_len) ? owner[label] : 0;
            if (o < 1 || o > subjects) o = 0;
            if (o == 0) continue;
            if (mine == 0) mine = o;
            if (o == mine) {
                rowbits |= 1u << r;
            } else {
                int32_t* box = boxes + 4 * (static_cast<int64_t>(o - 1) * frames + f);
                atomicMin(box + 0, y0 + r); atomicMax(box + 1, y0 + r); atomicMin(box + 2, x); atomicMax(box + 3, x);
            }
        }
    }
    const unsigned long long set = __ballot(mine != 0);
    if (set == 0) return;                                          // wave-uniform
    const int first = __shfl(mine, __builtin_ctzll(set), kWave);
    const bool uniform = __ballot(mine != 0 && mine != first) == 0;
    if (uniform) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) rowbits |= __shfl_xor(rowbits, off);
        if (lane == 0) {
            const int wx = x;                                       // lane 0's column: the wave's first
            int32_t* box = boxes + 4 * (static_cast<int64_t>(first - 1) * frames + f);
            atomicMin(box + 0, y0 + __builtin_ctz(rowbits)); atomicMax(box + 1, y0 + 31 - __builtin_clz(rowbits));
            atomicMin(box + 2, wx + __builtin_ctzll(set)); atomicMax(box + 3, wx + 63 - __builtin_clzll(set));
        }
    } else if (mine != 0) {
        int32_t* box = boxes + 4 * (static_cast<int64_t>(mine - 1) * frames + f);
        atomicMin(box + 0, y0 + __builtin_ctz(rowbits)); atomicMax(box + 1, y0 + 31 - __builtin_clz(rowbits));
        atomicMin(box + 2, x); atomicMax(box + 3, x);
    }
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

// ---- where a window is -----------------------------------------------------------------------------------------------------
// Block z of a crop or stitch grid works on window z.  A policy, passed to the kernel by value, says which image `b` of the
// batch that window lies in, which region `r` it is, and where its origin is in an H x W image.
struct WindowAt {                                                 // the descriptor's (y0, x0), the same in every image
    int y0, x0;
    __device__ __forceinline__ void locate(int z, int, int, int, int, int, int& r, int& b, int& y, int& x) const {
        r = 0; b = z; y = y0; x = x0;
    }
};
enum class OriginOf { Region, Image, Window };                    // which row of a device table [n, 2] of origins is block z's
template <OriginOf BY>
struct WindowFrom {
    const int32_t* origins;
    __device__ __forceinline__ void locate(int z, int batch, int H, int W, int h, int w, int& r, int& b, int& y, int& x) const {
        if constexpr (BY == OriginOf::Image) { r = 0; b = z; } else { r = z / batch; b = z - r * batch; }
        const int i = BY == OriginOf::Region ? r : BY == OriginOf::Image ? b : z;
        y = min(max(origins[2 * i], 0), H - h);                   // clamped: a bad table reads nothing outside the image
        x = min(max(origins[2 * i + 1], 0), W - w);
    }
};
using WindowOfRegion = WindowFrom<OriginOf::Region>;              // z = region * batch + image, origins[region]
using WindowOfImage = WindowFrom<OriginOf::Image>;                // one window per image, origins[image]
using WindowOfSubject = WindowFrom<OriginOf::Window>;             // z = subject * batch + image, origins[z]

// A region's view of the mask: components that belong to another region, or to none, read as 0.  Label 0 -- every value at or
// below 0.5 -- is nobody's and stays, so feathered edges survive.  `mine` is the owner id (region + 1) of the launch's region 0;
// view(r, b, plane) is window (r, b)'s edit: region r of the launch, and with PER_IMAGE -- the labels a volume, one plane of
// `plane` elements per image -- through image b's plane.  MaskAsIs::view (mask_tile.h) is the mask itself for every window.
template <bool PER_IMAGE>
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
    __device__ __forceinline__ EraseForeign view(int r, int b, int64_t plane) const {
        EraseForeign e = *this;
        e.mine += r;
        if constexpr (PER_IMAGE) e.labels += b * plane;
        return e;
    }
};

// ---- crop + resample ----------------------------------------------------------------------------------------------------
// `images` windows of win_h x win_w, one per grid z, out of src [batch, src_h, src_w, channels] into dst [images, out_h, out_w,
// channels].  `scratch`: the erased windows on their way to the resample, null when there are none.
struct ResampleJob {
    int batch, src_h, src_w, channels, win_h, win_w, out_h, out_w, ksize_x, ksize_y;
    int64_t images;
    const float* src;
    const int32_t* bounds_x;
    const float* weights_x;
    const int32_t* bounds_y;
    const float* weights_y;
    float *dst, *scratch;
    bool same() const { return out_h == win_h && out_w == win_w; }
};

// One block: a 16 x 256 tile of window z's output (resample_tile.h).
template <class Window>
__global__ __launch_bounds__(256) void lp_detail_resample_kernel(const ResampleJob j, const Window win) {
    const int C = j.channels, z = blockIdx.z, rowE = j.out_w * C;
    int r, b, y0, x0;
    win.locate(z, j.batch, j.src_h, j.src_w, j.win_h, j.win_w, r, b, y0, x0);
    resample_tile<TorchAA>(j.src + ((static_cast<int64_t>(b) * j.src_h + y0) * j.src_w + x0) * C,
                           static_cast<int64_t>(j.src_w) * C, C, j.win_h, j.win_w, j.out_h, rowE, j.bounds_x, j.weights_x,
                           j.ksize_x, j.bounds_y, j.weights_y, j.ksize_y, j.dst + static_cast<int64_t>(z) * j.out_h * rowE);
}

// Same size in and out: the windows' rows copied as flat streams, one element per lane.  EraseForeign (C == 1): window z's view.
template <class Window, class Edit>
__global__ __launch_bounds__(256) void lp_detail_crop_kernel(const ResampleJob j, const Window win, const Edit edit) {
    const int C = j.channels, rowE = j.win_w * C;
    const int e = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (e >= rowE) return;
    int r, b, y0, x0;
    win.locate(z, j.batch, j.src_h, j.src_w, j.win_h, j.win_w, r, b, y0, x0);
    const int64_t at = static_cast<int64_t>(y0 + y) * j.src_w + x0;    // of the window row's first pixel in its plane
    const float v = j.src[(static_cast<int64_t>(b) * j.src_h * j.src_w + at) * C + e];
    j.dst[(static_cast<int64_t>(z) * j.win_h + y) * rowE + e] = edit.view(r, b, static_cast<int64_t>(j.src_h) * j.src_w)(v, at + e);
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

// detail [batch, win_h, win_w, channels] into the windows of out [batch, height, width, channels], one window per image.
struct StitchJob {
    int batch, height, width, channels, win_h, win_w, k, mask_batch;
    const float *mask, *original, *detail;
    float* out;
};

// A block owns a TH x TW tile of image b's window; tile origins are image coordinates, so the smoothed mask is the whole
// image's.  m goes to LDS, then the tile's rows are blended as flat streams of TW * C elements.  `edit` is how a mask element
// enters the passes (mask_tile.h): as it is, or with another region's components erased.  out may be original: one thread
// reads and writes a given element, and the halo is read from the mask alone.
template <int TH, int TW, class Window, class Edit>
__global__ __launch_bounds__(256) void lp_detail_stitch_kernel(const StitchJob j, const Window win, const Edit edit) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int k = j.k, tid = threadIdx.x;
    const int H = j.height, W = j.width, C = j.channels;
    int r, b, wy0, wx0;
    win.locate(blockIdx.z, j.batch, H, W, j.win_h, j.win_w, r, b, wy0, wx0);
    const int x0 = wx0 + blockIdx.x * TW, y0 = wy0 + blockIdx.y * TH;
    const float* mplane = j.mask + static_cast<int64_t>(j.mask_batch == 1 ? 0 : b) * H * W;
    float *D, *g;
    mask_tile_passes<TH, TW>(lds, mplane, H, W, LP_NN_ATEN_SCALAR, k, x0, y0, H, W, D, g,
                             edit.view(r, b, static_cast<int64_t>(H) * W));
    float* M = lds;                                               // the passes' A, free now: TH x TW smoothed mask
    for (int idx = tid; idx < TH * TW; idx += 256) {
        const int ty = idx / TW, tx = idx - ty * TW;
        M[idx] = smoothed_mask_at<TW>(D, g, k, ty, tx);
    }
    __syncthreads();
    const int ty_end = min(TH, wy0 + j.win_h - y0), tx_end = min(TW, wx0 + j.win_w - x0);
    const int rowE = tx_end * C;
    for (int idx = tid; idx < ty_end * rowE; idx += 256) {
        const int ty = idx / rowE, e = idx - ty * rowE;
        const float m = M[ty * TW + e / C];
        const int64_t io = ((static_cast<int64_t>(b) * H + y0 + ty) * W + x0) * C + e;
        const int64_t id = ((static_cast<int64_t>(b) * j.win_h + (y0 - wy0) + ty) * j.win_w + (x0 - wx0)) * C + e;
        j.out[io] = j.original[io] * (1.0f - m) + j.detail[id] * m;
    }
}

// ---- checks and launches, shared by the single, regions, track and subjects entries ----------------------------------------
bool side_ok(int s) { return s > 0 && s <= LP_DETAIL_MAX_SIDE; }
bool chan_ok(int c) { return c > 0 && c <= LP_DETAIL_MAX_CHANNELS; }
bool window_ok(int y0, int x0, int h, int w, int H, int W) {
    return y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && h <= H - y0 && w <= W - x0;
}
int launched() { return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH; }

// `at`: the descriptor's origin.  A table's windows are clamped on the device, so there only the size has to fit.
int check_resample(const ResampleJob& j, WindowAt at = {0, 0}) {
    if (j.batch <= 0 || !side_ok(j.src_h) || !side_ok(j.src_w) || !chan_ok(j.channels)) return LP_E_INVALID;
    if (!window_ok(at.y0, at.x0, j.win_h, j.win_w, j.src_h, j.src_w) || !side_ok(j.out_h) || !side_ok(j.out_w)) return LP_E_INVALID;
    if (!j.src || !j.dst) return LP_E_INVALID;
    if (!j.same()) {
        if (j.ksize_x <= 0 || j.ksize_y <= 0) return LP_E_INVALID;
        if (!j.bounds_x || !j.weights_x || !j.bounds_y || !j.weights_y) return LP_E_INVALID;
        if (!aligned16(j.dst) || !aligned16(j.scratch)) return LP_E_ALIGN;
    }
    return j.images > 65535 ? LP_E_UNSUPPORTED : LP_OK;          // the grid's z
}

int check_stitch(const StitchJob& j, WindowAt at = {0, 0}) {
    if (j.batch <= 0 || !side_ok(j.height) || !side_ok(j.width) || !chan_ok(j.channels)) return LP_E_INVALID;
    if (!window_ok(at.y0, at.x0, j.win_h, j.win_w, j.height, j.width)) return LP_E_INVALID;
    if (j.k < 1 || j.k > 51 || (j.k % 2) == 0) return LP_E_INVALID;
    if (j.mask_batch != 1 && j.mask_batch != j.batch) return LP_E_INVALID;
    if (!j.mask || !j.original || !j.detail || !j.out || j.out == j.original) return LP_E_INVALID;
    return j.batch > 65535 ? LP_E_UNSUPPORTED : LP_OK;
}

// The same-size copy of the job's windows into j.dst.
template <class Window, class Edit>
void launch_crop(const ResampleJob& j, Window win, Edit edit, hipStream_t stream) {
    const dim3 grid((j.win_w * j.channels + 255) / 256, j.win_h, static_cast<uint32_t>(j.images));
    hipLaunchKernelGGL((lp_detail_crop_kernel<Window, Edit>), grid, dim3(256), 0, stream, j, win, edit);
}

// The job's windows as they are in src: the resample tile, or the plain copy when the size stays.
template <class Window>
int launch_resample(const ResampleJob& j, Window win, hipStream_t stream) {
    if (j.same()) {
        launch_crop(j, win, MaskAsIs(), stream);
    } else {
        const dim3 grid((j.out_w * j.channels + kResampleTX - 1) / kResampleTX, (j.out_h + kResampleTY - 1) / kResampleTY,
                        static_cast<uint32_t>(j.images));
        hipLaunchKernelGGL(lp_detail_resample_kernel<Window>, grid, dim3(256), 0, stream, j, win);
    }
    return launched();
}

// A mask's windows as each window's owner sees them: erased on the way out when the size stays, otherwise erased into
// j.scratch and each resampled whole from there.
template <class Window, class Edit>
int launch_resample_erased(const ResampleJob& j, Window win, Edit erase, hipStream_t stream) {
    if (j.same()) {
        launch_crop(j, win, erase, stream);
        return launched();
    }
    ResampleJob crop = j, rest = j;
    crop.dst = j.scratch;
    launch_crop(crop, win, erase, stream);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    rest.batch = static_cast<int>(j.images);
    rest.src_h = j.win_h;
    rest.src_w = j.win_w;
    rest.src = j.scratch;
    return launch_resample(rest, WindowAt{0, 0}, stream);
}

// One streaming copy original -> out on `stream`, the first launch of every stitch.
hipError_t launch_frame_copy(const StitchJob& j, hipStream_t stream) {
    const int64_t n = static_cast<int64_t>(j.batch) * j.height * j.width * j.channels;
    const uint32_t blocks = static_cast<uint32_t>(min(static_cast<int64_t>(kCopyBlocks), (n + 1023) / 1024));
    if (aligned16(j.original) && aligned16(j.out))
        hipLaunchKernelGGL(lp_detail_copy_kernel<true>, dim3(blocks), dim3(256), 0, stream, j.original, j.out, n);
    else                                                          // a frame range of a larger tensor need not start on 16 bytes
        hipLaunchKernelGGL(lp_detail_copy_kernel<false>, dim3(blocks), dim3(256), 0, stream, j.original, j.out, n);
    return hipGetLastError();
}

template <int TH, int TW, class Window, class Edit>
hipError_t launch_stitch_tiles(const StitchJob& j, Window win, Edit edit, hipStream_t stream) {
    const auto kernel = lp_detail_stitch_kernel<TH, TW, Window, Edit>;
    const size_t lds = mask_tile_lds_bytes<TH, TW>(j.k);
    if (lds > 64 * 1024)                                          // per device, like lp_mask_blend
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const dim3 grid((j.win_w + TW - 1) / TW, (j.win_h + TH - 1) / TH, j.batch);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, j, win, edit);
    return hipGetLastError();
}

// The blend of every image's window, in place on j.out when j.original is j.out.
template <class Window, class Edit>
int launch_stitch(const StitchJob& j, Window win, Edit edit, hipStream_t stream) {
    const hipError_t err = (j.k <= 15) ? launch_stitch_tiles<16, 64>(j, win, edit, stream)
                                       : launch_stitch_tiles<8, 32>(j, win, edit, stream);
    return err == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

// The regions and the subjects crop: `groups` windows per image (the descriptor's `count`), origins from a device table read
// by `Window`, a mask's windows through `Erase` when the descriptor has labels.  The two descriptors differ in that field's name.
template <class Window, class Erase, class Desc>
int resample_groups_dispatch(const Desc* dp, int Desc::*count, hipStream_t stream) {
    if (!dp) return LP_E_INVALID;
    const Desc& d = *dp;
    const int groups = d.*count;
    if (groups < 1 || groups > LP_DETAIL_MAX_REGIONS || !d.origins) return LP_E_INVALID;
    ResampleJob j = {d.batch, d.src_h, d.src_w, d.channels, d.win_h, d.win_w, d.out_h, d.out_w, d.ksize_x, d.ksize_y,
                     static_cast<int64_t>(groups) * d.batch, d.src, d.bounds_x, d.weights_x, d.bounds_y, d.weights_y, d.dst,
                     nullptr};
    const bool erased_resample = d.labels && !j.same();          // erased windows go to scratch, the resample reads them there
    if (d.labels && (d.channels != 1 || !d.owner || d.owner_len < 1 || (erased_resample && !d.scratch))) return LP_E_INVALID;
    if (erased_resample) j.scratch = d.scratch;
    if (const int err = check_resample(j)) return err;
    const Window win = {d.origins};
    if (!d.labels) return launch_resample(j, win, stream);
    return launch_resample_erased(j, win, Erase{d.labels, d.owner, d.owner_len, 1}, stream);
}

// The regions and the subjects stitch, after each entry's own checks: one copy of the frames, then group after group in order
// and in place, out_{g+1} from out_g; group g's windows are where `window_of(g)` says and see the mask through `Erase`.
template <class Erase, class Desc, class WindowOf>
int stitch_groups(StitchJob j, const Desc& d, int groups, WindowOf window_of, hipStream_t stream) {
    if (launch_frame_copy(j, stream) != hipSuccess) return LP_E_LAUNCH;
    const int64_t per_group = static_cast<int64_t>(d.batch) * d.win_h * d.win_w * d.channels;
    j.original = d.out;
    for (int g = 0; g < groups; ++g, j.detail += per_group) {
        const auto win = window_of(g);
        const int err = d.labels ? launch_stitch(j, win, Erase{d.labels, d.owner, d.owner_len, g + 1}, stream)
                                 : launch_stitch(j, win, MaskAsIs(), stream);
        if (err) return err;
    }
    return LP_OK;
}

// lp_mask_bbox (one box over every plane) and lp_mask_bbox_frames (a box per plane)
int mask_bbox(const float* mask, int planes, int H, int W, int32_t* boxes, bool per_plane, hipStream_t stream) {
    if (!mask || !boxes || planes <= 0 || !side_ok(H) || !side_ok(W)) return LP_E_INVALID;
    if (planes > 65535) return LP_E_UNSUPPORTED;
    const int n = per_plane ? planes : 1;
    hipLaunchKernelGGL(lp_detail_bbox_init_kernel, dim3((4 * n + 255) / 256), dim3(256), 0, stream, boxes, H, W, n);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    const bool vec = (W & 3) == 0 && aligned16(mask);              // then every plane starts on 16 bytes too
    const dim3 grid(vec ? (W + 1023) / 1024 : (W + 255) / 256, (H + kBboxRows - 1) / kBboxRows, planes);
    const auto kernel = vec ? (per_plane ? lp_detail_bbox_kernel<4, true> : lp_detail_bbox_kernel<4, false>)
                            : (per_plane ? lp_detail_bbox_kernel<1, true> : lp_detail_bbox_kernel<1, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, mask, boxes, H, W);
    return launched();
}

}  // namespace

extern "C" int lp_mask_bbox(const float* mask, int32_t planes, int32_t height, int32_t width, int32_t* bbox, void* stream) {
    return mask_bbox(mask, planes, height, width, bbox, false, as_stream(stream));
}

extern "C" int lp_mask_bbox_frames(const float* mask, int32_t planes, int32_t height, int32_t width, int32_t* boxes, void* stream) {
    return mask_bbox(mask, planes, height, width, boxes, true, as_stream(stream));
}

extern "C" int lp_detail_resample(const lp_detail_resample_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_detail_resample_desc& d = *dp;
    const ResampleJob j = {d.batch, d.src_h, d.src_w, d.channels, d.win_h, d.win_w, d.out_h, d.out_w, d.ksize_x, d.ksize_y,
                           d.batch, d.src, d.bounds_x, d.weights_x, d.bounds_y, d.weights_y, d.dst, nullptr};
    const WindowAt at = {d.y0, d.x0};
    if (const int err = check_resample(j, at)) return err;
    return launch_resample(j, at, stream);
}

extern "C" int lp_detail_stitch(const lp_detail_stitch_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_detail_stitch_desc& d = *dp;
    const StitchJob j = {d.batch, d.height, d.width, d.channels, d.win_h, d.win_w, d.k, d.mask_batch, d.mask, d.original,
                         d.detail, d.out};
    const WindowAt at = {d.y0, d.x0};
    if (const int err = check_stitch(j, at)) return err;
    if (launch_frame_copy(j, stream) != hipSuccess) return LP_E_LAUNCH;
    return launch_stitch(j, at, MaskAsIs(), stream);
}

extern "C" int lp_detail_resample_regions(const lp_detail_resample_regions_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    return resample_groups_dispatch<WindowOfRegion, EraseForeign<false>>(dp, &lp_detail_resample_regions_desc::regions, stream);
}

extern "C" int lp_detail_stitch_regions(const lp_detail_stitch_regions_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_detail_stitch_regions_desc& d = *dp;
    if (d.regions < 1 || d.regions > LP_DETAIL_MAX_REGIONS || !d.origins) return LP_E_INVALID;
    for (int r = 0; r < d.regions; ++r)                           // a host table: checked here, not clamped
        if (!window_ok(d.origins[2 * r], d.origins[2 * r + 1], d.win_h, d.win_w, d.height, d.width)) return LP_E_INVALID;
    if (d.labels && (!d.owner || d.owner_len < 1)) return LP_E_INVALID;
    const StitchJob j = {d.batch, d.height, d.width, d.channels, d.win_h, d.win_w, d.k, d.mask_batch, d.mask, d.original,
                         d.detail, d.out};
    if (const int err = check_stitch(j)) return err;
    const auto window_of = [&d](int r) { return WindowAt{d.origins[2 * r], d.origins[2 * r + 1]}; };      // checked above
    return stitch_groups<EraseForeign<false>>(j, d, d.regions, window_of, stream);
}

extern "C" int lp_subject_boxes(const int32_t* labels, int32_t frames, int32_t H, int32_t W, const int32_t* owner, int32_t owner_len,
                                int32_t subjects, int32_t* boxes, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!labels || !owner || !boxes || frames <= 0 || !side_ok(H) || !side_ok(W) || owner_len < 1) return LP_E_INVALID;
    if (subjects < 1 || subjects > LP_DETAIL_MAX_REGIONS) return LP_E_INVALID;
    if (frames > 65535) return LP_E_UNSUPPORTED;
    const int n = subjects * frames;
    hipLaunchKernelGGL(lp_detail_bbox_init_kernel, dim3((4 * n + 255) / 256), dim3(256), 0, stream, boxes, H, W, n);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    const dim3 grid((W + 255) / 256, (H + kBboxRows - 1) / kBboxRows, frames);
    hipLaunchKernelGGL(lp_detail_subject_boxes_kernel, grid, dim3(256), 0, stream, labels, owner, owner_len, subjects, boxes, H, W);
    return launched();
}

extern "C" int lp_detail_resample_subjects(const lp_detail_resample_subjects_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    return resample_groups_dispatch<WindowOfSubject, EraseForeign<true>>(dp, &lp_detail_resample_subjects_desc::subjects, stream);
}

extern "C" int lp_detail_stitch_subjects(const lp_detail_stitch_subjects_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_detail_stitch_subjects_desc& d = *dp;
    if (d.subjects < 1 || d.subjects > LP_DETAIL_MAX_REGIONS || !d.origins) return LP_E_INVALID;
    if (d.labels && (!d.owner || d.owner_len < 1)) return LP_E_INVALID;
    const StitchJob j = {d.batch, d.height, d.width, d.channels, d.win_h, d.win_w, d.k, d.batch, d.mask, d.original, d.detail, d.out};
    if (const int err = check_stitch(j)) return err;
    const auto window_of = [&d](int s) { return WindowOfImage{d.origins + 2 * static_cast<int64_t>(s) * d.batch}; };   // s's row
    return stitch_groups<EraseForeign<true>>(j, d, d.subjects, window_of, stream);
}

extern "C" int lp_detail_resample_track(const lp_detail_resample_track_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_detail_resample_track_desc& d = *dp;
    if (!d.origins) return LP_E_INVALID;
    const ResampleJob j = {d.batch, d.src_h, d.src_w, d.channels, d.win_h, d.win_w, d.out_h, d.out_w, d.ksize_x, d.ksize_y,
                           d.batch, d.src, d.bounds_x, d.weights_x, d.bounds_y, d.weights_y, d.dst, nullptr};
    if (const int err = check_resample(j)) return err;
    return launch_resample(j, WindowOfImage{d.origins}, stream);
}

extern "C" int lp_detail_stitch_track(const lp_detail_stitch_track_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_detail_stitch_track_desc& d = *dp;
    if (!d.origins) return LP_E_INVALID;
    const StitchJob j = {d.batch, d.height, d.width, d.channels, d.win_h, d.win_w, d.k, d.mask_batch, d.mask, d.original,
                         d.detail, d.out};
    if (const int err = check_stitch(j)) return err;
    if (launch_frame_copy(j, stream) != hipSuccess) return LP_E_LAUNCH;
    return launch_stitch(j, WindowOfImage{d.origins}, MaskAsIs(), stream);
}

}  // namespace lp
