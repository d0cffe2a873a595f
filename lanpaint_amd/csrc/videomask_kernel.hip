// videomask_kernel.hip -- the video mask editor's per-frame masks on gfx950 (reference
// src/LanPaint/videomask.py, nodes.py:890-995).  Three jobs, each a handful of launches on the caller's stream:
//
//   lp_vmask_edt     binarise every keyframe (k >= 0.5), exact squared EDT to the nearest foreground AND to the nearest
//                    background pixel (separable: a column scan per lane, then Meijster's linear-time lower envelope per
//                    row in LDS), the fp64 SDF sqrt(d2_bg) - sqrt(d2_fg), and exact integer centroid sums;
//   lp_vmask_morph   one launch over [frames, h, w] driven by a per-frame table the host builds (zero / keyframe / inner
//                    frame with its blend weights and whole-pixel shifts): the fp64 SDF blend + sigmoid, written as fp32 or
//                    directly as the uint8 codes the resize reads;
//   lp_vmask_resize  Pillow's 8-bit two-pass BILINEAR from host-built coefficient tables, both passes in one launch: a block
//                    stages the horizontal pass of the source rows its output tile needs in LDS, then runs the vertical
//                    pass and writes fp32 -- the only large tensor, written once, 16 B per lane.
// Entry points defined here: lp_vmask_edt, lp_vmask_morph, lp_vmask_resize.
#include "lp_common.h"
#include "resample_tile.h"

namespace lp {
namespace {

constexpr int kColBlock = 64;       // EDT column pass: one lane per column
constexpr int kRowBlock = 64;       // EDT row pass: one wave per row (the envelope is built by lane 0)
constexpr int kColUnroll = 16;      // rows whose loads the column pass issues back to back
constexpr int kPrec = 22;           // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)

// ---- EDT column pass ---------------------------------------------------------------------------------------------------
// Lane = (key, column x).  Forward scan: distance to the nearest foreground / background pixel at or above y; backward scan
// folds in the one below and stores the squared 1-D distance (LP_VMASK_D2_NONE when the column holds no such pixel), plane 0
// = foreground, plane 1 = background.  Rows step by W: every row access of a wave is one coalesced 256 B line.  The
// per-column foreground count and row sum go to the key's centroid sums through one wave reduction and three atomics.
__global__ __launch_bounds__(kColBlock) void lp_vmask_col_kernel(const float* __restrict__ keys, int32_t* __restrict__ d2,
                                                                 unsigned long long* __restrict__ csum, int H, int W) {
    const int x = blockIdx.x * kColBlock + threadIdx.x;
    const int k = blockIdx.y;
    const int64_t plane = static_cast<int64_t>(H) * W;
    const int far = H + W;                                   // larger than any in-column distance
    unsigned long long cnt = 0, sy = 0;
    if (x < W) {
        const float* col = keys + static_cast<int64_t>(k) * plane + x;
        int32_t* pf = d2 + static_cast<int64_t>(k) * 2 * plane + x;
        int32_t* pb = pf + plane;
        int last_f = -far, last_b = -far;
        for (int y0 = 0; y0 < H; y0 += kColUnroll) {
            float v[kColUnroll];
#pragma unroll
            for (int j = 0; j < kColUnroll; ++j) v[j] = (y0 + j < H) ? col[static_cast<int64_t>(y0 + j) * W] : 0.0f;
#pragma unroll
            for (int j = 0; j < kColUnroll; ++j) {
                const int y = y0 + j;
                if (y < H) {
                    if (v[j] >= 0.5f) { last_f = y; ++cnt; sy += static_cast<unsigned long long>(y); } else { last_b = y; }
                    pf[static_cast<int64_t>(y) * W] = y - last_f;
                    pb[static_cast<int64_t>(y) * W] = y - last_b;
                }
            }
        }
        int next_f = 2 * far, next_b = 2 * far;
        for (int y1 = H; y1 > 0; y1 -= kColUnroll) {
            int uf[kColUnroll], ub[kColUnroll];
#pragma unroll
            for (int j = 0; j < kColUnroll; ++j) {
                const int y = y1 - 1 - j;
                uf[j] = y >= 0 ? pf[static_cast<int64_t>(y) * W] : 0;
                ub[j] = y >= 0 ? pb[static_cast<int64_t>(y) * W] : 0;
            }
#pragma unroll
            for (int j = 0; j < kColUnroll; ++j) {
                const int y = y1 - 1 - j;
                if (y >= 0) {
                    if (uf[j] == 0) next_f = y;
                    if (ub[j] == 0) next_b = y;
                    const int df = min(uf[j], next_f - y), db = min(ub[j], next_b - y);
                    pf[static_cast<int64_t>(y) * W] = df < far ? df * df : LP_VMASK_D2_NONE;
                    pb[static_cast<int64_t>(y) * W] = db < far ? db * db : LP_VMASK_D2_NONE;
                }
            }
        }
    }
    unsigned long long sx = cnt * static_cast<unsigned long long>(x < W ? x : 0);
    for (int off = kWave / 2; off > 0; off >>= 1) {
        cnt += __shfl_down(cnt, off);
        sy += __shfl_down(sy, off);
        sx += __shfl_down(sx, off);
    }
    if (threadIdx.x == 0 && cnt) {
        atomicAdd(csum + 3 * k + 0, cnt);
        atomicAdd(csum + 3 * k + 1, sy);
        atomicAdd(csum + 3 * k + 2, sx);
    }
}

// ---- EDT row pass -----------------------------------------------------------------------------------------------------
// d2(x) = min over columns u of g(u)^2 + (x - u)^2 with g the column pass's distance.  Meijster, Roerdink & Hesselink's lower
// envelope in integer arithmetic (exact; every term < 2^31 for sides <= 16384): lane 0 builds the envelope in one O(W) sweep
// over the row held in LDS -- columns without a pixel of the plane's kind do not enter it -- then every lane reads its
// columns' parabola by binary search over the segment starts.  Written back in place.
__global__ __launch_bounds__(kRowBlock) void lp_vmask_row_kernel(int32_t* __restrict__ d2, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    int32_t* G = lds + 4;                                         // lds[0]: envelope top
    uint16_t* S = reinterpret_cast<uint16_t*>(G + W);             // parabola apex columns
    uint16_t* T = S + W;                                          // first column where that parabola is the minimum
    const int y = blockIdx.x, plane = blockIdx.y, k = blockIdx.z;
    int32_t* row = d2 + ((static_cast<int64_t>(k) * 2 + plane) * H + y) * W;
    for (int x = threadIdx.x; x < W; x += kRowBlock) G[x] = row[x];
    __syncthreads();
    if (threadIdx.x == 0) {
        int q = -1, sq = 0, tq = 0, gsq = 0;                      // the top entry, kept in registers
        for (int u = 0; u < W; ++u) {
            const int gu = G[u];
            if (gu < 0) continue;
            while (q >= 0 && (tq - sq) * (tq - sq) + gsq > (tq - u) * (tq - u) + gu) {
                if (--q >= 0) { sq = S[q]; tq = T[q]; gsq = G[sq]; }
            }
            if (q < 0) {
                q = 0; sq = u; tq = 0; gsq = gu;
                S[0] = static_cast<uint16_t>(u); T[0] = 0;
            } else {
                // the envelope keeps s_q on [t_q, sep]; here sep >= t_q >= 0, so '/' truncating is the floor
                const int w = 1 + (u * u - sq * sq + gu - gsq) / (2 * (u - sq));
                if (w < W) {
                    ++q; sq = u; tq = w; gsq = gu;
                    S[q] = static_cast<uint16_t>(u); T[q] = static_cast<uint16_t>(w);
                }
            }
        }
        lds[0] = q;
    }
    __syncthreads();
    const int q = lds[0];
    for (int x = threadIdx.x; x < W; x += kRowBlock) {
        int out = LP_VMASK_D2_NONE;
        if (q >= 0) {
            int lo = 0, hi = q;                                   // last segment with T[j] <= x (T[0] = 0)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (T[mid] <= x) lo = mid; else hi = mid - 1;
            }
            const int s = S[lo];
            out = (x - s) * (x - s) + G[s];
        }
        row[x] = out;
    }
}

// ---- SDF ----------------------------------------------------------------------------------------------------------------
// sdf = sqrt(d2_bg) - sqrt(d2_fg) in fp64 (correctly rounded sqrt: equal to scipy's distance_transform_edt); a keyframe with
// no foreground gets -max(h, w)/2, one with no background +max(h, w)/2 (videomask.py _signed_distance).
__global__ __launch_bounds__(256) void lp_vmask_sdf_kernel(const int32_t* __restrict__ d2,
                                                           const unsigned long long* __restrict__ csum,
                                                           double* __restrict__ sdf, int H, int W) {
    const int64_t plane = static_cast<int64_t>(H) * W;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= plane) return;
    const unsigned long long n = csum[3 * k];
    const double half = static_cast<double>(max(H, W)) / 2.0;
    double v;
    if (n == 0) {
        v = -half;
    } else if (n == static_cast<unsigned long long>(plane)) {
        v = half;
    } else {
        const int32_t* p = d2 + static_cast<int64_t>(k) * 2 * plane + i;
        v = sqrt(static_cast<double>(p[plane])) - sqrt(static_cast<double>(p[0]));
    }
    sdf[static_cast<int64_t>(k) * plane + i] = v;
}

// ---- morph --------------------------------------------------------------------------------------------------------------
// S(f, dy, dx)(y, x) = f(y - dy, x - dx), 0 where that falls outside the frame (the reference's _shift fills vacated pixels
// with 0, not with "outside").
__device__ __forceinline__ double shifted(const double* f, int64_t y, int64_t x, int H, int W) {
    return (y >= 0 && y < H && x >= 0 && x < W) ? f[y * W + x] : 0.0;
}

__global__ __launch_bounds__(256) void lp_vmask_morph_kernel(const lp_vmask_morph_desc d) {
#pragma clang fp contract(off)
    const int H = d.height, W = d.width;
    const int64_t plane = static_cast<int64_t>(H) * W;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int f = blockIdx.y;
    if (i >= plane) return;
    const lp_vmask_frame fr = d.frames[f];
    const bool lo_ok = fr.key_lo >= 0 && fr.key_lo < d.n_keys, hi_ok = fr.key_hi >= 0 && fr.key_hi < d.n_keys;
    float m = 0.0f;                                              // a table entry naming no key reads nothing
    if (fr.kind == LP_VMASK_KEY && lo_ok) {
        m = d.keys[static_cast<int64_t>(fr.key_lo) * plane + i];
    } else if (fr.kind == LP_VMASK_INNER && d.sdf && lo_ok && hi_ok) {
        const int64_t y = i / W, x = i - y * W;
        const double a = shifted(d.sdf + static_cast<int64_t>(fr.key_lo) * plane, y - fr.sy1, x - fr.sx1, H, W);
        const double b = shifted(d.sdf + static_cast<int64_t>(fr.key_hi) * plane, y + fr.sy2, x + fr.sx2, H, W);
        // (1 - wf) * a + wf * b with each product and the sum rounded on its own, as numpy evaluates it
        double v = __dadd_rn(__dmul_rn(fr.omw, a), __dmul_rn(fr.wf, b));
        v = v < -50.0 ? -50.0 : (v > 50.0 ? 50.0 : v);
        m = static_cast<float>(1.0 / (1.0 + exp(-v)));
    }
    const int64_t o = static_cast<int64_t>(f) * plane + i;
    if (d.flags & LP_VMASK_OUT_U8)
        static_cast<uint8_t*>(d.out)[o] = static_cast<uint8_t>(static_cast<int>(m * 255.0f));   // (m * 255).astype(uint8)
    else
        static_cast<float*>(d.out)[o] = m;
}

// ---- resize -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t clip8(int ss) {
    return ss >= (1 << kPrec << 8) ? 255u : (ss <= 0 ? 0u : static_cast<uint32_t>(ss >> kPrec));
}

// Pillow's 8-bit passes for resample_tile: uint8 source, 22-bit fixed-point sums that start at one half, and the horizontal
// pass parked as four clipped bytes (Pillow's uint8 intermediate image) in one dword.  Integer sums: exact in any order.
struct Pillow8 {
    using Src = uint8_t;
    using Weight = int32_t;
    using Acc = int;
    using Staged = uint32_t;
    static __device__ __forceinline__ int acc0() { return 1 << (kPrec - 1); }
    static __device__ __forceinline__ int hsum(const uint8_t* s, const int32_t* w, int n, int C) {
        int ss = acc0();
        for (int t = 0; t < n; ++t) ss += static_cast<int>(s[t * C]) * w[t];
        return ss;
    }
    static __device__ __forceinline__ uint32_t pack(const int (&v)[4]) {
        return clip8(v[0]) | clip8(v[1]) << 8 | clip8(v[2]) << 16 | clip8(v[3]) << 24;
    }
    static __device__ __forceinline__ int tap(uint32_t p, int j) { return static_cast<int>((p >> (8 * j)) & 255u); }
    static __device__ __forceinline__ float finish(int acc) { return static_cast<float>(clip8(acc)) / 255.0f; }
};

// One block: a 16 x 256 tile of frame f (resample_tile.h; a frame is one plane, C = 1).
__global__ __launch_bounds__(256) void lp_vmask_resize_kernel(const lp_vmask_resize_desc d) {
    const int f = blockIdx.z;
    resample_tile<Pillow8>(d.src + static_cast<int64_t>(f) * d.in_h * d.in_w, d.in_w, 1, d.in_h, d.in_w, d.out_h, d.out_w,
                           d.bounds_x, d.weights_x, d.ksize_x, d.bounds_y, d.weights_y, d.ksize_y,
                           d.dst + static_cast<int64_t>(f) * d.out_h * d.out_w);
}

bool side_ok(int s) { return s > 0 && s <= LP_VMASK_MAX_SIDE; }

}  // namespace

extern "C" int lp_vmask_edt(const lp_vmask_edt_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_vmask_edt_desc& d = *dp;
    if (d.n_keys <= 0 || !side_ok(d.height) || !side_ok(d.width)) return LP_E_INVALID;
    if (!d.keys || !d.d2 || !d.sdf || !d.csum) return LP_E_INVALID;
    if (d.n_keys > 65535) return LP_E_UNSUPPORTED;
    const int H = d.height, W = d.width, K = d.n_keys;
    auto* csum = reinterpret_cast<unsigned long long*>(d.csum);
    if (hipMemsetAsync(csum, 0, sizeof(uint64_t) * 3 * static_cast<size_t>(K), stream) != hipSuccess) return LP_E_LAUNCH;
    hipLaunchKernelGGL(lp_vmask_col_kernel, dim3((W + kColBlock - 1) / kColBlock, K), dim3(kColBlock), 0, stream,
                       d.keys, d.d2, csum, H, W);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    const size_t lds = 16 + static_cast<size_t>(W) * (sizeof(int32_t) + 2 * sizeof(uint16_t));   // <= 128 KiB + 16
    if (lds > 64 * 1024 &&                                       // a refused opt-in is this job's error, not a later launch's
        hipFuncSetAttribute(reinterpret_cast<const void*>(&lp_vmask_row_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        return LP_E_LAUNCH;
    hipLaunchKernelGGL(lp_vmask_row_kernel, dim3(H, 2, K), dim3(kRowBlock), lds, stream, d.d2, H, W);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    const int64_t plane = static_cast<int64_t>(H) * W;
    hipLaunchKernelGGL(lp_vmask_sdf_kernel, dim3(static_cast<uint32_t>((plane + 255) / 256), K), dim3(256), 0, stream,
                       d.d2, csum, d.sdf, H, W);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

extern "C" int lp_vmask_morph(const lp_vmask_morph_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_vmask_morph_desc& d = *dp;
    if (d.n_frames <= 0 || d.n_keys <= 0 || !side_ok(d.height) || !side_ok(d.width)) return LP_E_INVALID;
    if (!d.frames || !d.keys || !d.out || (d.flags & ~static_cast<uint32_t>(LP_VMASK_OUT_U8))) return LP_E_INVALID;
    if (d.n_frames > 65535) return LP_E_UNSUPPORTED;
    const int64_t plane = static_cast<int64_t>(d.height) * d.width;
    hipLaunchKernelGGL(lp_vmask_morph_kernel, dim3(static_cast<uint32_t>((plane + 255) / 256), d.n_frames), dim3(256), 0,
                       stream, d);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

extern "C" int lp_vmask_resize(const lp_vmask_resize_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_vmask_resize_desc& d = *dp;
    if (d.n_frames <= 0 || !side_ok(d.in_h) || !side_ok(d.in_w) || !side_ok(d.out_h) || !side_ok(d.out_w)) return LP_E_INVALID;
    if (d.ksize_x <= 0 || d.ksize_y <= 0) return LP_E_INVALID;
    if (!d.src || !d.dst || !d.bounds_x || !d.weights_x || !d.bounds_y || !d.weights_y) return LP_E_INVALID;
    if (d.n_frames > 65535) return LP_E_UNSUPPORTED;
    const dim3 grid((d.out_w + kResampleTX - 1) / kResampleTX, (d.out_h + kResampleTY - 1) / kResampleTY, d.n_frames);
    hipLaunchKernelGGL(lp_vmask_resize_kernel, grid, dim3(256), 0, stream, d);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

}  // namespace lp
