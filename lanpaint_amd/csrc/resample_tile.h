// resample_tile.h -- one tile of a separable, table-driven two-pass resize, shared by lp_vmask_resize (videomask_kernel.hip:
// Pillow's 8-bit BILINEAR) and lp_detail_resample (detail_kernel.hip: torch's antialiased bilinear / bicubic in fp32).
//
// Rows are flat streams: element e of a row is column e / C, channel e % C (C = 1 for a single-plane image).  The host builds
// per axis a bounds table [out, 2] = (first source index, tap count) and a weights table [out, ksize].  Both passes run in
// one launch: a block stages the horizontal pass of the source rows its output tile needs in LDS, then the vertical pass
// writes fp32, 16 B per lane.  What the two callers do differently is a policy type P, fixed at compile time:
//   P::Src, P::Weight     element types of the source image and of the weights tables
//   P::Acc                type of a sum;  P::acc0() its start value
//   P::hsum(s, w, n, C)   one horizontal sum: taps s[t * C] * w[t], t = 0 .. n - 1, ascending
//   P::Staged             four horizontal sums of one lane as they are parked in LDS;  P::pack(v) makes one
//   P::tap(p, j)          component j of a staged value, as the vertical pass multiplies it
//   P::finish(acc)        a finished vertical sum -> the fp32 written out
// 256 threads.
#pragma once
#include "lp_common.h"

namespace lp {

constexpr int kResampleTX = 256;    // tile: 64 lanes x 4 flat elements of the output row ...
constexpr int kResampleTY = 16;     // ... by 16 output rows, 4 waves of 4 rows each
constexpr int kResampleCR = 32;     // source rows staged in LDS per chunk

// A table entry clamped to the source, so a bad table reads nothing outside it.
__device__ __forceinline__ void tap_window(const int32_t* __restrict__ bounds, int i, int ksize, int in_size, int& first,
                                           int& count) {
    first = min(max(bounds[2 * i], 0), in_size - 1);
    count = min(max(bounds[2 * i + 1], 0), min(ksize, in_size - first));
}

// One block: output rows [yy0, yy0 + 16) x flat elements [e0, e0 + 256) of one image, yy0 and e0 from blockIdx.y / .x.  Lane l
// of wave w owns elements e0 + 4l .. +3 and output rows yy0 + w + 4r (r < 4).  The source rows those output rows read,
// [ylo, yhi), go through LDS in chunks of 32: horizontal pass of the chunk, then each thread adds the chunk's rows that fall
// in its rows' windows -- chunks ascend, so the vertical taps do too.
// `src`: element (0, 0) of the in_h x in_w source window, its rows `sstride` elements apart;  `dst`: the image's out_h rows
// of rowE = out_w * C elements, 16 B aligned when rowE % 4 == 0.
template <class P>
__device__ __forceinline__ void resample_tile(const typename P::Src* src, int64_t sstride, int C, int inH, int inW, int outH,
                                              int rowE, const int32_t* bounds_x, const typename P::Weight* weights_x, int kx,
                                              const int32_t* bounds_y, const typename P::Weight* weights_y, int ky, float* dst) {
    __shared__ typename P::Staged stage[kResampleCR][kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int e0 = blockIdx.x * kResampleTX + lane * 4, yy0 = blockIdx.y * kResampleTY;

    int ylo = inH, yhi = 0;                                       // source rows of the whole tile
    for (int r = 0; r < kResampleTY && yy0 + r < outH; ++r) {
        int b0, b1;
        tap_window(bounds_y, yy0 + r, ky, inH, b0, b1);
        ylo = min(ylo, b0);
        yhi = max(yhi, b0 + b1);
    }
    int rmin[4], rcnt[4];
    typename P::Acc acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int yy = yy0 + wave + 4 * r;
        rmin[r] = 0; rcnt[r] = 0;
        if (yy < outH) tap_window(bounds_y, yy, ky, inH, rmin[r], rcnt[r]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[r][j] = P::acc0();
    }
    int soff[4], ccnt[4], wbase[4];                               // first tap's offset in the source row, taps, table row
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        soff[j] = 0; ccnt[j] = 0; wbase[j] = 0;
        if (e0 + j < rowE) {
            const int xx = (e0 + j) / C, c = (e0 + j) - xx * C;
            int first;
            tap_window(bounds_x, xx, kx, inW, first, ccnt[j]);
            soff[j] = first * C + c;
            wbase[j] = xx * kx;
        }
    }

    for (int c0 = ylo; c0 < yhi; c0 += kResampleCR) {
        const int rows = min(kResampleCR, yhi - c0);
        for (int rr = wave; rr < rows; rr += 4) {                 // horizontal pass of the chunk
            const typename P::Src* srow = src + static_cast<int64_t>(c0 + rr) * sstride;
            typename P::Acc v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = P::hsum(srow + soff[j], weights_x + wbase[j], ccnt[j], C);
            stage[rr][lane] = P::pack(v);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {                            // vertical pass: this chunk's share of each row's sum
            const int t0 = max(rmin[r], c0), t1 = min(rmin[r] + rcnt[r], c0 + rows);
            const typename P::Weight* w = weights_y + static_cast<int64_t>(yy0 + wave + 4 * r) * ky - rmin[r];
            for (int t = t0; t < t1; ++t) {
                const typename P::Staged p = stage[t - c0][lane];
                const typename P::Weight wt = w[t];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[r][j] += P::tap(p, j) * wt;
            }
        }
        __syncthreads();
    }

    const bool vec = (rowE & 3) == 0 && e0 + 3 < rowE;           // dst rows then start 16 B aligned
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int yy = yy0 + wave + 4 * r;
        if (yy >= outH) continue;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = P::finish(acc[r][j]);
        float* o = dst + static_cast<int64_t>(yy) * rowE + e0;
        if (vec) {
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j < rowE) o[j] = v[j];
        }
    }
}

}  // namespace lp
