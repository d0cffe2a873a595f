// color_kernel.hip -- Detailer colour match for gfx950: undo the gain and offset a crop picks up on its way through resample,
// VAE and sampler, measured where the decoded crop and the original crop show the same thing (outside the mask).  Pixel space,
// once per job, between decode and stitch (lanpaint_amd/detail_color.py).  Three jobs on the caller's stream:
//
//   lp_color_stats  per image {n, per channel sum d, sum r, sum d^2, sum r^2} over the pixels whose (2 margin + 1)^2 neighbourhood
//                   of the mask is all <= 0.5.  A streaming read of two images and one mask: a block owns a 32 x 128 tile, holds
//                   the mask's halo as one bit per element in LDS (a row of 256 columns is one 16 B load per lane of a wave),
//                   widens the bits by `margin` along x and then along y with word shifts, and adds its pixels in fp64 -- a lane
//                   takes 4 neighbouring pixels of 4 rows, 16 B per load.  One partial row per block goes to the workspace; a
//                   second launch folds an image's rows in a fixed order.  No floating-point atomics: the same bits every run.
//   lp_color_fit    one thread per (image, channel): pool the rows of the frames in the window, moments, gain, bias, strength.
//   lp_color_apply  out = d * gain + bias, unfused, 16 B per lane.
//
// The library is built with -ffp-contract=on: every fp64 step whose fusing would change a bit goes through __dmul_rn / __dadd_rn
// and friends, one operation per call.
// Entry points defined here: lp_color_stats, lp_color_fit, lp_color_apply.
#include "lp_common.h"

namespace lp {
namespace {

constexpr int kTH = LP_COLOR_TILE_H, kTW = LP_COLOR_TILE_W;
constexpr int kMaxM = LP_COLOR_MAX_MARGIN;
constexpr int kHaloRows = kTH + 2 * kMaxM;      // mask rows a tile can need
constexpr int kRowsPerPass = 256 / (kTW / 4);   // 8: a lane owns 4 pixels of a row, 32 lanes a row, the block 8 rows per pass
constexpr int kApplyBlocks = 65535;

static_assert(kTW == 128 && kTH % kRowsPerPass == 0 && kMaxM < 64, "the bit rows below are 4 words: 64 | tile 128 | 64 columns");

// ---- statistics -----------------------------------------------------------------------------------------------------------
// Bit (64 + tx) of row r of `bits` <-> mask element (y0 - margin + r, x0 + tx) is NOT <= 0.5 (a NaN drops the pixel, as the
// rule's "every element <= 0.5" does); elements outside the image are 0: they do not count.  One wave per row: lane l loads
// columns x0 - 64 + 4 l .. + 3, as one float4 when the plane's rows start on 16 bytes (MVEC), and 8 lanes gather their nibbles
// into a 32-bit word by three xor-shuffles.
__device__ __forceinline__ void load_mask_bits(const float* __restrict__ plane, int H, int W, int y0, int x0, int margin, bool mvec,
                                               uint32_t (*bits)[8]) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int rows = kTH + 2 * margin;
    const int col = x0 - 64 + 4 * lane;
    const bool wanted = col + 3 >= x0 - margin && col <= x0 + kTW - 1 + margin;     // this lane's columns touch the halo
    for (int r = wave; r < rows; r += 4) {
        const int y = y0 - margin + r;
        uint32_t nib = 0;
        if (wanted && y >= 0 && y < H) {
            const float* p = plane + static_cast<int64_t>(y) * W + col;
            if (mvec) {                                            // W % 4 == 0 and col % 4 == 0: all four inside or none
                if (col >= 0 && col < W) {
                    const float4 q = *reinterpret_cast<const float4*>(p);
                    nib = (!(q.x <= 0.5f) ? 1u : 0u) | (!(q.y <= 0.5f) ? 2u : 0u) | (!(q.z <= 0.5f) ? 4u : 0u) |
                          (!(q.w <= 0.5f) ? 8u : 0u);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (col + j >= 0 && col + j < W) nib |= !(p[j] <= 0.5f) ? (1u << j) : 0u;
            }
        }
        nib <<= (lane & 7) * 4;
        nib |= __shfl_xor(nib, 1);
        nib |= __shfl_xor(nib, 2);
        nib |= __shfl_xor(nib, 4);
        if ((lane & 7) == 0) bits[r][lane >> 3] = nib;
    }
}

// The tile's drop bits: drop[ty][w] bit i <-> pixel (y0 + ty, x0 + 64 w + i) has a mask element that is not <= 0.5 within
// `margin` rows and columns.  Separable: rows widened along x by OR-ing the 2 margin + 1 shifts of a row, then along y by
// OR-ing 2 margin + 1 rows.
__device__ __forceinline__ void widen_mask_bits(int margin, const uint64_t (*bits)[4], uint64_t (*wide)[2], uint64_t (*drop)[2]) {
    const int tid = threadIdx.x, rows = kTH + 2 * margin;
    if (tid < 2 * rows) {
        const int r = tid >> 1, w = 1 + (tid & 1);
        const uint64_t lo = bits[r][w - 1], mid = bits[r][w], hi = bits[r][w + 1];
        uint64_t acc = mid;
        for (int s = 1; s <= margin; ++s)                          // column c + s, column c - s;  1 <= s < 64
            acc |= (mid >> s) | (hi << (64 - s)) | (mid << s) | (lo >> (64 - s));
        wide[r][w - 1] = acc;
    }
    __syncthreads();
    if (tid < 2 * kTH) {
        const int ty = tid >> 1, w = tid & 1;
        uint64_t acc = 0;
        for (int r = ty; r <= ty + 2 * margin; ++r) acc |= wide[r][w];
        drop[ty][w] = acc;
    }
    __syncthreads();
}

// One block: tile (blockIdx.x, blockIdx.y) of image b, channels c0 .. c0 + CG - 1 (those below C), z = b * groups + group.
// VEC: C == CG, W % 4 == 0 and both images start on 16 bytes, so a lane's 4 pixels are CG float4 loads.  The partial row of
// the tile: ws[tile][0] = n (written by group 0), ws[tile][1 + 4 c ..] = the four sums of channel c.
template <int CG, bool VEC>
__global__ __launch_bounds__(256) void lp_color_stats_kernel(const lp_color_stats_desc d, const int groups, const bool mvec) {
    __shared__ __attribute__((aligned(16))) uint64_t bits[kHaloRows][4];
    __shared__ uint64_t wide[kHaloRows][2];
    __shared__ uint64_t drop[kTH][2];
    __shared__ double part[4][4 * CG + 1];
    const int tid = threadIdx.x, H = d.height, W = d.width, C = d.channels;
    const int b = blockIdx.z / groups, c0 = (blockIdx.z - b * groups) * CG;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    if (d.mask) {                                                  // block-uniform
        const float* plane = d.mask + static_cast<int64_t>(d.mask_batch == 1 ? 0 : b) * H * W;
        load_mask_bits(plane, H, W, y0, x0, d.margin, mvec, reinterpret_cast<uint32_t(*)[8]>(bits));
        __syncthreads();
        widen_mask_bits(d.margin, bits, wide, drop);
    }
    const int px = (tid & (kTW / 4 - 1)) * 4, ry = tid / (kTW / 4);
    const int x = x0 + px;
    double acc[4 * CG + 1];                                        // [4 j + {0, 1, 2, 3}] = sum d, r, d^2, r^2 of channel c0 + j; last: n
#pragma unroll
    for (int k = 0; k < 4 * CG + 1; ++k) acc[k] = 0.0;
    int n = 0;
    if (x < W) {
#pragma unroll
        for (int pass = 0; pass < kTH / kRowsPerPass; ++pass) {
            const int ty = ry + pass * kRowsPerPass, y = y0 + ty;
            if (y >= H) break;
            const uint32_t dropped = d.mask ? static_cast<uint32_t>(drop[ty][px >> 6] >> (px & 63)) & 15u : 0u;
            const int64_t at = ((static_cast<int64_t>(b) * H + y) * W + x) * C + c0;
            float dv[4][CG], rv[4][CG];
            bool keep[4];
            if constexpr (VEC) {                                   // 4 pixels x CG channels = CG float4, all four pixels inside
                float df[4 * CG], rf[4 * CG];
#pragma unroll
                for (int q = 0; q < CG; ++q) {
                    const float4 a = reinterpret_cast<const float4*>(d.detail + at)[q];
                    const float4 r = reinterpret_cast<const float4*>(d.reference + at)[q];
                    df[4 * q] = a.x; df[4 * q + 1] = a.y; df[4 * q + 2] = a.z; df[4 * q + 3] = a.w;
                    rf[4 * q] = r.x; rf[4 * q + 1] = r.y; rf[4 * q + 2] = r.z; rf[4 * q + 3] = r.w;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    keep[i] = !((dropped >> i) & 1u);
#pragma unroll
                    for (int j = 0; j < CG; ++j) { dv[i][j] = df[i * CG + j]; rv[i][j] = rf[i * CG + j]; }
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    keep[i] = x + i < W && !((dropped >> i) & 1u);
#pragma unroll
                    for (int j = 0; j < CG; ++j) {
                        const bool in = x + i < W && c0 + j < C;
                        dv[i][j] = in ? d.detail[at + static_cast<int64_t>(i) * C + j] : 0.0f;
                        rv[i][j] = in ? d.reference[at + static_cast<int64_t>(i) * C + j] : 0.0f;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!keep[i]) continue;
                ++n;
#pragma unroll
                for (int j = 0; j < CG; ++j) {
                    const double dd = static_cast<double>(dv[i][j]), rr = static_cast<double>(rv[i][j]);
                    acc[4 * j + 0] = __dadd_rn(acc[4 * j + 0], dd);
                    acc[4 * j + 1] = __dadd_rn(acc[4 * j + 1], rr);
                    acc[4 * j + 2] = __dadd_rn(acc[4 * j + 2], __dmul_rn(dd, dd));
                    acc[4 * j + 3] = __dadd_rn(acc[4 * j + 3], __dmul_rn(rr, rr));
                }
            }
        }
    }
    acc[4 * CG] = static_cast<double>(n);
    wave_sum_dpp(acc);                                             // fixed order; the wave's sums in its last lane
    const int lane = tid & (kWave - 1), wave = tid >> 6;
    if (lane == kWave - 1) {
#pragma unroll
        for (int k = 0; k < 4 * CG + 1; ++k) part[wave][k] = acc[k];
    }
    __syncthreads();
    if (tid < 4 * CG + 1) {
        const double s = __dadd_rn(__dadd_rn(part[0][tid], part[1][tid]), __dadd_rn(part[2][tid], part[3][tid]));
        const int64_t tile = (static_cast<int64_t>(b) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        double* row = static_cast<double*>(d.workspace) + tile * (1 + 4 * C);
        if (tid == 4 * CG) {
            if (c0 == 0) row[0] = s;
        } else if (c0 + (tid >> 2) < C) {
            row[1 + 4 * c0 + tid] = s;
        }
    }
}

// stats[b][k] = the sum of image b's partial rows: one block per image, a wave per entry k, lane l adds tiles l, l + 64, ... in
// order, then the wave's fixed tree.
__global__ __launch_bounds__(256) void lp_color_fold_kernel(const double* __restrict__ ws, double* __restrict__ stats, int tiles,
                                                            int row) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6, b = blockIdx.x;
    const double* base = ws + static_cast<int64_t>(b) * tiles * row;
    for (int k = wave; k < row; k += 4) {
        double s[1] = {0.0};
        for (int t = lane; t < tiles; t += kWave) s[0] = __dadd_rn(s[0], base[static_cast<int64_t>(t) * row + k]);
        wave_sum_dpp(s);
        if (lane == kWave - 1) stats[static_cast<int64_t>(b) * row + k] = s[0];
    }
}

// ---- fit ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lp_color_fit_kernel(const lp_color_fit_desc d) {
    const int t = blockIdx.x * 256 + threadIdx.x, C = d.channels;
    if (t >= d.batch * C) return;
    const int i = t / C, c = t - i * C, row = 1 + 4 * C;
    const int L = d.clip_frames ? d.clip_frames : d.batch, q = i / L, f = i - q * L;
    const int r = d.smooth / 2;
    const int f0 = d.smooth ? max(0, f - r) : 0, f1 = d.smooth ? min(L - 1, f + r) : L - 1;
    double N = 0.0, sd = 0.0, sr = 0.0, sdd = 0.0, srr = 0.0;
    for (int g = f0; g <= f1; ++g) {
        const double* s = d.stats + static_cast<int64_t>(q * L + g) * row;
        N = __dadd_rn(N, s[0]);
        sd = __dadd_rn(sd, s[1 + 4 * c]);
        sr = __dadd_rn(sr, s[2 + 4 * c]);
        sdd = __dadd_rn(sdd, s[3 + 4 * c]);
        srr = __dadd_rn(srr, s[4 + 4 * c]);
    }
    double gain = 1.0, bias = 0.0;
    if (N >= static_cast<double>(LP_COLOR_MIN_COUNT)) {
        const double md = __ddiv_rn(sd, N), mr = __ddiv_rn(sr, N);
        const double vd = __dsub_rn(__ddiv_rn(sdd, N), __dmul_rn(md, md));
        const double vr = __dsub_rn(__ddiv_rn(srr, N), __dmul_rn(mr, mr));
        double g = 1.0;
        if (d.method == LP_COLOR_METHOD_MEAN_STD && !(vd <= 1e-8) && vr >= 0.0) {
            g = __dsqrt_rn(__ddiv_rn(vr, vd));
            g = g < 0.25 ? 0.25 : g > 4.0 ? 4.0 : g;
        }
        const double bb = __dsub_rn(mr, __dmul_rn(g, md));
        gain = __dadd_rn(1.0, __dmul_rn(d.strength, __dsub_rn(g, 1.0)));
        bias = __dmul_rn(d.strength, bb);
    }
    d.coef[2 * t] = static_cast<float>(gain);
    d.coef[2 * t + 1] = static_cast<float>(bias);
}

// ---- apply ----------------------------------------------------------------------------------------------------------------
// blockIdx.y = image; its H * W * C elements as a flat stream, the channel of element e is e % C.  The image's 2 C coefficients
// sit in LDS.
template <bool VEC>
__global__ __launch_bounds__(256) void lp_color_apply_kernel(const lp_color_apply_desc d, const int64_t n_img) {
    __shared__ float gb[2 * LP_DETAIL_MAX_CHANNELS];
    const int C = d.channels, b = blockIdx.y;
    if (threadIdx.x < 2 * C) gb[threadIdx.x] = d.coef[static_cast<int64_t>(b) * 2 * C + threadIdx.x];
    __syncthreads();
    const float* src = d.detail + b * n_img;
    float* dst = d.out + b * n_img;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    constexpr int V = VEC ? 4 : 1;                                 // VEC: n_img % 4 == 0
    int c = static_cast<int>((i * V) % C);                         // the channel of this lane's first element, kept by steps
    const int cstep = static_cast<int>((stride * V) % C);
    for (; i < n_img / V; i += stride) {
        if constexpr (VEC) {
            const float4 v = reinterpret_cast<const float4*>(src)[i];
            float o[4] = {v.x, v.y, v.z, v.w};
            int cj = c;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = __fadd_rn(__fmul_rn(o[j], gb[2 * cj]), gb[2 * cj + 1]);
                cj = cj + 1 == C ? 0 : cj + 1;
            }
            reinterpret_cast<float4*>(dst)[i] = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            dst[i] = __fadd_rn(__fmul_rn(src[i], gb[2 * c]), gb[2 * c + 1]);
        }
        c += cstep;
        c = c >= C ? c - C : c;
    }
}

bool side_ok(int s) { return s > 0 && s <= LP_DETAIL_MAX_SIDE; }
bool chan_ok(int c) { return c > 0 && c <= LP_DETAIL_MAX_CHANNELS; }

template <int CG>
void launch_stats(const lp_color_stats_desc& d, bool vec, bool mvec, hipStream_t stream) {
    const int groups = (d.channels + CG - 1) / CG;
    const dim3 grid((d.width + kTW - 1) / kTW, (d.height + kTH - 1) / kTH, d.batch * groups);
    if (vec)
        hipLaunchKernelGGL((lp_color_stats_kernel<CG, true>), grid, dim3(256), 0, stream, d, groups, mvec);
    else
        hipLaunchKernelGGL((lp_color_stats_kernel<CG, false>), grid, dim3(256), 0, stream, d, groups, mvec);
}

}  // namespace

extern "C" int lp_color_stats(const lp_color_stats_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_color_stats_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.height) || !side_ok(d.width) || !chan_ok(d.channels)) return LP_E_INVALID;
    if (d.margin < 0 || d.margin > LP_COLOR_MAX_MARGIN) return LP_E_INVALID;
    if (!d.detail || !d.reference || !d.stats || !d.workspace) return LP_E_INVALID;
    if (d.mask && d.mask_batch != 1 && d.mask_batch != d.batch) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    if (!aligned16(d.workspace)) return LP_E_ALIGN;
    if (d.workspace_bytes < LP_COLOR_WS_BYTES(d.batch, d.height, d.width, d.channels)) return LP_E_INVALID;
    const int C = d.channels;
    if (static_cast<int64_t>(d.batch) * ((C + 3) / 4) > 65535) return LP_E_UNSUPPORTED;   // a grid axis (C > 4 only)
    const bool rows16 = (d.width & 3) == 0;                       // then every row of every plane starts on 16 bytes
    const bool vec = C <= 4 && rows16 && aligned16(d.detail) && aligned16(d.reference);
    const bool mvec = rows16 && aligned16(d.mask);
    switch (C) {
        case 1: launch_stats<1>(d, vec, mvec, stream); break;
        case 2: launch_stats<2>(d, vec, mvec, stream); break;
        case 3: launch_stats<3>(d, vec, mvec, stream); break;
        default: launch_stats<4>(d, vec, mvec, stream); break;
    }
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    const int tiles = ((d.width + kTW - 1) / kTW) * ((d.height + kTH - 1) / kTH);
    hipLaunchKernelGGL(lp_color_fold_kernel, dim3(d.batch), dim3(256), 0, stream, static_cast<const double*>(d.workspace),
                       d.stats, tiles, 1 + 4 * C);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

extern "C" int lp_color_fit(const lp_color_fit_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_color_fit_desc& d = *dp;
    if (d.batch <= 0 || !chan_ok(d.channels) || !d.stats || !d.coef) return LP_E_INVALID;
    if (d.clip_frames < 0 || (d.clip_frames > 0 && d.batch % d.clip_frames != 0)) return LP_E_INVALID;
    if (d.smooth < 0 || d.smooth > 129 || (d.smooth > 0 && d.smooth % 2 == 0)) return LP_E_INVALID;
    if (d.method != LP_COLOR_METHOD_MEAN && d.method != LP_COLOR_METHOD_MEAN_STD) return LP_E_INVALID;
    if (!(d.strength >= 0.0 && d.strength <= 1.0)) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    hipLaunchKernelGGL(lp_color_fit_kernel, dim3((d.batch * d.channels + 255) / 256), dim3(256), 0, stream, d);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

extern "C" int lp_color_apply(const lp_color_apply_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_color_apply_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.height) || !side_ok(d.width) || !chan_ok(d.channels)) return LP_E_INVALID;
    if (!d.detail || !d.coef || !d.out) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    const int64_t n_img = static_cast<int64_t>(d.height) * d.width * d.channels;
    const bool vec = (n_img & 3) == 0 && aligned16(d.detail) && aligned16(d.out);
    const int64_t per_block = vec ? 4096 : 1024;                  // four loop trips per lane
    const uint32_t gx = static_cast<uint32_t>(min(static_cast<int64_t>(kApplyBlocks), (n_img + per_block - 1) / per_block));
    if (vec)
        hipLaunchKernelGGL(lp_color_apply_kernel<true>, dim3(gx, d.batch), dim3(256), 0, stream, d, n_img);
    else
        hipLaunchKernelGGL(lp_color_apply_kernel<false>, dim3(gx, d.batch), dim3(256), 0, stream, d, n_img);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

}  // namespace lp
