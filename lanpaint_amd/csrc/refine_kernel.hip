// refine_kernel.hip -- mask refine for gfx950 (lanpaint_amd/refine.py): the colour guided filter (He et al.) that pulls a rough
// mask's edge onto the nearest edge of the image underneath it.  include/lanpaint_hip.h (lp_mask_refine) states the rule: 8-bit
// codes, exact integer box sums, a 3 x 3 solve per pixel in fp64, and fp64 box sums of the coefficients in a fixed order.
//
//   coeff     stages 1 and 2.  A block owns a 32 x 32 tile of pixels and stages the four code planes of its (32 + 2r)-square
//             region as one uchar4 per pixel in LDS (zero outside the image).  Then, 16 region rows at a time: the thirteen
//             horizontal window sums of every (row, tile column) -- a thread forms the window of one column and slides it to
//             the next, integer sums being free in their order -- go to LDS as four uint4 per entry, and every thread adds the
//             rows that lie in the windows of its four pixels (one column, four consecutive rows: the rows all four windows
//             share are added once).  The solve follows in registers; (a_0, a_1, a_2, b) goes to the workspace as one float4.
//   apply     stage 3.  A block owns a 32 x 64 tile and walks the (64 + 2r) rows of its region 16 at a time: the float4s of the
//             rows are staged in LDS (+0.0 outside the image), the row sums over ascending x are formed in fp64 for every (row,
//             tile column), and every thread adds them in ascending y to the sums of the pixels whose window holds the row
//             (one column, eight consecutive rows).  The codes of the pixel's own guide are formed again at the end.
//
// Two launches on the caller's stream.  The sums of stage 3 cost O(r) additions per pixel: the rule fixes their order, which
// keeps exact zeros away from the mask and makes the result the same bits whatever the tiling.  Every fp64 step goes through
// __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn (the library is built with -ffp-contract=on).  No floating-point atomics.
// Entry points defined here: lp_mask_refine, lp_refine_ws_bytes.
#include "lp_common.h"

namespace lp {
namespace {

constexpr int kTW = 32;                  // tile width of both kernels
constexpr int kCoeffTH = 32;             // coeff: tile height, 4 pixels per thread
constexpr int kApplyTH = 64;             // apply: tile height, 8 pixels per thread
constexpr int kChunk = 16;               // region rows per pass
constexpr int kCoeffPix = kCoeffTH / 8, kApplyPix = kApplyTH / 8;

// (G_0, G_1, G_2, P) of pixel (y, x) of image `img` as one dword, G_0 in bits 0..7; a grey guide leaves G_1 = G_2 = 0
__device__ __forceinline__ uint32_t codes_at(const lp_refine_desc& d, int img, int y, int x) {
    const int64_t pix = static_cast<int64_t>(y) * d.width + x, plane = static_cast<int64_t>(d.height) * d.width;
    const float* g = d.guide + (static_cast<int64_t>(img) * plane + pix) * d.channels;
    uint32_t w = static_cast<uint32_t>(code_of(g[0]));
    if (d.channels >= 3) w |= (static_cast<uint32_t>(code_of(g[1])) << 8) | (static_cast<uint32_t>(code_of(g[2])) << 16);
    return w | (static_cast<uint32_t>(code_of(d.mask[(d.mask_batch == 1 ? 0 : static_cast<int64_t>(img) * plane) + pix])) << 24);
}

// the pixel count of the (2r + 1) window around index i, cut at [0, n)
__device__ __forceinline__ int window_len(int i, int r, int n) { return min(i + r, n - 1) - max(i - r, 0) + 1; }

// The thirteen sums, in the order they are kept: S_0 S_1 S_2 S_p | S_0p S_1p S_2p S_00 | S_01 S_02 S_11 S_12 | S_22
template <bool ADD>
__device__ __forceinline__ void sums13(uint32_t (&s)[13], uint32_t w) {
    const uint32_t g0 = w & 255u, g1 = (w >> 8) & 255u, g2 = (w >> 16) & 255u, p = w >> 24;
    const uint32_t t[13] = {g0, g1, g2, p, g0 * p, g1 * p, g2 * p, g0 * g0, g0 * g1, g0 * g2, g1 * g1, g1 * g2, g2 * g2};
#pragma unroll
    for (int k = 0; k < 13; ++k) s[k] = ADD ? s[k] + t[k] : s[k] - t[k];                 // (mod 2^32: a window's sum fits)
}

// Stage 2 for one pixel: the window's thirteen sums and its pixel count -> (a_0, a_1, a_2, b) rounded to fp32
__device__ __forceinline__ float4 solve(const uint32_t (&s)[13], int n_i, double eps, bool grey) {
    const double n = static_cast<double>(n_i);
    const double S0 = s[0], S1 = s[1], S2 = s[2], Sp = s[3];
    const double R = __dmul_rn(__dmul_rn(n, n), __dmul_rn(eps, 65025.0));
    const double C0 = __dsub_rn(__dmul_rn(n, static_cast<double>(s[4])), __dmul_rn(S0, Sp));
    const double m00 = __dadd_rn(__dsub_rn(__dmul_rn(n, static_cast<double>(s[7])), __dmul_rn(S0, S0)), R);
    double a0, a1 = 0.0, a2 = 0.0, dot;
    if (grey) {
        a0 = m00 > 0.0 ? __ddiv_rn(C0, m00) : 0.0;
        dot = __dmul_rn(a0, S0);
    } else {
        const double C1 = __dsub_rn(__dmul_rn(n, static_cast<double>(s[5])), __dmul_rn(S1, Sp));
        const double C2 = __dsub_rn(__dmul_rn(n, static_cast<double>(s[6])), __dmul_rn(S2, Sp));
        const double m01 = __dsub_rn(__dmul_rn(n, static_cast<double>(s[8])), __dmul_rn(S0, S1));
        const double m02 = __dsub_rn(__dmul_rn(n, static_cast<double>(s[9])), __dmul_rn(S0, S2));
        const double m11 = __dadd_rn(__dsub_rn(__dmul_rn(n, static_cast<double>(s[10])), __dmul_rn(S1, S1)), R);
        const double m12 = __dsub_rn(__dmul_rn(n, static_cast<double>(s[11])), __dmul_rn(S1, S2));
        const double m22 = __dadd_rn(__dsub_rn(__dmul_rn(n, static_cast<double>(s[12])), __dmul_rn(S2, S2)), R);
        const double c00 = __dsub_rn(__dmul_rn(m11, m22), __dmul_rn(m12, m12));
        const double c01 = __dsub_rn(__dmul_rn(m02, m12), __dmul_rn(m01, m22));
        const double c02 = __dsub_rn(__dmul_rn(m01, m12), __dmul_rn(m02, m11));
        const double c11 = __dsub_rn(__dmul_rn(m00, m22), __dmul_rn(m02, m02));
        const double c12 = __dsub_rn(__dmul_rn(m01, m02), __dmul_rn(m00, m12));
        const double c22 = __dsub_rn(__dmul_rn(m00, m11), __dmul_rn(m01, m01));
        const double det = __dadd_rn(__dadd_rn(__dmul_rn(m00, c00), __dmul_rn(m01, c01)), __dmul_rn(m02, c02));
        if (det > 0.0) {
            a0 = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(c00, C0), __dmul_rn(c01, C1)), __dmul_rn(c02, C2)), det);
            a1 = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(c01, C0), __dmul_rn(c11, C1)), __dmul_rn(c12, C2)), det);
            a2 = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(c02, C0), __dmul_rn(c12, C1)), __dmul_rn(c22, C2)), det);
        } else {
            a0 = 0.0;
        }
        dot = __dadd_rn(__dadd_rn(__dmul_rn(a0, S0), __dmul_rn(a1, S1)), __dmul_rn(a2, S2));
    }
    const double b = __ddiv_rn(__dsub_rn(Sp, dot), n);
    return make_float4(static_cast<float>(a0), static_cast<float>(a1), static_cast<float>(a2), static_cast<float>(b));
}

// ---- coeff: stages 1 and 2 --------------------------------------------------------------------------------------------------
// LDS: the region's codes [32 + 2r][32 + 2r + 1] dwords (the odd row stride keeps the two rows a half-wave reads, each at a
// stride of two dwords, on banks of different parity), then the chunk's row sums [16][4][32] uint4.
__global__ __launch_bounds__(256) void lp_refine_coeff_kernel(const lp_refine_desc d) {
    extern __shared__ __attribute__((aligned(16))) uint32_t refine_lds[];
    const int tid = threadIdx.x, r = d.radius, img = blockIdx.z;
    const int y0 = blockIdx.y * kCoeffTH, x0 = blockIdx.x * kTW;
    const int RW = kTW + 2 * r, RH = kCoeffTH + 2 * r, RS = RW + 1;
    uint32_t* cd = refine_lds;
    uint4* rs = reinterpret_cast<uint4*>(refine_lds + ((RH * RS + 3) & ~3));
    const int nr = min(kCoeffTH, d.height - y0);                     // tile rows inside the image
    const int rows = nr + 2 * r;                                     // region rows any of them reads
    for (int it = tid; it < rows * RW; it += 256) {
        const int ry = it / RW, rx = it - ry * RW, gy = y0 - r + ry, gx = x0 - r + rx;
        cd[ry * RS + rx] = (gy >= 0 && gy < d.height && gx >= 0 && gx < d.width) ? codes_at(d, img, gy, gx) : 0u;
    }
    __syncthreads();
    const int j = tid & 31, i0 = (tid >> 5) * kCoeffPix;              // this thread's pixels: column j, rows i0 .. i0 + 3
    uint32_t core[13] = {}, edge[kCoeffPix][13] = {};
    const int core_lo = i0 + kCoeffPix - 1, core_hi = i0 + 2 * r;     // region rows in all four windows (empty when r < 2)
    const int hr = tid >> 4, hj = (tid & 15) * 2;                     // row sums: row hr of the chunk, columns hj and hj + 1
    for (int c0 = 0; c0 < rows; c0 += kChunk) {
        if (c0) __syncthreads();                                     // the previous chunk's sums are read
        if (c0 + hr < rows) {
            const uint32_t* q = cd + (c0 + hr) * RS + hj;
            uint32_t s[13] = {};
            for (int k = 0; k <= 2 * r; ++k) sums13<true>(s, q[k]);
            uint4* o = rs + (hr * 4) * kTW + hj;
            o[0] = make_uint4(s[0], s[1], s[2], s[3]);
            o[kTW] = make_uint4(s[4], s[5], s[6], s[7]);
            o[2 * kTW] = make_uint4(s[8], s[9], s[10], s[11]);
            o[3 * kTW] = make_uint4(s[12], 0u, 0u, 0u);
            sums13<true>(s, q[2 * r + 1]);
            sums13<false>(s, q[0]);
            o[1] = make_uint4(s[0], s[1], s[2], s[3]);
            o[kTW + 1] = make_uint4(s[4], s[5], s[6], s[7]);
            o[2 * kTW + 1] = make_uint4(s[8], s[9], s[10], s[11]);
            o[3 * kTW + 1] = make_uint4(s[12], 0u, 0u, 0u);
        }
        __syncthreads();
        const int lo = max(c0, i0), hi = min(min(c0 + kChunk, rows) - 1, i0 + kCoeffPix - 1 + 2 * r);
        for (int ry = lo; ry <= hi; ++ry) {
            const uint4* q = rs + ((ry - c0) * 4) * kTW + j;
            const uint4 v0 = q[0], v1 = q[kTW], v2 = q[2 * kTW], v3 = q[3 * kTW];
            const uint32_t v[13] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x};
            if (ry >= core_lo && ry <= core_hi) {
#pragma unroll
                for (int k = 0; k < 13; ++k) core[k] += v[k];
            } else {
#pragma unroll
                for (int p = 0; p < kCoeffPix; ++p)
                    if (ry >= i0 + p && ry <= i0 + p + 2 * r) {
#pragma unroll
                        for (int k = 0; k < 13; ++k) edge[p][k] += v[k];
                    }
            }
        }
    }
    const int gx = x0 + j;
    if (gx >= d.width) return;
    const int nx = window_len(gx, r, d.width);
    float4* ws = static_cast<float4*>(d.ws) + static_cast<int64_t>(img) * d.height * d.width;
#pragma unroll
    for (int p = 0; p < kCoeffPix; ++p) {
        const int gy = y0 + i0 + p;
        if (gy >= d.height) break;
        uint32_t s[13];
#pragma unroll
        for (int k = 0; k < 13; ++k) s[k] = core[k] + edge[p][k];
        ws[static_cast<int64_t>(gy) * d.width + gx] = solve(s, nx * window_len(gy, r, d.height), d.eps, d.channels < 3);
    }
}

// ---- apply: stage 3 ---------------------------------------------------------------------------------------------------------
// LDS: the chunk's float4s [16][32 + 2r], then its row sums [16][4][32] doubles.
__global__ __launch_bounds__(256) void lp_refine_apply_kernel(const lp_refine_desc d) {
    extern __shared__ __attribute__((aligned(16))) uint32_t refine_lds[];
    const int tid = threadIdx.x, r = d.radius, img = blockIdx.z;
    const int y0 = blockIdx.y * kApplyTH, x0 = blockIdx.x * kTW;
    const int RW = kTW + 2 * r;
    float4* st = reinterpret_cast<float4*>(refine_lds);
    double* hs = reinterpret_cast<double*>(st + kChunk * RW);
    const int nr = min(kApplyTH, d.height - y0), rows = nr + 2 * r;
    const int64_t plane = static_cast<int64_t>(d.height) * d.width;
    const float4* ws = static_cast<const float4*>(d.ws) + static_cast<int64_t>(img) * plane;
    const int j = tid & 31, i0 = (tid >> 5) * kApplyPix;              // this thread's pixels: column j, rows i0 .. i0 + 7
    double acc[kApplyPix][4] = {};
    for (int c0 = 0; c0 < rows; c0 += kChunk) {
        const int nc = min(kChunk, rows - c0);
        if (c0) __syncthreads();                                     // the previous chunk is read
        for (int it = tid; it < nc * RW; it += 256) {
            const int ry = it / RW, rx = it - ry * RW, gy = y0 - r + c0 + ry, gx = x0 - r + rx;
            st[it] = (gy >= 0 && gy < d.height && gx >= 0 && gx < d.width) ? ws[static_cast<int64_t>(gy) * d.width + gx]
                                                                          : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        __syncthreads();
        for (int ry = tid >> 5; ry < nc; ry += 8) {                  // the row sum over ascending x, from +0.0
            const float4* q = st + ry * RW + j;
            double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0;
            for (int k = 0; k <= 2 * r; ++k) {
                const float4 v = q[k];
                h0 = __dadd_rn(h0, static_cast<double>(v.x));
                h1 = __dadd_rn(h1, static_cast<double>(v.y));
                h2 = __dadd_rn(h2, static_cast<double>(v.z));
                h3 = __dadd_rn(h3, static_cast<double>(v.w));
            }
            double* o = hs + (ry * 4) * kTW + j;
            o[0] = h0; o[kTW] = h1; o[2 * kTW] = h2; o[3 * kTW] = h3;
        }
        __syncthreads();
        const int lo = max(c0, i0), hi = min(c0 + nc - 1, i0 + kApplyPix - 1 + 2 * r);
        for (int ry = lo; ry <= hi; ++ry) {                          // ascending y
            const double* q = hs + ((ry - c0) * 4) * kTW + j;
            const double h0 = q[0], h1 = q[kTW], h2 = q[2 * kTW], h3 = q[3 * kTW];
#pragma unroll
            for (int p = 0; p < kApplyPix; ++p)
                if (ry >= i0 + p && ry <= i0 + p + 2 * r) {
                    acc[p][0] = __dadd_rn(acc[p][0], h0);
                    acc[p][1] = __dadd_rn(acc[p][1], h1);
                    acc[p][2] = __dadd_rn(acc[p][2], h2);
                    acc[p][3] = __dadd_rn(acc[p][3], h3);
                }
        }
    }
    const int gx = x0 + j;
    if (gx >= d.width) return;
    const int nx = window_len(gx, r, d.width);
#pragma unroll
    for (int p = 0; p < kApplyPix; ++p) {
        const int gy = y0 + i0 + p;
        if (gy >= d.height) break;
        const uint32_t w = codes_at(d, img, gy, gx);
        double t = __dmul_rn(acc[p][0], static_cast<double>(w & 255u));
        if (d.channels >= 3) {
            t = __dadd_rn(t, __dmul_rn(acc[p][1], static_cast<double>((w >> 8) & 255u)));
            t = __dadd_rn(t, __dmul_rn(acc[p][2], static_cast<double>((w >> 16) & 255u)));
        }
        t = __dadd_rn(t, acc[p][3]);
        t = __ddiv_rn(t, static_cast<double>(nx * window_len(gy, r, d.height)));
        t = __ddiv_rn(t, 255.0);
        d.out[static_cast<int64_t>(img) * plane + static_cast<int64_t>(gy) * d.width + gx] =
            static_cast<float>(fmin(fmax(t, 0.0), 1.0));
    }
}

bool side_ok(int s) { return s > 0 && s <= LP_DETAIL_MAX_SIDE; }
bool chan_ok(int c) { return c == 1 || (c >= 3 && c <= LP_DETAIL_MAX_CHANNELS); }
bool radius_ok(int r) { return r >= 1 && r <= LP_REFINE_MAX_RADIUS; }

size_t coeff_lds(int r) {
    const int RW = kTW + 2 * r, RH = kCoeffTH + 2 * r;
    return (static_cast<size_t>((RH * (RW + 1) + 3) & ~3)) * 4 + static_cast<size_t>(kChunk) * 4 * kTW * sizeof(uint4);
}
size_t apply_lds(int r) { return static_cast<size_t>(kChunk) * ((kTW + 2 * r) * sizeof(float4) + 4 * kTW * sizeof(double)); }

}  // namespace

extern "C" int64_t lp_refine_ws_bytes(int32_t batch, int32_t height, int32_t width, int32_t channels, int32_t radius) {
    if (batch <= 0 || !side_ok(height) || !side_ok(width) || !chan_ok(channels) || !radius_ok(radius)) return LP_E_INVALID;
    if (batch > 65535) return LP_E_UNSUPPORTED;
    return static_cast<int64_t>(batch) * height * width * 16;
}

extern "C" int lp_mask_refine(const lp_refine_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_refine_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.height) || !side_ok(d.width) || !chan_ok(d.channels) || !radius_ok(d.radius)) return LP_E_INVALID;
    if (!(d.eps >= 1e-6 && d.eps <= 1.0)) return LP_E_INVALID;       // (a NaN fails both)
    if (!d.guide || !d.mask || !d.out || !d.ws || d.out == d.guide || d.out == d.mask) return LP_E_INVALID;
    if (d.mask_batch != 1 && d.mask_batch != d.batch) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    if (!aligned16(d.ws)) return LP_E_ALIGN;
    if (d.ws_bytes < lp_refine_ws_bytes(d.batch, d.height, d.width, d.channels, d.radius)) return LP_E_INVALID;
    const size_t lds_c = coeff_lds(d.radius), lds_a = apply_lds(d.radius);       // at r = 64: 135 808 and 57 344 bytes
    if (lds_c > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(&lp_refine_coeff_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024) != hipSuccess)
        return LP_E_LAUNCH;
    const dim3 grid_c((d.width + kTW - 1) / kTW, (d.height + kCoeffTH - 1) / kCoeffTH, d.batch);
    hipLaunchKernelGGL(lp_refine_coeff_kernel, grid_c, dim3(256), lds_c, stream, d);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    const dim3 grid_a((d.width + kTW - 1) / kTW, (d.height + kApplyTH - 1) / kApplyTH, d.batch);
    hipLaunchKernelGGL(lp_refine_apply_kernel, grid_a, dim3(256), lds_a, stream, d);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

}  // namespace lp
