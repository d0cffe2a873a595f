// multiband_kernel.hip -- Laplacian-pyramid (Burt-Adelson) seam blend for gfx950 (lanpaint_amd/multiband.py).  A single-width
// feather squeezes whatever low-frequency difference is left between a generated image and the original into one band; here
// every frequency band is blended over a width in proportion to its wavelength.  include/lanpaint_hip.h (lp_multiband_blend)
// states the rule; it works on the difference image D = b - a, so one image pyramid is carried instead of two.
//
//   reduce    level l -> l + 1.  A block owns a 16 x 16 tile of level l + 1 and stages the 35 x 35 region of level l it reads
//             (2 T + 3, indices clamped) in LDS, runs the vertical 5-tap pass into a 16 x 35 strip and the horizontal pass out
//             of it.  The weight plane travels as one more channel: C + 1 channels in groups of four.  At l = 0 the block
//             forms b - a and W_0 from the inputs; level 0 is never stored.
//   collapse  level l + 1 -> l.  A block owns a 32 x 32 tile of level l and stages the 18 x 18 regions (T / 2 + 2, clamped) of
//             R_{l+1} and D_{l+1}, expands both vertically into 32 x 18 strips and horizontally out of them, forms Lap_l and
//             R_l and writes R_l; at l = 0 it reads a, b and the mask again and writes out = a + R_0.  R_n = W_n * D_n is
//             formed while the top level is staged, so it costs no launch and is never stored.
//
// n reduce launches and max(n, 1) collapse launches, all on the caller's stream.  A block recomputes the halo it needs from the
// level below or above as the previous launch left it; nothing waits inside a launch.  The rule fixes every value and the
// order of every operation, so tiling, halos and vector width cannot change a bit; every product, sum and difference below is
// one __f*_rn call (the library is built with -ffp-contract=on).
// A negative `levels` is the focus form's mode word: the entry's checks, then focus_kernel.hip's launches.
// Entry points defined here: lp_multiband_blend, lp_multiband_ws_bytes.
#include "lp_common.h"

namespace lp {
namespace {

constexpr int kCG = 4;                                   // channels held in LDS at a time
constexpr int kRT = 16, kRS = 2 * kRT + 3;               // reduce: the tile of level l + 1 and the region of level l it reads
constexpr int kCT = 32, kCS = kCT / 2 + 2;               // collapse: the tile of level l and the region of level l + 1
constexpr int kMaxLevels = 16;                           // halvings of the largest side (32768) down to 1, plus level 0

// The two levels one launch works on.  Level 0 is the images themselves; levels 1 .. n live in the workspace, per image
// `pix` pixels: D (C floats per pixel, all levels), then W (1), then R (C).
struct MbLaunch {
    int32_t hf, wf, hc, wc;     // the finer level (l) and the coarser one (l + 1)
    int64_t off_f, off_c;       // their pixel offsets inside an image's planes (off_f unused at l = 0)
    int64_t pix;
    int32_t fine0;              // the finer level is level 0
    int32_t top;                // collapse: the finer level is the top one (n = 0), there is no coarser level
    int32_t coarse_top;         // collapse: the coarser level is level n, R = W * D
};

struct MbPlanes {
    float* D;
    float* W;
    float* R;
};

__device__ __forceinline__ MbPlanes planes(const lp_multiband_desc& d, const MbLaunch& g, int img) {
    float* base = static_cast<float*>(d.ws) + static_cast<int64_t>(img) * g.pix * (2 * d.channels + 1);
    return {base, base + g.pix * d.channels, base + g.pix * (d.channels + 1)};
}

__device__ __forceinline__ float weight0(float m) { return m > 0.0f ? (m < 1.0f ? m : 1.0f) : 0.0f; }      // a NaN gives 0

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// ---- reduce -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tap5(float a, float b, float c, float e, float f) {
    float s = __fmul_rn(0.0625f, a);
    s = __fadd_rn(s, __fmul_rn(0.25f, b));
    s = __fadd_rn(s, __fmul_rn(0.375f, c));
    s = __fadd_rn(s, __fmul_rn(0.25f, e));
    return __fadd_rn(s, __fmul_rn(0.0625f, f));
}

// One group of CG channels of the C + 1 (channel C is the weight).  s: [kRS * kRS][CG], t: [kRT * kRS][CG].
template <int CG>
__device__ __forceinline__ void reduce_group(const lp_multiband_desc& d, const MbLaunch& g, const MbPlanes& ws, int img, int c0,
                                             float* s, float* t) {
    const int tid = threadIdx.x, C = d.channels;
    const int y0 = blockIdx.y * kRT, x0 = blockIdx.x * kRT;
    const int64_t img0 = static_cast<int64_t>(img) * g.hf * g.wf, m0 = static_cast<int64_t>(d.mask_batch == 1 ? 0 : img) * g.hf * g.wf;
    for (int it = tid; it < kRS * kRS * CG; it += 256) {
        const int p = it / CG, c = it - p * CG, r = p / kRS, x = p - r * kRS, ch = c0 + c;
        const int64_t at = static_cast<int64_t>(clampi(2 * y0 - 2 + r, g.hf - 1)) * g.wf + clampi(2 * x0 - 2 + x, g.wf - 1);
        float v;
        if (g.fine0) {
            if (ch < C)
                v = __fsub_rn(d.image2[(img0 + at) * C + ch], d.image1[(img0 + at) * C + ch]);
            else
                v = weight0(d.mask[m0 + at]);
        } else {
            v = ch < C ? ws.D[(g.off_f + at) * C + ch] : ws.W[g.off_f + at];
        }
        s[it] = v;
    }
    __syncthreads();
    for (int it = tid; it < kRT * kRS * CG; it += 256) {             // rows first, over the full width of the region
        const int p = it / CG, c = it - p * CG, i = p / kRS, x = p - i * kRS;
        const float* q = s + (2 * i * kRS + x) * CG + c;
        t[it] = tap5(q[0], q[kRS * CG], q[2 * kRS * CG], q[3 * kRS * CG], q[4 * kRS * CG]);
    }
    __syncthreads();
    for (int it = tid; it < kRT * kRT * CG; it += 256) {
        const int p = it / CG, c = it - p * CG, i = p / kRT, j = p - i * kRT, ch = c0 + c;
        const int gy = y0 + i, gx = x0 + j;
        if (gy >= g.hc || gx >= g.wc) continue;
        const float* q = t + (i * kRS + 2 * j) * CG + c;
        const float v = tap5(q[0], q[CG], q[2 * CG], q[3 * CG], q[4 * CG]);
        const int64_t at = g.off_c + static_cast<int64_t>(gy) * g.wc + gx;
        if (ch < C)
            ws.D[at * C + ch] = v;
        else
            ws.W[at] = v;
    }
}

__global__ __launch_bounds__(256) void lp_multiband_reduce_kernel(const lp_multiband_desc d, const MbLaunch g) {
    __shared__ float s[kRS * kRS * kCG];
    __shared__ float t[kRT * kRS * kCG];
    const int img = blockIdx.z, CT = d.channels + 1;
    const MbPlanes ws = planes(d, g, img);
    for (int c0 = 0; c0 < CT; c0 += kCG) {
        if (c0) __syncthreads();                                     // the previous group's reads of t are done
        switch (min(kCG, CT - c0)) {                                 // block-uniform
            case 4: reduce_group<4>(d, g, ws, img, c0, s, t); break;
            case 3: reduce_group<3>(d, g, ws, img, c0, s, t); break;
            case 2: reduce_group<2>(d, g, ws, img, c0, s, t); break;
            default: reduce_group<1>(d, g, ws, img, c0, s, t); break;
        }
    }
}

// ---- collapse ---------------------------------------------------------------------------------------------------------------
// One axis of EXPAND at fine index i (its parity is `odd`): q points at c[p - 1], already clamped, the next taps `step` apart.
__device__ __forceinline__ float expand_tap(const float* q, int step, bool odd) {
    if (odd) return __fadd_rn(__fmul_rn(0.5f, q[step]), __fmul_rn(0.5f, q[2 * step]));
    float e = __fmul_rn(0.125f, q[0]);
    e = __fadd_rn(e, __fmul_rn(0.75f, q[step]));
    return __fadd_rn(e, __fmul_rn(0.125f, q[2 * step]));
}

// R_l (or out at l = 0) of one element: dl = D_l, wl = W_l, (ed, er) = EXPAND(D_{l+1}), EXPAND(R_{l+1}) there
__device__ __forceinline__ float collapse_value(bool top, float dl, float wl, float ed, float er) {
    if (top) return __fmul_rn(wl, dl);
    return __fadd_rn(er, __fmul_rn(wl, __fsub_rn(dl, ed)));
}

// One group of CG channels.  s: [2][kCS * kCS][CG] (R then D of the coarser level), t: [2][kCT * kCS][CG].
// VEC: level 0, CG == C, rows of a multiple of 4 floats, image1, image2 and out 16-byte aligned: a tile row is whole float4s.
template <int CG, bool VEC>
__device__ __forceinline__ void collapse_group(const lp_multiband_desc& d, const MbLaunch& g, const MbPlanes& ws, int img, int c0,
                                               float* s, float* t) {
    const int tid = threadIdx.x, C = d.channels;
    const int y0 = blockIdx.y * kCT, x0 = blockIdx.x * kCT;
    const int nr = min(kCT, g.hf - y0), nc = min(kCT, g.wf - x0);
    constexpr int kS = kCS * kCS * CG, kTt = kCT * kCS * CG;
    if (!g.top) {
        for (int it = tid; it < kS; it += 256) {
            const int p = it / CG, c = it - p * CG, r = p / kCS, x = p - r * kCS;
            const int64_t at = g.off_c + static_cast<int64_t>(clampi(y0 / 2 - 1 + r, g.hc - 1)) * g.wc + clampi(x0 / 2 - 1 + x, g.wc - 1);
            const float dv = ws.D[at * C + c0 + c];
            s[it] = g.coarse_top ? __fmul_rn(ws.W[at], dv) : ws.R[at * C + c0 + c];
            s[kS + it] = dv;
        }
        __syncthreads();
        for (int it = tid; it < kTt; it += 256) {                    // rows first: [kCT][kCS]
            const int p = it / CG, c = it - p * CG, i = p / kCS, x = p - i * kCS;
            const float* q = s + ((i >> 1) * kCS + x) * CG + c;      // the tile starts at an even row: i's parity is the row's
            t[it] = expand_tap(q, kCS * CG, i & 1);
            t[kTt + it] = expand_tap(q + kS, kCS * CG, i & 1);
        }
        __syncthreads();
    }
    const int64_t img0 = static_cast<int64_t>(img) * g.hf * g.wf, m0 = static_cast<int64_t>(d.mask_batch == 1 ? 0 : img) * g.hf * g.wf;
    if constexpr (VEC) {                                             // fine0, CG == C
        constexpr int per_row = kCT * CG / 4;
        for (int it = tid; it < kCT * per_row; it += 256) {
            const int i = it / per_row, e = 4 * (it - i * per_row);
            if (i >= nr || e >= nc * CG) continue;
            const int64_t row = img0 + static_cast<int64_t>(y0 + i) * g.wf + x0;
            const float4 a4 = *reinterpret_cast<const float4*>(d.image1 + row * CG + e);
            const float4 b4 = *reinterpret_cast<const float4*>(d.image2 + row * CG + e);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = (e + k) / CG, c = e + k - x * CG;
                const float wl = weight0(d.mask[m0 + static_cast<int64_t>(y0 + i) * g.wf + x0 + x]);
                float ed = 0.0f, er = 0.0f;
                if (!g.top) {
                    const float* q = t + (i * kCS + (x >> 1)) * CG + c;
                    er = expand_tap(q, CG, x & 1);
                    ed = expand_tap(q + kTt, CG, x & 1);
                }
                o[k] = __fadd_rn(a[k], collapse_value(g.top, __fsub_rn(b[k], a[k]), wl, ed, er));
            }
            *reinterpret_cast<float4*>(d.out + row * CG + e) = make_float4(o[0], o[1], o[2], o[3]);
        }
    } else {
        for (int it = tid; it < kCT * kCT * CG; it += 256) {
            const int p = it / CG, c = it - p * CG, i = p / kCT, x = p - i * kCT, ch = c0 + c;
            if (i >= nr || x >= nc) continue;
            const int64_t pix = static_cast<int64_t>(y0 + i) * g.wf + x0 + x;
            float ed = 0.0f, er = 0.0f;
            if (!g.top) {
                const float* q = t + (i * kCS + (x >> 1)) * CG + c;
                er = expand_tap(q, CG, x & 1);
                ed = expand_tap(q + kTt, CG, x & 1);
            }
            if (g.fine0) {
                const float a = d.image1[(img0 + pix) * C + ch], b = d.image2[(img0 + pix) * C + ch];
                d.out[(img0 + pix) * C + ch] = __fadd_rn(a, collapse_value(g.top, __fsub_rn(b, a), weight0(d.mask[m0 + pix]), ed, er));
            } else {
                const int64_t at = g.off_f + pix;
                ws.R[at * C + ch] = collapse_value(false, ws.D[at * C + ch], ws.W[at], ed, er);
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void lp_multiband_collapse_kernel(const lp_multiband_desc d, const MbLaunch g) {
    __shared__ float s[2 * kCS * kCS * kCG];
    __shared__ float t[2 * kCT * kCS * kCG];
    const int img = blockIdx.z, C = d.channels;
    const MbPlanes ws = planes(d, g, img);
    for (int c0 = 0; c0 < C; c0 += kCG) {
        if (c0) __syncthreads();                                     // the previous group's reads of t are done
        switch (min(kCG, C - c0)) {                                  // block-uniform; VEC: one group, C <= 4
            case 4: collapse_group<4, VEC>(d, g, ws, img, c0, s, t); break;
            case 3: collapse_group<3, VEC>(d, g, ws, img, c0, s, t); break;
            case 2: collapse_group<2, VEC>(d, g, ws, img, c0, s, t); break;
            default: collapse_group<1, VEC>(d, g, ws, img, c0, s, t); break;
        }
    }
}

bool side_ok(int s) { return s > 0 && s <= LP_DETAIL_MAX_SIDE; }
bool chan_ok(int c) { return c > 0 && c <= LP_DETAIL_MAX_CHANNELS; }

// Sides and workspace offsets of levels 0 .. n, n = min(levels, halvings down to (1, 1)); *pix = the pixels of levels 1 .. n.
int multiband_levels(int H, int W, int levels, int32_t* h, int32_t* w, int64_t* off, int64_t* pix) {
    int n = 0;
    int64_t at = 0;
    h[0] = H; w[0] = W; off[0] = 0;
    while (n < levels && (h[n] > 1 || w[n] > 1)) {
        h[n + 1] = (h[n] + 1) / 2;
        w[n + 1] = (w[n] + 1) / 2;
        off[n + 1] = at;
        at += static_cast<int64_t>(h[n + 1]) * w[n + 1];
        ++n;
    }
    *pix = at;
    return n;
}

}  // namespace

extern "C" int64_t lp_multiband_ws_bytes(int32_t batch, int32_t height, int32_t width, int32_t channels, int32_t levels) {
    if (batch <= 0 || !side_ok(height) || !side_ok(width) || !chan_ok(channels)) return LP_E_INVALID;
    if (levels < 0) {                                                // the focus form (focus_kernel.hip)
        const int st = focus_check(batch, height, width, levels);
        return st != LP_OK ? st : LP_FOCUS_WS_BYTES(batch, height, width, channels);
    }
    if (batch > 65535) return LP_E_UNSUPPORTED;
    int32_t h[kMaxLevels + 1], w[kMaxLevels + 1];
    int64_t off[kMaxLevels + 1], pix;
    multiband_levels(height, width, levels, h, w, off, &pix);
    const int64_t bytes = static_cast<int64_t>(batch) * pix * (2 * channels + 1) * 4;
    return bytes < 16 ? 16 : (bytes + 15) / 16 * 16;
}

extern "C" int lp_multiband_blend(const lp_multiband_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_multiband_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.height) || !side_ok(d.width) || !chan_ok(d.channels) || (d.levels < 0 && !focus_word_ok(d.levels)))
        return LP_E_INVALID;
    if (!d.image1 || !d.image2 || !d.mask || !d.out || !d.ws || d.out == d.image1 || d.out == d.image2) return LP_E_INVALID;
    if (d.mask_batch != 1 && d.mask_batch != d.batch) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    if (!aligned16(d.ws)) return LP_E_ALIGN;
    const int64_t need = lp_multiband_ws_bytes(d.batch, d.height, d.width, d.channels, d.levels);
    if (need < 0) return static_cast<int>(need);                     // (the focus form's pooled limit; never for levels >= 0 here)
    if (d.ws_bytes < need) return LP_E_INVALID;
    if (d.levels < 0) return focus_enqueue(d, stream);
    int32_t h[kMaxLevels + 1], w[kMaxLevels + 1];
    int64_t off[kMaxLevels + 1], pix;
    const int n = multiband_levels(d.height, d.width, d.levels, h, w, off, &pix);
    const bool vec = d.channels <= kCG && ((d.width * d.channels) & 3) == 0 && aligned16(d.image1) && aligned16(d.image2) &&
                     aligned16(d.out);
    MbLaunch g = {};
    g.pix = pix;
    for (int l = 0; l < n; ++l) {
        g.hf = h[l]; g.wf = w[l]; g.off_f = off[l];
        g.hc = h[l + 1]; g.wc = w[l + 1]; g.off_c = off[l + 1];
        g.fine0 = l == 0;
        const dim3 grid((g.wc + kRT - 1) / kRT, (g.hc + kRT - 1) / kRT, d.batch);
        hipLaunchKernelGGL(lp_multiband_reduce_kernel, grid, dim3(256), 0, stream, d, g);
        if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    }
    for (int l = n > 0 ? n - 1 : 0; l >= 0; --l) {                   // (n = 0: one launch, out = a + W_0 * (b - a))
        g.hf = h[l]; g.wf = w[l]; g.off_f = off[l];
        g.top = n == 0;
        g.hc = g.top ? 1 : h[l + 1]; g.wc = g.top ? 1 : w[l + 1]; g.off_c = g.top ? 0 : off[l + 1];
        g.fine0 = l == 0;
        g.coarse_top = l + 1 == n;
        const dim3 grid((g.wf + kCT - 1) / kCT, (g.hf + kCT - 1) / kCT, d.batch);
        if (vec && l == 0)
            hipLaunchKernelGGL(lp_multiband_collapse_kernel<true>, grid, dim3(256), 0, stream, d, g);
        else
            hipLaunchKernelGGL(lp_multiband_collapse_kernel<false>, grid, dim3(256), 0, stream, d, g);
        if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    }
    return LP_OK;
}

}  // namespace lp
