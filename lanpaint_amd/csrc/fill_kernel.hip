// fill_kernel.hip -- masked-area fill and outpaint canvas for gfx950 (lanpaint_amd/fill.py).  What lies under a mask still goes
// through the VAE encoder, whose receptive field reaches across the mask's edge; these jobs put a smooth continuation of the
// known pixels there, on the device, before the encode.
//
//   lp_mask_fill     push-pull pyramid (include/lanpaint_hip.h states the rule).  PULL: a block stages a 32 x 32 tile of level s
//                    in LDS and writes the parts of levels s + 1 .. s + 5 that the tile determines completely (16 x 16 .. 1 x 1:
//                    level l + 1 halves level l from the origin, so an aligned tile owns its ancestors); the next launch starts
//                    at s + 5.  PUSH: the same spans downwards.  A block owns a 32 x 32 tile of the span's lowest level and needs,
//                    level by level upwards, that tile's parents plus one pixel of halo: regions of 18, 12, 8, 6 and 5 pixels a
//                    side.  It recomputes that rim itself instead of waiting for its neighbours, from the span's top level as the
//                    previous launch left it.  720 x 1280 (12 levels) is three launches each way.  A push block whose tile has no
//                    masked pixel only copies; an image with no known pixel is recognised by the top level's flag, on the device.
//                    Filled values of a level go into the workspace where that level's flag is 0 -- places no block reads in the
//                    same launch -- so the next span finds its top level complete.
//                    With a mode word in reserved0 (LP_FILL_PATCH) the same launches make the pre-fill of the patch form, whose
//                    kernels are patch_fill_kernel.hip's.
//   lp_outpaint_pad  one streaming launch over the canvas: a block row per canvas row writes the image (original or 0) and the
//                    mask (max(band, incoming)).
//
// The rule fixes every value and the order of every operation, so what a launch covers cannot change a bit; every product,
// sum and quotient below is one __f*_rn call (the library is built with -ffp-contract=on).
// Entry points defined here: lp_mask_fill, lp_fill_ws_bytes, lp_outpaint_pad.
#include "lp_common.h"

namespace lp {
namespace {

constexpr int kT = LP_FILL_TILE, kSpan = LP_FILL_SPAN;
constexpr int kCG = 4;                                  // channels held in LDS at a time
constexpr int kPullPix = 1024 + 256 + 64 + 16 + 4 + 1;  // a tile and its five ancestors
constexpr int kPushPix = 324 + 144 + 64 + 36 + 25;      // the regions of the five levels above a tile
static_assert(kT == 32 && kSpan == 5, "the region sizes below are those of a 32 x 32 tile and a span of five levels");

// The levels one launch works on: [0] is the span's lowest level (`bottom`; level 0 is the image itself), [n] its top.
struct FillSpan {
    int32_t h[kSpan + 1], w[kSpan + 1];
    int64_t off[kSpan + 1];     // pixel offset of the level inside an image's part of the workspace (unused for level 0)
    int32_t n, bottom;
    int64_t pix;                // workspace pixels per image: levels 1 .. L - 1
    int64_t top_flag;           // pixel offset of level L - 1: its flag says whether the image has a known pixel; -1 when L = 1
};

__device__ __forceinline__ float* ws_values(const lp_fill_desc& d, const FillSpan& g, int img) {
    return static_cast<float*>(d.ws) + static_cast<int64_t>(img) * g.pix * d.channels;
}
__device__ __forceinline__ uint8_t* ws_flags(const lp_fill_desc& d, const FillSpan& g, int img) {
    return static_cast<uint8_t*>(d.ws) + static_cast<int64_t>(d.batch) * g.pix * d.channels * 4 + static_cast<int64_t>(img) * g.pix;
}
__device__ __forceinline__ bool known_at(const lp_fill_desc& d, const FillSpan& g, int img, const uint8_t* wk, int y, int x) {
    if (g.bottom == 0) {
        const float m = d.mask[(static_cast<int64_t>(d.mask_batch == 1 ? 0 : img) * g.h[0] + y) * g.w[0] + x];
        return !(m > 0.5f);
    }
    return wk[g.off[0] + static_cast<int64_t>(y) * g.w[0] + x] != 0;
}

// ---- pull -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pull_base(int lev) {     // where level `lev` of the block's little pyramid starts, in pixels
    return lev == 0 ? 0 : lev == 1 ? 1024 : lev == 2 ? 1280 : lev == 3 ? 1344 : lev == 4 ? 1360 : 1364;
}

// VEC: the span starts at the image, C <= 4, rows of a multiple of 4 floats from a 16-byte aligned base: a tile row is whole
// float4s in memory and in LDS.
template <bool VEC>
__global__ __launch_bounds__(256) void lp_fill_pull_kernel(const lp_fill_desc d, const FillSpan g) {
    __shared__ __attribute__((aligned(16))) float v[kPullPix * kCG];     // level lev, pixel p, channel c: [(base + p) * cg + c]
    __shared__ uint8_t k[kPullPix];
    const int tid = threadIdx.x, C = d.channels, img = blockIdx.z;
    const int h0 = g.h[0], w0 = g.w[0], y0 = blockIdx.y * kT, x0 = blockIdx.x * kT;
    const int nr = min(kT, h0 - y0), nc = min(kT, w0 - x0);
    float* wv = ws_values(d, g, img);
    uint8_t* wk = ws_flags(d, g, img);
    const float* src = g.bottom == 0 ? d.image + static_cast<int64_t>(img) * h0 * w0 * C : wv + g.off[0] * C;
    for (int p = tid; p < kT * kT; p += 256) {
        const int r = p >> 5, c = p & 31;
        k[p] = r < nr && c < nc && known_at(d, g, img, wk, y0 + r, x0 + c);
    }
    for (int c0 = 0; c0 < C; c0 += kCG) {
        const int cg = min(kCG, C - c0);
        if constexpr (VEC) {                                       // cg == C
            const int per_row = 8 * cg;
            for (int q = tid; q < kT * per_row; q += 256) {
                const int r = q / per_row, e = 4 * (q - r * per_row);
                if (r < nr && e < nc * cg)
                    *reinterpret_cast<float4*>(v + r * kT * cg + e) =
                        *reinterpret_cast<const float4*>(src + (static_cast<int64_t>(y0 + r) * w0 + x0) * C + e);
            }
        } else {
            const int per_row = kT * cg;
            for (int q = tid; q < kT * per_row; q += 256) {
                const int r = q / per_row, e = q - r * per_row, c = e / cg;
                if (r < nr && c < nc) v[r * per_row + e] = src[(static_cast<int64_t>(y0 + r) * w0 + x0 + c) * C + c0 + (e - c * cg)];
            }
        }
        __syncthreads();
#pragma unroll
        for (int lev = 1; lev <= kSpan; ++lev) {
            if (lev <= g.n) {                                      // block-uniform
                const int side = kT >> lev, sh = 5 - lev;
                const int pb = pull_base(lev - 1), cb = pull_base(lev);
                const int hl = g.h[lev], wl = g.w[lev];
                for (int it = tid; it < side * side * cg; it += 256) {
                    const int p = it / cg, c = it - p * cg, i = p >> sh, j = p & (side - 1);
                    float s = 0.0f;
                    int n = 0;
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) {               // (0,0), (0,1), (1,0), (1,1)
                        const int q = pb + (2 * i + (ch >> 1)) * (2 * side) + 2 * j + (ch & 1);
                        if (k[q]) {
                            s = __fadd_rn(s, v[q * cg + c]);
                            ++n;
                        }
                    }
                    const float val = n ? __fdiv_rn(s, static_cast<float>(n)) : 0.0f;
                    v[(cb + p) * cg + c] = val;
                    if (c == 0 && c0 == 0) k[cb + p] = n > 0;
                    const int gy = (y0 >> lev) + i, gx = (x0 >> lev) + j;
                    if (gy < hl && gx < wl) {
                        const int64_t at = g.off[lev] + static_cast<int64_t>(gy) * wl + gx;
                        wv[at * C + c0 + c] = val;
                        if (c == 0 && c0 == 0) wk[at] = n > 0;
                    }
                }
                __syncthreads();
            }
        }
    }
}

// ---- push -------------------------------------------------------------------------------------------------------------------
// The region of level `lev` of the span a block needs: reg_n(lev) pixels a side from reg_o(32 t, lev), t = the tile's index.
__device__ __forceinline__ int reg_n(int lev) { return lev == 0 ? 32 : lev == 1 ? 18 : lev == 2 ? 12 : lev == 3 ? 8 : lev == 4 ? 6 : 5; }
__device__ __forceinline__ int reg_o(int o0, int lev) { return (o0 >> lev) - (lev == 0 ? 0 : lev == 1 ? 1 : 2); }
__device__ __forceinline__ int push_base(int lev) { return lev == 1 ? 0 : lev == 2 ? 324 : lev == 3 ? 468 : lev == 4 ? 532 : 568; }

// One axis of the 2x upsample with pixel centres aligned: fine index i over a coarse axis of nc entries whose region starts at o.
__device__ __forceinline__ void up_taps(int i, int nc, int o, int& t0, int& t1, float& a0, float& a1) {
    const int i0 = ((i + 1) >> 1) - 1;                             // even: i / 2 - 1;  odd: (i - 1) / 2
    a0 = (i & 1) ? 0.75f : 0.25f;
    a1 = (i & 1) ? 0.25f : 0.75f;
    t0 = min(max(i0, 0), nc - 1) - o;
    t1 = min(max(i0 + 1, 0), nc - 1) - o;
}

// up(gy, gx), channel c: `f` is the coarser level's region in LDS, n1 pixels a side from (oy, ox), of a level hc x wc
__device__ __forceinline__ float upsample(const float* f, int cg, int c, int gy, int gx, int hc, int wc, int oy, int ox, int n1) {
    int ty0, ty1, tx0, tx1;
    float a0, a1, b0, b1;
    up_taps(gy, hc, oy, ty0, ty1, a0, a1);
    up_taps(gx, wc, ox, tx0, tx1, b0, b1);
    const float r0 = __fadd_rn(__fmul_rn(a0, f[(ty0 * n1 + tx0) * cg + c]), __fmul_rn(a1, f[(ty1 * n1 + tx0) * cg + c]));
    const float r1 = __fadd_rn(__fmul_rn(a0, f[(ty0 * n1 + tx1) * cg + c]), __fmul_rn(a1, f[(ty1 * n1 + tx1) * cg + c]));
    return __fadd_rn(__fmul_rn(b0, r0), __fmul_rn(b1, r1));
}

// VEC: as for the pull, and `out` 16-byte aligned too; only spans that end at the image take it.
template <bool VEC>
__global__ __launch_bounds__(256) void lp_fill_push_kernel(const lp_fill_desc d, const FillSpan g) {
    __shared__ float f[kPushPix * kCG];                            // level lev >= 1, region pixel p, channel c: [(base + p) * cg + c]
    __shared__ uint8_t kb[kT * kT];                                // the tile's own flags
    const int tid = threadIdx.x, C = d.channels, img = blockIdx.z;
    const int h0 = g.h[0], w0 = g.w[0], y0 = blockIdx.y * kT, x0 = blockIdx.x * kT;
    const int nr = min(kT, h0 - y0), nc = min(kT, w0 - x0);
    float* wv = ws_values(d, g, img);
    const uint8_t* wk = ws_flags(d, g, img);
    int masked = 0;
    for (int p = tid; p < kT * kT; p += 256) {
        const int r = p >> 5, c = p & 31;
        const bool in = r < nr && c < nc;
        const bool kn = in && known_at(d, g, img, wk, y0 + r, x0 + c);
        kb[p] = kn;
        masked |= in && !kn;
    }
    const bool any_masked = __syncthreads_or(masked);              // (also the barrier behind kb)
    const int64_t img0 = static_cast<int64_t>(img) * h0 * w0 * C;
    if (!any_masked || g.top_flag < 0 || wk[g.top_flag] == 0) {    // block-uniform: nothing to fill here, or nothing to fill from
        if (g.bottom != 0) return;
        const int seg = nc * C;                                    // a tile row, all channels: contiguous
        if constexpr (VEC) {
            for (int q = tid; q < kT * 8 * C; q += 256) {
                const int r = q / (8 * C), e = 4 * (q - r * 8 * C);
                const int64_t at = img0 + (static_cast<int64_t>(y0 + r) * w0 + x0) * C + e;
                if (r < nr && e < seg) *reinterpret_cast<float4*>(d.out + at) = *reinterpret_cast<const float4*>(d.image + at);
            }
        } else {
            for (int r = 0; r < nr; ++r) {
                const int64_t at = img0 + (static_cast<int64_t>(y0 + r) * w0 + x0) * C;
                for (int e = tid; e < seg; e += 256) d.out[at + e] = d.image[at + e];
            }
        }
        return;
    }
    for (int c0 = 0; c0 < C; c0 += kCG) {
        const int cg = min(kCG, C - c0);
        if (c0) __syncthreads();                                   // the previous group's reads of f are done
#pragma unroll
        for (int lev = kSpan; lev >= 1; --lev) {
            if (lev <= g.n) {                                      // block-uniform
                const int n0 = reg_n(lev), oy = reg_o(y0, lev), ox = reg_o(x0, lev), fb = push_base(lev);
                const int hl = g.h[lev], wl = g.w[lev];
                const int up = lev < kSpan ? lev + 1 : kSpan;      // (the span's top level has no coarser one and reads none)
                const int n1 = reg_n(up), oy1 = reg_o(y0, up), ox1 = reg_o(x0, up);
                for (int it = tid; it < n0 * n0 * cg; it += 256) {
                    const int p = it / cg, c = it - p * cg, ry = p / n0, rx = p - ry * n0;
                    const int gy = oy + ry, gx = ox + rx;
                    if (gy < 0 || gy >= hl || gx < 0 || gx >= wl) continue;
                    const int64_t at = g.off[lev] + static_cast<int64_t>(gy) * wl + gx;
                    float val;
                    if (lev == g.n || wk[at])                      // the span's top is complete; below it, known pixels keep v
                        val = wv[at * C + c0 + c];
                    else
                        val = upsample(f + push_base(up) * cg, cg, c, gy, gx, g.h[up], g.w[up], oy1, ox1, n1);
                    f[(fb + p) * cg + c] = val;
                }
                __syncthreads();
            }
        }
        // the tile itself, from level 1's region
        const int hc = g.h[1], wc = g.w[1], oy1 = reg_o(y0, 1), ox1 = reg_o(x0, 1);
        if constexpr (VEC) {                                       // bottom == 0, cg == C
            const int per_row = 8 * cg;
            for (int q = tid; q < kT * per_row; q += 256) {
                const int r = q / per_row, e = 4 * (q - r * per_row);
                if (r >= nr || e >= nc * cg) continue;
                const int64_t at = img0 + (static_cast<int64_t>(y0 + r) * w0 + x0) * C + e;
                const float4 in = *reinterpret_cast<const float4*>(d.image + at);
                float o[4] = {in.x, in.y, in.z, in.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = (e + j) / cg, ch = e + j - c * cg;
                    if (!kb[r * kT + c]) o[j] = upsample(f, cg, ch, y0 + r, x0 + c, hc, wc, oy1, ox1, 18);
                }
                *reinterpret_cast<float4*>(d.out + at) = make_float4(o[0], o[1], o[2], o[3]);
            }
        } else {
            const int per_row = kT * cg;
            for (int q = tid; q < kT * per_row; q += 256) {
                const int r = q / per_row, e = q - r * per_row, c = e / cg, ch = e - c * cg;
                if (r >= nr || c >= nc) continue;
                const int64_t pix = static_cast<int64_t>(y0 + r) * w0 + x0 + c;
                if (g.bottom == 0) {
                    const int64_t at = img0 + pix * C + c0 + ch;
                    d.out[at] = kb[r * kT + c] ? d.image[at] : upsample(f, cg, ch, y0 + r, x0 + c, hc, wc, oy1, ox1, 18);
                } else if (!kb[r * kT + c]) {                      // f of this level, where no block reads v in this launch
                    wv[(g.off[0] + pix) * C + c0 + ch] = upsample(f, cg, ch, y0 + r, x0 + c, hc, wc, oy1, ox1, 18);
                }
            }
        }
    }
}

// ---- outpaint canvas --------------------------------------------------------------------------------------------------------
// blockIdx.y = canvas row, blockIdx.z = image.  VEC: canvas rows, source rows and the left pad are whole float4s and all three
// bases 16-byte aligned, so a float4 of the canvas lies inside the original or outside it.
template <bool VEC>
__global__ __launch_bounds__(256) void lp_outpaint_pad_kernel(const lp_outpaint_desc d) {
    const int C = d.channels, H = d.height, W = d.width, b = blockIdx.z, y = blockIdx.y;
    const int Wc = d.left + W + d.right, Hc = d.top + H + d.bottom;
    const int sy = y - d.top;
    const bool row_in = sy >= 0 && sy < H;
    const int e0 = d.left * C, e1 = (d.left + W) * C, ne = Wc * C;
    const float* src = d.image + (static_cast<int64_t>(b) * H + (row_in ? sy : 0)) * W * C;
    float* dst = d.image_out + (static_cast<int64_t>(b) * Hc + y) * Wc * C;
    const int stride = gridDim.x * 256;
    constexpr int V = VEC ? 4 : 1;
    for (int e = (blockIdx.x * 256 + threadIdx.x) * V; e < ne; e += stride * V) {
        const bool in = row_in && e >= e0 && e < e1;
        if constexpr (VEC) {
            float4 val = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (in) val = *reinterpret_cast<const float4*>(src + (e - e0));
            *reinterpret_cast<float4*>(dst + e) = val;
        } else {
            dst[e] = in ? src[e - e0] : 0.0f;
        }
    }
    const int bm = d.mask_batch ? d.mask_batch : 1;
    if (b >= bm) return;
    const bool band_row = !row_in || (d.top > 0 && sy < d.overlap) || (d.bottom > 0 && sy >= H - d.overlap);
    const float* mrow = d.mask_batch ? d.mask + (static_cast<int64_t>(b) * H + (row_in ? sy : 0)) * W : nullptr;
    float* mdst = d.mask_out + (static_cast<int64_t>(b) * Hc + y) * Wc;
    for (int x = blockIdx.x * 256 + threadIdx.x; x < Wc; x += stride) {
        const int sx = x - d.left;
        const bool in = row_in && sx >= 0 && sx < W;
        const bool band = band_row || !in || (d.left > 0 && sx < d.overlap) || (d.right > 0 && sx >= W - d.overlap);
        const float bv = band ? 1.0f : 0.0f;
        const float m = in && mrow ? mrow[sx] : 0.0f;
        mdst[x] = m > bv ? m : bv;                                 // a NaN m gives the band
    }
}

bool side_ok(int s) { return s > 0 && s <= LP_DETAIL_MAX_SIDE; }
bool chan_ok(int c) { return c > 0 && c <= LP_DETAIL_MAX_CHANNELS; }

// The pyramid of an H x W image: sides and workspace offsets of levels 0 .. L - 1 (at most 16); returns L, *pix = the
// workspace pixels of one image.
int fill_levels(int H, int W, int32_t* h, int32_t* w, int64_t* off, int64_t* pix) {
    int L = 1;
    int64_t at = 0;
    h[0] = H; w[0] = W; off[0] = 0;
    while (h[L - 1] > 1 || w[L - 1] > 1) {
        h[L] = (h[L - 1] + 1) / 2;
        w[L] = (w[L - 1] + 1) / 2;
        off[L] = at;
        at += static_cast<int64_t>(h[L]) * w[L];
        ++L;
    }
    *pix = at;
    return L;
}

FillSpan make_span(int L, const int32_t* h, const int32_t* w, const int64_t* off, int64_t pix, int bottom) {
    FillSpan g = {};
    g.bottom = bottom;
    g.n = min(kSpan, L - 1 - bottom);
    for (int i = 0; i <= g.n; ++i) { g.h[i] = h[bottom + i]; g.w[i] = w[bottom + i]; g.off[i] = off[bottom + i]; }
    for (int i = g.n + 1; i <= kSpan; ++i) { g.h[i] = 1; g.w[i] = 1; g.off[i] = 0; }
    g.pix = pix;
    g.top_flag = L > 1 ? off[L - 1] : -1;
    return g;
}

}  // namespace

extern "C" int64_t lp_fill_ws_bytes(int32_t batch, int32_t height, int32_t width, int32_t channels) {
    if (batch <= 0 || !side_ok(height) || !side_ok(width) || !chan_ok(channels)) return LP_E_INVALID;
    if (batch > 65535) return LP_E_UNSUPPORTED;
    int32_t h[17], w[17];
    int64_t off[17], pix;
    fill_levels(height, width, h, w, off, &pix);
    const int64_t bytes = static_cast<int64_t>(batch) * pix * (4 * channels + 1);     // fp32 values, then one flag byte per pixel
    return bytes < 16 ? 16 : (bytes + 15) / 16 * 16;
}

extern "C" int lp_mask_fill(const lp_fill_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_fill_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.height) || !side_ok(d.width) || !chan_ok(d.channels)) return LP_E_INVALID;
    if (!d.image || !d.mask || !d.out || !d.ws || d.out == d.image) return LP_E_INVALID;
    if (d.mask_batch != 1 && d.mask_batch != d.batch) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    if (!aligned16(d.ws)) return LP_E_ALIGN;
    if (d.reserved0 != 0) {                                        // the patch form: its mode word, channels and larger workspace
        const int rc = patch_fill_check(d);
        if (rc != LP_OK) return rc;
    } else if (d.ws_bytes < lp_fill_ws_bytes(d.batch, d.height, d.width, d.channels)) {
        return LP_E_INVALID;
    }
    int32_t h[17], w[17];
    int64_t off[17], pix;
    const int L = fill_levels(d.height, d.width, h, w, off, &pix);
    const bool vec = d.channels <= kCG && ((d.width * d.channels) & 3) == 0 && aligned16(d.image) && aligned16(d.out);
    int last = 0;                                                  // the lowest level of the topmost span
    for (int s = 0; s < L - 1; s += kSpan) {
        const FillSpan g = make_span(L, h, w, off, pix, s);
        const dim3 grid((w[s] + kT - 1) / kT, (h[s] + kT - 1) / kT, d.batch);
        if (vec && s == 0)
            hipLaunchKernelGGL(lp_fill_pull_kernel<true>, grid, dim3(256), 0, stream, d, g);
        else
            hipLaunchKernelGGL(lp_fill_pull_kernel<false>, grid, dim3(256), 0, stream, d, g);
        if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
        last = s;
    }
    for (int s = last; s >= 0; s -= kSpan) {                       // (a 1 x 1 image: one launch that copies)
        const FillSpan g = make_span(L, h, w, off, pix, s);
        const dim3 grid((w[s] + kT - 1) / kT, (h[s] + kT - 1) / kT, d.batch);
        if (vec && s == 0)
            hipLaunchKernelGGL(lp_fill_push_kernel<true>, grid, dim3(256), 0, stream, d, g);
        else
            hipLaunchKernelGGL(lp_fill_push_kernel<false>, grid, dim3(256), 0, stream, d, g);
        if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    }
    return d.reserved0 != 0 ? patch_fill_enqueue(d, stream) : LP_OK;   // `out` is the push-pull result: the patch form's pre-fill
}

extern "C" int lp_outpaint_pad(const lp_outpaint_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_outpaint_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.height) || !side_ok(d.width) || !chan_ok(d.channels)) return LP_E_INVALID;
    if (d.left < 0 || d.top < 0 || d.right < 0 || d.bottom < 0 || d.overlap < 0) return LP_E_INVALID;
    if (d.left == 0 && d.top == 0 && d.right == 0 && d.bottom == 0) return LP_E_INVALID;
    const int64_t Hc = static_cast<int64_t>(d.top) + d.height + d.bottom, Wc = static_cast<int64_t>(d.left) + d.width + d.right;
    if (Hc > LP_DETAIL_MAX_SIDE || Wc > LP_DETAIL_MAX_SIDE) return LP_E_INVALID;
    if (d.mask_batch != 0 && d.mask_batch != 1 && d.mask_batch != d.batch) return LP_E_INVALID;
    if (!d.image || !d.image_out || !d.mask_out || (d.mask_batch != 0 && !d.mask)) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    const int C = d.channels;
    const bool vec = ((Wc * C) & 3) == 0 && ((d.width * C) & 3) == 0 && ((d.left * C) & 3) == 0 && aligned16(d.image) &&
                     aligned16(d.image_out);
    const int64_t per_block = vec ? 1024 : 256;
    const uint32_t gx = static_cast<uint32_t>(min(static_cast<int64_t>(64), (Wc * C + per_block - 1) / per_block));
    const dim3 grid(gx, static_cast<uint32_t>(Hc), d.batch);
    if (vec)
        hipLaunchKernelGGL(lp_outpaint_pad_kernel<true>, grid, dim3(256), 0, stream, d);
    else
        hipLaunchKernelGGL(lp_outpaint_pad_kernel<false>, grid, dim3(256), 0, stream, d);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

}  // namespace lp
