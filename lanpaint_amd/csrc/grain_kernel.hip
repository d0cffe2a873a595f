// grain_kernel.hip -- grain match for gfx950: measure the grain of a photograph or video frame, fit what the clean inpainted area
// lacks, and add a synthesized grain under the mask (lanpaint_amd/grain.py; the rule in full: include/lanpaint_hip.h).  Pixel
// space, last in the chain.  Four entries on the caller's stream:
//
//   lp_grain_stats  per image, channel and tone band {n, sum e1^2, sum e2^2} of two noise operators over the flat pixels of a
//                   region.  A block owns a 16 x 64 tile and four channels: the tile's 8-bit codes with a 2-pixel halo sit in
//                   LDS four to a word; the region test is two prefix sums of the mask's fail flags (rows, then columns), so a
//                   margin of 25 costs what a margin of 0 does.  A lane owns one column of four neighbouring rows and forms each
//                   row's min, max and row sums once (every operator is separable).  Integers only: a lane adds into one of 16 copies of the
//                   block's 32-bit LDS counters (a copy sees at most 64 pixels: no overflow, a quarter of the same-address
//                   traffic), the block then adds its non-zero sums into the table with 64-bit integer atomics.
//   lp_grain_fit    one block per clip, a thread per (channel, band): pool, energies, nearest valid band, need, size, amplitude.
//   lp_grain_field  the integer grain alone, and
//   lp_grain_apply  out = image + (m * a) * g: one kernel, a block per tile and four channels.  Each white value of the tile's
//                   lattice (halo = the grain size) is computed once -- one Philox4x32-10 block gives the four channels --, kept
//                   as 4 x int16 per point in LDS, filtered along x into a second LDS image and along y into registers.
//
// The library is built with -ffp-contract=on: every floating-point step goes through __fmul_rn / __dadd_rn and friends.
// Entry points defined here: lp_grain_stats, lp_grain_fit, lp_grain_field, lp_grain_apply.
#include "lp_common.h"

namespace lp {
namespace {

constexpr int kTH = LP_GRAIN_TILE_H, kTW = LP_GRAIN_TILE_W, kK = LP_GRAIN_BANDS, kMaxM = LP_GRAIN_MAX_MARGIN;
constexpr int kCopies = 16;                         // copies of the block's counters; lane l adds into copy l % 16
constexpr int kEntries = 4 * kK * 3;                // four channels x bands x {n, e1^2, e2^2}

static_assert(kTW == 64 && kTH == 16, "a lane owns column tid % 64; of four rows: 4 wave + j (stats), wave + 4 j (grain)");
static_assert(255 * 8 * 255 * 8 * (kTH * kTW / kCopies) < (1ll << 32), "a copy's sum of squares stays inside 32 bits");

// codes of channels c0 .. c0 + 3 (those below C) of pixel (y, x) of image b, channel c0 in bits 0..7
__device__ __forceinline__ uint32_t codes4(const float* __restrict__ image, int b, int y, int x, int H, int W, int C, int c0) {
    const float* p = image + ((static_cast<int64_t>(b) * H + y) * W + x) * C + c0;
    uint32_t w = static_cast<uint32_t>(code_of(p[0]));
    if (c0 + 1 < C) w |= static_cast<uint32_t>(code_of(p[1])) << 8;
    if (c0 + 2 < C) w |= static_cast<uint32_t>(code_of(p[2])) << 16;
    if (c0 + 3 < C) w |= static_cast<uint32_t>(code_of(p[3])) << 24;
    return w;
}

__device__ __forceinline__ int byte_of(uint32_t w, int j) { return static_cast<int>((w >> (8 * j)) & 0xffu); }

// ---- statistics -----------------------------------------------------------------------------------------------------------
// grid: x = tile (row-major over the image), y = image, z = group of four channels
__global__ __launch_bounds__(256) void lp_grain_stats_kernel(const lp_grain_stats_desc d, const int tiles_x) {
    __shared__ uint32_t q[kTH + 4][kTW + 4];
    __shared__ uint16_t fail[kTH + 2 * kMaxM][kTW + 2 * kMaxM + 2];      // [r][1 + i]: the flag, then the row's prefix sum
    __shared__ uint16_t vert[kTH + 2 * kMaxM + 1][kTW];                 // prefix sums down the columns of the widened rows
    __shared__ uint32_t acc[kEntries][kCopies];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int H = d.height, W = d.width, C = d.channels;
    const int b = blockIdx.y, c0 = blockIdx.z * 4;
    const int ty0 = blockIdx.x / tiles_x, y0 = ty0 * kTH, x0 = (blockIdx.x - ty0 * tiles_x) * kTW;
    for (int i = tid; i < kEntries * kCopies; i += 256) (&acc[0][0])[i] = 0u;
    for (int i = tid; i < (kTH + 4) * (kTW + 4); i += 256) {
        const int r = i / (kTW + 4), cx = i - r * (kTW + 4);
        const int y = y0 - 2 + r, x = x0 - 2 + cx;
        q[r][cx] = (y >= 0 && y < H && x >= 0 && x < W) ? codes4(d.image, b, y, x, H, W, C, c0) : 0u;
    }
    const bool masked = d.region != LP_GRAIN_REGION_ALL;                // block-uniform
    const int m = d.region == LP_GRAIN_REGION_OUTSIDE ? d.margin : 2;
    const int rows = kTH + 2 * m, cols = kTW + 2 * m;
    if (masked) {
        const float* plane = d.mask + static_cast<int64_t>(d.mask_batch == 1 ? 0 : b) * H * W;
        const bool outside = d.region == LP_GRAIN_REGION_OUTSIDE;
        for (int r = wave; r < rows; r += 4) {
            const int y = y0 - m + r;
            for (int i = lane; i < cols; i += kWave) {
                const int x = x0 - m + i;
                uint16_t f = 0;
                if (y >= 0 && y < H && x >= 0 && x < W) {               // elements outside the image do not count
                    const float v = plane[static_cast<int64_t>(y) * W + x];
                    f = outside ? !(v <= 0.5f) : !(v > 0.5f);
                }
                fail[r][1 + i] = f;
            }
        }
        __syncthreads();
        if (tid < rows) {                                               // fail[r][i] = flags of columns [0, i)
            uint16_t s = 0;
            fail[tid][0] = 0;
            for (int i = 1; i <= cols; ++i) {
                s = static_cast<uint16_t>(s + fail[tid][i]);
                fail[tid][i] = s;
            }
        }
        __syncthreads();
        if (tid < kTW) {                                                // vert[r][x] = widened flags of rows [0, r)
            uint16_t s = 0;
            vert[0][tid] = 0;
            for (int r = 0; r < rows; ++r) {
                s = static_cast<uint16_t>(s + (fail[r][tid + 2 * m + 1] != fail[r][tid] ? 1 : 0));
                vert[r + 1][tid] = s;
            }
        }
    }
    __syncthreads();
    // a lane owns column tx of the four rows 4 wave .. 4 wave + 3: their windows share eight rows of five codes, and every
    // operator is separable, so a row's min, max and three row sums are formed once and used by up to five pixels
    const int tx = lane, x = x0 + tx, tyb = 4 * wave;
    bool take[4], any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ty = tyb + j, y = y0 + ty;
        take[j] = y >= 2 && y < H - 2 && x >= 2 && x < W - 2;
        if (take[j] && masked) take[j] = vert[ty + 2 * m + 1][tx] == vert[ty][tx];
        any |= take[j];
    }
    if (any) {
        uint32_t w[8][5];
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) w[r][dx] = q[tyb + r][tx + dx];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (c0 + ch >= C) break;                                    // block-uniform
            int lo[8], hi[8], hb[8], hn[8], h5[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int v0 = byte_of(w[r][0], ch), v1 = byte_of(w[r][1], ch), v2 = byte_of(w[r][2], ch),
                          v3 = byte_of(w[r][3], ch), v4 = byte_of(w[r][4], ch);
                lo[r] = min(min(min(v0, v1), min(v2, v3)), v4);
                hi[r] = max(max(max(v0, v1), max(v2, v3)), v4);
                hb[r] = v1 + 2 * v2 + v3;                               // [1 2 1]
                hn[r] = v1 - 2 * v2 + v3;                               // [1 -2 1]
                h5[r] = v0 - 2 * v2 + v4;                               // [1 0 -2 0 1]
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!take[j]) continue;
                const int l = min(min(min(lo[j], lo[j + 1]), min(lo[j + 2], lo[j + 3])), lo[j + 4]);
                const int h = max(max(max(hi[j], hi[j + 1]), max(hi[j + 2], hi[j + 3])), hi[j + 4]);
                if (h - l > d.flat) continue;
                const int mu16 = hb[j + 1] + 2 * hb[j + 2] + hb[j + 3];
                const int e1 = hn[j + 1] - 2 * hn[j + 2] + hn[j + 3];
                const int e2 = h5[j] - 2 * h5[j + 2] + h5[j + 4];
                const int band = (mu16 * kK) / 4081;
                uint32_t* e = &acc[(ch * kK + band) * 3][lane & (kCopies - 1)];
                atomicAdd(e, 1u);
                atomicAdd(e + kCopies, static_cast<uint32_t>(e1 * e1));
                atomicAdd(e + 2 * kCopies, static_cast<uint32_t>(e2 * e2));
            }
        }
    }
    __syncthreads();
    if (tid < kEntries) {
        const int ch = tid / (kK * 3);
        unsigned long long s = 0;
#pragma unroll
        for (int k = 0; k < kCopies; ++k) s += acc[tid][k];
        if (c0 + ch < C && s != 0)
            atomicAdd(reinterpret_cast<unsigned long long*>(d.stats) + (static_cast<int64_t>(b) * C + c0) * (kK * 3) + tid, s);
    }
}

// ---- fit ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pooled(const int64_t* __restrict__ t, int first, int count, int C, int entry) {
    double s = 0.0;
    for (int i = first; i < first + count; ++i)
        s = __dadd_rn(s, static_cast<double>(t[(static_cast<int64_t>(i) * C * kK * 3) + entry]));
    return s;
}

// the nearest band of this thread's channel with valid[] set, the lower index on a tie; -1: none
__device__ __forceinline__ int nearest_valid(const int* valid, int base, int k) {
    for (int dist = 0; dist < kK; ++dist) {
        if (k - dist >= 0 && valid[base + k - dist]) return k - dist;
        if (k + dist < kK && valid[base + k + dist]) return k + dist;
    }
    return -1;
}

// one block per clip; thread t < C * K is (channel t / K, band t % K)
__global__ __launch_bounds__(512) void lp_grain_fit_kernel(const lp_grain_fit_desc d) {
    constexpr int kMax = LP_DETAIL_MAX_CHANNELS * kK;
    __shared__ double e1s[2][kMax], e2s[2][kMax];                       // [0]: gen, [1]: ref
    __shared__ int valid[2][kMax];
    __shared__ double need1[kMax], need2[kMax];
    __shared__ int chosen[2];                                           // size, every amplitude 0
    const int t = threadIdx.x, C = d.channels, n_ck = C * kK;
    const int L = d.clip_frames ? d.clip_frames : d.batch, first = blockIdx.x * L;
    const bool own = t < n_ck;
    if (own) {
        const bool plate = d.ref_batch != d.batch;
        for (int side = 0; side < 2; ++side) {
            const int64_t* tab = side ? d.ref : d.gen;
            const int f0 = side && plate ? 0 : first, cnt = side && plate ? d.ref_batch : L;
            const double n = pooled(tab, f0, cnt, C, 3 * t), s1 = pooled(tab, f0, cnt, C, 3 * t + 1),
                         s2 = pooled(tab, f0, cnt, C, 3 * t + 2);
            const bool ok = n >= static_cast<double>(LP_GRAIN_MIN_COUNT);
            valid[side][t] = ok;
            e1s[side][t] = ok ? __ddiv_rn(s1, n) : 0.0;
            e2s[side][t] = ok ? __ddiv_rn(s2, n) : 0.0;
        }
    }
    __syncthreads();
    double n1 = 0.0, n2 = 0.0;
    if (own) {
        const int base = (t / kK) * kK, k = t - base;
        const int kg = nearest_valid(valid[0], base, k), kr = nearest_valid(valid[1], base, k);
        if (kr >= 0) {
            const double g1 = kg >= 0 ? e1s[0][base + kg] : 0.0, g2 = kg >= 0 ? e2s[0][base + kg] : 0.0;
            const double d1 = __dsub_rn(e1s[1][base + kr], g1), d2 = __dsub_rn(e2s[1][base + kr], g2);
            n1 = d1 > 0.0 ? d1 : 0.0;
            n2 = d2 > 0.0 ? d2 : 0.0;
        }
        need1[t] = n1;
        need2[t] = n2;
    }
    __syncthreads();
    if (t == 0) {
        int s = d.size, none = 0;
        if (s < 0) {
            double A = 0.0, Bq = 0.0;
            for (int i = 0; i < n_ck; ++i) {
                A = __dadd_rn(A, need1[i]);
                Bq = __dadd_rn(Bq, need2[i]);
            }
            if (!(A > 0.0)) { s = 0; none = 1; }
            else if (__dmul_rn(3.0, Bq) < __dmul_rn(14.0, A)) s = 0;
            else if (Bq < __dmul_rn(33.0, A)) s = 1;
            else s = 2;
        }
        chosen[0] = s;
        chosen[1] = none;
    }
    __syncthreads();
    const int s = chosen[0];
    if (own) {
        // V * (S1_s + S2_s) and V * sum k_s^2, exact integers
        const double V = static_cast<double>(LP_GRAIN_WHITE_VAR);
        const double den = s == 0 ? V * 72.0 : s == 1 ? V * 820.0 : V * 39988.0;
        const double pow_s = s == 0 ? V * 1.0 : s == 1 ? V * 36.0 : V * 4900.0;
        double a = __dmul_rn(d.strength, __dsqrt_rn(__ddiv_rn(__dadd_rn(n1, n2), den)));
        const double cap = __ddiv_rn(static_cast<double>(LP_GRAIN_MAX_STD), __dsqrt_rn(pow_s));
        a = a < cap ? a : cap;
        if (chosen[1]) a = 0.0;
        const float amp = static_cast<float>(__ddiv_rn(a, 255.0));
        for (int f = 0; f < L; ++f) d.amp[static_cast<int64_t>(first + f) * n_ck + t] = amp;
    }
    for (int f = t; f < L; f += 512) d.size_out[first + f] = s;
}

// ---- field and apply --------------------------------------------------------------------------------------------------------
struct GrainArgs {
    int32_t batch, height, width, channels, mask_batch, monochrome, size;
    int64_t frame0;
    uint64_t seed;
    const float* image;
    const float* mask;
    const float* amp;
    const int32_t* size_tab;
    float* out;
    int32_t* field;
};

__device__ __forceinline__ int lo16(uint32_t w) { return static_cast<int16_t>(w & 0xffffu); }
__device__ __forceinline__ int hi16(uint32_t w) { return static_cast<int>(w) >> 16; }
__device__ __forceinline__ uint32_t pack16(int lo, int hi) { return (static_cast<uint32_t>(lo) & 0xffffu) | (static_cast<uint32_t>(hi) << 16); }
__device__ __forceinline__ int white_of(uint32_t word) {               // the sum of the four bytes, minus 510
    return static_cast<int>((word & 0xffu) + ((word >> 8) & 0xffu) + ((word >> 16) & 0xffu) + (word >> 24)) - 510;
}

// grid: x = tile (row-major over the image), y = image, z = group of four channels.  FIELD: the integer grain to a.field.
template <bool FIELD>
__global__ __launch_bounds__(256) void lp_grain_kernel(const GrainArgs a, const int tiles_x) {
    __shared__ uint2 white[kTH + 4][kTW + 4];                           // 4 x int16: channels c0 .. c0 + 3 of a lattice point
    __shared__ uint2 horiz[kTH + 4][kTW];
    __shared__ uint32_t q[FIELD ? 1 : kTH + 2][FIELD ? 1 : kTW + 2];
    __shared__ float amps[4][kK];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int H = a.height, W = a.width, C = a.channels;
    const int b = blockIdx.y, grp = blockIdx.z, c0 = grp * 4;
    const int ty0 = blockIdx.x / tiles_x, y0 = ty0 * kTH, x0 = (blockIdx.x - ty0 * tiles_x) * kTW;
    int s = FIELD ? a.size : a.size_tab[b];
    s = s < 0 ? 0 : s > 2 ? 2 : s;
    const int w0 = s == 2 ? 1 : 0, w1 = s == 2 ? 4 : s, w2 = s == 2 ? 6 : s + 1;      // [w0 w1 w2 w1 w0]
    const uint64_t subseq = static_cast<uint64_t>(a.frame0 + b) * 16u + (a.monochrome ? 0u : static_cast<uint64_t>(grp));
    for (int i = tid; i < (kTH + 4) * (kTW + 4); i += 256) {
        const int r = i / (kTW + 4), cx = i - r * (kTW + 4);
        const int ly = y0 - 2 + r, lx = x0 - 2 + cx;                    // lattice point (ly, lx), -2 <= ly < H + 2
        uint2 v = make_uint2(0u, 0u);
        // needed: within s of a pixel of this tile that lies inside the image
        if (r >= 2 - s && r < kTH + 2 + s && cx >= 2 - s && cx < kTW + 2 + s && ly < H + s && lx < W + s) {
            const uint64_t ctr = static_cast<uint64_t>(ly + 2) * static_cast<uint64_t>(W + 4) + static_cast<uint64_t>(lx + 2);
            const uint4 blk = philox4x32_10<true>(ctr, subseq, a.seed);
            const int v0 = white_of(blk.x);
            if (a.monochrome) v = make_uint2(pack16(v0, v0), pack16(v0, v0));
            else v = make_uint2(pack16(v0, white_of(blk.y)), pack16(white_of(blk.z), white_of(blk.w)));
        }
        white[r][cx] = v;
    }
    if constexpr (!FIELD) {
        for (int i = tid; i < (kTH + 2) * (kTW + 2); i += 256) {        // the image's codes, coordinates clamped
            const int r = i / (kTW + 2), cx = i - r * (kTW + 2);
            const int y = min(max(y0 - 1 + r, 0), H - 1), x = min(max(x0 - 1 + cx, 0), W - 1);
            q[r][cx] = codes4(a.image, b, y, x, H, W, C, c0);
        }
        if (tid < 4 * kK) {
            const int ch = tid / kK;
            amps[ch][tid - ch * kK] = c0 + ch < C ? a.amp[(static_cast<int64_t>(b) * C + c0 + ch) * kK + (tid - ch * kK)] : 0.0f;
        }
    }
    __syncthreads();
    for (int i = tid; i < (kTH + 4) * kTW; i += 256) {                  // along x: |sum| <= 16 * 510, inside int16
        const int r = i >> 6, tx = i & (kTW - 1);
        const uint2 p0 = white[r][tx], p1 = white[r][tx + 1], p2 = white[r][tx + 2], p3 = white[r][tx + 3], p4 = white[r][tx + 4];
        const int h0 = w0 * (lo16(p0.x) + lo16(p4.x)) + w1 * (lo16(p1.x) + lo16(p3.x)) + w2 * lo16(p2.x);
        const int h1 = w0 * (hi16(p0.x) + hi16(p4.x)) + w1 * (hi16(p1.x) + hi16(p3.x)) + w2 * hi16(p2.x);
        const int h2 = w0 * (lo16(p0.y) + lo16(p4.y)) + w1 * (lo16(p1.y) + lo16(p3.y)) + w2 * lo16(p2.y);
        const int h3 = w0 * (hi16(p0.y) + hi16(p4.y)) + w1 * (hi16(p1.y) + hi16(p3.y)) + w2 * hi16(p2.y);
        horiz[r][tx] = make_uint2(pack16(h0, h1), pack16(h2, h3));
    }
    __syncthreads();
    const int tx = lane, x = x0 + tx;
    if (x >= W) return;
#pragma unroll 1
    for (int j = 0; j < kTH / 4; ++j) {
        const int ty = wave + 4 * j, y = y0 + ty;
        if (y >= H) break;
        const uint2 p0 = horiz[ty][tx], p1 = horiz[ty + 1][tx], p2 = horiz[ty + 2][tx], p3 = horiz[ty + 3][tx], p4 = horiz[ty + 4][tx];
        int g[4];
        g[0] = w0 * (lo16(p0.x) + lo16(p4.x)) + w1 * (lo16(p1.x) + lo16(p3.x)) + w2 * lo16(p2.x);
        g[1] = w0 * (hi16(p0.x) + hi16(p4.x)) + w1 * (hi16(p1.x) + hi16(p3.x)) + w2 * hi16(p2.x);
        g[2] = w0 * (lo16(p0.y) + lo16(p4.y)) + w1 * (lo16(p1.y) + lo16(p3.y)) + w2 * lo16(p2.y);
        g[3] = w0 * (hi16(p0.y) + hi16(p4.y)) + w1 * (hi16(p1.y) + hi16(p3.y)) + w2 * hi16(p2.y);
        const int64_t at = ((static_cast<int64_t>(b) * H + y) * W + x) * C + c0;
        if constexpr (FIELD) {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch)
                if (c0 + ch < C) a.field[at + ch] = g[ch];
        } else {
            const float mv = a.mask[(static_cast<int64_t>(a.mask_batch == 1 ? 0 : b) * H + y) * W + x];
            const float m = mv > 0.0f ? (mv < 1.0f ? mv : 1.0f) : 0.0f;  // a NaN gives 0
            uint32_t cw[3][3];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) cw[dy][dx] = q[ty + dy][tx + dx];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                if (c0 + ch >= C) break;                                // block-uniform
                const float v = a.image[at + ch];
                const int mu16 = byte_of(cw[0][0], ch) + byte_of(cw[0][2], ch) + byte_of(cw[2][0], ch) + byte_of(cw[2][2], ch) +
                                 2 * (byte_of(cw[0][1], ch) + byte_of(cw[1][0], ch) + byte_of(cw[1][2], ch) + byte_of(cw[2][1], ch)) +
                                 4 * byte_of(cw[1][1], ch);
                float u = __fsub_rn(__fdiv_rn(static_cast<float>(mu16 * kK), 4080.0f), 0.5f);
                u = u > 0.0f ? u : 0.0f;
                u = u < static_cast<float>(kK - 1) ? u : static_cast<float>(kK - 1);
                const int k0 = min(static_cast<int>(u), kK - 2);
                const float f = __fsub_rn(u, static_cast<float>(k0));
                const float a0 = amps[ch][k0], a1 = amps[ch][k0 + 1];
                const float amp = __fadd_rn(a0, __fmul_rn(f, __fsub_rn(a1, a0)));
                const float t = __fmul_rn(m, amp);
                const float o = __fadd_rn(v, __fmul_rn(t, static_cast<float>(g[ch])));
                a.out[at + ch] = t == 0.0f ? v : o;
            }
        }
    }
}

bool side_ok(int s) { return s > 0 && s <= LP_DETAIL_MAX_SIDE; }
bool chan_ok(int c) { return c > 0 && c <= LP_DETAIL_MAX_CHANNELS; }

dim3 tile_grid(int batch, int H, int W, int C, int* tiles_x) {
    *tiles_x = (W + kTW - 1) / kTW;
    return dim3(static_cast<uint32_t>(*tiles_x) * static_cast<uint32_t>((H + kTH - 1) / kTH), batch, (C + 3) / 4);
}

}  // namespace

extern "C" int lp_grain_stats(const lp_grain_stats_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_grain_stats_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.height) || !side_ok(d.width) || !chan_ok(d.channels)) return LP_E_INVALID;
    if (d.region != LP_GRAIN_REGION_ALL && d.region != LP_GRAIN_REGION_OUTSIDE && d.region != LP_GRAIN_REGION_INSIDE)
        return LP_E_INVALID;
    if (d.margin < 0 || d.margin > LP_GRAIN_MAX_MARGIN || d.flat < 0 || d.flat > 255) return LP_E_INVALID;
    if (!d.image || !d.stats) return LP_E_INVALID;
    if (d.region != LP_GRAIN_REGION_ALL && (!d.mask || (d.mask_batch != 1 && d.mask_batch != d.batch))) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    const size_t bytes = static_cast<size_t>(d.batch) * d.channels * kK * 3 * sizeof(int64_t);
    if (hipMemsetAsync(d.stats, 0, bytes, stream) != hipSuccess) return LP_E_LAUNCH;
    if (d.height < 5 || d.width < 5) return LP_OK;                      // no pixel has its 5 x 5 window inside the image
    int tiles_x;
    const dim3 grid = tile_grid(d.batch, d.height, d.width, d.channels, &tiles_x);
    hipLaunchKernelGGL(lp_grain_stats_kernel, grid, dim3(256), 0, stream, d, tiles_x);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

extern "C" int lp_grain_fit(const lp_grain_fit_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_grain_fit_desc& d = *dp;
    if (d.batch <= 0 || d.ref_batch <= 0 || !chan_ok(d.channels)) return LP_E_INVALID;
    if (!d.gen || !d.ref || !d.amp || !d.size_out) return LP_E_INVALID;
    if (d.clip_frames < 0 || (d.clip_frames > 0 && d.batch % d.clip_frames != 0)) return LP_E_INVALID;
    if (d.size < LP_GRAIN_SIZE_AUTO || d.size > 2) return LP_E_INVALID;
    if (!(d.strength >= 0.0 && d.strength <= 2.0)) return LP_E_INVALID;
    if (d.batch > 65535 || d.ref_batch > 65535) return LP_E_UNSUPPORTED;
    const int clips = d.clip_frames ? d.batch / d.clip_frames : 1;
    hipLaunchKernelGGL(lp_grain_fit_kernel, dim3(clips), dim3(512), 0, stream, d);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

extern "C" int lp_grain_field(const lp_grain_field_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_grain_field_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.height) || !side_ok(d.width) || !chan_ok(d.channels)) return LP_E_INVALID;
    if (d.size < 0 || d.size > 2 || !d.out) return LP_E_INVALID;
    if (d.frame0 < 0 || d.frame0 > LP_GRAIN_MAX_FRAME0) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    GrainArgs a{d.batch, d.height, d.width, d.channels, 1, d.monochrome != 0, d.size, d.frame0, d.seed,
                nullptr, nullptr, nullptr, nullptr, nullptr, d.out};
    int tiles_x;
    const dim3 grid = tile_grid(d.batch, d.height, d.width, d.channels, &tiles_x);
    hipLaunchKernelGGL(lp_grain_kernel<true>, grid, dim3(256), 0, stream, a, tiles_x);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

extern "C" int lp_grain_apply(const lp_grain_apply_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_grain_apply_desc& d = *dp;
    if (d.batch <= 0 || !side_ok(d.height) || !side_ok(d.width) || !chan_ok(d.channels)) return LP_E_INVALID;
    if (!d.image || !d.mask || !d.amp || !d.size || !d.out || d.out == d.image) return LP_E_INVALID;
    if (d.mask_batch != 1 && d.mask_batch != d.batch) return LP_E_INVALID;
    if (d.frame0 < 0 || d.frame0 > LP_GRAIN_MAX_FRAME0) return LP_E_INVALID;
    if (d.batch > 65535) return LP_E_UNSUPPORTED;
    GrainArgs a{d.batch, d.height, d.width, d.channels, d.mask_batch, d.monochrome != 0, 0, d.frame0, d.seed,
                d.image, d.mask, d.amp, d.size, d.out, nullptr};
    int tiles_x;
    const dim3 grid = tile_grid(d.batch, d.height, d.width, d.channels, &tiles_x);
    hipLaunchKernelGGL(lp_grain_kernel<false>, grid, dim3(256), 0, stream, a, tiles_x);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

}  // namespace lp
