// focus_kernel.hip -- focus match for gfx950 (lanpaint_amd/focus.py): the focus form of lp_multiband_blend, a negative `levels`.
// include/lanpaint_hip.h ("the focus form") states the rule; multiband_kernel.hip holds the entry and dispatches here on the sign.
//
//   flags    one block per 32 x 32 tile of a mask plane: bit 0 a pixel > 0.5, bit 1 a pixel with m > 0.  The first block clears the
//            statistics, so no memset is needed and no byte of the workspace is read before it is written.
//   stats    one block per tile and image, gone at once unless a marked tile lies within `ring` tiles.  The mask's support (42 x 42,
//            one byte a pixel: not masked / masked / outside) goes to LDS once and is counted separably over 11 x 11; per region the
//            tile's luma codes with their 5-pixel halo (42 x 42 bytes, four to a dword) go to LDS once and both binomial planes are
//            built from them separably (34 x 34 each: the tile and the ring of the central differences).  Sums per lane in 64-bit
//            integers, per wave through shuffles, then one 64-bit atomic per wave and figure: integer sums, any order the same bits.
//   fit      one block.  The pooled form first adds the rows up (64-bit LDS atomics); then a lane per image does the fp64 fit and
//            writes the image's 67 taps from a table of binomial coefficients built at compile time.
//   blur     two launches of one kernel through the workspace plane, rows then columns, 32 x 32 tiles; the taps in LDS, the
//            samples read from global memory (a tile's rows are contiguous and the taps walk along or across them, so the lines
//            stay in L1 / L2).  One launch with the tile and a 33-pixel halo in LDS would need 98 x 98 x 16 bytes = 150 KB at four
//            channels of the CU's 160 KB: one block a CU and no room to hide the staging; the plane costs one write and one read.
//            A tile without m > 0 copies; the rows pass leaves out every tile no column pass reads; K = 0 copies.
// Every float operation is one __f*_rn call or stands under `fp contract(off)`.  No array is indexed by a register: no scratch.
#include "motion_tile.h"

namespace lp {
namespace {

constexpr int kT = LP_FOCUS_TILE, kHalo = 5, kS = kT + 2 * kHalo, kG = kT + 2;
constexpr int kTapR = (LP_FOCUS_TAPS - 1) / 2;                       // 33

struct FocusWs {
    uint8_t* flags;
    unsigned long long* stats;
    double* var;
    int32_t* K;
    float* taps;
    float* plane;
};

FocusWs focus_ws(const lp_multiband_desc& d) {
    char* p = static_cast<char*>(d.ws);
    const int64_t b = d.batch, h = d.height, w = d.width, c = d.channels;
    return {reinterpret_cast<uint8_t*>(p + LP_FOCUS_WS_FLAGS(b, h, w, c)),
            reinterpret_cast<unsigned long long*>(p + LP_FOCUS_WS_STATS(b, h, w, c)),
            reinterpret_cast<double*>(p + LP_FOCUS_WS_VAR(b, h, w, c)), reinterpret_cast<int32_t*>(p + LP_FOCUS_WS_K(b, h, w, c)),
            reinterpret_cast<float*>(p + LP_FOCUS_WS_TAPS(b, h, w, c)), reinterpret_cast<float*>(p + LP_FOCUS_WS_PLANE(b, h, w, c))};
}

struct FocusWord {
    int edge, ring, strength16, per_frame;
    bool ok;
};

FocusWord focus_word(int32_t levels) {
    const uint32_t u = static_cast<uint32_t>(levels);
    FocusWord f = {static_cast<int>(u & 255u), static_cast<int>((u >> 8) & 15u), static_cast<int>((u >> 12) & 31u),
                   static_cast<int>((u >> 17) & 1u), false};
    f.ok = (u >> 31) == 1u && ((u >> 18) & 0x1FFFu) == 0u && f.edge >= 1 && f.ring >= 1 && f.ring <= LP_FOCUS_MAX_RING &&
           f.strength16 <= 16;
    return f;
}

__device__ __forceinline__ float focus_weight(float m) { return m > 0.0f ? (m < 1.0f ? m : 1.0f) : 0.0f; }      // a NaN gives 0

// the flags of image `mi`'s tile (ty, tx); 0 outside the grid
__device__ __forceinline__ int tile_flag(const uint8_t* flags, int mi, int th, int tw, int ty, int tx) {
    if (ty < 0 || ty >= th || tx < 0 || tx >= tw) return 0;
    return flags[(static_cast<int64_t>(mi) * th + ty) * tw + tx];
}

// ---- flags ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lp_focus_flags_kernel(const lp_multiband_desc d, const FocusWs ws) {
    const int H = d.height, W = d.width, y0 = blockIdx.y * kT, x0 = blockIdx.x * kT;
    const float* m = d.mask + static_cast<int64_t>(blockIdx.z) * H * W;
    int f = 0;
    for (int it = threadIdx.x; it < kT * kT; it += 256) {
        const int y = y0 + (it >> 5), x = x0 + (it & 31);
        if (y < H && x < W) {
            const float v = m[static_cast<int64_t>(y) * W + x];
            f |= (v > 0.5f ? 1 : 0) | (v > 0.0f ? 2 : 0);
        }
    }
    const int marked = __syncthreads_or(f & 1), soft = __syncthreads_or(f & 2);
    if (threadIdx.x == 0)
        ws.flags[(static_cast<int64_t>(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] =
            static_cast<uint8_t>((marked ? 1 : 0) | (soft ? 2 : 0));
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int i = threadIdx.x; i < d.batch * 6; i += 256) ws.stats[i] = 0ull;
}

// ---- stats ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long wave_total(unsigned long long v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

// One region of one tile: the codes of `src` to LDS, both planes, the sums over the pixels whose s_r is `want`.
__device__ __forceinline__ void focus_region(const float* __restrict__ src, int H, int W, int C, int y0, int x0, bool stage, int want,
                                             long long thr, uint8_t* s_y, const uint8_t* s_r, int32_t* s_ha, int32_t* s_hb,
                                             int32_t* s_a, int32_t* s_b, unsigned long long* out) {
    const int tid = threadIdx.x;
    if (stage) {
        __syncthreads();                                             // the previous region's reads are done
        for (int it = tid; it < kS * kS; it += 256) {
            const int r = it / kS, c = it - r * kS, y = y0 - kHalo + r, x = x0 - kHalo + c;
            int v = 0;                                               // outside: read by no pixel that takes part
            if (y >= 0 && y < H && x >= 0 && x < W) v = luma_of(src + (static_cast<int64_t>(y) * W + x) * C, C);
            s_y[it] = static_cast<uint8_t>(v);
        }
        __syncthreads();
        for (int it = tid; it < kS * kG; it += 256) {                // along x: column g is pixel x0 - 1 + g, code column g + 4
            const int r = it / kG, g = it - r * kG;
            const uint8_t* q = s_y + r * kS + g;
            s_ha[it] = q[3] + 2 * q[4] + q[5];
            s_hb[it] = q[0] + 8 * q[1] + 28 * q[2] + 56 * q[3] + 70 * q[4] + 56 * q[5] + 28 * q[6] + 8 * q[7] + q[8];
        }
        __syncthreads();
        for (int it = tid; it < kG * kG; it += 256) {                // along y: row g is pixel y0 - 1 + g, code row g + 4
            const int g = it / kG, c = it - g * kG;
            const int32_t *qa = s_ha + g * kG + c, *qb = s_hb + g * kG + c;
            s_a[it] = qa[3 * kG] + 2 * qa[4 * kG] + qa[5 * kG];
            s_b[it] = qb[0] + 8 * qb[kG] + 28 * qb[2 * kG] + 56 * qb[3 * kG] + 70 * qb[4 * kG] + 56 * qb[5 * kG] + 28 * qb[6 * kG] +
                      8 * qb[7 * kG] + qb[8 * kG];
        }
        __syncthreads();
    }
    unsigned long long n = 0, sa = 0, sb = 0;
    for (int it = tid; it < kT * kT; it += 256) {
        if (s_r[it] != want) continue;
        const int at = ((it >> 5) + 1) * kG + (it & 31) + 1;
        const long long ax = s_a[at + 1] - s_a[at - 1], ay = s_a[at + kG] - s_a[at - kG];
        const long long bx = static_cast<long long>(s_b[at + 1]) - s_b[at - 1], by = static_cast<long long>(s_b[at + kG]) - s_b[at - kG];
        const long long gb = bx * bx + by * by;
        if (gb >= thr) {
            n += 1;
            sa += static_cast<unsigned long long>(ax * ax + ay * ay);
            sb += static_cast<unsigned long long>(gb >> 16);
        }
    }
    n = wave_total(n); sa = wave_total(sa); sb = wave_total(sb);
    if ((tid & (kWave - 1)) == 0 && n) {
        atomicAdd(out, n);
        atomicAdd(out + 1, sa);
        atomicAdd(out + 2, sb);
    }
}

__global__ __launch_bounds__(256) void lp_focus_stats_kernel(const lp_multiband_desc d, const FocusWs ws, int edge, int ring) {
    __shared__ uint8_t s_m[kS * kS];                                 // 0 not masked, 1 masked, 2 outside the image
    __shared__ uint8_t s_y[kS * kS];
    __shared__ uint16_t s_c[kS * kT];                                // over 11 along x: masked | outside << 8
    __shared__ uint8_t s_r[kT * kT];                                 // 1 ring, 2 inside
    __shared__ int32_t s_ha[kS * kG], s_hb[kS * kG], s_a[kG * kG], s_b[kG * kG];
    const int tid = threadIdx.x, H = d.height, W = d.width, C = d.channels, img = blockIdx.z;
    const int th = gridDim.y, tw = gridDim.x, ty = blockIdx.y, tx = blockIdx.x, y0 = ty * kT, x0 = tx * kT;
    const int mi = d.mask_batch == 1 ? 0 : img;
    const int span = 2 * ring + 1;
    int near = 0;
    for (int it = tid; it < span * span; it += 256) near |= tile_flag(ws.flags, mi, th, tw, ty - ring + it / span, tx - ring + it % span) & 1;
    if (!__syncthreads_or(near)) return;
    const float* m = d.mask + static_cast<int64_t>(mi) * H * W;
    for (int it = tid; it < kS * kS; it += 256) {
        const int r = it / kS, c = it - r * kS, y = y0 - kHalo + r, x = x0 - kHalo + c;
        int v = 2;
        if (y >= 0 && y < H && x >= 0 && x < W) v = m[static_cast<int64_t>(y) * W + x] > 0.5f ? 1 : 0;
        s_m[it] = static_cast<uint8_t>(v);
    }
    __syncthreads();
    for (int it = tid; it < kS * kT; it += 256) {
        const int r = it >> 5, c = it & 31;
        const uint8_t* q = s_m + r * kS + c;
        int cm = 0, co = 0;
#pragma unroll
        for (int k = 0; k < 2 * kHalo + 1; ++k) {
            cm += q[k] == 1;
            co += q[k] == 2;
        }
        s_c[it] = static_cast<uint16_t>(cm | (co << 8));
    }
    __syncthreads();
    int has = 0;
    for (int it = tid; it < kT * kT; it += 256) {
        const int i = it >> 5, j = it & 31;
        int sum = 0;
#pragma unroll
        for (int k = 0; k < 2 * kHalo + 1; ++k) sum += s_c[(i + k) * kT + j];
        int reg = 0;                                                 // (a support that leaves the image: sum >> 8 != 0)
        if (y0 + i < H && x0 + j < W && (sum >> 8) == 0) reg = sum == 121 ? 2 : (sum == 0 ? 1 : 0);
        s_r[it] = static_cast<uint8_t>(reg);
        has |= reg;
    }
    const int any_ring = __syncthreads_or(has & 1), any_inside = __syncthreads_or(has & 2);
    const long long e = static_cast<long long>(edge) * 2 * 65536, thr = e * e;
    unsigned long long* out = ws.stats + static_cast<int64_t>(img) * 6;
    const int64_t img0 = static_cast<int64_t>(img) * H * W * C;
    if (any_ring) focus_region(d.image2 + img0, H, W, C, y0, x0, true, 1, thr, s_y, s_r, s_ha, s_hb, s_a, s_b, out);
    if (any_inside)
        focus_region(d.image1 + img0, H, W, C, y0, x0, !(any_ring && d.image1 == d.image2), 2, thr, s_y, s_r, s_ha, s_hb, s_a, s_b,
                     out + 3);
}

// ---- fit --------------------------------------------------------------------------------------------------------------------------------
// c[k][i] = C(2 k, k + i), i = 0 .. k, k = 0 .. 33: C(66, 33) = 7219428434016265740 < 2^63
struct BinomTable {
    unsigned long long c[kTapR + 1][kTapR + 1];
};
constexpr BinomTable make_binom() {
    BinomTable t = {};
    unsigned long long row[2 * kTapR + 2] = {};
    row[0] = 1;
    t.c[0][0] = 1;
    for (int n = 1; n <= 2 * kTapR; ++n) {
        for (int j = n; j >= 1; --j) row[j] += row[j - 1];
        if (n % 2 == 0)
            for (int i = 0; i <= n / 2; ++i) t.c[n / 2][i] = row[n / 2 + i];
    }
    return t;
}
__device__ const BinomTable kBinom = make_binom();

__device__ __forceinline__ double focus_variance(unsigned long long n, unsigned long long sa, unsigned long long sb) {
#pragma clang fp contract(off)
    if (n < LP_FOCUS_MIN_COUNT) return LP_FOCUS_NO_FIT;
    const double a = static_cast<double>(sa) / 256.0;
    const double b = static_cast<double>(sb) / 65536.0;
    const double r = a / b;
    const double q = r * r;
    if (!(q > 1.0)) return static_cast<double>(LP_FOCUS_MAX_VAR);
    const double num = 2.0 - 0.5 * q;
    const double den = q - 1.0;
    return num / den;
}

// b_k(i) in fp64: the coefficient rounded to nearest even, times 4^-k exactly
__device__ __forceinline__ double binom_weight(int k, int j) {
    if (j > k) return 0.0;
    return static_cast<double>(kBinom.c[k][j]) * __longlong_as_double(static_cast<long long>(1023 - 2 * k) << 52);
}

__global__ __launch_bounds__(256) void lp_focus_fit_kernel(int batch, int strength16, int per_frame, const FocusWs ws) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_tot[6];
    const int tid = threadIdx.x;
    if (!per_frame) {
        if (tid < 6) s_tot[tid] = 0ull;
        __syncthreads();
        unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
        for (int b = tid; b < batch; b += 256) {
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[k] += ws.stats[static_cast<int64_t>(b) * 6 + k];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (acc[k]) atomicAdd(&s_tot[k], acc[k]);
        __syncthreads();
    }
    for (int b = tid; b < batch; b += 256) {
        unsigned long long s[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] = per_frame ? ws.stats[static_cast<int64_t>(b) * 6 + k] : s_tot[k];
        const unsigned long long n0 = s[0], n1 = s[3];
        const double var_ring = focus_variance(n0, s[1], s[2]), var_inside = focus_variance(n1, s[4], s[5]);
        int K = 0;
        if (n0 >= LP_FOCUS_MIN_COUNT && n1 >= LP_FOCUS_MIN_COUNT) {
            double dv = var_ring - var_inside;
            dv = dv > 0.0 ? dv : 0.0;
            double v = (static_cast<double>(strength16) / 16.0) * dv;
            v = v < static_cast<double>(LP_FOCUS_MAX_VAR) ? v : static_cast<double>(LP_FOCUS_MAX_VAR);
            const double scaled = v * 32.0;
            K = static_cast<int>(scaled + 0.5);
        }
        ws.var[static_cast<int64_t>(b) * 2] = var_ring;
        ws.var[static_cast<int64_t>(b) * 2 + 1] = var_inside;
        ws.K[b] = K;
        const int k = K >> 4, t = K & 15;
        float* w = ws.taps + static_cast<int64_t>(b) * LP_FOCUS_TAPS;
        for (int i = -kTapR; i <= kTapR; ++i) {
            const int j = i < 0 ? -i : i;
            float tap = 0.0f;
            if (j <= k + 1) {
                const double lo = static_cast<double>(16 - t) * binom_weight(k, j);
                const double hi = static_cast<double>(t) * binom_weight(k + 1, j);
                const double sum = lo + hi;
                tap = static_cast<float>(sum / 16.0);
            }
            w[kTapR + i] = tap;
        }
    }
}

// ---- blur -------------------------------------------------------------------------------------------------------------------------------
// AXIS 0: image1 along x into the plane.  AXIS 1: the plane along y, the mix with image1, out.
template <int AXIS>
__global__ __launch_bounds__(256) void lp_focus_blur_kernel(const lp_multiband_desc d, const FocusWs ws) {
    __shared__ float s_w[LP_FOCUS_TAPS];
    const int tid = threadIdx.x, H = d.height, W = d.width, C = d.channels, img = blockIdx.z;
    const int th = gridDim.y, tw = gridDim.x, ty = blockIdx.y, tx = blockIdx.x, y0 = ty * kT, x0 = tx * kT;
    const int mi = d.mask_batch == 1 ? 0 : img;
    const int K = ws.K[img];
    const int nr = min(kT, H - y0), nc = min(kT, W - x0), row_el = nc * C;
    const int64_t img0 = static_cast<int64_t>(img) * H * W;
    bool work = false;                                               // block-uniform: every lane reads the same words
    if (K > 0) {
        if (AXIS == 0) {
            for (int dy = -2; dy <= 2; ++dy) work = work || (tile_flag(ws.flags, mi, th, tw, ty + dy, tx) & 2);      // 33 pixels: two tiles
        } else {
            work = tile_flag(ws.flags, mi, th, tw, ty, tx) & 2;
        }
    }
    if (!work) {
        if (AXIS == 1)
            for (int it = tid; it < nr * row_el; it += 256) {
                const int i = it / row_el, e = it - i * row_el;
                const int64_t at = (img0 + static_cast<int64_t>(y0 + i) * W + x0) * C + e;
                d.out[at] = d.image1[at];
            }
        return;
    }
    if (tid < LP_FOCUS_TAPS) s_w[tid] = ws.taps[static_cast<int64_t>(img) * LP_FOCUS_TAPS + tid];
    __syncthreads();
    const int r = (K >> 4) + ((K & 15) ? 1 : 0);
    const float* plane = ws.plane + img0 * C;
    const float* a1 = d.image1 + img0 * C;
    for (int it = tid; it < nr * row_el; it += 256) {
        const int i = it / row_el, e = it - i * row_el, j = e / C, c = e - j * C, y = y0 + i, x = x0 + j;
        const int64_t at = (static_cast<int64_t>(y) * W + x) * C + c;
        if (AXIS == 0) {
            const float* q = a1 + static_cast<int64_t>(y) * W * C + c;
            float s = __fmul_rn(s_w[kTapR - r], q[static_cast<int64_t>(clampi(x - r, 0, W - 1)) * C]);
            for (int k = -r + 1; k <= r; ++k) s = __fadd_rn(s, __fmul_rn(s_w[kTapR + k], q[static_cast<int64_t>(clampi(x + k, 0, W - 1)) * C]));
            ws.plane[img0 * C + at] = s;
        } else {
            const float a = a1[at];
            const float m = focus_weight(d.mask[static_cast<int64_t>(mi) * H * W + static_cast<int64_t>(y) * W + x]);
            float o = a;
            if (m != 0.0f) {
                const float* q = plane + static_cast<int64_t>(x) * C + c;
                float s = __fmul_rn(s_w[kTapR - r], q[static_cast<int64_t>(clampi(y - r, 0, H - 1)) * W * C]);
                for (int k = -r + 1; k <= r; ++k)
                    s = __fadd_rn(s, __fmul_rn(s_w[kTapR + k], q[static_cast<int64_t>(clampi(y + k, 0, H - 1)) * W * C]));
                o = __fadd_rn(a, __fmul_rn(m, __fsub_rn(s, a)));
            }
            d.out[img0 * C + at] = o;
        }
    }
}

}  // namespace

int focus_check(int32_t batch, int32_t height, int32_t width, int32_t levels) {
    const FocusWord f = focus_word(levels);
    if (!f.ok) return LP_E_INVALID;
    if (batch > 65535) return LP_E_UNSUPPORTED;
    if (!f.per_frame && static_cast<int64_t>(batch) * height * width > (1ll << 30)) return LP_E_UNSUPPORTED;
    return LP_OK;
}

bool focus_word_ok(int32_t levels) { return focus_word(levels).ok; }

int focus_enqueue(const lp_multiband_desc& d, hipStream_t stream) {
    const FocusWord f = focus_word(d.levels);
    const FocusWs ws = focus_ws(d);
    const int tw = (d.width + kT - 1) / kT, th = (d.height + kT - 1) / kT;
    hipLaunchKernelGGL(lp_focus_flags_kernel, dim3(tw, th, d.mask_batch), dim3(256), 0, stream, d, ws);
    if (launched() != LP_OK) return LP_E_LAUNCH;
    const dim3 grid(tw, th, d.batch);
    hipLaunchKernelGGL(lp_focus_stats_kernel, grid, dim3(256), 0, stream, d, ws, f.edge, f.ring);
    if (launched() != LP_OK) return LP_E_LAUNCH;
    hipLaunchKernelGGL(lp_focus_fit_kernel, dim3(1), dim3(256), 0, stream, d.batch, f.strength16, f.per_frame, ws);
    if (launched() != LP_OK) return LP_E_LAUNCH;
    hipLaunchKernelGGL(lp_focus_blur_kernel<0>, grid, dim3(256), 0, stream, d, ws);
    if (launched() != LP_OK) return LP_E_LAUNCH;
    hipLaunchKernelGGL(lp_focus_blur_kernel<1>, grid, dim3(256), 0, stream, d, ws);
    return launched();
}

}  // namespace lp
