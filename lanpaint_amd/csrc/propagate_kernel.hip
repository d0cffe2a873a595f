// propagate_kernel.hip -- video mask propagate for gfx950 (lanpaint_amd/propagate.py): a mask painted on one frame follows the
// picture's motion.  include/lanpaint_hip.h (lp_prop_*) states the rule, all of it integer arithmetic.
//
//   luma, down   one lane per pixel: the 8-bit luma of every frame into level 0 of its pyramid, then one launch per further level.
//   key_mask     a block per 32 x 32 tile: binarises the key mask and writes every level of its bits' pyramid (OR over the 2^l
//                footprint) from LDS.  advance ends in the same tile code, so a step needs no launch of its own for the pyramid.
//   match        the hot path.  One wave per 8 x 8 block of the level's grid.  The 16 x 16 source window goes to LDS as 64 dwords
//                of four pixels, already ANDed with its per-byte mask (0xFF on a mask pixel inside the image, else 0); the mask
//                dwords go next to it; the (16 + 2R)^2 target patch, read with clamped coordinates around the predictor, goes to
//                rows of 32 bytes.  Lane c takes candidates c, c + 64, ...: per window row and dword, v_alignbyte_b32 cuts the
//                four target pixels out of two patch dwords, the AND with the mask drops what is not mask, v_sad_u8 adds the four
//                absolute differences.  The candidate's S stays in LDS for the sub-pixel step, the 32-bit key is reduced across
//                the wave with a butterfly of minima.  A block whose window holds fewer than 16 mask pixels leaves after staging.
//   fill         a block per 16 x 16 tile of the grid with a halo of 4 in LDS: three Jacobi passes between two buffers (a pass
//                is wrong on the outermost ring it still reads, so three passes leave the tile and one ring around it exact),
//                then the 3 x 3 median (the 19-exchange network) per component.
//   advance      a block per 32 x 32 tile, four pixels per lane: the per-pixel vector from the block field, the new position
//                map, the mask code through it, the output, and the bits' pyramid for the next step.
//   batches      match, fill and advance take up to LP_PROP_MAX_JOBS independent chain steps in one launch, the job on blockIdx.z.
//                The job table (the jobs' pointers) travels by value in the kernel's arguments and is read with scalar loads;
//                nothing is uploaded.  The single entries are one-job batches: every stage has one device body and one dispatch.
//   visible      the occlusion-aware form's hot path.  A block per 32 x 32 tile: d = Yt - K (K the key frame's luma sampled through
//                P_t) of the tile and its halo of 4 goes to LDS once as int16, a marker where the pixel is outside the image or the
//                mask, four pixels per lane, P_t read as two 16-byte vectors; then 16 lanes per window of the tile's 4 x 4 blocks,
//                a row each (two ds_read_b128 on an 80-byte pitch), D and n and then R summed across them with shuffles.
//   occlude      a block per 32 x 32 tile, four pixels per lane: the flags interpolated as advance interpolates the field, the
//                visible and the hidden part of the advance's code, and the visible bits' pyramid from the same tile code.  With a
//                count pointer, the number of visible bits goes into it: a sum per wave, one integer atomic add per wave.
//                visible and occlude are batches like match, fill and advance; a job's vector path is a bit of a mask.
//   anchor match the anchored form's hot path: the warp of the key luma and its match against the frame in one launch.  A block per
//                32 x 32 tile: K of the tile and its halo of 4 goes to LDS once, four pixels a dword, ANDed with its per-byte mask
//                as match has it, P_t read as two 16-byte vectors; the (40 + 2R)^2 clamped target patch goes to rows of 56 bytes.  A
//                wave takes four of the tile's 4 x 4 windows in turn, the candidates over its lanes in up to four passes, match's
//                v_alignbyte_b32 / v_sad_u8 inner loop, key and sub-pixel step.  A tile with no mask pixel leaves after staging K.
//                The anchored occlusion-aware form's launch is the same kernel with a compile-time tail on the window loop: behind
//                the minimum a lane per dword of the window takes visible's D, mu and R at the winner's alignment from the same LDS.
//                Four ways in, one body: the two single entries, and lp_prop_match_batch's warped-key and gated forms.
//   merge        one lane per pixel and frame of a gap between two keys: the two chains' signed squared distances, their capped
//                fp64 roots, the weighted mean in a fixed order, the ramp of half-width 1/2 around the zero crossing.
//   merge_visible the merge of a gap whose chains are occlusion-aware: a streaming kernel over [frames, H, W], four pixels per lane
//                as 16-byte vectors when the width allows.  Per frame the two chains' lost bits come from their visible-bit
//                counts (a uniform loop over scalar loads).  Exactly one lost: the other chain's planes pass through.  Else the
//                merge of the subject codes' distances, rounded to a code and split by the nearer key's flags as occlude does.
// No scratch, no floating point beyond the luma codes, the final c / 256 (read back by occlude) and the merges.  The only atomics
// are occlude's integer adds into a count: any order gives the same bits.
// Entry points defined here: the seventeen lp_prop_* (lp_prop_pyramid_ws_bytes, _luma, _key_mask; _match, _fill, _advance, _visible and
// _occlude, each beside its _batch form, which it calls with a batch of one job; _anchor_match, _anchor_match_gated; _merge,
// _merge_visible).
#include "motion_tile.h"

#include <math.h>

#include <algorithm>

namespace lp {
namespace {

constexpr int kB = LP_PROP_BLOCK, kHalo = LP_PROP_HALO, kWin = kB + 2 * kHalo;        // 8, 4, 16
constexpr int kPatchPitch = 8;                                                         // dwords per patch row: 32 bytes >= 30
constexpr int kPatchRows = kWin + 2 * LP_PROP_MAX_SEARCH;                              // 30
constexpr int kMaxCand = (2 * LP_PROP_MAX_SEARCH + 1) * (2 * LP_PROP_MAX_SEARCH + 1);  // 225
constexpr int kTile = 32;                                                              // key_mask / advance: pixels per tile side
constexpr int kFillTile = 16, kFillHalo = LP_PROP_FILL_ITERS + 1, kFillSide = kFillTile + 2 * kFillHalo;   // 16, 4, 24

static_assert(kWin == 16 && kPatchRows <= 32 && kWin + 2 * LP_PROP_MAX_SEARCH <= 4 * kPatchPitch, "the match kernel's LDS layout");
static_assert(kTile == 1 << (LP_PROP_MAX_LEVELS - 1), "a tile holds one pixel of the coarsest level");

// ---- luma and pyramids ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lp_prop_luma_kernel(const float* __restrict__ image, uint8_t* __restrict__ pyr, int64_t plane,
                                                           int channels, int64_t stride) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= plane) return;
    const int64_t f = blockIdx.y;
    pyr[f * stride + p] = static_cast<uint8_t>(luma_of(image + (f * plane + p) * channels, channels));
}

__global__ __launch_bounds__(256) void lp_prop_down_kernel(uint8_t* __restrict__ pyr, int64_t stride, int64_t src_off, int64_t dst_off,
                                                           int sh, int sw, int dh, int dw) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= static_cast<int64_t>(dh) * dw) return;
    const int y = static_cast<int>(p / dw), x = static_cast<int>(p - static_cast<int64_t>(y) * dw);
    const uint8_t* src = pyr + static_cast<int64_t>(blockIdx.y) * stride + src_off;
    const int y0 = 2 * y, y1 = min(2 * y + 1, sh - 1), x0 = 2 * x, x1 = min(2 * x + 1, sw - 1);        // 2y <= sh - 1 always
    const uint32_t s = src[static_cast<int64_t>(y0) * sw + x0] + src[static_cast<int64_t>(y0) * sw + x1] +
                       src[static_cast<int64_t>(y1) * sw + x0] + src[static_cast<int64_t>(y1) * sw + x1];
    pyr[static_cast<int64_t>(blockIdx.y) * stride + dst_off + p] = static_cast<uint8_t>((s + 2u) >> 2);
}

// Every level of the bits' pyramid of one 32 x 32 tile.  s0 holds the tile's level-0 bits (0 outside the image) and is complete
// (the caller has synchronised); tile (ty, tx) of a height x width plane.  256 lanes.
__device__ __forceinline__ void tile_mask_pyramid(uint8_t* s0, uint8_t* s1, int ty, int tx, int height, int width, int levels,
                                                  uint8_t* __restrict__ out) {
    const int tid = threadIdx.x;
    uint8_t* cur = s0;
    uint8_t* nxt = s1;
    int64_t off = 0;
    for (int l = 0; l < levels; ++l) {
        const int side = kTile >> l, h = level_side(height, l), w = level_side(width, l);
        const int oy = (ty * kTile) >> l, ox = (tx * kTile) >> l;
        for (int i = tid; i < side * side; i += 256) {
            const int y = i / side, x = i - y * side;
            if (oy + y < h && ox + x < w) out[off + static_cast<int64_t>(oy + y) * w + ox + x] = cur[i];
        }
        if (l + 1 == levels) break;
        const int half = side >> 1;
        for (int i = tid; i < half * half; i += 256) {
            const int y = i / half, x = i - y * half;
            const uint8_t* r = cur + (2 * y) * side + 2 * x;
            nxt[i] = r[0] | r[1] | r[side] | r[side + 1];
        }
        __syncthreads();
        uint8_t* t = cur; cur = nxt; nxt = t;
        off += (static_cast<int64_t>(h) * w + LP_PROP_ALIGN - 1) / LP_PROP_ALIGN * LP_PROP_ALIGN;
    }
}

__global__ __launch_bounds__(256) void lp_prop_key_mask_kernel(const float* __restrict__ mask, int height, int width, int levels,
                                                               uint8_t* __restrict__ mpyr, float* __restrict__ out) {
    __shared__ uint8_t s0[kTile * kTile], s1[kTile * kTile / 4];
    for (int i = threadIdx.x; i < kTile * kTile; i += 256) {
        const int y = blockIdx.y * kTile + (i >> 5), x = blockIdx.x * kTile + (i & 31);
        uint8_t bit = 0;
        if (y < height && x < width) {
            const int64_t p = static_cast<int64_t>(y) * width + x;
            bit = mask[p] >= 0.5f ? 1 : 0;                                               // a NaN gives 0
            if (out) out[p] = bit ? 1.0f : 0.0f;
        }
        s0[i] = bit;
    }
    __syncthreads();
    tile_mask_pyramid(s0, s1, blockIdx.y, blockIdx.x, height, width, levels, mpyr);
}

// ---- the masked block matching ---------------------------------------------------------------------------------------------------------
struct match_job {
    const uint8_t* src;          // this level's planes
    const uint8_t* tgt;
    const uint8_t* msk;
    const int32_t* parent;       // [pgh, pgw, 2] or null
    int32_t*       vec;
    int32_t*       valid;
};

struct match_args {
    int32_t h, w, gw, pgh, pgw, search, smooth, subpel;
    match_job job[LP_PROP_MAX_JOBS];                                 // blockIdx.z picks one: a uniform index, scalar loads
};

__global__ __launch_bounds__(kWave) void lp_prop_match_kernel(const match_args a) {
    __shared__ uint32_t s_src[kWin * 4], s_bm[kWin * 4], s_pat[kPatchRows * kPatchPitch];
    __shared__ int32_t s_S[kMaxCand];
    const match_job jb = a.job[blockIdx.z];
    const int lane = threadIdx.x, bx = blockIdx.x, by = blockIdx.y;
    const int R = a.search, n = 2 * R + 1, ncand = n * n;
    int py = 0, px = 0;
    if (jb.parent) {
        const int32_t* pv = jb.parent + (static_cast<int64_t>(min(by >> 1, a.pgh - 1)) * a.pgw + min(bx >> 1, a.pgw - 1)) * 2;
        py = 2 * ((pv[0] + 8) >> 4);
        px = 2 * ((pv[1] + 8) >> 4);
    }
    const int64_t cell = static_cast<int64_t>(by) * a.gw + bx;
    // the window: lane = row * 4 + dword
    const int wy = by * kB - kHalo, wx = bx * kB - kHalo;
    int count = 0;
    {
        const int y = wy + (lane >> 2);
        uint32_t sv = 0, bm = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = wx + (lane & 3) * 4 + k;
            if (y >= 0 && y < a.h && x >= 0 && x < a.w) {
                const int64_t p = static_cast<int64_t>(y) * a.w + x;
                if (jb.msk[p]) {
                    bm |= 0xFFu << (8 * k);
                    sv |= static_cast<uint32_t>(jb.src[p]) << (8 * k);
                    ++count;
                }
            }
        }
        s_src[lane] = sv;
        s_bm[lane] = bm;
    }
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) count += __shfl_xor(count, d, kWave);
    if (count < LP_PROP_MIN_PIXELS) {                                    // the whole wave leaves together
        if (lane == 0) {
            jb.vec[cell * 2] = 16 * py;
            jb.vec[cell * 2 + 1] = 16 * px;
            jb.valid[cell] = 0;
        }
        return;
    }
    // the target patch: row j, byte i is Yt(clamp(wy + py - R + j), clamp(wx + px - R + i))
    const int rows = kWin + 2 * R;
    for (int i = lane; i < rows * kPatchPitch; i += kWave) {
        const int j = i >> 3, c0 = (i & 7) * 4;
        const uint8_t* row = jb.tgt + static_cast<int64_t>(clampi(wy + py - R + j, 0, a.h - 1)) * a.w;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= static_cast<uint32_t>(row[clampi(wx + px - R + c0 + k, 0, a.w - 1)]) << (8 * k);
        s_pat[i] = v;
    }
    __syncthreads();
    uint32_t best = 0xFFFFFFFFu;
    for (int c = lane; c < ncand; c += kWave) {
        const int cy = c / n, cx = c - cy * n;                          // oy + R, ox + R
        const int word = cx >> 2, shift = cx & 3;                       // word + 3 + 1 <= 7: inside the patch row
        uint32_t S = 0;
        for (int r = 0; r < kWin; ++r) {
            const uint32_t* pr = s_pat + (r + cy) * kPatchPitch + word;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t t = __builtin_amdgcn_alignbyte(pr[k + 1], pr[k], shift) & s_bm[r * 4 + k];
                S = __builtin_amdgcn_sad_u8(s_src[r * 4 + k], t, S);
            }
        }
        s_S[c] = static_cast<int32_t>(S);
        const uint32_t dist = static_cast<uint32_t>(abs(cy - R) + abs(cx - R));
        best = min(best, ((S + static_cast<uint32_t>(a.smooth) * dist) << 12) | (dist << 8) | static_cast<uint32_t>(c));
    }
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) best = min(best, static_cast<uint32_t>(__shfl_xor(static_cast<int>(best), d, kWave)));
    __syncthreads();                                                     // s_S is complete
    if (lane == 0) {
        const int c = static_cast<int>(best & 255u), cy = c / n, cx = c - cy * n;
        int vy = 16 * (py + cy - R), vx = 16 * (px + cx - R);
        const int s0 = s_S[c];
        if (a.subpel && s0 != 0) {
            if (cy > 0 && cy < 2 * R) {
                const int cm = s_S[c - n], cp = s_S[c + n], d = cm + cp - 2 * s0, g = cm - cp;
                if (d > 0) vy += (g > 0 ? 1 : (g < 0 ? -1 : 0)) * min(abs(8 * g) / d, 8);
            }
            if (cx > 0 && cx < 2 * R) {
                const int cm = s_S[c - 1], cp = s_S[c + 1], d = cm + cp - 2 * s0, g = cm - cp;
                if (d > 0) vx += (g > 0 ? 1 : (g < 0 ? -1 : 0)) * min(abs(8 * g) / d, 8);
            }
        }
        jb.vec[cell * 2] = vy;
        jb.vec[cell * 2 + 1] = vx;
        jb.valid[cell] = 1;
    }
}

// ---- fill and median ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int median9(int p0, int p1, int p2, int p3, int p4, int p5, int p6, int p7, int p8) {
    cmpswap(p1, p2); cmpswap(p4, p5); cmpswap(p7, p8); cmpswap(p0, p1); cmpswap(p3, p4); cmpswap(p6, p7);
    cmpswap(p1, p2); cmpswap(p4, p5); cmpswap(p7, p8); cmpswap(p0, p3); cmpswap(p5, p8); cmpswap(p4, p7);
    cmpswap(p3, p6); cmpswap(p1, p4); cmpswap(p2, p5); cmpswap(p4, p7); cmpswap(p4, p2); cmpswap(p6, p4);
    cmpswap(p4, p2);
    return p4;
}

__device__ __forceinline__ int floor_div(int a, int b) {                 // b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

struct fill_job {
    const int32_t* vec;
    const int32_t* valid;
    int32_t*       out;
};

struct fill_args {
    int32_t gh, gw;
    fill_job job[LP_PROP_MAX_JOBS];
};

__global__ __launch_bounds__(256) void lp_prop_fill_kernel(const fill_args a) {
    constexpr int N = kFillSide * kFillSide;                             // 576
    const int gh = a.gh, gw = a.gw;
    const int32_t* __restrict__ vec = a.job[blockIdx.z].vec;
    const int32_t* __restrict__ valid = a.job[blockIdx.z].valid;
    int32_t* __restrict__ out = a.job[blockIdx.z].out;
    __shared__ int32_t s_y[2][N], s_x[2][N], s_ok[2][N];                 // ok: 1 valid, 0 invalid, -1 outside the grid
    const int y00 = blockIdx.y * kFillTile - kFillHalo, x00 = blockIdx.x * kFillTile - kFillHalo;
    for (int i = threadIdx.x; i < N; i += 256) {
        const int y = y00 + i / kFillSide, x = x00 + i % kFillSide;
        int vy = 0, vx = 0, ok = -1;
        if (y >= 0 && y < gh && x >= 0 && x < gw) {
            const int64_t c = static_cast<int64_t>(y) * gw + x;
            vy = vec[c * 2];
            vx = vec[c * 2 + 1];
            ok = valid[c] != 0;
        }
        s_y[0][i] = vy; s_x[0][i] = vx; s_ok[0][i] = ok;
    }
    __syncthreads();
    int cur = 0;
#pragma unroll 1
    for (int pass = 0; pass < LP_PROP_FILL_ITERS; ++pass) {
        for (int i = threadIdx.x; i < N; i += 256) {
            const int r = i / kFillSide, c = i % kFillSide;
            int vy = s_y[cur][i], vx = s_x[cur][i], ok = s_ok[cur][i];
            if (ok == 0) {
                int cnt = 0, sy = 0, sx = 0;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int rr = r + dy, cc = c + dx;
                        if (rr < 0 || rr >= kFillSide || cc < 0 || cc >= kFillSide) continue;
                        const int j = rr * kFillSide + cc;
                        if (s_ok[cur][j] == 1) { ++cnt; sy += s_y[cur][j]; sx += s_x[cur][j]; }
                    }
                if (cnt > 0) {
                    vy = floor_div(2 * sy + cnt, 2 * cnt);
                    vx = floor_div(2 * sx + cnt, 2 * cnt);
                    ok = 1;
                }
            }
            s_y[cur ^ 1][i] = vy; s_x[cur ^ 1][i] = vx; s_ok[cur ^ 1][i] = ok;
        }
        __syncthreads();
        cur ^= 1;
    }
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int y = blockIdx.y * kFillTile + ty, x = blockIdx.x * kFillTile + tx;
    if (y >= gh || x >= gw) return;
    int py[9], px[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = clampi(y + k / 3 - 1, 0, gh - 1) - y00, xx = clampi(x + k % 3 - 1, 0, gw - 1) - x00;
        py[k] = s_y[cur][yy * kFillSide + xx];
        px[k] = s_x[cur][yy * kFillSide + xx];
    }
    const int64_t c = static_cast<int64_t>(y) * gw + x;
    out[c * 2] = median9(py[0], py[1], py[2], py[3], py[4], py[5], py[6], py[7], py[8]);
    out[c * 2 + 1] = median9(px[0], px[1], px[2], px[3], px[4], px[5], px[6], px[7], px[8]);
}

// ---- advance -------------------------------------------------------------------------------------------------------------------------------
struct advance_job {
    const int32_t* vec;
    const int32_t* pos_src;
    const uint8_t* key;
    int32_t*       pos_dst;
    float*         out;
    uint8_t*       mpyr;
};

struct advance_args {
    int32_t height, width, levels, gh, gw;
    advance_job job[LP_PROP_MAX_JOBS];
};

struct bil_tap { int i0, i1, f; };

__device__ __forceinline__ bil_tap tap_of(int q, int n) {
    q = clampi(q, 0, 16 * (n - 1));
    bil_tap t;
    t.i0 = q >> 4;
    t.f = q & 15;
    t.i1 = min(t.i0 + 1, n - 1);
    return t;
}

__global__ __launch_bounds__(256) void lp_prop_advance_kernel(const advance_args a) {
    __shared__ uint8_t s0[kTile * kTile], s1[kTile * kTile / 4];
    const advance_job jb = a.job[blockIdx.z];
    const int H = a.height, W = a.width;
    for (int i = threadIdx.x; i < kTile * kTile; i += 256) {
        const int y = blockIdx.y * kTile + (i >> 5), x = blockIdx.x * kTile + (i & 31);
        uint8_t bit = 0;
        if (y < H && x < W) {
            // the per-pixel vector
            const field_tap by = field_tap_of(y, a.gh), bx = field_tap_of(x, a.gw);
            const int64_t r0 = static_cast<int64_t>(by.b0) * a.gw, r1 = static_cast<int64_t>(by.b1) * a.gw;
            const int32_t *v00 = jb.vec + (r0 + bx.b0) * 2, *v01 = jb.vec + (r0 + bx.b1) * 2, *v10 = jb.vec + (r1 + bx.b0) * 2, *v11 = jb.vec + (r1 + bx.b1) * 2;
            const int Vy = field_vector(v00[0], v01[0], v10[0], v11[0], by.f, bx.f);
            const int Vx = field_vector(v00[1], v01[1], v10[1], v11[1], by.f, bx.f);
            // the new position
            const bil_tap ty = tap_of(16 * y - Vy, H), tx = tap_of(16 * x - Vx, W);
            int Py, Px;
            if (jb.pos_src) {
                const int32_t *p00 = jb.pos_src + (static_cast<int64_t>(ty.i0) * W + tx.i0) * 2, *p01 = jb.pos_src + (static_cast<int64_t>(ty.i0) * W + tx.i1) * 2;
                const int32_t *p10 = jb.pos_src + (static_cast<int64_t>(ty.i1) * W + tx.i0) * 2, *p11 = jb.pos_src + (static_cast<int64_t>(ty.i1) * W + tx.i1) * 2;
                Py = (bil_sum(p00[0], p01[0], p10[0], p11[0], ty.f, tx.f) + 128) >> 8;
                Px = (bil_sum(p00[1], p01[1], p10[1], p11[1], ty.f, tx.f) + 128) >> 8;
            } else {                                                     // P_key(y, x) = (16 y, 16 x)
                Py = (bil_sum(16 * ty.i0, 16 * ty.i0, 16 * ty.i1, 16 * ty.i1, ty.f, tx.f) + 128) >> 8;
                Px = (bil_sum(16 * tx.i0, 16 * tx.i1, 16 * tx.i0, 16 * tx.i1, ty.f, tx.f) + 128) >> 8;
            }
            const int64_t p = static_cast<int64_t>(y) * W + x;
            jb.pos_dst[p * 2] = Py;
            jb.pos_dst[p * 2 + 1] = Px;
            // the mask code through it
            const bil_tap ky = tap_of(Py, H), kx = tap_of(Px, W);
            const uint8_t *k0 = jb.key + static_cast<int64_t>(ky.i0) * W, *k1 = jb.key + static_cast<int64_t>(ky.i1) * W;
            const int c = bil_sum(k0[kx.i0], k0[kx.i1], k1[kx.i0], k1[kx.i1], ky.f, kx.f);
            jb.out[p] = static_cast<float>(c) * (1.0f / 256.0f);           // c <= 256 and a power of two: exact
            bit = c >= 128 ? 1 : 0;
        }
        s0[i] = bit;
    }
    __syncthreads();
    tile_mask_pyramid(s0, s1, blockIdx.y, blockIdx.x, H, W, a.levels, jb.mpyr);
}

// ---- visible and occlude: the occlusion-aware form ------------------------------------------------------------------------------------
constexpr int kVisSide = kTile + 2 * kHalo;                             // 40: a tile and its halo
constexpr int kVisQuads = kVisSide / 4;                                 // 10 quads of four pixels per row
constexpr int16_t kVisNone = INT16_MIN;                                 // a pixel outside the image or the mask; |d| <= 255

static_assert(kVisSide % 8 == 0 && kTile / kB == 4 && kWin == 16, "the visible kernel's window rows: 16 int16, 16-byte aligned");

// The warped key luma of one pixel: K = (bil(Yk, P_t) + 128) >> 8, in 0..255
__device__ __forceinline__ int warped_key_of(const uint8_t* __restrict__ key, int H, int W, int Py, int Px) {
    const bil_tap ky = tap_of(Py, H), kx = tap_of(Px, W);
    const uint8_t *k0 = key + static_cast<int64_t>(ky.i0) * W, *k1 = key + static_cast<int64_t>(ky.i1) * W;
    return (bil_sum(k0[kx.i0], k0[kx.i1], k1[kx.i0], k1[kx.i1], ky.f, kx.f) + 128) >> 8;
}

// d = Yt - K for one mask pixel inside the image
__device__ __forceinline__ int16_t residual_of(const uint8_t* __restrict__ key, int H, int W, int Py, int Px, int yt) {
    return static_cast<int16_t>(yt - warped_key_of(key, H, W, Py, Px));
}

struct visible_job {
    const int32_t* pos;
    const uint8_t* tgt;
    const uint8_t* key;
    const uint8_t* msk;
    int32_t*       flags;
};

struct visible_args {
    int32_t  H, W, gh, gw, occlusion;
    uint32_t wide;                                                   // bit i: job i takes the vector path
    visible_job job[LP_PROP_MAX_JOBS];
};

__global__ __launch_bounds__(256) void lp_prop_visible_kernel(const visible_args a) {
    const int32_t* __restrict__ pos = a.job[blockIdx.z].pos;
    const uint8_t* __restrict__ tgt = a.job[blockIdx.z].tgt;
    const uint8_t* __restrict__ key = a.job[blockIdx.z].key;
    const uint8_t* __restrict__ msk = a.job[blockIdx.z].msk;
    int32_t* __restrict__ flags = a.job[blockIdx.z].flags;
    const int H = a.H, W = a.W, gh = a.gh, gw = a.gw, occlusion = a.occlusion;
    const int wide = static_cast<int>((a.wide >> blockIdx.z) & 1u);
    __shared__ __attribute__((aligned(16))) int16_t s_d[kVisSide * kVisSide];      // 3200 bytes; a row is 80 bytes = 5 x 16
    const int y00 = blockIdx.y * kTile - kHalo, x00 = blockIdx.x * kTile - kHalo;     // x00 is a multiple of 4
    // wide: width % 4 == 0 and the planes 16-byte aligned, so a quad is inside its row or outside it, and one vector
    for (int i = threadIdx.x; i < kVisSide * kVisQuads; i += 256) {
        const int r = i / kVisQuads, q = i - r * kVisQuads;
        const int y = y00 + r, x = x00 + 4 * q;
        int16_t d[4] = {kVisNone, kVisNone, kVisNone, kVisNone};
        if (y >= 0 && y < H && x + 3 >= 0 && x < W) {
            const int64_t p = static_cast<int64_t>(y) * W + x;
            if (wide) {                                                  // x >= 0 and x + 3 < W; p is a multiple of 4
                const uchar4 m4 = *reinterpret_cast<const uchar4*>(msk + p);
                if (m4.x | m4.y | m4.z | m4.w) {
                    const uchar4 t4 = *reinterpret_cast<const uchar4*>(tgt + p);
                    const int4 pa = *reinterpret_cast<const int4*>(pos + p * 2), pb = *reinterpret_cast<const int4*>(pos + p * 2 + 4);
                    if (m4.x) d[0] = residual_of(key, H, W, pa.x, pa.y, t4.x);
                    if (m4.y) d[1] = residual_of(key, H, W, pa.z, pa.w, t4.y);
                    if (m4.z) d[2] = residual_of(key, H, W, pb.x, pb.y, t4.z);
                    if (m4.w) d[3] = residual_of(key, H, W, pb.z, pb.w, t4.w);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + k >= 0 && x + k < W && msk[p + k]) d[k] = residual_of(key, H, W, pos[(p + k) * 2], pos[(p + k) * 2 + 1], tgt[p + k]);
            }
        }
        *reinterpret_cast<short4*>(s_d + r * kVisSide + 4 * q) = make_short4(d[0], d[1], d[2], d[3]);
    }
    __syncthreads();
    // 16 lanes per window, a row each: block (wy, wx) of the tile's 4 x 4, window row `row`
    const int win = threadIdx.x >> 4, row = threadIdx.x & 15, wy = win >> 2, wx = win & 3;
    const int16_t* src = s_d + (wy * kB + row) * kVisSide + wx * kB;     // 16 int16, 16-byte aligned
    const int4 lo = *reinterpret_cast<const int4*>(src), hi = *reinterpret_cast<const int4*>(src + 8);
    const int packed[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    int v[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        v[2 * k] = static_cast<int16_t>(packed[k] & 0xFFFF);
        v[2 * k + 1] = packed[k] >> 16;                                  // arithmetic: the sign comes along
    }
    int D = 0, n = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool in = v[k] != kVisNone;
        D += in ? v[k] : 0;
        n += in ? 1 : 0;
    }
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) {                                   // the 16 lanes of a window are one aligned group of a wave
        D += __shfl_xor(D, s, kWave);
        n += __shfl_xor(n, s, kWave);
    }
    const int mu = n > 0 ? clampi(floor_div(2 * D + n, 2 * n), -LP_PROP_VIS_MAX_BIAS, LP_PROP_VIS_MAX_BIAS) : 0;
    int R = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) R += v[k] != kVisNone ? abs(v[k] - mu) : 0;
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) R += __shfl_xor(R, s, kWave);
    const int by = blockIdx.y * (kTile / kB) + wy, bx = blockIdx.x * (kTile / kB) + wx;
    if (row == 0 && by < gh && bx < gw)
        flags[static_cast<int64_t>(by) * gw + bx] = (n >= LP_PROP_MIN_PIXELS && R > occlusion * n) ? 1 : 0;
}

// w of one pixel: v = 1 - flag between the block centres, the advance's weights, unrounded (0..256)
__device__ __forceinline__ int weight_of(const int32_t* __restrict__ flags, int gh, int gw, int y, int x) {
    const field_tap by = field_tap_of(y, gh), bx = field_tap_of(x, gw);
    const int64_t r0 = static_cast<int64_t>(by.b0) * gw, r1 = static_cast<int64_t>(by.b1) * gw;
    return bil_sum(flags[r0 + bx.b0] == 0, flags[r0 + bx.b1] == 0, flags[r1 + bx.b0] == 0, flags[r1 + bx.b1] == 0, by.f, bx.f);
}

struct occlude_job {
    const float*   code;
    const int32_t* flags;
    float*         out;
    float*         hidden;
    uint8_t*       mpyr;
    int32_t*       count;        // or null
};

struct occlude_args {
    int32_t  H, W, levels, gh, gw;
    uint32_t wide;
    occlude_job job[LP_PROP_MAX_JOBS];
};

__global__ __launch_bounds__(256) void lp_prop_occlude_kernel(const occlude_args a) {
    const float* __restrict__ code = a.job[blockIdx.z].code;
    const int32_t* __restrict__ flags = a.job[blockIdx.z].flags;
    float* __restrict__ out = a.job[blockIdx.z].out;
    float* __restrict__ hidden = a.job[blockIdx.z].hidden;
    uint8_t* __restrict__ mpyr = a.job[blockIdx.z].mpyr;
    int32_t* count = a.job[blockIdx.z].count;
    const int H = a.H, W = a.W, levels = a.levels, gh = a.gh, gw = a.gw;
    const int wide = static_cast<int>((a.wide >> blockIdx.z) & 1u);
    __shared__ uint8_t s0[kTile * kTile], s1[kTile * kTile / 4];
    const int r = threadIdx.x >> 3, q = threadIdx.x & 7;                  // four pixels per lane: row r, columns 4 q .. 4 q + 3
    const int y = blockIdx.y * kTile + r, x = blockIdx.x * kTile + 4 * q;
    float c4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m4[4], h4[4];
    const bool row_in = y < H && x < W;                                  // wide (as in the visible kernel): x + 3 < W too
    const int64_t p = static_cast<int64_t>(y) * W + x;
    if (row_in) {
        if (wide) {
            *reinterpret_cast<float4*>(c4) = *reinterpret_cast<const float4*>(code + p);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < W) c4[k] = code[p + k];
        }
    }
    uint8_t bits[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        m4[k] = h4[k] = 0.0f;
        if (row_in && x + k < W) {
            const int c = clampi(static_cast<int>(c4[k] * 256.0f), 0, 256);
            const int cv = (c * weight_of(flags, gh, gw, y, x + k) + 128) >> 8;
            m4[k] = static_cast<float>(cv) * (1.0f / 256.0f);               // exact, as the advance's
            h4[k] = static_cast<float>(c - cv) * (1.0f / 256.0f);
            bits[k] = cv >= 128 ? 1 : 0;
        }
    }
    if (row_in) {
        if (wide) {
            *reinterpret_cast<float4*>(out + p) = *reinterpret_cast<const float4*>(m4);
            *reinterpret_cast<float4*>(hidden + p) = *reinterpret_cast<const float4*>(h4);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < W) { out[p + k] = m4[k]; hidden[p + k] = h4[k]; }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s0[r * kTile + 4 * q + k] = bits[k];
    if (count) {                                                         // the job's: the whole block takes the branch
        int n = bits[0] + bits[1] + bits[2] + bits[3];
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) n += __shfl_xor(n, d, kWave);
        if ((threadIdx.x & (kWave - 1)) == 0 && n != 0) atomicAdd(count, n);
    }
    __syncthreads();
    tile_mask_pyramid(s0, s1, blockIdx.y, blockIdx.x, H, W, levels, mpyr);
}

// ---- anchor match: the anchored form ---------------------------------------------------------------------------------------------------
constexpr int kAncPitch = kVisQuads;                                    // dwords per row of K and of its mask: 40 bytes
constexpr int kAncPatRows = kVisSide + 2 * LP_PROP_MAX_SEARCH;          // 54
constexpr int kAncPatPitch = 14;                                        // dwords per patch row: 56 bytes >= 54

static_assert(4 * kAncPatPitch >= kAncPatRows, "a patch row holds the tile, its halo and the search range");
static_assert((kTile - kB + 2 * LP_PROP_MAX_SEARCH) / 4 + 4 < kAncPatPitch, "a window row's four dwords and the one behind them lie inside a patch row");
static_assert(kWin * 4 == kWave, "a lane per dword of a window's mask");

struct anchor_job {
    const int32_t* pos;
    const uint8_t* tgt;
    const uint8_t* key;
    const uint8_t* msk;
    int32_t*       vec;
    int32_t*       valid;
    int32_t*       gated;                                            // the gated form's third output, else null
};

struct anchor_args {
    int32_t  H, W, gh, gw, search, smooth, occlusion;
    uint32_t wide;                                                   // bit i: job i takes the vector path
    anchor_job job[LP_PROP_MAX_JOBS];
};

static_assert(sizeof(anchor_args) <= 4096, "the job table travels by value in the kernel's arguments");

// Gated: the anchored occlusion-aware form.  Behind the wave-wide minimum every lane knows the winner; lane = row * 4 + dword of the
// window cuts its four target pixels for the winner out of s_pat and takes lp_prop_visible's statistic there: D, mu and R over the
// window's mask pixels.  A gated block gives no correction: vec 0, valid 0.  The `gated` plane is written where the job has one: the
// batched gated form (lp_prop_match_batch with LP_PROP_MATCH_GATED) has none, its jobs hold six pointers.
template <bool Gated>
__global__ __launch_bounds__(256) void lp_prop_anchor_match_kernel(const anchor_args a) {
    __shared__ uint32_t s_src[kVisSide * kAncPitch], s_bm[kVisSide * kAncPitch], s_pat[kAncPatRows * kAncPatPitch];
    __shared__ int32_t s_S[4][kMaxCand];
    const int32_t* __restrict__ pos = a.job[blockIdx.z].pos;
    const uint8_t* __restrict__ tgt = a.job[blockIdx.z].tgt;
    const uint8_t* __restrict__ key = a.job[blockIdx.z].key;
    const uint8_t* __restrict__ msk = a.job[blockIdx.z].msk;
    int32_t* __restrict__ vec = a.job[blockIdx.z].vec;
    int32_t* __restrict__ valid = a.job[blockIdx.z].valid;
    int32_t* __restrict__ gated = Gated ? a.job[blockIdx.z].gated : nullptr;
    const int wide = static_cast<int>((a.wide >> blockIdx.z) & 1u);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
    const int H = a.H, W = a.W, R = a.search, n = 2 * R + 1, ncand = n * n;
    const int y00 = blockIdx.y * kTile - kHalo, x00 = blockIdx.x * kTile - kHalo;     // x00 is a multiple of 4
    // K of the tile and its halo, four pixels a dword, 0 where the pixel is outside the image or the mask, and the per-byte mask.
    // wide: width % 4 == 0 and the planes 16-byte aligned, so a quad is inside its row or outside it, and one vector
    uint32_t any = 0;
    for (int i = tid; i < kVisSide * kAncPitch; i += 256) {
        const int r = i / kAncPitch, q = i - r * kAncPitch;
        const int y = y00 + r, x = x00 + 4 * q;
        uint32_t sv = 0, bm = 0;
        if (y >= 0 && y < H && x + 3 >= 0 && x < W) {
            const int64_t p = static_cast<int64_t>(y) * W + x;
            if (wide) {                                                  // x >= 0 and x + 3 < W; p is a multiple of 4
                const uchar4 m4 = *reinterpret_cast<const uchar4*>(msk + p);
                if (m4.x | m4.y | m4.z | m4.w) {
                    const int4 pa = *reinterpret_cast<const int4*>(pos + p * 2), pb = *reinterpret_cast<const int4*>(pos + p * 2 + 4);
                    if (m4.x) { bm |= 0xFFu;       sv |= static_cast<uint32_t>(warped_key_of(key, H, W, pa.x, pa.y)); }
                    if (m4.y) { bm |= 0xFFu << 8;  sv |= static_cast<uint32_t>(warped_key_of(key, H, W, pa.z, pa.w)) << 8; }
                    if (m4.z) { bm |= 0xFFu << 16; sv |= static_cast<uint32_t>(warped_key_of(key, H, W, pb.x, pb.y)) << 16; }
                    if (m4.w) { bm |= 0xFFu << 24; sv |= static_cast<uint32_t>(warped_key_of(key, H, W, pb.z, pb.w)) << 24; }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + k >= 0 && x + k < W && msk[p + k]) {
                        bm |= 0xFFu << (8 * k);
                        sv |= static_cast<uint32_t>(warped_key_of(key, H, W, pos[(p + k) * 2], pos[(p + k) * 2 + 1])) << (8 * k);
                    }
            }
        }
        s_src[i] = sv;
        s_bm[i] = bm;
        any |= bm;
    }
    const int by0 = blockIdx.y * (kTile / kB), bx0 = blockIdx.x * (kTile / kB);
    if (!__syncthreads_or(any != 0)) {                                   // no mask pixel in reach of the tile: the whole block leaves
        const int by = by0 + (tid >> 2), bx = bx0 + (tid & 3);
        if (tid < 16 && by < a.gh && bx < a.gw) {
            const int64_t cell = static_cast<int64_t>(by) * a.gw + bx;
            vec[cell * 2] = 0;
            vec[cell * 2 + 1] = 0;
            valid[cell] = 0;
            if (Gated && gated) gated[cell] = 0;
        }
        return;
    }
    // the target patch: row j, byte i is Yt(clamp(y00 - R + j), clamp(x00 - R + i))
    const int rows = kVisSide + 2 * R;
    for (int i = tid; i < rows * kAncPatPitch; i += 256) {
        const int j = i / kAncPatPitch, c0 = (i - j * kAncPatPitch) * 4;
        const uint8_t* row = tgt + static_cast<int64_t>(clampi(y00 - R + j, 0, H - 1)) * W;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= static_cast<uint32_t>(row[clampi(x00 - R + c0 + k, 0, W - 1)]) << (8 * k);
        s_pat[i] = v;
    }
    __syncthreads();
    // a wave takes four of the tile's 4 x 4 windows, one a round; every wave reaches every barrier
#pragma unroll 1
    for (int round = 0; round < 4; ++round) {
        const int win = round * 4 + wv, wy = win >> 2, wx = win & 3;
        const int by = by0 + wy, bx = bx0 + wx;
        const int q0 = wy * kB * kAncPitch + wx * (kB / 4);              // the window's first dword of s_src / s_bm
        int count = __popc(s_bm[q0 + (lane >> 2) * kAncPitch + (lane & 3)]) >> 3;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) count += __shfl_xor(count, d, kWave);
        const bool live = by < a.gh && bx < a.gw && count >= LP_PROP_MIN_PIXELS;      // the same in every lane of the wave
        uint32_t best = 0xFFFFFFFFu;
        bool gate = false;                                               // the same in every lane of the wave
        if (live) {
            for (int c = lane; c < ncand; c += kWave) {
                const int cy = c / n, cx = c - cy * n;                  // oy + R, ox + R
                const int o = wx * kB + cx, word = o >> 2, shift = o & 3;       // word + 4 <= 13: inside the patch row
                uint32_t S = 0;
                for (int r = 0; r < kWin; ++r) {
                    const uint32_t* pr = s_pat + (wy * kB + r + cy) * kAncPatPitch + word;
                    const int q = q0 + r * kAncPitch;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t t = __builtin_amdgcn_alignbyte(pr[k + 1], pr[k], shift) & s_bm[q + k];
                        S = __builtin_amdgcn_sad_u8(s_src[q + k], t, S);
                    }
                }
                s_S[wv][c] = static_cast<int32_t>(S);
                const uint32_t dist = static_cast<uint32_t>(abs(cy - R) + abs(cx - R));
                best = min(best, ((S + static_cast<uint32_t>(a.smooth) * dist) << 12) | (dist << 8) | static_cast<uint32_t>(c));
            }
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) best = min(best, static_cast<uint32_t>(__shfl_xor(static_cast<int>(best), d, kWave)));
            if (Gated) {
                const int c = static_cast<int>(best & 255u), cy = c / n, cx = c - cy * n;
                const int o = wx * kB + cx, shift = o & 3, r = lane >> 2, k = lane & 3;
                const uint32_t* pr = s_pat + (wy * kB + r + cy) * kAncPatPitch + (o >> 2) + k;
                const uint32_t t = __builtin_amdgcn_alignbyte(pr[1], pr[0], shift);
                const uint32_t bm = s_bm[q0 + r * kAncPitch + k], sv = s_src[q0 + r * kAncPitch + k];
                int dd[4], D = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {                            // d = Yt - K on a mask pixel
                    dd[b] = static_cast<int>((t >> (8 * b)) & 255u) - static_cast<int>((sv >> (8 * b)) & 255u);
                    D += (bm >> (8 * b)) & 1u ? dd[b] : 0;
                }
#pragma unroll
                for (int d = 1; d < kWave; d <<= 1) D += __shfl_xor(D, d, kWave);
                const int mu = clampi(floor_div(2 * D + count, 2 * count), -LP_PROP_VIS_MAX_BIAS, LP_PROP_VIS_MAX_BIAS);
                int Rs = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) Rs += (bm >> (8 * b)) & 1u ? abs(dd[b] - mu) : 0;
#pragma unroll
                for (int d = 1; d < kWave; d <<= 1) Rs += __shfl_xor(Rs, d, kWave);
                gate = Rs > a.occlusion * count;
            }
        }
        __syncthreads();                                                 // the wave's s_S is complete
        if (lane == 0 && by < a.gh && bx < a.gw) {
            int vy = 0, vx = 0;
            if (live && !gate) {
                const int c = static_cast<int>(best & 255u), cy = c / n, cx = c - cy * n;
                vy = 16 * (cy - R);
                vx = 16 * (cx - R);
                const int s0 = s_S[wv][c];
                if (s0 != 0) {
                    if (cy > 0 && cy < 2 * R) {
                        const int cm = s_S[wv][c - n], cp = s_S[wv][c + n], d = cm + cp - 2 * s0, g = cm - cp;
                        if (d > 0) vy += (g > 0 ? 1 : (g < 0 ? -1 : 0)) * min(abs(8 * g) / d, 8);
                    }
                    if (cx > 0 && cx < 2 * R) {
                        const int cm = s_S[wv][c - 1], cp = s_S[wv][c + 1], d = cm + cp - 2 * s0, g = cm - cp;
                        if (d > 0) vx += (g > 0 ? 1 : (g < 0 ? -1 : 0)) * min(abs(8 * g) / d, 8);
                    }
                }
            }
            const int64_t cell = static_cast<int64_t>(by) * a.gw + bx;
            vec[cell * 2] = vy;
            vec[cell * 2 + 1] = vx;
            valid[cell] = live && !gate ? 1 : 0;
            if (Gated && gated) gated[cell] = gate ? 1 : 0;
        }
    }
}

// ---- merge ---------------------------------------------------------------------------------------------------------------------------------
// Frame f of the stack is frame j = first + f of a gap of n = span frames: out = 0.5 + ((n - j) sA + j sB) / n, clamped to 0..1.
__device__ __forceinline__ float merge_value(int32_t qa, int32_t qb, int span, int j) {
    const double sa = capped_distance(qa), sb = capped_distance(qb);
    const double acc = __dadd_rn(__dmul_rn(static_cast<double>(span - j), sa), __dmul_rn(static_cast<double>(j), sb));
    const double sd = __ddiv_rn(acc, static_cast<double>(span));
    return static_cast<float>(fmin(fmax(__dadd_rn(0.5, sd), 0.0), 1.0));
}

__global__ __launch_bounds__(256) void lp_prop_merge_kernel(const int32_t* __restrict__ qa, const int32_t* __restrict__ qb,
                                                            float* __restrict__ out, int64_t plane, int span, int first) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= plane) return;
    const int64_t i = static_cast<int64_t>(blockIdx.y) * plane + p;
    out[i] = merge_value(qa[i], qb[i], span, first + static_cast<int>(blockIdx.y));
}

// ---- merge of occlusion-aware chains ---------------------------------------------------------------------------------------------------------
// out may be mask_a and hidden may be code_a (the caller's in-place form): a lane reads its pixels before it writes them, and no
// other lane touches them, so these four carry no __restrict__.
struct merge_visible_args {
    const int32_t* qa;
    const int32_t* qb;
    const float*   code_a;
    const float*   mask_a;
    const float*   code_b;
    const float*   mask_b;
    const int32_t* flags_a;
    const int32_t* flags_b;
    const int32_t* count_a;
    const int32_t* count_b;
    float*         out;
    float*         hidden;
    int64_t plane;
    int32_t W, gh, gw, span, first;
};

// a chain is lost at its step s: its key has at least LP_PROP_MIN_PIXELS bits and some step 1..s has fewer visible bits
__device__ __forceinline__ bool lost_at(const int32_t* __restrict__ count, int s) {
    if (count[0] < LP_PROP_MIN_PIXELS) return false;
    bool lost = false;
#pragma unroll 1
    for (int u = 1; u <= s; ++u) lost |= count[u] < LP_PROP_MIN_PIXELS;
    return lost;
}

template <int V>                                                         // pixels per lane: 4 (16-byte accesses) or 1
__global__ __launch_bounds__(256) void lp_prop_merge_visible_kernel(const merge_visible_args a) {
    const int64_t p = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * V;
    if (p >= a.plane) return;                                            // V == 4: the plane is a multiple of 4
    const int f = static_cast<int>(blockIdx.y), j = a.first + f;
    const bool lost_a = lost_at(a.count_a, j), lost_b = lost_at(a.count_b, a.span - j);       // the same in every lane
    const int64_t i = static_cast<int64_t>(f) * a.plane + p;
    float m[V], h[V];
    if (lost_a != lost_b) {                                              // the chain that is not lost, bit for bit
        const float* code = lost_a ? a.code_b : a.code_a;
        const float* mask = lost_a ? a.mask_b : a.mask_a;
        float c[V];
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(c) = *reinterpret_cast<const float4*>(code + i);
            *reinterpret_cast<float4*>(m) = *reinterpret_cast<const float4*>(mask + i);
        } else {
            c[0] = code[i];
            m[0] = mask[i];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int cc = clampi(static_cast<int>(c[k] * 256.0f), 0, 256), cv = clampi(static_cast<int>(m[k] * 256.0f), 0, 256);
            m[k] = static_cast<float>(cv) * (1.0f / 256.0f);
            h[k] = static_cast<float>(cc - cv) * (1.0f / 256.0f);
        }
    } else {
        int32_t qa[V], qb[V];
        if constexpr (V == 4) {
            *reinterpret_cast<int4*>(qa) = *reinterpret_cast<const int4*>(a.qa + i);
            *reinterpret_cast<int4*>(qb) = *reinterpret_cast<const int4*>(a.qb + i);
        } else {
            qa[0] = a.qa[i];
            qb[0] = a.qb[i];
        }
        const int32_t* __restrict__ flags = (2 * j <= a.span ? a.flags_a : a.flags_b) + static_cast<int64_t>(f) * a.gh * a.gw;
        const int y = static_cast<int>(p / a.W), x = static_cast<int>(p - static_cast<int64_t>(y) * a.W);   // V == 4: one row
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float s = merge_value(qa[k], qb[k], a.span, j);
            const int cs = static_cast<int>(__fadd_rn(__fmul_rn(s, 256.0f), 0.5f));
            const int cv = (cs * weight_of(flags, a.gh, a.gw, y, x + k) + 128) >> 8;
            m[k] = static_cast<float>(cv) * (1.0f / 256.0f);
            h[k] = static_cast<float>(cs - cv) * (1.0f / 256.0f);
        }
    }
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(a.out + i) = *reinterpret_cast<const float4*>(m);
        *reinterpret_cast<float4*>(a.hidden + i) = *reinterpret_cast<const float4*>(h);
    } else {
        a.out[i] = m[0];
        a.hidden[i] = h[0];
    }
}

bool jobs_ok(int n) { return n >= 1 && n <= LP_PROP_MAX_JOBS; }

}  // namespace

extern "C" int64_t lp_prop_pyramid_ws_bytes(int32_t frames, int32_t height, int32_t width, int32_t levels) {
    if (frames <= 0 || !side_ok(height) || !side_ok(width) || !levels_ok(levels)) return LP_E_INVALID;
    return static_cast<int64_t>(frames) * level_offset(height, width, levels);
}

extern "C" int lp_prop_luma(const lp_prop_luma_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_prop_luma_desc& d = *dp;
    if (d.frames <= 0 || !side_ok(d.height) || !side_ok(d.width) || !levels_ok(d.levels)) return LP_E_INVALID;
    if (d.channels < 1 || d.channels > LP_DETAIL_MAX_CHANNELS || !d.image || !d.pyramid) return LP_E_INVALID;
    if (d.frames > 65535) return LP_E_UNSUPPORTED;
    const int64_t plane = static_cast<int64_t>(d.height) * d.width, stride = level_offset(d.height, d.width, d.levels);
    hipLaunchKernelGGL(lp_prop_luma_kernel, dim3(blocks_of(plane, 256), d.frames), dim3(256), 0, stream, d.image, d.pyramid, plane,
                       d.channels, stride);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    for (int l = 1; l < d.levels; ++l) {
        const int sh = level_side(d.height, l - 1), sw = level_side(d.width, l - 1), dh = level_side(d.height, l), dw = level_side(d.width, l);
        hipLaunchKernelGGL(lp_prop_down_kernel, dim3(blocks_of(static_cast<int64_t>(dh) * dw, 256), d.frames), dim3(256), 0, stream,
                           d.pyramid, stride, level_offset(d.height, d.width, l - 1), level_offset(d.height, d.width, l), sh, sw, dh, dw);
        if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    }
    return LP_OK;
}

extern "C" int lp_prop_key_mask(const float* mask, int32_t height, int32_t width, int32_t levels, uint8_t* mpyr, float* out, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!mask || !mpyr || !side_ok(height) || !side_ok(width) || !levels_ok(levels)) return LP_E_INVALID;
    if (out == mask) return LP_E_INVALID;
    hipLaunchKernelGGL(lp_prop_key_mask_kernel, dim3(blocks_of(width, kTile), blocks_of(height, kTile)), dim3(256), 0, stream, mask,
                       height, width, levels, mpyr, out);
    return launched();
}

// The anchor match's one dispatch, `jobs` of them on blockIdx.z: the two single entries with one job, `gated` the anchored
// occlusion-aware form's, and lp_prop_match_batch's warped-key and gated forms.  A launch is all gated or all ungated, with one
// `occlusion`; a gated job may go without its `gated` plane (the batch's jobs do), an ungated job has none.
static int anchor_launch(int height, int width, int anchor, int smooth, int occlusion, const anchor_job* job, int jobs, bool gated,
                         hipStream_t stream) {
    if (!side_ok(height) || !side_ok(width)) return LP_E_INVALID;
    if (anchor < 1 || anchor > LP_PROP_MAX_SEARCH || smooth < 0 || smooth > LP_PROP_MAX_SMOOTH) return LP_E_INVALID;
    if (!jobs_ok(jobs) || !job) return LP_E_INVALID;
    anchor_args a = {};
    for (int i = 0; i < jobs; ++i) {
        const anchor_job& j = job[i];
        if (!j.pos || !j.tgt || !j.key || !j.msk || !j.vec || !j.valid || (j.gated && !gated)) return LP_E_INVALID;
        const void* outs[3] = {j.vec, j.valid, j.gated};
        for (int k = 0; k < 3; ++k) {                                    // gated may be null; an output aliases nothing
            if (!outs[k]) continue;
            for (const void* in : {static_cast<const void*>(j.pos), static_cast<const void*>(j.tgt), static_cast<const void*>(j.key),
                                   static_cast<const void*>(j.msk)})
                if (outs[k] == in) return LP_E_INVALID;
            for (int m = k + 1; m < 3; ++m)
                if (outs[k] == outs[m]) return LP_E_INVALID;
        }
        a.job[i] = j;
        // wide: the kernel reads a row's four pixels as one vector
        if (width % 4 == 0 && aligned16(j.pos) && aligned16(j.msk)) a.wide |= 1u << i;
    }
    a.H = height;
    a.W = width;
    a.gh = (height + kB - 1) / kB;
    a.gw = (width + kB - 1) / kB;
    a.search = anchor;
    a.smooth = smooth;
    a.occlusion = occlusion;
    const dim3 grid(blocks_of(width, kTile), blocks_of(height, kTile), jobs);
    if (gated)
        hipLaunchKernelGGL(lp_prop_anchor_match_kernel<true>, grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(lp_prop_anchor_match_kernel<false>, grid, dim3(256), 0, stream, a);
    return launched();
}

extern "C" int lp_prop_match_batch(const lp_prop_match_batch_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_prop_match_batch_desc& d = *dp;
    // the source form: 0, LP_PROP_MATCH_WARPED_KEY, or LP_PROP_MATCH_GATED(occlusion) with occlusion 1..255 in bits 8..15
    const bool warped = (d.reserved0 & 0xFF) == LP_PROP_MATCH_WARPED_KEY && (d.reserved0 & ~0xFFFF) == 0;
    if (d.reserved0 != 0 && !warped) return LP_E_INVALID;
    const int occlusion = d.reserved0 >> 8;                              // 0: the ungated form
    if (!side_ok(d.height) || !side_ok(d.width) || !levels_ok(d.levels) || d.level < 0 || d.level >= d.levels) return LP_E_INVALID;
    if (d.search < 1 || d.search > LP_PROP_MAX_SEARCH || d.smooth < 0 || d.smooth > LP_PROP_MAX_SMOOTH) return LP_E_INVALID;
    if (!jobs_ok(d.jobs) || !d.job) return LP_E_INVALID;
    if (warped) {                                                        // the anchor match: level 0 of the three pyramids is their start
        if (d.level != 0) return LP_E_INVALID;
        anchor_job job[LP_PROP_MAX_JOBS];
        for (int i = 0; i < d.jobs; ++i) {
            const lp_prop_match_job& j = d.job[i];
            job[i] = {j.parent, j.tgt, j.src, j.mask, j.vec, j.valid, nullptr};
        }
        return anchor_launch(d.height, d.width, d.search, d.smooth, occlusion, job, d.jobs, occlusion != 0, stream);
    }
    match_args a = {};
    const int64_t off = level_offset(d.height, d.width, d.level);
    for (int i = 0; i < d.jobs; ++i) {
        const lp_prop_match_job& j = d.job[i];
        if (!j.src || !j.tgt || !j.mask || !j.vec || !j.valid) return LP_E_INVALID;
        if ((j.parent == nullptr) != (d.level == d.levels - 1) || j.parent == j.vec) return LP_E_INVALID;
        a.job[i] = {j.src + off, j.tgt + off, j.mask + off, j.parent, j.vec, j.valid};
    }
    a.h = level_side(d.height, d.level);
    a.w = level_side(d.width, d.level);
    a.gw = (a.w + kB - 1) / kB;
    const int gh = (a.h + kB - 1) / kB;
    a.pgh = (level_side(d.height, d.level + 1) + kB - 1) / kB;
    a.pgw = (level_side(d.width, d.level + 1) + kB - 1) / kB;
    a.search = d.search;
    a.smooth = d.smooth;
    a.subpel = d.level == 0;
    hipLaunchKernelGGL(lp_prop_match_kernel, dim3(a.gw, gh, d.jobs), dim3(kWave), 0, stream, a);
    return launched();
}

extern "C" int lp_prop_match(const lp_prop_match_desc* dp, void* stream) {
    if (!dp) return LP_E_INVALID;
    const lp_prop_match_job job = {dp->src, dp->tgt, dp->mask, dp->parent, dp->vec, dp->valid};
    const lp_prop_match_batch_desc d = {dp->height, dp->width, dp->levels, dp->level, dp->search, dp->smooth, 1, 0, &job};
    return lp_prop_match_batch(&d, stream);
}

extern "C" int lp_prop_fill_batch(const lp_prop_fill_job* job, int32_t jobs, int32_t gh, int32_t gw, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!job || !jobs_ok(jobs) || gh < 1 || gw < 1 || gh > LP_PROP_MAX_GRID || gw > LP_PROP_MAX_GRID) return LP_E_INVALID;
    fill_args a = {};
    a.gh = gh;
    a.gw = gw;
    for (int i = 0; i < jobs; ++i) {
        if (!job[i].vec || !job[i].valid || !job[i].out || job[i].out == job[i].vec) return LP_E_INVALID;
        a.job[i] = {job[i].vec, job[i].valid, job[i].out};
    }
    hipLaunchKernelGGL(lp_prop_fill_kernel, dim3(blocks_of(gw, kFillTile), blocks_of(gh, kFillTile), jobs), dim3(256), 0, stream, a);
    return launched();
}

extern "C" int lp_prop_fill(const int32_t* vec, const int32_t* valid, int32_t gh, int32_t gw, int32_t* out, void* stream) {
    const lp_prop_fill_job job = {vec, valid, out};
    return lp_prop_fill_batch(&job, 1, gh, gw, stream);
}

extern "C" int lp_prop_advance_batch(const lp_prop_advance_batch_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_prop_advance_batch_desc& d = *dp;
    if (!side_ok(d.height) || !side_ok(d.width) || !levels_ok(d.levels) || !jobs_ok(d.jobs) || !d.job) return LP_E_INVALID;
    advance_args a = {};
    for (int i = 0; i < d.jobs; ++i) {
        const lp_prop_advance_job& j = d.job[i];
        if (!j.vec || !j.key || !j.pos_dst || !j.out || !j.mask_pyramid || j.pos_dst == j.pos_src || j.mask_pyramid == j.key)
            return LP_E_INVALID;
        a.job[i] = {j.vec, j.pos_src, j.key, j.pos_dst, j.out, j.mask_pyramid};
    }
    a.height = d.height;
    a.width = d.width;
    a.levels = d.levels;
    a.gh = (d.height + kB - 1) / kB;
    a.gw = (d.width + kB - 1) / kB;
    hipLaunchKernelGGL(lp_prop_advance_kernel, dim3(blocks_of(d.width, kTile), blocks_of(d.height, kTile), d.jobs), dim3(256), 0, stream, a);
    return launched();
}

extern "C" int lp_prop_advance(const lp_prop_advance_desc* dp, void* stream) {
    if (!dp) return LP_E_INVALID;
    const lp_prop_advance_job job = {dp->vec, dp->pos_src, dp->key, dp->pos_dst, dp->out, dp->mask_pyramid};
    const lp_prop_advance_batch_desc d = {dp->height, dp->width, dp->levels, 1, &job};
    return lp_prop_advance_batch(&d, stream);
}

extern "C" int lp_prop_visible_batch(const lp_prop_visible_batch_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_prop_visible_batch_desc& d = *dp;
    if (!side_ok(d.height) || !side_ok(d.width) || d.occlusion < 1 || d.occlusion > 255) return LP_E_INVALID;
    if (!jobs_ok(d.jobs) || !d.job) return LP_E_INVALID;
    visible_args a = {};
    for (int i = 0; i < d.jobs; ++i) {
        const lp_prop_visible_job& j = d.job[i];
        if (!j.pos || !j.tgt || !j.key || !j.mask || !j.flags) return LP_E_INVALID;
        const void* out = j.flags;
        if (out == j.pos || out == j.tgt || out == j.key || out == j.mask) return LP_E_INVALID;
        a.job[i] = {j.pos, j.tgt, j.key, j.mask, j.flags};
        // wide: the kernel reads a row's four pixels as one vector
        if (d.width % 4 == 0 && aligned16(j.pos) && aligned16(j.tgt) && aligned16(j.mask)) a.wide |= 1u << i;
    }
    a.H = d.height;
    a.W = d.width;
    a.gh = (d.height + kB - 1) / kB;
    a.gw = (d.width + kB - 1) / kB;
    a.occlusion = d.occlusion;
    hipLaunchKernelGGL(lp_prop_visible_kernel, dim3(blocks_of(d.width, kTile), blocks_of(d.height, kTile), d.jobs), dim3(256), 0, stream, a);
    return launched();
}

extern "C" int lp_prop_visible(const lp_prop_visible_desc* dp, void* stream) {
    if (!dp) return LP_E_INVALID;
    const lp_prop_visible_job job = {dp->pos, dp->tgt, dp->key, dp->mask, dp->flags};
    const lp_prop_visible_batch_desc d = {dp->height, dp->width, dp->occlusion, 1, &job};
    return lp_prop_visible_batch(&d, stream);
}

extern "C" int lp_prop_occlude_batch(const lp_prop_occlude_batch_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_prop_occlude_batch_desc& d = *dp;
    if (!side_ok(d.height) || !side_ok(d.width) || !levels_ok(d.levels) || !jobs_ok(d.jobs) || !d.job) return LP_E_INVALID;
    occlude_args a = {};
    for (int i = 0; i < d.jobs; ++i) {
        const lp_prop_occlude_job& j = d.job[i];
        if (!j.code || !j.flags || !j.out || !j.hidden || !j.mask_pyramid) return LP_E_INVALID;
        const void *in[2] = {j.code, j.flags}, *outs[4] = {j.out, j.hidden, j.mask_pyramid, j.count};
        for (int k = 0; k < 4; ++k) {                                    // count may be null; given, it aliases nothing
            if (!outs[k]) continue;
            if (outs[k] == in[0] || outs[k] == in[1]) return LP_E_INVALID;
            for (int m = k + 1; m < 4; ++m)
                if (outs[k] == outs[m]) return LP_E_INVALID;
        }
        a.job[i] = {j.code, j.flags, j.out, j.hidden, j.mask_pyramid, j.count};
        if (d.width % 4 == 0 && aligned16(j.code) && aligned16(j.out) && aligned16(j.hidden)) a.wide |= 1u << i;
    }
    a.H = d.height;
    a.W = d.width;
    a.levels = d.levels;
    a.gh = (d.height + kB - 1) / kB;
    a.gw = (d.width + kB - 1) / kB;
    hipLaunchKernelGGL(lp_prop_occlude_kernel, dim3(blocks_of(d.width, kTile), blocks_of(d.height, kTile), d.jobs), dim3(256), 0, stream, a);
    return launched();
}

extern "C" int lp_prop_occlude(const lp_prop_occlude_desc* dp, void* stream) {
    if (!dp) return LP_E_INVALID;
    const lp_prop_occlude_job job = {dp->code, dp->flags, dp->out, dp->hidden, dp->mask_pyramid, nullptr};
    const lp_prop_occlude_batch_desc d = {dp->height, dp->width, dp->levels, 1, &job};
    return lp_prop_occlude_batch(&d, stream);
}

extern "C" int lp_prop_anchor_match(const lp_prop_anchor_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const anchor_job job = {dp->pos, dp->tgt, dp->key, dp->mask, dp->vec, dp->valid, nullptr};
    return anchor_launch(dp->height, dp->width, dp->anchor, dp->smooth, 0, &job, 1, false, stream);
}

extern "C" int lp_prop_anchor_match_gated(const lp_prop_anchor_gated_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    if (!dp->gated || dp->occlusion < 1 || dp->occlusion > 255 || dp->reserved0 != 0) return LP_E_INVALID;
    const anchor_job job = {dp->pos, dp->tgt, dp->key, dp->mask, dp->vec, dp->valid, dp->gated};
    return anchor_launch(dp->height, dp->width, dp->anchor, dp->smooth, dp->occlusion, &job, 1, true, stream);
}

extern "C" int lp_prop_merge(const lp_prop_merge_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_prop_merge_desc& d = *dp;
    if (!d.qa || !d.qb || !d.out || !side_ok(d.height) || !side_ok(d.width)) return LP_E_INVALID;
    if (d.span < 2 || d.first < 1 || d.frames < 1 || static_cast<int64_t>(d.first) + d.frames - 1 > static_cast<int64_t>(d.span) - 1)
        return LP_E_INVALID;
    if (static_cast<const void*>(d.out) == d.qa || static_cast<const void*>(d.out) == d.qb) return LP_E_INVALID;
    if (d.span > 65535) return LP_E_UNSUPPORTED;                     // frames <= span - 1: inside a grid's y limit
    const int64_t plane = static_cast<int64_t>(d.height) * d.width;
    hipLaunchKernelGGL(lp_prop_merge_kernel, dim3(blocks_of(plane, 256), d.frames), dim3(256), 0, stream, d.qa, d.qb, d.out, plane, d.span,
                       d.first);
    return launched();
}

extern "C" int lp_prop_merge_visible(const lp_prop_merge_visible_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_prop_merge_visible_desc& d = *dp;
    const void* in[10] = {d.qa, d.qb, d.code_a, d.mask_a, d.code_b, d.mask_b, d.flags_a, d.flags_b, d.count_a, d.count_b};
    for (const void* p : in)
        if (!p) return LP_E_INVALID;
    if (!d.out || !d.hidden || d.out == d.hidden || !side_ok(d.height) || !side_ok(d.width)) return LP_E_INVALID;
    if (d.span < 2 || d.first < 1 || d.frames < 1 || static_cast<int64_t>(d.first) + d.frames - 1 > static_cast<int64_t>(d.span) - 1)
        return LP_E_INVALID;
    for (const void* p : in) {                                       // in place on the forward chain's planes only
        if (p == d.out && p != d.mask_a) return LP_E_INVALID;
        if (p == d.hidden && p != d.code_a) return LP_E_INVALID;
    }
    if (d.span > 65535) return LP_E_UNSUPPORTED;                     // frames <= span - 1: inside a grid's y limit
    merge_visible_args a = {d.qa, d.qb, d.code_a, d.mask_a, d.code_b, d.mask_b, d.flags_a, d.flags_b, d.count_a, d.count_b, d.out, d.hidden};
    a.plane = static_cast<int64_t>(d.height) * d.width;
    a.W = d.width;
    a.gh = (d.height + kB - 1) / kB;
    a.gw = (d.width + kB - 1) / kB;
    a.span = d.span;
    a.first = d.first;
    bool wide = d.width % 4 == 0;
    for (const void* p : {in[0], in[1], in[2], in[3], in[4], in[5], static_cast<const void*>(d.out), static_cast<const void*>(d.hidden)})
        wide = wide && aligned16(p);
    if (wide)
        hipLaunchKernelGGL(lp_prop_merge_visible_kernel<4>, dim3(blocks_of(a.plane / 4, 256), d.frames), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(lp_prop_merge_visible_kernel<1>, dim3(blocks_of(a.plane, 256), d.frames), dim3(256), 0, stream, a);
    return launched();
}

}  // namespace lp
