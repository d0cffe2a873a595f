// patch_fill_kernel.hip -- the patch form of lp_mask_fill for gfx950 (lanpaint_amd/fill.py, fill_masked_patch): under the mask,
// the push-pull fill is replaced by texture copied from the known part of the same image.  include/lanpaint_hip.h states the rule
// (LP_FILL_PATCH); lp_mask_fill itself, its checks and the push-pull launches are fill_kernel.hip's.
//
//   codes, down  a lane per pixel: the 8-bit codes of the push-pull result, four channels a dword, and the hole flags; then level
//                by level the rounded means of the children and the OR of their flags.  `work` (T) starts as a copy of the codes.
//   sets         a lane per pixel reads the (2r + 1)^2 hole flags around it: target and source bits.
//   field        a level's first field: the level above doubled, or all INVALID at the coarsest level.
//   search       the hot kernel.  A block per 16 x 16 tile of targets, T of the tile and its r-halo staged once in LDS, a lane per
//                target walking its candidates: its own entry, eight neighbours' entries, then the random search around the best so
//                far with one Philox4x32-10 block per radius.  A candidate's distance is one v_sad_u8 per pixel, the four channel
//                bytes being the instruction's four lanes; its patch is read through L2.  A candidate is dropped as soon as its
//                partial distance exceeds the best one -- strictly, so that the key (D, s_y, s_x) still decides a tie.  Jacobi:
//                reads one field, writes the other; a tile with no target writes its INVALIDs and leaves.
//   vote         a gather, no atomics: a block per 16 x 16 tile, the field of the tile and its r-halo in LDS, a lane per hole pixel
//                sums the (2r + 1)^2 source pixels that the patches around it bring.  The last vote of level 0 also writes `out`.
// Everything is integer arithmetic on values that do not depend on what a launch covers, so the bits are the same for every batch.
#include "lp_common.h"

namespace lp {
namespace {

constexpr int kTile = LP_FILL_PATCH_TILE, kMaxR = LP_FILL_PATCH_MAX_RADIUS;
constexpr int kSide = kTile + 2 * kMaxR;                 // a tile and its halo at the largest radius
constexpr int kHole = 1, kTarget = 2, kSource = 4;       // the bits of a `sets` byte
constexpr int32_t kInvalid = -1;
static_assert(kTile == 16, "a block is 256 lanes, one per pixel of a 16 x 16 tile");

// One level of one call: the planes of include/lanpaint_hip.h's workspace layout, image b at element b * h * w.
struct PatchLevel {
    uint32_t* codes;
    uint32_t* work;
    int32_t*  nnf;
    int32_t*  nnf2;
    uint8_t*  hole;
    uint8_t*  sets;
    int32_t   h, w;
};

__device__ __forceinline__ uint32_t mean4(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t n) {
    const uint32_t half = n >> 1;
    return (s0 + half) / n | ((s1 + half) / n) << 8 | ((s2 + half) / n) << 16 | ((s3 + half) / n) << 24;
}

// ---- codes and pyramid --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lp_patch_codes_kernel(const float* __restrict__ pp, const float* __restrict__ mask,
                                                             int mask_batch, int C, PatchLevel g) {
    const int64_t n = static_cast<int64_t>(g.h) * g.w, p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= n) return;
    const int img = blockIdx.z;
    const float* v = pp + (static_cast<int64_t>(img) * n + p) * C;
    uint32_t word = 0;
    for (int c = 0; c < C; ++c) word |= static_cast<uint32_t>(code_of(v[c])) << (8 * c);
    const float m = mask[static_cast<int64_t>(mask_batch == 1 ? 0 : img) * n + p];
    const int64_t at = static_cast<int64_t>(img) * n + p;
    g.codes[at] = word;
    g.work[at] = word;
    g.hole[at] = m > 0.5f;
}

__global__ __launch_bounds__(256) void lp_patch_down_kernel(PatchLevel f, PatchLevel g) {      // f: the finer level, g = f halved
    const int64_t n = static_cast<int64_t>(g.h) * g.w, p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= n) return;
    const int img = blockIdx.z, i = static_cast<int>(p / g.w), j = static_cast<int>(p - static_cast<int64_t>(i) * g.w);
    const int64_t fine = static_cast<int64_t>(img) * f.h * f.w;
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, cnt = 0, hole = 0;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const int y = 2 * i + (ch >> 1), x = 2 * j + (ch & 1);
        if (y < f.h && x < f.w) {
            const int64_t at = fine + static_cast<int64_t>(y) * f.w + x;
            const uint32_t c = f.codes[at];
            s0 += c & 255u; s1 += (c >> 8) & 255u; s2 += (c >> 16) & 255u; s3 += c >> 24;
            hole |= f.hole[at];
            ++cnt;
        }
    }
    const uint32_t word = mean4(s0, s1, s2, s3, cnt);     // cnt >= 1: child (0, 0) is always inside
    const int64_t at = static_cast<int64_t>(img) * n + p;
    g.codes[at] = word;
    g.work[at] = word;
    g.hole[at] = hole != 0;
}

__global__ __launch_bounds__(256) void lp_patch_sets_kernel(PatchLevel g, int r) {
    const int64_t n = static_cast<int64_t>(g.h) * g.w, p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= n) return;
    const int img = blockIdx.z, y = static_cast<int>(p / g.w), x = static_cast<int>(p - static_cast<int64_t>(y) * g.w);
    const uint8_t* hole = g.hole + static_cast<int64_t>(img) * n;
    const int ya = max(y - r, 0), yb = min(y + r, g.h - 1), xa = max(x - r, 0), xb = min(x + r, g.w - 1);
    uint32_t any = 0;
    for (int yy = ya; yy <= yb; ++yy)
        for (int xx = xa; xx <= xb; ++xx) any |= hole[static_cast<int64_t>(yy) * g.w + xx];
    const bool whole = y - r >= 0 && y + r < g.h && x - r >= 0 && x + r < g.w;
    g.sets[static_cast<int64_t>(img) * n + p] =
        static_cast<uint8_t>((hole[p] ? kHole : 0) | (any ? kTarget : 0) | (whole && !any ? kSource : 0));
}

// ---- a level's first field ------------------------------------------------------------------------------------------------------
// `coarse`: the field the level above ended with, hc x wc; null at the coarsest level
__global__ __launch_bounds__(256) void lp_patch_field_kernel(PatchLevel g, const int32_t* __restrict__ coarse, int hc, int wc,
                                                             int32_t* __restrict__ field) {
    const int64_t n = static_cast<int64_t>(g.h) * g.w, p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= n) return;
    const int img = blockIdx.z, y = static_cast<int>(p / g.w), x = static_cast<int>(p - static_cast<int64_t>(y) * g.w);
    const uint8_t* sets = g.sets + static_cast<int64_t>(img) * n;
    int32_t e = kInvalid;
    if (coarse && (sets[p] & kTarget)) {                  // (y >> 1, x >> 1) lies inside the level above: its sides are rounded up
        const int32_t up = coarse[static_cast<int64_t>(img) * hc * wc + static_cast<int64_t>(y >> 1) * wc + (x >> 1)];
        if (up >= 0) {
            const int sy = 2 * (up >> 16) + (y & 1), sx = 2 * (up & 0xFFFF) + (x & 1);
            if (sy < g.h && sx < g.w && (sets[static_cast<int64_t>(sy) * g.w + sx] & kSource)) e = sy << 16 | sx;
        }
    }
    field[static_cast<int64_t>(img) * n + p] = e;
}

// ---- search -------------------------------------------------------------------------------------------------------------------
struct Best {
    uint32_t d;        // 0xFFFFFFFF while there is none (a distance is at most 81 * 4 * 255)
    int32_t  s;        // s_y << 16 | s_x: for equal d the lower word is the lower (s_y, s_x)
};

// Candidate (sy, sx) for the target at (py, px), whose patch is clipped to rows dy0 .. dy1 and columns dx0 .. dx1; `t` points at the
// target's own pixel in the LDS tile, `img` at the image's codes and `sets` at its set bytes.
__device__ __forceinline__ void consider(Best& best, int sy, int sx, int h, int w, int dy0, int dy1, int dx0, int dx1,
                                         const uint32_t* t, int pitch, const uint32_t* __restrict__ img,
                                         const uint8_t* __restrict__ sets) {
    if (sy < 0 || sy >= h || sx < 0 || sx >= w) return;
    const int64_t at = static_cast<int64_t>(sy) * w + sx;
    if (!(sets[at] & kSource)) return;                    // a source's whole patch lies inside the picture
    uint32_t d = 0;
    for (int dy = dy0; dy <= dy1; ++dy) {
        const uint32_t* srow = img + at + static_cast<int64_t>(dy) * w;
        const uint32_t* trow = t + dy * pitch;
        for (int dx = dx0; dx <= dx1; ++dx) d = __builtin_amdgcn_sad_u8(trow[dx], srow[dx], d);
        if (d > best.d) return;                           // it can neither win nor tie any more
    }
    const int32_t s = sy << 16 | sx;
    if (d < best.d || (d == best.d && s < best.s)) {
        best.d = d;
        best.s = s;
    }
}

__global__ __launch_bounds__(256) void lp_patch_search_kernel(PatchLevel g, const int32_t* __restrict__ fin,
                                                              int32_t* __restrict__ fout, int r, uint32_t level, uint32_t round,
                                                              uint32_t seed) {
    __shared__ uint32_t sT[kSide * kSide];
    const int tid = threadIdx.x, tx = tid & (kTile - 1), ty = tid >> 4, img = blockIdx.z;
    const int h = g.h, w = g.w, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile, px = x0 + tx, py = y0 + ty;
    const int64_t base = static_cast<int64_t>(img) * h * w;
    const uint8_t* sets = g.sets + base;
    const bool in = px < w && py < h;
    const bool target = in && (sets[static_cast<int64_t>(py) * w + px] & kTarget);
    if (in && !target) fout[base + static_cast<int64_t>(py) * w + px] = kInvalid;
    if (!__syncthreads_or(target)) return;                // block-uniform: no target in this tile
    const int side = kTile + 2 * r;
    for (int i = tid; i < side * side; i += 256) {
        const int ly = i / side, lx = i - ly * side, gy = y0 - r + ly, gx = x0 - r + lx;
        sT[i] = gy >= 0 && gy < h && gx >= 0 && gx < w ? g.work[base + static_cast<int64_t>(gy) * w + gx] : 0u;
    }
    __syncthreads();
    if (!target) return;                                  // no barrier below
    const uint32_t* img_codes = g.codes + base;
    const int32_t* field = fin + base;
    const uint32_t* t = sT + (ty + r) * side + tx + r;
    const int dy0 = max(-r, -py), dy1 = min(r, h - 1 - py), dx0 = max(-r, -px), dx1 = min(r, w - 1 - px);
    Best best = {0xFFFFFFFFu, kInvalid};
    const int32_t own = field[static_cast<int64_t>(py) * w + px];
    if (own >= 0) consider(best, own >> 16, own & 0xFFFF, h, w, dy0, dy1, dx0, dx1, t, side, img_codes, sets);
    for (int step = 1; step <= 4; step += 3) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {                     // (0, -1), (-1, 0), (0, 1), (1, 0)
            const int ey = step * (k == 1 ? -1 : k == 3 ? 1 : 0), ex = step * (k == 0 ? -1 : k == 2 ? 1 : 0);
            const int ny = py + ey, nx = px + ex;
            if (ny < 0 || ny >= h || nx < 0 || nx >= w) continue;
            const int64_t at = static_cast<int64_t>(ny) * w + nx;
            if (!(sets[at] & kTarget)) continue;
            const int32_t e = field[at];
            if (e >= 0) consider(best, (e >> 16) - ey, (e & 0xFFFF) - ex, h, w, dy0, dy1, dx0, dx1, t, side, img_codes, sets);
        }
    }
    const int R0 = max(h, w);
    const uint64_t ctr = static_cast<uint64_t>(py) * 65536u + static_cast<uint64_t>(px);
    const uint64_t sub = static_cast<uint64_t>(level) << 40 | static_cast<uint64_t>(round) << 32;
    for (int j = 0; (R0 >> j) >= 1; ++j) {
        const int R = R0 >> j;
        const int cy = best.s >= 0 ? best.s >> 16 : py, cx = best.s >= 0 ? best.s & 0xFFFF : px;
        const uint4 word = philox4x32_10(ctr, sub | static_cast<uint64_t>(j), static_cast<uint64_t>(seed));
        const uint32_t span = 2u * static_cast<uint32_t>(R) + 1u;
        const int uy = static_cast<int>(__umulhi(word.x, span)) - R, ux = static_cast<int>(__umulhi(word.y, span)) - R;
        consider(best, cy + uy, cx + ux, h, w, dy0, dy1, dx0, dx1, t, side, img_codes, sets);
    }
    fout[base + static_cast<int64_t>(py) * w + px] = best.s;
}

// ---- vote ---------------------------------------------------------------------------------------------------------------------
// `out`: null, or the call's output [batch, h, w, C] for the last vote of level 0
__global__ __launch_bounds__(256) void lp_patch_vote_kernel(PatchLevel g, const int32_t* __restrict__ field, int r,
                                                            float* __restrict__ out, int C) {
    __shared__ int32_t sN[kSide * kSide];
    const int tid = threadIdx.x, tx = tid & (kTile - 1), ty = tid >> 4, img = blockIdx.z;
    const int h = g.h, w = g.w, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile, px = x0 + tx, py = y0 + ty;
    const int64_t base = static_cast<int64_t>(img) * h * w;
    const bool hole = px < w && py < h && (g.sets[base + static_cast<int64_t>(py) * w + px] & kHole);
    if (!__syncthreads_or(hole)) return;                  // block-uniform: no hole pixel in this tile
    const int side = kTile + 2 * r;
    for (int i = tid; i < side * side; i += 256) {
        const int ly = i / side, lx = i - ly * side, gy = y0 - r + ly, gx = x0 - r + lx;
        sN[i] = gy >= 0 && gy < h && gx >= 0 && gx < w ? field[base + static_cast<int64_t>(gy) * w + gx] : kInvalid;
    }
    __syncthreads();
    if (!hole) return;
    const uint32_t* codes = g.codes + base;
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, cnt = 0;
    for (int dy = -r; dy <= r; ++dy) {
        const int32_t* row = sN + (ty + r - dy) * side + tx + r;
        for (int dx = -r; dx <= r; ++dx) {
            const int32_t e = row[-dx];                   // the entry of p = q - d
            if (e < 0) continue;
            // a valid entry is a source: its whole patch, e + d included, lies inside the picture
            const uint32_t c = codes[static_cast<int64_t>((e >> 16) + dy) * w + (e & 0xFFFF) + dx];
            s0 += c & 255u; s1 += (c >> 8) & 255u; s2 += (c >> 16) & 255u; s3 += c >> 24;
            ++cnt;
        }
    }
    if (cnt == 0) return;
    const uint32_t word = mean4(s0, s1, s2, s3, cnt);
    const int64_t at = base + static_cast<int64_t>(py) * w + px;
    g.work[at] = word;
    if (out)
        for (int c = 0; c < C; ++c) out[at * C + c] = __fdiv_rn(static_cast<float>((word >> (8 * c)) & 255u), 255.0f);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct PatchMode {
    int r, levels, iters;
    uint32_t seed;
};

bool parse_mode(int32_t reserved0, PatchMode* m) {
    const uint32_t v = static_cast<uint32_t>(reserved0);
    m->r = (v >> 4) & 15;
    m->levels = (v >> 8) & 15;
    m->iters = (v >> 12) & 15;
    m->seed = v >> 16;
    return (v & 15u) == 1u && m->r >= 1 && m->r <= LP_FILL_PATCH_MAX_RADIUS && m->levels >= 1 && m->levels <= LP_FILL_PATCH_MAX_LEVELS &&
           m->iters >= 1 && m->iters <= LP_FILL_PATCH_MAX_ITERS;
}

int64_t round16(int64_t n) { return (n + 15) / 16 * 16; }

// The planes of level l, in the header's order, from `at`; returns the byte behind them.
uint8_t* place_level(uint8_t* at, int batch, int h, int w, PatchLevel* g) {
    const int64_t n = static_cast<int64_t>(batch) * h * w;
    g->h = h;
    g->w = w;
    g->codes = reinterpret_cast<uint32_t*>(at); at += round16(4 * n);
    g->work = reinterpret_cast<uint32_t*>(at);  at += round16(4 * n);
    g->nnf = reinterpret_cast<int32_t*>(at);    at += round16(4 * n);
    g->nnf2 = reinterpret_cast<int32_t*>(at);   at += round16(4 * n);
    g->hole = at;                               at += round16(n);
    g->sets = at;                               at += round16(n);
    return at;
}

}  // namespace

int patch_fill_check(const lp_fill_desc& d) {
    PatchMode m;
    if (!parse_mode(d.reserved0, &m)) return LP_E_INVALID;
    if (d.channels > LP_FILL_PATCH_MAX_CHANNELS) return LP_E_UNSUPPORTED;
    const int64_t pull = lp_fill_ws_bytes(d.batch, d.height, d.width, d.channels);
    if (pull < 0) return static_cast<int>(pull);
    if (d.ws_bytes < LP_FILL_PATCH_WS_BYTES(pull, d.batch, d.height, d.width, m.levels)) return LP_E_INVALID;
    return LP_OK;
}

int patch_fill_enqueue(const lp_fill_desc& d, hipStream_t stream) {
    PatchMode m;
    if (!parse_mode(d.reserved0, &m)) return LP_E_INVALID;
    PatchLevel lev[LP_FILL_PATCH_MAX_LEVELS];
    uint8_t* at = static_cast<uint8_t*>(d.ws) + lp_fill_ws_bytes(d.batch, d.height, d.width, d.channels);
    for (int l = 0; l < m.levels; ++l)
        at = place_level(at, d.batch, static_cast<int>(LP_FILL_PATCH_SIDE(d.height, l)), static_cast<int>(LP_FILL_PATCH_SIDE(d.width, l)),
                         &lev[l]);
    const auto pixels = [&](const PatchLevel& g) {
        return dim3(static_cast<uint32_t>((static_cast<int64_t>(g.h) * g.w + 255) / 256), 1, d.batch);
    };
    const auto tiles = [&](const PatchLevel& g) { return dim3((g.w + kTile - 1) / kTile, (g.h + kTile - 1) / kTile, d.batch); };
    hipLaunchKernelGGL(lp_patch_codes_kernel, pixels(lev[0]), dim3(256), 0, stream, d.out, d.mask, d.mask_batch, d.channels, lev[0]);
    for (int l = 1; l < m.levels; ++l)
        hipLaunchKernelGGL(lp_patch_down_kernel, pixels(lev[l]), dim3(256), 0, stream, lev[l - 1], lev[l]);
    for (int l = 0; l < m.levels; ++l)
        hipLaunchKernelGGL(lp_patch_sets_kernel, pixels(lev[l]), dim3(256), 0, stream, lev[l], m.r);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    for (int l = m.levels - 1; l >= 0; --l) {
        const PatchLevel& g = lev[l];
        const bool top = l == m.levels - 1;
        // the rounds go to and fro between the two fields; the first one is chosen so that the last round writes g.nnf
        int32_t* cur = (m.iters & 1) ? g.nnf2 : g.nnf;
        int32_t* other = (m.iters & 1) ? g.nnf : g.nnf2;
        hipLaunchKernelGGL(lp_patch_field_kernel, pixels(g), dim3(256), 0, stream, g, top ? nullptr : lev[l + 1].nnf,
                           top ? 0 : lev[l + 1].h, top ? 0 : lev[l + 1].w, cur);
        if (!top) hipLaunchKernelGGL(lp_patch_vote_kernel, tiles(g), dim3(256), 0, stream, g, cur, m.r, nullptr, d.channels);
        for (int it = 0; it < m.iters; ++it) {
            hipLaunchKernelGGL(lp_patch_search_kernel, tiles(g), dim3(256), 0, stream, g, cur, other, m.r, static_cast<uint32_t>(l),
                               static_cast<uint32_t>(it), m.seed);
            int32_t* swap = cur;
            cur = other;
            other = swap;
            hipLaunchKernelGGL(lp_patch_vote_kernel, tiles(g), dim3(256), 0, stream, g, cur, m.r,
                               l == 0 && it == m.iters - 1 ? d.out : nullptr, d.channels);
        }
        if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    }
    return LP_OK;
}

}  // namespace lp
