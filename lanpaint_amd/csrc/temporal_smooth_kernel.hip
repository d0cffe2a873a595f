// temporal_smooth_kernel.hip -- video temporal smooth for gfx950 (lanpaint_amd/temporal_smooth.py): what the sampler put under the
// mask of a frame is pulled towards the weighted mean of what it put at the same scene point in the frames around it, as far as
// that agrees with the pixel.  include/lanpaint_hip.h (lp_tsmooth) states the rule.  The fields are the temporal fill's, computed
// by lp_prop_match_batch and lp_prop_fill_batch unchanged; this file holds the gather.
//
//   smooth   one launch for all frames of a chunk: a block per 32 x 32 tile and frame, a lane per pixel.  A lane reads its known
//            byte first.  A wave -- two rows of the tile -- in which none is masked, most of a frame, copies its two runs of
//            pixels, 16 bytes a lane where they are aligned, writes support = -1 and leaves; no wave waits for another, so a
//            block's slots on its CU free up wave by wave (with a barrier and a copy by the whole block the launch was slower:
//            profiles/r33_temporal_smooth.md).  Else a known pixel is copied by its lane, and a masked pixel walks up to R steps
//            into the past, then into the future: per step the four block vectors around its position (the field stays cached:
//            gh gw 8 bytes), the sample's taps, the codes' comparison.  The walk of a pixel depends on nothing another pixel
//            computes: no barrier, no LDS -- every step, the first included, reads its vectors from the field, so the tile's
//            6 x 6 vectors of the carry are not staged.
// Registers: a chain accepts a prefix of its steps, so two counts describe it.  Channels go four at a time: the first four are
// accumulated while the walk decides (every further group is sampled there only to be compared), and each further group walks the
// accepted steps again -- the positions are integers and come out the same -- to accumulate its own four.  Nothing is indexed by a
// register, so nothing lives in scratch.  The sums keep the rule's order: past before future, nearer before farther.
// fp32 in a fixed order, every operation rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn: nothing contracts).
// No atomics.
//
//   robust   (lp_tsmooth_robust, the header's robust section) the same geometry and the same copy of what is not masked.  A masked
//            pixel walks up to three times, the positions being integers that come out the same: for the 8-bit lumas of the up to
//            17 samples, a byte each in three named registers (two 64-bit words and one more), ranked by counting -- a candidate
//            in a register against the others named by constants --, which gives j*; along the chain of j* for the position of r;
//            and for the acceptance against r and the sums, the first four channels while the walk decides, every further four
//            in a walk of their own.  What exists is two counts, what is accepted a bit mask in one register.  No array is
//            indexed by a register: nothing in scratch, no LDS.
// Entry points defined here: lp_tsmooth, lp_tsmooth_robust.
#include "motion_tile.h"

namespace lp {
namespace {

constexpr int kB = LP_PROP_BLOCK;                                                     // 8
constexpr int kTile = kFieldTile;                                                    // 32
constexpr int kWave = 64;                                                            // two rows of a tile

struct smooth_args {
    const int32_t* fwd;          // row j: the field of frame fwd0 + j towards the next frame, [gh, gw, 2]
    const int32_t* bwd;          // row j: of frame bwd0 + j towards the one before
    const uint8_t* known;        // frame `first`'s bits [H, W]; the next frame's lie known_stride bytes on
    int64_t        known_stride;
    const float*   images;       // [frames, H, W, C]
    float*         out;
    int32_t*       support;      // [frames, H, W]
    int32_t H, W, C, gh, gw, frames, first, fwd0, bwd0, radius, tolerance, w0;
};

__device__ __forceinline__ void own4(const float* __restrict__ x, int C, int c0, float (&v)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = c0 + k < C ? x[c0 + k] : 0.0f;
}

// the largest |code(s) - code(x)| over the group; channels beyond C are 0 on both sides
__device__ __forceinline__ int apart4(const float (&s)[4], const float (&x)[4]) {
    int m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) m = max(m, abs(code_of(s[k]) - code_of(x[k])));
    return m;
}

// One step from p (inside the plane) along `vec`: the propagate section's per-pixel interpolation at the integer pixel nearest p.
// False: q leaves the plane.
__device__ __forceinline__ bool step(const smooth_args& a, const int32_t* __restrict__ vec, int py, int px, int& qy, int& qx) {
    const field_tap by = field_tap_of((py + 8) >> 4, a.gh), bx = field_tap_of((px + 8) >> 4, a.gw);
    const int2 v00 = *reinterpret_cast<const int2*>(vec + (static_cast<int64_t>(by.b0) * a.gw + bx.b0) * 2);
    const int2 v01 = *reinterpret_cast<const int2*>(vec + (static_cast<int64_t>(by.b0) * a.gw + bx.b1) * 2);
    const int2 v10 = *reinterpret_cast<const int2*>(vec + (static_cast<int64_t>(by.b1) * a.gw + bx.b0) * 2);
    const int2 v11 = *reinterpret_cast<const int2*>(vec + (static_cast<int64_t>(by.b1) * a.gw + bx.b1) * 2);
    qy = py + field_vector(v00.x, v01.x, v10.x, v11.x, by.f, bx.f);
    qx = px + field_vector(v00.y, v01.y, v10.y, v11.y, by.f, bx.f);
    return qy >= 0 && qy <= 16 * (a.H - 1) && qx >= 0 && qx <= 16 * (a.W - 1);
}

// The chain of direction d from pixel (y, x) of frame t, for the channels c0 .. c0 + 3 with their own values x4.
// Decide: at most `limit` = R steps; the chain ends at the clip's end, where q leaves the plane or at the first sample some channel
// of which is more than `tolerance` codes away from the pixel; W gathers the accepted weights.  Else: exactly `limit` steps, those
// an earlier deciding walk accepted.  Returns the steps accepted.
template <bool Decide>
__device__ __forceinline__ int chain(const smooth_args& a, int t, int d, int limit, int y, int x, const float* __restrict__ own, int c0,
                                     const float (&x4)[4], float (&acc)[4], int& W) {
    const int64_t field = static_cast<int64_t>(a.gh) * a.gw * 2;
    int py = 16 * y, px = 16 * x, w = a.w0, n = 0;
#pragma unroll 1
    for (int k = 1; k <= limit; ++k) {
        const int u = t + (k - 1) * d, v = u + d;
        if (Decide && (v < 0 || v >= a.frames)) break;
        const int32_t* vec = d > 0 ? a.fwd + (u - a.fwd0) * field : a.bwd + (u - a.bwd0) * field;
        int qy, qx;
        const bool inside = step(a, vec, py, px, qy, qx);
        if (Decide && !inside) break;
        const tap_rows taps = taps_of(a.images, a.H, a.W, a.C, v, qy, qx);
        float s[4];
        sample4(taps, a.C, c0, s);
        if (Decide) {
            int apart = apart4(s, x4);
#pragma unroll 1
            for (int c = 4; c < a.C && apart <= a.tolerance; c += 4) {  // the further groups: compared here, accumulated later
                float sc[4], xc[4];
                sample4(taps, a.C, c, sc);
                own4(own, a.C, c, xc);
                apart = max(apart, apart4(sc, xc));
            }
            if (apart > a.tolerance) break;
        }
        w = w * (a.radius - k + 1) / (a.radius + k);                     // C(2R, R + k) from C(2R, R + k - 1): the division is exact
        const float wf = static_cast<float>(w);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __fadd_rn(acc[j], __fmul_rn(wf, __fsub_rn(s[j], x4[j])));
        if (Decide) W += w;
        py = qy;
        px = qx;
        ++n;
    }
    return n;
}

// `rows` runs of `run` elements, `pitch` elements apart, by one wave: consecutive lanes take consecutive elements of a run, and two
// loads are asked for before the first store.
template <typename T>
__device__ __forceinline__ void copy_rows(const T* __restrict__ src, T* __restrict__ dst, int rows, int run, int64_t pitch, int lane) {
    const int total = rows * run;
#pragma unroll 1
    for (int i0 = lane; i0 < total; i0 += 2 * kWave) {
        const int i1 = min(i0 + kWave, total - 1);                       // past the end: the last element again, not stored
        const int r0 = i0 / run, r1 = i1 / run;
        const T v0 = src[r0 * pitch + (i0 - r0 * run)], v1 = src[r1 * pitch + (i1 - r1 * run)];
        dst[r0 * pitch + (i0 - r0 * run)] = v0;
        if (i0 + kWave < total) dst[r1 * pitch + (i1 - r1 * run)] = v1;
    }
}

// The geometry of both kernels and their copy of what is not masked: the lane's pixel (y, x) of frame t, element `at` of a plane
// stack.  A wave -- two rows of the tile -- in which none is masked copies its two runs and leaves; else a known pixel is copied by
// its lane.  Both write support = -1, and `replaced` = -1 where the robust form passes its plane (the plain form: null).
// True: the pixel is masked and the lane goes on; false: the lane is done.
__device__ __forceinline__ bool masked_pixel(const smooth_args& a, int32_t* __restrict__ replaced, int& y, int& x, int& t, int64_t& at) {
    const int H = a.H, W = a.W, C = a.C;
    const int ly = threadIdx.x >> 5, lx = threadIdx.x & 31;
    y = blockIdx.y * kTile + ly;
    x = blockIdx.x * kTile + lx;
    t = a.first + static_cast<int>(blockIdx.z);
    const int64_t p = static_cast<int64_t>(y) * W + x;
    const bool inside = y < H && x < W;
    const bool masked = inside && a.known[static_cast<int64_t>(blockIdx.z) * a.known_stride + p] == 0;
    at = static_cast<int64_t>(t) * H * W + p;
    if (__all(!masked)) {                                                // the whole wave, two rows of the tile: nothing under a mask here
        if (inside) {
            a.support[at] = -1;
            if (replaced) replaced[at] = -1;
        }
        const int y0 = static_cast<int>(blockIdx.y) * kTile + (ly & ~1);
        if (y0 >= H) return false;
        const int tw = min(kTile, W - static_cast<int>(blockIdx.x) * kTile), rows = min(2, H - y0), lane = threadIdx.x & (kWave - 1);
        const int64_t pitch = static_cast<int64_t>(W) * C;               // floats from a row to the next
        const int64_t corner = ((static_cast<int64_t>(t) * H + y0) * W + static_cast<int64_t>(blockIdx.x) * kTile) * C;
        // 16 bytes a lane where both rows start and end on them: the tile's first column is a multiple of 32 pixels
        if (((pitch | (tw * C)) & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.images) | reinterpret_cast<uintptr_t>(a.out)) & 15) == 0)
            copy_rows(reinterpret_cast<const float4*>(a.images + corner), reinterpret_cast<float4*>(a.out + corner), rows, tw * C / 4, pitch / 4, lane);
        else
            copy_rows(a.images + corner, a.out + corner, rows, tw * C, pitch, lane);
        return false;
    }
    if (!inside) return false;
    if (!masked) {
        const float* __restrict__ own = a.images + at * C;
        float* __restrict__ out = a.out + at * C;
#pragma unroll 1
        for (int c = 0; c < C; ++c) out[c] = own[c];
        a.support[at] = -1;
        if (replaced) replaced[at] = -1;
        return false;
    }
    return true;
}

// One lane per pixel, as the temporal fill's carry has it: a masked pixel's work is a chain of dependent reads.
__global__ __launch_bounds__(kTile * kTile) void lp_tsmooth_kernel(const smooth_args a) {
    const int C = a.C;
    int y, x, t;
    int64_t at;
    if (!masked_pixel(a, nullptr, y, x, t, at)) return;
    const float* __restrict__ own = a.images + at * C;
    float* __restrict__ out = a.out + at * C;
    float x4[4], acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    own4(own, C, 0, x4);
    int Wsum = a.w0;
    const int n_past = chain<true>(a, t, -1, a.radius, y, x, own, 0, x4, acc, Wsum);
    const int n_next = chain<true>(a, t, +1, a.radius, y, x, own, 0, x4, acc, Wsum);
    const int n = n_past + n_next;
    a.support[at] = n;
    const float Wf = static_cast<float>(Wsum);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < C) out[j] = n ? __fadd_rn(x4[j], __fdiv_rn(acc[j], Wf)) : x4[j];
#pragma unroll 1
    for (int c0 = 4; c0 < C; c0 += 4) {
        float xc[4], ac[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        own4(own, C, c0, xc);
        int unused = 0;
        chain<false>(a, t, -1, n_past, y, x, own, c0, xc, ac, unused);
        chain<false>(a, t, +1, n_next, y, x, own, c0, xc, ac, unused);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < C) out[c0 + j] = n ? __fadd_rn(xc[j], __fdiv_rn(ac[j], Wf)) : xc[j];
    }
}

// ---- the robust form (lp_tsmooth_robust): the reference is the temporal median of the samples along the motion ----------------------
constexpr int kSlots = 2 * LP_TSMOOTH_MAX_RADIUS + 1;                                // order indices o = 0 .. 16

// One step of direction d on from p, step k of the walk from frame t: false where the chain ends (the clip's end, or q leaves the
// plane); else p moves on to q.  The fields alone decide.
__device__ __forceinline__ bool advance(const smooth_args& a, int t, int d, int k, int& py, int& px) {
    const int u = t + (k - 1) * d, v = u + d;
    if (v < 0 || v >= a.frames) return false;
    const int64_t field = static_cast<int64_t>(a.gh) * a.gw * 2;
    int qy, qx;
    if (!step(a, d > 0 ? a.fwd + (u - a.fwd0) * field : a.bwd + (u - a.bwd0) * field, py, px, qy, qx)) return false;
    py = qy;
    px = qx;
    return true;
}

// The lumas of the order indices, a byte each: 0..7 in `lo`, 8..15 in `hi`, 16 in `top`.  Three named registers and no array, so
// that an index in a register selects and shifts and nothing goes to scratch.
struct lumas17 {
    uint64_t lo, hi;
    uint32_t top;
};

__device__ __forceinline__ void put_luma(lumas17& pk, int o, int Y) {
    const uint64_t b = static_cast<uint64_t>(Y) << ((o & 7) * 8);
    pk.lo |= o < 8 ? b : 0;
    pk.hi |= o >= 8 && o < 16 ? b : 0;
    pk.top = o == 16 ? static_cast<uint32_t>(Y) : pk.top;
}

__device__ __forceinline__ int get_luma(const lumas17& pk, int o) {
    const uint64_t word = o < 8 ? pk.lo : pk.hi;
    return o == 16 ? static_cast<int>(pk.top) : static_cast<int>((word >> ((o & 7) * 8)) & 255u);
}

// The first walk: the lumas of the steps that exist in direction d go to the bytes o0 + 1 ..; returns how many exist.
__device__ __forceinline__ int lumas(const smooth_args& a, int t, int d, int o0, int y, int x, lumas17& pk) {
    int py = 16 * y, px = 16 * x, n = 0;
#pragma unroll 1
    for (int k = 1; k <= a.radius; ++k) {
        if (!advance(a, t, d, k, py, px)) break;
        float s[4];
        sample4(taps_of(a.images, a.H, a.W, a.C, t + k * d, py, px), a.C, 0, s);
        put_luma(pk, o0 + k, luma_of(s, a.C));
        ++n;
    }
    return n;
}

// how many of the existing keys Y_j * 32 + j, j = J .. J + 7, of a word lie in front of `key`
template <int J>
__device__ __forceinline__ int in_front(uint64_t word, uint32_t exist, int key) {
    int before = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int other = (static_cast<int>((word >> (8 * b)) & 255u) << 5) | (J + b);
        before += (other < key ? 1 : 0) & static_cast<int>((exist >> (J + b)) & 1u);
    }
    return before;
}

// The lower median of the existing o by (Y_o, o): the one with exactly (n - 1) >> 1 others in front of it.  The keys Y_o * 32 + o
// are all different.  The candidates run over a register, the others over constants; with R < 4 `hi` and `top` hold nothing.
__device__ __forceinline__ int median_of(const lumas17& pk, uint32_t exist, int n, int radius) {
    const int want = (n - 1) >> 1;
    int found = 0;
#pragma unroll 1
    for (int i = 0; i <= 2 * radius; ++i) {
        const int key = (get_luma(pk, i) << 5) | i;
        int before = in_front<0>(pk.lo, exist, key);
        if (radius >= 4) {
            before += in_front<8>(pk.hi, exist, key);
            before += (((static_cast<int>(pk.top) << 5) | (kSlots - 1)) < key ? 1 : 0) & static_cast<int>((exist >> (kSlots - 1)) & 1u);
        }
        found = ((exist >> i) & 1u) && before == want ? i : found;
    }
    return found;
}

// Where r is: the own pixel (v < 0) or a position in frame v
struct ref_at {
    int v, qy, qx;
};

__device__ __forceinline__ void ref4(const smooth_args& a, const ref_at& r, const float* __restrict__ own, int c0, float (&v)[4]) {
    if (r.v < 0)
        own4(own, a.C, c0, v);
    else
        sample4(taps_of(a.images, a.H, a.W, a.C, r.v, r.qy, r.qx), a.C, c0, v);
}

// The chain of direction d again, all `steps` of it that exist, for the channels c0 .. c0 + 3: the sums of the accepted samples
// about `base` (x or r of these channels), the sample `skip` left out of the sum (j* where r overrules the pixel; -1 else).
// Decide (c0 = 0): a sample is accepted where no channel's code is more than `tolerance` from r's (r4: its first four channels);
// its bit goes into `accepted` and its weight into W.  Else the bits decide.
template <bool Decide>
__device__ __forceinline__ void robust_chain(const smooth_args& a, int t, int d, int steps, int o0, int y, int x, const float* __restrict__ own,
                                             int c0, const float (&base)[4], const float (&r4)[4], const ref_at& r, int skip,
                                             float (&acc)[4], int& W, uint32_t& accepted) {
    int py = 16 * y, px = 16 * x, w = a.w0;
#pragma unroll 1
    for (int k = 1; k <= steps; ++k) {
        advance(a, t, d, k, py, px);                                     // exists: the first walk came this far
        const tap_rows taps = taps_of(a.images, a.H, a.W, a.C, t + k * d, py, px);
        float s[4];
        sample4(taps, a.C, c0, s);
        w = w * (a.radius - k + 1) / (a.radius + k);
        const int o = o0 + k;
        bool ok;
        if (Decide) {
            int apart = apart4(s, r4);
#pragma unroll 1
            for (int c = 4; c < a.C && apart <= a.tolerance; c += 4) {
                float sc[4], rc[4];
                sample4(taps, a.C, c, sc);
                ref4(a, r, own, c, rc);
                apart = max(apart, apart4(sc, rc));
            }
            ok = apart <= a.tolerance;
            if (ok) {
                accepted |= 1u << o;
                W += w;
            }
        } else {
            ok = (accepted >> o) & 1u;
        }
        if (ok && o != skip) {
            const float wf = static_cast<float>(w);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __fadd_rn(acc[j], __fmul_rn(wf, __fsub_rn(s[j], base[j])));
        }
    }
}

struct robust_args {
    smooth_args s;
    int32_t*    replaced;        // [frames, H, W]
};

// The plain kernel's geometry and its copy of what is not masked; a masked pixel ranks its lumas and walks again.
__global__ __launch_bounds__(kTile * kTile) void lp_tsmooth_robust_kernel(const robust_args ra) {
    const smooth_args& a = ra.s;
    const int C = a.C, R = a.radius;
    int y, x, t;
    int64_t at;
    if (!masked_pixel(a, ra.replaced, y, x, t, at)) return;
    const float* __restrict__ own = a.images + at * C;
    float* __restrict__ out = a.out + at * C;
    // the first walk: the lumas
    float x4[4];
    own4(own, C, 0, x4);
    lumas17 pk = {static_cast<uint64_t>(luma_of(x4, C)), 0, 0};
    const int n_past = lumas(a, t, -1, 0, y, x, pk), n_next = lumas(a, t, +1, R, y, x, pk);
    const int n = 1 + n_past + n_next;
    const uint32_t exist = 1u | (((1u << n_past) - 1u) << 1) | (((1u << n_next) - 1u) << (R + 1));
    const int js = n < 3 ? 0 : median_of(pk, exist, n, R);
    // the second walk: to j*
    ref_at r = {-1, 0, 0};
    if (js) {
        const int d = js <= R ? -1 : +1, steps = js <= R ? js : js - R;
        r.qy = 16 * y;
        r.qx = 16 * x;
#pragma unroll 1
        for (int k = 1; k <= steps; ++k) advance(a, t, d, k, r.qy, r.qx);
        r.v = t + steps * d;
    }
    float r4[4];
    ref4(a, r, own, 0, r4);
    int apart = apart4(x4, r4);
#pragma unroll 1
    for (int c = 4; c < C && apart <= a.tolerance; c += 4) {
        float xc[4], rc[4];
        own4(own, C, c, xc);
        ref4(a, r, own, c, rc);
        apart = max(apart, apart4(xc, rc));
    }
    const bool own_ok = apart <= a.tolerance;                            // with j* = 0 always
    // the third walk: what is accepted, and the first four channels' sums about x, or about r where r may overrule the pixel
    const int skip = own_ok ? -1 : js;
    uint32_t accepted = 0;
    int Wsum = own_ok ? a.w0 : 0;
    float base[4], acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j) base[j] = own_ok ? x4[j] : r4[j];
    robust_chain<true>(a, t, -1, n_past, 0, y, x, own, 0, base, r4, r, skip, acc, Wsum, accepted);
    robust_chain<true>(a, t, +1, n_next, R, y, x, own, 0, base, r4, r, skip, acc, Wsum, accepted);
    const int count = __popc(accepted);
    const bool moved = own_ok ? count > 0 : count >= LP_TSMOOTH_ROBUST_QUORUM;
    a.support[at] = moved ? count : 0;
    ra.replaced[at] = !own_ok && moved ? 1 : 0;
    const float Wf = static_cast<float>(Wsum);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < C) out[j] = moved ? __fadd_rn(base[j], __fdiv_rn(acc[j], Wf)) : x4[j];
#pragma unroll 1
    for (int c0 = 4; c0 < C; c0 += 4) {
        float xc[4], bc[4], ac[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        own4(own, C, c0, xc);
        ref4(a, r, own, c0, bc);
#pragma unroll
        for (int j = 0; j < 4; ++j) bc[j] = own_ok ? xc[j] : bc[j];
        if (moved) {
            int unused = 0;
            robust_chain<false>(a, t, -1, n_past, 0, y, x, own, c0, bc, bc, r, skip, ac, unused, accepted);
            robust_chain<false>(a, t, +1, n_next, R, y, x, own, c0, bc, bc, r, skip, ac, unused, accepted);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < C) out[c0 + j] = moved ? __fadd_rn(bc[j], __fdiv_rn(ac[j], Wf)) : xc[j];
    }
}

// The checks both entries share, and the kernel's arguments; `extra` is the robust form's third output (null: the plain form)
int smooth_args_of(const lp_tsmooth_desc& d, const void* extra, smooth_args& a) {
    if (d.frames < 1 || !side_ok(d.height) || !side_ok(d.width) || d.channels < 1 || d.channels > LP_DETAIL_MAX_CHANNELS) return LP_E_INVALID;
    if (d.radius < 1 || d.radius > LP_TSMOOTH_MAX_RADIUS || d.tolerance < 0 || d.tolerance > 255) return LP_E_INVALID;
    if (d.frames > 65535) return LP_E_UNSUPPORTED;
    if (d.first < 0 || d.count < 1 || d.count > d.frames - d.first) return LP_E_INVALID;
    if (!d.known || !d.images || !d.out || !d.support) return LP_E_INVALID;
    const int64_t plane = static_cast<int64_t>(d.height) * d.width;
    if (d.known_stride < plane && d.count > 1) return LP_E_INVALID;
    // the frames whose fields the walks of first .. first + count - 1 can read
    const int last = d.first + d.count - 1;
    const int f_lo = d.first, f_hi = min(last + d.radius - 1, d.frames - 2);             // towards the next frame
    const int b_lo = max(d.first - d.radius + 1, 1), b_hi = last;                        // towards the one before
    if (f_lo <= f_hi && (!d.fwd || d.fwd_first < 0 || d.fwd_count < 1 || d.fwd_first > f_lo || f_hi - d.fwd_first >= d.fwd_count)) return LP_E_INVALID;
    if (b_lo <= b_hi && (!d.bwd || d.bwd_first < 0 || d.bwd_count < 1 || d.bwd_first > b_lo || b_hi - d.bwd_first >= d.bwd_count)) return LP_E_INVALID;
    const void* in[4] = {d.fwd, d.bwd, d.known, d.images};
    for (const void* q : in)
        if (q && (q == d.out || q == d.support)) return LP_E_INVALID;
    if (static_cast<const void*>(d.out) == static_cast<const void*>(d.support)) return LP_E_INVALID;
    for (const void* q : in)
        if (q && q == extra) return LP_E_INVALID;
    if (extra && (extra == static_cast<const void*>(d.out) || extra == static_cast<const void*>(d.support))) return LP_E_INVALID;
    a.fwd = d.fwd;
    a.bwd = d.bwd;
    a.known = d.known;
    a.known_stride = d.known_stride;
    a.images = d.images;
    a.out = d.out;
    a.support = d.support;
    a.H = d.height;
    a.W = d.width;
    a.C = d.channels;
    a.gh = (d.height + kB - 1) / kB;
    a.gw = (d.width + kB - 1) / kB;
    a.frames = d.frames;
    a.first = d.first;
    a.fwd0 = d.fwd_first;
    a.bwd0 = d.bwd_first;
    a.radius = d.radius;
    a.tolerance = d.tolerance;
    a.w0 = 1;
    for (int k = 1; k <= d.radius; ++k) a.w0 = a.w0 * (d.radius + k) / k;                // C(2R, R): C(R + k, k) at every step
    return LP_OK;
}

}  // namespace

extern "C" int lp_tsmooth(const lp_tsmooth_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    smooth_args a = {};
    const int status = smooth_args_of(*dp, nullptr, a);
    if (status != LP_OK) return status;
    const dim3 grid(blocks_of(dp->width, kTile), blocks_of(dp->height, kTile), static_cast<uint32_t>(dp->count));
    hipLaunchKernelGGL(lp_tsmooth_kernel, grid, dim3(kTile * kTile), 0, stream, a);
    return launched();
}

extern "C" int lp_tsmooth_robust(const lp_tsmooth_robust_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    if (!dp->replaced) return LP_E_INVALID;
    const lp_tsmooth_desc d = {dp->frames, dp->height, dp->width, dp->channels, dp->first, dp->count, dp->radius, dp->tolerance,
                               dp->fwd_first, dp->fwd_count, dp->bwd_first, dp->bwd_count, dp->fwd, dp->bwd, dp->known, dp->known_stride,
                               dp->images, dp->out, dp->support};
    robust_args ra = {};
    const int status = smooth_args_of(d, dp->replaced, ra.s);
    if (status != LP_OK) return status;
    ra.replaced = dp->replaced;
    const dim3 grid(blocks_of(d.width, kTile), blocks_of(d.height, kTile), static_cast<uint32_t>(d.count));
    hipLaunchKernelGGL(lp_tsmooth_robust_kernel, grid, dim3(kTile * kTile), 0, stream, ra);
    return launched();
}

}  // namespace lp
