// shot_kernel.hip -- video shot detect for gfx950 (lanpaint_amd/shots.py): two integer scores per pair of neighbouring frames and
// the decision that turns them into a shot index per frame.  include/lanpaint_hip.h (lp_shot_*) states the rule.  The planes are
// a level of the luma pyramids lp_prop_luma builds; this file holds the measurement and the decision.
//
//   measure  one launch for all frames of a chunk: a 256-lane block per 32 x 32 tile and frame.  A lane packs four pixels of the
//            tile into a dword (0 outside the plane, with a per-byte mask beside it, as the propagate's matcher has it) and adds
//            them into its wave's 64-bin histogram in LDS; the four are folded once per block, at most one integer atomic per
//            bin.  If the next frame is in the chunk, its (32 + 2R)^2 window, read with clamped coordinates, goes to LDS rows of
//            40 bytes, and the tile's sixteen 8 x 8 blocks are matched, one per wave and round: lane c takes displacement c of
//            the (2R + 1)^2 <= 49, per block row and dword v_alignbyte_b32 cuts the four target pixels out of two window dwords,
//            the AND with the mask drops what lies outside the plane, v_sad_u8 adds the four absolute differences; a butterfly
//            of minima gives the block's residual.  A block outside the plane is skipped by its whole wave.  The tile's sum
//            leaves as one 64-bit integer atomic.
//   fold     a wave per pair: |h_t[k] - h_{t+1}[k]| on lane k, summed across the wave, into B.
//   decide   one block.  Lanes stride over the pairs; a pair that passes the two absolute conditions looks at its up to 2 window
//            neighbours.  The cut bits of 64 consecutive pairs are one ballot word in LDS; the words' counts are scanned (four
//            words a lane, then the lanes' sums), and shot[f] is a word's prefix plus the count of the bits up to pair f - 1.
// Integers only: the atomics are integer adds, any order gives the same bits.  No scratch, no floating point.
// Entry points defined here: lp_shot_measure, lp_shot_decide.
#include "motion_tile.h"

namespace lp {
namespace {

constexpr int kB = LP_PROP_BLOCK;                                                     // 8
constexpr int kTile = 32;
constexpr int kBins = LP_SHOT_BINS;                                                   // 64: one per lane of the folding wave
constexpr int kPatRows = kTile + 2 * LP_SHOT_MAX_SEARCH;                              // 38
constexpr int kPatPitch = 10;                                                         // dwords per window row: 40 bytes >= 38
constexpr int kMaxWords = 1024;                                                       // 65534 pairs in ballot words

static_assert(kBins == kWave && kTile % kB == 0, "a lane per bin, whole blocks per tile");
static_assert((kTile - kB + 2 * LP_SHOT_MAX_SEARCH) / 4 + 2 < kPatPitch, "a block row's two dwords and the one behind them lie inside a window row");
static_assert((2 * LP_SHOT_MAX_SEARCH + 1) * (2 * LP_SHOT_MAX_SEARCH + 1) <= kWave, "the displacements fit the lanes of a wave");

struct measure_args {
    const uint8_t* plane;        // frame 0's plane [h, w]; the next frame's lies `stride` bytes on
    int64_t        stride;
    int32_t*       hist;         // [frames, 64], cleared
    int64_t*       score;        // [frames - 1, 2], cleared
    int32_t h, w, frames, search;
};

__global__ __launch_bounds__(256) void lp_shot_measure_kernel(const measure_args a) {
    __shared__ uint32_t s_src[kTile * 8], s_bm[kTile * 8], s_pat[kPatRows * kPatPitch];
    __shared__ uint32_t s_hist[4][kBins];
    __shared__ uint32_t s_A[4];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
    const int t = blockIdx.z, ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
    const uint8_t* __restrict__ Yt = a.plane + static_cast<int64_t>(t) * a.stride;
    const bool pair = t + 1 < a.frames;                                  // uniform: the chunk's last frame has a histogram only
    s_hist[wv][lane] = 0;
    __syncthreads();
    {                                                                    // the tile: lane = row * 8 + dword
        const int y = ty0 + (tid >> 3);
        uint32_t sv = 0, bm = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = tx0 + (tid & 7) * 4 + k;
            if (y < a.h && x < a.w) {
                const uint32_t v = Yt[static_cast<int64_t>(y) * a.w + x];
                sv |= v << (8 * k);
                bm |= 0xFFu << (8 * k);
                atomicAdd(&s_hist[wv][v >> 2], 1u);
            }
        }
        s_src[tid] = sv;
        s_bm[tid] = bm;
    }
    uint32_t sum = 0;
    if (pair) {
        // the window of t + 1: row j, byte i is Y(clamp(ty0 - R + j), clamp(tx0 - R + i))
        const int R = a.search, rows = kTile + 2 * R;
        const uint8_t* __restrict__ Yn = Yt + a.stride;
        for (int i = tid; i < rows * kPatPitch; i += 256) {
            const int j = i / kPatPitch, c0 = (i - j * kPatPitch) * 4;
            const uint8_t* row = Yn + static_cast<int64_t>(clampi(ty0 - R + j, 0, a.h - 1)) * a.w;
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v |= static_cast<uint32_t>(row[clampi(tx0 - R + c0 + k, 0, a.w - 1)]) << (8 * k);
            s_pat[i] = v;
        }
        __syncthreads();
        const int n = 2 * R + 1, cy = lane / n, cx = lane - cy * n;     // lane = (dy + R) n + dx + R
        const bool cand = lane < n * n;
#pragma unroll 1
        for (int round = 0; round < 4; ++round) {
            const int blk = round * 4 + wv, bly = blk >> 2, blx = blk & 3;
            if (ty0 + bly * kB >= a.h || tx0 + blx * kB >= a.w) continue;    // the whole wave: no pixel of this block in the plane
            uint32_t S = 0xFFFFFFFFu;
            if (cand) {
                const int o = blx * kB + cx, word = o >> 2, shift = o & 3;  // word + 2 <= 9: inside the window row
                S = 0;
#pragma unroll
                for (int r = 0; r < kB; ++r) {
                    const uint32_t* pr = s_pat + (bly * kB + r + cy) * kPatPitch + word;
                    const int q = (bly * kB + r) * 8 + blx * 2;
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const uint32_t tg = __builtin_amdgcn_alignbyte(pr[k + 1], pr[k], shift) & s_bm[q + k];
                        S = __builtin_amdgcn_sad_u8(s_src[q + k], tg, S);
                    }
                }
            }
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) S = min(S, static_cast<uint32_t>(__shfl_xor(static_cast<int>(S), d, kWave)));
            sum += S;                                                    // <= 64 * 255 a block
        }
    }
    if (lane == 0) s_A[wv] = sum;
    __syncthreads();
    if (tid < kBins) {
        const uint32_t c = s_hist[0][tid] + s_hist[1][tid] + s_hist[2][tid] + s_hist[3][tid];
        if (c) atomicAdd(a.hist + static_cast<int64_t>(t) * kBins + tid, static_cast<int32_t>(c));
    }
    if (tid == 0 && pair) {
        const uint32_t total = s_A[0] + s_A[1] + s_A[2] + s_A[3];
        if (total) atomicAdd(reinterpret_cast<unsigned long long*>(a.score + 2 * static_cast<int64_t>(t)), static_cast<unsigned long long>(total));
    }
}

// B[t] of the pair blockIdx.x: a lane per bin
__global__ __launch_bounds__(kWave) void lp_shot_fold_kernel(const int32_t* __restrict__ hist, int64_t* __restrict__ score) {
    const int64_t t = blockIdx.x;
    int d = abs(hist[t * kBins + threadIdx.x] - hist[(t + 1) * kBins + threadIdx.x]);
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) d += __shfl_xor(d, s, kWave);    // <= 2 N <= 2^29
    if (threadIdx.x == 0) score[2 * t + 1] = d;
}

struct decide_args {
    const int64_t* score;        // [frames - 1, 2]
    int32_t*       shot;         // [frames]
    int64_t        n;            // N
    int32_t frames, threshold, hist, ratio, window;
};

__global__ __launch_bounds__(256) void lp_shot_decide_kernel(const decide_args a) {
    __shared__ unsigned long long s_bits[kMaxWords];
    __shared__ uint32_t s_pref[kMaxWords], s_sum[256];
    const int tid = threadIdx.x, pairs = a.frames - 1, words = (pairs + kWave - 1) / kWave;
    for (int base = 0; base < words * kWave; base += 256) {              // uniform: every lane takes part in the ballot
        const int t = base + tid;
        bool cut = false;
        if (t < pairs) {
            const int64_t A = a.score[2 * static_cast<int64_t>(t)], B = a.score[2 * static_cast<int64_t>(t) + 1];
            cut = A >= a.threshold * a.n && 100 * B >= a.hist * (2 * a.n);
            if (cut) {
                const int lo = max(t - a.window, 0), hi = min(t + a.window, pairs - 1);
                for (int u = lo; u <= hi; ++u)
                    cut = cut && (u == t || 100 * A >= a.ratio * a.score[2 * static_cast<int64_t>(u)]);
            }
        }
        const unsigned long long m = __ballot(cut);
        if ((tid & (kWave - 1)) == 0) s_bits[t >> 6] = m;                // t >> 6 < 1024; a word past `words` is never read
    }
    __syncthreads();
    uint32_t own = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                        // words 4 tid .. 4 tid + 3: their counts in front of them
        const int i = 4 * tid + j;
        s_pref[i] = own;
        if (i < words) own += static_cast<uint32_t>(__popcll(s_bits[i]));
    }
    s_sum[tid] = own;
    __syncthreads();
    uint32_t before = 0;
    for (int i = 0; i < tid; ++i) before += s_sum[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) s_pref[4 * tid + j] += before;
    __syncthreads();
    for (int f = tid; f < a.frames; f += 256) {
        int32_t v = 0;
        if (f > 0) {                                                     // the inclusive scan at pair f - 1
            const int t = f - 1;
            v = static_cast<int32_t>(s_pref[t >> 6]) + __popcll(s_bits[t >> 6] & (~0ull >> (63 - (t & 63))));
        }
        a.shot[f] = v;
    }
}

}  // namespace

extern "C" int lp_shot_measure(const lp_shot_measure_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_shot_measure_desc& d = *dp;
    if (d.frames < 1 || !side_ok(d.height) || !side_ok(d.width) || d.search < 1 || d.search > LP_SHOT_MAX_SEARCH) return LP_E_INVALID;
    if (d.frames > 65535) return LP_E_UNSUPPORTED;
    if (!d.plane || !d.hist || (!d.score && d.frames > 1)) return LP_E_INVALID;
    if (d.frames > 1 && d.stride < static_cast<int64_t>(d.height) * d.width) return LP_E_INVALID;
    if (static_cast<const void*>(d.hist) == static_cast<const void*>(d.plane) || static_cast<const void*>(d.hist) == static_cast<const void*>(d.score) ||
        static_cast<const void*>(d.score) == static_cast<const void*>(d.plane))
        return LP_E_INVALID;
    if (hipMemsetAsync(d.hist, 0, sizeof(int32_t) * kBins * static_cast<size_t>(d.frames), stream) != hipSuccess) return LP_E_LAUNCH;
    if (d.frames > 1 && hipMemsetAsync(d.score, 0, sizeof(int64_t) * 2 * static_cast<size_t>(d.frames - 1), stream) != hipSuccess) return LP_E_LAUNCH;
    measure_args a = {};
    a.plane = d.plane;
    a.stride = d.stride;
    a.hist = d.hist;
    a.score = d.score;
    a.h = d.height;
    a.w = d.width;
    a.frames = d.frames;
    a.search = d.search;
    const dim3 grid(blocks_of(d.width, kTile), blocks_of(d.height, kTile), static_cast<uint32_t>(d.frames));
    hipLaunchKernelGGL(lp_shot_measure_kernel, grid, dim3(256), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    if (d.frames > 1) hipLaunchKernelGGL(lp_shot_fold_kernel, dim3(static_cast<uint32_t>(d.frames - 1)), dim3(kWave), 0, stream, d.hist, d.score);
    return launched();
}

extern "C" int lp_shot_decide(const lp_shot_decide_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_shot_decide_desc& d = *dp;
    if (d.frames < 1) return LP_E_INVALID;
    if (d.threshold < 1 || d.threshold > 255 || d.hist < 0 || d.hist > 100 || d.ratio < 100 || d.ratio > 10000 || d.window < 1 ||
        d.window > LP_SHOT_MAX_WINDOW || d.n_pixels < 1 || d.n_pixels > (static_cast<int64_t>(1) << 28))
        return LP_E_INVALID;
    if (d.frames > 65535) return LP_E_UNSUPPORTED;
    if (!d.shot || (!d.score && d.frames > 1)) return LP_E_INVALID;
    if (static_cast<const void*>(d.shot) == static_cast<const void*>(d.score)) return LP_E_INVALID;
    decide_args a = {};
    a.score = d.score;
    a.shot = d.shot;
    a.n = d.n_pixels;
    a.frames = d.frames;
    a.threshold = d.threshold;
    a.hist = d.hist;
    a.ratio = d.ratio;
    a.window = d.window;
    hipLaunchKernelGGL(lp_shot_decide_kernel, dim3(1), dim3(256), 0, stream, a);
    return launched();
}

}  // namespace lp
