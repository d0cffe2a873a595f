// stabilize_kernel.hip -- video mask stabilize for gfx950 (lanpaint_amd/stabilize.py): a temporal median and a binomial smoothing of
// the mask's signed distance field.  include/lanpaint_hip.h (lp_mask_stabilize) states the rule: exact integer medians of the
// signed squared distances, the fp64 square root capped at 64, a weighted sum in fp64 in a fixed order, a threshold or a ramp.
//
//   signed_d2   stage 1.  One lane per pixel and frame folds lp_vmask_edt's two int32 planes into the signed squared distance q.
//   stabilize   stages 2 to 5 in one launch.  The plane is taken as H * W pixels in a row; a block owns 256 neighbouring pixels
//               and one segment of the time axis, a lane one pixel.  The lane marches over t with the median window (2 TM + 1
//               int32) and the smoothing window (2 TS + 1 doubles) in registers: per frame one q is loaded (a wave reads 256
//               contiguous bytes; the load for the next frame is issued before this frame's arithmetic), the median window
//               moves on, one capped distance is formed and pushed into the smoothing window, one fp32 is stored.  q is read
//               once and out written once; nothing else goes through memory.  A segment that does not start at frame 0 warms
//               its windows up over the TM + TS frames in front of it and reads TM + TS past its end: the values are those the
//               rule names, so the cut cannot change a bit.
//
// The windows are indexed at compile time, so the kernel is a template on the windows' radii (TM, TS), and four instantiations
// serve every (Tm, Ts): TM in {1, 3}, TS in {2, 8}, the smallest that hold the call's radii.  A median of fewer values than the
// window holds replaces the outer slots by as many INT32_MIN as INT32_MAX, which leaves the median where it was; a smoothing of
// fewer taps gives the outer taps the weight 0.0, whose products are +-0.0 and leave the sum's bits alone (the sum starts from +0.0
// and the capped distances are finite).  Every fp64 step goes through __dmul_rn / __dadd_rn / __ddiv_rn (the library is built with
// -ffp-contract=on).  No scratch, no LDS, no atomics.
// Entry points defined here: lp_mask_signed_d2, lp_mask_stabilize.
#include "lp_common.h"

#include <math.h>

#include <algorithm>

namespace lp {
namespace {

constexpr int kBlock = 256;              // pixels per block, one per lane
constexpr int kWantBlocks = 2048;        // the time axis is cut only while the grid is smaller than this (8 blocks per CU)
constexpr int kTaps = 2 * LP_STAB_MAX_SMOOTH + 1;

struct stab_args {
    const int32_t* q;
    float*         out;
    int64_t        plane;                // H * W
    int32_t        frames, seg_len, tm, reserved0;
    double         grow, feather2, scale;    // 2 * feather; 4^-Ts
    double         w[kTaps];             // C(2 Ts, Ts + k) at [LP_STAB_MAX_SMOOTH + k], 0.0 beyond Ts
};

__device__ __forceinline__ void cmpswap(int32_t& a, int32_t& b) {
    const int32_t lo = min(a, b), hi = max(a, b);
    a = lo; b = hi;
}

// the median of the 2 tm + 1 middle slots of the window
template <int TM>
__device__ __forceinline__ int32_t window_median(const int32_t (&m)[2 * TM + 1], int tm) {
    static_assert(TM == 1 || TM == 3, "sorting networks for 3 and 7 values");
    int32_t v[2 * TM + 1];
#pragma unroll
    for (int j = 0; j <= 2 * TM; ++j) v[j] = j < TM - tm ? INT32_MIN : (j > TM + tm ? INT32_MAX : m[j]);
    if constexpr (TM == 1) {
        return max(min(v[0], v[1]), min(max(v[0], v[1]), v[2]));
    } else {                                                         // the 16-exchange network for 7 values; v[3] is read
        cmpswap(v[0], v[6]); cmpswap(v[2], v[3]); cmpswap(v[4], v[5]);
        cmpswap(v[0], v[2]); cmpswap(v[1], v[4]); cmpswap(v[3], v[6]);
        cmpswap(v[0], v[1]); cmpswap(v[2], v[5]); cmpswap(v[3], v[4]);
        cmpswap(v[1], v[2]); cmpswap(v[4], v[6]);
        cmpswap(v[2], v[3]); cmpswap(v[4], v[5]);
        cmpswap(v[1], v[2]); cmpswap(v[3], v[4]); cmpswap(v[5], v[6]);
        return v[3];
    }
}

template <int TM, int TS>
__global__ __launch_bounds__(kBlock) void lp_stabilize_kernel(const stab_args a) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (p >= a.plane) return;
    const int F = a.frames, last = F - 1;
    const int t0 = blockIdx.y * a.seg_len, t1 = t0 + min(a.seg_len, F - t0);     // this segment's output frames; t0 < F
    const int32_t* q = a.q + p;
    float* out = a.out + p;
    int32_t M[2 * TM + 1];
    double S[2 * TS + 1];
    int uc = max(t0 - TS, 0);                                        // the frame the median window is centred on
#pragma unroll
    for (int j = 0; j <= 2 * TM; ++j) M[j] = q[static_cast<int64_t>(min(max(uc + j - TM, 0), last)) * a.plane];
    int32_t q_next = q[static_cast<int64_t>(min(uc + 1 + TM, last)) * a.plane];
    double s_cur = capped_distance(window_median<TM>(M, a.tm));
#pragma unroll
    for (int j = 0; j <= 2 * TS; ++j) S[j] = 0.0;                    // every slot is pushed out before the first output
    // u runs over the frames whose capped distance enters the smoothing window: s[clamp(u, 0, F - 1)]
    for (int u = t0 - TS; u < t1 + TS; ++u) {
        const int c = min(max(u, 0), last);
        if (c != uc) {                                               // c == uc + 1: the median window moves on by one frame
#pragma unroll
            for (int j = 0; j < 2 * TM; ++j) M[j] = M[j + 1];
            M[2 * TM] = q_next;
            uc = c;
            q_next = q[static_cast<int64_t>(min(c + 1 + TM, last)) * a.plane];
            s_cur = capped_distance(window_median<TM>(M, a.tm));
        }
#pragma unroll
        for (int j = 0; j < 2 * TS; ++j) S[j] = S[j + 1];
        S[2 * TS] = s_cur;
        if (u < t0 + TS) continue;                                   // warming up
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j <= 2 * TS; ++j) acc = __dadd_rn(acc, __dmul_rn(a.w[LP_STAB_MAX_SMOOTH - TS + j], S[j]));
        const double v = __dadd_rn(__dmul_rn(acc, a.scale), a.grow);
        float o;
        if (a.feather2 == 0.0) {
            o = v > 0.0 ? 1.0f : 0.0f;
        } else {
            o = static_cast<float>(fmin(fmax(__dadd_rn(0.5, __ddiv_rn(v, a.feather2)), 0.0), 1.0));
        }
        out[static_cast<int64_t>(u - TS) * a.plane] = o;
    }
}

__global__ __launch_bounds__(kBlock) void lp_signed_d2_kernel(const int32_t* __restrict__ d2, int32_t* __restrict__ q,
                                                              int64_t plane, int frames) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (p >= plane) return;
    for (int f = blockIdx.y; f < frames; f += gridDim.y) {
        const int32_t* src = d2 + static_cast<int64_t>(f) * 2 * plane + p;
        const int32_t d_fg = src[0], d_bg = src[plane];
        q[static_cast<int64_t>(f) * plane + p] = d_fg == 0 ? (d_bg == LP_VMASK_D2_NONE ? LP_STAB_Q_FAR : d_bg)
                                                           : (d_fg == LP_VMASK_D2_NONE ? -LP_STAB_Q_FAR : -d_fg);
    }
}

bool side_ok(int s) { return s > 0 && s <= LP_VMASK_MAX_SIDE; }

template <int TM, int TS>
int launch(const stab_args& a, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((lp_stabilize_kernel<TM, TS>), grid, dim3(kBlock), 0, stream, a);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

}  // namespace

extern "C" int lp_mask_signed_d2(const int32_t* d2, int32_t frames, int32_t height, int32_t width, int32_t* q, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!d2 || !q || d2 == q || frames <= 0 || !side_ok(height) || !side_ok(width)) return LP_E_INVALID;
    const int64_t plane = static_cast<int64_t>(height) * width;
    const dim3 grid(static_cast<uint32_t>((plane + kBlock - 1) / kBlock), static_cast<uint32_t>(std::min(frames, 65535)));
    hipLaunchKernelGGL(lp_signed_d2_kernel, grid, dim3(kBlock), 0, stream, d2, q, plane, frames);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

extern "C" int lp_mask_stabilize(const lp_stabilize_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_stabilize_desc& d = *dp;
    if (d.frames <= 0 || !side_ok(d.height) || !side_ok(d.width)) return LP_E_INVALID;
    if (d.median_radius < 0 || d.median_radius > LP_STAB_MAX_MEDIAN || d.smooth_radius < 0 || d.smooth_radius > LP_STAB_MAX_SMOOTH)
        return LP_E_INVALID;
    if (!(d.grow >= -LP_STAB_MAX_GROW && d.grow <= LP_STAB_MAX_GROW)) return LP_E_INVALID;       // (a NaN fails both)
    if (!(d.feather >= 0.0 && d.feather <= LP_STAB_MAX_FEATHER)) return LP_E_INVALID;
    if (!d.q || !d.out || static_cast<const void*>(d.q) == static_cast<const void*>(d.out)) return LP_E_INVALID;
    if (d.frames > (1 << 30)) return LP_E_UNSUPPORTED;              // the frame counters stay inside an int32
    stab_args a = {};
    a.q = d.q;
    a.out = d.out;
    a.plane = static_cast<int64_t>(d.height) * d.width;
    a.frames = d.frames;
    a.tm = d.median_radius;
    a.grow = d.grow;
    a.feather2 = 2.0 * d.feather;
    const int ts = d.smooth_radius;
    a.scale = ldexp(1.0, -2 * ts);
    double c = 1.0;                                                  // C(2 ts, j), exact: at most C(16, 8) = 12870
    for (int j = 0; j <= 2 * ts; ++j) {
        a.w[LP_STAB_MAX_SMOOTH - ts + j] = c;
        c = c * (2 * ts - j) / (j + 1);
    }
    const int64_t blocks = (a.plane + kBlock - 1) / kBlock;          // at most 2^20
    const int64_t want = (kWantBlocks + blocks - 1) / blocks;        // segments that would fill the device
    a.seg_len = static_cast<int32_t>(std::max(static_cast<int64_t>(LP_STAB_SEG_FRAMES), (d.frames + want - 1) / want));
    const dim3 grid(static_cast<uint32_t>(blocks), static_cast<uint32_t>((d.frames + a.seg_len - 1) / a.seg_len));   // y <= 2048
    const bool wide_m = d.median_radius > 1, wide_s = ts > 2;
    if (wide_m) return wide_s ? launch<3, 8>(a, grid, stream) : launch<3, 2>(a, grid, stream);
    return wide_s ? launch<1, 8>(a, grid, stream) : launch<1, 2>(a, grid, stream);
}

}  // namespace lp
