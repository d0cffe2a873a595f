// audio_kernel.hip -- the audio half of the AV decode merge on gfx950 (reference nodes.py:1091-1136
// merge_audio_with_mask, run by LanPaint_AVDecode, nodes.py:1139-1227).  Two launches on the caller's stream:
//
//   lp_audio_plan_kernel   (only when cf > 1) one workgroup: the segment table of the up-sampled mask -- start[s], the first
//                          sample whose nearest-exact source is >= s -- and the fp64 prefix table P[s] = sum over the
//                          segments t < s of mask[t] * len(t).  Mask-sized (mask_len + 1 entries), not sample-sized.
//   lp_audio_merge_kernel  4 samples per lane: the weight w (one index-rule evaluation), the crossfade as a difference of the
//                          prefix function C(j) = P[seg(j)] + mask[seg(j)] * (j - start[seg(j)]) plus the two replicate-pad
//                          end terms -- O(1) per sample for any cf -- then o * (1 - w') + p * w' for every output row.
//
// The weight is piecewise constant over at most mask_len segments and src() is monotone, so the window sum of samples
// [lo, hi) is C(hi) - C(lo).  For a 0/1 mask every term is an integer and the sum exact; for soft values the difference
// carries the rounding of two whole-signal fp64 prefixes, at most (mask_len + 4) * 2^-52 * sum |w| (include/lanpaint_hip.h):
// small in absolute terms, many fp32 ulps where w' itself is tiny.  w' = float(S * double(1.0f / cf)).
// Bytes moved: 3 x 4 B per sample and row (two loads, one store); the mask and its tables stay in L2.
// Entry point defined here: lp_audio_merge.
#include "lp_common.h"

namespace lp {
namespace {

constexpr int kPlanThreads = 1024;   // the plan is one workgroup: mask-sized work, one launch, an LDS scan of 1024 partials
constexpr int kMergeBlock = 256;
constexpr int kVec = 4;              // samples per lane: one float4 per row operand

// source index of sample i: identity for a per-sample mask (the reference takes it as given), else ATen's nearest-exact rule
__device__ __forceinline__ int src_of(int64_t i, int fm, int n, int rule) {
    return fm == n ? static_cast<int>(i) : nearest_exact_index(static_cast<int>(i), fm, n, rule);
}

// start[s] = min { i in [0, n] : src(i) >= s }.  src() is monotone (every rule is a chain of monotone roundings), so a
// closed-form estimate fixed up by a short monotone walk lands on it; the walk is a step or two, longer only at sizes where
// float(i) itself is inexact, and always ends inside [0, n].
__device__ __forceinline__ int64_t seg_start(int s, int fm, int n, int rule) {
    if (s <= 0) return 0;
    if (s >= fm) return n;
    if (fm == n) return s;
    double est = ceil(static_cast<double>(s) * static_cast<double>(n) / static_cast<double>(fm) - 0.5);
    int64_t i = est < 0.0 ? 0 : (est > static_cast<double>(n) ? n : static_cast<int64_t>(est));
    while (i > 0 && src_of(i - 1, fm, n, rule) >= s) --i;
    while (i < n && src_of(i, fm, n, rule) < s) ++i;
    return i;
}

__global__ __launch_bounds__(kPlanThreads) void lp_audio_plan_kernel(const float* __restrict__ mask, int fm, int n, int rule,
                                                                     double* __restrict__ P, int32_t* __restrict__ start) {
#pragma clang fp contract(off)
    __shared__ double part[2][kPlanThreads];
    const int t = threadIdx.x;
    const int chunk = (fm + kPlanThreads - 1) / kPlanThreads;
    const int s0 = min(fm, t * chunk), s1 = min(fm, s0 + chunk);
    double sum = 0.0;
    int64_t st = seg_start(s0, fm, n, rule);
    for (int s = s0; s < s1; ++s) {
        const int64_t en = seg_start(s + 1, fm, n, rule);
        start[s] = static_cast<int32_t>(st);
        sum += static_cast<double>(mask[s]) * static_cast<double>(en - st);
        st = en;
    }
    // inclusive Hillis-Steele scan of the 1024 chunk sums, double-buffered in LDS
    int cur = 0;
    part[cur][t] = sum;
    __syncthreads();
    for (int off = 1; off < kPlanThreads; off <<= 1) {
        const double v = part[cur][t] + (t >= off ? part[cur][t - off] : 0.0);
        part[cur ^ 1][t] = v;
        cur ^= 1;
        __syncthreads();
    }
    double run = t > 0 ? part[cur][t - 1] : 0.0;    // exclusive prefix: what the chunks before this one hold
    st = seg_start(s0, fm, n, rule);
    for (int s = s0; s < s1; ++s) {
        const int64_t en = seg_start(s + 1, fm, n, rule);
        P[s] = run;
        run += static_cast<double>(mask[s]) * static_cast<double>(en - st);
        st = en;
    }
    if (s0 < s1 && s1 == fm) {                   // the one thread that owns the last segment closes both tables
        P[fm] = run;
        start[fm] = n;
    }
}

struct MergeArgs {
    const float* mask;
    const float* orig;
    const float* inp;
    float* out;
    const double* P;
    const int32_t* start;
    int64_t osb, osc, psb, psc;
    int n, fm, cf, rule, batch, channels;
};

// C(j) = sum of w[0 .. j), j in [0, n]
__device__ __forceinline__ double prefix_w(const MergeArgs& a, int64_t j) {
#pragma clang fp contract(off)
    if (j >= a.n) return a.P[a.fm];
    const int s = src_of(j, a.fm, a.n, a.rule);
    return a.P[s] + static_cast<double>(a.mask[s]) * static_cast<double>(j - a.start[s]);
}

__device__ __forceinline__ float weight_at(const MergeArgs& a, int64_t i, float w_first, float w_last, double inv_cf) {
#pragma clang fp contract(off)
    if (a.cf <= 1) return a.mask[src_of(i, a.fm, a.n, a.rule)];
    const int64_t lo_raw = i - a.cf / 2;                       // window [lo_raw, lo_raw + cf) before the replicate clamp
    const int64_t hi_raw = lo_raw + a.cf;
    const int64_t lo = lo_raw < 0 ? 0 : lo_raw;
    const int64_t hi = hi_raw > a.n ? a.n : hi_raw;              // lo < hi always: lo_raw <= i < hi_raw
    const double ends = static_cast<double>(lo - lo_raw) * w_first + static_cast<double>(hi_raw - hi) * w_last;
    const double s = ends + (prefix_w(a, hi) - prefix_w(a, lo));
    return static_cast<float>(s * inv_cf);
}

template <bool VEC>
__global__ __launch_bounds__(kMergeBlock) void lp_audio_merge_kernel(MergeArgs a) {
#pragma clang fp contract(off)
    const int64_t i0 = (static_cast<int64_t>(blockIdx.x) * kMergeBlock + threadIdx.x) * kVec;
    if (i0 >= a.n) return;
    const float w_first = a.mask[src_of(0, a.fm, a.n, a.rule)];
    const float w_last = a.mask[src_of(a.n - 1, a.fm, a.n, a.rule)];
    const double inv_cf = static_cast<double>(1.0f / static_cast<float>(a.cf > 1 ? a.cf : 1));
    float w[kVec], omw[kVec];
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        w[k] = (i0 + k < a.n) ? weight_at(a, i0 + k, w_first, w_last, inv_cf) : 0.0f;
        omw[k] = 1.0f - w[k];
    }
    for (int b = 0; b < a.batch; ++b) {
        for (int c = 0; c < a.channels; ++c) {
            const float* o = a.orig + b * a.osb + c * a.osc;
            const float* p = a.inp + b * a.psb + c * a.psc;
            float* y = a.out + (static_cast<int64_t>(b) * a.channels + c) * a.n;
            if constexpr (VEC) {                                  // n % 4 == 0, every row base 16 B aligned
                const float4 ov = *reinterpret_cast<const float4*>(o + i0);
                const float4 pv = *reinterpret_cast<const float4*>(p + i0);
                float4 r;
                r.x = ov.x * omw[0] + pv.x * w[0];
                r.y = ov.y * omw[1] + pv.y * w[1];
                r.z = ov.z * omw[2] + pv.z * w[2];
                r.w = ov.w * omw[3] + pv.w * w[3];
                *reinterpret_cast<float4*>(y + i0) = r;
            } else {
#pragma unroll
                for (int k = 0; k < kVec; ++k) {
                    if (i0 + k < a.n) y[i0 + k] = o[i0 + k] * omw[k] + p[i0 + k] * w[k];
                }
            }
        }
    }
}


}  // namespace

extern "C" int lp_audio_merge(const lp_audio_desc* dp, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!dp) return LP_E_INVALID;
    const lp_audio_desc& d = *dp;
    if (d.n < 1 || d.mask_len < 1 || d.mask_len == INT32_MAX || d.batch < 1 || d.channels < 1 || d.cf < 0) return LP_E_INVALID;
    if (d.nn_rule < LP_NN_ATEN_SCALAR || d.nn_rule > LP_NN_ATEN_CPU_GENERIC) return LP_E_INVALID;
    if (d.orig_sb < 0 || d.orig_sc < 0 || d.inp_sb < 0 || d.inp_sc < 0) return LP_E_INVALID;
    if (!d.mask || !d.orig || !d.inpainted || !d.out) return LP_E_INVALID;
    if (d.cf > 1 && (!d.workspace || (reinterpret_cast<uintptr_t>(d.workspace) & 7u))) return LP_E_INVALID;
    if (static_cast<int64_t>(d.batch) * d.channels > INT32_MAX) return LP_E_UNSUPPORTED;

    MergeArgs a{};
    a.mask = d.mask;
    a.orig = d.orig;
    a.inp = d.inpainted;
    a.out = d.out;
    a.osb = d.orig_sb; a.osc = d.orig_sc; a.psb = d.inp_sb; a.psc = d.inp_sc;
    a.n = d.n; a.fm = d.mask_len; a.cf = d.cf; a.rule = d.nn_rule; a.batch = d.batch; a.channels = d.channels;
    if (d.cf > 1) {
        double* P = static_cast<double*>(d.workspace);
        int32_t* start = reinterpret_cast<int32_t*>(P + (static_cast<int64_t>(d.mask_len) + 1));
        a.P = P;
        a.start = start;
        hipLaunchKernelGGL(lp_audio_plan_kernel, dim3(1), dim3(kPlanThreads), 0, stream, d.mask, d.mask_len, d.n, d.nn_rule,
                           P, start);
        if (hipGetLastError() != hipSuccess) return LP_E_LAUNCH;
    }
    const bool vec = (d.n % kVec == 0) && aligned16(d.orig) && aligned16(d.inpainted) && aligned16(d.out) &&
                     d.orig_sb % kVec == 0 && d.orig_sc % kVec == 0 && d.inp_sb % kVec == 0 && d.inp_sc % kVec == 0;
    const int64_t lanes = (static_cast<int64_t>(d.n) + kVec - 1) / kVec;
    const dim3 grid(static_cast<uint32_t>((lanes + kMergeBlock - 1) / kMergeBlock));
    if (vec) hipLaunchKernelGGL(lp_audio_merge_kernel<true>, grid, dim3(kMergeBlock), 0, stream, a);
    else hipLaunchKernelGGL(lp_audio_merge_kernel<false>, grid, dim3(kMergeBlock), 0, stream, a);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

}  // namespace lp
