// label_kernel.hip -- connected components of a mask on the device for gfx950 (lp_mask_components): the Detailer's split of a
// mask into regions (lanpaint_amd/detail.py plans them on the host from the table this writes).
//
//   S = { (y, x) : mask[p, y, x] > 0.5 for some plane p },  8-connected components, label = 1 + rank of the component's
//   smallest flat index y * W + x  (scipy.ndimage.label(S, ones((3, 3)))), plus per component (r0, r1, c0, c1, area).
//
// Union-find over a parent array P [H * W] int32 in the workspace: P[i] = -1 is background, otherwise the flat index of
// another pixel of i's component that is <= i.  Every union is an integer atomicMin onto a root, so parents only ever
// decrease and a component's root ends as its smallest flat index -- whatever the order of arrival.  Seven plain launches on
// the caller's stream, each finished before the next begins; no block reads a value it needs another block of the SAME
// launch to have written first (concurrent unions read parents others are lowering, but any value read is a valid ancestor):
//
//   1 union      every plane once, 16 B per lane: P[i] = i where some plane is set, -1 elsewhere
//   2 tile       a 16 x 64 tile's unions in LDS, then P[i] = the tile-local root (parents one step deep inside a tile)
//   3 border     unions across tile edges, in global memory
//   4 flatten    P[i] = root(i);  roots (P[i] == i) counted per 1024-element chunk
//   5 scan       exclusive prefix sum of the chunk counts (one block), table[0] = n, table rows reset
//   6 rank       per chunk: exclusive scan of its root flags; a root's rank r goes back into P as -(r + 1) <= -2
//   7 relabel    labels[i] from P (read-only here), boxes and areas by integer atomicMin / atomicMax / atomicAdd
//
// The prefix sum is reduce (4) / scan of sums (5) / apply (6) in separate launches: no look-back, no block waits for another.
//
// In space and time (lp_mask_components_frames): S = { (f, y, x) : mask[f, y, x] > 0.5 }, no union over planes, 26-connected
// components, label = 1 + rank of the smallest flat index (f * H + y) * W + x  (scipy.ndimage.label(S, ones((3, 3, 3)))), plus
// per component (f0, f1, r0, r1, c0, c1, volume).  P is [F * H * W]; the same launches on the volume and one more:
//
//   1 union      one voxel per element (planes = 1, n = F * H * W)
//   2 tile       per frame, the frame on blockIdx.z; a frame's flat indices are a contiguous range, so tile-local order still
//                ascends with the flat index
//   3 border     per frame
//   3t temporal  a set voxel of frame f >= 1 unites with frame f - 1: with (f - 1, y, x) when that is set -- every other set
//                voxel of the 3 x 3 neighbourhood there is 8-adjacent to it and so already in its component after 2 and 3 --
//                otherwise with each set voxel among the other eight, which need not be adjacent to each other.  16 B per
//                lane where W % 4 == 0
//   4 .. 7       over n = F * H * W; 7 derives (f, y, x) from the flat index and sends seven integer atomics
//
// The temporal launch needs no value another block of it must write first, by the argument of launch 3: whether a voxel is set
// (P >= 0) was settled by launch 1 and no union changes it, so which unions a thread makes does not depend on the others;
// `unite` reads parents that others are lowering, every value read is a valid ancestor of the same component (parents only
// decrease, by atomicMin onto a root), and each union ends with both voxels under one root whatever happened meanwhile.  When
// the launch has finished every 26-adjacent pair has been united once, so a component's root is its smallest flat index.
// Entry points defined here: lp_mask_components, lp_mask_components_frames.
#include "lp_common.h"

namespace lp {
namespace {

constexpr int kTileH = 16, kTileW = 64;      // LDS tile of launch 2: 1024 pixels, 4 per thread, rows of 256 B
constexpr int kChunk = 1024;                 // elements per block of launches 4, 6, 7: 4 per thread

// ---- union-find ---------------------------------------------------------------------------------------------------------
// The only data-dependent loops of this file are these two.  `find` walks parent pointers: L[a] < a at every step that is not
// a root, so the value strictly decreases and the walk ends within `a` steps whatever other threads do meanwhile (they only
// lower parents).  `unite` retries only when its atomicMin met a parent that somebody else had lowered in between (old != the
// root it aimed at); the retry continues from that lower value, so the pair (a, b) strictly decreases from one round to the
// next and the loop ends.  Nobody waits: every round does work of its own.
template <class T>
__device__ __forceinline__ int find(const T* L, int a) {
    int p = L[a];
    while (p != a) { a = p; p = L[a]; }     // strictly decreasing, ends at a root
    return a;
}

template <class T>
__device__ __forceinline__ void unite(T* L, int a, int b) {
    bool done = false;
    while (!done) {                          // (a, b) strictly decreases per round, see above
        a = find(L, a);
        b = find(L, b);
        if (a == b) {
            done = true;
        } else {
            const int hi = max(a, b), lo = min(a, b);
            const int old = atomicMin(const_cast<int*>(L) + hi, lo);
            done = old == hi;                // hi was still a root: linked.  Otherwise go on from what it had become
            a = old; b = lo;
        }
    }
}

// ---- 1: thresholded union over planes --------------------------------------------------------------------------------------
// Thread t owns elements V * t .. V * t + V - 1 of the flat plane (V = 4: n % 4 == 0 and a 16 B aligned mask, one 16 B load per
// plane and one 16 B store).
template <int V>
__global__ __launch_bounds__(256) void lp_label_union_kernel(const float* __restrict__ mask, int32_t* __restrict__ P, int planes,
                                                             int n) {
    const int i = (blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= n) return;
    bool s0 = false, s1 = false, s2 = false, s3 = false;
    const float* p = mask + i;
#pragma unroll 8
    for (int f = 0; f < planes; ++f, p += n) {
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(p);
            s0 |= q.x > 0.5f; s1 |= q.y > 0.5f; s2 |= q.z > 0.5f; s3 |= q.w > 0.5f;
        } else {
            s0 |= p[0] > 0.5f;
        }
    }
    if constexpr (V == 4)
        *reinterpret_cast<int4*>(P + i) = make_int4(s0 ? i : -1, s1 ? i + 1 : -1, s2 ? i + 2 : -1, s3 ? i + 3 : -1);
    else
        P[i] = s0 ? i : -1;
}

// ---- 2: unions inside a tile, in LDS -----------------------------------------------------------------------------------------
// Local index q = ty * 64 + tx ascends with the flat index y * W + x inside a tile, so the tile-local root (smallest q) is the
// tile-local smallest flat index.  A pixel unites with its W, NW, N and NE neighbours: every 8-adjacent pair once.  blockIdx.z
// is the frame of a volume.
__global__ __launch_bounds__(256) void lp_label_tile_kernel(int32_t* __restrict__ P, int H, int W) {
    __shared__ int L[kTileH * kTileW];
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH, tid = threadIdx.x;
    const int base = blockIdx.z * H * W;                          // of the frame; 0 for the single plane
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = tid + 256 * j, ty = q >> 6, tx = q & 63, y = y0 + ty, x = x0 + tx;
        L[q] = (y < H && x < W && P[base + y * W + x] >= 0) ? q : -1;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = tid + 256 * j, ty = q >> 6, tx = q & 63;
        if (L[q] < 0) continue;
        if (tx > 0 && L[q - 1] >= 0) unite(L, q, q - 1);
        if (ty > 0) {
            if (tx > 0 && L[q - kTileW - 1] >= 0) unite(L, q, q - kTileW - 1);
            if (L[q - kTileW] >= 0) unite(L, q, q - kTileW);
            if (tx < kTileW - 1 && L[q - kTileW + 1] >= 0) unite(L, q, q - kTileW + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = tid + 256 * j, ty = q >> 6, tx = q & 63;
        if (L[q] < 0) continue;
        const int r = find(L, q);
        P[base + (y0 + ty) * W + x0 + tx] = base + (y0 + (r >> 6)) * W + x0 + (r & 63);
    }
}

// ---- 3: unions across tile edges ------------------------------------------------------------------------------------------
// One thread per pixel; only pixels of a tile's top row, left column or right column have a W / NW / N / NE neighbour in
// another tile.
__global__ __launch_bounds__(256) void lp_label_border_kernel(int32_t* __restrict__ P, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int tx = x & (kTileW - 1), ty = y & (kTileH - 1);
    const bool top = ty == 0 && y > 0, left = tx == 0 && x > 0, right = tx == kTileW - 1 && x + 1 < W && y > 0;
    if (!(top || left || right)) return;
    const int i = blockIdx.z * H * W + y * W + x;                 // blockIdx.z: the frame of a volume
    if (P[i] < 0) return;
    if (left && P[i - 1] >= 0) unite(P, i, i - 1);
    if (y > 0) {
        if ((top || left) && x > 0 && P[i - W - 1] >= 0) unite(P, i, i - W - 1);
        if (top && P[i - W] >= 0) unite(P, i, i - W);
        if ((top || right) && x + 1 < W && P[i - W + 1] >= 0) unite(P, i, i - W + 1);
    }
}

// ---- 3t: unions between a frame and the one before it --------------------------------------------------------------------
// Thread t owns voxels V * t .. V * t + V - 1 of frames 1 .. F - 1 (V = 4: W % 4 == 0, so the four share a row and both 16 B
// loads, the voxels' parents and those straight below, are aligned; the file's header has the rule and why the launch needs
// no order).  Only whether a loaded parent is >= 0 is used, and no union changes that.
template <int V>
__global__ __launch_bounds__(256) void lp_label_temporal_kernel(int32_t* __restrict__ P, int H, int W, int n) {
    const int plane = H * W, i0 = plane + (blockIdx.x * 256 + threadIdx.x) * V;
    if (i0 >= n) return;
    int own[V], under[V];
    if constexpr (V == 4) {
        const int4 a = *reinterpret_cast<const int4*>(P + i0), b = *reinterpret_cast<const int4*>(P + i0 - plane);
        own[0] = a.x; own[1] = a.y; own[2] = a.z; own[3] = a.w;
        under[0] = b.x; under[1] = b.y; under[2] = b.z; under[3] = b.w;
    } else {
        own[0] = P[i0];
        under[0] = P[i0 - plane];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
        if (own[e] < 0) continue;
        const int i = i0 + e, below = i - plane;
        if (under[e] >= 0) {
            unite(P, i, below);
            continue;
        }
        const int yx = i % plane, y = yx / W, x = yx - y * W;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if ((dy == 0 && dx == 0) || y + dy < 0 || y + dy >= H || x + dx < 0 || x + dx >= W) continue;
                const int j = below + dy * W + dx;
                if (P[j] >= 0) unite(P, i, j);
            }
        }
    }
}

// ---- 4: flatten, count roots per chunk -----------------------------------------------------------------------------------
// Roots stay roots in this launch (P[r] == r is never written), so the count does not depend on the order of arrival; a walk
// that passes through an element another thread is flattening reads its old parent or its root, both ancestors.
__global__ __launch_bounds__(256) void lp_label_flatten_kernel(int32_t* __restrict__ P, int32_t* __restrict__ sums, int n) {
    __shared__ int part[4];
    const int base = blockIdx.x * kChunk, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    int roots = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = base + threadIdx.x + 256 * j;
        bool root = false;
        if (i < n && P[i] >= 0) {
            const int r = find(P, i);
            root = r == i;
            if (!root) P[i] = r;
        }
        roots += __popcll(__ballot(root));
    }
    if (lane == 0) part[wave] = roots;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// Exclusive scan over the block's 256 threads; `total` gets the block's sum.
__device__ __forceinline__ int block_exclusive_scan(int v, int* part, int& total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int o = __shfl_up(inc, off, kWave);
        if (lane >= off) inc += o;
    }
    if (lane == kWave - 1) part[wave] = inc;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) before += (w < wave) ? part[w] : 0;
    total = part[0] + part[1] + part[2] + part[3];
    __syncthreads();                                            // part is reused by the caller's next round
    return before + inc - v;
}

// ---- 5: scan of the chunk counts (one block), table header and reset ---------------------------------------------------------
// VOLUME: rows of seven, {F, -1, H, -1, W, -1, 0}.
template <bool VOLUME>
__global__ __launch_bounds__(256) void lp_label_scan_kernel(int32_t* __restrict__ sums, int chunks, int32_t* __restrict__ table,
                                                            int F, int H, int W) {
    __shared__ int part[4];
    int carry = 0;
    for (int c0 = 0; c0 < chunks; c0 += 256) {
        const int c = c0 + threadIdx.x;
        const int v = c < chunks ? sums[c] : 0;
        int total;
        const int ex = block_exclusive_scan(v, part, total);
        if (c < chunks) sums[c] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) table[0] = carry;
    for (int id = threadIdx.x; id < LP_DETAIL_MAX_COMPONENTS; id += 256) {
        int32_t* row = table + 1 + (VOLUME ? 7 : 5) * id;
        if constexpr (VOLUME) { row[0] = F; row[1] = -1; row += 2; }
        row[0] = H; row[1] = -1; row[2] = W; row[3] = -1; row[4] = 0;
    }
}

// ---- 6: rank the roots -------------------------------------------------------------------------------------------------------
// Thread t owns elements 4t .. 4t + 3 of the chunk, so ranks ascend with the flat index.  Root i of rank r (0-based):
// P[i] = -(r + 2), i.e. label r + 1 coded as -(label + 1): below the background's -1, and nothing else in P is.
__global__ __launch_bounds__(256) void lp_label_rank_kernel(int32_t* __restrict__ P, const int32_t* __restrict__ sums, int n) {
    __shared__ int part[4];
    const int i0 = blockIdx.x * kChunk + threadIdx.x * 4;
    bool root[4];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        root[j] = i0 + j < n && P[i0 + j] == i0 + j;
        mine += root[j] ? 1 : 0;
    }
    int total;
    int rank = sums[blockIdx.x] + block_exclusive_scan(mine, part, total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (root[j]) {
            P[i0 + j] = -(rank + 2);
            ++rank;
        }
    }
}

// ---- 7: relabel, boxes and areas ---------------------------------------------------------------------------------------------
// A wave holds 64 consecutive flat indices.  When all its set lanes carry one label (the usual case inside a blob) the wave
// reduces its box and count by shuffles and one lane sends the five atomics; otherwise each lane sends its own.  Integer
// atomics: the table does not depend on the order of arrival.  Labels past the cap leave the table alone.  VOLUME: (f, y, x)
// from the flat index and seven atomics, the frame bounds first.
template <bool VOLUME>
__global__ __launch_bounds__(256) void lp_label_relabel_kernel(const int32_t* __restrict__ P, int32_t* __restrict__ labels,
                                                               int32_t* __restrict__ table, int n, int H, int W) {
    constexpr int kRow = VOLUME ? 7 : 5;
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = blockIdx.x * kChunk + threadIdx.x + 256 * j;
        int label = 0;
        if (i < n) {
            int v = P[i];
            if (v >= 0) v = P[v];                                   // a flattened element points at its root
            label = v < -1 ? -(v + 1) : 0;
            labels[i] = label;
        }
        const unsigned long long set = __ballot(label != 0);
        if (set == 0) continue;                                     // wave-uniform
        const int first = __shfl(label, __builtin_ctzll(set), kWave);
        const bool uniform = __ballot(label != 0 && label != first) == 0;
        const int row_of = i / W, x = i - row_of * W;               // row_of = f * H + y
        const int f = VOLUME ? row_of / H : 0, y = row_of - f * H;
        if (uniform) {
            int f0 = label ? f : INT32_MAX, f1 = label ? f : -1;
            int r0 = label ? y : INT32_MAX, r1 = label ? y : -1, c0 = label ? x : INT32_MAX, c1 = label ? x : -1;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                if constexpr (VOLUME) { f0 = min(f0, __shfl_xor(f0, off, kWave)); f1 = max(f1, __shfl_xor(f1, off, kWave)); }
                r0 = min(r0, __shfl_xor(r0, off, kWave)); r1 = max(r1, __shfl_xor(r1, off, kWave));
                c0 = min(c0, __shfl_xor(c0, off, kWave)); c1 = max(c1, __shfl_xor(c1, off, kWave));
            }
            if (lane == 0 && first <= LP_DETAIL_MAX_COMPONENTS) {
                int32_t* row = table + 1 + kRow * (first - 1);
                if constexpr (VOLUME) { atomicMin(row + 0, f0); atomicMax(row + 1, f1); row += 2; }
                atomicMin(row + 0, r0); atomicMax(row + 1, r1); atomicMin(row + 2, c0); atomicMax(row + 3, c1);
                atomicAdd(row + 4, __popcll(set));
            }
        } else if (label != 0 && label <= LP_DETAIL_MAX_COMPONENTS) {
            int32_t* row = table + 1 + kRow * (label - 1);
            if constexpr (VOLUME) { atomicMin(row + 0, f); atomicMax(row + 1, f); row += 2; }
            atomicMin(row + 0, y); atomicMax(row + 1, y); atomicMin(row + 2, x); atomicMax(row + 3, x);
            atomicAdd(row + 4, 1);
        }
    }
}

bool side_ok(int s) { return s > 0 && s <= LP_DETAIL_MAX_SIDE; }

// The launches after the threshold, shared by the plane and the volume: F frames of H x W in P, n = F * H * W.
template <bool VOLUME>
int launch_label(int F, int H, int W, int32_t* P, int32_t* sums, int32_t* labels, int32_t* table, hipStream_t stream) {
    const int n = F * H * W, chunks = (n + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(lp_label_tile_kernel, dim3((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH, F), dim3(256), 0, stream,
                       P, H, W);
    hipLaunchKernelGGL(lp_label_border_kernel, dim3((W + 255) / 256, H, F), dim3(256), 0, stream, P, H, W);
    if (VOLUME && F > 1) {
        const int rest = n - H * W;                                // P is 16 B aligned (the workspace is)
        if ((W & 3) == 0)
            hipLaunchKernelGGL(lp_label_temporal_kernel<4>, dim3((rest / 4 + 255) / 256), dim3(256), 0, stream, P, H, W, n);
        else
            hipLaunchKernelGGL(lp_label_temporal_kernel<1>, dim3((rest + 255) / 256), dim3(256), 0, stream, P, H, W, n);
    }
    hipLaunchKernelGGL(lp_label_flatten_kernel, dim3(chunks), dim3(256), 0, stream, P, sums, n);
    hipLaunchKernelGGL(lp_label_scan_kernel<VOLUME>, dim3(1), dim3(256), 0, stream, sums, chunks, table, F, H, W);
    hipLaunchKernelGGL(lp_label_rank_kernel, dim3(chunks), dim3(256), 0, stream, P, sums, n);
    hipLaunchKernelGGL(lp_label_relabel_kernel<VOLUME>, dim3(chunks), dim3(256), 0, stream, P, labels, table, n, H, W);
    return hipGetLastError() == hipSuccess ? LP_OK : LP_E_LAUNCH;
}

// Launch 1 over `planes` planes of n elements each.
bool launch_union(const float* mask, int32_t* P, int planes, int n, hipStream_t stream) {
    if ((n & 3) == 0 && aligned16(mask))
        hipLaunchKernelGGL(lp_label_union_kernel<4>, dim3((n / 4 + 255) / 256), dim3(256), 0, stream, mask, P, planes, n);
    else
        hipLaunchKernelGGL(lp_label_union_kernel<1>, dim3((n + 255) / 256), dim3(256), 0, stream, mask, P, planes, n);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

extern "C" int lp_mask_components(const float* mask, int32_t planes, int32_t H, int32_t W, int32_t* labels, int32_t* table,
                                  void* workspace, int64_t workspace_bytes, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!mask || !labels || !table || !workspace || planes <= 0 || !side_ok(H) || !side_ok(W)) return LP_E_INVALID;
    if (workspace_bytes < LP_COMPONENTS_WS_BYTES(H, W)) return LP_E_INVALID;
    if (!aligned16(workspace)) return LP_E_ALIGN;
    if (planes > 65535) return LP_E_UNSUPPORTED;
    const int n = H * W;                                            // <= 2^30 by the side limit: flat indices are int32
    const int chunks = (n + kChunk - 1) / kChunk;
    int32_t* P = static_cast<int32_t*>(workspace);                  // chunks * 1024 elements, then the chunk counts
    int32_t* sums = P + static_cast<int64_t>(chunks) * kChunk;
    if (!launch_union(mask, P, planes, n, stream)) return LP_E_LAUNCH;
    return launch_label<false>(1, H, W, P, sums, labels, table, stream);
}

extern "C" int lp_mask_components_frames(const float* mask, int32_t F, int32_t H, int32_t W, int32_t* labels, int32_t* table,
                                         void* workspace, int64_t workspace_bytes, void* stream_) {
    const hipStream_t stream = as_stream(stream_);
    if (!mask || !labels || !table || !workspace || F <= 0 || !side_ok(H) || !side_ok(W)) return LP_E_INVALID;
    if (workspace_bytes < LP_COMPONENTS_FRAMES_WS_BYTES(F, H, W)) return LP_E_INVALID;
    if (!aligned16(workspace)) return LP_E_ALIGN;
    if (F > 65535 || static_cast<int64_t>(F) * H * W > (1ll << 30)) return LP_E_UNSUPPORTED;   // the grid's z; int32 parents
    const int n = F * H * W;
    const int chunks = (n + kChunk - 1) / kChunk;
    int32_t* P = static_cast<int32_t*>(workspace);
    int32_t* sums = P + static_cast<int64_t>(chunks) * kChunk;
    if (!launch_union(mask, P, 1, n, stream)) return LP_E_LAUNCH;   // one voxel per element: no union over planes
    return launch_label<true>(F, H, W, P, sums, labels, table, stream);
}

}  // namespace lp
